"""What the profile entry points of the TEST build promise (include/prt_hip_test.h, the tools under tools/*_bench.py), on the MI355X:
each leaves the context in the state of the plain call its comment names, byte for byte, and fills every slot of its `ms` array as
documented; and the timing ring of the product library folds its oldest launches when a caller renders more than PRT_TIMING_RING
times without reading the statistics.  Context A runs the profile call, context B the plain call.  What the calls must not LEAK on
their error paths is not observable from here: tests/test_devres_cpu.py holds that part."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_gpukit import upload
from prt_refit_ref import bend, teapot_scene

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL = -2
ARRAYS = ("wnodes", "hot", "tris", "shade", "bump", "root_boxes", "radius")
SHADING = ("mats", "alpha_class", "texels", "env_texels", "env_vertical", "env_horizontal", "env_first_x", "env_first_y", "has_light",
           "has_env", "light_dir", "light_intensity")
ENV = ("env_texels", "env_vertical", "env_horizontal", "env_first_x", "env_first_y", "has_env")


@pytest.fixture(scope="module")
def A():
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=True)
    yield t
    t.close()


@pytest.fixture(scope="module")
def B():
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=True)
    yield t
    t.close()


def same(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs"


def times(ms, n, what, positive=False):
    v = np.array(ms[:n], dtype=np.float64)
    print(what, v)
    assert np.isfinite(v).all() and ((v > 0) if positive else (v >= 0)).all(), (what, v)


def framebuffer(t):
    return t._download_rect(0, 0, t._camera.width - 1, t._camera.height - 1, stats=False)


def mesh_updates(scene, ids):
    """The array PathTracer.update_meshes hands to prt_hip_update_meshes."""
    d = scene.describe().contents
    ups = (prt_amd.MeshUpdate * len(ids))()
    for k, m in enumerate(ids):
        md = d.meshes[m]
        ups[k].mesh, ups[k].vertexCount, ups[k].positions, ups[k].normals, ups[k].radius = m, md.vertexCount, md.positions, md.normals, d.radius
    return ups


def texture_updates(scene, textures):
    d = scene.describe().contents
    ups = (prt_amd.TextureUpdate * len(textures))()
    for k, t in enumerate(textures):
        td = d.textures[t]
        ups[k].texture, ups[k].width, ups[k].height, ups[k].component, ups[k].texels = t, td.width, td.height, td.component, td.texels
    return ups


# ----------------------------------------------------------------------------- geometry
def test_refit_profile_ends_in_one_update(A, B):
    scene, camera, _ = teapot_scene()
    for t in (A, B):
        upload(t, scene, camera)
    before = A.scene_arrays()
    tea = scene.arrays()["meshes"][1]
    scene.update_positions(1, bend(tea["positions"]), tea["normals"])
    ms = (C.c_float * 2)(-1.0, -1.0)
    A._chk(A._L.prt_hip_test_refit_profile(A._ctx, 1, mesh_updates(scene, [1]), 3, ms), "prt_hip_test_refit_profile")
    B.update_meshes(scene, [1])
    got = A.scene_arrays()
    same(got, B.scene_arrays(), ARRAYS, "refit profile against one update_meshes")
    assert got["tris"].tobytes() != before["tris"].tobytes() and got["wnodes"].tobytes() != before["wnodes"].tobytes()
    times(ms, 2, "refit profile ms")


def test_deform_profile_ends_in_one_deform(A, B):
    scene, camera, _ = teapot_scene()
    for t in (A, B):
        upload(t, scene, camera)
    before = A.scene_arrays()
    P = bend(scene.arrays()["meshes"][1]["positions"])
    ups, keep = A._deforms([(1, P, prt_amd.MeshDeform.NORMALS_RECOMPUTE)], True)
    ms = (C.c_float * 5)(*([-1.0] * 5))
    A._chk(A._L.prt_hip_test_deform_profile(A._ctx, 1, ups, prt_amd.MeshDeform.HOST | prt_amd.MeshDeform.RADIUS_AUTO, 3, ms), "prt_hip_test_deform_profile")
    B.deform_meshes([(1, P, prt_amd.MeshDeform.NORMALS_RECOMPUTE)], host=True, radius_auto=True)
    got = A.scene_arrays()
    same(got, B.scene_arrays(), ARRAYS, "deform profile against one deform_meshes")
    assert got["tris"].tobytes() != before["tris"].tobytes() and got["shade"].tobytes() != before["shade"].tobytes()
    (pa, na), (pb, nb) = A.mesh_vertices(1), B.mesh_vertices(1)
    assert pa.tobytes() == pb.tobytes() == P.tobytes() and na.tobytes() == nb.tobytes()
    ia, ib = A.mesh_info(1), B.mesh_info(1)
    assert ia.keys() == ib.keys()
    for k in ia:
        assert np.asarray(ia[k]).tobytes() == np.asarray(ib[k]).tobytes(), k
    times(ms, 5, "deform profile ms")


# ----------------------------------------------------------------------------- the preview filters
def accumulated(t, scene, camera):
    """The smallest accumulation the library takes: one pass of 8 samples per pixel."""
    upload(t, scene, camera)
    t.accum_reset()
    t.accumulate(8)


def test_denoise_profile_ends_in_one_denoise(A, B):
    scene, camera, _ = teapot_scene(32)
    for t in (A, B):
        accumulated(t, scene, camera)
    p = A.denoise_params(iterations=3)
    ms = (C.c_float * 7)(*([-1.0] * 7))
    A._chk(A._L.prt_hip_test_denoise_profile(A._ctx, C.byref(p), 1.0, ms), "prt_hip_test_denoise_profile")
    want = B.denoise(iterations=3)
    assert framebuffer(A).tobytes() == want.tobytes()
    assert A.denoise_variance().tobytes() == B.denoise_variance().tobytes()
    assert np.isfinite(want).all() and want.any()
    times(ms, 7, "denoise profile ms")
    assert ms[4] == 0.0 and ms[5] == 0.0 and ms[6] > 0.0, list(ms)


def test_temporal_profile_ends_in_one_temporal_denoise(A, B):
    scene, camera, _ = teapot_scene(32)
    for t in (A, B):
        accumulated(t, scene, camera)
        t.history_reset()
        t.denoise_temporal(iterations=3)  # the pending record of this view ...
        t.set_camera(camera)              # ... becomes the history
        t.accumulate(8)
        assert t.history_export(0)["color_var"].any()
    p, tp = A.denoise_params(iterations=3), A.temporal_params()
    ms = (C.c_float * 4)(*([-1.0] * 4))
    A._chk(A._L.prt_hip_test_temporal_profile(A._ctx, C.byref(p), C.byref(tp), 1.0, ms), "prt_hip_test_temporal_profile")
    want = B.denoise_temporal(iterations=3)
    assert framebuffer(A).tobytes() == want.tobytes()
    ra, rb = A.history_export(1), B.history_export(1)
    same(ra, rb, ("color_var", "pos_len", "normal"), "pending record")
    assert bytes(ra["camera"]) == bytes(rb["camera"])
    assert (rb["pos_len"][..., 3] > 8).any()  # the history was taken
    times(ms, 4, "temporal profile ms")


# ----------------------------------------------------------------------------- display
def test_display_profile_ends_in_one_display(A, B):
    scene, camera, _ = teapot_scene(32)
    rng = np.random.default_rng(3)
    img = (rng.uniform(0.0, 4.0, (32, 32, 3)) ** 2).astype(F)
    for t in (A, B):
        upload(t, scene, camera)
        t.upload_image(img)
        t.display_reset()
    p = prt_amd.DisplayParams.make(meter=True)
    assert p.adaptRate == 1.0
    ms = (C.c_float * 3)(-1.0, -1.0, -1.0)
    A._chk(A._L.prt_hip_test_display_profile(A._ctx, C.byref(p), 2, ms), "prt_hip_test_display_profile")
    want = B.display(p)
    got = np.zeros((32, 32, p.bpp), dtype=np.uint8)
    A._chk(A._L.prt_hip_download_display(A._ctx, got.ctypes.data_as(C.c_void_p), 0, 0, 31, 31), "prt_hip_download_display")
    assert got.tobytes() == want.tobytes() and len(np.unique(want)) > 16
    sa, sb = prt_amd.DisplayState(), prt_amd.DisplayState()
    for t, s in ((A, sa), (B, sb)):
        t._chk(t._L.prt_hip_display_get_state(t._ctx, C.byref(s)), "prt_hip_display_get_state")
    assert bytes(sa) == bytes(sb) and sb.valid == 1 and sb.metered + sb.ignored == 32 * 32 and sb.metered > 0
    times(ms, 3, "display profile ms, metered")
    q = prt_amd.DisplayParams.make(meter=False)
    A._chk(A._L.prt_hip_test_display_profile(A._ctx, C.byref(q), 2, ms), "prt_hip_test_display_profile")
    times(ms, 3, "display profile ms, manual gain")
    assert ms[0] == 0.0 and ms[1] == 0.0, list(ms)


# ----------------------------------------------------------------------------- scene edits
def test_edit_profile_ends_in_one_texture_update(A, B):
    scene, camera, _ = prt_amd.setup_atrium_standin(64, 64, tris=2000)
    scene.set_infinite_area_light(T.sky_env(8, 4))
    for t in (A, B):
        upload(t, scene, camera)
    before = A.shading_arrays()
    assert before["env_texels"].shape == (4, 8, 4) and before["has_env"][0] == 1
    leaf = scene.arrays()["textures"][1]
    paint = np.random.default_rng(12).integers(0, 256, leaf.shape, dtype=np.uint8)
    scene.set_texture_texels(1, paint)
    ms = (C.c_float * 2)(-1.0, -1.0)
    A._chk(A._L.prt_hip_test_edit_profile(A._ctx, 1, texture_updates(scene, [1]), 2, ms), "prt_hip_test_edit_profile")
    B.update_textures(scene, [1])
    got = A.shading_arrays()
    same(got, B.shading_arrays(), SHADING, "edit profile against one update_textures")
    same(got, before, ENV, "the environment tables after the edit profile")
    assert got["texels"].tobytes() != before["texels"].tobytes() and got["alpha_class"].tobytes() != before["alpha_class"].tobytes()
    times(ms, 2, "edit profile ms")


def test_copy_yardstick(A):
    ms = C.c_float(-1.0)
    A._chk(A._L.prt_hip_test_copy_yardstick(A._ctx, 1000, 3, 0, 3, 0, C.byref(ms)), "prt_hip_test_copy_yardstick")
    times([ms.value], 1, "copy yardstick ms", positive=True)


# ----------------------------------------------------------------------------- the timing ring
def test_timing_ring_folds_beyond_its_size():
    prt_amd.build()
    t = prt_amd.PathTracer()
    try:
        scene, camera, _ = teapot_scene(16)
        upload(t, scene, camera)
        t.stats()
        for _ in range(40):  # more than PRT_TIMING_RING = 32 launches without a statistics read in between
            t.render_async(0, 0, 15, 15, 1)
        st = t.stats()
        print({k: st[k] for k in ("kernelLaunches", "kernelMs", "kernelMsSum")})
        assert st["kernelLaunches"] == 40
        assert st["kernelMsSum"] >= st["kernelMs"] > 0
        assert t.stats()["kernelLaunches"] == 0
    finally:
        t.close()


# ----------------------------------------------------------------------------- refusals
def test_refused_profile_calls_leave_the_context_usable(A):
    scene, camera, _ = teapot_scene(32)
    accumulated(A, scene, camera)
    L, ctx = A._L, A._ctx
    ups = mesh_updates(scene, [1])
    P = scene.arrays()["meshes"][1]["positions"]
    dups, keep = A._deforms([(1, P, prt_amd.MeshDeform.NORMALS_KEEP)], True)
    flags = prt_amd.MeshDeform.HOST
    p, tp, dp = A.denoise_params(iterations=3), A.temporal_params(), prt_amd.DisplayParams.make()
    ms = (C.c_float * 8)()
    refused = {
        "refit, reps 0": lambda: L.prt_hip_test_refit_profile(ctx, 1, ups, 0, ms),
        "refit, NULL ms": lambda: L.prt_hip_test_refit_profile(ctx, 1, ups, 2, None),
        "deform, reps 0": lambda: L.prt_hip_test_deform_profile(ctx, 1, dups, flags, 0, ms),
        "deform, NULL ms": lambda: L.prt_hip_test_deform_profile(ctx, 1, dups, flags, 2, None),
        "denoise, NULL ms": lambda: L.prt_hip_test_denoise_profile(ctx, C.byref(p), 1.0, None),
        "temporal, NULL ms": lambda: L.prt_hip_test_temporal_profile(ctx, C.byref(p), C.byref(tp), 1.0, None),
        "display, reps 0": lambda: L.prt_hip_test_display_profile(ctx, C.byref(dp), 0, ms),
        "display, NULL ms": lambda: L.prt_hip_test_display_profile(ctx, C.byref(dp), 2, None),
        "edit, reps 0": lambda: L.prt_hip_test_edit_profile(ctx, 0, None, 0, ms),
        "edit, NULL ms": lambda: L.prt_hip_test_edit_profile(ctx, 0, None, 2, None),
        "yardstick, NULL ms": lambda: L.prt_hip_test_copy_yardstick(ctx, 1000, 3, 0, 3, 0, None),
    }
    for what, call in refused.items():
        assert call() == EINVAL, what
        assert L.prt_hip_last_error().decode() == "NULL argument", what
    # the BVH builder, a product entry point: an index past the vertices
    idx = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.uint32)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F)
    nodes, remap, count = np.zeros(4, dtype=prt_amd.NODE_DTYPE), np.zeros(2, dtype=np.uint32), C.c_uint32()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.prt_hip_build_bvh(ctx, 2, vp(idx), 3, vp(pos), vp(nodes), C.byref(count), vp(remap), None) == EINVAL
    assert L.prt_hip_last_error().decode() == "vertex index out of range"
    # and every call works afterwards
    idx[1] = (2, 1, 0)
    got, _, build_ms = A.build_bvh(idx, pos)
    assert len(got) >= 1 and np.isfinite(build_ms) and build_ms >= 0
    A._chk(L.prt_hip_test_refit_profile(ctx, 1, ups, 2, ms), "prt_hip_test_refit_profile")
    A._chk(L.prt_hip_test_deform_profile(ctx, 1, dups, flags, 2, ms), "prt_hip_test_deform_profile")
    A.accumulate(8)  # (the geometry calls emptied the accumulator)
    A._chk(L.prt_hip_test_denoise_profile(ctx, C.byref(p), 1.0, ms), "prt_hip_test_denoise_profile")
    A._chk(L.prt_hip_test_temporal_profile(ctx, C.byref(p), C.byref(tp), 1.0, ms), "prt_hip_test_temporal_profile")
    A._chk(L.prt_hip_test_display_profile(ctx, C.byref(dp), 2, ms), "prt_hip_test_display_profile")
    A._chk(L.prt_hip_test_edit_profile(ctx, 0, None, 2, ms), "prt_hip_test_edit_profile")
    assert ms[0] == 0.0 and ms[1] == 0.0  # no environment map, no texture named
    y = C.c_float()
    A._chk(L.prt_hip_test_copy_yardstick(ctx, 1000, 3, 0, 3, 0, C.byref(y)), "prt_hip_test_copy_yardstick")
    assert np.isfinite(framebuffer(A)).all()
