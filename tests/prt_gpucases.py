"""Helpers that drive a context through cases several GPU test modules share (a library module, no tests of its own): each section
names the module whose tests it was written for.  The fixtures and the small helpers are in prt_gpukit.py."""
import numpy as np

import prt_amd
import prt_temporal_ref as TR
import prt_testlib as T
from prt_denoise_ref import DEFAULTS
from prt_gpukit import assert_bits_equal, assert_same_image, upload
from prt_refit_ref import bend, teapot_scene
from prt_temporal_ref import TDEFAULTS

F = np.float32


# ----------------------------------------------------------------------------- the temporal stage against its restatement (tests/test_gpu_temporal.py)
def record_equal(got, want, what):
    for k in ("color_var", "pos_len", "normal"):
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


def camera_equal(a, b):
    return bytes(a) == bytes(b)


def check(t, s, exposure=1.0, what="", temporal=None, **kw):
    p = dict(DEFAULTS, **kw)
    tp = dict(TDEFAULTS, **(temporal or {}))
    img = t.denoise_temporal(exposure=exposure, **tp, **p)
    var = t.denoise_variance()
    pend = t.history_export(1)
    want, want_var, want_pend = TR.denoise_temporal(exposure=exposure, **s, **tp, **p)
    assert_bits_equal(img, want, f"{what} {tp} {kw}: image")
    assert_bits_equal(var, want_var, f"{what} {tp} {kw}: variance")
    record_equal(pend, want_pend, f"{what} {tp} {kw}: pending")
    assert camera_equal(pend["camera"], t._camera.desc)
    return img, want_pend


def exported(t, guide_samples=8):
    state, mom = t.accum_export(), t.accum_export_moments()
    albedo, normal = t.denoise_guides(guide_samples)
    return dict(total=state["sum"], count=state["count"], mom=mom, albedo=albedo, normal=normal, position=t.denoise_position())


# ----------------------------------------------------------------------------- deformations against a fresh upload (tests/test_gpu_refit.py)
ARRAYS = ("wnodes", "hot", "tris", "shade", "bump", "root_boxes", "radius")


def moved_normals(mesh, P):
    """calculateVertexNormals of the mesh at positions P, through the oracle."""
    md = T.MeshDesc(mesh["indices"], P, mesh["prim_material"], mesh["materials"].view(T.MATERIAL_DTYPE), texcoords=mesh["texcoords"])
    return T.oracle_vertex_normals(md).normals


def arrays_equal(got, want, what):
    for k in ARRAYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs in {(got[k].view(np.uint32) != want[k].view(np.uint32)).sum()} words"


def soup_scene():
    rng = np.random.default_rng(5)
    n = 3000
    centre = rng.uniform(-1.0, 1.0, (n, 1, 3))
    P = (centre + rng.uniform(-0.08, 0.08, (n, 3, 3))).reshape(-1, 3).astype(F)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    mats = np.array([T.make_material(diffuse=(0.7, 0.6, 0.5)), T.make_material(emissive=(6, 6, 5)),
                     T.make_material(diffuse=(0.9, 0.9, 0.9), reflection=1)], dtype=T.MATERIAL_DTYPE)
    scene = prt_amd.Scene()
    scene.add(prt_amd.Mesh.from_arrays(idx, P, rng.integers(0, 3, n), mats.view(prt_amd.MATERIAL_DTYPE)))
    scene.set_directional_light(prt_amd._normalize((0.2, 1.0, 0.3)), (8.0, 8.0, 7.0))
    return scene, prt_amd.Camera().create((0.0, 0.2, 3.5), (0.0, 0.0, -1.0), 64, 48), 1.0


def atrium_face_normals():
    scene = prt_amd.Scene()
    scene.add(prt_amd.Mesh.atrium(20000, 1, True, True, 0.05))  # no calculate_vertex_normals: the face-normal path
    scene.set_directional_light(prt_amd._normalize((0.05, 1.0, 0.1)), (16.7, 15.6, 11.7))
    return scene, prt_amd.Camera().create((-15.0, 4.0, 0.5), (1.0, 0.08, -0.05), 64, 36), 1.0


def jitter(P):
    return (P + np.random.default_rng(9).normal(0.0, 0.01, P.shape)).astype(F)


def bent_normals(mesh, P):
    n = mesh["normals"] + F(0.2) * np.sin(P, dtype=F)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


CASES = {
    "teapot_bend": (teapot_scene, 1, bend, moved_normals, False),
    "soup_jitter": (soup_scene, 0, jitter, None, False),
    "atrium_normals_passed": (lambda: prt_amd.setup_atrium_standin(64, 36, tris=20000, emissive_fraction=0.05), 0, bend, bent_normals, False),
    "atrium_normals_kept": (lambda: prt_amd.setup_atrium_standin(64, 36, tris=20000, emissive_fraction=0.05), 0, bend, None, True),
    "atrium_face_normals": (atrium_face_normals, 0, bend, None, False),
}


# ----------------------------------------------------------------------------- a scene against the oracle, timed and counting (tests/test_gpu_shadow_skip.py)
COUNTS = ("raysTraced", "occludedTraced", "nBox", "nTri", "nHit", "nTap", "nPx")


def check_scene(tracer, scene, camera, spp, depth, what, exposure=1.0):
    """Timed render: image, raysTraced, occludedTraced = the oracle's; counting render: image and all event counts = the oracle's, and
    no ray skipped.  Returns (oracle stats, rays skipped by the timed render, the oracle's image)."""
    upload(tracer, scene, camera)
    desc = T.scene_desc_from_product(scene, camera, exposure)
    ref, ost = T.OracleScene(desc).render(spp, max_depth=depth)
    img = tracer.render(spp, max_depth=depth, exposure=exposure)
    st = tracer.last_stats
    skipped = tracer.occlusion_skipped()
    print(f"{what}: occlusion rays {ost['occludedTraced']} of {ost['raysTraced']} rays, answered without a walk {skipped}")
    assert_same_image(img, ref, what + ", timed build")
    assert st["raysTraced"] == ost["raysTraced"] and st["occludedTraced"] == ost["occludedTraced"], (what, st, ost)
    img = tracer.render(spp, max_depth=depth, exposure=exposure, count_traffic=True)
    st = tracer.last_stats
    assert tracer.occlusion_skipped() == 0, what
    assert_same_image(img, ref, what + ", counting build")
    for k in COUNTS:
        assert st[k] == ost[k], (what, k, st[k], ost[k])
    return ost, skipped, ref


# ----------------------------------------------------------------------------- the device BVH build against the host builder (tests/test_gpu_parity.py)
def _host_bvh(idx, pos):
    import ctypes as C
    L = prt_amd.lib()
    n = len(idx)
    nodes_p, cnt, remap_p = C.POINTER(prt_amd.BvhNode)(), C.c_uint32(), C.POINTER(C.c_uint32)()
    assert L.prt_host_bvh_build(n, idx.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), 0, C.byref(nodes_p), C.byref(cnt),
                                C.byref(remap_p)) == 0
    nodes = np.frombuffer(C.string_at(nodes_p, cnt.value * C.sizeof(prt_amd.BvhNode)), dtype=T.NODE_DTYPE).copy()
    remap = np.ctypeslib.as_array(remap_p, shape=(n,)).copy()
    L.prt_host_free(nodes_p)
    L.prt_host_free(remap_p)
    return nodes, remap


def _assert_same_tree(nodes, remap, ref_nodes, ref_remap, what):
    assert len(nodes) == len(ref_nodes), (what, len(nodes), len(ref_nodes))
    for f in ("primOrSecondNodeIndex", "triVectorIndex", "primCount", "splitAxis"):
        assert (nodes[f] == ref_nodes[f]).all(), (what, f, int(np.argmax(nodes[f] != ref_nodes[f])))
    # bounds: equal as floats (the min / max of the same vertices; only the sign of a zero bound can depend on the merge order)
    assert np.array_equal(nodes["lower"], ref_nodes["lower"]) and np.array_equal(nodes["upper"], ref_nodes["upper"]), what
    assert (remap == ref_remap).all(), what
