"""Geometry updates from device memory on the MI355X (include/prt_hip.h): prt_hip_deform_meshes reads the caller's positions where they
lie, recomputes the reference's vertex normals and scene radius on the device, and must leave the context in exactly the state
prt_hip_upload_scene produces from the Scene that was updated on the host with the oracle's normals.  Everything at tolerance 0,
except the f64 SAH sums of prt_hip_mesh_info, which are held to the worst case of an f64 sum in any order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import prt_amd
import prt_deform_ref as D
import prt_testlib as T
from prt_denoise_ref import DEFAULTS
from prt_gpucases import CASES, arrays_equal, moved_normals, record_equal
from prt_gpukit import assert_bits_equal
from prt_gpukit import dev, rows, rows2  # noqa: F401  (fixtures)
from prt_refit_ref import RIGID_MOVES, bend, no_negative_zero, refit_nodes, teapot_scene
from prt_temporal_ref import TDEFAULTS

pytestmark = pytest.mark.gpu
F = np.float32
KEEP, GIVEN, RECOMPUTE = 0, 1, 2
EINVAL, ESTATE = -2, -5


def on_device(dev, a):
    """The device address of a float32 copy of `a`."""
    return dev.upload(np.ascontiguousarray(a, dtype=F))


def render_with_counts(t, samples=16):
    img = t.render(samples)
    return img, (t.last_stats["raysTraced"], t.last_stats["occludedTraced"])


# ----------------------------------------------------------------------------- 1. the state after a deform (fails without the feature)
STATE_CASES = {"teapot_bend": RECOMPUTE, "atrium_normals_kept": KEEP, "atrium_face_normals": KEEP}


@pytest.mark.parametrize("case", list(STATE_CASES))
def test_deform_from_device_memory_equals_a_fresh_upload(rows, rows2, dev, case):
    make, m, deform, _, _ = CASES[case]
    mode = STATE_CASES[case]
    scene, camera, _ = make()
    mesh = scene.arrays()["meshes"][m]
    rows.upload_scene(scene)
    rows.set_camera(camera)
    old = rows.scene_arrays()
    P = deform(mesh["positions"])
    assert no_negative_zero(P)
    rows.deform_meshes([(m, on_device(dev, P), mode)])  # radius_auto
    scene.update_positions(m, P, moved_normals(mesh, P) if mode == RECOMPUTE else None)  # the host's way, with the oracle's normals
    rows2.upload_scene(scene)
    rows2.set_camera(camera)
    got, want = rows.scene_arrays(), rows2.scene_arrays()
    arrays_equal(got, want, case)
    assert got["tris"].tobytes() != old["tris"].tobytes() and got["wnodes"].tobytes() != old["wnodes"].tobytes()
    assert got["radius"][0].tobytes() == F(scene.arrays()["radius"]).tobytes()
    img, rays = render_with_counts(rows)
    img2, rays2 = render_with_counts(rows2)
    assert_bits_equal(img, img2, f"{case}: 16 spp")
    assert rays == rays2, (case, rays, rays2)


# ----------------------------------------------------------------------------- 2. rows: normals, boxes, radius
def one_mesh_scene(idx, P):
    mats = np.array([T.make_material(diffuse=(0.7, 0.6, 0.5))], dtype=T.MATERIAL_DTYPE)
    pm = prt_amd.Mesh.from_arrays(idx, P, np.zeros(len(idx), np.uint32), mats.view(prt_amd.MATERIAL_DTYPE))
    pm.calculate_vertex_normals()
    pm.calculate_bounds()
    scene = prt_amd.Scene()
    scene.add(pm)
    return scene, T.MeshDesc(idx, P, np.zeros(len(idx), np.uint32), mats)


def fan_257():
    t = np.linspace(0.0, 5.0, 256)
    P = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(t), np.sin(t), 0.1 * t], axis=1)]).astype(F)
    idx = np.array([(0, k, k + 1) for k in range(1, 256)], dtype=np.uint32)
    assert len(P) == 257
    return idx, P


ROW_MESHES = {
    "hostile": D.hostile_mesh,
    "one_triangle": lambda: (np.array([[0, 1, 2]], dtype=np.uint32), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], dtype=F)),
    "fan_257_vertices": fan_257,
}


@pytest.mark.parametrize("which", list(ROW_MESHES))
def test_recomputed_normals_boxes_and_radius(rows, dev, which):
    idx, P = ROW_MESHES[which]()
    scene, desc = one_mesh_scene(idx, (F(2.0) * P).astype(F))  # uploaded at twice the size (exact), deformed to P
    rows.upload_scene(scene)
    with pytest.raises(prt_amd.PrtError, match=r"\(-5\).*no update yet"):
        rows.mesh_vertices(0)
    rows.deform_meshes([(0, on_device(dev, P), RECOMPUTE)])
    gotP, gotN = rows.mesh_vertices(0)
    want = T.oracle_vertex_normals(desc).normals
    assert gotP.tobytes() == P.tobytes()
    differ = ~(np.isnan(gotN) & np.isnan(want)) & (gotN.view(np.uint32) != want.view(np.uint32))
    assert D.bits_equal(gotN, want), f"{which}: {differ.sum()} words differ, first at vertex {np.nonzero(differ.any(axis=1))[0][:4]}"
    info = rows.mesh_info(0)
    assert (info["vertexBox"] == np.concatenate([P.min(axis=0), P.max(axis=0)])).all(), which
    scene.update_positions(0, P, want)
    a = scene.arrays()
    assert info["radius"].tobytes() == F(a["radius"]).tobytes() == D.radius([D.vertex_box(P)]).tobytes()
    assert rows.scene_arrays()["radius"][0].tobytes() == F(a["radius"]).tobytes()
    nodes = a["meshes"][0]["nodes"]
    assert (info["internalNodes"], info["leaves"]) == (int((nodes["primCount"] == 0xF).sum()), int((nodes["primCount"] != 0xF).sum()))
    assert info["rootBox"].tobytes() == np.concatenate([nodes["lower"][0], nodes["upper"][0]]).tobytes()


# ----------------------------------------------------------------------------- 3. GIVEN and HOST against prt_hip_update_meshes
@pytest.mark.parametrize("flavour", ["device_given", "host_given", "host_recompute", "host_keep"])
def test_flavours_equal_update_meshes_on_a_twin(rows, rows2, dev, flavour):
    scene, camera, _ = teapot_scene()
    twin, _, _ = teapot_scene()
    tea = scene.arrays()["meshes"][1]
    P = bend(tea["positions"])
    N = moved_normals(tea, P)
    keep = flavour == "host_keep"
    twin_scene_normals = None if keep else N
    rows2.upload_scene(twin)
    twin.update_positions(1, P, twin_scene_normals)
    rows2.update_meshes(twin, [1], keep_normals=keep)
    rows.upload_scene(scene)
    if flavour == "device_given":
        rows.deform_meshes([(1, on_device(dev, P), on_device(dev, N))])
    else:
        rows.deform_meshes([(1, P, {"host_given": N, "host_recompute": RECOMPUTE, "host_keep": KEEP}[flavour])], host=True)
    arrays_equal(rows.scene_arrays(), rows2.scene_arrays(), flavour)
    gotP, gotN = rows.mesh_vertices(1, normals=not keep)
    assert gotP.tobytes() == P.tobytes() and (keep or gotN.tobytes() == N.tobytes())
    # without RADIUS_AUTO the radius is the caller's: 0 keeps it
    before = rows.scene_arrays()["radius"][0]
    rows.deform_meshes([(1, (F(4.0) * P).astype(F), KEEP)], host=True, radius_auto=False)
    assert rows.scene_arrays()["radius"][0].tobytes() == before.tobytes()


def test_auto_radius_sees_meshes_the_host_path_changed(rows, rows2, dev):
    """Mesh 0 goes through prt_hip_update_meshes, mesh 1 through the device path: the radius is the host Scene's after both."""
    scene, camera, _ = teapot_scene()
    a = scene.arrays()
    box, tea = a["meshes"]
    rows.upload_scene(scene)
    P0 = (box["positions"] * F(1.25)).astype(F)
    scene.update_positions(0, P0)
    rows.update_meshes(scene, [0])
    assert (rows.mesh_info(0)["vertexBox"] == D.vertex_box(P0)).all()  # the staged copy, reduced on demand
    rows.upload_scene(teapot_scene()[0])
    rows.update_meshes(scene, [0])
    P1 = RIGID_MOVES["shift0.25x"](tea["positions"])
    rows.deform_meshes([(1, on_device(dev, P1), RECOMPUTE)])
    scene.update_positions(1, P1, moved_normals(tea, P1))
    rows2.upload_scene(scene)
    arrays_equal(rows.scene_arrays(), rows2.scene_arrays(), "host path for mesh 0, device path for mesh 1")


# ----------------------------------------------------------------------------- 4. a caller's stream
def test_copy_and_deform_on_a_callers_stream(rows, rows2, dev):
    scene, camera, _ = teapot_scene()
    tea = scene.arrays()["meshes"][1]
    P = bend(tea["positions"])
    rows.upload_scene(scene)
    stream, dP = dev.stream(), dev.alloc(P.nbytes)
    dev.fill(dP, 0xA5, P.nbytes)
    dev.upload_async(P, stream, dP)
    rows.deform_meshes([(1, dP, RECOMPUTE)], stream=stream)  # no synchronisation in between
    dev.synchronize(stream)
    scene.update_positions(1, P, moved_normals(tea, P))
    rows2.upload_scene(scene)
    arrays_equal(rows.scene_arrays(), rows2.scene_arrays(), "copy and deform on one stream")


def test_torch_tensor_on_torchs_stream():
    """tests/deform_torch_child.py in a process of its own (torch must load its HIP runtime before the library binds to one)."""
    prt_amd.build()
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(T.ROOT, "tests", "deform_torch_child.py")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "ok deform" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- 5. what a deform invalidates
def test_invalidation_is_update_meshes(dev):
    prt_amd.build()
    out = []
    for device_path in (True, False):
        scene, camera, exposure = teapot_scene()
        tea = scene.arrays()["meshes"][1]
        P = RIGID_MOVES["shift0.25x"](tea["positions"])
        N = moved_normals(tea, P)
        t = prt_amd.PathTracer()
        try:
            t.upload_scene(scene)
            t.set_camera(camera)
            t.history_reset()
            for k in range(2):
                t.adaptive_pass(8, 0.0, 8 * (k + 1), 8 * (k + 1), 0.01)
            t.denoise_temporal(exposure=exposure, **TDEFAULTS, **DEFAULTS)
            if device_path:
                t.deform_meshes([(1, on_device(dev, P), RECOMPUTE)])
            else:
                scene.update_positions(1, P, N)
                t.update_meshes(scene, [1])
            counts = t.accum_counts()
            assert (counts == 0).all(), "the accumulator is empty after the call"
            t.adaptive_pass(8, 0.0, 8, 8, 0.01)
            out.append((t.denoise_temporal(exposure=exposure, **TDEFAULTS, **DEFAULTS), t.history_export(0)))
        finally:
            t.close()
    assert_bits_equal(out[0][0], out[1][0], "denoise_temporal after deform_meshes against after update_meshes")
    record_equal(out[0][1], out[1][1], "the history after deform_meshes against after update_meshes")


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_change_nothing(rows, dev):
    scene, camera, _ = teapot_scene()
    a = scene.arrays()
    box, tea = a["meshes"]
    rows.upload_scene(scene)
    rows.set_camera(camera)
    rows.accumulate(8)
    before = rows.scene_arrays()
    L = rows._L
    P, PB = bend(tea["positions"]), np.ascontiguousarray(box["positions"])
    dP, dB = on_device(dev, P), on_device(dev, PB)
    AUTO, HOST = prt_amd.MeshDeform.RADIUS_AUTO, prt_amd.MeshDeform.HOST

    def de(mesh=1, count=len(P), pos=dP, normals=None, mode=KEEP, radius=0.0):
        d = prt_amd.MeshDeform()
        d.mesh, d.vertexCount, d.positions, d.normals, d.normalsMode, d.radius = mesh, count, pos, normals, mode, radius
        return d

    bad = [([de(mesh=2)], AUTO, "mesh index"), ([de(count=len(P) - 1)], AUTO, "vertexCount"), ([de(pos=None)], AUTO, "positions"),
           ([de(), de()], AUTO, "twice"), ([de(radius=-1.0)], 0, "radius"), ([de(radius=float("inf"))], 0, "radius"),
           ([de(radius=float("nan"))], 0, "radius"), ([], AUTO, "no mesh"),
           ([de(mode=3)], AUTO, "normalsMode"), ([de()], 4, "flag"), ([de()], AUTO | HOST | 8, "flag"),
           ([de(mode=GIVEN)], AUTO, "NULL normals"), ([de(mode=KEEP, normals=dP)], AUTO, "normals must be NULL"),
           ([de(mode=RECOMPUTE, normals=dP)], AUTO, "normals must be NULL"),
           ([de(mesh=0, count=len(PB), pos=dB, normals=dB, mode=GIVEN)], AUTO, "without vertex normals"),
           ([de(mesh=0, count=len(PB), pos=dB, mode=RECOMPUTE)], AUTO, "without vertex normals"),
           ([de(radius=1.0)], AUTO, "RADIUS_AUTO")]
    for ds, flags, word in bad:
        arr = (prt_amd.MeshDeform * max(len(ds), 1))(*ds)
        assert L.prt_hip_deform_meshes(rows._ctx, len(ds), arr, flags, None) == EINVAL, word
        assert word in L.prt_hip_last_error().decode(), (word, L.prt_hip_last_error().decode())
    assert L.prt_hip_deform_meshes(rows._ctx, 1, None, AUTO, None) == EINVAL
    assert (rows.accum_counts() == 8).all()  # a refused call does not even empty the accumulator
    arrays_equal(rows.scene_arrays(), before, "after the refused calls")
    with pytest.raises(prt_amd.PrtError, match=r"\(-5\)"):
        rows.mesh_vertices(1)  # and no refused call counted as an update
    with pytest.raises(prt_amd.PrtError, match=r"\(-2\)"):
        rows.mesh_info(2)
    fresh = prt_amd.PathTracer()
    try:
        arr = (prt_amd.MeshDeform * 1)(de())
        assert L.prt_hip_deform_meshes(fresh._ctx, 1, arr, AUTO, None) == ESTATE
        assert L.prt_hip_get_mesh_vertices(fresh._ctx, 0, None, None, 0, None) == ESTATE
        assert L.prt_hip_mesh_info(fresh._ctx, 0, C.byref(prt_amd.MeshInfo())) == ESTATE
    finally:
        fresh.close()
    rows.deform_meshes([(1, dP, RECOMPUTE)])  # and the accepted call still works
    assert rows.mesh_vertices(1)[0].tobytes() == P.tobytes()


# ----------------------------------------------------------------------------- 7. the tree readout
def test_mesh_info(rows, rows2, dev):
    scene, camera, _ = teapot_scene()
    a = scene.arrays()
    tea = a["meshes"][1]
    rows.upload_scene(scene)

    def check(info, nodes, what):
        ref = D.sah(nodes)
        assert (info["internalNodes"], info["leaves"]) == (ref["internalNodes"], ref["leaves"]), what
        for k, n in (("internalArea", ref["internalNodes"]), ("leafArea", ref["leaves"])):
            err = abs(info[k] - ref[k]) / ref[k]
            print(f"{what}: {k} {info[k]!r} against fsum {ref[k]!r}: relative {err:.3e}, bound {n * 2.0 ** -52:.3e}")
            assert err <= n * 2.0 ** -52, (what, k)
        assert info["rootArea"] == ref["rootArea"], what
        assert info["sahCost"] == (0.125 * info["internalArea"] + info["leafArea"]) / info["rootArea"], what

    for m in (0, 1):
        first = rows.mesh_info(m)
        check(first, a["meshes"][m]["nodes"], f"mesh {m} as uploaded")
        assert first["sahCost"] == first["sahCostAtUpload"]
        assert (first["vertexBox"] == D.vertex_box(a["meshes"][m]["positions"])).all()
        again = rows.mesh_info(m)
        assert all(np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes() for k in first), "two calls return identical bits"
    at_upload = rows.mesh_info(1)["sahCost"]
    P = bend(tea["positions"])
    dP, dBack = on_device(dev, P), on_device(dev, tea["positions"])
    rows.deform_meshes([(1, dP, RECOMPUTE)])
    bent = rows.mesh_info(1)
    check(bent, refit_nodes(tea["nodes"], tea["remap"], tea["indices"], P), "after the bend")
    assert bent["sahCostAtUpload"] == at_upload and bent["sahCost"] > at_upload
    assert rows.mesh_info(0)["sahCost"] == rows.mesh_info(0)["sahCostAtUpload"]  # the box did not move
    rows.deform_meshes([(1, dBack, RECOMPUTE)])
    back = rows.mesh_info(1)
    assert back["sahCost"] == back["sahCostAtUpload"] == at_upload
    # a rigid move costs nothing: the refitted tree is the rebuilt one (tests/test_refit_cpu.py)
    name = "scale2"
    Pm = RIGID_MOVES[name](tea["positions"])
    rows.deform_meshes([(1, Pm, RECOMPUTE)], host=True)
    pm = prt_amd.Mesh.from_arrays(tea["indices"], Pm, tea["prim_material"], tea["materials"], texcoords=tea["texcoords"])
    rebuilt = prt_amd.setup_cornell_box(64, 64, teapot_mesh=pm)[0]
    rows2.upload_scene(rebuilt)
    moved, fresh = rows.mesh_info(1), rows2.mesh_info(1)
    assert moved["sahCost"] == fresh["sahCost"] == fresh["sahCostAtUpload"], name
    assert moved["sahCostAtUpload"] == at_upload
    # the host path captures the tree as uploaded too
    scene2, _, _ = teapot_scene()
    rows2.upload_scene(scene2)
    scene2.update_positions(1, P)
    rows2.update_meshes(scene2, [1], keep_normals=True)
    info = rows2.mesh_info(1)
    assert info["sahCostAtUpload"] == at_upload and info["sahCost"] == bent["sahCost"]
