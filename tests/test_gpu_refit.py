"""Geometry updates on the MI355X (include/prt_hip.h "geometry updates"): prt_hip_update_meshes must leave the context in exactly the
state prt_hip_upload_scene produces from the updated scene.  Everything is compared at tolerance 0: against the oracle rendering a
scene BUILT FROM SCRATCH with the moved teapot (for the rigid moves whose rebuild is the refit, tests/test_refit_cpu.py), against
a second context that uploaded the updated Scene (device arrays byte for byte, images, event counts), against the numpy
restatement of the refit rule, and -- for the temporal stage -- against tests/prt_temporal_ref.py."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_temporal_ref as TR
import prt_testlib as T
from prt_denoise_ref import DEFAULTS
from prt_gpucases import CASES, arrays_equal, camera_equal, check, exported, moved_normals, record_equal
from prt_gpukit import assert_bits_equal
from prt_gpukit import dev, rows, rows2, tracer  # noqa: F401  (fixtures)
from prt_refit_ref import RIGID_MOVES, bend, no_negative_zero, refit_nodes, teapot_scene
from prt_temporal_ref import TDEFAULTS

pytestmark = pytest.mark.gpu
F = np.float32
EVENTS = ("raysTraced", "occludedTraced", "nBox", "nTri", "nTap", "modeBox", "modeTri", "modeTap")


def record_boxes(nodes):
    """The box part (12 floats) of the wide records of a node array: one record per internal node, in node order (prt_device.h)."""
    inner = np.nonzero(nodes["primCount"] == 0xF)[0]
    c0, c1 = nodes[inner + 1], nodes[nodes["primOrSecondNodeIndex"][inner]]
    lo0, hi0, lo1, hi1 = c0["lower"], c0["upper"], c1["lower"], c1["upper"]
    return np.stack([lo0[:, 0], hi0[:, 0], lo0[:, 1], hi0[:, 1], lo0[:, 2], hi0[:, 2], lo1[:, 2], hi1[:, 2],
                     lo1[:, 0], hi1[:, 0], lo1[:, 1], hi1[:, 1]], axis=1).astype(F)


def traffic(t, samples=8):
    img = t.render(samples, count_traffic=True)
    return img, {k: t.last_stats[k] for k in EVENTS}


# ----------------------------------------------------------------------------- 1. rigid moves against the oracle
def against_oracle(tracer, scene, camera, exposure, what):
    img = tracer.render(16)
    st = tracer.last_stats
    o = T.OracleScene(T.scene_desc_from_product(scene, camera, exposure))  # built from scratch from the moved arrays
    ref, ost = o.render(16)
    assert_bits_equal(img, ref, f"{what}: image against the oracle")
    assert st["raysTraced"] == ost["raysTraced"] and st["occludedTraced"] == ost["occludedTraced"], (what, st, ost)
    for kind in (0, 2):
        assert_bits_equal(tracer.gbuffer(kind), o.gbuffer(kind, (0, 0, camera.width - 1, camera.height - 1)), f"{what}: gbuffer {kind}")
    return img


def test_rigid_moves_match_the_oracle(tracer):
    scene, camera, exposure = teapot_scene()
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    tea = scene.arrays()["meshes"][1]
    first = against_oracle(tracer, scene, camera, exposure, "as uploaded")
    images = [first]
    for name, move in RIGID_MOVES.items():  # a chain of three updates, no upload in between
        P = move(tea["positions"])
        assert no_negative_zero(P)
        scene.update_positions(1, P, moved_normals(tea, P))
        tracer.update_meshes(scene, [1])
        images.append(against_oracle(tracer, scene, camera, exposure, name))
    assert all(images[i].tobytes() != images[j].tobytes() for i in range(4) for j in range(i))  # the moves are visible
    scene.update_positions(1, tea["positions"], tea["normals"])
    tracer.update_meshes(scene, [1])
    assert_bits_equal(tracer.render(16), first, "back at the original positions")


# ----------------------------------------------------------------------------- 2. general deformations against a fresh upload


@pytest.mark.parametrize("case", list(CASES))
def test_deformation_equals_a_fresh_upload(rows, rows2, case):
    make, m, deform, normals_of, keep = CASES[case]
    scene, camera, _ = make()
    before = scene.arrays()
    mesh = before["meshes"][m]
    if case.startswith("atrium"):
        mats = mesh["materials"]
        assert (mats["bumpMap"] >= 0).any() and (mats["alphaTest"] != 0).any() and (mats["emissive"] > 0).any()
        assert (mesh["normals"] is None) == (case == "atrium_face_normals")
    rows.upload_scene(scene)
    rows.set_camera(camera)
    old_img = rows.render(8)
    old = rows.scene_arrays()
    P = deform(mesh["positions"])
    assert no_negative_zero(P)
    scene.update_positions(m, P, None if normals_of is None else normals_of(mesh, P))
    rows.update_meshes(scene, [m], keep_normals=keep)
    rows2.upload_scene(scene)
    rows2.set_camera(camera)
    got, want = rows.scene_arrays(), rows2.scene_arrays()
    arrays_equal(got, want, case)
    assert got["tris"].tobytes() != old["tris"].tobytes() and got["wnodes"].tobytes() != old["wnodes"].tobytes()
    # the device's node boxes are the numpy refit of the uploaded tree
    first = sum(int((mm["nodes"]["primCount"] == 0xF).sum()) for mm in before["meshes"][:m])
    expect = refit_nodes(mesh["nodes"], mesh["remap"], mesh["indices"], P)
    boxes = record_boxes(expect)
    assert got["wnodes"][first:first + len(boxes), :12].tobytes() == boxes.tobytes(), case
    assert got["root_boxes"][m].tobytes() == np.concatenate([expect["lower"][0], expect["upper"][0]]).tobytes()
    assert got["radius"][0].tobytes() == F(scene.arrays()["radius"]).tobytes()
    # pad slots stay zero, and what is not positional stays what it was
    assert got["shade"][:, [3, 7, 11, 12, 13, 14, 15]].tobytes() == old["shade"][:, [3, 7, 11, 12, 13, 14, 15]].tobytes()
    assert got["wnodes"][:, 12:].tobytes() == old["wnodes"][:, 12:].tobytes()
    # images and event counts
    img, ev = traffic(rows)
    img2, ev2 = traffic(rows2)
    assert_bits_equal(img, img2, f"{case}: counting render")
    assert ev == ev2, (case, ev, ev2)
    timed = rows.render(8)
    assert_bits_equal(timed, rows2.render(8), f"{case}: render")
    assert timed.tobytes() != old_img.tobytes()


def test_c4_class_arrays_equal_a_fresh_upload(rows, rows2):
    """2.5 M triangles, arrays only: every launch-size path of the two kernels."""
    scene, camera, _ = prt_amd.setup_atrium_standin(64, 36, tris=2500000, seed=4)
    rows.upload_scene(scene)
    P = bend(scene.arrays()["meshes"][0]["positions"])
    assert no_negative_zero(P)
    scene.update_positions(0, P)
    rows.update_meshes(scene, keep_normals=True)
    rows2.upload_scene(scene)
    arrays_equal(rows.scene_arrays(), rows2.scene_arrays(), "c4")
    small = teapot_scene()[0]
    rows.upload_scene(small)  # give the memory back
    rows2.upload_scene(small)


# ----------------------------------------------------------------------------- 3. several meshes
def test_one_mesh_of_two_and_two_in_one_call(rows, rows2):
    scene, camera, _ = teapot_scene()
    a = scene.arrays()
    box, tea = a["meshes"]
    only_box = prt_amd.Scene()
    only_box.add(prt_amd.Mesh.cornell_box(True))
    rows2.upload_scene(only_box)
    s0 = rows2.scene_arrays()
    slots0, recs0 = len(s0["tris"]), len(s0["wnodes"])
    rows.upload_scene(scene)
    rows.set_camera(camera)
    old = rows.scene_arrays()
    assert old["tris"][:slots0].tobytes() == s0["tris"].tobytes()  # the box's slots come first
    P1 = RIGID_MOVES["shift0.25x"](tea["positions"])
    scene.update_positions(1, P1)
    rows.update_meshes(scene, [1], keep_normals=True)
    got = rows.scene_arrays()
    for k, n in (("tris", slots0), ("shade", slots0), ("wnodes", recs0)):
        assert got[k][:n].tobytes() == old[k][:n].tobytes(), k  # the box is untouched
        if k != "shade":  # (the teapot's vertex normals were kept)
            assert got[k][n:].tobytes() != old[k][n:].tobytes(), k  # the teapot moved
    assert got["shade"][slots0:].tobytes() == old["shade"][slots0:].tobytes()
    assert got["root_boxes"][0].tobytes() == old["root_boxes"][0].tobytes()
    # both meshes in one call = one call each = a fresh upload
    P0 = (box["positions"] * F(1.25)).astype(F)
    assert no_negative_zero(P0)
    scene.update_positions(0, P0)
    rows2.upload_scene(teapot_scene()[0])
    rows2.update_meshes(scene, [0])
    rows2.update_meshes(scene, [1])
    rows.update_meshes(scene, [1, 0])
    arrays_equal(rows.scene_arrays(), rows2.scene_arrays(), "one call against two")
    rows2.upload_scene(scene)
    arrays_equal(rows.scene_arrays(), rows2.scene_arrays(), "one call against a fresh upload")


# ----------------------------------------------------------------------------- 4. life cycle
def test_life_cycle_after_an_update(tracer):
    scene, camera, exposure = teapot_scene()
    tea = scene.arrays()["meshes"][1]
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    tracer.seed = 12345
    tracer.accumulate(16)
    tracer.set_denoise_guides(np.full((64, 64, 3), 0.5, F), np.full((64, 64, 3), 0.25, F))
    tracer.set_denoise_position(np.ones((64, 64, 4), F))
    P = RIGID_MOVES["shift0.25x"](tea["positions"])
    scene.update_positions(1, P, moved_normals(tea, P))
    tracer.update_meshes(scene, [1])
    # emptied and unbound: another seed is accepted, and every pixel starts again
    state = tracer.accum_export()
    assert state["seed"] == 0 and (state["count"] == 0).all()
    tracer.seed = 777
    try:
        img8 = tracer.accumulate(8)
        state = tracer.accum_export()
        assert state["seed"] == 777 and (state["count"] == 8).all()
        img16 = tracer.accumulate(8)
        assert_bits_equal(img16, tracer.render(16), "accumulate after an update against render on the new scene")
        fresh = prt_amd.PathTracer(seed=777)
        try:
            fresh.upload_scene(scene)
            fresh.set_camera(camera)
            assert_bits_equal(fresh.accumulate(8), img8, "first pass after the update against a fresh context")
            fresh.accumulate(8)
            # host planes were dropped; guides and position are rendered again, of the new geometry
            for got, want, what in zip(tracer.denoise_guides(8), fresh.denoise_guides(8), ("albedo", "normal")):
                assert_bits_equal(got, want, what)
            assert_bits_equal(tracer.denoise_position(), fresh.denoise_position(), "position")
            assert_bits_equal(tracer.denoise(**DEFAULTS), fresh.denoise(**DEFAULTS), "denoise after an update")
        finally:
            fresh.close()
    finally:
        tracer.seed = 12345


def test_temporal_records_survive_an_update(tracer):
    scene, camera, exposure = teapot_scene(128)
    tea = scene.arrays()["meshes"][1]
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    tracer.history_reset()
    for k in range(4):
        tracer.adaptive_pass(8, 0.0, 8 * (k + 1), 8 * (k + 1), 0.01)
    tracer.denoise_temporal(exposure=exposure, **TDEFAULTS, **DEFAULTS)
    pend = tracer.history_export(1)
    with pytest.raises(prt_amd.PrtError):
        tracer.history_export(0)
    P = RIGID_MOVES["shift0.25x"](tea["positions"])
    scene.update_positions(1, P, moved_normals(tea, P))
    tracer.update_meshes(scene, [1])
    hist = tracer.history_export(0)
    record_equal(hist, pend, "the pending record is promoted")
    assert camera_equal(hist["camera"], camera.desc)
    with pytest.raises(prt_amd.PrtError, match="no pending"):
        tracer.history_export(1)
    tracer.adaptive_pass(8, 0.0, 8, 8, 0.01)
    s = exported(tracer)
    s["history"] = hist
    check(tracer, s, exposure=exposure, what="after the update")
    record_equal(tracer.history_export(0), pend, "the history after the denoise")
    # who takes history: from the restatement's own masks
    m = TR.merge(s["total"], s["count"], s["mom"], s["albedo"], s["normal"], s["position"], hist, **TDEFAULTS)
    X, t = s["position"][..., :3].astype(np.float64), s["position"][..., 3].astype(np.float64)
    hX, hlen = hist["pos_len"][..., :3].astype(np.float64), hist["pos_len"][..., 3]
    same_surface = (t >= 0) & (hlen > 0) & (((X - hX) ** 2).sum(-1) <= (0.01 * t) ** 2)
    moved_surface = (t >= 0) & ~same_surface
    kept, fresh = same_surface & m["have"], moved_surface & ~m["have"]
    print(f"update (0.25, 0, 0): {same_surface.sum()} pixels see the surface they saw, {kept.sum()} of them take history; "
          f"{moved_surface.sum()} see another one, {fresh.sum()} of them take none")
    assert kept.sum() > 0 and fresh.sum() > 0
    # an update in a view that was never denoised keeps the history
    scene.update_positions(1, tea["positions"], tea["normals"])
    tracer.update_meshes(scene, [1])
    promoted = tracer.history_export(0)
    scene.update_positions(1, P)
    tracer.update_meshes(scene, [1], keep_normals=True)
    record_equal(tracer.history_export(0), promoted, "an undenoised state keeps the history")


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing(tracer):
    EINVAL, ESTATE = -2, -5
    scene, camera, _ = teapot_scene()
    a = scene.arrays()
    box, tea = a["meshes"]
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    before = tracer.render(16)
    tracer.accumulate(8)
    L = tracer._L
    P = RIGID_MOVES["shift0.25x"](tea["positions"])
    PB = np.ascontiguousarray(box["positions"])
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

    def up(mesh=1, count=len(P), pos=P, normals=None, radius=0.0):
        u = prt_amd.MeshUpdate()
        u.mesh, u.vertexCount, u.radius = mesh, count, radius
        u.positions = None if pos is None else fp(pos)
        u.normals = None if normals is None else fp(normals)
        return u

    bad = [([up(mesh=2)], "mesh index"), ([up(count=len(P) - 1)], "vertexCount"), ([up(pos=None)], "positions"),
           ([up(mesh=0, count=len(PB), pos=PB, normals=PB)], "normals"), ([up(), up()], "twice"), ([up(radius=-1.0)], "radius"),
           ([up(radius=float("inf"))], "radius"), ([up(radius=float("nan"))], "radius"), ([], "no mesh")]
    for ups, word in bad:
        arr = (prt_amd.MeshUpdate * max(len(ups), 1))(*ups)
        assert L.prt_hip_update_meshes(tracer._ctx, len(ups), arr, None) == EINVAL, word
        assert word in L.prt_hip_last_error().decode(), (word, L.prt_hip_last_error().decode())
    assert L.prt_hip_update_meshes(tracer._ctx, 1, None, None) == EINVAL
    assert (tracer.accum_export()["count"] == 8).all()  # a refused call does not even empty the accumulator
    assert_bits_equal(tracer.render(16), before, "render after the refused calls")
    fresh = prt_amd.PathTracer()
    try:
        arr = (prt_amd.MeshUpdate * 1)(up())
        assert L.prt_hip_update_meshes(fresh._ctx, 1, arr, None) == ESTATE
        with pytest.raises(prt_amd.PrtError, match=r"\(-5\)"):
            fresh.update_meshes(scene)
    finally:
        fresh.close()
    tracer.update_meshes(scene)  # and the accepted call still works: nothing moved, the same image
    assert_bits_equal(tracer.render(16), before, "an update with the uploaded positions")


# ----------------------------------------------------------------------------- 6. a caller's stream
def test_update_render_download_on_a_callers_stream(tracer, dev):
    scene, camera, _ = teapot_scene()
    tea = scene.arrays()["meshes"][1]
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    P = bend(tea["positions"])
    scene.update_positions(1, P, moved_normals(tea, P))
    fresh = prt_amd.PathTracer()
    try:
        fresh.upload_scene(scene)
        fresh.set_camera(camera)
        want = fresh.render(16)
    finally:
        fresh.close()
    stream, target = dev.stream(), dev.alloc(64 * 64 * 3 * 4)
    tracer.render_async(0, 0, 63, 63, 16, d_rgb=target, stream=stream)  # the old geometry, queued ahead
    tracer.update_meshes(scene, [1], stream=stream)
    tracer.render_async(0, 0, 63, 63, 16, d_rgb=target, stream=stream)
    got = np.zeros((64, 64, 3), F)
    dev.download_async(got, target, stream)
    dev.synchronize(stream)
    tracer.stats()
    assert_bits_equal(got, want, "update, render and download on one stream")
