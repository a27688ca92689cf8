"""Hostile rays and geometry on the MI355X (tests/prt_hostile.py; the CPU half is tests/test_hostile_cpu.py): the edge logic of the
traversal stepper (prt_device.h) -- the FAST = false selects for NaN slab products, strict against non-strict box compares on boxes of
zero extent, near-child and first-mesh ties on coincident geometry -- through prt_hip_trace_rays and the frame kernel, the device BVH
build on snapped / duplicated / planar soups, and prt_hip_update_meshes with -0.0 positions, degenerate triangles and a one-triangle
mesh.  Everything at tolerance 0 against the compiled reference's stored answers, the live oracle, the host builder, or a second
context that uploaded the updated scene (where the sign of a zero box bound and the bits of a never-hit triangle's NaN may differ)."""

import numpy as np
import pytest

import prt_amd
import prt_hostile as H
import prt_testlib as T
from prt_gpucases import _assert_same_tree, _host_bvh
from prt_gpukit import assert_bits_equal
from prt_gpukit import gpu_event_accounting, rows, rows2  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
F = np.float32
EVENTS = ("raysTraced", "occludedTraced", "nBox", "nTri", "nTap", "modeBox", "modeTri", "modeTap")
ORACLE_EVENTS = ("raysTraced", "occludedTraced", "nBox", "nTri", "nHit", "nTap", "nPx")
MODES = ((0, "single"), (1, "packet"), (2, "occluded_single"), (3, "occluded_packet"))
LIGHT = {"grid": (0.0, 1.0, 0.0), "twins": (0.0, 1.0, 0.0), "flat": (0.0, 0.0, 1.0)}
CASES = [(name, seed) for name in H.SCENES for seed in H.SEEDS]


# (differs from prt_gpukit.tracer: max_depth=8)
@pytest.fixture(scope="module")
def tracer():
    prt_amd.build()
    t = prt_amd.PathTracer(max_depth=8)
    yield t
    t.close()


def oracle_answers(desc, org, d, max_t):
    o = T.OracleScene(desc)
    single, occ1 = o.intersect_single(org, d, max_t)
    packet, occ8 = o.intersect_packet(org, d, max_t)
    return dict(single=single, packet=packet, occluded_single=occ1, occluded_packet=occ8)


def trace_all(rows, org, d, max_t):
    return {key: rows.trace_rays(mode, org, d, max_t) for mode, key in MODES}


def assert_answers(got, want, what):
    for mode, key in MODES:
        if mode < 2:
            if got[key].tobytes() != want[key].tobytes():
                bad = np.nonzero(got[key].view(np.uint8).reshape(len(got[key]), -1) != want[key].view(np.uint8).reshape(len(want[key]), -1))[0]
                raise AssertionError(f"{what}: mode {mode}, {len(np.unique(bad))} rays differ, first {bad[:1]}")
        else:
            assert (got[key]["t"] == want[key]).all(), f"{what}: mode {mode}, {int((got[key]['t'] != want[key]).sum())} flags differ"


# ----------------------------------------------------------------------------- 1. the four traversals
@pytest.mark.parametrize("name,seed", CASES)
def test_traversals_match_reference_and_oracle(rows, name, seed):
    g = H.golden(name, seed)
    scene, camera, desc = H.product_scene(g["meshes"])
    rows.upload_scene(scene)
    got = trace_all(rows, g["org"], g["dir"], g["max_t"])
    assert_answers(got, g, f"{name}{seed} against the compiled reference")
    assert_answers(got, oracle_answers(desc, g["org"], g["dir"], g["max_t"]), f"{name}{seed} against the oracle")


@pytest.mark.parametrize("which,seed", [(w, s) for w in H.SCALES for s in H.SEEDS])
def test_traversals_match_oracle_on_scaled_scenes(rows, which, seed):
    """The twins scene times 2**-60 (squares of edge lengths are denormal or zero) and 2**40 (they overflow in normalize3)."""
    meshes, org, d, max_t = H.scaled(which, seed)
    scene, camera, desc = H.product_scene(meshes)
    rows.upload_scene(scene)
    want = oracle_answers(desc, org, d, max_t)
    assert_answers(trace_all(rows, org, d, max_t), want, f"{which}{seed}")
    if which == "huge":
        assert (want["single"]["t"] != -1).any() and (want["packet"]["t"] != -1).any()


# ----------------------------------------------------------------------------- 2. wave composition
def test_answers_do_not_depend_on_the_launch_a_ray_is_part_of(rows):
    """Launches smaller than a wave (8 rays), of a wave and a bit (72), and the 128 packets in another order: the cooperative leaf
    rounds with mostly idle lanes, and with other neighbours, give every ray the answer of the full launch."""
    g = H.golden("grid", 0)
    scene, _, _ = H.product_scene(g["meshes"])
    rows.upload_scene(scene)
    org, d, max_t = g["org"], g["dir"], g["max_t"]
    full = trace_all(rows, org, d, max_t)
    assert_answers(full, g, "the full launch")
    order = np.random.default_rng(1000).permutation(H.RAYS // 8)
    perm = (order[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
    assert (perm != np.arange(H.RAYS)).any()
    for mode, key in MODES:
        for n in (8, 72):
            part = rows.trace_rays(mode, org[:n], d[:n], max_t)
            assert part.tobytes() == full[key][:n].tobytes(), f"mode {mode}: the first {n} rays alone"
        shuffled = rows.trace_rays(mode, org[perm], d[perm], max_t)
        assert shuffled.tobytes() == full[key][perm].tobytes(), f"mode {mode}: packets in another order"


# ----------------------------------------------------------------------------- 3. the frame kernel
@pytest.mark.parametrize("name,reflective", [("grid", ()), ("twins", ()), ("flat", ()), ("grid", (2,))])
def test_frames_match_the_oracle(tracer, name, reflective):
    g = H.golden(name, 0)
    scene, camera, desc = H.product_scene(g["meshes"], light=LIGHT[name], reflective=reflective)
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    ref, ost = T.OracleScene(desc).render(8, max_depth=8)
    assert not np.isnan(ref).any() and (ref != 0).any() and ost["occludedTraced"] > 0
    what = f"{name} reflective {reflective}"
    img = tracer.render(8, max_depth=8)
    st = tracer.last_stats
    assert_bits_equal(img, ref, what + ": timed build")
    assert st["raysTraced"] == ost["raysTraced"] and st["occludedTraced"] == ost["occludedTraced"], (what, st, ost)
    img = tracer.render(8, max_depth=8, count_traffic=True)
    st = tracer.last_stats
    assert_bits_equal(img, ref, what + ": counting build")
    for k in ORACLE_EVENTS:
        assert st[k] == ost[k], (what, k, st[k], ost[k])


# ----------------------------------------------------------------------------- 4. the device BVH build
def build_cases():
    for name, seed in CASES:
        for i, pos in enumerate(H.golden(name, seed)["meshes"]):
            yield f"{name}{seed} mesh {i}", pos
    for which in H.SCALES:
        for seed in H.SEEDS:
            for i, pos in enumerate(H.scaled(which, seed)[0]):
                if i != 1:  # (mesh 1 is mesh 0 byte for byte)
                    yield f"{which}{seed} mesh {i}", pos
    big = H.golden("grid", 0)["meshes"][2]
    for n in (1, 2, 8, 9):
        yield f"the first {n} triangles of grid0 mesh 2", big[:3 * n]


def test_device_bvh_build_matches_host_builder_on_hostile_soups(tracer):
    count = 0
    for what, pos in build_cases():
        pos = np.ascontiguousarray(pos, dtype=F)
        idx = np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)
        nodes, remap, _ = tracer.build_bvh(idx, pos)
        ref_nodes, ref_remap = _host_bvh(idx, pos)
        _assert_same_tree(nodes, remap, ref_nodes, ref_remap, what)
        count += 1
    assert count == 4 * (3 + 3 + 2) + 2 * 4 * 2 + 4


# ----------------------------------------------------------------------------- 5. refit
BOX_WORDS = {"wnodes": slice(0, 12), "hot": slice(0, 12), "root_boxes": slice(0, 6)}


def degenerate(tris):
    """Slots (S,) of a (S, 9) corner array whose triangle has two equal corners (pad slots, all zeros, are not triangles)."""
    p = tris.reshape(-1, 3, 3)
    same = lambda a, b: (p[:, a] == p[:, b]).all(axis=1)  # noqa: E731
    return (same(0, 1) | same(0, 2) | same(1, 2)) & (tris != 0).any(axis=1)


def assert_same_state(rows, rows2, camera, what, expect_nan):
    """The device arrays of the context that was updated against those of the context that uploaded the updated scene, then images
    and event counts.  Returns the excepted-word counts per array."""
    got, want = rows.scene_arrays(), rows2.scene_arrays()
    assert got["tris"].tobytes() == want["tris"].tobytes(), what
    dead = degenerate(got["tris"])
    report = {}
    for k in ("wnodes", "hot", "shade", "bump", "root_boxes", "radius"):
        zero, nan = H.excepted_words(got[k], want[k], f"{what}: {k}")
        report[k] = (int(zero.sum()), int(nan.sum()))
        if got[k].size == 0:  # (no bump map in the scene)
            continue
        zero, nan = zero.reshape(got[k].shape), nan.reshape(got[k].shape)
        if k in BOX_WORDS:
            inside = np.zeros(zero.shape, dtype=bool)
            inside[:, BOX_WORDS[k]] = True
            assert not (zero & ~inside).any(), f"{what}: {k}: a zero of another sign outside the box floats"
        else:
            assert not zero.any(), f"{what}: {k}: {int(zero.sum())} zeros of another sign"
        if k in ("shade", "bump"):  # normals / tangents derived from positions: the first three floats of a record's float4s
            positional = np.zeros(nan.shape, dtype=bool)
            positional[:, [0, 1, 2] if k == "shade" else [0, 1, 2, 4, 5, 6]] = True
            assert not (nan & ~(positional & dead[:, None])).any(), f"{what}: {k}: a NaN pair outside a degenerate triangle's derived floats"
        else:
            assert not nan.any(), f"{what}: {k}: NaN pairs"
    print(f"{what}: excepted (zero, NaN) word pairs {report}; {int(dead.sum())} degenerate slots")
    if expect_nan:
        assert dead.any()
    rows.set_camera(camera)
    rows2.set_camera(camera)
    img = rows.render(8, count_traffic=True)
    ev = {k: rows.last_stats[k] for k in EVENTS}
    img2 = rows2.render(8, count_traffic=True)
    ev2 = {k: rows2.last_stats[k] for k in EVENTS}
    assert_bits_equal(img, img2, f"{what}: counting render")
    assert ev == ev2, (what, ev, ev2)
    assert ev["raysTraced"] > 64 * 64 * 8 and (img != 0).any(), what  # the camera sees the geometry
    assert_bits_equal(rows.render(8), rows2.render(8), f"{what}: render")
    return report


def test_refit_onto_the_grid_with_negative_zeros(rows, rows2):
    pairs = H.grid_positions(np.random.default_rng(1000))
    scene, camera, _ = H.product_scene([raw for raw, _ in pairs], light=LIGHT["grid"])
    rows.upload_scene(scene)
    old = rows.scene_arrays()
    for m, (_, snapped) in enumerate(pairs):
        assert np.signbit(snapped[snapped == 0]).any() or m == 0
        scene.update_positions(m, snapped)
    rows.update_meshes(scene)
    rows2.upload_scene(scene)
    assert rows.scene_arrays()["tris"].tobytes() != old["tris"].tobytes()
    assert_same_state(rows, rows2, camera, "grid refit", expect_nan=False)


def degenerate_scene():
    """A bump-mapped atrium with vertex normals and, inside it in front of the camera, a soup with face normals."""
    scene = prt_amd.Scene()
    m = prt_amd.Mesh.atrium(4000, 1, True, True, 0.05)
    m.calculate_vertex_normals()
    scene.add(m)
    rng = np.random.default_rng(1001)
    soup = (rng.uniform(-1.0, 1.0, (120, 1, 3)) + 0.3 * rng.normal(size=(120, 3, 3)) + np.array([-11.0, 4.3, 0.3])).astype(F)
    scene.add(H.soup_mesh(soup.reshape(-1, 3)))
    scene.set_directional_light(prt_amd._normalize((0.05, 1.0, 0.1)), (16.7, 15.6, 11.7))
    return scene, prt_amd.Camera().create((-15.0, 4.0, 0.5), (1.0, 0.08, -0.05), 64, 64), soup


def test_refit_with_degenerate_triangles(rows, rows2):
    scene, camera, soup = degenerate_scene()
    a = scene.arrays()["meshes"]
    assert (a[0]["materials"]["bumpMap"] >= 0).any() and a[0]["normals"] is not None and a[1]["normals"] is None
    rows.upload_scene(scene)
    rng = np.random.default_rng(1002)
    # the atrium is indexed: moving a corner onto another collapses the triangle (and bends its neighbours)
    P = a[0]["positions"].copy()
    picked = a[0]["indices"][rng.choice(len(a[0]["indices"]), 20, replace=False)]
    P[picked[:10, 1]] = P[picked[:10, 0]]
    P[picked[10:, 1]] = P[picked[10:, 0]]
    P[picked[10:, 2]] = P[picked[10:, 0]]
    S = soup.copy()
    S[:10, 2] = S[:10, 1]
    S[10:20, 1] = S[10:20, 0]
    S[10:20, 2] = S[10:20, 0]
    scene.update_positions(0, P)
    scene.update_positions(1, S.reshape(-1, 3))
    rows.update_meshes(scene)
    rows2.upload_scene(scene)
    assert_same_state(rows, rows2, camera, "degenerate triangles", expect_nan=True)
    got = rows.scene_arrays()
    dead = degenerate(got["tris"])
    assert dead.sum() >= 40
    # face normals and bump tangents of degenerate triangles are NaN (on both sides: a NaN against a number is no excepted pair)
    assert np.isnan(got["shade"][dead][:, :3]).any() and np.isnan(got["bump"][dead][:, [0, 1, 2, 4, 5, 6]]).any()
    assert not np.isnan(got["shade"][~dead]).any() and not np.isnan(got["bump"][~dead]).any()
    # for the record (profiles/r13_hostile_parity.txt): the words themselves, refit against upload
    want = rows2.scene_arrays()
    for k, cols in (("shade", [0, 1, 2]), ("bump", [0, 1, 2, 4, 5, 6])):
        a, b = H.words(got[k][:, cols]), H.words(want[k][:, cols])
        nan = np.isnan(got[k][:, cols])
        print(f"{k}: {int(nan.sum())} NaN words in {int(nan.any(axis=1).sum())} slots; bit patterns after the refit "
              f"{sorted(hex(int(w)) for w in np.unique(a[nan]))}, after the upload {sorted(hex(int(w)) for w in np.unique(b[nan]))}")


def test_refit_of_a_one_triangle_mesh_beside_another(rows, rows2):
    """The second mesh's root is a leaf: no wide record, no level launch, the root box straight from the triangle's corners."""
    g = H.golden("grid", 1)
    one = np.array([[-0.5, -0.5, 1.0], [0.75, -0.25, 1.0], [0.0, 0.5, 1.25]], dtype=F)
    scene, camera, _ = H.product_scene([g["meshes"][1], one], light=LIGHT["grid"])
    rows.upload_scene(scene)
    old = rows.scene_arrays()
    moved = (g["meshes"][1] * F(0.5)).astype(F)
    one2 = np.array([[-0.25, -0.5, 1.5], [0.5, -0.0, 1.5], [-0.0, 0.75, 1.25]], dtype=F)
    scene.update_positions(0, moved)
    scene.update_positions(1, one2)
    rows.update_meshes(scene, [1, 0])
    rows2.upload_scene(scene)
    assert_same_state(rows, rows2, camera, "one-triangle mesh", expect_nan=False)
    got = rows.scene_arrays()
    assert got["root_boxes"][1].tobytes() != old["root_boxes"][1].tobytes()
    assert np.array_equal(got["root_boxes"][1], np.concatenate([one2.min(axis=0), one2.max(axis=0)]))
