"""The cooperative leaf round (prt_device.h tracer_leaf_coop) at the edges of its bookkeeping: the prefix sums of the leaves' triangle
counts, the pair table, the takers' cut-off at 64 pairs, the axis permutations of the watertight test and the owners' update walk.

Every scene is made of meshes of k <= 8 triangles, each of which is one root leaf (asserted), up to 8 meshes standing 4 units apart
along x.  Every batch is exactly 64 rays: ray i is lane i of wave 0, and every lane finds its first root box in the refill turn, so all
64 lanes stand on a leaf in the same round -- the leaf of the mesh whose column the ray runs in, which is how a case chooses the leaf
size of each lane.  prt_hip_trace_rays in all four modes against the live oracle, bit for bit."""
import os

import numpy as np
import pytest

import prt_amd
import prt_hostile as H
import prt_testlib as T
from prt_gpukit import rows  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ((0, "single"), (1, "packet"), (2, "occluded_single"), (3, "occluded_packet"))
FAR = 1e5
PITCH = 4.0  # distance of the meshes' columns along x


def stack(m, k, rng):
    """k triangles over the column of mesh m: each covers the column's centre, at heights 0, -0.25, ... in a shuffled order (so the
    leaf's triangle order is not the order along a ray), every vertex a little off its plane (no box of zero extent)."""
    cx = PITCH * m
    z = -0.25 * rng.permutation(k)
    tri = np.zeros((k, 3, 3))
    tri[:, 0] = (cx - 1.0, -0.8, 0.0)
    tri[:, 1] = (cx + 1.0, -0.8, 0.0)
    tri[:, 2] = (cx, 1.2, 0.0)
    tri[:, :, 2] = z[:, None] + rng.uniform(-0.03, 0.03, size=(k, 3))
    return tri.astype(F)


def column_rays(which, rng, up=None, spread=0.2):
    """One ray per entry of `which` (the mesh a lane aims at): from above the column going down, or (up[i]) from below going up."""
    which = np.asarray(which)
    n = len(which)
    up = np.zeros(n, dtype=bool) if up is None else np.asarray(up, dtype=bool)
    org = np.zeros((n, 3))
    org[:, 0] = PITCH * which + rng.uniform(-spread, spread, n)
    org[:, 1] = rng.uniform(-spread, spread, n)
    org[:, 2] = np.where(up, -6.0, 4.0)
    d = np.zeros((n, 3))
    d[:, :2] = rng.uniform(-0.03, 0.03, size=(n, 2))
    d[:, 2] = np.where(up, 1.0, -1.0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return org.astype(F), d.astype(F)


def check(rows, scene, desc, org, d, what, leaves):
    """All four modes of the 64-ray batch against the oracle; `leaves` = the triangle counts of the meshes, each one root leaf."""
    assert len(org) == 64
    o = T.OracleScene(desc)
    for m, k in enumerate(leaves):
        nodes = o.nodes(m)
        assert len(nodes) == 1 and k <= 8, f"{what}: mesh {m} of {k} triangles is not one root leaf ({len(nodes)} nodes)"
    rows.upload_scene(scene)
    single, occ1 = o.intersect_single(org, d, FAR)
    packet, occ8 = o.intersect_packet(org, d, FAR)
    want = dict(single=single, packet=packet, occluded_single=occ1, occluded_packet=occ8)
    for mode, key in MODES:
        got = rows.trace_rays(mode, org, d, FAR)
        if mode < 2:
            if got.tobytes() != want[key].tobytes():
                bad = np.nonzero((got.view(np.uint8).reshape(64, -1) != want[key].view(np.uint8).reshape(64, -1)).any(axis=1))[0]
                raise AssertionError(f"{what}: mode {mode}, lanes {bad.tolist()} differ: {got[bad[0]]} against {want[key][bad[0]]}")
        else:
            assert (got["t"] == want[key]).all(), f"{what}: mode {mode}, lanes {np.nonzero(got['t'] != want[key])[0].tolist()} differ"
    assert rows.stats()["stackOverflow"] == 0
    return want


def soup_scene(meshes):
    scene, camera, desc = H.product_scene(meshes)
    return scene, desc


# lane -> mesh patterns; the meshes' triangle counts beside them
PATTERNS = {
    # 64 lanes x 1 triangle: 64 pairs, the table full to its last word, lane 63 an owner
    "exact_fill": ([1], [0] * 64),
    # 64 lanes x 8 triangles: eight lanes take per round, the other 56 wait (eight rounds)
    "overflow": ([8], [0] * 64),
    # 3, 5, 3, 5, ...: lane 15's leaf ends at pair 64 exactly and takes; lane 16 starts at 64 and waits
    "exact_fit": ([3, 5], [0, 1] * 32),
    # nine leaves of 7 = 63 pairs, then a leaf of 2 that would end at 65 and must not take -- nor may the leaves of 1 behind it,
    # which would fit: the takers are a prefix of the leaf lanes
    "cut_off": ([7, 2, 1], [0] * 9 + [1] * 5 + [2] * 50),
    # lane 0 on the scene's first triangle: table word 0 (triangle 0 - prefix 0, owner 0); the other lanes on every size 1..8
    "slot0": ([4, 1, 2, 3, 5, 6, 7, 8], [0] + [1 + (i * 5) % 7 for i in range(63)]),
}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_pair_table_at_its_edges(rows, name):
    leaves, which = PATTERNS[name]
    rng = np.random.default_rng(7000 + len(name))
    scene, desc = soup_scene([stack(m, k, rng) for m, k in enumerate(leaves)])
    # every other lane from below: the leaf's triangles arrive in the opposite order along the ray
    org, d = column_rays(which, rng, up=(np.arange(64) % 4 == 3))
    want = check(rows, scene, desc, org, d, name, leaves)
    assert (want["single"]["t"] != -1).all() and want["occluded_single"].all()  # every lane's leaf is hit
    assert (np.asarray(want["single"]["meshId"]) == np.asarray(which)).all()  # ... and it is the leaf of the lane's own column


def test_owner_updates_in_either_order(rows):
    """Two and more triangles of one leaf are hit at different t.  Going down the column a ray meets them in one order, going up in the
    other: with the leaf's (shuffled) triangle order fixed, the owner's walk over its accepted pairs updates at a later pair for some
    lanes and keeps an earlier one for others.  Both must occur, which the oracle's winners show: the nearest triangle is the first of
    the leaf for some lanes and a later one for others."""
    rng = np.random.default_rng(7100)
    leaves = [6, 2, 8]
    meshes = [stack(m, k, rng) for m, k in enumerate(leaves)]
    scene, desc = soup_scene(meshes)
    which = [(i * 7) % 3 for i in range(64)]
    org, d = column_rays(which, rng, up=(np.arange(64) % 2 == 1))
    want = check(rows, scene, desc, org, d, "updates", leaves)
    hit = want["single"]
    assert (hit["t"] != -1).all() and (np.asarray(hit["meshId"]) == np.asarray(which)).all()
    o = T.OracleScene(desc)
    # a hit names its triangle by the index in its mesh; prim_remap lists those indices in the leaf's order
    order = [o.prim_remap(m).tolist() for m in range(len(leaves))]
    slot = np.array([order[int(m)].index(int(p)) for m, p in zip(hit["meshId"], hit["primId"])])
    assert (slot == 0).any() and (slot > 0).any(), slot  # the first pair of a leaf stays the winner / a later pair replaces it


def test_axis_permutations_and_ties(rows):
    """One leaf of 8 triangles around the origin, rays from all around it: directions dominated by +x, -x, +y, -y, +z, -z in turn, and
    ties between two and three components of either sign.  The single-ray rule takes the largest SIGNED component with strict compares
    (ray.h:26-40), the packet rule the largest magnitude with x before y (ray.h:58-71): every one of the three permutations runs under
    both rules, and lanes of different permutations share a round."""
    rng = np.random.default_rng(7200)
    k = 8
    tri = (rng.normal(size=(k, 1, 3)) * 0.25 + rng.normal(size=(k, 3, 3)) * 0.9).astype(F)
    scene, desc = soup_scene([tri])
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    ties = [(1, 1, 0.3), (-1, -1, 0.3), (1, -1, 0.2), (1, 0.3, 1), (-1, 0.3, -1), (0.3, 1, 1), (0.3, -1, -1), (0.2, 1, -1),
            (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (0.5, 0.5, -0.5), (-0.25, 0.25, 0.25), (1, -1, -1)]
    d = np.zeros((64, 3))
    for i in range(48):
        d[i] = np.array(axes[i % 6], dtype=float) + rng.uniform(-0.35, 0.35, 3)
    for i in range(16):
        d[48 + i] = ties[i]  # exact ties: not normalised (a normalisation may round them apart)
    d[:48] /= np.linalg.norm(d[:48], axis=1, keepdims=True)
    d = d.astype(F)
    target = rng.uniform(-0.3, 0.3, size=(64, 3))
    org = (target - 3.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    # the three permutations under both rules, from the directions themselves
    a = np.abs(d)
    soa = np.where(a[:, 0] >= np.maximum(a[:, 1], a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    single = np.where(d[:, 0] > d[:, 1], np.where(d[:, 0] > d[:, 2], 0, 2), np.where(d[:, 1] > d[:, 2], 1, 2))
    assert set(soa) == {0, 1, 2} and set(single) == {0, 1, 2} and (soa != single).any()
    want = check(rows, scene, desc, org, d, "permutations", [k])
    assert (want["single"]["t"] != -1).sum() >= 16 and (want["packet"]["t"] != -1).sum() >= 16


def test_alpha_tested_leaf(rows, tmp_path):
    """One alpha-tested leaf of 8 triangles (an OBJ with a map_Kd whose alpha channel has holes, as in
    test_gpu_parity.py::test_alpha_cell_classes_at_the_threshold_bytes) beside a plain leaf of 3: candidates of the alpha leaf are
    accepted or rejected by the pair's lane before the owners read the ballot, so a ray passes through the holes of the nearer
    triangles and stops at the first opaque texel."""
    from prt_images import _png
    rng = np.random.default_rng(7300)
    td = str(tmp_path)
    vals = np.array([0, 126, 127, 128, 255], dtype=np.uint8)
    a = rng.integers(0, 256, size=(20, 28, 4)).astype(np.uint8)
    for by in range(0, 20, 4):
        for bx in range(0, 28, 4):
            a[by:by + 4, bx:bx + 4, 3] = vals[int(rng.integers(0, len(vals)))]
    _png(os.path.join(td, "mask.png"), a, level=6)
    with open(os.path.join(td, "m.mtl"), "w") as f:
        f.write("newmtl holes\nKd 0.9 0.9 0.9\nmap_Kd mask.png\n")
    k = 8
    tri = stack(0, k, rng)
    uv = rng.uniform(-1.5, 2.5, size=(k, 3, 2))
    with open(os.path.join(td, "s.obj"), "w") as f:
        f.write("mtllib m.mtl\n")
        for v in tri.reshape(-1, 3):
            f.write("v %.9g %.9g %.9g\n" % tuple(v))
        for v in uv.reshape(-1, 2):
            f.write("vt %.9g %.9g\n" % tuple(v))
        f.write("usemtl holes\n")
        for j in range(k):
            i = 3 * j + 1
            f.write(f"f {i}/{i} {i + 1}/{i + 1} {i + 2}/{i + 2}\n")
    mesh = prt_amd.Mesh.load_obj(os.path.join(td, "s.obj"))
    mesh.calculate_bounds()
    scene = prt_amd.Scene()
    scene.add(mesh)
    scene.add(H.soup_mesh(stack(1, 3, rng)))
    assert int(scene.arrays()["meshes"][0]["materials"]["alphaTest"].sum()) == 1
    camera = prt_amd.Camera().create((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), 64, 64)
    desc = T.scene_desc_from_product(scene, camera, 1.0)
    which = [0] * 6 + [1] + [0] * 50 + [1] * 7  # eight alpha leaves take in the first round, among them a plain one
    org, d = column_rays(which, rng, up=(np.arange(64) % 3 == 2), spread=0.45)
    want = check(rows, scene, desc, org, d, "alpha leaf", [k, 3])
    on_alpha = np.asarray(which) == 0
    t = want["single"]["t"][on_alpha]
    # holes and opaque texels both decide: some rays pass the whole stack, and the rays that stop do so at more than one triangle
    assert (t == -1).any() and len(np.unique(want["single"]["primId"][on_alpha][t != -1])) >= 3
