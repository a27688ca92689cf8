"""Hostile rays and geometry without a GPU (tests/prt_hostile.py): the generators produce what they claim (NaN slab products, zero-extent
boxes, ties, -0.0), the compiled reference's answers in tests/golden/hostile_rays.npz show the behaviours the GPU suite pins
(tests/test_gpu_hostile.py), the oracle reproduces them byte for byte, and the host's refit takes -0.0 positions."""
import functools

import numpy as np
import pytest

import prt_amd
import prt_hostile as H
import prt_testlib as T
from prt_refit_ref import refit_nodes

CASES = [(name, seed) for name in H.SCENES for seed in H.SEEDS]
MIN_ON_PLANES = {"grid": 128, "flat": 128, "twins": 32}


@pytest.fixture(scope="module", autouse=True)
def built():
    prt_amd.build()


@functools.lru_cache(maxsize=None)
def oracle_case(name, seed):
    """(golden record, oracle scene, product scene) of one golden scene; built once."""
    g = H.golden(name, seed)
    scene, _, desc = H.product_scene(g["meshes"])
    return g, T.OracleScene(desc), scene


@pytest.mark.parametrize("name,seed", CASES)
def test_rays_meet_box_planes_with_a_zero_direction_component(name, seed):
    """The FAST = false select path only matters for a slab product 0 * inf: a zero direction component AND the origin on a box plane
    of that axis."""
    g, o, _ = oracle_case(name, seed)
    nodes = [o.nodes(i) for i in range(len(g["meshes"]))]
    n = H.rays_on_box_planes(nodes, g["org"], g["dir"])
    print(f"{name}{seed}: {n} rays with a NaN slab product")
    assert n >= MIN_ON_PLANES[name], (name, seed, n)
    assert ((g["dir"] == 0).sum(axis=1) < 3).all() and np.isfinite(g["org"]).all() and np.isfinite(g["dir"]).all()


@pytest.mark.parametrize("name,seed", CASES)
def test_reference_answers_show_the_edge_rules(name, seed):
    g = H.golden(name, seed)
    single, packet = g["single"]["t"] != -1, g["packet"]["t"] != -1
    assert len(single) == H.RAYS and (single != packet).any(), "strict against non-strict box compares must be visible"
    if name == "flat":  # a box of zero extent: min_t1 > max_t0 never holds, min_t1 >= max_t0 does
        assert not single.any() and not g["occluded_single"].any() and packet.any() and g["occluded_packet"].any()
    else:
        assert single.any() and packet.any()
    if name == "twins":  # coincident triangles of meshes 0, 1 (and 2): t < hit.t keeps the first mesh
        assert (g["single"]["meshId"][single] == 0).all() and (g["packet"]["meshId"][packet] == 0).all()
        pos = g["meshes"][0].reshape(-1, 3, 3)
        assert (pos[:10, 1] == pos[:10, 2]).all() and (pos[10:20, 0] == pos[10:20, 1]).all() and (pos[10:20, 0] == pos[10:20, 2]).all()
        assert g["meshes"][1].tobytes() == g["meshes"][0].tobytes() and g["meshes"][2].tobytes() == pos[50].tobytes()
    if name == "grid":
        allv = np.concatenate(g["meshes"])
        assert (allv * 4 == np.round(allv * 4)).all()
        zeros = np.signbit(allv[allv == 0])
        assert zeros.any() and not zeros.all()
    if name == "flat":
        a, b = g["meshes"]
        assert (a[:, 1] == 0).all() and np.signbit(a[:, 1]).all() and (b[:, 2] == 0.25).all()


@pytest.mark.parametrize("name,seed", CASES)
def test_oracle_equals_the_golden_reference_answers(name, seed):
    g, o, _ = oracle_case(name, seed)
    single, occ1 = o.intersect_single(g["org"], g["dir"], g["max_t"])
    packet, occ8 = o.intersect_packet(g["org"], g["dir"], g["max_t"])
    assert single.tobytes() == g["single"].tobytes(), (name, seed)
    assert packet.tobytes() == g["packet"].tobytes(), (name, seed)
    assert (occ1 == g["occluded_single"]).all() and (occ8 == g["occluded_packet"]).all(), (name, seed)


@pytest.mark.ref
@pytest.mark.parametrize("name,seed", CASES)
def test_generators_and_compiled_reference_reproduce_the_golden_file(name, seed):
    if T.ref_binary("ref_core") is None:
        pytest.skip("oracle/_ref/ref_core is only built where the reference's tree is present")
    g = H.golden(name, seed)
    meshes, org, d, max_t = H.generate(name, seed)
    assert len(meshes) == len(g["meshes"]) and all(a.tobytes() == b.tobytes() for a, b in zip(meshes, g["meshes"]))
    assert org.tobytes() == g["org"].tobytes() and d.tobytes() == g["dir"].tobytes() and np.float32(max_t) == np.float32(g["max_t"])
    _, _, desc = H.product_scene(meshes)
    single, occ1, packet, occ8 = T.ref_rays(desc, org, d, max_t)
    assert single.tobytes() == g["single"].tobytes() and packet.tobytes() == g["packet"].tobytes()
    assert (occ1 == g["occluded_single"]).all() and (occ8 == g["occluded_packet"]).all()


def test_golden_file_holds_arrays_only_and_stays_small():
    import os
    z = np.load(H.GOLDEN_FILE, allow_pickle=False)
    assert all(z[k].dtype.kind in "fu" for k in z.files)
    assert os.path.getsize(H.GOLDEN_FILE) <= os.path.getsize(os.path.join(T.GOLDEN, "c5_tile_rows.npz"))


def test_negative_zero_reaches_the_host_builders_nodes():
    """include/prt_hip.h: the builders agree "except for the sign of a zero".  On the grid scenes that exception is entered: the host
    builder's nodes differ from the oracle's in bytes for at least one mesh, while being equal as floats in the boxes and byte-equal
    in everything else."""
    differing = 0
    for seed in H.SEEDS:
        g, o, scene = oracle_case("grid", seed)
        for i, m in enumerate(scene.arrays()["meshes"]):
            want, remap = o.nodes(i), o.prim_remap(i)
            got = m["nodes"]
            assert len(got) == len(want), (seed, i)
            for f in ("primOrSecondNodeIndex", "triVectorIndex", "primCount", "splitAxis"):
                assert got[f].tobytes() == want[f].tobytes(), (seed, i, f)
            assert (m["remap"] == remap).all(), (seed, i)
            assert np.array_equal(got["lower"], want["lower"]) and np.array_equal(got["upper"], want["upper"]), (seed, i)
            n = H.words_equal(got, want, f"grid{seed} mesh {i}")  # and so only zeros of another sign
            assert (n > 0) == (got.tobytes() != want.tobytes())
            differing += n > 0
            print(f"grid{seed} mesh {i}: {n} box words differ in the sign of a zero")
    assert differing >= 1


def test_word_comparison_excepts_zero_and_nan_pairs_only():
    a = np.array([0.0, -0.0, np.nan, 1.0, 2.0], np.float32)
    b = np.array([-0.0, -0.0, -np.nan, 1.0, 2.0], np.float32)
    b.view(np.uint32)[2] = 0xffc00000
    a.view(np.uint32)[2] = 0x7fc00000
    zero, nan = H.excepted_words(a, b)
    assert zero.tolist() == [True, False, False, False, False] and nan.tolist() == [False, False, True, False, False]
    assert H.words_equal(a, b) == 2 and H.words_equal(a, a) == 0
    for other in (np.array([0.0, -0.0, 0.0, 1.0, 2.0], np.float32), np.array([0.0, -0.0, np.nan, 1.0, np.nextafter(np.float32(2), np.float32(3))], np.float32),
                  np.array([np.float32(1e-45), -0.0, np.nan, 1.0, 2.0], np.float32)):
        with pytest.raises(AssertionError):
            H.words_equal(a, other)


@pytest.mark.parametrize("seed", H.SEEDS)
def test_host_refit_on_snapped_positions_is_the_numpy_refit(seed):
    """Scene.update_positions of the 300-triangle grid mesh, built from the unsnapped soup and moved onto the grid with -0.0 zeros:
    the refit rule of tests/prt_refit_ref.py, up to the sign of a zero."""
    pairs = H.grid_positions(np.random.default_rng(1000 + seed))
    scene, _, _ = H.product_scene([raw for raw, _ in pairs])
    before = scene.arrays()["meshes"]
    raw, snapped = pairs[2]
    assert np.signbit(snapped[snapped == 0]).any()
    scene.update_positions(2, snapped)
    after = scene.arrays()["meshes"]
    got = after[2]
    assert got["positions"].tobytes() == snapped.tobytes()
    assert (got["remap"] == before[2]["remap"]).all()
    want = refit_nodes(before[2]["nodes"], before[2]["remap"], before[2]["indices"], snapped)
    n = H.words_equal(got["nodes"], want, f"grid{seed}: refitted nodes")
    print(f"grid{seed}: host refit against numpy, {n} zero words of another sign")
    assert got["nodes"].tobytes() != before[2]["nodes"].tobytes()
    for other in (0, 1):
        assert after[other]["nodes"].tobytes() == before[other]["nodes"].tobytes()
