"""Ray queries on the MI355X (include/prt_hip.h "ray queries"; the CPU half is tests/test_query_cpu.py): prt_hip_query_nearest /
_any / _surface of the PRODUCT library against the compiled reference's stored answers (tests/golden/hostile_rays.npz,
hostile_taps.npz), the live oracle, and the test build's row-level entry points -- everything at tolerance 0."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_hostile as H
import prt_hostile_taps as HT
import prt_testlib as T
from prt_gpukit import same_records, snapped_scene
from prt_gpukit import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F = np.float32
CASES = [(name, seed) for name in H.SCENES for seed in H.SEEDS]
MISS_HIT = np.array([(-1.0, 0.0, 0.0, 0.0, 0, 0)], dtype=prt_amd.HIT_DTYPE)[0]


def miss_surface():
    s = np.zeros(1, dtype=prt_amd.SURFACE_DTYPE)
    s["t"] = -1.0
    return s[0]


# (differs from prt_gpukit.tracer: max_depth=8)
@pytest.fixture(scope="module")
def tracer():
    prt_amd.build()
    t = prt_amd.PathTracer(max_depth=8)
    yield t
    t.close()


def upload_hostile(tracer, name, seed):
    g = H.golden(name, seed)
    scene, camera, desc = H.product_scene(g["meshes"])
    tracer.upload_scene(scene)
    return g, scene, camera, desc


# ----------------------------------------------------------------------------- 1. the goldens
@pytest.mark.parametrize("name,seed", CASES)
def test_nearest_and_any_equal_the_compiled_reference(tracer, name, seed):
    g, _, _, _ = upload_hostile(tracer, name, seed)
    hits = tracer.query_nearest(g["org"], g["dir"], g["max_t"])
    same_records(hits, g["single"], f"{name}{seed} nearest")
    occ = tracer.query_any(g["org"], g["dir"], g["max_t"])
    assert occ.dtype == np.uint8 and (occ == g["occluded_single"]).all(), f"{name}{seed}: {int((occ != g['occluded_single']).sum())} flags differ"
    if name == "flat":
        assert (hits["t"] == -1).all()
    else:
        assert (hits["t"] != -1).any() and occ.any()


# ----------------------------------------------------------------------------- 2. a limit per ray
def test_every_ray_has_its_own_limit(tracer):
    g, _, _, desc = upload_hostile(tracer, "grid", 0)
    org, d = g["org"], g["dir"]
    t_max = np.where(np.arange(H.RAYS) % 2 == 0, F(4.0), F(1e5)).astype(F)
    hits = tracer.query_nearest(org, d, t_max)
    occ = tracer.query_any(org, d, t_max)
    o = T.OracleScene(desc)
    for first, limit in ((0, 4.0), (1, 1e5)):
        want, wocc = o.intersect_single(org[first::2], d[first::2], limit)
        same_records(hits[first::2], want, f"rays {first}::2 with tMax {limit}")
        assert (occ[first::2] == wocc).all()
    # and a limit that matters for every ray that hits: half of its own hit distance leaves nothing in reach, the float above it keeps the hit
    found = g["single"]["t"] != -1
    assert found.sum() > 100
    half = np.where(found, g["single"]["t"] * F(0.5), F(1e5)).astype(F)
    assert (tracer.query_nearest(org, d, half)["t"] == -1).all() and not tracer.query_any(org, d, half)[found].any()
    # one float above it, against the oracle ray by ray (the hit stays unless a box test that is strict at the limit drops it)
    above = np.where(found, np.nextafter(g["single"]["t"], F(np.inf)), F(1e5)).astype(F)
    want = np.concatenate([o.intersect_single(org[r:r + 1], d[r:r + 1], float(above[r]))[0] for r in range(H.RAYS)])
    got = tracer.query_nearest(org, d, above)
    same_records(got, want, "limits one float above the hit")
    print("hits kept one float above the hit:", int((got["t"] != -1).sum()), "of", int(found.sum()))
    assert (got["t"] != -1).sum() > found.sum() // 2


# ----------------------------------------------------------------------------- 3. batch shapes
@pytest.mark.parametrize("n", [1, 7, 63, 65, 1000])
def test_prefixes_give_the_prefix_of_the_full_answer(tracer, n):
    g, _, _, _ = upload_hostile(tracer, "grid", 0)
    same_records(tracer.query_nearest(g["org"][:n], g["dir"][:n], g["max_t"]), g["single"][:n], f"the first {n} rays")
    assert (tracer.query_any(g["org"][:n], g["dir"][:n], g["max_t"]) == g["occluded_single"][:n]).all()


def test_a_batch_larger_than_the_static_ranges():
    """2^20 rays: grid0's 1024 tiled 1024 times.  The grid is min(ceil(n / 1024), 2 workgroups per CU) = 512 workgroups on the
    MI355X's 256 CUs, i.e. 8192 waves; trace_loop gives every wave one static range of chunk = clamp(n / (4 * waves), 64, 1024) =
    clamp(32, ...) = 64 rays, which covers 8192 * 64 = 2^19 rays.  The other half of the batch lies beyond the static ranges and is
    only ever reached by a wave claiming a range from the shared cursor (the same holds for any device with fewer than 512 CUs:
    2048 rays of static range per CU)."""
    prt_amd.build()
    t = prt_amd.PathTracer()
    try:
        g, _, _, _ = upload_hostile(t, "grid", 0)
        assert t.device_info()[1] < 512
        k = 1024
        org, d = np.tile(g["org"], (k, 1)), np.tile(g["dir"], (k, 1))
        hits = t.query_nearest(org, d, g["max_t"])
        assert len(hits) == 1 << 20
        assert hits.tobytes() == np.tile(g["single"], k).tobytes()
        occ = t.query_any(org, d, g["max_t"])
        assert (occ.reshape(k, -1) == g["occluded_single"][None, :]).all()
        st = t.stats()
        assert st["raysTraced"] == 1 << 20 and st["occludedTraced"] == 1 << 20 and st["stackOverflow"] == 0
    finally:
        t.close()


# ----------------------------------------------------------------------------- 4. NaN rays
def test_nan_rays_are_misses_and_leave_their_neighbours_alone(tracer):
    g, _, _, _ = upload_hostile(tracer, "grid", 0)
    rays = prt_amd.make_rays(g["org"], g["dir"], g["max_t"])
    bad = np.arange(32) * 31 + 5
    w = rays.view(np.uint32).reshape(-1, 8)
    for k, r in enumerate(bad):
        w[r, (0, 1, 2, 4, 5, 6, 3)[k % 7]] = 0x7fc00000 if k % 2 else 0xffc12345  # org x y z, dir x y z, tMax
    assert np.isnan(rays["org"]).any() and np.isnan(rays["dir"]).any() and np.isnan(rays["tMax"]).sum() >= 4
    hits, surf = tracer.query_nearest(rays["org"], rays["dir"], rays["tMax"], surface=True)
    occ = tracer.query_any(rays["org"], rays["dir"], rays["tMax"])
    rest = np.ones(H.RAYS, bool)
    rest[bad] = False
    same_records(hits[bad], np.repeat(MISS_HIT, 32), "NaN rays")
    same_records(surf[bad], np.repeat(miss_surface(), 32), "NaN rays' surfaces")
    assert not occ[bad].any()
    same_records(hits[rest], g["single"][rest], "the other rays")
    assert (occ[rest] == g["occluded_single"][rest]).all()
    assert not np.isnan(hits["t"]).any() and not np.isnan(surf["t"]).any()


# ----------------------------------------------------------------------------- 5. the fused surface record
def sphere_rays(desc, n, seed):
    """n rays from a sphere around the scene's bounding box towards uniform points inside the box."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([m.positions for m in desc.meshes])
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    centre, radius = (lo + hi) / 2, 2.0 * np.linalg.norm(hi - lo) / 2
    u = rng.normal(size=(n, 3))
    org = (centre + radius * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
    target = rng.uniform(lo, hi, (n, 3)).astype(F)
    return org, (target - org).astype(F)


class TapsCase:
    pass


@pytest.fixture(scope="module")
def taps():
    """The scene of tests/golden/hostile_taps.npz in a product context and in a test-build context, 4096 rays, and the product's
    answers to them: computed once, shared by tests 5 to 8 and left unchanged."""
    prt_amd.build()
    c = TapsCase()
    c.z = HT.golden()
    c.desc = HT.golden_desc(c.z)
    c.t = prt_amd.PathTracer()
    c.rows = prt_amd.PathTracer(test_entry_points=True)
    c.keep = [HT.upload(c.t, c.desc), HT.upload(c.rows, c.desc)]
    c.org, c.dir = sphere_rays(c.desc, 4096, 17)
    c.hits, c.surf = c.t.query_nearest(c.org, c.dir, 1e5, surface=True)
    c.mat_base = np.concatenate([[0], np.cumsum([len(m.materials) for m in c.desc.meshes])]).astype(np.uint32)
    yield c
    c.t.close()
    c.rows.close()


def surface_words(surf):
    """(n, 9) uint32: normal, uv, meshMaterial, shadingNormal -- words [0..5] and [16..18] of the row-level surface entry."""
    return np.column_stack([surf["normal"].view(np.uint32), surf["uv"].view(np.uint32), surf["meshMaterial"], surf["shadingNormal"].view(np.uint32)])


ROW_WORDS = [0, 1, 2, 3, 4, 5, 16, 17, 18]


def test_fused_surface_records_equal_the_row_level_entries(taps):
    c = taps
    pinned = c.rows.trace_rays(0, c.org, c.dir, 1e5)  # the reference-pinned side alone
    hit = pinned["t"] != -1
    mats = [c.desc.meshes[m].materials[c.desc.meshes[m].prim_material[p]] for m, p in zip(pinned["meshId"][hit], pinned["primId"][hit])]
    print("hits", int(hit.sum()), "on bump-mapped materials", sum(int(m["bumpMap"] >= 0) for m in mats))
    assert hit.sum() >= 256 and any(m["bumpMap"] >= 0 for m in mats)
    same_records(c.hits, pinned, "query_nearest against the row-level trace")
    h, s, org, d = c.hits[hit], c.surf[hit], c.org[hit], c.dir[hit]
    assert s["t"].tobytes() == h["t"].tobytes() and (s["primId"] == h["primId"]).all() and (s["meshId"] == h["meshId"]).all() and not s["pad"].any()
    rec = np.column_stack([h["meshId"], h["primId"], h["i"].view(np.uint32), h["j"].view(np.uint32), h["k"].view(np.uint32)])
    want = c.rows.test_surface(rec)
    HT.words_equal_but_nan(surface_words(s), want[:, ROW_WORDS], "normal, uv, meshMaterial, shadingNormal")
    assert (s["material"] == c.mat_base[h["meshId"]] + s["meshMaterial"]).all()
    # diffuse: sampleDiffuse at uv where the material has its maps (the row-level taps entry needs both), the plain colour where it has none
    both = np.array([m["diffuseMap"] >= 0 and m["bumpMap"] >= 0 for m in mats])
    none = np.array([m["diffuseMap"] < 0 for m in mats])
    assert (both | none).all() and both.any() and none.any()
    taps_rec = np.column_stack([s["material"][both], s["uv"][both].view(np.uint32), np.ones(int(both.sum()), np.uint32)])
    HT.words_equal_but_nan(s["diffuse"][both], c.rows.test_taps(taps_rec)[:, 6:9], "diffuse through the maps")
    kd = np.array([m["diffuse"] for m, n in zip(mats, none) if n], dtype=F)
    assert s["diffuse"][none].tobytes() == kd.tobytes()
    P = (org + (h["t"][:, None] * d).astype(F)).astype(F)
    assert s["P"].tobytes() == P.tobytes()
    same_records(c.surf[~hit], np.repeat(miss_surface(), int((~hit).sum())), "misses")
    same_records(c.hits[~hit], np.repeat(MISS_HIT, int((~hit).sum())), "missed hits")


# ----------------------------------------------------------------------------- 6. the stand-alone surface fetch
def test_surface_of_the_goldens_records_equals_the_compiled_reference(taps):
    c = taps
    rec = c.z["surface"]
    hits = np.zeros(len(rec), dtype=prt_amd.HIT_DTYPE)
    hits["t"] = 1.0
    hits["meshId"], hits["primId"] = rec[:, 0], rec[:, 1]
    hits["i"], hits["j"], hits["k"] = rec[:, 2].view(F), rec[:, 3].view(F), rec[:, 4].view(F)
    org, d = np.zeros((len(rec), 3), F), np.tile(np.array([0, 0, 1], F), (len(rec), 1))
    surf = c.t.query_surface(org, d, hits)
    assert c.t.query_get_counts() == 0
    nan = HT.words_equal_but_nan(surface_words(surf), c.z["ref_surface"][:, ROW_WORDS], "surface records of the golden")
    print("NaN / NaN pairs with other bits:", nan)
    deg = HT.degenerate_mask(rec)
    assert not np.isnan(surface_words(surf)[~deg][:, [0, 1, 2, 3, 4, 6, 7, 8]].view(F)).any(), "a NaN outside the degenerate triangles"
    assert (surf["t"] == 1).all() and (surf["primId"] == rec[:, 1]).all() and (surf["meshId"] == rec[:, 0]).all()


def test_surface_of_the_products_own_hits_equals_the_fused_records(taps):
    c = taps
    same_records(c.t.query_surface(c.org, c.dir, c.hits), c.surf, "query_surface(hits) against the fused records")
    assert c.t.query_get_counts() == 0


# ----------------------------------------------------------------------------- 7. the range check
def test_indices_outside_the_scene_are_refused_on_the_device(taps):
    """No fault is provoked: a refused record reads nothing of the scene."""
    c = taps
    idx = np.nonzero(c.hits["t"] != -1)[0][:64]
    assert len(idx) == 64
    hits, want = c.hits[idx].copy(), c.surf[idx].copy()
    prims = np.array([m.prim_count for m in c.desc.meshes], dtype=np.uint32)
    bad = np.array([3, 10, 20, 30, 40, 50, 60, 63])
    hits["meshId"][3], hits["meshId"][40] = 8, len(prims)
    hits["meshId"][10], hits["meshId"][50] = 0xffffffff, 0x80000000
    hits["primId"][20], hits["primId"][60] = prims[hits["meshId"][20]], prims[hits["meshId"][60]]
    hits["primId"][30], hits["primId"][63] = 0xffffffff, 0x7fffffff
    got = c.t.query_surface(c.org[idx], c.dir[idx], hits)
    assert c.t.query_get_counts() == 8
    same_records(got[bad], np.repeat(miss_surface(), 8), "the refused records")
    want[bad] = miss_surface()
    same_records(got, want, "the 56 others")
    c.t.stats()  # no launch error


# ----------------------------------------------------------------------------- 8. device pointers, a caller's stream


def test_device_arrays_on_a_callers_stream(taps, dev):
    c = taps
    n = len(c.org)
    rays = prt_amd.make_rays(c.org, c.dir, 1e5)
    stream = dev.stream()
    d_rays, d_hits, d_surf = dev.alloc(rays.nbytes + 16), dev.alloc(n * 24), dev.alloc(n * 80)
    got_h, got_s = np.zeros(n, prt_amd.HIT_DTYPE), np.zeros(n, prt_amd.SURFACE_DTYPE)
    assert d_rays % 16 == 0 and d_surf % 16 == 0
    c.t.stats()
    with pytest.raises(prt_amd.PrtError, match="16-byte aligned"):
        c.t.query_nearest_async(n - 1, d_rays + 4, d_hits, None, stream)
    with pytest.raises(prt_amd.PrtError, match="16-byte aligned"):
        c.t.query_surface_async(n - 1, d_rays, d_hits, d_surf + 8, stream)
    assert c.t.stats()["kernelLaunches"] == 0  # refused before anything was launched
    dev.upload_async(rays, stream, d_rays)
    dev.fill_async(d_hits, 0xA5, n * 24, stream)
    dev.fill_async(d_surf, 0xA5, n * 80, stream)
    c.t.query_nearest_async(n, d_rays, d_hits, None, stream)
    c.t.query_surface_async(n, d_rays, d_hits, d_surf, stream)
    dev.synchronize(stream)
    assert got_h.nbytes == n * 24 and got_s.nbytes == n * 80
    dev.download(got_h, d_hits)
    dev.download(got_s, d_surf)
    same_records(got_h, c.hits, "hits through device pointers")
    same_records(got_s, c.surf, "surfaces through device pointers")
    st = c.t.stats()
    assert st["raysTraced"] == n and st["kernelLaunches"] == 1


# ----------------------------------------------------------------------------- 9. the scene's life cycle
def test_queries_follow_mesh_updates_and_new_uploads(tracer):
    g, scene, _, _ = upload_hostile(tracer, "grid", 0)
    org, d, max_t = g["org"], g["dir"], g["max_t"]
    hits0, surf0 = tracer.query_nearest(org, d, max_t, surface=True)
    same_records(tracer.query_surface(org, d, hits0), surf0, "before the update")  # (builds the inverse table)
    moved = (g["meshes"][1] + np.array([0.25, 0.0, 0.0], F)).astype(F)
    scene.update_positions(1, moved)
    tracer.update_meshes(scene, [1])
    hits1, surf1 = tracer.query_nearest(org, d, max_t, surface=True)
    other = prt_amd.PathTracer()
    try:
        other.upload_scene(scene)  # a second context that uploads the moved scene
        want_h, want_s = other.query_nearest(org, d, max_t, surface=True)
    finally:
        other.close()
    same_records(hits1, want_h, "after update_meshes")
    same_records(surf1, want_s, "surfaces after update_meshes")
    assert hits1.tobytes() != hits0.tobytes()
    same_records(tracer.query_surface(org, d, hits1), surf1, "query_surface after update_meshes")  # the table was kept: same primIds
    assert tracer.query_get_counts() == 0
    g2, _, _, _ = upload_hostile(tracer, "twins", 0)
    hits2, surf2 = tracer.query_nearest(g2["org"], g2["dir"], g2["max_t"], surface=True)
    same_records(hits2, g2["single"], "twins0 after a new upload")
    same_records(tracer.query_surface(g2["org"], g2["dir"], hits2), surf2, "query_surface after a new upload")  # the table was rebuilt
    assert tracer.query_get_counts() == 0


# ----------------------------------------------------------------------------- 10. pick


def test_pick_agrees_with_the_position_guide():
    """The centre, the four corners (background: the far quad ends at x = 2.5 where the image reaches 3.2), a pixel inside the near quad's
    outline and one that can only show the far quad."""
    prt_amd.build()
    desc = snapped_scene(HT.golden())
    t = prt_amd.PathTracer()
    try:
        keep = HT.upload(t, desc)
        t.set_camera(prt_amd.Camera().create(desc.cam_pos, desc.cam_dir, desc.width, desc.height))
        pos = t.denoise_position()
        shown = {}
        for x, y in ((32, 24), (0, 0), (63, 0), (0, 47), (63, 47), (40, 24), (52, 24)):
            hit, surf = t.pick(x, y)
            assert hit["t"].tobytes() == pos[y, x, 3].tobytes(), (x, y, hit, pos[y, x])
            assert surf["t"].tobytes() == hit["t"].tobytes()
            if hit["t"] == -1:
                assert hit.tobytes() == MISS_HIT.tobytes() and surf.tobytes() == miss_surface().tobytes()
                shown[x, y] = "background"
                continue
            assert surf["P"].tobytes() == pos[y, x, :3].tobytes()
            quad = 0 if abs(float(surf["P"][2])) < 1e-4 else 1
            assert abs(float(surf["P"][2]) + quad) < 1e-4 and hit["meshId"] == 0 and hit["primId"] in ((0, 1), (2, 3))[quad], (x, y, hit, surf)
            assert surf["meshMaterial"] == quad and surf["material"] == quad
            shown[x, y] = quad
        assert shown[52, 24] == 1  # x = 1.5 in the plane z = 0: outside the near quad's outline
        print("pick:", shown)
        assert shown[40, 24] in (0, 1)  # inside it: the near quad, or the far one through its mask
        assert all(shown[p] == "background" for p in ((0, 0), (63, 0), (0, 47), (63, 47)))
        del keep
    finally:
        t.close()


# ----------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    """No scene: PRT_HIP_ESTATE (a camera is not needed, a scene is); n = 0, n above 2^30 and unknown flag bits: PRT_HIP_EINVAL."""
    prt_amd.build()
    t = prt_amd.PathTracer()
    try:
        L, buf = t._L, np.zeros(4, prt_amd.SURFACE_DTYPE).ctypes.data_as(C.c_void_p)
        calls = (lambda n, f: L.prt_hip_query_nearest(t._ctx, n, buf, buf, None, f, None), lambda n, f: L.prt_hip_query_any(t._ctx, n, buf, buf, f, None),
                 lambda n, f: L.prt_hip_query_surface(t._ctx, n, buf, buf, buf, f, None))
        for call in calls:
            assert call(1, prt_amd.QUERY_HOST) == -5 and b"upload a scene" in L.prt_hip_last_error()
        upload_hostile(t, "grid", 0)  # no camera is ever set
        for call in calls:
            for n, flags in ((0, prt_amd.QUERY_HOST), ((1 << 30) + 1, prt_amd.QUERY_HOST), (1, prt_amd.QUERY_HOST | 2), (1, 0x80000000)):
                assert call(n, flags) == -2, (n, flags, L.prt_hip_last_error())
        assert t.stats()["kernelLaunches"] == 0 and t.query_get_counts() == 0
        g = H.golden("grid", 0)
        same_records(t.query_nearest(g["org"][:8], g["dir"][:8], g["max_t"]), g["single"][:8], "a query without a camera")
    finally:
        t.close()


# ----------------------------------------------------------------------------- 11. side effects
def test_a_query_changes_nothing_but_the_statistics(tracer):
    g, _, camera, _ = upload_hostile(tracer, "grid", 0)
    tracer.set_camera(camera)
    before = tracer.render(8, max_depth=8)
    tracer.accum_reset()
    tracer.accumulate(8)
    acc = tracer.accum_export()
    n = 100
    tracer.query_nearest(g["org"][:n], g["dir"][:n], g["max_t"])
    st = tracer.stats()
    assert st["raysTraced"] == n and st["occludedTraced"] == 0 and st["kernelLaunches"] == 1 and st["kernelMs"] > 0
    tracer.query_any(g["org"][:n], g["dir"][:n], g["max_t"])
    st = tracer.stats()
    assert st["raysTraced"] == n and st["occludedTraced"] == n and st["kernelLaunches"] == 1 and st["kernelMs"] > 0
    tracer.query_surface(g["org"][:n], g["dir"][:n], g["single"][:n])
    assert tracer.stats()["kernelLaunches"] == 0  # not a launch for the statistics
    after = tracer.accum_export()
    for k in ("rng", "sum", "count"):
        assert acc[k].tobytes() == after[k].tobytes(), k
    assert (after["seed"], after["max_depth"], after["rr_depth"]) == (acc["seed"], acc["max_depth"], acc["rr_depth"])
    assert tracer.render(8, max_depth=8).tobytes() == before.tobytes()
