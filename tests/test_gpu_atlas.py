"""Lightmap atlases on the MI355X (include/prt_hip.h "lightmap atlases"; the CPU half is tests/test_atlas_cpu.py): prt_hip_atlas_rasterize,
prt_hip_atlas_points and prt_hip_atlas_resolve of the PRODUCT library against the numpy restatement tests/prt_atlas_ref.py, and
PathTracer.lightmap against the four calls composed by the test and against the restatement around the merged bake.  Everything at
tolerance 0, compared as bytes (a NaN of the restatement asks for a NaN: prt_bake_ref.same_bytes), with sentinel words behind every
output."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_atlas_ref as AR
import prt_bake_ref as BR
import prt_hostile_shade as HS
import prt_testlib as T
from prt_gpukit import SENTINEL, TAIL, fetch, ptr, sentinel, stage_tracers
from prt_gpukit import dev  # noqa: F401  (fixture: device memory and streams for one test)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
DEPTH = 8
HOST = prt_amd.QUERY_HOST
BLOCKS_PER_CU = 8       # PRT_ATLAS_BLOCKS_PER_CU (prt_atlas.hip): four waves a block, one triangle a wave


# (differs from prt_refit_ref.teapot_scene: 8 x 8, and the Scene alone)
def teapot_scene():
    """The Cornell box (no vertex normals) and the teapot of tests/golden/teapot_mesh.npz with computed vertex normals."""
    return prt_amd.setup_cornell_box(8, 8, teapot_mesh=T.teapot_product_mesh())[0]


SCENES = {"plain": lambda: HS.scene("plain")[0], "box_rr": lambda: HS.scene("box_rr")[0], "teapot": teapot_scene}
tracers = stage_tracers(SCENES, arrays=True, max_depth=DEPTH)  # tracers(name) -> (context, the scene's mesh arrays)


def grid_uvs(prims, inset=0.1):
    """(prims, 3, 2) float32: triangle p in a cell of its own of a G x G grid, as a lightmapper without chart packing would lay it."""
    G = int(np.ceil(np.sqrt(prims)))
    p = np.arange(prims)
    cx, cy = (p % G).astype(np.float64), (p // G).astype(np.float64)
    corner = np.array([(inset, inset), (1 - inset, inset), (inset, 1 - inset)])
    return ((np.stack([cx, cy], axis=1)[:, None, :] + corner[None]) / G).astype(F)


# ----------------------------------------------------------------------------- 1. the rasteriser
def run_rasterize(t, dev, meshes, W, H, device, order=None):
    """prt_hip_atlas_rasterize of {meshId: uv} on host or device arrays: (counts dict, texels and hits, each followed by sentinel
    words).  order: the meshIds in the order of the caller's records."""
    order = sorted(meshes) if order is None else order
    uvs = {m: np.ascontiguousarray(meshes[m], dtype=F).reshape(-1, 3, 2) for m in order}
    texels, hits, counts = sentinel(W * H + TAIL), sentinel(W * H * 6 + TAIL), prt_amd.AtlasCounts()
    if not device:
        recs = (prt_amd.AtlasMesh * len(order))(*[prt_amd.AtlasMesh(meshId=m, primCount=len(uvs[m]), uv=uvs[m].ctypes.data) for m in order])
        rc = t._L.prt_hip_atlas_rasterize(t._ctx, W, H, len(order), recs, ptr(texels), ptr(hits), C.byref(counts), HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return counts.as_dict(), texels, hits
    d_uvs, d_texels, d_hits = [dev.upload(uvs[m]) for m in order], dev.upload(texels), dev.upload(hits)
    recs = (prt_amd.AtlasMesh * len(order))(*[prt_amd.AtlasMesh(meshId=m, primCount=len(uvs[m]), uv=d) for m, d in zip(order, d_uvs)])
    rc = t._L.prt_hip_atlas_rasterize(t._ctx, W, H, len(order), recs, d_texels, d_hits, C.byref(counts), 0, None)
    assert rc == 0, t._L.prt_hip_last_error()
    return counts.as_dict(), fetch(dev, d_texels, texels.size), fetch(dev, d_hits, hits.size)


def check_rasterize(got, meshes, W, H, what):
    counts, texels, hits = got
    want_t, want_h, want_c = AR.rasterize(meshes, W, H)
    print(f"{what}: {want_c}")
    assert counts == want_c, (what, counts, want_c)
    n = want_c["n"]
    assert texels[:n].tobytes() == want_t.tobytes(), f"{what}: texels"
    BR.same_bytes(hits[:6 * n], want_h, f"{what}: hits")
    assert (texels[n:] == SENTINEL).all() and (hits[6 * n:] == SENTINEL).all(), f"{what}: entries at and beyond n were written"
    return want_t, want_h, want_c


def soup():
    """{0: ..., 5: ...} for a 64 x 48 atlas: every case of the issue's list.  fx = u * 16384, fy = v * 12288."""
    nan, inf = np.nan, np.inf
    limit = F(8388608.0) / F(16384.0)  # u = 512: fabsf(fx) exactly 2^23
    over = np.nextafter(limit, F(inf))
    shared = [(0.55, 0.55), (0.8, 0.6), (0.6, 0.9)]
    m0 = [
        [(0, 0), (0.5, 0), (0.5, 0.5)], [(0, 0), (0.5, 0.5), (0, 0.5)],       # the split square: prims 0 and 1
        [(0.1, 0.55), (0.45, 0.6), (0.2, 0.95)], [(0.15, 0.5), (0.5, 0.7), (0.1, 0.9)],  # two that overlap: the lower primId owns
        shared,                                                                # the same triangle in both meshes: meshId decides
        [(0.3, 0.1), (0.3 + 40 / 64, 0.1), (0.3, 0.1 + 40 / 48)],             # a 40 x 40 texel box: 25 lane trips
        [(-0.2, 0.5), (0.2, 0.6), (-0.1, 1.3)], [(0.9, -0.3), (1.4, 0.2), (0.95, 0.4)],  # partly outside [0, 1]
        [(1.2, 1.2), (1.5, 1.2), (1.2, 1.6)], [(-0.5, -0.5), (-0.1, -0.4), (-0.3, -0.05)],  # wholly outside
        [(0.6, 0.05), (0.62, 0.4), (0.95, 0.08)],                              # negative area
        [(0.01, 0.261), (0.99, 0.29), (0.99, 0.3)], [(0.7, 0.01), (0.705, 0.99), (0.71, 0.99)],  # slivers
        [(0, 0), (0.5, 0.5), (1, 1)], [(0.25, 0.25), (0.25, 0.25), (0.25, 0.25)], [(0.3, 0.3), (0.3, 0.3), (0.7, 0.1)],  # A == 0
        [(nan, 0), (1, 0), (1, 1)], [(0, 0), (1, nan), (1, 1)], [(0, 0), (inf, 0), (1, 1)], [(0, -inf), (1, 0), (1, 1)],
        [(0, 0), (1, 0), (1e9, 1)], [(0, 0), (1, -1e9), (1, 1)],               # rejected
        [(0.6, 0.5), (limit, 0.5), (0.6, 0.7)], [(0.2, 0.3), (-limit, 0.35), (0.2, 0.45)],  # a corner at exactly 2^23: accepted
        [(0.6, 0.5), (over, 0.5), (0.6, 0.7)], [(0.2, 0.3), (-over, 0.35), (0.2, 0.45)],    # the next float up: rejected
    ]
    m5 = [shared, [(0.85, 0.85), (0.99, 0.85), (0.85, 0.99)], [(0.0, 0.0), (0.3, 0.0), (0.0, 0.3)]]  # (the last lies under mesh 0's square)
    return {0: np.array(m0, F), 5: np.array(m5, F)}


def test_the_soup_equals_the_restatement(tracers, dev):
    t, _ = tracers("none")  # prt_hip_atlas_rasterize needs no scene
    meshes, W, H = soup(), 64, 48
    host = run_rasterize(t, dev, meshes, W, H, device=False, order=[5, 0])  # (the lower key later in memory)
    texels, hits, counts = check_rasterize(host, meshes, W, H, "the soup, host arrays")
    assert counts["rejected"] == 8 and counts["degenerate"] == 3 and counts["pairs"] > counts["n"] > 1024
    owner = {int(tx): (int(m), int(p)) for tx, m, p in zip(texels, hits["meshId"], hits["primId"])}
    assert owner[36 * 64 + 42] == (0, 4), "the triangle both meshes hold belongs to the lower meshId"
    assert owner[2 * 64 + 4] == (0, 0) and owner[2 * 64 + 2] == (0, 1) and owner[41 * 64 + 55] == (5, 1)
    assert set(p for m, p in owner.values() if m == 0) == {0, 1, 2, 3, 4, 5, 6, 7, 10, 22}, "the triangles that cover a centre no lower key covers"
    on_device = run_rasterize(t, dev, meshes, W, H, device=True, order=[5, 0])
    for a, b, name in zip(host, on_device, ("counts", "texels", "hits")):
        assert a == b if name == "counts" else a.tobytes() == b.tobytes(), f"device and host pointers give different {name}"
    again = run_rasterize(t, dev, meshes, W, H, device=True, order=[0, 5])
    assert again[0] == on_device[0] and again[1].tobytes() == on_device[1].tobytes() and again[2].tobytes() == on_device[2].tobytes(), "a second run differs"
    swapped = run_rasterize(t, dev, meshes, H, W, device=False)
    check_rasterize(swapped, meshes, H, W, "the soup in a 48 x 64 atlas")


@pytest.mark.parametrize("W,H", [(1, 1), (8192, 1), (1, 8192)])
def test_the_smallest_and_the_widest_atlas(tracers, dev, W, H):
    t, _ = tracers("none")
    meshes = {2: np.array([[(0, 0), (1, 0), (0, 1)], [(0.25, 0.0), (0.75, 0.0), (0.5, 1.0)], [(0.9, 0.2), (0.95, 0.9), (0.2, 0.95)]], F)}
    _, _, counts = check_rasterize(run_rasterize(t, dev, meshes, W, H, device=False), meshes, W, H, f"{W} x {H}")
    assert counts["n"] == 1 if W * H == 1 else counts["n"] > 4096


def test_a_fan_beyond_one_trip_of_the_persistent_grid(tracers, dev):
    t, _ = tracers("none")
    prims = 20000
    assert prims > t.device_info()[1] * BLOCKS_PER_CU * 4 + 256
    a = np.linspace(0.0, 2 * np.pi, prims + 1)
    rim = 0.5 + 0.45 * np.stack([np.cos(a), np.sin(a)], axis=1)
    fan = np.stack([np.broadcast_to([0.5, 0.5], (prims, 2)), rim[:-1], rim[1:]], axis=1).astype(F)
    meshes, W, H = {1: fan}, 64, 64
    _, hits, counts = check_rasterize(run_rasterize(t, dev, meshes, W, H, device=False), meshes, W, H, "the fan")
    assert counts["n"] > 2000 and len(np.unique(hits["primId"])) > 1500


# ----------------------------------------------------------------------------- 2. points
def scene_atlas(t, arrays, W, H):
    """The scene's meshes rasterised in a per-triangle grid layout (each mesh in a quadrant of its own): texels, hits."""
    uvs = {}
    for m, mesh in enumerate(arrays):
        uv = grid_uvs(len(mesh["indices"])) * F(0.5)
        uv[:, :, 0] += F(0.5) * (m % 2)
        uv[:, :, 1] += F(0.5) * (m // 2)
        uvs[m] = uv
    texels, hits, counts = t.atlas_rasterize(uvs, W, H)
    assert counts["n"] == len(texels) > 0 and counts["rejected"] == 0
    return uvs, texels, hits


def run_points(t, dev, texels, hits, W, bias, tile, device=False, flags=HOST, n=None, reserved=(0, 0), out=None):
    """prt_hip_atlas_points itself: (code, the points as words followed by sentinel words)."""
    n = len(hits) if n is None else n
    out = sentinel(len(hits) * 8 + TAIL) if out is None else out
    p = prt_amd.AtlasPointParams(bias=bias, setTile=tile)
    p.reserved[0], p.reserved[1] = reserved
    if not device:
        return t._L.prt_hip_atlas_points(t._ctx, n, W, ptr(texels), ptr(hits), C.byref(p), ptr(out), flags, None), out
    d_texels, d_hits, d_out = (dev.upload(a) for a in (texels, hits, out))
    rc = t._L.prt_hip_atlas_points(t._ctx, n, W, d_texels, d_hits, C.byref(p), d_out, 0, None)
    return rc, fetch(dev, d_out, out.size)


def surface_normals(t, hits):
    """normal of prt_hip_query_surface for the same hits (their t = 0 is neither -1 nor NaN: the record is fetched)."""
    z = np.zeros((len(hits), 3), F)
    return t.query_surface(z, z, hits)["normal"]


def check_points(t, dev, arrays, texels, hits, W, bias, tile, what, device=False):
    want = AR.points(texels, hits, W, [(m["indices"], m["positions"]) for m in arrays], surface_normals(t, hits), bias, tile)
    rc, got = run_points(t, dev, texels, hits, W, bias, tile, device=device)
    assert rc == 0, t._L.prt_hip_last_error()
    words = 8 * len(hits)
    g = got[:words].view(AR.POINT_DTYPE)
    assert g["N"].tobytes() == want["N"].tobytes(), f"{what}: N is not query_surface's normal word for word"
    assert g["set"].tobytes() == want["set"].tobytes(), f"{what}: set"
    BR.same_bytes(got[:words], want, what)
    assert (got[words:] == SENTINEL).all(), f"{what}: words behind the points were written"
    return want


@pytest.mark.parametrize("tile", [1, 4, 32])
@pytest.mark.parametrize("name", ["plain", "box_rr", "teapot"])
def test_points_equal_the_restatement(tracers, dev, name, tile):
    t, arrays = tracers(name)
    W, H = (160, 144) if name == "teapot" else (45, 37)
    _, texels, hits = scene_atlas(t, arrays, W, H)
    want = check_points(t, dev, arrays, texels, hits, W, F(1e-3), tile, f"{name} setTile={tile}", device=(tile == 4))
    assert (want["set"] != AR.NEVER).all() and want["set"].max() == (tile * tile - 1 if tile < 32 else want["set"].max())
    assert len(np.unique(hits["meshId"])) == len(arrays), "every mesh of the scene owns texels"
    if name == "teapot":  # interpolated vertex normals beside face normals
        pot = want["N"][hits["meshId"] == 1]
        assert len(np.unique(pot, axis=0)) > len(pot) // 2
    print(f"{name}: {len(hits)} points, sets up to {want['set'].max()}")


def test_hits_outside_the_scene_give_the_point_never_followed(tracers, dev):
    t, arrays = tracers("plain")
    pot_t, pot_arrays = tracers("teapot")
    W, H = 160, 144
    _, texels, hits = scene_atlas(pot_t, pot_arrays, W, H)  # hits of ANOTHER scene: most primIds lie beyond the stage's meshes
    prims = [len(m["indices"]) for m in arrays]
    bad = np.zeros(8, AR.HIT_DTYPE)
    bad["i"] = 1.0
    bad["meshId"] = [len(arrays), 7, 8, 0xffffffff, 0, 1, 0, 1]
    bad["primId"] = [0, 0, 0, 0, prims[0], prims[1], 0xffffffff, 0x80000000]
    hits = np.concatenate([bad, hits])
    texels = np.concatenate([np.arange(8, dtype=U), texels])
    want = check_points(t, dev, arrays, texels, hits, W, F(0.5), 4, "hits of another scene")
    never = want["set"] == AR.NEVER
    assert never[:8].all() and never.sum() > len(hits) // 2 and (~never).sum() > 8
    assert not want[never]["P"].any() and not want[never]["N"].any() and not want[never]["bias"].any()


def test_the_same_hits_follow_a_moved_mesh(dev):
    prt_amd.build()
    scene = HS.scene("plain")[0]
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        t.upload_scene(scene)
        arrays = scene.arrays()["meshes"]
        _, texels, hits = scene_atlas(t, arrays, 45, 37)
        first = check_points(t, dev, arrays, texels, hits, 45, F(0), 1, "before the move")
        for m, shift in ((0, (0.4, 0.0, 0.3)), (1, (-0.1, 0.2, 0.0))):
            scene.update_positions(m, (arrays[m]["positions"] * F(1.25) + np.array(shift, F)).astype(F))
        t.update_meshes(scene, [0, 1])
        moved = scene.arrays()["meshes"]
        second = check_points(t, dev, moved, texels, hits, 45, F(0), 1, "after update_meshes")
        assert (second["P"] != first["P"]).any(axis=1).all()
    finally:
        t.close()


# ----------------------------------------------------------------------------- 3. resolve
RW, RH = 37, 23


def islands(seed=5):
    """Texel indices of a 37 x 23 image: two islands, one with a hole, single texels, texels on every border and in a corner."""
    rng = np.random.default_rng(seed)
    m = np.zeros((RH, RW), bool)
    m[4:11, 5:14] = True
    m[6:9, 8:11] = False   # a hole
    m[14:19, 22:30] = rng.random((5, 8)) < 0.7
    m[0, 3], m[RH - 1, 17], m[11, 0], m[12, RW - 1], m[0, 0], m[RH - 1, RW - 1] = (True,) * 6
    m[2, 30], m[20, 4] = True, True
    t = np.nonzero(m.reshape(-1))[0].astype(U)
    return rng.permutation(t)


def resolve_values(n, stride, seed=6):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, stride)).astype(F)
    v[rng.random((n, stride)) < 0.05] = -0.0
    v[rng.random((n, stride)) < 0.03] = 1e-40
    v[3, 0], v[7, stride - 1], v[11, 0], v[12, 0] = np.nan, np.inf, -np.inf, 3e38
    v[13, 0] = 3e38  # (two of them next to each other overflow in a sum)
    return v


def run_resolve(t, dev, texels, values, W, H, stride, gutter, device=False, with_mask=True, flags=HOST, n=None, image=None, mask=None):
    n = len(texels) if n is None else n
    image = sentinel(W * H * stride + TAIL) if image is None else image
    mask = np.full(W * H + TAIL, 0xab, np.uint8) if mask is None else mask
    if not device:
        rc = t._L.prt_hip_atlas_resolve(t._ctx, W, H, n, ptr(texels), ptr(values), stride, gutter, ptr(image), ptr(mask) if with_mask else None, flags, None)
        return rc, image, mask
    d_texels, d_values, d_image, d_mask = (dev.upload(a) for a in (texels, values, image, mask))
    rc = t._L.prt_hip_atlas_resolve(t._ctx, W, H, n, d_texels, d_values, stride, gutter, d_image, d_mask if with_mask else None, 0, None)
    return rc, fetch(dev, d_image, image.size), fetch(dev, d_mask, mask.size, np.uint8)


@pytest.mark.parametrize("gutter", [0, 1, 3, 64])
@pytest.mark.parametrize("stride", [1, 3, 48])
def test_resolve_equals_the_restatement(tracers, dev, stride, gutter):
    t, _ = tracers("none")  # prt_hip_atlas_resolve needs no scene
    inside = islands()
    texels = np.concatenate([inside[:20], np.array([RW * RH, 0xffffffff], U), inside[20:]])  # two indices outside the image: ignored
    values = resolve_values(len(texels), stride)
    want_i, want_m = AR.resolve(texels, values, RW, RH, gutter)
    rc, image, mask = run_resolve(t, dev, texels, values, RW, RH, stride, gutter)
    assert rc == 0, t._L.prt_hip_last_error()
    words = RW * RH * stride
    nans = BR.same_bytes(image[:words], want_i, f"stride={stride} gutter={gutter}")
    assert mask[:RW * RH].tobytes() == want_m.tobytes() and (image[words:] == SENTINEL).all() and (mask[RW * RH:] == 0xab).all()
    assert nans >= (1 if gutter == 0 else 3)
    assert want_m.all() if gutter == 64 else int(want_m.max()) == gutter + 1, "64 passes fill the image, fewer leave texels empty"
    rc, dev_i, dev_m = run_resolve(t, dev, texels, values, RW, RH, stride, gutter, device=True)
    assert rc == 0 and dev_i.tobytes() == image.tobytes() and dev_m.tobytes() == mask.tobytes(), "device and host pointers give different bytes"
    for device in (False, True):  # mask = NULL
        rc, no_mask_i, untouched = run_resolve(t, dev, texels, values, RW, RH, stride, gutter, device=device, with_mask=False)
        assert rc == 0 and no_mask_i.tobytes() == image.tobytes() and (untouched == 0xab).all()


# ----------------------------------------------------------------------------- 4. end to end
def test_lightmap_equals_the_four_calls_and_the_restatement(tracers):
    t, arrays = tracers("box_rr")
    W, H, K, spp, seed, tile, gutter, bias = 40, 36, 16, 8, 4242, 2, 3, 1e-3
    uvs = {0: grid_uvs(len(arrays[0]["indices"]))}
    rng = np.random.default_rng(9)
    sets = [prt_amd.bake_cosine_set(K, rng) for _ in range(tile * tile)]
    dirs, weights = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    image, mask = t.lightmap(uvs, W, H, dirs, weights, spp, seed=seed, bias=bias, set_tile=tile, gutter=gutter)
    stats = t.last_stats
    assert image.shape == (H, W, 1, 3) and mask.shape == (H, W) and image.dtype == F and mask.dtype == np.uint8
    # the four calls composed here, on host arrays
    texels, hits, counts = t.atlas_rasterize(uvs, W, H)
    assert counts == t.last_atlas_counts and counts["n"] == len(texels) > 300
    pts = t.atlas_points(texels, hits, W, bias=bias, set_tile=tile)
    baked = t.bake(pts["P"], pts["N"], dirs, weights, spp, bias=pts["bias"], sets=pts["set"], seed=seed)
    assert (stats["nPx"], stats["raysTraced"]) == (t.last_stats["nPx"], t.last_stats["raysTraced"]) and stats["nPx"] == len(texels) * K
    composed_i, composed_m = t.atlas_resolve(texels, baked, W, H, gutter=gutter)
    assert composed_i.shape == image.shape
    BR.same_bytes(image, composed_i, "lightmap() against the four calls")
    assert mask.tobytes() == composed_m.tobytes()
    # the restatement around the merged bake
    r_texels, r_hits, _ = AR.rasterize(uvs, W, H)
    r_pts = AR.points(r_texels, r_hits, W, [(m["indices"], m["positions"]) for m in arrays], surface_normals(t, r_hits), bias, tile)
    r_baked = t.bake(r_pts["P"], r_pts["N"], dirs, weights, spp, bias=r_pts["bias"], sets=r_pts["set"], seed=seed)
    r_image, r_mask = AR.resolve(r_texels, r_baked.reshape(len(r_texels), -1), W, H, gutter)
    BR.same_bytes(image, r_image, "lightmap() against the restatement")
    assert mask.tobytes() == r_mask.tobytes()
    lit = int((image.reshape(H * W, 3)[mask.reshape(-1) == 1] != 0).any(axis=1).sum())
    print(f"lightmap of box_rr: {len(texels)} texels, {lit} lit, {int((mask > 1).sum())} gutter texels")
    assert lit > len(texels) // 4 and (mask > 1).sum() > 100 and r_pts["set"].max() == tile * tile - 1


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_queue_nothing_and_leave_the_outputs_untouched(tracers, dev):
    t, arrays = tracers("plain")
    bare, _ = tracers("none")
    L = t._L
    W, H = 16, 8
    uv = grid_uvs(4)
    texels_out, hits_out = sentinel(W * H), sentinel(W * H * 6)

    def rasterize(recs=None, count=None, W=W, H=H, flags=HOST, texels=texels_out, hits=hits_out, counts=True):
        recs = [(0, 4, uv.ctypes.data)] if recs is None else recs
        arr = (prt_amd.AtlasMesh * len(recs))(*[prt_amd.AtlasMesh(meshId=m, primCount=p, uv=u) for m, p, u in recs])
        c = prt_amd.AtlasCounts(n=77, rejected=77, degenerate=77, reserved=77, pairs=77)
        rc = L.prt_hip_atlas_rasterize(t._ctx, W, H, len(recs) if count is None else count, arr, ptr(texels), ptr(hits),
                                       C.byref(c) if counts else None, flags, None)
        assert (c.n, c.rejected, c.degenerate, c.reserved, c.pairs) == (77,) * 5, "a refused call wrote the counts"
        return rc
    u = uv.ctypes.data
    for kw in (dict(flags=HOST | 2), dict(flags=0x80000000), dict(W=0), dict(W=8193), dict(H=0), dict(H=8193), dict(count=0), dict(count=9),
               dict(recs=[(8, 4, u)]), dict(recs=[(0, 4, u), (1, 4, u), (0, 4, u)]), dict(recs=[(0, 0, u)]), dict(recs=[(0, (1 << 28) + 1, u)]),
               dict(recs=[(0, 4, None)]), dict(texels=None), dict(hits=None), dict(counts=False)):
        assert rasterize(**kw) == -2 and L.prt_hip_last_error(), kw
    arr = (prt_amd.AtlasMesh * 1)(prt_amd.AtlasMesh(meshId=0, primCount=4, uv=u))
    c = prt_amd.AtlasCounts()
    assert L.prt_hip_atlas_rasterize(t._ctx, W, H, 1, None, ptr(texels_out), ptr(hits_out), C.byref(c), HOST, None) == -2
    # points
    _, texels, hits = scene_atlas(t, arrays, 45, 37)
    pts_out = sentinel(len(hits) * 8)
    rc, _ = run_points(bare, dev, texels, hits, 45, F(0), 1, out=pts_out)
    assert rc == -5 and b"upload a scene" in L.prt_hip_last_error()
    for kw in (dict(flags=HOST | 4), dict(flags=2), dict(n=0), dict(n=(1 << 26) + 1), dict(W=0), dict(W=8193), dict(tile=0), dict(tile=33),
               dict(reserved=(1, 0)), dict(reserved=(0, 1))):
        args = dict(W=45, bias=F(0), tile=1)
        args.update(kw)
        rc, _ = run_points(t, dev, texels, hits, out=pts_out, **args)
        assert rc == -2 and L.prt_hip_last_error(), kw
    p = prt_amd.AtlasPointParams(bias=0.0, setTile=1)
    for args in ((None, ptr(hits), C.byref(p), ptr(pts_out)), (ptr(texels), None, C.byref(p), ptr(pts_out)), (ptr(texels), ptr(hits), None, ptr(pts_out)),
                 (ptr(texels), ptr(hits), C.byref(p), None)):
        assert L.prt_hip_atlas_points(t._ctx, len(hits), 45, *args, HOST, None) == -2
    # resolve
    inside = islands()
    values = resolve_values(len(inside), 3)
    image_out, mask_out = sentinel(RW * RH * 3), np.full(RW * RH, 0xab, np.uint8)

    def resolve(W=RW, H=RH, stride=3, gutter=2, **kw):
        return run_resolve(t, dev, inside, values, W, H, stride, gutter, image=image_out, mask=mask_out, **kw)[0]
    for kw in (dict(flags=HOST | 8), dict(flags=0x40000000), dict(W=0), dict(W=8193), dict(H=0), dict(H=8193), dict(n=0), dict(n=(1 << 26) + 1),
               dict(stride=0), dict(stride=49), dict(gutter=65)):
        assert resolve(**kw) == -2 and L.prt_hip_last_error(), kw
    for args in ((None, ptr(values), 3, 2, ptr(image_out), ptr(mask_out)), (ptr(inside), None, 3, 2, ptr(image_out), ptr(mask_out)),
                 (ptr(inside), ptr(values), 3, 2, None, ptr(mask_out))):
        assert L.prt_hip_atlas_resolve(t._ctx, RW, RH, len(inside), *args, HOST, None) == -2
    # device pointers that are not aligned
    base = dev.upload(np.zeros(1 << 16, np.uint8))
    one = (prt_amd.AtlasMesh * 1)(prt_amd.AtlasMesh(meshId=0, primCount=4, uv=base + 2))
    assert L.prt_hip_atlas_rasterize(t._ctx, W, H, 1, one, base + 4096, base + 8192, C.byref(c), 0, None) == -2 and b"4-byte aligned" in L.prt_hip_last_error()
    one[0].uv = base
    assert L.prt_hip_atlas_rasterize(t._ctx, W, H, 1, one, base + 4096 + 1, base + 8192, C.byref(c), 0, None) == -2
    assert L.prt_hip_atlas_rasterize(t._ctx, W, H, 1, one, base + 4096, base + 8192 + 2, C.byref(c), 0, None) == -2
    assert L.prt_hip_atlas_points(t._ctx, 16, 45, base, base + 4096, C.byref(p), base + 8192 + 8, 0, None) == -2 and b"16-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_atlas_points(t._ctx, 16, 45, base + 2, base + 4096, C.byref(p), base + 8192, 0, None) == -2
    assert L.prt_hip_atlas_points(t._ctx, 16, 45, base, base + 4096 + 1, C.byref(p), base + 8192, 0, None) == -2
    assert L.prt_hip_atlas_resolve(t._ctx, 8, 8, 16, base + 2, base + 4096, 3, 2, base + 8192, base + 16384, 0, None) == -2 and b"4-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_atlas_resolve(t._ctx, 8, 8, 16, base, base + 4096 + 1, 3, 2, base + 8192, base + 16384, 0, None) == -2
    assert L.prt_hip_atlas_resolve(t._ctx, 8, 8, 16, base, base + 4096, 3, 2, base + 8192 + 2, base + 16384, 0, None) == -2
    assert not fetch(dev, base, 1 << 16, np.uint8).any(), "a refused call wrote device memory"
    for name, o in (("texels", texels_out), ("hits", hits_out), ("points", pts_out), ("image", image_out)):
        assert (o == SENTINEL).all(), f"a refused call wrote its {name}"
    assert (mask_out == 0xab).all()
    # and the same arguments are accepted
    c = prt_amd.AtlasCounts()
    assert L.prt_hip_atlas_rasterize(t._ctx, W, H, 1, arr, ptr(texels_out), ptr(hits_out), C.byref(c), HOST, None) == 0 and c.n > 0
    assert run_points(t, dev, texels, hits, 45, F(0), 1, out=pts_out)[0] == 0 and not (pts_out == SENTINEL).any()
    assert resolve() == 0 and not (image_out == SENTINEL).any()
