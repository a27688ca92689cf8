"""Baking on the MI355X (include/prt_hip.h "baking"; the CPU half is tests/test_bake_cpu.py): prt_hip_bake_rays and prt_hip_bake_reduce of
the PRODUCT library against the numpy restatement tests/prt_bake_ref.py, and prt_hip_bake against reduce(query_radiance(rays())) with
the merged prt_hip_query_radiance under the same parameters and seed.  Everything at tolerance 0, compared as bytes (a NaN of the
restatement asks for a NaN: prt_bake_ref.same_bytes says why), on the plain, sky and box_rr stages of tests/prt_hostile_shade.py."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_bake_ref as BR
import prt_hostile_shade as HS
import prt_probe_ref as PR
from prt_gpukit import SCENES, SENTINEL, TAIL, fetch, ptr, sentinel, stage_tracers
from prt_gpukit import dev  # noqa: F401  (fixture: device memory and streams for one test)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
DEPTH = 8
N_POINTS = 37
KS = (1, 63, 64, 65, 130)
BLOCKS_PER_CU = 8       # PRT_BAKE_BLOCKS_PER_CU (prt_bake.hip): blocks of 256 lanes either kernel is launched with at the most
tracers = stage_tracers(SCENES, max_depth=DEPTH)
HOST = "the host array of the Sets"


def table(sets, dirs=HOST, weights=HOST, **fields):
    """prt_bake_sets of `sets`; dirs / weights: HOST, None (a NULL pointer) or a device address (int)."""
    assert all(v is HOST or v is None or type(v) is int for v in (dirs, weights)), (dirs, weights)
    t = prt_amd.BakeSets(K=sets.K, C=sets.C, nSets=sets.nSets, reserved=0, dirs=sets.dirs.ctypes.data if dirs is HOST else dirs,
                         weights=sets.weights.ctypes.data if weights is HOST else weights)
    for k, v in fields.items():
        setattr(t, k, v)
    return t


# ----------------------------------------------------------------------------- the points
def hostile_normals():
    nan = np.array([PR.NAN_PAYLOAD], dtype=U).view(F)[0]
    tenth = F(0.1)
    return np.array([
        (0.05, 1.0, 0.0), (tenth, 1.0, 0.0), (-tenth, 0.5, 0.5), (np.nextafter(tenth, F(1)), 1.0, 0.0), (np.nextafter(tenth, F(0)), 0.0, 1.0),  # around 0.1
        (0.6, 0.0, 0.8), (-0.6, 0.8, 0.0),
        (-0.0, 1.0, 0.0), (0.0, -0.0, 1.0), (1.0, -0.0, -0.0), (-0.0, -0.0, -1.0),  # negative zero components
        (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0),                     # N = 0: the identity frame
        (0.0, 2.0, 0.0), (3.0, 4.0, 12.0), (0.01, 0.02, 0.02),                     # not normalised
        (1e-30, 1e-30, 0.0), (0.0, 1e-30, 0.0), (0.0, 3e20, 1e20), (3e20, 0.0, 0.0),
        (0.0, np.inf, 0.0), (-np.inf, 1.0, 0.0), (nan, 1.0, 0.0), (0.0, nan, 0.0), (0.0, 1.0, nan),
    ], dtype=F)


def make_points(nSets, origins, seed=1):
    """The 37 points of tests 1 to 3: the hostile normals, then unit normals; bias 1e-4, 0 and negative; sets over the whole table,
    one point with set = nSets and one with 0xffffffff."""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(N_POINTS, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    h = hostile_normals()
    N[:len(h)] = h
    bias = np.full(N_POINTS, 1e-4, F)
    bias[::5], bias[3::7] = 0.0, -0.25
    sets = (np.arange(N_POINTS) % nSets).astype(U)
    sets[30], sets[33] = nSets, 0xffffffff
    return BR.points(origins(N_POINTS, rng), N, bias, sets)


def stage_origins(n, rng):
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.3, 1.5, n), rng.uniform(0.5, 3.0, n)], axis=1).astype(F)


def box_origins(n, rng):
    return rng.uniform(-0.8, 0.8, size=(n, 3)).astype(F)


def make_sets(nSets, K, Cc, seed=2):
    """Directions of any length around the upper hemisphere (with a -0.0 and a zero direction), positive weights."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(nSets, K, 3))
    d[..., 2] = np.abs(d[..., 2])
    d = d.astype(F)
    d[0, 0, 0] = -0.0
    if K > 2:
        d[nSets - 1, 2] = 0.0
    return BR.Sets(d, rng.uniform(0.05, 1.0, size=(nSets, K, Cc)).astype(F))


# ----------------------------------------------------------------------------- 1. rays
def run_rays(t, dev, pts, sets, device):
    """prt_hip_bake_rays on host or device arrays: the n*K rays followed by the sentinel words."""
    n = len(pts)
    out = sentinel(n * sets.K * 8 + TAIL)
    if not device:
        tb = table(sets, weights=None)
        rc = t._L.prt_hip_bake_rays(t._ctx, n, ptr(pts), C.byref(tb), ptr(out), prt_amd.QUERY_HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return out
    d_pts, d_dirs, d_out = (dev.upload(a) for a in (pts, sets.dirs, out))
    tb = table(sets, weights=None, dirs=d_dirs)
    rc = t._L.prt_hip_bake_rays(t._ctx, n, d_pts, C.byref(tb), d_out, 0, None)
    assert rc == 0, t._L.prt_hip_last_error()
    return fetch(dev, d_out, out.size)


def check_rays(got, pts, sets, what):
    want = BR.rays(pts, sets)
    words = len(want) * 8
    nans = BR.same_bytes(got[:words], want, what)
    w = want.view(U).reshape(-1)
    other = np.nonzero(got[:words] != w)[0]
    print(f"{what}: {nans} NaN words, {len(other)} of them with other bits than the restatement's" +
          (f" (first: {got[other[0]]:#x} for {w[other[0]]:#x})" if len(other) else ""))
    assert (got[words:] == SENTINEL).all(), f"{what}: words behind the rays were written"
    return nans


@pytest.mark.parametrize("nSets", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_rays_equal_the_restatement(tracers, dev, K, nSets):
    t = tracers("none")  # prt_hip_bake_rays needs no scene
    pts, sets = make_points(nSets, stage_origins), make_sets(nSets, K, 1)
    host = run_rays(t, dev, pts, sets, device=False)
    nans = check_rays(host, pts, sets, f"K={K} nSets={nSets}, host arrays")
    r = host[:N_POINTS * K * 8].view(BR.RAY_DTYPE).reshape(N_POINTS, K)
    assert not r["org"][[30, 33]].view(U).any() and not r["dir"][[30, 33]].view(U).any(), "a set outside the table was followed"
    assert np.isfinite(r["dir"][:17]).all() and nans > 0
    on_device = run_rays(t, dev, pts, sets, device=True)
    assert on_device.tobytes() == host.tobytes(), "device and host pointers give different bytes"


def test_rays_beyond_one_trip_of_the_grid_stride_loop(tracers, dev):
    t = tracers("none")
    K, nSets = 65, 3
    one_trip = t.device_info()[1] * BLOCKS_PER_CU * 256
    n = one_trip // K + 41
    assert n * K > one_trip + 256
    base = make_points(nSets, stage_origins)
    pts = np.tile(base, n // N_POINTS + 1)[:n].copy()
    pts["P"][:, 0] += np.arange(n, dtype=F) * F(0.001)  # (no two points alike)
    sets = make_sets(nSets, K, 1)
    got = run_rays(t, dev, pts, sets, device=False)
    check_rays(got, pts, sets, f"{n} points x {K} directions")


# ----------------------------------------------------------------------------- 2. reduce
# (differs from test_gpu_lens.py's: a +1e38 / -1e38 pair that cancels in every point, NaN in point 5 only, no infinities)
def synthetic_radiance(n, K, seed=3):
    """(n*K, 3): random values, -0.0, denormals, a +1e38 / -1e38 pair that cancels in every point (k = 0 and 1, where the weights are
    1), and NaN in rows of point 5 only."""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, K, 3)).astype(F)
    L[rng.random((n, K, 3)) < 0.05] = -0.0
    L[rng.random((n, K, 3)) < 0.05] = 1e-40
    L[rng.random((n, K, 3)) < 0.02] = -3e-45
    if K >= 2:
        L[:, 0], L[:, 1] = 1e38, -1e38
    L[5, K // 2, 1] = np.nan
    L[5, K - 1] = np.nan
    return L.reshape(n * K, 3)


def run_reduce(t, dev, pts, sets, L, device):
    n = len(pts)
    out = sentinel(n * sets.C * 3 + TAIL)
    if not device:
        tb = table(sets, dirs=None)
        rc = t._L.prt_hip_bake_reduce(t._ctx, n, ptr(pts), C.byref(tb), ptr(L), ptr(out), prt_amd.QUERY_HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return out
    d_pts, d_w, d_L, d_out = (dev.upload(a) for a in (pts, sets.weights, L, out))
    tb = table(sets, dirs=None, weights=d_w)
    rc = t._L.prt_hip_bake_reduce(t._ctx, n, d_pts, C.byref(tb), d_L, d_out, 0, None)
    assert rc == 0, t._L.prt_hip_last_error()
    return fetch(dev, d_out, out.size)


def check_reduce(t, dev, K, Cc, nSets=3):
    pts, sets = make_points(nSets, stage_origins), make_sets(nSets, K, Cc)
    sets.weights[:, :2] = 1.0
    L = synthetic_radiance(N_POINTS, K)
    want = BR.reduce(pts, sets, L)
    words = want.size
    assert np.isnan(want[5]).all() and not np.isnan(np.delete(want, 5, axis=0)).any(), "the NaN stays in its point"
    assert want[[30, 33]].tobytes() == np.zeros((2, Cc, 3), F).tobytes()
    host = run_reduce(t, dev, pts, sets, L, device=False)
    BR.same_bytes(host[:words], want, f"K={K} C={Cc}, host arrays")
    assert (host[words:] == SENTINEL).all(), "words behind out were written"
    on_device = run_reduce(t, dev, pts, sets, L, device=True)
    assert on_device.tobytes() == host.tobytes(), "device and host pointers give different bytes"


@pytest.mark.parametrize("Cc", [1, 3, 9, 16])
@pytest.mark.parametrize("K", KS)
def test_reduce_equals_the_restatement(tracers, dev, K, Cc):
    check_reduce(tracers("none"), dev, K, Cc)


def test_reduce_of_the_largest_set(tracers, dev):
    check_reduce(tracers("none"), dev, 4096, 3, nSets=2)


def test_a_nan_weight_stays_in_its_set(tracers, dev):
    t = tracers("none")
    pts, sets = make_points(3, stage_origins), make_sets(3, 65, 3)
    sets.weights[1, 64, 2] = np.nan
    L = np.random.default_rng(4).gamma(1.0, 1.0, size=(N_POINTS * 65, 3)).astype(F)
    want = BR.reduce(pts, sets, L)
    got = run_reduce(t, dev, pts, sets, L, device=False)
    BR.same_bytes(got[:want.size], want, "a NaN weight")
    hit = np.isnan(want).any(axis=(1, 2))
    assert (hit == (pts["set"] == 1)).all() and np.isnan(want[hit][:, 2]).all() and not np.isnan(want[hit][:, :2]).any()


# ----------------------------------------------------------------------------- 3. the fused call
def composition(t, pts, sets, spp, seed):
    """reduce(points, sets, query_radiance(rays(points, sets))) with the merged query under the same parameters and seed; the
    statistics of that query."""
    r = BR.rays(pts, sets)
    L = t.query_radiance(r["org"], r["dir"], spp, seed=seed)
    return BR.reduce(pts, sets, L), t.last_stats, L


def run_bake(t, pts, sets, spp, seed, flags=prt_amd.QUERY_HOST, out=None, n=None, tb=None, points=True, params=True, **fields):
    """prt_hip_bake itself on host arrays: (code, out followed by sentinel words); fields override render parameters."""
    p = t.params(spp, max_depth=DEPTH)
    p.seed = seed
    for k, v in fields.items():
        setattr(p, k, v)
    out = sentinel(len(pts) * sets.C * 3 + TAIL) if out is None else out
    tb = table(sets) if tb is None else tb
    rc = t._L.prt_hip_bake(t._ctx, len(pts) if n is None else n, ptr(pts) if points else None, C.byref(tb) if tb else None,
                           C.byref(p) if params else None, ptr(out), flags, None)
    return rc, out


@pytest.mark.parametrize("spp", [8, 24])
@pytest.mark.parametrize("Cc", [1, 9])
@pytest.mark.parametrize("K", [8, 65])
@pytest.mark.parametrize("name", ["plain", "sky", "box_rr"])
def test_bake_equals_reduce_of_query_radiance_of_rays(tracers, name, K, Cc, spp):
    t = tracers(name)
    pts, sets = make_points(3, box_origins if name == "box_rr" else stage_origins), make_sets(3, K, Cc)
    seed = 4000 + K
    want, qstats, L = composition(t, pts, sets, spp, seed)
    assert not np.isnan(want).any()
    rc, got = run_bake(t, pts, sets, spp, seed)
    assert rc == 0, t._L.prt_hip_last_error()
    st = t.stats()
    BR.same_bytes(got[:want.size], want, f"{name} K={K} C={Cc} at {spp} spp")
    assert (got[want.size:] == SENTINEL).all()
    assert (st["raysTraced"], st["nPx"]) == (qstats["raysTraced"], qstats["nPx"]) and st["nPx"] == N_POINTS * K
    assert st["kernelLaunches"] == 1 and st["stackOverflow"] == 0
    lit = int((want != 0).any(axis=(1, 2)).sum())
    print(f"{name} K={K} C={Cc} spp={spp}: {lit} of {N_POINTS} points are not black")
    assert lit >= 8
    assert not L.reshape(N_POINTS, K, 3)[17:26].any(), "a hostile normal's rays are black"
    # the Python wrapper is the same call
    if spp == 8 and Cc == 1:
        with_wrapper = t.bake(pts["P"], pts["N"], sets.dirs, sets.weights, spp, bias=pts["bias"], sets=pts["set"], seed=seed)
        assert with_wrapper.shape == (N_POINTS, Cc, 3) and with_wrapper.tobytes() == want.tobytes()
        assert t.bake_rays(pts["P"], pts["N"], sets.dirs, bias=pts["bias"], sets=pts["set"]).view(U).tobytes() == \
            run_rays(t, None, pts, sets, device=False)[:N_POINTS * K * 8].tobytes()
        assert t.bake_reduce(sets.weights, L.reshape(N_POINTS, K, 3), sets=pts["set"]).tobytes() == want.tobytes()


# ----------------------------------------------------------------------------- 4. meaning
def test_a_cosine_set_gives_the_irradiance_of_the_c10_recipe(tracers):
    """A point of the open floor under the sky, 256 cosine-weighted directions from bake_cosine_set against the recipe of INTEGRATION.md
    C10 with 256 other directions.  Both are means of 256 independent terms pi * L_k, so each has the standard error pi * std(L) /
    sqrt(256) of its own per-ray radiances, their difference has the root of the two squares, and three of those bound it (a
    chance of 0.3 % per channel for a correct estimator; a missing pi, a frame about another axis or weights that do not sum to pi
    move the estimate by its own size).  A ray that leaves the stage returns black (the sky lights surfaces; a primary ray that misses
    sees none of it), so the estimate is carried by the rays that meet the patches and the wall: the point lies on the floor close in
    front of the patches, where about a fifth of the directions do.  (From (1.5, 0, 2) hardly any did: 0.0016 against 0.0106 with a
    standard error of 0.0077, a bound of three times the estimate that could tell nothing.)"""
    t = tracers("sky")
    K, spp, seed = 256, 8, 99
    P, N = np.array([[0.0, 0.0, 0.4]], F), np.array([[0.0, 1.0, 0.0]], F)
    d, w = prt_amd.bake_cosine_set(K, np.random.default_rng(10))
    E1 = t.bake(P, N, d, w, spp, seed=seed)[0, 0].astype(np.float64)
    r = t.bake_rays(P, N, d)
    L1 = t.query_radiance(r["org"], r["dir"], spp, seed=seed).astype(np.float64)
    # the recipe, with its own tangent frame
    rng = np.random.default_rng(11)
    u1, u2 = rng.random(K), rng.random(K)
    rr, phi = np.sqrt(u1), 2 * np.pi * u2
    local = np.stack([rr * np.cos(phi), rr * np.sin(phi), np.sqrt(1 - u1)], axis=1)
    dirs = local @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    L2 = t.query_radiance(np.tile(P[0] + F(1e-4) * N[0], (K, 1)), dirs, spp, seed=seed + 7).astype(np.float64)
    E2 = np.pi * L2.mean(axis=0)
    se = np.pi * np.sqrt(L1.var(axis=0, ddof=1) / K + L2.var(axis=0, ddof=1) / K)
    print(f"irradiance: bake {E1}, recipe {E2}, standard error of the difference {se}")
    assert (E2 > 0).all() and (3 * se < E2).all(), "the bound must be able to tell a factor of two"
    assert np.abs(E1 - np.pi * L1.mean(axis=0)).max() <= K * 2.0 ** -23 * np.pi * np.abs(L1).mean(axis=0).max()
    assert (np.abs(E1 - E2) <= 3 * se).all()


# ----------------------------------------------------------------------------- 5. refusals and state
def test_refusals_queue_nothing_and_leave_out_untouched(tracers, dev):
    t, bare = tracers("plain"), tracers("none")
    L = t._L
    pts, sets = make_points(3, stage_origins), make_sets(3, 8, 2)
    rad = np.zeros((N_POINTS * 8, 3), F)
    t.stats()
    # without a scene
    rc, out = run_bake(bare, pts, sets, 8, 1)
    assert rc == -5 and b"upload a scene" in bare._L.prt_hip_last_error() and (out == SENTINEL).all()
    # the table, n and the flags: all three calls
    big = prt_amd.BakeSets(K=4096, C=1, nSets=1, reserved=0, dirs=sets.dirs.ctypes.data, weights=sets.weights.ctypes.data)
    bad_tables = [dict(K=0), dict(K=4097), dict(C=0), dict(C=17), dict(nSets=0), dict(nSets=1025), dict(reserved=1)]
    cases = [dict(tb=table(sets, **kw)) for kw in bad_tables] + [dict(n=0), dict(n=(1 << 24) // 8 + 1), dict(tb=big, n=4097),
                                                                  dict(flags=prt_amd.QUERY_HOST | 2), dict(flags=0x80000000)]
    outs = {"rays": sentinel(N_POINTS * 8 * 8), "reduce": sentinel(N_POINTS * 2 * 3), "bake": sentinel(N_POINTS * 2 * 3)}
    for kw in cases:
        tb, n, flags = kw.get("tb", table(sets)), kw.get("n", N_POINTS), kw.get("flags", prt_amd.QUERY_HOST)
        assert L.prt_hip_bake_rays(t._ctx, n, ptr(pts), C.byref(tb), ptr(outs["rays"]), flags, None) == -2 and L.prt_hip_last_error(), kw
        assert L.prt_hip_bake_reduce(t._ctx, n, ptr(pts), C.byref(tb), ptr(rad), ptr(outs["reduce"]), flags, None) == -2 and L.prt_hip_last_error(), kw
        rc, _ = run_bake(t, pts, sets, 8, 1, out=outs["bake"], **kw)
        assert rc == -2 and L.prt_hip_last_error(), (kw, rc)
    # what prt_hip_query_radiance refuses of the parameters
    for kw in (dict(samples=0), dict(samples=12), dict(samples=2048), dict(nranks=2), dict(rank=1, nranks=2), dict(countTraffic=1), dict(maxDepth=256)):
        rc, _ = run_bake(t, pts, sets, 8, 1, out=outs["bake"], **kw)
        assert rc == -2 and L.prt_hip_last_error(), (kw, rc)
    # NULL pointers
    tb = table(sets)
    for args in ((None, C.byref(tb), ptr(outs["rays"])), (ptr(pts), None, ptr(outs["rays"])), (ptr(pts), C.byref(tb), None),
                 (ptr(pts), C.byref(table(sets, dirs=None)), ptr(outs["rays"]))):
        assert L.prt_hip_bake_rays(t._ctx, N_POINTS, *args, prt_amd.QUERY_HOST, None) == -2
    for args in ((None, C.byref(tb), ptr(rad), ptr(outs["reduce"])), (ptr(pts), None, ptr(rad), ptr(outs["reduce"])),
                 (ptr(pts), C.byref(tb), None, ptr(outs["reduce"])), (ptr(pts), C.byref(tb), ptr(rad), None),
                 (ptr(pts), C.byref(table(sets, weights=None)), ptr(rad), ptr(outs["reduce"]))):
        assert L.prt_hip_bake_reduce(t._ctx, N_POINTS, *args, prt_amd.QUERY_HOST, None) == -2
    for kw in (dict(points=False), dict(params=False), dict(tb=table(sets, dirs=None)), dict(tb=table(sets, weights=None))):
        assert run_bake(t, pts, sets, 8, 1, out=outs["bake"], **kw)[0] == -2, kw
    p = t.params(8, max_depth=DEPTH)
    assert L.prt_hip_bake(t._ctx, N_POINTS, ptr(pts), None, C.byref(p), ptr(outs["bake"]), prt_amd.QUERY_HOST, None) == -2
    assert L.prt_hip_bake(t._ctx, N_POINTS, ptr(pts), C.byref(tb), C.byref(p), None, prt_amd.QUERY_HOST, None) == -2
    # device pointers that are not aligned
    base = dev.upload(np.zeros(1 << 16, np.uint8))
    dt = table(sets, dirs=base, weights=base + 4096)
    assert L.prt_hip_bake(t._ctx, N_POINTS, base + 8192 + 8, C.byref(dt), C.byref(p), base + 16384, 0, None) == -2 and b"16-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_bake(t._ctx, N_POINTS, base + 8192, C.byref(dt), C.byref(p), base + 16384 + 2, 0, None) == -2 and b"4-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_bake_rays(t._ctx, N_POINTS, base + 8192, C.byref(dt), base + 16384 + 8, 0, None) == -2 and b"16-byte aligned" in L.prt_hip_last_error()
    dt.weights = base + 4096 + 1
    assert L.prt_hip_bake_reduce(t._ctx, N_POINTS, base + 8192, C.byref(dt), base + 16384, base + 32768, 0, None) == -2
    assert not fetch(dev, base, 1 << 16, np.uint8).any(), "a refused call wrote device memory"
    assert t.stats()["kernelLaunches"] == 0
    for k, o in outs.items():
        assert (o == SENTINEL).all(), f"a refused {k} call wrote its output"
    rc, out = run_bake(t, pts, sets, 8, 1)  # and the same arguments are accepted
    assert rc == 0 and not (out[:N_POINTS * 6] == SENTINEL).any()


def test_a_bake_leaves_the_context_alone():
    prt_amd.build()
    scene, camera = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        t.upload_scene(scene)
        t.set_camera(camera)
        want16 = t.render(16)
        t.accumulate(8)
        t.display(prt_amd.DisplayParams.make(meter=True))
        W, H = camera.width, camera.height
        org, d = PR.stage_probes(100, seed=23)
        probes = t.query_radiance(org, d, 8, seed=5)  # (the staging arena holds this batch)

        def snapshot():
            acc = t.accum_export()
            return dict(rng=acc["rng"], sum=acc["sum"], count=acc["count"], bound=np.array([acc["seed"], acc["max_depth"], acc["rr_depth"]]),
                        display=np.frombuffer(repr(sorted(t.display_state().items())).encode(), np.uint8),
                        framebuffer=t._download_rect(0, 0, W - 1, H - 1, stats=False))
        before = snapshot()
        assert before["count"].any() and before["framebuffer"].any()
        pts, sets = make_points(3, stage_origins), make_sets(3, 65, 9)
        want, _, _ = composition(t, pts, sets, 8, 77)
        before = snapshot()
        rc, got = run_bake(t, pts, sets, 8, 77)
        assert rc == 0, t._L.prt_hip_last_error()
        BR.same_bytes(got[:want.size], want, "the bake between the passes")
        after = snapshot()
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        assert t.accumulate(8).tobytes() == want16.tobytes(), "the accumulate pass behind the bake continues the one-shot render"
        assert t.render(16).tobytes() == want16.tobytes(), "the render digest"
        assert t.query_radiance(org, d, 8, seed=5).tobytes() == probes.tobytes()
    finally:
        t.close()


def test_a_bake_sees_the_moved_mesh():
    prt_amd.build()
    scene, _ = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        t.upload_scene(scene)
        pts, sets = make_points(3, stage_origins), make_sets(3, 65, 1)
        rc, first = run_bake(t, pts, sets, 8, 66)
        assert rc == 0
        moved = (scene.arrays()["meshes"][0]["positions"] + np.array([0.4, 0.0, 0.3], F)).astype(F)
        scene.update_positions(0, moved)
        t.update_meshes(scene, [0])
        rc, second = run_bake(t, pts, sets, 8, 66)
        assert rc == 0
        want, _, _ = composition(t, pts, sets, 8, 66)
        BR.same_bytes(second[:want.size], want, "after update_meshes")
        assert second.tobytes() != first.tobytes()
    finally:
        t.close()


def test_device_arrays_on_a_callers_stream_with_a_copy_behind(tracers, dev):
    t = tracers("sky")
    pts, sets = make_points(3, stage_origins), make_sets(3, 130, 9)
    spp, seed = 8, 31
    rc, want = run_bake(t, pts, sets, spp, seed)
    assert rc == 0
    words = N_POINTS * 9 * 3
    stream = dev.stream()
    zeros = np.zeros_like(pts)
    d_pts, d_dirs, d_w, d_out, d_copy = (dev.upload(a) for a in (zeros, sets.dirs, sets.weights, sentinel(words + TAIL), sentinel(words + TAIL)))
    got = np.zeros(words + TAIL, U)
    # the points arrive on the caller's stream, the bake is queued behind them and a device copy of the answer behind the bake
    dev.upload_async(pts, stream, d_pts)
    tb = prt_amd.BakeSets(K=sets.K, C=sets.C, nSets=sets.nSets, reserved=0, dirs=d_dirs, weights=d_w)
    t.stats()
    t.bake_async(N_POINTS, d_pts, tb, d_out, spp, seed=seed, stream=stream)
    dev.copy_async(d_copy, d_out, (words + TAIL) * 4, stream)
    dev.download_async(got, d_copy, stream)
    dev.synchronize(stream)
    assert got.tobytes() == want.tobytes()
    st = t.stats()
    assert st["kernelLaunches"] == 1 and st["nPx"] == N_POINTS * 130
