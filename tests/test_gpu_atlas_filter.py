"""The lightmap filter on the MI355X (include/prt_hip.h "lightmap filter"; the CPU half is tests/test_atlas_filter_cpu.py):
prt_hip_atlas_filter of the PRODUCT library against the numpy restatement tests/prt_atlas_filter_ref.py, on host arrays and on
device pointers, and PathTracer.lightmap(filter=...) against the five calls composed by the test.  Everything at tolerance 0, compared
as bytes (a NaN of the restatement asks for a NaN: prt_bake_ref.same_bytes), with sentinel words behind every output.  The inputs
are tests/prt_atlas_filter_cases.py, which says where a hostile point sits and why it can leave the others' results unchanged."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_atlas_filter_cases as AC
import prt_atlas_filter_ref as AF
import prt_bake_ref as BR
import prt_testlib as T
from prt_gpukit import SENTINEL, TAIL, fetch, ptr, sentinel, stage_tracers
from prt_gpukit import dev  # noqa: F401  (fixture: device memory and streams for one test)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
HOST = prt_amd.QUERY_HOST
BLOCKS_PER_CU = 8  # PRT_AF_BLOCKS_PER_CU (prt_atlas_filter.hip): blocks of 256 lanes, one point a lane


# (the teapot stage of tests/test_gpu_atlas.py)
def teapot_scene():
    return prt_amd.setup_cornell_box(8, 8, teapot_mesh=T.teapot_product_mesh())[0]


tracers = stage_tracers({"teapot": teapot_scene}, arrays=True, max_depth=8)  # tracers(name) -> (context, the scene's mesh arrays)


def params(iterations=5, npl2=5, sigma_l=4.0, sigma_p=4.0, reserved=(0, 0, 0, 0)):
    p = prt_amd.AtlasFilterParams(iterations, npl2, sigma_l, sigma_p)
    for k, r in enumerate(reserved):
        p.reserved[k] = r
    return p


def run_filter(t, dev, texels, points, values, W, H, p, device=False, flags=HOST, n=None, stride=None, out=None):
    """prt_hip_atlas_filter itself: (code, out as words followed by sentinel words)."""
    texels, points = np.ascontiguousarray(texels, U), np.ascontiguousarray(points)
    values = np.ascontiguousarray(values, F).reshape(len(texels), -1)
    n = len(texels) if n is None else n
    stride = values.shape[1] if stride is None else stride
    out = sentinel(values.size + TAIL) if out is None else out
    if not device:
        return t._L.prt_hip_atlas_filter(t._ctx, W, H, n, ptr(texels), ptr(points), ptr(values), stride, C.byref(p), ptr(out), flags, None), out
    d_t, d_p, d_v, d_o = (dev.upload(a) for a in (texels, points, values, out))
    rc = t._L.prt_hip_atlas_filter(t._ctx, W, H, n, d_t, d_p, d_v, stride, C.byref(p), d_o, 0, None)
    return rc, fetch(dev, d_o, out.size)


def check(t, dev, texels, points, values, W, H, what, iterations=5, npl2=5, sigma_l=4.0, sigma_p=4.0, both=True):
    """Host arrays (and device pointers) against the restatement; returns (the product's out (n, stride) float32, the NaNs)."""
    want = AF.filter(texels, points, values, W, H, iterations, npl2, sigma_l, sigma_p)
    p = params(iterations, npl2, sigma_l, sigma_p)
    rc, got = run_filter(t, dev, texels, points, values, W, H, p)
    assert rc == 0, t._L.prt_hip_last_error()
    nans = BR.same_bytes(got[:want.size], want, f"{what}, host arrays")
    assert (got[want.size:] == SENTINEL).all(), f"{what}: words behind out were written"
    if both:
        rc, on_device = run_filter(t, dev, texels, points, values, W, H, p, device=True)
        assert rc == 0, t._L.prt_hip_last_error()
        BR.same_bytes(on_device[:want.size], want, f"{what}, device pointers")
        assert (on_device[want.size:] == SENTINEL).all(), f"{what}: words behind out were written on the device"
    return got[:want.size].view(F).reshape(want.shape), nans


# ----------------------------------------------------------------------------- 1. the two charts
@pytest.mark.parametrize("npl2", [0, 7])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("Cc", [1, 3, 16])
def test_two_charts_equal_the_restatement(tracers, dev, Cc, iterations, npl2):
    t, _ = tracers("none")  # prt_hip_atlas_filter needs no scene
    texels, pts, v, _, _ = AC.two_charts(C=Cc)
    out, nans = check(t, dev, texels, pts, v, AC.W2, AC.H2, f"C={Cc} iterations={iterations} npl2={npl2}", iterations, npl2)
    assert nans == 0 and np.isfinite(out).all() and out.tobytes() != v.tobytes()


def test_other_sigmas_and_the_python_wrapper(tracers, dev):
    t, _ = tracers("none")
    texels, pts, v, _, _ = AC.two_charts(C=2)
    out, _ = check(t, dev, texels, pts, v, AC.W2, AC.H2, "sigmas 0.7 and 1.5", 3, 2, 0.7, 1.5)
    wrapped = t.atlas_filter(texels, pts, v.reshape(-1, 2, 3), AC.W2, AC.H2, params(3, 2, 0.7, 1.5))
    assert wrapped.shape == (len(texels), 2, 3) and wrapped.tobytes() == out.tobytes()
    assert t.atlas_filter(texels, pts, v, AC.W2, AC.H2).tobytes() == AF.filter(texels, pts, v, AC.W2, AC.H2).tobytes()  # the defaults


def test_small_atlases_and_one_point(tracers, dev):
    t, _ = tracers("none")
    for W, H in ((129, 5), (1, 1)):
        texels, pts, v = AC.owned(W, H, C=2)
        out, _ = check(t, dev, texels, pts, v, W, H, f"{W} x {H}")
        assert out.tobytes() == v.tobytes() if W * H == 1 else out.tobytes() != v.tobytes()  # (one point: S/sumW = (w*C)/w is C again)
    texels, pts, v = AC.owned(129, 5)
    out, _ = check(t, dev, texels[300:301], pts[300:301], v[300:301], 129, 5, "n = 1")
    assert np.isfinite(out).all()


# ----------------------------------------------------------------------------- 2. hostile points
@pytest.mark.parametrize("kind", AC.HOSTILE)
def test_a_hostile_point_leaves_the_others_as_a_run_without_it(tracers, dev, kind):
    t, _ = tracers("none")
    with_, without, keep = AC.hostile(kind)
    a, nans = check(t, dev, *with_, AC.W2, AC.H2, kind)
    b, _ = check(t, dev, *without, AC.W2, AC.H2, f"{kind}: the run without", both=False)
    assert a[keep].tobytes() == b.tobytes(), f"{kind}: the others' results differ from a run without the hostile point"
    assert np.isfinite(a[keep]).all() and nans == (1 if kind in ("nan_c0", "nan_later", "duplicate") else 0)


def test_a_long_normal_and_values_that_overflow_the_sums(tracers, dev):
    t, _ = tracers("none")
    (texels, pts, v), _, keep = AC.hostile("long_normal")
    out, nans = check(t, dev, texels, pts, v, AC.W2, AC.H2, "long_normal")
    assert nans == 0 and np.isfinite(out).all()
    (texels, pts, v), _, _ = AC.hostile("huge_values")
    assert np.isfinite(v).all() and v.max() > 1e38
    out, nans = check(t, dev, texels, pts, v, AC.W2, AC.H2, "huge_values")
    print(f"huge values: {nans} NaN words of {out.size}")
    assert nans > 0
    # after one iteration the NaNs (0 * inf in V0 where a chart border zeroes a weight) have not spread: most words are finite
    out, nans = check(t, dev, texels, pts, v, AC.W2, AC.H2, "huge_values, one iteration", iterations=1)
    assert 0 < nans < out.size // 2


def test_texels_in_shuffled_order(tracers, dev):
    t, _ = tracers("none")
    texels, pts, v, _, _ = AC.two_charts(C=3, seed=4)
    order = np.random.default_rng(8).permutation(len(texels))
    a, _ = check(t, dev, texels, pts, v, AC.W2, AC.H2, "ascending", both=False)
    b, _ = check(t, dev, texels[order], pts[order], v[order], AC.W2, AC.H2, "shuffled")
    assert b.tobytes() == a[order].tobytes()


# ----------------------------------------------------------------------------- 3. beyond one trip of the grid-stride loops
def test_more_points_than_lanes_are_launched(tracers, dev):
    t, _ = tracers("none")
    lanes = t.device_info()[1] * BLOCKS_PER_CU * 256
    W, H = 1024, lanes // 1024 + 1  # the smallest whole rows past one trip of the index, prepare and iterate loops: 1024 x 513 on 256 CUs
    texels, pts, v = AC.owned(W, H)
    assert lanes < len(texels) <= lanes + 1024
    out, _ = check(t, dev, texels, pts, v, W, H, f"{W} x {H}", iterations=1, both=False)
    assert (out[lanes:] != v[lanes:]).any(axis=1).all(), "the points of the second trip were filtered"


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals_queue_nothing_and_leave_out_untouched(tracers, dev):
    t, _ = tracers("none")
    L = t._L
    texels, pts, v, _, _ = AC.two_charts(C=2)
    n = len(texels)
    out = sentinel(v.size + TAIL)

    def call(W=AC.W2, H=AC.H2, p=None, **kw):
        return run_filter(t, dev, texels, pts, v, W, H, params() if p is None else p, out=out, **kw)[0]
    nan, inf = float("nan"), float("inf")
    for kw in (dict(flags=HOST | 2), dict(flags=0x80000000), dict(W=0), dict(W=8193), dict(H=0), dict(H=8193), dict(n=0), dict(n=(1 << 26) + 1),
               dict(stride=0), dict(stride=4), dict(stride=5), dict(stride=51), dict(stride=2),
               dict(p=params(iterations=0)), dict(p=params(iterations=6)), dict(p=params(npl2=8)),
               dict(p=params(sigma_l=0.0)), dict(p=params(sigma_l=-1.0)), dict(p=params(sigma_l=nan)), dict(p=params(sigma_l=inf)),
               dict(p=params(sigma_p=0.0)), dict(p=params(sigma_p=-2.0)), dict(p=params(sigma_p=nan)), dict(p=params(sigma_p=inf)),
               dict(p=params(reserved=(1, 0, 0, 0))), dict(p=params(reserved=(0, 0, 0, 1)))):
        assert call(**kw) == -2 and L.prt_hip_last_error(), kw
    p = params()
    good = (ptr(texels), ptr(pts), ptr(v), 6, C.byref(p), ptr(out))
    for k in (0, 1, 2, 4, 5):  # a NULL pointer
        args = list(good)
        args[k] = None
        assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, *args, HOST, None) == -2, k
    # ranges of values and out that overlap, by one float at either end, and out == values
    both = np.concatenate([v.reshape(-1), np.zeros(v.size, F)])
    for off in (0, 1, v.size - 1):
        assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, ptr(texels), ptr(pts), both.ctypes.data + 4 * off, 6, C.byref(p), both.ctypes.data, HOST, None) == -2
        assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, ptr(texels), ptr(pts), both.ctypes.data, 6, C.byref(p), both.ctypes.data + 4 * off, HOST, None) == -2
        assert b"overlap" in L.prt_hip_last_error()
    assert both[:v.size].tobytes() == v.tobytes() and not both[v.size:].any()
    # device pointers: not aligned, and ranges that overlap
    base = dev.upload(np.zeros(1 << 18, np.uint8))
    d_t, d_p, d_v, d_o = base, base + (1 << 14), base + (1 << 16), base + (1 << 17)
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, d_t, d_p + 8, d_v, 6, C.byref(p), d_o, 0, None) == -2 and b"16-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, d_t + 2, d_p, d_v, 6, C.byref(p), d_o, 0, None) == -2
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, d_t, d_p, d_v + 1, 6, C.byref(p), d_o, 0, None) == -2
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, d_t, d_p, d_v, 6, C.byref(p), d_o + 2, 0, None) == -2
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, d_t, d_p, d_v, 6, C.byref(p), d_v + 4 * (v.size - 1), 0, None) == -2 and b"overlap" in L.prt_hip_last_error()
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, d_t, d_p, d_v, 6, C.byref(p), d_v, 0, None) == -2
    assert not fetch(dev, base, 1 << 18, np.uint8).any(), "a refused call wrote device memory"
    assert (out == SENTINEL).all(), "a refused call wrote out"
    # and the same arguments are accepted; out right behind values is no overlap
    assert call() == 0 and not (out[:v.size] == SENTINEL).any() and (out[v.size:] == SENTINEL).all()
    assert L.prt_hip_atlas_filter(t._ctx, AC.W2, AC.H2, n, ptr(texels), ptr(pts), both.ctypes.data, 6, C.byref(p), both.ctypes.data + 4 * v.size, HOST, None) == 0
    assert both[v.size:].tobytes() == out[:v.size].tobytes()


# ----------------------------------------------------------------------------- 5. a caller's stream
def test_device_arrays_on_a_callers_stream_with_a_copy_behind(tracers, dev):
    t, _ = tracers("none")
    texels, pts, v, _, _ = AC.two_charts(C=3)
    want = AF.filter(texels, pts, v, AC.W2, AC.H2)
    words = want.size
    stream = dev.stream()
    d_t, d_p, d_v = dev.upload(texels), dev.upload(pts), dev.upload(np.zeros_like(v))
    d_out, d_copy = dev.upload(sentinel(words + TAIL)), dev.upload(sentinel(words + TAIL))
    got = np.zeros(words + TAIL, U)
    # the values arrive on the caller's stream, the filter is queued behind them and a device copy of the answer behind the filter
    dev.upload_async(v, stream, d_v)
    t.atlas_filter_async(AC.W2, AC.H2, len(texels), d_t, d_p, d_v, v.shape[1], d_out, stream=stream)
    dev.copy_async(d_copy, d_out, (words + TAIL) * 4, stream)
    dev.download_async(got, d_copy, stream)
    dev.synchronize(stream)
    assert got[:words].tobytes() == want.tobytes() and (got[words:] == SENTINEL).all()


def test_the_filter_is_no_launch_for_the_statistics(tracers, dev):
    t, _ = tracers("teapot")
    t.stats()  # (reads and clears the launch counters)
    texels, pts, v, _, _ = AC.two_charts(C=1)
    t.atlas_filter(texels, pts, v, AC.W2, AC.H2)
    assert t.stats()["kernelLaunches"] == 0


def test_the_profile_entry_point_runs_the_same_filter(dev):
    """prt_hip_test_atlas_filter_profile of the TEST build (tools/query_bench.py --atlas-filter): the call's answer, and a time per launch."""
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=True)
    try:
        texels, pts, v, _, _ = AC.two_charts(C=2)
        want = AF.filter(texels, pts, v, AC.W2, AC.H2, 3)
        d_t, d_p, d_v, d_o = dev.upload(texels), dev.upload(pts), dev.upload(v), dev.upload(sentinel(want.size + TAIL))
        ms, p = (C.c_float * 8)(*([-1.0] * 8)), params(iterations=3)
        assert t._L.prt_hip_test_atlas_filter_profile(t._ctx, AC.W2, AC.H2, len(texels), d_t, d_p, d_v, 6, C.byref(p), d_o, ms) == 0, t._L.prt_hip_last_error()
        got = fetch(dev, d_o, want.size + TAIL)
        assert got[:want.size].tobytes() == want.tobytes() and (got[want.size:] == SENTINEL).all()
        assert all(ms[k] > 0 for k in (0, 1, 2, 3, 4, 7)) and ms[5] == 0 and ms[6] == 0, list(ms)
        assert t._L.prt_hip_test_atlas_filter_profile(t._ctx, AC.W2, AC.H2, len(texels), d_t, d_p + 8, d_v, 6, C.byref(p), d_o, ms) == -2
        assert t._L.prt_hip_test_atlas_filter_profile(t._ctx, AC.W2, AC.H2, len(texels), d_t, d_p, d_v, 6, C.byref(p), d_o, None) == -2
        assert t._L.prt_hip_test_atlas_filter_profile(t._ctx, AC.W2, AC.H2, len(texels), d_t, d_p, d_v, 6, C.byref(p), d_v, ms) == -2
    finally:
        t.close()


# ----------------------------------------------------------------------------- 6. end to end
def test_lightmap_with_a_filter_equals_the_five_calls(tracers):
    t, arrays = tracers("teapot")
    W, H, K, spp, seed, tile, gutter, bias = 64, 56, 16, 8, 977, 2, 2, 1e-3
    uvs = {}
    for m, mesh in enumerate(arrays):  # each mesh in a half of the atlas, a cell per triangle (tests/test_gpu_atlas.py scene_atlas)
        prims = len(mesh["indices"])
        G = int(np.ceil(np.sqrt(prims)))
        k = np.arange(prims)
        corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
        uv = ((np.stack([k % G, k // G], axis=1).astype(np.float64)[:, None, :] + corner[None]) / G).astype(F)
        uv[:, :, 0] = uv[:, :, 0] * F(0.5) + F(0.5) * m
        uvs[m] = uv
    rng = np.random.default_rng(9)
    sets = [prt_amd.bake_cosine_set(K, rng) for _ in range(tile * tile)]
    dirs, weights = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    p = params(iterations=3, npl2=4, sigma_l=3.0, sigma_p=2.0)
    kw = dict(seed=seed, bias=bias, set_tile=tile, gutter=gutter)
    filtered, f_mask = t.lightmap(uvs, W, H, dirs, weights, spp, filter=p, **kw)
    plain, p_mask = t.lightmap(uvs, W, H, dirs, weights, spp, **kw)
    assert filtered.shape == plain.shape == (H, W, 1, 3) and f_mask.tobytes() == p_mask.tobytes()
    # the calls composed here, on host arrays
    texels, hits, counts = t.atlas_rasterize(uvs, W, H)
    assert counts["n"] == len(texels) > 300
    pts = t.atlas_points(texels, hits, W, bias=bias, set_tile=tile)
    baked = t.bake(pts["P"], pts["N"], dirs, weights, spp, bias=pts["bias"], sets=pts["set"], seed=seed)
    composed, c_mask = t.atlas_resolve(texels, baked, W, H, gutter=gutter)
    BR.same_bytes(plain, composed, "lightmap() without a filter against the four calls")
    assert p_mask.tobytes() == c_mask.tobytes()
    smooth = t.atlas_filter(texels, pts, baked, W, H, p)
    composed_f, _ = t.atlas_resolve(texels, smooth, W, H, gutter=gutter)
    BR.same_bytes(filtered, composed_f, "lightmap(filter=p) against the five calls")
    BR.same_bytes(smooth, AF.filter(texels, pts, baked.reshape(len(texels), -1), W, H, 3, 4, 3.0, 2.0).reshape(smooth.shape), "the baked values against the restatement")
    owned = p_mask.reshape(-1) == 1
    changed = int((filtered.reshape(H * W, 3)[owned] != plain.reshape(H * W, 3)[owned]).any(axis=1).sum())
    print(f"lightmap of the teapot stage: {len(texels)} texels, {changed} changed by the filter")
    assert changed > 0
