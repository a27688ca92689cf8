"""Baking without a GPU (include/prt_hip.h "baking"; the GPU half is tests/test_gpu_bake.py): the three entry points are declared,
documented and exported, and the numpy restatement the GPU tests hold the product to (tests/prt_bake_ref.py) is pinned against its
own arithmetic and against what the direction sets are for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_bake_ref as BR
import prt_testlib as T

F = np.float32
NAMES = ("prt_hip_bake_rays", "prt_hip_bake_reduce", "prt_hip_bake")


# ----------------------------------------------------------------------------- the interface
def test_header_declares_the_entry_points_and_carries_the_rules():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    section = src[src.index("---- baking"):]
    flat = re.sub(r"\s+", " ", section)
    for decl in ("int prt_hip_bake_rays(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, "
                 "prt_ray* rays /* n*K */, uint32_t flags, void* stream);",
                 "int prt_hip_bake_reduce(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, "
                 "const float* radiance /* 3*n*K */, float* out /* 3*C*n */, uint32_t flags, void* stream);",
                 "int prt_hip_bake(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, "
                 "const prt_render_params* params, float* out /* 3*C*n */, uint32_t flags, void* stream);",
                 "typedef struct { float P[3]; float bias; float N[3]; uint32_t set; } prt_bake_point;"):
        assert decl in flat, decl
    text = re.sub(r"[\s*]+", " ", section)  # (comment stars and line breaks go; so does every '*' of a formula)
    for rule in ("if all three components of N compare equal to 0: org = P, dir = d",  # the frame formula
                 "u = fabsf(N.x) > 0.1f ? (0,1,0) : (1,0,0)", "T = normalize3(cross3(N, u))", "B = normalize3(cross3(T, N))",
                 "dir = (d.x B + d.y T) + d.z N per component, with N as given and not normalised", "org = P + bias N per component",
                 "tMax = 0, pad = 0",
                 "for lane l = 0..63, for channel c and colour component h: a_l = +0",  # the reduce order
                 "for k = l, l+64, l+128, ... < K: a_l = a_l + (weights[(s K + k) C + c] L[3r + h])",
                 "for step = 32, 16, 8, 4, 2, 1, for l < step: a_l = a_l + a_(l+step)", "out[(i C + c) 3 + h] = a_0",
                 "n = 0 or n K > 2^24", "batches beyond 2^24 rays",  # the limit
                 "set >= nSets is never followed: the point's K rays get org = dir = 0",  # the out-of-range set
                 "A point with set >= nSets writes +0 to all its 3 C floats",
                 "probe r under seed + r", "K outside 1 .. 4096, C outside 1 .. 16, nSets outside 1 .. 1024", "reserved != 0"):
        assert rule in text, rule


def test_the_entry_points_are_exported_and_wrapped():
    prt_amd.build()
    for name in NAMES:
        assert name in prt_amd.EXPORTS
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in NAMES:
            assert f" T {name}\n" in syms, (path, name)
    assert "prt_bake.hip" in prt_amd._build.SOURCES
    for method in ("bake", "bake_async", "bake_rays", "bake_reduce"):
        assert callable(getattr(prt_amd.PathTracer, method))
    assert prt_amd.BAKE_POINT_DTYPE.itemsize == 32 and prt_amd.BAKE_POINT_DTYPE == BR.POINT_DTYPE
    assert C.sizeof(prt_amd.BakeSets) == 32 and prt_amd.BakeSets.dirs.offset == 16 and prt_amd.BakeSets.weights.offset == 24


def test_the_calls_fail_loudly_without_a_context():
    """As the queries: PRT_HIP_ENODEVICE where no device exists, PRT_HIP_EINVAL for a NULL context where one does."""
    prt_amd.build()
    L = prt_amd.lib()
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    table = prt_amd.BakeSets(K=1, C=1, nSets=1, reserved=0, dirs=buf.ctypes.data, weights=buf.ctypes.data)
    rp = prt_amd.RenderParams()
    rp.samples, rp.nranks = 8, 1
    assert L.prt_hip_bake_rays(None, 1, p, C.byref(table), p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_bake_reduce(None, 1, p, C.byref(table), p, p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_bake(None, 1, p, C.byref(table), C.byref(rp), p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_last_error()


def test_python_helpers_shape_their_arguments():
    pts = prt_amd.make_bake_points(np.ones((5, 3)), np.zeros((5, 3)), 0.5, sets=[0, 1, 2, 3, 4])
    assert pts.dtype == prt_amd.BAKE_POINT_DTYPE and pts["bias"].tolist() == [0.5] * 5 and pts["set"].tolist() == [0, 1, 2, 3, 4]
    d, w, t = prt_amd.make_bake_sets(np.zeros((7, 3)), np.ones(7))
    assert (d.shape, w.shape, t.K, t.C, t.nSets, t.reserved) == ((1, 7, 3), (1, 7, 1), 7, 1, 1, 0)
    d, w, t = prt_amd.make_bake_sets(np.zeros((2, 7, 3)), np.ones((2, 7, 9)))
    assert (t.K, t.C, t.nSets, t.dirs, t.weights) == (7, 9, 2, d.ctypes.data, w.ctypes.data)
    with pytest.raises(prt_amd.PrtError):
        prt_amd.make_bake_sets(np.zeros((7, 3)), np.ones((2, 6, 1)))


# ----------------------------------------------------------------------------- the restatement: rays
def test_frames_of_unit_normals_are_orthonormal():
    rng = np.random.default_rng(1)
    N = rng.normal(size=(1000, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    N[:4, 0] = [0.1, -0.1, 0.10000001, 0.0]  # both sides of the threshold (the rows are no longer quite unit: renormalise)
    N = (N / np.linalg.norm(N.astype(np.float64), axis=1, keepdims=True)).astype(F)
    Tn, Bn = BR.frames(N)
    M = np.stack([Bn, Tn, N], axis=1).astype(np.float64)
    err = np.abs(M @ M.transpose(0, 2, 1) - np.eye(3)).max()
    print("largest deviation of a frame from orthonormal:", err)
    assert err <= 1e-6
    assert (np.linalg.det(M) > 0.99).all(), "right-handed: B x T = N"


def test_a_zero_normal_is_the_identity_frame_bit_for_bit():
    rng = np.random.default_rng(2)
    d = rng.normal(size=(1, 5, 3)).astype(F)
    d[0, 0] = [-0.0, 1e-40, np.inf]
    P = rng.normal(size=(3, 3)).astype(F)
    N = np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [0, 0, 1]], F)
    r = BR.rays(BR.points(P, N, 0.25), BR.Sets(d, np.ones((1, 5, 1), F))).reshape(3, 5)
    for i in (0, 1):
        assert r["dir"][i].tobytes() == d[0].tobytes() and r["org"][i].tobytes() == np.broadcast_to(P[i], (5, 3)).tobytes()
    assert r["org"][2].tobytes() == np.broadcast_to(P[2] + F(0.25) * N[2], (5, 3)).astype(F).tobytes()
    assert not r["tMax"].any() and not r["pad"].any()


def test_rays_follow_the_frame_and_never_an_outside_set():
    rng = np.random.default_rng(3)
    d = rng.normal(size=(2, 4, 3)).astype(F)
    P, N = rng.normal(size=(6, 3)).astype(F), rng.normal(size=(6, 3)).astype(F)
    sets = np.array([0, 1, 2, 0xffffffff, 1, 0], np.uint32)
    pts = BR.points(P, N, -0.5, sets)
    r = BR.rays(pts, BR.Sets(d, np.ones((2, 4, 1), F))).reshape(6, 4)
    assert not r["org"][2:4].any() and not r["dir"][2:4].any()
    Tn, Bn = BR.frames(N)
    for i in (0, 1, 4, 5):
        for k in range(4):
            dd = d[sets[i], k]
            want = (dd[0] * Bn[i] + dd[1] * Tn[i]) + dd[2] * N[i]
            assert r["dir"][i, k].tobytes() == want.astype(F).tobytes()
        assert r["org"][i, 0].tobytes() == (P[i] + F(-0.5) * N[i]).tobytes()


# ----------------------------------------------------------------------------- the restatement: reduce
def three_lines(w, L):
    """reduce for one point and one channel, by hand: (K,) weights, (K, 3) radiance."""
    a = [sum((F(w[k]) * L[k] for k in range(l, len(w), 64)), np.zeros(3, F)) for l in range(64)]
    for step in (32, 16, 8, 4, 2, 1):
        a[:step] = [a[l] + a[l + step] for l in range(step)]
    return a[0]


@pytest.mark.parametrize("K", [1, 64, 65])
def test_reduce_equals_the_hand_written_version(K):
    rng = np.random.default_rng(K)
    n, Cc = 3, 2
    w = rng.normal(size=(1, K, Cc)).astype(F)
    L = rng.normal(size=(n * K, 3)).astype(F)
    got = BR.reduce(BR.points(np.zeros((n, 3)), np.zeros((n, 3)), 0), BR.Sets(np.zeros((1, K, 3)), w), L)
    assert got.shape == (n, Cc, 3) and got.dtype == F
    for i in range(n):
        for c in range(Cc):
            want = three_lines(w[0, :, c], L[i * K:(i + 1) * K])
            assert want.dtype == F and got[i, c].tobytes() == want.tobytes(), (i, c)


@pytest.mark.parametrize("K", [1, 63, 130, 4096])
def test_reduce_is_within_the_bound_of_an_f64_sum(K):
    """Every one of the at most K roundings of a sum (one per product, one per add) is relative 2^-24 of a partial result no larger
    than sum |w L| (1 + K 2^-24): K 2^-23 sum |w L| covers it."""
    rng = np.random.default_rng(K)
    n, Cc = 4, 3
    w = rng.normal(size=(2, K, Cc)).astype(F)
    L = rng.gamma(1.0, 2.0, size=(n * K, 3)).astype(F)
    s = np.array([0, 1, 1, 2], np.uint32)
    got = BR.reduce(BR.points(np.zeros((n, 3)), np.zeros((n, 3)), 0, s), BR.Sets(np.zeros((2, K, 3)), w), L)
    assert got[3].tobytes() == np.zeros((Cc, 3), F).tobytes(), "set 2 of 2 sets: +0"
    for i in range(3):
        prod = w[s[i]].astype(np.float64)[:, :, None] * L.reshape(n, K, 3)[i].astype(np.float64)[:, None, :]
        err = np.abs(got[i] - prod.sum(axis=0))
        bound = K * 2.0 ** -23 * np.abs(prod).sum(axis=0)
        assert (err <= bound).all(), (i, err.max(), bound.min())


def test_a_nan_weight_stays_in_its_point():
    K = 70
    rng = np.random.default_rng(5)
    w = rng.normal(size=(2, K, 1)).astype(F)
    w[1, 69, 0] = np.nan
    L = rng.normal(size=(3 * K, 3)).astype(F)
    got = BR.reduce(BR.points(np.zeros((3, 3)), np.zeros((3, 3)), 0, [0, 1, 0]), BR.Sets(np.zeros((2, K, 3)), w), L)
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


# ----------------------------------------------------------------------------- the set helpers
SET_HELPERS = {"restated": (BR.bake_cosine_set, BR.bake_sh9_set), "prt_amd": (prt_amd.bake_cosine_set, prt_amd.bake_sh9_set)}


@pytest.mark.parametrize("which", sorted(SET_HELPERS))
def test_cosine_set_weights_sum_to_pi_and_its_directions_are_cosine_weighted(which):
    K = 4096
    d, w = SET_HELPERS[which][0](K, np.random.default_rng(7))
    assert d.shape == (K, 3) and w.shape == (K, 1) and d.dtype == F and w.dtype == F
    assert abs(float(w.astype(np.float64).sum()) - np.pi) <= K * 2.0 ** -24 * np.pi  # (each weight is pi / K rounded to float32)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6 and (d[:, 2] >= 0).all()
    # under pdf cos / pi the mean of cos is 2/3 with variance 1/2 - 4/9 = 1/18: five standard errors
    assert abs(d[:, 2].astype(np.float64).mean() - 2 / 3) <= 5 * np.sqrt(1 / 18 / K)


@pytest.mark.parametrize("which", sorted(SET_HELPERS))
def test_sh9_set_reproduces_the_coefficients_of_a_constant_and_of_a_linear_field(which):
    """L(d) = a + b . d has the coefficients (a sqrt(4 pi), b_y sqrt(4 pi / 3), b_z ..., b_x ..., 0, 0, 0, 0, 0).  The estimate of
    coefficient c is the mean of K independent terms X = 4 pi L(d) Y_c(d) with d uniform, so its standard error is sqrt(Var X / K)
    with Var X <= E X^2 <= (4 pi)^2 max|L|^2 E Y_c^2 = 4 pi max|L|^2 (the basis is orthonormal: E Y_c^2 = 1 / (4 pi)).  The bound
    is five of those: 5 max|L| sqrt(4 pi / K) -- at K = 4096, 0.277 max|L|; the reduce's own rounding (K 2^-23 of sum |w L|) is four
    orders of magnitude below it."""
    K = 4096
    d, w = SET_HELPERS[which][1](K, np.random.default_rng(8))
    assert d.shape == (K, 3) and w.shape == (K, 9) and d.dtype == F and w.dtype == F
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    sets = BR.Sets(d[None], w[None])
    pts = BR.points(np.zeros((2, 3)), np.zeros((2, 3)), 0)
    a, b = 1.5, np.array([0.5, -1.0, 0.25])
    field = np.stack([np.full(K, a), a + d.astype(np.float64) @ b])  # the two points: constant, linear
    L = np.repeat(field.reshape(2 * K, 1), 3, axis=1).astype(F)
    got = BR.reduce(pts, sets, L)[:, :, 0].astype(np.float64)
    want = np.zeros((2, 9))
    want[:, 0] = a * np.sqrt(4 * np.pi)
    want[1, 1:4] = np.sqrt(4 * np.pi / 3) * b[[1, 2, 0]]
    for i, peak in enumerate((a, a + np.abs(b).sum())):
        bound = 5 * peak * np.sqrt(4 * np.pi / K)
        print(f"{which} point {i}: largest error {np.abs(got[i] - want[i]).max():.4f}, bound {bound:.4f}")
        assert (np.abs(got[i] - want[i]) <= bound).all(), (i, got[i], want[i])
    assert abs(got[0, 0] - want[0, 0]) <= 1e-3, "the constant term of a constant field has no variance: the weights of Y_0 sum to sqrt(4 pi)"
