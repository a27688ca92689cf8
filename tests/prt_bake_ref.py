"""The definition of include/prt_hip.h "baking" restated in numpy: rays(points, sets) and reduce(points, sets, L), float32 throughout,
every product rounded before the sum that uses it, vectorised over points, with the loop over k and the tree exactly as the header
orders them.  tests/test_bake_cpu.py pins this file against its own arithmetic; tests/test_gpu_bake.py holds the product to it byte
for byte.  Nothing here is product code.

Bytes and NaN.  IEEE 754 fixes every finite result, every infinity and where a NaN appears, but not which NaN an invalid operation
(inf * 0, inf - inf, 0 / 0) gives, nor which of two NaN operands survives: x86 gives the default NaN with the sign bit set and the
first operand's payload, gfx950 the default NaN with the sign bit clear.  same_bytes() therefore asks for equal bytes of every float
that is not a NaN in the restatement, and for a NaN -- any NaN -- where the restatement has one."""
import numpy as np

F = np.float32
U = np.uint32
POINT_DTYPE = np.dtype([("P", "<f4", 3), ("bias", "<f4"), ("N", "<f4", 3), ("set", "<u4")])
RAY_DTYPE = np.dtype([("org", "<f4", 3), ("tMax", "<f4"), ("dir", "<f4", 3), ("pad", "<u4")])


class Sets:
    """prt_bake_sets on the host: dirs (nSets, K, 3), weights (nSets, K, C) float32."""

    def __init__(self, dirs, weights):
        self.dirs = np.ascontiguousarray(dirs, dtype=F)
        self.weights = np.ascontiguousarray(weights, dtype=F)
        assert self.dirs.ndim == 3 and self.dirs.shape[2] == 3 and self.weights.ndim == 3 and self.weights.shape[:2] == self.dirs.shape[:2]
        self.nSets, self.K, self.C = self.weights.shape


def points(P, N, bias, sets=0):
    p = np.zeros(len(P), dtype=POINT_DTYPE)
    p["P"], p["N"], p["bias"], p["set"] = np.asarray(P, F), np.asarray(N, F), np.asarray(bias, F), np.asarray(sets, U)
    return p


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def normalize3(v):
    inv = F(1.0) / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return inv[..., None] * v


def frames(N):
    """(T, B) of normals N (n, 3) float32: the bounce loop's frame (path_tracer.cpp:147-153), N as given."""
    N = np.asarray(N, dtype=F)
    with np.errstate(all="ignore"):
        u = np.where((np.abs(N[:, 0]) > F(0.1))[:, None], np.array([0, 1, 0], F), np.array([1, 0, 0], F)).astype(F)
        T = normalize3(cross3(N, u))
        B = normalize3(cross3(T, N))
    assert T.dtype == F and B.dtype == F
    return T, B


def rays(pts, sets):
    """(n * K,) RAY_DTYPE: ray i*K + k of point i."""
    n, K = len(pts), sets.K
    P, N, bias, s = pts["P"], pts["N"], pts["bias"], pts["set"]
    out = np.zeros((n, K), dtype=RAY_DTYPE)  # set >= nSets: org = dir = 0; tMax = 0, pad = 0
    ok = s < sets.nSets
    d = np.zeros((n, K, 3), dtype=F)
    d[ok] = sets.dirs[s[ok]]
    T, B = frames(N)
    with np.errstate(all="ignore"):
        Nk, Tk, Bk = N[:, None, :], T[:, None, :], B[:, None, :]
        framed_dir = (d[:, :, 0:1] * Bk + d[:, :, 1:2] * Tk) + d[:, :, 2:3] * Nk
        framed_org = np.broadcast_to((P + bias[:, None] * N)[:, None, :], (n, K, 3))
    identity = ((N[:, 0] == 0) & (N[:, 1] == 0) & (N[:, 2] == 0))[:, None, None]
    org = np.where(identity, np.broadcast_to(P[:, None, :], (n, K, 3)), framed_org)
    dr = np.where(identity, d, framed_dir)
    assert org.dtype == F and dr.dtype == F
    out["org"][ok], out["dir"][ok] = org[ok], dr[ok]
    return out.reshape(-1)


def reduce(pts, sets, L):
    """(n, C, 3) float32 from the per-ray radiance L (n * K, 3): one wavefront per point, lane l sums k = l, l + 64, ... in order, then
    the tree step = 32 .. 1, a_l = a_l + a_(l + step) for l < step."""
    n, K, C = len(pts), sets.K, sets.C
    L = np.ascontiguousarray(L, dtype=F).reshape(n, K, 3)
    s = pts["set"]
    ok = s < sets.nSets
    w = np.zeros((n, K, C), dtype=F)
    w[ok] = sets.weights[s[ok]]
    a = np.zeros((n, 64, C, 3), dtype=F)  # 1. a_l = +0
    with np.errstate(all="ignore"):
        for k0 in range(0, K, 64):  # 2. trip k0 / 64 of every lane that still has a k
            m = min(64, K - k0)
            a[:, :m] = a[:, :m] + (w[:, k0:k0 + m, :, None] * L[:, k0:k0 + m, None, :])
        step = 32
        while step >= 1:  # 3.
            a[:, :step] = a[:, :step] + a[:, step:2 * step]
            step //= 2
    out = a[:, 0].copy()  # 4.
    out[~ok] = F(0.0)
    assert out.dtype == F
    return out


def same_bytes(got, want, what):
    """Equal bytes of every float that is not a NaN in `want`; a NaN where `want` has one (see the module's docstring)."""
    g = np.ascontiguousarray(got).view(U).reshape(-1)
    w = np.ascontiguousarray(want).view(U).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    nan = (w & U(0x7fffffff)) > U(0x7f800000)
    bad = np.nonzero(np.where(nan, (g & U(0x7fffffff)) <= U(0x7f800000), g != w))[0]
    if len(bad):
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} words differ, first at {bad[:6]}: {g[bad[:6]]} != {w[bad[:6]]}")
    return int(nan.sum())


# ----------------------------------------------------------------------------- the two set helpers, restated
def sh9(d):
    x, y, z = (np.asarray(d, dtype=np.float64)[:, k] for k in range(3))
    c0, c1, c2, c3, c4 = 0.5 * np.sqrt(1 / np.pi), np.sqrt(3 / (4 * np.pi)), 0.5 * np.sqrt(15 / np.pi), 0.25 * np.sqrt(5 / np.pi), 0.25 * np.sqrt(15 / np.pi)
    return np.stack([c0 + 0 * x, c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z, c4 * (x * x - y * y)], axis=1)


def bake_cosine_set(K, rng):
    """K cosine-weighted directions about +z and weights pi / K: irradiance."""
    u1, u2 = rng.random(K), rng.random(K)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - u1)], axis=1).astype(F), np.full((K, 1), np.pi / K, dtype=F)


def bake_sh9_set(K, rng):
    """K uniform directions on the sphere and weights 4 pi / K * Y_c(d_k): SH9 coefficients."""
    z, phi = rng.uniform(-1, 1, K), rng.uniform(0, 2 * np.pi, K)
    r = np.sqrt(1 - z * z)
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(F)
    return d, (4 * np.pi / K * sh9(d)).astype(F)
