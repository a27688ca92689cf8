"""The lightmap filter restated in numpy (include/prt_hip.h "lightmap filter"): every operation in float32 in the header's order, one
rounding per operation, vectorised over the points and looped over the taps.  The GPU tests hold prt_hip_atlas_filter to it and the
CPU tests hold it to tests/atlas_filter_main.cpp (the kernels' own text compiled for the host), both at tolerance 0, compared as
bytes; where this has a NaN any NaN is accepted (prt_bake_ref.same_bytes)."""
import numpy as np

F = np.float32
U = np.uint32
NONE = 0xffffffff
POINT_DTYPE = np.dtype([("P", "<f4", 3), ("bias", "<f4"), ("N", "<f4", 3), ("set", "<u4")])
H_TAP = {0: F(0.375), 1: F(0.25), 2: F(0.0625)}


def f(x):
    y = F(0.125) * x
    r = F(1.0) / ((F(1.0) + y) + (F(0.5) * y) * y)
    r = r * r
    r = r * r
    r = r * r
    return r


def lum(v):
    return (F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]) + F(0.0722) * v[..., 2]


def eligible(texels, points, values, W, H):
    ok = texels.astype(np.int64) < W * H
    ok &= points["set"] != U(NONE)
    ok &= np.isfinite(points["P"]).all(axis=1) & np.isfinite(points["N"]).all(axis=1) & np.isfinite(values).all(axis=1)
    return ok


def build_map(texels, ok, W, H):
    """map[t]: the smallest eligible q with texels[q] == t, or NONE."""
    m = np.full(W * H, NONE, dtype=np.int64)
    q = np.nonzero(ok)[0]
    np.minimum.at(m, texels[q].astype(np.int64), q)
    return m


def placed(texels, points, values, W, H):
    """(placed (n,) bool, map (W*H,) int64)."""
    ok = eligible(texels, points, values, W, H)
    m = build_map(texels, ok, W, H)
    q = np.arange(len(texels))
    return ok & (m[np.where(ok, texels, 0).astype(np.int64)] == q), m


class _Taps:
    """The placed points q (global indices), their texel coordinates, and nb(q, dx, dy)."""

    def __init__(self, texels, points, values, W, H):
        self.W, self.H = W, H
        self.is_placed, self.map = placed(texels, points, values, W, H)
        self.q = np.nonzero(self.is_placed)[0]
        t = texels[self.q].astype(np.int64)
        self.x, self.y = t % W, t // W
        self.P, self.N = points["P"].astype(F), points["N"].astype(F)

    def nb(self, dx, dy):
        """(exists (m,) bool, r (m,) global index, 0 where none)."""
        nx, ny = self.x + dx, self.y + dy
        inside = (nx >= 0) & (ny >= 0) & (nx < self.W) & (ny < self.H)
        r = self.map[np.where(inside, ny * self.W + nx, 0)]
        have = inside & (r != NONE)
        return have, np.where(have, r, 0)

    def d2(self, r):
        e = self.P[r] - self.P[self.q]
        return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]

    def geo(self, r, inv_p, npl2):
        Nq, Nr = self.N[self.q], self.N[r]
        dn = (Nq[:, 0] * Nr[:, 0] + Nq[:, 1] * Nr[:, 1]) + Nq[:, 2] * Nr[:, 2]
        wn = np.where(dn > 0, dn, F(0.0)).astype(F)
        for _ in range(npl2):
            wn = wn * wn
        d2 = self.d2(r)
        wp = np.where(d2 == 0, F(1.0), f(d2 * inv_p)).astype(F)
        return wn * wp


def footprint(T):
    f2 = np.full(len(T.q), np.inf, dtype=F)
    taken = np.zeros(len(T.q), bool)
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        have, r = T.nb(dx, dy)
        d2 = T.d2(r)
        take = have & (d2 > 0) & (d2 < f2)
        f2 = np.where(take, d2, f2).astype(F)
        taken |= take
    return np.where(taken, f2, F(0.0)).astype(F)


def inv_p(sig_p2, s, f2):
    return F(1.0) / ((sig_p2 * F(s * s)) * f2)


def variance(T, values, f2, sig_p2, npl2):
    m = len(T.q)
    ip = inv_p(sig_p2, 1, f2)
    L = lum(values)
    taps = []
    sw, sl = np.zeros(m, F), np.zeros(m, F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            have, r = T.nb(dx, dy)
            g = np.ones(m, F) if dx == 0 and dy == 0 else T.geo(r, ip, npl2)
            taps.append((have, g, L[r]))
            sw = np.where(have, sw + g, sw).astype(F)
            sl = np.where(have, sl + g * L[r], sl).astype(F)
    m1 = sl / sw
    sv = np.zeros(m, F)
    for have, g, lr in taps:
        d = lr - m1
        sv = np.where(have, sv + g * (d * d), sv).astype(F)
    return sv / sw


def filter(texels, points, values, W, H, iterations=5, npl2=5, sigma_l=4.0, sigma_p=4.0, stages=None):
    """out (n, stride) float32.  stages (a list): receives (C, V) after every iteration, V0 first."""
    texels = np.ascontiguousarray(texels, dtype=U).reshape(-1)
    points = np.ascontiguousarray(points).view(POINT_DTYPE).reshape(-1)
    n = len(texels)
    values = np.ascontiguousarray(values, dtype=F).reshape(n, -1)
    stride = values.shape[1]
    assert stride % 3 == 0 and len(points) == n
    out = values.copy()
    with np.errstate(all="ignore"):
        T = _Taps(texels, points, values, W, H)
        q, m = T.q, len(T.q)
        if m == 0:
            return out
        sig_l, sig_p2 = F(sigma_l), F(sigma_p) * F(sigma_p)
        f2 = footprint(T)
        C = values.copy()
        V = np.zeros(n, F)
        V[q] = variance(T, values, f2, sig_p2, npl2)
        if stages is not None:
            stages.append((C.copy(), V.copy()))
        for i in range(iterations):
            s = 1 << i
            ip = inv_p(sig_p2, s, f2)
            a, b = np.zeros(m, F), np.zeros(m, F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    have, r = T.nb(dx, dy)
                    wt = (F(0.5) if dx == 0 else F(0.25)) * (F(0.5) if dy == 0 else F(0.25))
                    a = np.where(have, a + wt * V[r], a).astype(F)
                    b = np.where(have, b + wt, b).astype(F)
            inv_den = F(1.0) / (sig_l * np.sqrt(a / b) + F(1e-6))
            L = lum(C)
            sumW, sumV, S = np.zeros(m, F), np.zeros(m, F), np.zeros((m, stride), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    have, r = T.nb(dx * s, dy * s)
                    if dx == 0 and dy == 0:
                        w = np.full(m, F(0.375) * F(0.375), F)
                    else:
                        w = ((H_TAP[abs(dy)] * H_TAP[abs(dx)]) * T.geo(r, ip, npl2)) * f(np.abs(L[q] - L[r]) * inv_den)
                    sumW = np.where(have, sumW + w, sumW).astype(F)
                    S = np.where(have[:, None], S + w[:, None] * C[r], S).astype(F)
                    sumV = np.where(have, sumV + (w * w) * V[r], sumV).astype(F)
            C2, V2 = C.copy(), V.copy()
            C2[q] = S / sumW[:, None]
            V2[q] = sumV / (sumW * sumW)
            C, V = C2, V2
            if stages is not None:
                stages.append((C.copy(), V.copy()))
        out[q] = C[q]
    return out
