"""numpy restatement of the denoiser of include/prt_hip.h ("denoised previews"), written from that text: float32 throughout, one
array operation per operation of the header, the 25 taps as 25 shifted-array passes in the header's tap order (dy outer, dx inner),
so that every sum is accumulated in the order the header fixes.  numpy's float32 +, -, *, / and sqrt are correctly rounded and
numpy never contracts a multiply and an add, which is what the header asks of an implementation."""
import numpy as np

F = np.float32
H_TAPS = {-2: F(0.0625), -1: F(0.25), 0: F(0.375), 1: F(0.25), 2: F(0.0625)}
G_TAPS = {-1: F(0.25), 0: F(0.5), 1: F(0.25)}  # the 3x3 weights {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; ...} are products of these


def lum(c):
    return F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]


def f(x):
    y = F(0.125) * x
    r = F(1.0) / ((F(1.0) + y) + (F(0.5) * y) * y)
    r = r * r
    r = r * r
    r = r * r
    return r


def shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that is inside the image, else fill."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return b


def guide_average(planes):
    """g = g_0; g = g + g_k; g = g * (1.0f / K)"""
    g = np.asarray(planes[0], dtype=F).copy()
    for p in planes[1:]:
        g = g + np.asarray(p, dtype=F)
    return (g * (F(1.0) / F(len(planes)))).astype(F)


def denoise(total, count, mom, albedo, normal, iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True,
            exposure=1.0):
    """total (H, W, 3) f32 sums, count (H, W) u32, mom (H, W, 4) f32 {mean, M2, bits(m), 0}, albedo / normal (H, W, 3) guide planes.
    Returns (image (H, W, 3), V_final (H, W))."""
    total = np.asarray(total, dtype=F)
    count = np.asarray(count, dtype=np.uint32)
    mom = np.ascontiguousarray(mom, dtype=F)
    A = np.asarray(albedo, dtype=F)
    G = np.asarray(normal, dtype=F)
    sig_l, sig_a = F(sigma_luminance), F(sigma_albedo)
    sig_a2 = sig_a * sig_a
    with np.errstate(all="ignore"):
        valid = count > 0
        miss = (G[..., 0] == 0) & (G[..., 1] == 0) & (G[..., 2] == 0)
        N = np.where(miss[..., None], F(0), (G - F(0.5)) * F(2.0)).astype(F)
        c = (total / count.astype(F)[..., None]).astype(F)
        m = mom[..., 2].view(np.uint32)
        v = (mom[..., 1] / (m.astype(np.int64) - 1).astype(F)) / (count >> 3).astype(F)
        v = np.where(m >= 2, v, F(-1)).astype(F)
        if demodulate:
            d = np.where(A > F(0.015625), A, F(0.015625)).astype(F)  # the header's max(a, b) = a > b ? a : b: 1/64 for a NaN albedo
            C = (c / d).astype(F)
            ld = lum(d)
            V = np.where(v < 0, F(-1), v / (ld * ld)).astype(F)
        else:
            d = np.ones_like(A)
            C, V = c, v
        C = np.where(valid[..., None], C, F(0)).astype(F)  # an invalid pixel is never read as a tap; keep it finite
        V = np.where(valid, V, F(-1)).astype(F)
        for i in range(iterations):
            s = 1 << i
            known = V >= 0
            L = lum(C)
            sum_vw = np.zeros(V.shape, F)
            sum_wt = np.zeros(V.shape, F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    wt = G_TAPS[dy] * G_TAPS[dx]
                    Vq = shifted(V, dx, dy, F(-1))
                    ok = shifted(valid, dx, dy, False) & (Vq >= 0)
                    sum_vw = np.where(ok, sum_vw + wt * Vq, sum_vw)
                    sum_wt = np.where(ok, sum_wt + wt, sum_wt)
            g = sum_vw / sum_wt
            den = sig_l * np.sqrt(g) + F(1e-6)
            sum_w = np.zeros(V.shape, F)
            sum_c = np.zeros(C.shape, F)
            sum_v = np.zeros(V.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = s * dx, s * dy
                    ok = shifted(valid, ox, oy, False)
                    if not ok.any():
                        continue
                    Cq = shifted(C, ox, oy, F(0))
                    Vq = shifted(V, ox, oy, F(-1))
                    if dx == 0 and dy == 0:
                        w = np.full(V.shape, H_TAPS[0] * H_TAPS[0], F)
                    else:
                        Nq = shifted(N, ox, oy, F(0))
                        Aq = shifted(A, ox, oy, F(0))
                        dn = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                        wn = np.where(dn > 0, dn, F(0))
                        for _ in range(normal_power_log2):
                            wn = wn * wn
                        da = A - Aq
                        wa = f(((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) / sig_a2)
                        wl = np.where(known, f(np.abs(L - lum(Cq)) / den), F(1.0))
                        w = ((((H_TAPS[dy] * H_TAPS[dx]) * wn) * wa) * wl).astype(F)
                    sum_w = np.where(ok, sum_w + w, sum_w)
                    sum_c = np.where(ok[..., None], sum_c + w[..., None] * Cq, sum_c)
                    sum_v = np.where(ok & known, sum_v + (w * w) * np.where(Vq >= 0, Vq, V), sum_v)
            C = np.where(valid[..., None], sum_c / sum_w[..., None], F(0)).astype(F)
            V = np.where(valid & known, sum_v / (sum_w * sum_w), F(-1)).astype(F)
        image = np.where(valid[..., None], F(exposure) * (C * d), F(0)).astype(F)
    return image, V


# the parameters the tests run the filter with unless they say otherwise
DEFAULTS = dict(iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True)
