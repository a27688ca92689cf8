"""numpy restatement of the temporal stage of include/prt_hip.h ("temporal reprojection"), written from that text: float32
throughout, one array operation per operation of the header, the four taps as four gathers in the header's order (j outer, i inner).
The spatial stage mirrors prt_denoise_ref.denoise from its planes (C0, V0) on: the same iterations, operation for operation.  numpy's
float32 +, -, *, / and sqrt are correctly rounded and numpy never contracts a multiply and an add, which is what the header asks."""
import numpy as np

import prt_denoise_ref as R

F = np.float32
lum = R.lum


def dot3(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def camera_fields(cam):
    """pos, dir, up, right as float32 (3,) arrays from a prt_amd.CameraDesc or a dict with those keys."""
    get = (lambda k: cam[k]) if isinstance(cam, dict) else (lambda k: getattr(cam, k))
    return {k: np.array([F(v) for v in get(k)], dtype=F) for k in ("pos", "dir", "up", "right")}


def centre_directions(cam, width, height):
    """dirp of every pixel (H, W, 3): camera_dir with both jitter terms 0.0f.  cam also carries invWidth / invHeight."""
    get = (lambda k: cam[k]) if isinstance(cam, dict) else (lambda k: getattr(cam, k))
    c = camera_fields(cam)
    inv_w, inv_h = F(get("invWidth")), F(get("invHeight"))
    k_aspect = F(width) / F(height)
    x = np.arange(width, dtype=np.uint32).astype(F)[None, :]
    y = np.arange(height, dtype=np.uint32).astype(F)[:, None]
    nx = F(2.0) * (x * inv_w - F(0.5) + F(0.0)) * F(0.6) * k_aspect
    ny = F(-2.0) * (y * inv_h - F(0.5) + F(0.0)) * F(0.6)
    nx = np.broadcast_to(nx, (height, width)).astype(F)
    ny = np.broadcast_to(ny, (height, width)).astype(F)
    v = ((nx[..., None] * c["right"] + ny[..., None] * c["up"]) + c["dir"]).astype(F)
    inv = F(1.0) / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return (inv[..., None] * v).astype(F)


def position_plane(cam, width, height, t):
    """{X, t} (H, W, 4) from the hit distances t (H, W; -1 = miss): X = pos + t*dirp, a miss is {0, 0, 0, -1}."""
    d = centre_directions(cam, width, height)
    t = np.asarray(t, dtype=F)
    X = (camera_fields(cam)["pos"] + t[..., None] * d).astype(F)
    hit = t != F(-1)
    out = np.zeros((height, width, 4), F)
    out[..., :3] = np.where(hit[..., None], X, F(0))
    out[..., 3] = np.where(hit, t, F(-1))
    return out


def prepare(total, count, mom, albedo, normal):
    """valid, c, v, N, A, d_demod of "denoised previews"; an invalid pixel has c = 0 and v = -1."""
    total = np.asarray(total, dtype=F)
    count = np.asarray(count, dtype=np.uint32)
    mom = np.ascontiguousarray(mom, dtype=F)
    A = np.asarray(albedo, dtype=F)
    G = np.asarray(normal, dtype=F)
    valid = count > 0
    miss = (G[..., 0] == 0) & (G[..., 1] == 0) & (G[..., 2] == 0)
    N = np.where(miss[..., None], F(0), (G - F(0.5)) * F(2.0)).astype(F)
    c = (total / count.astype(F)[..., None]).astype(F)
    m = mom[..., 2].view(np.uint32)
    v = (mom[..., 1] / (m.astype(np.int64) - 1).astype(F)) / (count >> 3).astype(F)
    v = np.where(m >= 2, v, F(-1)).astype(F)
    c = np.where(valid[..., None], c, F(0)).astype(F)
    v = np.where(valid, v, F(-1)).astype(F)
    return valid, c, v, N, A


def merge(total, count, mom, albedo, normal, position, history=None, position_tolerance=0.01, normal_cos=0.9, max_history=256.0):
    """The per-pixel block of the header up to (cm, vm, len).  history = None or dict(camera=..., color_var, pos_len, normal) with
    (H, W, 4) planes.  Returns dict(valid, cm, vm, len, have, N, A, pending=(color_var, pos_len, normal), fx, fy)."""
    with np.errstate(all="ignore"):
        valid, c, v, N, A = prepare(total, count, mom, albedo, normal)
        h, w = valid.shape
        P = np.ascontiguousarray(position, dtype=F).reshape(h, w, 4)
        X, t = P[..., :3], P[..., 3]
        tol, ncos, maxh = F(position_tolerance), F(normal_cos), F(max_history)
        n = count.astype(F) if isinstance(count, np.ndarray) else np.asarray(count, dtype=np.uint32).astype(F)
        geom = valid & (t >= 0)
        have = np.zeros((h, w), bool)
        cm, vm = c.copy(), v.copy()
        ln = np.where(valid, n, F(0)).astype(F)
        fx = np.full((h, w), np.nan, F)
        fy = np.full((h, w), np.nan, F)
        if history is not None and maxh > 0:
            hc = camera_fields(history["camera"])
            hC = np.ascontiguousarray(history["color_var"], dtype=F).reshape(h, w, 4)
            hX = np.ascontiguousarray(history["pos_len"], dtype=F).reshape(h, w, 4)
            hN = np.ascontiguousarray(history["normal"], dtype=F).reshape(h, w, 4)
            e = (X - hc["pos"]).astype(F)
            a = dot3(e, hc["right"])
            b = dot3(e, hc["up"])
            z = dot3(e, hc["dir"])
            k_aspect = F(w) / F(h)
            fx = ((a / z) / ((F(2.0) * F(0.6)) * k_aspect) + F(0.5)) * F(w)
            fy = (F(0.5) - (b / z) / (F(2.0) * F(0.6))) * F(h)
            inside = geom & (z > 0) & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
            fxs = np.where(inside, fx, F(0)).astype(F)
            fys = np.where(inside, fy, F(0)).astype(F)
            ix, iy = np.floor(fxs), np.floor(fys)
            tx, ty = (fxs - ix).astype(F), (fys - iy).astype(F)
            ixi, iyi = ix.astype(np.int64), iy.astype(np.int64)
            lim = (tol * tol) * (t * t)
            sum_w = np.zeros((h, w), F)
            sum_l = np.zeros((h, w), F)
            sum_vh = np.zeros((h, w), F)
            sum_wv = np.zeros((h, w), F)
            sum_c = np.zeros((h, w, 3), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ixi + i, iyi + j
                    ok = inside & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                    cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    Cq, Xq, Nq = hC[cy, cx], hX[cy, cx], hN[cy, cx]
                    ok &= Xq[..., 3] > 0
                    g = (X - Xq[..., :3]).astype(F)
                    ok &= (dot3(g, g) <= lim) & (dot3(N, Nq[..., :3]) >= ncos)
                    wb = ((tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)).astype(F)
                    sum_w = np.where(ok, sum_w + wb, sum_w)
                    sum_c = np.where(ok[..., None], sum_c + wb[..., None] * Cq[..., :3], sum_c)
                    sum_l = np.where(ok, sum_l + wb * Xq[..., 3], sum_l)
                    okv = ok & (Cq[..., 3] >= 0)
                    sum_vh = np.where(okv, sum_vh + wb * Cq[..., 3], sum_vh)
                    sum_wv = np.where(okv, sum_wv + wb, sum_wv)
            have = inside & (sum_w > F(0.015625))
            Hc = (sum_c / sum_w[..., None]).astype(F)
            q = sum_l / sum_w
            Hl = np.where(q < maxh, q, maxh).astype(F)
            Hv = np.where(sum_wv > 0, sum_vh / sum_wv, F(-1)).astype(F)
            tot = n + Hl
            cmh = ((n[..., None] * c + Hl[..., None] * Hc) / tot[..., None]).astype(F)
            both = ((n * n) * v + (Hl * Hl) * Hv) / (tot * tot)
            own = (v * n) / tot
            his = (Hv * Hl) / tot
            vmh = np.where((v >= 0) & (Hv >= 0), both, np.where(v >= 0, own, np.where(Hv >= 0, his, F(-1)))).astype(F)
            cm = np.where(have[..., None], cmh, c).astype(F)
            vm = np.where(have, vmh, v).astype(F)
            ln = np.where(have, tot, ln).astype(F)
        pend_c = np.concatenate([cm, vm[..., None]], -1).astype(F)
        pend_x = np.concatenate([X, np.where(geom, ln, F(0))[..., None]], -1).astype(F)
        pend_n = np.concatenate([N, np.zeros((h, w, 1), F)], -1).astype(F)
    return dict(valid=valid, cm=cm, vm=vm, len=ln, have=have, N=N, A=A, pending=(pend_c, pend_x, pend_n), fx=fx, fy=fy)


def iterate(valid, C, V, N, A, d, iterations, normal_power_log2, sigma_luminance, sigma_albedo, exposure):
    """The iterations and the output of "denoised previews" from (C0, V0): prt_denoise_ref.denoise's loop, operation for operation."""
    sig_l, sig_a = F(sigma_luminance), F(sigma_albedo)
    sig_a2 = sig_a * sig_a
    shifted, f, H_TAPS, G_TAPS = R.shifted, R.f, R.H_TAPS, R.G_TAPS
    with np.errstate(all="ignore"):
        C = np.where(valid[..., None], C, F(0)).astype(F)
        V = np.where(valid, V, F(-1)).astype(F)
        for it in range(iterations):
            s = 1 << it
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
                        wgt = np.full(V.shape, H_TAPS[0] * H_TAPS[0], F)
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
                        wgt = ((((H_TAPS[dy] * H_TAPS[dx]) * wn) * wa) * wl).astype(F)
                    sum_w = np.where(ok, sum_w + wgt, sum_w)
                    sum_c = np.where(ok[..., None], sum_c + wgt[..., None] * Cq, sum_c)
                    sum_v = np.where(ok & known, sum_v + (wgt * wgt) * np.where(Vq >= 0, Vq, V), sum_v)
            C = np.where(valid[..., None], sum_c / sum_w[..., None], F(0)).astype(F)
            V = np.where(valid & known, sum_v / (sum_w * sum_w), F(-1)).astype(F)
        image = np.where(valid[..., None], F(exposure) * (C * d), F(0)).astype(F)
    return image, V


def denoise_temporal(total, count, mom, albedo, normal, position, history=None, position_tolerance=0.01, normal_cos=0.9,
                     max_history=256.0, iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True,
                     exposure=1.0):
    """Returns (image (H, W, 3), V_final (H, W), pending = dict(color_var, pos_len, normal))."""
    m = merge(total, count, mom, albedo, normal, position, history, position_tolerance, normal_cos, max_history)
    with np.errstate(all="ignore"):
        if demodulate:
            d = np.where(m["A"] > F(0.015625), m["A"], F(0.015625)).astype(F)  # max(a, b) = a > b ? a : b: 1/64 for a NaN albedo
            C = (m["cm"] / d).astype(F)
            ld = lum(d)
            V = np.where(m["vm"] < 0, F(-1), m["vm"] / (ld * ld)).astype(F)
        else:
            d = np.ones_like(m["A"])
            C, V = m["cm"], m["vm"]
    image, var = iterate(m["valid"], C, V, m["N"], m["A"], d, iterations, normal_power_log2, sigma_luminance, sigma_albedo, exposure)
    p = m["pending"]
    return image, var, dict(color_var=p[0], pos_len=p[1], normal=p[2])


# the temporal parameters the tests run the stage with unless they say otherwise, and the three sets the sweeps use
TDEFAULTS = dict(position_tolerance=0.01, normal_cos=0.9, max_history=256.0)
PARAMETER_SETS = (TDEFAULTS, dict(position_tolerance=0.05, normal_cos=0.5, max_history=32.0),
                  dict(position_tolerance=0.02, normal_cos=-1.0, max_history=1e6))
