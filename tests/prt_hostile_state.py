"""Non-finite and hostile accumulator state for the two preview filters (include/prt_hip.h "denoised previews" and "temporal
reprojection"): the helper of tests/test_hostile_state_cpu.py and tests/test_gpu_hostile_state.py.  No GPU, no fixture file.

  denoise_scalar, merge_scalar, denoise_temporal_scalar
        a SECOND restatement of the header, pixel by pixel and tap by tap, np.float32 scalars in plain loops.  It shares no code
        with the array restatements (prt_denoise_ref, prt_temporal_ref): its purpose is to check their np.where and shift machinery
        under NaN.  Slow: meant for images of about 13 x 9 and 3 iterations.
  hostile_state(width, height, seed, sources)
        accumulator, moments, guides and a per-pixel label.  BENIGN classes stand anywhere; NON-FINITE SOURCES only in the columns
        x < BAND, so that the footprint law leaves the columns x >= BAND + 2*(2^k - 1) finite after k iterations.
  hostile_history(...)
        a position plane and history planes with NaN, inf and negative colours, variances, lengths and normals; the non-finite
        colours (and infinite variances) reproject into the same band.
  footprint(...)
        the law of the header's "what follows for non-finite state", from the tap offsets alone.
Comparisons go through prt_adaptive_ref.assert_words_equal (uint32 words; only NaN against NaN is excepted) with the labels."""
import collections

import numpy as np

import prt_denoise_ref as R
import prt_temporal_ref as TR

F, U32 = np.float32, np.uint32
BAND = 12
H5 = {-2: F(0.0625), -1: F(0.25), 0: F(0.375), 1: F(0.25), 2: F(0.0625)}
G3 = {-1: F(0.25), 0: F(0.5), 1: F(0.25)}
PAYLOADS = (0x7fc12345, 0xffc00000, 0x7f800001)  # a quiet NaN with a payload, the negative default NaN, a signalling NaN


# ============================================================================ the scalar restatement
def _max(a, b):
    """max(a, b) of the header: a > b ? a : b -- b when a is NaN."""
    return a if a > b else b


def _lum(c):
    return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]


def _f(x):
    y = F(0.125) * x
    r = F(1.0) / ((F(1.0) + y) + (F(0.5) * y) * y)
    r = r * r
    r = r * r
    r = r * r
    return r


def _dot3(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def _pixel(total, count, mom, albedo, normal, y, x):
    """valid_p, n, c_p, v_p, N_p, A_p of one pixel."""
    n = int(count[y, x])
    valid = n > 0
    A = [F(a) for a in albedo[y, x]]
    G = [F(g) for g in normal[y, x]]
    N = [F(0)] * 3 if (G[0] == 0 and G[1] == 0 and G[2] == 0) else [(g - F(0.5)) * F(2.0) for g in G]
    c, v = [F(0)] * 3, F(-1)
    if valid:
        c = [F(s) / F(n) for s in total[y, x]]
        m = int(mom[y, x, 2:3].view(U32)[0])
        if m >= 2:
            v = (F(mom[y, x, 1]) / F(m - 1)) / F(n >> 3)
    return valid, n, c, v, N, A


def _demodulated(valid, c, v, A, demodulate):
    """(C0_p, V0_p, d_p)."""
    if demodulate:
        d = [_max(a, F(0.015625)) for a in A]
        C0 = [c[k] / d[k] for k in range(3)]
        ld = _lum(d)
        V0 = F(-1) if v < 0 else v / (ld * ld)
    else:
        d, C0, V0 = [F(1.0)] * 3, c, v
    if not valid:
        C0, V0 = [F(0)] * 3, F(-1)
    return C0, V0, d


def _iterations(valid, C, V, N, A, d, iterations, normal_power_log2, sigma_luminance, sigma_albedo, exposure):
    """The iterations and the output from the planes (C0, V0); python lists of np.float32 per pixel."""
    h, w = len(valid), len(valid[0])
    sig_l, sig_a = F(sigma_luminance), F(sigma_albedo)
    sig_a2 = sig_a * sig_a
    for it in range(iterations):
        s = 1 << it
        C2 = [[None] * w for _ in range(h)]
        V2 = [[None] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                if not valid[y][x]:
                    C2[y][x], V2[y][x] = [F(0)] * 3, F(-1)
                    continue
                Cp, Vp, Np, Ap = C[y][x], V[y][x], N[y][x], A[y][x]
                Lp = _lum(Cp)
                known = bool(Vp >= 0)
                den = None
                if known:
                    sum_vw = sum_wt = F(0)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            qx, qy = x + dx, y + dy
                            if qx < 0 or qy < 0 or qx >= w or qy >= h or not valid[qy][qx]:
                                continue
                            Vq = V[qy][qx]
                            if not Vq >= 0:
                                continue
                            wt = G3[dy] * G3[dx]
                            sum_vw = sum_vw + wt * Vq
                            sum_wt = sum_wt + wt
                    g = sum_vw / sum_wt
                    den = sig_l * np.sqrt(g) + F(1e-6)
                sum_w = sum_v = F(0)
                sum_c = [F(0)] * 3
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + s * dx, y + s * dy
                        if qx < 0 or qy < 0 or qx >= w or qy >= h or not valid[qy][qx]:
                            continue
                        Cq, Vq = C[qy][qx], V[qy][qx]
                        if dx == 0 and dy == 0:
                            wgt = H5[0] * H5[0]
                        else:
                            Nq, Aq = N[qy][qx], A[qy][qx]
                            wn = _max(_dot3(Np, Nq), F(0.0))
                            for _ in range(normal_power_log2):
                                wn = wn * wn
                            da = [Ap[k] - Aq[k] for k in range(3)]
                            wa = _f(_dot3(da, da) / sig_a2)
                            wl = _f(np.abs(Lp - _lum(Cq)) / den) if known else F(1.0)  # "V_p < 0" there is "not V_p >= 0"
                            wgt = (((H5[dy] * H5[dx]) * wn) * wa) * wl
                        sum_w = sum_w + wgt
                        sum_c = [sum_c[k] + wgt * Cq[k] for k in range(3)]
                        if known:
                            sum_v = sum_v + (wgt * wgt) * (Vq if Vq >= 0 else Vp)
                C2[y][x] = [sum_c[k] / sum_w for k in range(3)]
                V2[y][x] = sum_v / (sum_w * sum_w) if known else F(-1)
        C, V = C2, V2
    image = np.zeros((h, w, 3), F)
    var = np.zeros((h, w), F)
    for y in range(h):
        for x in range(w):
            var[y, x] = V[y][x]
            if valid[y][x]:
                image[y, x] = [F(exposure) * (C[y][x][k] * d[y][x][k]) for k in range(3)]
    return image, var


def _inputs(total, count, mom, albedo, normal):
    return (np.ascontiguousarray(total, dtype=F), np.ascontiguousarray(count, dtype=U32), np.ascontiguousarray(mom, dtype=F),
            np.ascontiguousarray(albedo, dtype=F), np.ascontiguousarray(normal, dtype=F))


def denoise_scalar(total, count, mom, albedo, normal, iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1,
                   demodulate=True, exposure=1.0):
    """prt_hip_accum_denoise from the header's text: (image (H, W, 3), V_final (H, W))."""
    total, count, mom, albedo, normal = _inputs(total, count, mom, albedo, normal)
    h, w = count.shape
    with np.errstate(all="ignore"):
        px = [[_pixel(total, count, mom, albedo, normal, y, x) for x in range(w)] for y in range(h)]
        dm = [[_demodulated(p[0], p[2], p[3], p[5], demodulate) for p in row] for row in px]
        pick = lambda rows, k: [[p[k] for p in row] for row in rows]  # noqa: E731
        return _iterations(pick(px, 0), pick(dm, 0), pick(dm, 1), pick(px, 4), pick(px, 5), pick(dm, 2), iterations, normal_power_log2,
                           sigma_luminance, sigma_albedo, exposure)


def _camera(cam, key):
    v = cam[key] if isinstance(cam, dict) else getattr(cam, key)
    return [F(a) for a in v]


def merge_scalar(total, count, mom, albedo, normal, position, history=None, position_tolerance=0.01, normal_cos=0.9, max_history=256.0):
    """The per-pixel block of "temporal reprojection" up to the pending record: dict(cm (H, W, 3), vm, len, have, taken (H, W): whether
    an accepted tap had a non-finite colour, pending=(color_var, pos_len, normal))."""
    total, count, mom, albedo, normal = _inputs(total, count, mom, albedo, normal)
    h, w = count.shape
    P = np.ascontiguousarray(position, dtype=F).reshape(h, w, 4)
    tol, ncos, maxh = F(position_tolerance), F(normal_cos), F(max_history)
    out = dict(cm=np.zeros((h, w, 3), F), vm=np.zeros((h, w), F), len=np.zeros((h, w), F), have=np.zeros((h, w), bool),
               taken=np.zeros((h, w), bool))
    pend = [np.zeros((h, w, 4), F) for _ in range(3)]
    if history is not None:
        hc = {k: _camera(history["camera"], k) for k in ("pos", "right", "up", "dir")}
        hC, hX, hN = (np.ascontiguousarray(history[k], dtype=F).reshape(h, w, 4) for k in ("color_var", "pos_len", "normal"))
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                valid, cnt, c, v, N, _ = _pixel(total, count, mom, albedo, normal, y, x)
                X, t = [F(a) for a in P[y, x, :3]], F(P[y, x, 3])
                geom = bool(valid and t >= 0)
                have = False
                if geom and history is not None and maxh > 0:
                    e = [X[k] - hc["pos"][k] for k in range(3)]
                    a, b, z = _dot3(e, hc["right"]), _dot3(e, hc["up"]), _dot3(e, hc["dir"])
                    if z > 0:
                        k_aspect = F(w) / F(h)
                        fx = ((a / z) / ((F(2.0) * F(0.6)) * k_aspect) + F(0.5)) * F(w)
                        fy = (F(0.5) - (b / z) / (F(2.0) * F(0.6))) * F(h)
                        if fx >= F(-1.0) and fx < F(w) and fy >= F(-1.0) and fy < F(h):
                            ix, iy = np.floor(fx), np.floor(fy)
                            tx, ty = fx - ix, fy - iy
                            lim = (tol * tol) * (t * t)
                            sum_w = sum_l = sum_vh = sum_wv = F(0)
                            sum_c = [F(0)] * 3
                            for j in (0, 1):
                                for i in (0, 1):
                                    qx, qy = int(ix) + i, int(iy) + j
                                    if qx < 0 or qy < 0 or qx >= w or qy >= h or not hX[qy, qx, 3] > 0:
                                        continue
                                    g = [X[k] - hX[qy, qx, k] for k in range(3)]
                                    if not (_dot3(g, g) <= lim and _dot3(N, hN[qy, qx]) >= ncos):
                                        continue
                                    wb = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                                    sum_w = sum_w + wb
                                    sum_c = [sum_c[k] + wb * hC[qy, qx, k] for k in range(3)]
                                    sum_l = sum_l + wb * hX[qy, qx, 3]
                                    if hC[qy, qx, 3] >= 0:
                                        sum_vh = sum_vh + wb * hC[qy, qx, 3]
                                        sum_wv = sum_wv + wb
                                    out["taken"][y, x] |= not np.isfinite(hC[qy, qx, :3]).all()
                            have = bool(sum_w > F(0.015625))
                n = F(cnt)
                if have:
                    Hc = [sum_c[k] / sum_w for k in range(3)]
                    q = sum_l / sum_w
                    Hl = q if q < maxh else maxh
                    Hv = sum_vh / sum_wv if sum_wv > 0 else F(-1)
                    tot = n + Hl
                    cm = [(n * c[k] + Hl * Hc[k]) / tot for k in range(3)]
                    if v >= 0 and Hv >= 0:
                        vm = ((n * n) * v + (Hl * Hl) * Hv) / (tot * tot)
                    elif v >= 0:
                        vm = (v * n) / tot
                    elif Hv >= 0:
                        vm = (Hv * Hl) / tot
                    else:
                        vm = F(-1)
                    ln = tot
                else:
                    cm, vm, ln = c, v, (n if valid else F(0))
                    out["taken"][y, x] = False
                out["cm"][y, x], out["vm"][y, x], out["len"][y, x], out["have"][y, x] = cm, vm, ln, have
                pend[0][y, x] = cm + [vm]
                pend[1][y, x] = X + [ln if geom else F(0)]
                pend[2][y, x] = N + [F(0)]
    out["pending"] = tuple(pend)
    return out


def denoise_temporal_scalar(total, count, mom, albedo, normal, position, history=None, position_tolerance=0.01, normal_cos=0.9,
                            max_history=256.0, iterations=5, normal_power_log2=5, sigma_luminance=4.0, sigma_albedo=0.1, demodulate=True,
                            exposure=1.0):
    """prt_hip_accum_denoise_temporal from the header's text: (image, V_final, dict(color_var, pos_len, normal))."""
    m = merge_scalar(total, count, mom, albedo, normal, position, history, position_tolerance, normal_cos, max_history)
    total, count, mom, albedo, normal = _inputs(total, count, mom, albedo, normal)
    h, w = count.shape
    with np.errstate(all="ignore"):
        px = [[_pixel(total, count, mom, albedo, normal, y, x) for x in range(w)] for y in range(h)]
        dm = [[_demodulated(px[y][x][0], [F(a) for a in m["cm"][y, x]], F(m["vm"][y, x]), px[y][x][5], demodulate) for x in range(w)]
              for y in range(h)]
        pick = lambda rows, k: [[p[k] for p in row] for row in rows]  # noqa: E731
        image, var = _iterations(pick(px, 0), pick(dm, 0), pick(dm, 1), pick(px, 4), pick(px, 5), pick(dm, 2), iterations,
                                 normal_power_log2, sigma_luminance, sigma_albedo, exposure)
    p = m["pending"]
    return image, var, dict(color_var=p[0], pos_len=p[1], normal=p[2])


# ============================================================================ the footprint law
def reach(k):
    """A non-finite colour reaches |dx|, |dy| <= reach(k) after k iterations."""
    return 2 * ((1 << k) - 1)


def footprint(sources, k):
    """The pixels a non-finite colour at the pixels `sources` (bool (H, W)) of a fully valid image has reached after k iterations,
    from the tap offsets alone: iteration i reads the taps p + 2^i * (dx, dy), |dx|, |dy| <= 2, inside the image, and one non-finite
    tap makes the sum non-finite whatever its weight (0 * NaN and 0 * inf are NaN)."""
    cur = np.asarray(sources, dtype=bool)
    h, w = cur.shape
    for i in range(k):
        nxt = np.zeros_like(cur)
        for qy, qx in zip(*np.nonzero(cur)):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    py, px = qy - (dy << i), qx - (dx << i)  # the pixels that read (qx, qy) as their tap (dx, dy)
                    if 0 <= py < h and 0 <= px < w:
                        nxt[py, px] = True
        cur = nxt
    return cur


def square(shape, x, y, k):
    """The clipped square |dx|, |dy| <= reach(k) around (x, y)."""
    ys, xs = np.mgrid[:shape[0], :shape[1]]
    return (np.abs(xs - x) <= reach(k)) & (np.abs(ys - y) <= reach(k))


def nonfinite(a):
    """Per pixel: whether any channel is NaN or infinite."""
    a = np.asarray(a)
    return ~np.isfinite(a) if a.ndim == 2 else ~np.isfinite(a).all(-1)


# ============================================================================ hostile accumulator state
Hostile = collections.namedtuple("Hostile", "state mom albedo normal label")
SOURCES = ("all", "quiet", "island")


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def tame_state(width, height, seed, holes=True):
    """Ordinary state: 16 .. 64 samples per pixel in packets of 8 with a moment record each, radiance over five decades, guides that
    make regions (a few albedos and short normals blockwise, with jitter).  holes: some pixels with count 0, with m < 2, with a
    missed guide normal."""
    rng = np.random.default_rng([seed, width, height])
    shape = (height, width)
    packets = rng.integers(2, 9, shape)
    count = (packets * 8).astype(U32)
    mean = (rng.random(shape + (3,)) * 10.0 ** rng.uniform(-3, 2, shape + (1,))).astype(F)
    total = (mean * count[..., None].astype(F)).astype(F)
    lum = R.lum(mean)
    mom = np.zeros(shape + (4,), F)
    mom[..., 0] = lum
    mom[..., 1] = (lum * lum * rng.random(shape) * 4.0 * (packets - 1)).astype(F)
    m = packets.astype(U32)
    by, bx = np.meshgrid(np.arange(height) // 7, np.arange(width) // 5, indexing="ij")
    palette = (0.1 + 0.8 * rng.random((8, 3))).astype(F)
    albedo = np.abs(palette[(by * 3 + bx) % 8] + rng.normal(0, 0.01, shape + (3,))).astype(F)
    n = rng.normal(size=(8, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nn = n[(by + bx) % 8] + rng.normal(0, 0.05, shape + (3,))
    nn *= rng.uniform(0.3, 1.0, shape + (1,)) / np.linalg.norm(nn, axis=-1, keepdims=True)
    normal = (0.5 * nn + 0.5).astype(F)
    label = np.full(shape, "filler", dtype=object)
    if holes:
        r = rng.random(shape)
        for lo, hi, name in ((0.0, 0.06, "count 0"), (0.06, 0.12, "m < 2"), (0.12, 0.17, "miss normal")):
            label[(r >= lo) & (r < hi)] = name
        count[label == "count 0"] = 0
        m[label == "m < 2"] = rng.integers(0, 2, int((label == "m < 2").sum()))
        normal[label == "miss normal"] = 0.0
    mom[..., 2] = m.view(F)
    state = dict(width=width, height=height, seed=12345, max_depth=14, rr_depth=4, rng=rng.integers(1, 2 ** 32, shape, dtype=np.uint64).astype(U32),
                 sum=total, count=count)
    return Hostile(state, mom, albedo, normal, label)


def hostile_state(width, height, seed, sources="all"):
    """Hostile(state, mom, albedo, normal, label): state is what PathTracer.accum_import takes (sum (H, W, 3), count (H, W), ...), mom the
    moment records, albedo / normal the guide planes, label[y, x] the pixel's class.
    sources  "all"     every class below
             "quiet"   the benign classes and only those sources that leave every COLOUR finite (M2 NaN, M2 +inf, count < 8 with
                       m >= 2, a NaN normal: wn = max(NaN, 0) = 0): what the filters compute is then compared number for number,
                       not NaN for NaN
             "island"  "quiet" plus the NaN-albedo island, which stays finite through iterations 0..2
    A 1 x 1 image is the NaN-albedo pixel alone."""
    assert sources in SOURCES, sources
    s = tame_state(width, height, seed)
    state, mom, albedo, normal, label = s
    total, count = state["sum"], state["count"]
    m = mom[..., 2].view(U32)
    rng = np.random.default_rng([seed, width, height, 1])
    taken = set()

    def ordinary(p):  # a valid pixel with a known variance and a hit normal under the class
        if count[p] == 0 or m[p] < 2 or (normal[p] == 0).all():
            count[p], m[p] = 24, 3
            total[p] = np.abs(total[p]) + F(0.5)
            normal[p] = (0.5 * 0.8 * _unit(rng) + 0.5).astype(F)

    def island(cx, cy, name):
        for it in range(3):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    q = (cy + (dy << it), cx + (dx << it))
                    if (dx or dy) and 0 <= q[0] < height and 0 <= q[1] < width:
                        count[q], label[q] = 0, "moat"
                        taken.add(q)
        p = (cy, cx)
        ordinary(p)
        label[p] = name
        taken.add(p)
        return p

    nan_island = width * height == 1 or sources == "island" or (sources == "all" and width > BAND)
    if nan_island:
        p = island(min(5, (width - 1) // 2), height // 2, "island, albedo NaN")
        albedo[p][1] = np.nan
    if width >= 48:
        island(width - 20, height // 2, "island")

    def set_sum(p, value, channels):
        for c in channels:
            total[p][c] = value

    def set_bits(p, word, c):
        total.view(U32)[p][c] = word

    def long_normal(p, length):
        normal[p] = (0.5 * (length * _unit(rng)) + 0.5).astype(F)

    def short_count(p):
        count[p], m[p] = rng.integers(1, 8), 2
        mom[p][1] = np.abs(mom[p][1]) + F(1e-3)

    def odd_count(p, packets):
        count[p], m[p] = 8 * max(packets, 1) + rng.integers(1, 8), packets

    one = lambda: [int(rng.integers(0, 3))]  # noqa: E731
    quiet = [("M2 NaN", lambda p: mom[p].__setitem__(1, np.nan)), ("M2 +inf", lambda p: mom[p].__setitem__(1, np.inf)),
             ("count < 8, m >= 2", short_count), ("normal NaN", lambda p: normal[p].__setitem__(one()[0], np.nan))]
    loud = [("sum NaN, one channel", lambda p: set_sum(p, np.nan, one())), ("sum NaN", lambda p: set_sum(p, np.nan, range(3))),
            ("sum +inf, one channel", lambda p: set_sum(p, np.inf, one())), ("sum +inf", lambda p: set_sum(p, np.inf, range(3))),
            ("sum -inf, one channel", lambda p: set_sum(p, -np.inf, one())), ("sum -inf", lambda p: set_sum(p, -np.inf, range(3))),
            ("albedo NaN", lambda p: albedo[p].__setitem__(one()[0], np.nan)), ("albedo +inf", lambda p: albedo[p].__setitem__(one()[0], np.inf)),
            ("normal x 40", lambda p: long_normal(p, 40.0))] + \
           [(f"sum 0x{w:08x}", lambda p, w=w: set_bits(p, w, one()[0])) for w in PAYLOADS]
    benign = [("sum negative", lambda p: total.__setitem__(p, -np.abs(total[p]))),
              ("sum negative, one channel", lambda p: total[p].__setitem__(one()[0], -F(3.0))),
              ("sum -0.0", lambda p: total.__setitem__(p, -0.0)), ("sum denormal", lambda p: total.__setitem__(p, 1e-40)),
              ("albedo negative", lambda p: albedo.__setitem__(p, -albedo[p] - F(0.1))), ("albedo 3.0", lambda p: albedo.__setitem__(p, 3.0)),
              ("M2 negative", lambda p: mom[p].__setitem__(1, -np.abs(mom[p][1]) - F(1e-3))), ("M2 -0.0", lambda p: mom[p].__setitem__(1, -0.0)),
              ("count % 8, m < 2", lambda p: odd_count(p, int(rng.integers(0, 2)))), ("count % 8", lambda p: odd_count(p, 2)),
              ("normal 1.04", lambda p: long_normal(p, rng.uniform(1.0, 1.04)))]
    if width * height > 1:
        order = [divmod(int(i), width) for i in rng.permutation(width * height)]
        band = [p for p in order if p[1] < BAND and p not in taken]
        field = [p for p in order if p[1] >= BAND and p not in taken] or band  # an image no wider than the band: one pool
        wanted = [(c, band, max(1, round(0.03 * len(band)))) for c in quiet + (loud if sources == "all" else [])] + \
                 [(c, field, max(1, round(0.025 * len(field)))) for c in benign]
        budget = (2 * width * height) // 3 - len(taken)
        for turn in range(max(k for _, _, k in wanted)):  # one pixel per class and turn, so that a small image holds as many classes as fit
            for (name, apply), pool, k in wanted:
                if turn < k and pool and budget > 0:
                    p = pool.pop()
                    ordinary(p)
                    apply(p)
                    label[p] = name
                    budget -= 1
    if not (count > 0).any():
        count[0, 0] = 16
    return s


# ============================================================================ hostile history
def camera_pair(width, height, seed, pixels=1.0):
    """(current camera, history camera): near the Cornell view; the history's stands about `pixels` pixel footprints aside."""
    import prt_amd
    rng = np.random.default_rng([seed, 7])
    pos = np.array([0.0, 1.0, 3.0]) + rng.uniform(-0.2, 0.2, 3)
    d = np.array([0.0, 0.0, -1.0]) + np.append(rng.uniform(-0.1, 0.1, 2), 0.0)
    foot = 1.2 * 4.0 / height
    hpos = pos + rng.uniform(-1, 1, 3) * pixels * foot
    hd = d + np.append(rng.uniform(-1, 1, 2) * pixels * foot / 8.0, 0.0)
    make = lambda p, q: prt_amd.Camera().create(tuple(float(v) for v in p), tuple(float(v) for v in q), width, height)  # noqa: E731
    return make(pos, d), make(hpos, hd)


def plane_positions(cam):
    """{X, t} of a tilted plane around z = -1 seen through the pixel centres of a prt_amd.Camera."""
    w, h = cam.width, cam.height
    d = TR.centre_directions(cam.desc, w, h).astype(np.float64)
    n = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    pos = np.array(list(cam.desc.pos), np.float64)
    return TR.position_plane(cam.desc, w, h, ((-1.0 - n @ pos) / (d @ n)).astype(F))


def hostile_history(width, height, seed, cur, hist_cam, normal):
    """(position plane of the current view, history record seen from hist_cam).  Colours: NaN, +inf and -inf in the columns x < BAND - 4
    (a tap is at most a few pixels from where the camera pair puts it, so they merge into pixels of the band), negative anywhere.
    Variances: +inf in the same columns (it spreads as an infinite V does), NaN, -0.5 and -0.0 anywhere.  Lengths: +inf, NaN, -0.0
    and a denormal; normals: NaN and inf, anywhere: none of them makes a colour non-finite."""
    rng = np.random.default_rng([seed, width, height, 2])
    shape = (height, width)
    pos = plane_positions(cur)
    pos[rng.random(shape) < 0.05] = (0, 0, 0, -1)
    hpos = plane_positions(hist_cam)
    jitter = np.where(rng.random(shape + (1,)) < 0.7, 1e-4, 0.012) * hpos[..., 3:4] * rng.normal(size=shape + (3,)) / np.sqrt(3.0)
    hX = (hpos[..., :3] + jitter).astype(F)
    hlen = rng.choice(np.array([0.0, 8.0, 64.0, 300.0], F), shape, p=[0.1, 0.3, 0.4, 0.2]).astype(F)
    hC = (rng.random(shape + (3,)) * 10.0 ** rng.uniform(-3, 2, shape + (1,))).astype(F)
    hV = (rng.random(shape) * 10.0 ** rng.uniform(-4, 1, shape)).astype(F)
    hV[rng.random(shape) < 0.2] = -1.0
    G = np.asarray(normal, dtype=F)
    with np.errstate(all="ignore"):
        N = np.where((G == 0).all(-1, keepdims=True), F(0), (G - F(0.5)) * F(2.0)).astype(np.float64)
        N = np.where(np.isfinite(N).all(-1, keepdims=True) & (np.abs(N) < 4).all(-1, keepdims=True), N, 0.0)
        length = np.linalg.norm(N, axis=-1, keepdims=True)
        hN = np.where(length > 0, N / np.maximum(length * length, 1e-9), 0.0) + rng.normal(0, 0.03, shape + (3,))  # dot3(N_p, hN_p) ~ 1
    hN[rng.random(shape) < 0.1] *= -1.0
    inner = np.broadcast_to(np.arange(width) < BAND - 4, shape)

    def some(fraction, where=None):
        pick = rng.random(shape) < fraction
        return pick if where is None else pick & where

    for value in (np.nan, np.inf, -np.inf):
        hC[some(0.15, inner), int(rng.integers(0, 3))] = value
        hC[some(0.05, inner)] = value
    hC[some(0.04)] *= -1.0
    hV[some(0.2, inner)] = np.inf
    for value in (np.nan, -0.5, -0.0):
        hV[some(0.04)] = value
    for value in (np.inf, np.nan, -0.0, 1e-40):
        hlen[some(0.04)] = value
    for value in (np.nan, np.inf):
        hN[some(0.03), int(rng.integers(0, 3))] = value
    hist = dict(camera=hist_cam.desc, color_var=np.concatenate([hC, hV[..., None]], -1).astype(F),
                pos_len=np.concatenate([hX, hlen[..., None]], -1).astype(F),
                normal=np.concatenate([hN, np.zeros(shape + (1,))], -1).astype(F))
    return pos.astype(F), hist


def temporal_state(width, height, seed, sources="all", pixels=None):
    """The keyword arguments of prt_temporal_ref.denoise_temporal (total, count, mom, albedo, normal, position, history) of a hostile state
    with a hostile history, plus the Hostile it was made from and the current camera.  pixels: how far aside the history's camera
    stands; by default one pixel for images of 30 rows and more and the same camera for coarser ones, whose pixel footprint is many
    times the position tolerance, so that after any move no history tap would be accepted."""
    s = hostile_state(width, height, seed, sources)
    cur, hist_cam = camera_pair(width, height, seed, (1.0 if height >= 30 else 0.0) if pixels is None else pixels)
    position, hist = hostile_history(width, height, seed, cur, hist_cam, s.normal)
    return dict(total=s.state["sum"], count=s.state["count"], mom=s.mom, albedo=s.albedo, normal=s.normal, position=position, history=hist), s, cur


# ============================================================================ rendered cases
RENDERED_SCENES = ("nonfinite", "box_nan", "box_inf")


def rendered_cases(min_finite=0.25, min_nonfinite=0.05):
    """[(scene, iterations, predicted finite share)] of tests/golden/hostile_shade.npz: by the footprint law, the share of the stored
    image's pixels outside every non-finite pixel's square after 1 and 2 iterations; kept where at least min_finite of the image stays
    finite and at least min_nonfinite does not."""
    import prt_hostile_shade as S
    out = []
    for name in RENDERED_SCENES:
        bad = nonfinite(S.golden(name)["image"])
        for k in (1, 2):
            share = 1.0 - float(footprint(bad, k).mean())
            if share >= min_finite and 1.0 - share >= min_nonfinite:
                out.append((name, k, share))
    return out
