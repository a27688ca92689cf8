"""The display transform of include/prt_hip.h ("display transform") restated in numpy: the integer histogram and the u64 walk of the
meter, the f32 steps of resolve and transform in the order the header writes them, and powf through ctypes on the machine's libm.so.6
(not np.power, whose float32 loop need not be libm's).  The checker of prt_amd/csrc/prt_display.h, on the host and on the device, at
tolerance 0.  Parameters are prt_amd.DisplayParams; the state is a dict(gain, valid, octaves, target, metered, ignored, hist)."""
import ctypes as C
import functools

import numpy as np

F = np.float32
_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]
EXP_22 = F(1) / F(2.2)  # 1/2.2f and 1/2.4f as the C text computes them: one f32 division
EXP_24 = F(1) / F(2.4)


def powf(x, e):
    """libm's powf on every element of a float32 array (each distinct value once)."""
    x = np.asarray(x, dtype=F)
    u, inv = np.unique(x.view(np.uint32).reshape(-1), return_inverse=True)
    r = np.array([_libm.powf(float(v), float(e)) for v in u.view(F)], dtype=F)
    return r[inv].reshape(x.shape)


def lum(c):
    c = np.asarray(c, dtype=F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def fresh_state():
    return dict(gain=F(0), valid=0, octaves=F(0), target=F(0), metered=0, ignored=0, hist=np.zeros(256, np.uint32))


def histogram(rgb):
    """(hist (256,) uint32, ignored) of the pixels of an (h, w, 3) image."""
    L = lum(rgb).reshape(-1)
    with np.errstate(invalid="ignore"):
        counted = L > F(0)  # false for NaN, +-0 and negatives
    k = np.clip((L[counted].view(np.uint32) >> 20).astype(np.int64) - 888, 0, 255)
    return np.bincount(k, minlength=256).astype(np.uint32), int((~counted).sum())


def resolve(hist, ignored, p, state):
    """The state after one metering with this histogram (a new dict)."""
    s = dict(state, hist=np.array(state["hist"], dtype=np.uint32))
    N = int(hist.astype(np.uint64).sum())
    if N == 0:
        return s
    rlo, rhi = p.lowPermille * N // 1000, (p.highPermille * N + 999) // 1000
    cum = Nb = S = 0
    for k in range(256):
        a, end = max(cum, rlo), cum + int(hist[k])
        b = min(end, rhi)
        if b > a:
            Nb += b - a
            S += (b - a) * (2 * k + 1)
        cum = end
    assert Nb >= 1 and S < 2 ** 64
    m = np.array([S], np.uint64).astype(F)[0] / np.array([Nb], np.uint64).astype(F)[0]
    octaves = F(m * F(0.0625)) - F(16)
    i = np.floor(octaves)
    f = F(octaves - i)
    two = np.array([(int(i) + 127) << 23], np.uint32).view(F)[0]
    L = F(F(1) + f) * two
    t = F(p.key) / L
    target = min(max(t, F(p.minGain)), F(p.maxGain))
    if s["valid"] and F(p.adaptRate) < F(1):
        s["gain"] = F(F(s["gain"]) + F(F(target - F(s["gain"])) * F(p.adaptRate)))
    else:
        s["gain"] = F(target)
    s.update(valid=1, octaves=F(octaves), target=F(target), metered=N, ignored=ignored, hist=hist.copy())
    return s


def channel_bytes(v, g, tonemap, transfer):
    """The byte of every element of the float32 array v under the gain g."""
    with np.errstate(all="ignore"):
        x = F(g) * np.asarray(v, dtype=F)
        if tonemap:
            x = x / (x + F(1))
        x = np.where(x > F(0), x, F(0)).astype(F)  # fminf(fmaxf(x, 0), 1): NaN -> 0
        x = np.where(x < F(1), x, F(1)).astype(F)
        if transfer == 0:
            return (powf(x, EXP_22) * F(255)).astype(np.int32).astype(np.uint8)
        s = np.where(x <= F(0.0031308), F(12.92) * x, F(1.055) * powf(x, EXP_24) - F(0.055)).astype(F)
        return (s * F(255) + F(0.5)).astype(np.int32).astype(np.uint8)


def display(rgb, p, state=None, x0=0, y0=0, x1=None, y1=None, out=None):
    """(out (h, w, bpp) uint8 with the rectangle written, state after): one call of the display on an (h, w, 3) float32 image."""
    rgb = np.asarray(rgb, dtype=F)
    h, w, _ = rgb.shape
    x1 = w - 1 if x1 is None else x1
    y1 = h - 1 if y1 is None else y1
    state = fresh_state() if state is None else state
    rect = rgb[y0:y1 + 1, x0:x1 + 1]
    if p.meter:
        state = resolve(*histogram(rect), p, state)
        g = F(p.gain) * F(state["gain"])
    else:
        g = F(p.gain)
    bpp = 3 if p.format == 0 else 4
    out = np.zeros((h, w, bpp), np.uint8) if out is None else out.copy()
    b = channel_bytes(rect, g, p.tonemap, p.transfer)
    px = np.full(rect.shape[:2] + (bpp,), 255, np.uint8)
    px[..., :3] = b[..., ::-1] if p.format == 2 else b
    out[y0:y1 + 1, x0:x1 + 1] = px
    return out, state


def thresholds(transfer):
    """For every byte value 1..255 of a transfer (no tone map, gain 1): the least float whose byte reaches it and its predecessor,
    found by bisection on the restatement over the bit patterns of [0, 1] -- (255, 2) float32."""
    def byte(bits):
        return int(channel_bytes(np.array([bits], np.uint32).view(F), F(1), 0, transfer)[0])
    out = np.zeros((255, 2), np.uint32)
    for v in range(1, 256):
        lo, hi = 0, 0x3f800000  # byte(lo) < v <= byte(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if byte(mid) >= v else (mid, hi)
        out[v - 1] = (lo, hi)
    return out.view(F)


@functools.lru_cache(maxsize=None)
def hostile_image():
    """61 x 37: the straddling pairs of every byte threshold of both transfers, +-0, subnormals, 1.0, NaN, +-inf, negatives, 1e30 --
    as single channels and as whole pixels (black, NaN, +inf: the meter's special cases) -- in an HDR image from 1e-6 to 1e3."""
    rng = np.random.default_rng(20)
    w, h = 61, 37
    img = (rng.random((h, w, 3)) * 10.0 ** rng.uniform(-6, 3, (h, w, 1))).astype(F)
    flat = img.reshape(-1)
    special = np.array([0.0, -0.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 1.0, np.nan, np.inf, -np.inf, -1.0, -1e-3, 1e30, 0.99999994,
                        1.0000001, 0.0031308, 0.00313081, 0.5], F)
    vals = np.concatenate([thresholds(0).reshape(-1), thresholds(1).reshape(-1), special])
    where = rng.choice(flat.size - 30 * 3, len(vals), replace=False) + 30 * 3  # the first 30 pixels are set below
    flat[where] = vals
    for k, px in enumerate([(0, 0, 0), (np.nan,) * 3, (np.inf,) * 3, (-1, -2, -3), (np.inf, 0, 0), (-0.0, 0, 0), (1e30,) * 3, (3e-6,) * 3,
                            (1e-45, 0, 0), (np.nan, 1, 1), (-np.inf, 1, 1), (61000, 61000, 61000), (62000, 62000, 62000)]):
        img[0, k] = px
    img.setflags(write=False)
    return img


# ----------------------------------------------------------------------------- shared by the CPU and the GPU tests
def assert_state_equal(got, want, what=""):
    """got: a DisplayState (or its as_dict()); want: the restatement's dict.  Floats are compared as words."""
    g = got.as_dict() if hasattr(got, "as_dict") else got
    for k in ("gain", "octaves", "target"):
        assert F(g[k]).view(np.uint32) == F(want[k]).view(np.uint32), (what, k, g[k], want[k])
    for k in ("valid", "metered", "ignored"):
        assert int(g[k]) == int(want[k]), (what, k, g[k], want[k])
    assert np.array_equal(g["hist"], want["hist"]), (what, "hist")


def frame(level, seed, shape=(24, 40)):
    rng = np.random.default_rng(seed)
    return (rng.random(shape + (3,)) * level * 10.0 ** rng.uniform(-2, 2, shape + (1,))).astype(F)


BAD_FIELDS = [("tonemap", dict(tonemap=2)), ("transfer", dict(transfer=2)), ("format", dict(format=3)), ("meter", dict(meter=2)),
              ("gain", dict(gain=-1.0)), ("gain", dict(gain=float("nan"))), ("gain", dict(gain=float("inf"))),
              ("key", dict(meter=1, key=0.0)), ("key", dict(meter=1, key=float("nan"))), ("key", dict(meter=1, key=float("inf"))),
              ("lowPermille", dict(meter=1, low_permille=1000, high_permille=1000)),
              ("highPermille", dict(meter=1, low_permille=500, high_permille=500)), ("highPermille", dict(meter=1, low_permille=600, high_permille=500)),
              ("highPermille", dict(meter=1, high_permille=1001)),
              ("minGain", dict(meter=1, min_gain=0.0)), ("minGain", dict(meter=1, min_gain=float("nan"))),
              ("maxGain", dict(meter=1, min_gain=2.0, max_gain=1.0)), ("maxGain", dict(meter=1, max_gain=float("inf"))),
              ("adaptRate", dict(meter=1, adapt_rate=0.0)), ("adaptRate", dict(meter=1, adapt_rate=1.5)), ("adaptRate", dict(meter=1, adapt_rate=float("nan")))]
