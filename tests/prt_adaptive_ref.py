"""The adaptive-sampling estimator of include/prt_hip.h ("adaptive sampling") restated in numpy: every operation in np.float32 and in
the header's order (the build has no FMA and numpy has none), so that device results can be compared word for word.  Shared by
test_adaptive_ref_cpu.py, which checks this restatement on its own, and the GPU tests that hold the kernels to it."""
import collections
import itertools

import numpy as np

from prt_testlib import bits  # noqa: F401  (re-exported: the tests of this restatement call it as R.bits)

F32, U32 = np.float32, np.uint32
FLOOR = 0.01
EXPOSURES = (1.0, 2.5)  # the exposures the error is checked at; the selection runs at SELECT_EXPOSURE over a fill of FILL_EXPOSURE
SELECT_EXPOSURE, FILL_EXPOSURE = 2.5, 0.5
DENORMAL = 1e-40
TOP = 1 << 24


# ---- comparison
words_compared = 0  # running total over assert_words_equal calls (the GPU tests print it per test)


def assert_words_equal(got, want, what, label=None):
    """got == want as uint32 words: zeros with their sign, infinities, denormals.  The only pairs excepted are those where BOTH sides
    are NaN, whatever the payload.  label: per-pixel class names (the arrays' leading shape), quoted for the first mismatches."""
    global words_compared
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(U32) != want.view(U32)) & ~(np.isnan(got) & np.isnan(want))
    words_compared += got.size
    if bad.any():
        where = np.argwhere(bad)
        lines = []
        for idx in where[:6]:
            idx = tuple(int(i) for i in idx)
            name = "" if label is None else f" [{label[idx[:label.ndim]]}]"
            lines.append(f"  at {idx}{name}: got {got[idx]!r} (0x{int(got.view(U32)[idx]):08x}), want {want[idx]!r} (0x{int(want.view(U32)[idx]):08x})")
        raise AssertionError(f"{what}: {len(where)} of {got.size} words differ\n" + "\n".join(lines))
    return got.size


# ---- the header's formulas
def luminance(res):
    """The packet-mean luminance of the header, in float32 and in its order."""
    res = np.asarray(res, dtype=F32)
    return (F32(0.2126) * res[..., 0] + F32(0.7152) * res[..., 1] + F32(0.0722) * res[..., 2]) * F32(0.125)


def welford_step(mom, res, mask):
    """One packet end: the records `mom` (..., 4) with the packet sum `res` (..., 3) folded in where mask, untouched elsewhere."""
    mean, m2, m = mom[..., 0], mom[..., 1], mom[..., 2].view(U32)
    with np.errstate(all="ignore"):
        L = luminance(res)
        m1 = m + U32(1)
        d = L - mean
        mean1 = mean + d / m1.astype(F32)
        m21 = m2 + d * (L - mean1)
    out = mom.copy()
    out[..., 0] = np.where(mask, mean1, mean)
    out[..., 1] = np.where(mask, m21, m2)
    out[..., 2] = np.where(mask, m1, m).astype(U32).view(F32)
    out[..., 3] = np.where(mask, F32(0), mom[..., 3])
    return out


def welford_fold(P, packets):
    """The moment record {mean, M2, bits(m), 0} of a pixel that started empty and folded its packet sums P[0], ..., P[packets - 1] in
    this order.  P: (J, ..., 3) float32; packets: (...) integers, at most J."""
    P = np.asarray(P, dtype=F32)
    packets = np.asarray(packets)
    assert packets.shape == P.shape[1:-1] and int(packets.max(initial=0)) <= len(P), (packets.shape, P.shape)
    mom = np.zeros(P.shape[1:-1] + (4,), dtype=F32)
    for j in range(int(packets.max(initial=0))):
        mom = welford_step(mom, P[j], packets > j)
    return mom


def ordered_sum(P, packets):
    """The accumulator's sum after the same packets: ((+0 + P[0]) + P[1]) + ... in float32."""
    P = np.asarray(P, dtype=F32)
    packets = np.asarray(packets)
    total = np.zeros(P.shape[1:], dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(int(packets.max(initial=0))):
            total = np.where((packets > j)[..., None], total + P[j], total)
    return total


def error(count, mom, exposure=1.0, floor=FLOOR):
    """err of the header from an accumulator export's counts and a moment export, in float32: +inf when m < 2, otherwise
    var = M2 / (float)(m - 1); se = sqrtf(var / (float)(n >> 3)); err = (exposure * se) / (floor + exposure * mean)."""
    n = np.asarray(count, dtype=U32)
    mean, m2, m = mom[..., 0], mom[..., 1], mom[..., 2].view(U32)
    e, f = F32(exposure), F32(floor)
    with np.errstate(all="ignore"):
        var = m2 / (np.maximum(m, U32(1)) - U32(1)).astype(F32)
        se = np.sqrt(var / (n >> 3).astype(F32))
        err = (e * se) / (f + e * mean)
    return np.where(m < 2, F32(np.inf), err).astype(F32)


np_error = error  # the name the older tests use


def active(count, err, samples, threshold, min_spp, max_spp):
    """n + samples <= maxSamples and (n < minSamples or err > threshold): a NaN error is not above any threshold, +inf is."""
    n = np.asarray(count).astype(np.uint64)
    with np.errstate(all="ignore"):
        return (n + np.uint64(samples) <= np.uint64(max_spp)) & ((n < np.uint64(min_spp)) | (err > F32(threshold)))


active_set = active


def resolve(total, count, exposure):
    """exposure * (sum / (float)count), +0 where the count is 0."""
    total = np.asarray(total, dtype=F32)
    count = np.asarray(count, dtype=U32)
    with np.errstate(all="ignore"):
        out = F32(exposure) * (total / count.astype(F32)[..., None])
    out[count == 0] = F32(0)
    return out.astype(F32)


# ---- synthetic accumulator states: what prt_hip_accum_import and prt_hip_accum_import_moments accept and no render produces
def zero_denominator_mean(exposure, floor=FLOOR):
    """A float32 mean with floor + exposure * mean == 0 exactly in float32."""
    e, f = F32(exposure), F32(floor)
    c = -f / e
    for step in range(9):
        for cand in (c,) if step == 0 else (_walk(c, step), _walk(c, -step)):
            if f + e * cand == 0:
                return cand
    raise ValueError(f"no float32 mean cancels floor {floor} at exposure {exposure}")


def _walk(x, steps):
    for _ in range(abs(steps)):
        x = np.nextafter(x, F32(np.inf if steps > 0 else -np.inf), dtype=F32)
    return x


COUNT_CLASSES = (0, 7, 8, 16, 64, TOP - 8, TOP)
M_CLASSES = (0, 1, 2, 3, 1 << 21)
M2_CLASSES = (("+0", 0.0), ("denormal", DENORMAL), ("1e-30", 1e-30), ("1", 1.0), ("1e30", 1e30), ("+inf", np.inf), ("nan", np.nan), ("-1", -1.0))
MEAN_CLASSES = (("+0", 0.0),) + tuple((f"-floor/{e}", float(zero_denominator_mean(e))) for e in EXPOSURES) + \
    (("-1", -1.0), ("denormal", DENORMAL), ("0.5", 0.5), ("3e38", 3e38), ("nan", np.nan))
SUM_CLASSES = ("+0", "-0", "denormal", "ordinary", "+inf", "nan")
CROSS = list(itertools.product(range(len(COUNT_CLASSES)), range(len(M_CLASSES)), range(len(M2_CLASSES)), range(len(MEAN_CLASSES))))
MIN_FILLER = 1024

State = collections.namedtuple("State", "rng sum count mom label")


def synthetic_state(width, height, seed):
    """(rng, sum, count, mom, label) of a width x height accumulator built class by class: the full cross product of COUNT_CLASSES x
    M_CLASSES x M2_CLASSES x MEAN_CLASSES, one pixel each at seeded scattered positions, with the sum components running through
    SUM_CLASSES so that every sum class meets every count class; every other pixel is ordinary filler (m == count / 8, M2 > 0,
    mean > 0, a finite positive sum).  label[y, x] names the pixel's class."""
    n = width * height
    assert n >= len(CROSS) + MIN_FILLER, (width, height, len(CROSS))
    g = np.random.default_rng(seed)
    place = g.permutation(n)
    count, m = np.zeros(n, U32), np.zeros(n, U32)
    mean, m2 = np.zeros(n, F32), np.zeros(n, F32)
    total = np.zeros((n, 3), F32)
    label = np.empty(n, dtype=object)
    ordinary = (g.lognormal(0.0, 1.5, (n, 3)) * np.where(g.random((n, 3)) < 0.25, -1.0, 1.0)).astype(F32)
    sum_value = {"+0": F32(0.0), "-0": F32(-0.0), "denormal": F32(DENORMAL), "+inf": F32(np.inf), "nan": F32(np.nan)}
    for k, (ci, mi, vi, ai) in enumerate(CROSS):
        p = place[k]
        count[p], m[p], m2[p], mean[p] = COUNT_CLASSES[ci], M_CLASSES[mi], M2_CLASSES[vi][1], MEAN_CLASSES[ai][1]
        names = [SUM_CLASSES[(k + 2 * c + (k // len(SUM_CLASSES)) * c) % len(SUM_CLASSES)] for c in range(3)]
        for c, name in enumerate(names):
            total[p, c] = ordinary[p, c] if name == "ordinary" else sum_value[name]
        label[p] = f"n={COUNT_CLASSES[ci]} m={M_CLASSES[mi]} M2={M2_CLASSES[vi][0]} mean={MEAN_CLASSES[ai][0]} sum=({','.join(names)})"
    rest = place[len(CROSS):]
    packets = g.integers(2, 17, len(rest)).astype(U32)  # 16 .. 128 samples
    count[rest], m[rest] = packets * 8, packets
    mu = g.lognormal(-1.0, 1.0, len(rest))
    rel = g.lognormal(-1.5, 0.7, len(rest))  # the packets' relative spread
    mean[rest] = mu.astype(F32)
    m2[rest] = ((mu * rel) ** 2 * (packets - 1)).astype(F32)
    total[rest] = (np.abs(ordinary[rest]) * packets[:, None]).astype(F32)
    label[rest] = "filler"
    mom = np.zeros((n, 4), F32)
    mom[:, 0], mom[:, 1], mom[:, 2] = mean, m2, m.view(F32)
    rng = g.integers(1, 1 << 32, n, dtype=np.uint64).astype(U32)
    return State(rng.reshape(height, width), total.reshape(height, width, 3), count.reshape(height, width), mom.reshape(height, width, 4),
                 label.reshape(height, width))


def tile_state(state, width, height):
    """The state repeated over a larger image (cropped at its right and lower edge)."""
    h, w = state.count.shape
    ry, rx = -(-height // h), -(-width // w)
    rep = lambda a: np.ascontiguousarray(np.tile(a, (ry, rx) + (1,) * (a.ndim - 2))[:height, :width])  # noqa: E731
    return State(*(rep(a) for a in state))


def selection_cases(state, exposure=SELECT_EXPOSURE, floor=FLOOR):
    """The selection passes the tests run on a synthetic state, as (pixel, [(threshold, min_spp, max_spp), ...]).  The thresholds come
    from the reference's error e of one finite pixel, the filler pixel of median error among those whose count lets the error decide
    under every (min_spp, max_spp) below: e itself (err > e is false: that pixel is inactive), the float32 just below it (active), and 0."""
    err = error(state.count, state.mom, exposure, floor)
    ok = (state.label == "filler") & (state.count >= 16) & (state.count <= 56) & np.isfinite(err) & (err > 0)
    ys, xs = np.nonzero(ok)
    k = np.argsort(err[ok], kind="stable")[len(ys) // 2]
    pixel = (int(ys[k]), int(xs[k]))
    e = err[pixel]
    below = np.nextafter(e, F32(0), dtype=F32)
    cases = [(float(t), lo, hi) for t in (e, below, F32(0)) for lo in (0, 16) for hi in (64, TOP)]
    return pixel, cases


def selection_groups(count, mom, err, samples, min_spp, max_spp):
    """The pixel groups in which both outcomes of the rule have to occur (boolean masks by name)."""
    m = mom[..., 2].view(U32)
    n = count.astype(np.uint64)
    return {"err NaN": np.isnan(err), "err +inf with m < 2": (m < 2) & np.isposinf(err), "err finite": np.isfinite(err),
            "n < minSamples": n < min_spp, "n + samples > maxSamples": n + samples > max_spp}
