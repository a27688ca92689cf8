"""The numpy restatement of the adaptive estimator (tests/prt_adaptive_ref.py) checked on its own, without a GPU, so that the GPU
tests that hold the kernels to it word for word (test_gpu_adaptive_exact.py) cannot pass vacuously: the arithmetic keeps denormals,
the Welford fold is a mean and a sum of squared deviations, the synthetic state holds every class it promises, its errors take
every kind of value, and the selection rule has both outcomes in every group of pixels."""
import numpy as np
import pytest

import prt_adaptive_ref as R

F32, U32 = np.float32, np.uint32
W, H, SEED = 67, 61, 14


@pytest.fixture(scope="module")
def state():
    return R.synthetic_state(W, H, SEED)


def test_denormals_survive_in_this_process():
    d = F32(R.DENORMAL)
    assert d != 0 and d * F32(1) != 0 and F32(1e-40) * F32(1) != 0
    assert np.sqrt(np.full(4, d, dtype=F32))[0] == F32(np.sqrt(np.float64(d)))
    assert (np.full(4, d, dtype=F32) / F32(3))[0] != 0


def test_assert_words_equal_excepts_only_nan_pairs():
    nan_a, nan_b = U32(0x7fc00000).view(F32), U32(0xffc01234).view(F32)
    R.assert_words_equal(np.array([nan_a, 1.0, -0.0, np.inf], F32), np.array([nan_b, 1.0, -0.0, np.inf], F32), "equal up to NaN payloads")
    for got, want in (([0.0], [-0.0]), ([np.nan], [1.0]), ([1.0], [np.nan]), ([1.0], [np.nextafter(F32(1), F32(2))]), ([np.inf], [-np.inf]),
                      ([R.DENORMAL], [0.0])):
        with pytest.raises(AssertionError, match="1 of 1 words differ"):
            R.assert_words_equal(np.array(got, F32), np.array(want, F32), "must differ")
    label = np.array(["first", "second"], dtype=object)
    with pytest.raises(AssertionError, match=r"\[second\]"):
        R.assert_words_equal(np.array([[1, 2], [3, 4]], F32), np.array([[1, 2], [3, 5]], F32), "names the class", label)


def test_welford_fold_is_mean_and_sum_of_squared_deviations():
    """12 lognormal packets per pixel against a float64 two-pass mean and sum of squared deviations of the float32 luminances.  The
    bounds are four times what this draw gives (relative differences 2.13e-7 for the mean, 3.29e-7 for M2: a few float32 roundings
    over 12 folds); a fold in another order or with another divisor is off by orders of magnitude more."""
    g = np.random.default_rng(5)
    P = g.lognormal(0.0, 1.0, (12, 64, 64, 3)).astype(F32)
    mom = R.welford_fold(P, np.full((64, 64), 12))
    assert (mom[..., 2].view(U32) == 12).all() and (mom[..., 3] == 0).all()
    L = R.luminance(P).astype(np.float64)
    mean = L.mean(0)
    m2 = ((L - mean) ** 2).sum(0)
    rel_mean = float(np.max(np.abs(mom[..., 0] - mean) / mean))
    rel_m2 = float(np.max(np.abs(mom[..., 1] - m2) / m2))
    print(f"welford_fold vs float64 two-pass: mean {rel_mean:.2e}, M2 {rel_m2:.2e}")
    assert rel_mean <= 8.6e-7 and rel_m2 <= 1.4e-6, (rel_mean, rel_m2)
    # per-pixel packet counts: a pixel folds its first packets only, and one without packets keeps the empty record
    packets = g.integers(0, 13, (64, 64))
    part = R.welford_fold(P, packets)
    assert (part[..., 2].view(U32) == packets).all()
    for k in (0, 1, 5):
        sel = packets == k
        assert sel.any()
        R.assert_words_equal(part[sel], R.welford_fold(P[:k], np.full((64, 64), k))[sel] if k else np.zeros((int(sel.sum()), 4), F32), f"{k} packets")
    one = R.welford_fold(P, np.ones((64, 64), dtype=int))
    R.assert_words_equal(one[..., 0], R.luminance(P[0]), "mean after one packet = L")
    assert (one[..., 1] == 0).all()
    R.assert_words_equal(R.ordered_sum(P, packets)[packets == 3], ((P[0] + P[1]) + P[2])[packets == 3], "ordered sum of three packets")


def test_synthetic_state_contains_every_class(state):
    count, m = state.count, state.mom[..., 2].view(U32)
    mean, m2 = state.mom[..., 0], state.mom[..., 1]
    for v in (0, 7, 8, 16, 64, (1 << 24) - 8, 1 << 24):
        assert (count == v).sum() >= len(R.CROSS) // 7, v
    for v in (0, 1, 2, 3, 1 << 21):
        assert (m == v).sum() >= len(R.CROSS) // 5, v
    assert int(count.max()) <= 1 << 24 and int(m.max()) <= 1 << 21  # what the imports accept
    denormal = lambda a: (a != 0) & (np.abs(a) < np.finfo(F32).tiny)  # noqa: E731
    plus_zero = lambda a: R.bits(a) == 0  # noqa: E731
    for name, has in (("+0", plus_zero(m2)), ("denormal", denormal(m2)), ("1e-30", m2 == F32(1e-30)), ("1", m2 == 1), ("1e30", m2 == F32(1e30)),
                      ("+inf", np.isposinf(m2)), ("NaN", np.isnan(m2)), ("-1", m2 == -1)):
        assert has.sum() >= len(R.CROSS) // 8, ("M2", name)
    for e in R.EXPOSURES:
        with np.errstate(all="ignore"):
            assert ((F32(R.FLOOR) + F32(e) * mean) == 0).sum() >= len(R.CROSS) // 8, ("a denominator of exactly 0 at exposure", e)
    for name, has in (("+0", plus_zero(mean)), ("-1", mean == -1), ("denormal", denormal(mean)), ("0.5", mean == 0.5), ("3e38", mean == F32(3e38)),
                      ("NaN", np.isnan(mean))):
        assert has.sum() >= len(R.CROSS) // 8, ("mean", name)
    s = state.sum
    for c in range(3):
        for name, has in (("+0", plus_zero(s[..., c])), ("-0", R.bits(s[..., c]) == 0x80000000), ("denormal", denormal(s[..., c])),
                          ("ordinary", np.isfinite(s[..., c]) & (np.abs(s[..., c]) > 1e-3)), ("+inf", np.isposinf(s[..., c])), ("NaN", np.isnan(s[..., c]))):
            for v in (0, 7, 8, 16, 64, (1 << 24) - 8, 1 << 24):  # every sum class meets every count class, so every quotient of a resolve occurs
                assert (has & (count == v)).sum() >= 8, ("sum", c, name, v)
    # the full cross product, one pixel each, and the filler a render could have produced
    cross = state.label != "filler"
    assert cross.sum() == len(R.CROSS) == 7 * 5 * 8 * 8 and len(set(state.label[cross])) == len(R.CROSS)
    fill = ~cross
    assert fill.sum() >= R.MIN_FILLER and (m[fill] * 8 == count[fill]).all() and (m[fill] >= 2).all()
    assert (m2[fill] > 0).all() and (mean[fill] > 0).all() and np.isfinite(s[fill]).all() and (s[fill] > 0).all()
    assert (state.rng != 0).all() and (state.mom[..., 3] == 0).all()
    # scattered, not a block: both halves of the image and every third of its rows hold classes and filler
    for part in (cross[:, : W // 2], cross[:, W // 2:], cross[: H // 3], cross[H // 3: 2 * H // 3], cross[2 * H // 3:]):
        assert 0.3 < part.mean() < 0.8, part.mean()
    again = R.synthetic_state(W, H, SEED)
    assert all((R.bits(a) == R.bits(b)).all() for a, b in zip(state[1:4:2], again[1:4:2])) and (state.count == again.count).all()
    big = R.tile_state(state, 150, 130)
    assert big.count.shape == (130, 150) and big.mom.shape == (130, 150, 4) and big.sum.shape == (130, 150, 3)
    assert (big.count[H:2 * H, W:2 * W] == state.count).all() and (big.label[61 + 5, 67 + 3] == state.label[5, 3])


@pytest.mark.parametrize("exposure", R.EXPOSURES)
def test_restated_error_takes_every_kind_of_value(state, exposure):
    err = R.error(state.count, state.mom, exposure, R.FLOOR)
    assert err.dtype == F32
    b = R.bits(err)
    kinds = {"NaN": np.isnan(err), "+inf": np.isposinf(err), "-inf": np.isneginf(err), "+0": b == 0, "-0": b == 0x80000000,
             "finite > 0": np.isfinite(err) & (err > 0), "finite < 0": np.isfinite(err) & (err < 0)}
    print({k: int(v.sum()) for k, v in kinds.items()})
    for k, v in kinds.items():
        assert v.sum() >= 8, k
    m = state.mom[..., 2].view(U32)
    assert np.isposinf(err[m < 2]).all()  # +inf below two packets, whatever the record holds
    # n >> 3, not n / 8: a count of 7 divides by 0, and a positive variance over it gives an infinite error, not a finite one
    seven = (state.count == 7) & (m >= 2) & (state.mom[..., 1] == 1) & (state.mom[..., 0] == 0.5)
    assert seven.any() and np.isposinf(err[seven]).all()
    # +inf, NaN and a negative M2 come from the cross product only: the filler's errors are finite and positive
    fill = state.label == "filler"
    assert (np.isfinite(err[fill]) & (err[fill] > 0)).all()


def test_restated_rule_has_both_outcomes_in_every_group(state):
    """Over the passes test_gpu_adaptive_exact.py runs (thresholds e, the float32 below e and 0; minSamples 0 and 16; maxSamples 64 and
    2^24; 8 samples), every group of pixels holds at least 32 active pixels in one pass and at least 32 inactive ones in one pass.
    The groups are taken at minSamples 16 and maxSamples 64: under those a pixel with n < minSamples is always active and one with
    n + samples > maxSamples never, so their other outcome can only come from the passes with minSamples 0 and maxSamples 2^24."""
    pixel, cases = R.selection_cases(state)
    err = R.error(state.count, state.mom, R.SELECT_EXPOSURE, R.FLOOR)
    e = err[pixel]
    assert state.label[pixel] == "filler" and np.isfinite(e) and e > 0
    assert sorted({t for t, _, _ in cases}) == [0.0, float(np.nextafter(e, F32(0))), float(e)] and len(cases) == 12
    groups = R.selection_groups(state.count, state.mom, err, 8, 16, 64)
    most_on = {k: 0 for k in groups}
    most_off = {k: 0 for k in groups}
    for thr, lo, hi in cases:
        on = R.active(state.count, err, 8, thr, lo, hi)
        # the chosen pixel sits exactly on the threshold: > and >= differ on it
        assert bool(on[pixel]) == (thr < float(e)), (thr, lo, hi)
        assert 256 <= on.sum() <= on.size - 256, (thr, lo, hi, int(on.sum()))
        for k, gmask in groups.items():
            most_on[k] = max(most_on[k], int((on & gmask).sum()))
            most_off[k] = max(most_off[k], int((~on & gmask).sum()))
    print("active:", most_on, "inactive:", most_off)
    for k in groups:
        assert most_on[k] >= 32 and most_off[k] >= 32, (k, most_on[k], most_off[k])
    # within single passes, where the rule allows it: NaN never selects by itself, +inf always does, finite errors fall on both sides
    on = R.active(state.count, err, 8, float(e), 0, R.TOP)
    assert not on[np.isnan(err)].any() and on[np.isposinf(err) & (state.count <= R.TOP - 8)].all() and not on[state.count == R.TOP].any()
    fin = np.isfinite(err)
    assert (on & fin).sum() >= 32 and (~on & fin).sum() >= 32
    assert not on[R.bits(err) << 1 == 0].any() and not on[err < 0].any()  # threshold 0 and above: +-0 and negative errors are converged
    on16 = R.active(state.count, err, 8, float(e), 16, 64)
    assert on16[state.count < 16].all() and not on16[state.count > 56].any()
    assert (on16 & np.isnan(err)).sum() >= 32  # n < minSamples wins over a NaN error


def test_resolve_restated(state):
    for e in (1.0, 2.5, 0.0):
        img = R.resolve(state.sum, state.count, e)
        assert img.dtype == F32 and (R.bits(img[state.count == 0]) == 0).all()
        one = state.count == 16
        with np.errstate(all="ignore"):
            R.assert_words_equal(img[one], F32(e) * (state.sum[one] / F32(16)), f"exposure {e}")
    # exposure 0 keeps signs and non-finite sums: 0 * -x = -0, 0 * inf = NaN
    zero = R.resolve(state.sum, state.count, 0.0)
    live = state.count > 0
    assert np.isnan(zero[live][np.isinf(state.sum[live])]).all()
    assert (R.bits(zero[live][state.sum[live] < 0]) == 0x80000000).all()
