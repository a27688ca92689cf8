"""The two preview filters under non-finite and hostile state, without a GPU (include/prt_hip.h "denoised previews" and "temporal
reprojection": "what follows for non-finite state"; states and the scalar restatement: tests/prt_hostile_state.py).

  scalar against array   the restatements the GPU tests compare with (prt_denoise_ref, prt_temporal_ref) equal, word for word, a second
                         restatement written pixel by pixel from the header's text -- on states with NaN, inf, negative and denormal
                         values in every plane.  A NaN albedo demodulates by 1/64 (max(a, b) is a > b ? a : b), which np.maximum, the
                         earlier form of both restatements, got wrong: a 1 x 1 image and the island show it.
  the footprint law      derived from the tap offsets alone and checked on the array restatement: one non-finite channel of one pixel
                         of a fully valid image makes exactly the clipped square |dx|, |dy| <= 2*(2^k - 1) non-finite
  the variance plane     a NaN V is unknown (-1) for good and touches nobody; a +inf V takes its neighbours with it
  not vacuous            on the states the GPU tests use: the columns beyond the band's reach are finite, enough of the image is finite,
                         enough is not, enough variances stay known, and the hostile history is taken by some pixels and not by others
  rendered cases         which stored images of tests/golden/hostile_shade.npz keep a finite share the GPU test can compare"""
import numpy as np
import pytest

import prt_adaptive_ref as AR
import prt_denoise_ref as R
import prt_hostile_state as HS
import prt_temporal_ref as TR
from prt_temporal_ref import PARAMETER_SETS

F = np.float32
NAN, INF = float("nan"), float("inf")
SMALL = [(13, 9), (5, 3), (1, 1)]


def state_args(s):
    return s.state["sum"], s.state["count"], s.mom, s.albedo, s.normal


# ----------------------------------------------------------------------------- scalar against array
@pytest.mark.parametrize("sources", HS.SOURCES)
@pytest.mark.parametrize("size", SMALL)
def test_scalar_and_array_restatement_agree_on_the_denoiser(size, sources):
    w, h = size
    s = HS.hostile_state(w, h, 11, sources)
    for iterations in (1, 2, 3):
        for demodulate in (False, True):
            for power in (0, 7):
                kw = dict(iterations=iterations, demodulate=demodulate, normal_power_log2=power, exposure=1.0 if demodulate else 0.75)
                img, var = R.denoise(*state_args(s), **kw)
                want, want_var = HS.denoise_scalar(*state_args(s), **kw)
                AR.assert_words_equal(img, want, f"{w}x{h} {sources} {kw}: image", s.label)
                AR.assert_words_equal(var, want_var, f"{w}x{h} {sources} {kw}: variance", s.label)
                if sources != "all":  # nothing is compared NaN for NaN here
                    assert np.isfinite(img).all(), (size, sources, kw)


@pytest.mark.parametrize("sources", HS.SOURCES)
@pytest.mark.parametrize("size", SMALL)
def test_scalar_and_array_restatement_agree_on_the_temporal_stage(size, sources):
    w, h = size
    kw, s, _ = HS.temporal_state(w, h, 12, sources)
    took = 0
    for k, tp in enumerate(PARAMETER_SETS):
        m, ms = TR.merge(**kw, **tp), HS.merge_scalar(**kw, **tp)
        assert (m["have"] == ms["have"]).all(), (size, sources, tp)
        took += int(m["have"].sum())
        for iterations in (1, 2, 3):
            for demodulate in (False, True):
                p = dict(iterations=iterations, demodulate=demodulate, normal_power_log2=(0, 7)[(iterations + k) % 2])
                img, var, pend = TR.denoise_temporal(**kw, **tp, **p)
                want, want_var, want_pend = HS.denoise_temporal_scalar(**kw, **tp, **p)
                what = f"{w}x{h} {sources} {tp} {p}"
                AR.assert_words_equal(img, want, what + ": image", s.label)
                AR.assert_words_equal(var, want_var, what + ": variance", s.label)
                for key in ("color_var", "pos_len", "normal"):
                    AR.assert_words_equal(pend[key], want_pend[key], f"{what}: pending {key}", s.label)
    assert took > 0 or w * h == 1, (size, sources)  # (the 1 x 1 history has one pixel, which may stand for nothing)


def nan_albedo_cases():
    one = HS.hostile_state(1, 1, 5)
    island = HS.hostile_state(13, 9, 5, "island")
    return [(one, (0, 0)), (island, tuple(int(v[0]) for v in np.nonzero(island.label == "island, albedo NaN")))]


def test_a_nan_albedo_demodulates_by_one_64th():
    """d_p = max(A_p, 1/64) is A_p > 1/64 ? A_p : 1/64, so a NaN albedo channel demodulates by 1/64 and the pixel, which has no other tap
    (a 1 x 1 image; the island through iterations 0..2), comes out as exposure * ((c / d) * d) in every channel: finite.  np.maximum
    keeps the NaN -- the restatements used it, and gave NaN here where the kernels give a number."""
    assert np.isnan(np.maximum(F(NAN), F(0.015625))) and np.where(F(NAN) > F(0.015625), F(NAN), F(0.015625)) == F(0.015625)
    for s, p in nan_albedo_cases():
        assert s.label[p] == "island, albedo NaN" and np.isnan(s.albedo[p]).sum() == 1 and s.state["count"][p] > 0
        a = s.albedo[p]
        d = np.where(a > F(0.015625), a, F(0.015625)).astype(F)
        c = (s.state["sum"][p] / F(s.state["count"][p])).astype(F)
        want = F(0.5) * ((c / d).astype(F) * d)
        assert np.isfinite(want).all()
        for iterations in (1, 2, 3):
            img, _ = R.denoise(*state_args(s), iterations=iterations, demodulate=True, exposure=0.5)
            AR.assert_words_equal(img[p], want, f"denoise, {iterations} iterations")
            h, w = s.label.shape
            img, _, pend = TR.denoise_temporal(*state_args(s), np.ones((h, w, 4), F), None, iterations=iterations, demodulate=True, exposure=0.5)
            AR.assert_words_equal(img[p], want, f"denoise_temporal, {iterations} iterations")
            AR.assert_words_equal(pend["color_var"][p][:3], c, "pending: radiance, not demodulated")


# ----------------------------------------------------------------------------- the footprint law
LAW_SIZE = (48, 40)
LAW_PIXELS = [(20, 17), (1, 0), (47, 39), (45, 2)]


def test_the_law_from_the_tap_offsets_is_the_clipped_square():
    shape = (LAW_SIZE[1], LAW_SIZE[0])
    for x, y in LAW_PIXELS + [(0, 39), (24, 20)]:
        src = np.zeros(shape, bool)
        src[y, x] = True
        for k in range(6):
            assert (HS.footprint(src, k) == HS.square(shape, x, y, k)).all(), (x, y, k)
    assert [HS.reach(k) for k in range(1, 6)] == [2, 6, 14, 30, 62] and 2 * HS.reach(5) + 1 == 125


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_one_bad_channel_poisons_exactly_the_square(value, demodulate):
    w, h = LAW_SIZE
    s = HS.tame_state(w, h, 21, holes=False)
    assert (s.state["count"] > 0).all()
    for n, (x, y) in enumerate(LAW_PIXELS):
        total = s.state["sum"].copy()
        total[y, x, n % 3] = value
        src = np.zeros((h, w), bool)
        src[y, x] = True
        for k in (1, 2, 3, 4, 5):
            img, var = R.denoise(total, s.state["count"], s.mom, s.albedo, s.normal, iterations=k, demodulate=demodulate)
            bad = HS.nonfinite(img)
            assert (bad == HS.footprint(src, k)).all(), (value, demodulate, (x, y), k, int(bad.sum()))
            if np.isinf(value) and k == 1:  # an infinity keeps its own pixel (every other tap there has weight 0) and is NaN elsewhere
                assert np.isinf(img[y, x]).any() and not np.isnan(img[y, x]).any()
                assert np.isnan(img[bad & ~src]).any(-1).all()
            else:
                assert np.isnan(img[bad]).any(-1).all() and not np.isinf(img).any()
            assert not np.isinf(var).any()  # a variance that met the colour is NaN, which the next iteration reads as unknown


def test_a_nan_variance_is_unknown_for_good_and_an_infinite_one_spreads():
    w, h = LAW_SIZE
    s = HS.tame_state(w, h, 22, holes=False)
    x, y = 20, 17
    clean = {k: R.denoise(*state_args(s), iterations=k) for k in (1, 2, 5)}
    assert all((v >= 0).all() and np.isfinite(v).all() for _, v in clean.values())
    mom = s.mom.copy()
    mom[y, x, 1] = NAN
    for k in (1, 2, 5):
        img, var = R.denoise(s.state["sum"], s.state["count"], mom, s.albedo, s.normal, iterations=k)
        assert var[y, x] == -1 and np.isfinite(img).all()
        others = np.ones((h, w), bool)
        others[y, x] = False
        assert (var[others] >= 0).all() and np.isfinite(var).all()
    mom[y, x, 1] = INF
    lost = []
    for k in (1, 2, 5):
        img, var = R.denoise(s.state["sum"], s.state["count"], mom, s.albedo, s.normal, iterations=k)
        assert np.isfinite(img).all()  # an infinite V makes den infinite and wl = f(0) = 1: the colours stay finite
        gone = ~(np.isfinite(var) & (var >= 0))
        assert gone[y, x] and not (gone & ~HS.square((h, w), x, y, k)).any()
        lost.append(int(gone.sum()))
    print("pixels whose V one infinite V took after 1, 2, 5 iterations:", lost)
    assert lost[0] > 1 and lost[2] > lost[0]


# ----------------------------------------------------------------------------- the comparisons of the GPU tests are not vacuous
BIG = (131, 37)


@pytest.fixture(scope="module")
def big():
    return HS.hostile_state(*BIG, 1)


@pytest.mark.parametrize("demodulate", [False, True])
def test_the_band_keeps_the_rest_of_the_image_finite(big, demodulate):
    w, h = BIG
    assert (np.nonzero(HS.nonfinite(big.state["sum"]) | HS.nonfinite(big.albedo) | HS.nonfinite(big.normal) | HS.nonfinite(big.mom[..., 1]))[1]
            < HS.BAND).all()
    classes = set(big.label.reshape(-1))
    for name in ("sum NaN", "sum +inf, one channel", "sum -inf", "albedo NaN", "albedo +inf", "normal NaN", "normal x 40", "M2 NaN", "M2 +inf",
                 "count < 8, m >= 2", "sum 0x7fc12345", "sum 0xffc00000", "sum 0x7f800001", "sum negative", "sum -0.0", "sum denormal",
                 "albedo negative", "albedo 3.0", "M2 negative", "M2 -0.0", "count % 8, m < 2", "normal 1.04", "island", "island, albedo NaN"):
        assert name in classes, name
    with np.errstate(all="ignore"):
        v0 = (big.mom[..., 1] / F(1)) / (big.state["count"] >> 3).astype(F)
    assert np.isposinf(v0[big.label == "count < 8, m >= 2"]).all()
    for k in (1, 2, 5):
        img, var = R.denoise(*state_args(big), iterations=k, demodulate=demodulate)
        x0 = HS.BAND + HS.reach(k)
        fine = ~HS.nonfinite(img)
        known = float((var[:, x0:] >= 0).mean())
        print(f"{w}x{h}, {k} iterations, demodulate {int(demodulate)}: {fine.mean():.3f} finite, {known:.3f} of V known in the columns x >= {x0}")
        assert x0 < w and fine[:, x0:].all(), k                            # first condition
        assert known >= 0.30 and np.isfinite(var[:, x0:]).all(), (k, known)  # fourth condition
        if k == 5:
            assert fine.mean() >= 0.40, fine.mean()                        # second condition
            assert 1.0 - fine.mean() >= 0.10, fine.mean()                  # third condition
        if k <= 3:  # the NaN-albedo island has no other tap yet
            assert fine[big.label == "island, albedo NaN"].all()


def test_the_quiet_state_keeps_every_colour_finite():
    for size in (BIG, (65, 5), (64, 4), (5, 3)):
        s = HS.hostile_state(*size, 1, "quiet")
        assert {"M2 NaN", "M2 +inf", "count < 8, m >= 2"} <= set(s.label.reshape(-1)), size
        for k in (1, 5):
            img, var = R.denoise(*state_args(s), iterations=k)
            assert np.isfinite(img).all(), (size, k)
            assert k > 1 or not np.isfinite(var).all(), size  # (later iterations may have read every such V as unknown)


def test_the_hostile_history_is_taken_and_refused():
    w, h = BIG
    kw, s, _ = HS.temporal_state(w, h, 1)
    hist = kw["history"]
    for plane, column in (("color_var", slice(0, 3)), ("color_var", 3), ("pos_len", 3), ("normal", slice(0, 3))):
        values = hist[plane][..., column]
        assert np.isnan(values).any() and np.isinf(values).any(), (plane, column)
    assert (hist["color_var"] < 0).any() and (hist["pos_len"][..., 3] == F(1e-40)).any() and np.signbit(hist["pos_len"][..., 3]).any()
    own = TR.merge(**dict(kw, history=None))
    for tp in PARAMETER_SETS:
        m = TR.merge(**kw, **tp)
        frac = m["have"].mean()
        entered = m["have"] & HS.nonfinite(m["cm"]) & ~HS.nonfinite(own["cm"])  # finite samples, a non-finite merged colour
        print(f"{w}x{h} {tp}: {frac:.3f} of the pixels take history, {int(entered.sum())} of them a non-finite colour")
        assert 0.02 < frac < 0.98, (tp, frac)
        assert entered.any() and np.nonzero(entered)[1].max() < HS.BAND
        assert not np.isfinite(m["vm"][m["have"]]).all() and np.nonzero(~np.isfinite(m["vm"]))[1].max() < HS.BAND
        for k in (1, 5):
            img, var, _ = TR.denoise_temporal(**kw, **tp, iterations=k)
            x0 = HS.BAND + HS.reach(k)
            assert (~HS.nonfinite(img))[:, x0:].all() and (var[:, x0:] >= 0).mean() >= 0.30, (tp, k)
    ms = HS.merge_scalar(**kw, **PARAMETER_SETS[1])
    assert ms["taken"].any() and (ms["have"] == TR.merge(**kw, **PARAMETER_SETS[1])["have"]).all()


# ----------------------------------------------------------------------------- rendered cases
def test_rendered_cases_that_keep_a_finite_share():
    """By the law, from the stored reference images (8 spp): the closed boxes box_nan and box_inf are non-finite everywhere after one
    iteration (0.000 finite), the open stage `nonfinite` keeps 0.495 after one iteration and 0.192 after two.  With at least 25 % finite
    and 5 % non-finite, one pair is left for tests/test_gpu_hostile_state.py."""
    every = HS.rendered_cases(0.0, 0.0)
    for name, k, share in every:
        print(f"{name}, {k} iterations: {share:.3f} of the pixels predicted finite")
    assert len(every) == 6
    assert [(n, k) for n, k, _ in HS.rendered_cases()] == [("nonfinite", 1)]
