"""The a-trous denoiser (prt_denoise.hip) and the temporal merge (prt_temporal.hip) under non-finite and hostile state on the MI355X:
include/prt_hip.h "what follows for non-finite state".  States, the footprint law and the comparison are those of
tests/prt_hostile_state.py; tests/test_hostile_state_cpu.py holds the restatements to a second, scalar restatement and shows that what
is compared here is not one flood of NaN.  Everything is compared as uint32 words (prt_adaptive_ref.assert_words_equal: only NaN
against NaN is excepted), in the product build and in the test build of the library.

  synthetic state   image, denoise_variance() and, for the temporal filter, the pending record against the restatements: 131 x 37
                    (ragged in both directions against the kernels' 64 x 4 tile), 65 x 5, 64 x 4, 5 x 3, 1 x 1; "all" sources and the
                    "quiet" ones, which keep every colour finite, so that numbers are compared and not NaN with NaN
  the law           one NaN, then one inf pixel in a fully valid import: the output is non-finite exactly on the clipped square
  plain = temporal  without a history the two filters agree
  carry-over        a NaN pixel of frame 1 is NaN again in frame 2 through pending -> history, and finite after history_reset
  rendered state    the stage `nonfinite` of prt_hostile_shade after 16 samples: NaN and inf in sums AND guides
  display           the hostile image through display(): the restatement's bytes and meter figures, 0 bytes on the poisoned square
  pure read         accumulator, moments and history are exported as they were imported, NaN payloads included
Which of these fail under each flipped comparison of the two kernels: profiles/r23_hostile_state.txt."""
import functools

import numpy as np
import pytest

import prt_adaptive_ref as AR
import prt_amd
import prt_denoise_ref as R
import prt_display_ref as D
import prt_hostile_shade as S
import prt_hostile_state as HS
import prt_temporal_ref as TR
from prt_display_ref import assert_state_equal
from prt_gpukit import camera_of
from prt_gpukit import box_scene  # noqa: F401  (fixtures)
from prt_temporal_ref import PARAMETER_SETS

pytestmark = pytest.mark.gpu
F, U32 = np.float32, np.uint32
SIZES = [(131, 37), (65, 5), (64, 4), (5, 3), (1, 1)]
POWERS = (0, 5, 7)
SEED = 1


# (differs from prt_gpukit.tracer: every test runs on the product build and on the test build)
@pytest.fixture(scope="module", params=["product", "test"])
def tracer(request):
    prt_amd.build()
    t = prt_amd.PathTracer(test_entry_points=request.param == "test")
    yield t
    t.close()


def state_args(s):
    return s.state["sum"], s.state["count"], s.mom, s.albedo, s.normal


def load(t, s, camera):
    t.set_camera(camera)
    t.accum_import(s.state)
    t.accum_import_moments(s.mom)
    t.set_denoise_guides(s.albedo, s.normal)


# the restatements, once per argument set: both builds are held to the same arrays
@functools.lru_cache(maxsize=None)
def hostile(width, height, sources):
    return HS.hostile_state(width, height, SEED, sources)


@functools.lru_cache(maxsize=None)
def restated(width, height, sources, iterations, demodulate, power, exposure):
    return R.denoise(*state_args(hostile(width, height, sources)), iterations=iterations, demodulate=demodulate, normal_power_log2=power,
                     exposure=exposure)


@functools.lru_cache(maxsize=None)
def hostile_temporal(width, height, sources):
    return HS.temporal_state(width, height, SEED, sources)


@functools.lru_cache(maxsize=None)
def restated_temporal(width, height, sources, which, iterations, demodulate, power, exposure):
    kw = hostile_temporal(width, height, sources)[0]
    return TR.denoise_temporal(**kw, **PARAMETER_SETS[which], iterations=iterations, demodulate=demodulate, normal_power_log2=power,
                               exposure=exposure)


def strict_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = got.view(U32), want.view(U32)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} words differ"


# ----------------------------------------------------------------------------- synthetic hostile state against the restatement
@pytest.mark.parametrize("size", SIZES)
def test_denoiser_matches_the_restatement_on_hostile_state(tracer, box_scene, size):
    w, h = size
    tracer.upload_scene(box_scene)
    for sources in ("all", "quiet"):
        s = hostile(w, h, sources)
        load(tracer, s, camera_of(w, h))
        for iterations in (1, 2, 3, 4, 5):
            for demodulate in (False, True):
                for power in POWERS:
                    exposure = 1.0 if demodulate else 0.75
                    img = tracer.denoise(iterations=iterations, demodulate=demodulate, normal_power_log2=power, exposure=exposure)
                    var = tracer.denoise_variance()
                    want, want_var = restated(w, h, sources, iterations, demodulate, power, exposure)
                    what = f"{w}x{h} {sources}, {iterations} iterations, demodulate {int(demodulate)}, power {power}"
                    AR.assert_words_equal(img, want, what + ": image", s.label)
                    AR.assert_words_equal(var, want_var, what + ": variance", s.label)
        if sources == "quiet":
            assert np.isfinite(img).all()
    strict_equal(tracer.accum_export()["sum"], s.state["sum"], "sums after the denoises")
    strict_equal(tracer.accum_export_moments()[..., :3], s.mom[..., :3], "moments after the denoises")


@pytest.mark.parametrize("size", SIZES)
def test_temporal_filter_matches_the_restatement_on_hostile_state_and_history(tracer, box_scene, size):
    w, h = size
    tracer.upload_scene(box_scene)
    for sources in ("all", "quiet"):
        kw, s, cur = hostile_temporal(w, h, sources)
        load(tracer, s, cur)
        tracer.set_denoise_position(kw["position"])
        tracer.history_import(kw["history"])
        runs = [(k, bool(d), (k + d) % 3, POWERS[k % 3]) for k in (1, 2, 3, 4, 5) for d in (0, 1)] + [(5, True, which, 5) for which in range(3)]
        for iterations, demodulate, which, power in runs:
            exposure = 1.0 if demodulate else 0.75
            img = tracer.denoise_temporal(**PARAMETER_SETS[which], iterations=iterations, demodulate=demodulate, normal_power_log2=power,
                                          exposure=exposure)
            var = tracer.denoise_variance()
            pend = tracer.history_export(1)
            want, want_var, want_pend = restated_temporal(w, h, sources, which, iterations, demodulate, power, exposure)
            what = f"{w}x{h} {sources} {PARAMETER_SETS[which]}, {iterations} iterations, demodulate {int(demodulate)}, power {power}"
            AR.assert_words_equal(img, want, what + ": image", s.label)
            AR.assert_words_equal(var, want_var, what + ": variance", s.label)
            for key in ("color_var", "pos_len", "normal"):
                AR.assert_words_equal(pend[key], want_pend[key], f"{what}: pending {key}", s.label)
        got = tracer.history_export(0)
        for key in ("color_var", "pos_len", "normal"):
            strict_equal(got[key], kw["history"][key], f"history {key} after the denoises")


# ----------------------------------------------------------------------------- the footprint law on the device, without the restatement
@pytest.mark.parametrize("value,pixel", [(np.nan, (40, 20)), (np.inf, (129, 1)), (-np.inf, (3, 35))])
def test_one_bad_pixel_poisons_exactly_the_clipped_square(tracer, box_scene, value, pixel):
    w, h = 131, 37
    x, y = pixel
    s = HS.tame_state(w, h, 31, holes=False)
    s.state["sum"][y, x, 1] = value
    tracer.upload_scene(box_scene)
    load(tracer, s, camera_of(w, h))
    tracer.set_denoise_position(np.ones((h, w, 4), F))
    tracer.history_reset()
    for iterations in (1, 2, 3, 4, 5):
        for demodulate in (False, True):
            want = HS.square((h, w), x, y, iterations)
            for name, img in (("denoise", tracer.denoise(iterations=iterations, demodulate=demodulate)),
                              ("denoise_temporal", tracer.denoise_temporal(iterations=iterations, demodulate=demodulate))):
                bad = HS.nonfinite(img)
                assert (bad == want).all(), (name, value, pixel, iterations, demodulate, int(bad.sum()), int(want.sum()))
                if np.isinf(value) and iterations == 1:
                    assert np.isinf(img[y, x]).any() and not np.isnan(img[y, x]).any()
                    bad[y, x] = False
                assert np.isnan(img[bad]).any(-1).all()
            assert not np.isinf(tracer.denoise_variance()).any()


# ----------------------------------------------------------------------------- plain denoiser = temporal filter without a history
@pytest.mark.parametrize("size", [(131, 37), (5, 3), (1, 1)])
def test_without_history_both_filters_agree_on_hostile_state(tracer, box_scene, size):
    w, h = size
    kw, s, cur = hostile_temporal(w, h, "all")
    tracer.upload_scene(box_scene)
    load(tracer, s, cur)
    tracer.set_denoise_position(kw["position"])
    for reset in (True, False):
        if reset:
            tracer.history_reset()
        else:
            tracer.history_import(kw["history"])  # a hostile history that maxHistory = 0 switches off
        for p in (dict(), dict(demodulate=False, iterations=2, normal_power_log2=7), dict(iterations=1, normal_power_log2=0)):
            plain, plain_var = tracer.denoise(**p), tracer.denoise_variance()
            img = tracer.denoise_temporal(max_history=256.0 if reset else 0.0, **p)
            AR.assert_words_equal(img, plain, f"{w}x{h} {p} reset {reset}: image", s.label)
            AR.assert_words_equal(tracer.denoise_variance(), plain_var, f"{w}x{h} {p} reset {reset}: variance", s.label)


# ----------------------------------------------------------------------------- history carry-over
def test_a_nan_pixel_comes_back_through_the_history_until_history_reset(tracer, box_scene):
    w, h, k = 131, 37, 2
    x, y = 50, 18
    clean = HS.tame_state(w, h, 41, holes=False)
    dirty = HS.tame_state(w, h, 41, holes=False)
    dirty.state["sum"][y, x, 0] = np.nan
    cur, _ = HS.camera_pair(w, h, 41, 0.0)
    position = HS.plane_positions(cur)
    tp = PARAMETER_SETS[2]  # normalCos -1: the guide normals are short, and dot3(N_p, N_p) need not reach 0.9
    tracer.upload_scene(box_scene)
    tracer.history_reset()
    load(tracer, dirty, cur)
    tracer.set_denoise_position(position)
    first = tracer.denoise_temporal(**tp, iterations=k)
    assert (HS.nonfinite(first) == HS.square((h, w), x, y, k)).all()
    pend = tracer.history_export(1)
    assert np.isnan(pend["color_var"][y, x, 0]) and HS.nonfinite(pend["color_var"][..., :3]).sum() == 1
    # frame 2: the same camera set again promotes pending to history; a clean accumulator
    load(tracer, clean, cur)
    tracer.set_denoise_position(position)
    hist = tracer.history_export(0)
    for key in ("color_var", "pos_len", "normal"):
        strict_equal(hist[key], pend[key], f"history = pending of frame 1: {key}")
    args = dict(total=clean.state["sum"], count=clean.state["count"], mom=clean.mom, albedo=clean.albedo, normal=clean.normal, position=position)
    want, want_var, want_pend = TR.denoise_temporal(**args, history=hist, **tp, iterations=k)
    merged = HS.nonfinite(want_pend["color_var"][..., :3])  # the pixels whose accepted taps include (x, y)
    assert merged[y, x] and merged.sum() <= 9
    second = tracer.denoise_temporal(**tp, iterations=k)
    AR.assert_words_equal(second, want, "frame 2: image", clean.label)
    AR.assert_words_equal(tracer.denoise_variance(), want_var, "frame 2: variance", clean.label)
    AR.assert_words_equal(tracer.history_export(1)["color_var"], want_pend["color_var"], "frame 2: pending", clean.label)
    bad = HS.nonfinite(second)
    assert (bad == HS.footprint(merged, k)).all() and bad[HS.square((h, w), x, y, k)].all()
    assert np.isfinite(tracer.denoise(iterations=k)).all()  # the plain denoiser ignores the history
    tracer.history_reset()
    third = tracer.denoise_temporal(**tp, iterations=k)
    assert np.isfinite(third).all()
    AR.assert_words_equal(third, tracer.denoise(iterations=k), "after history_reset: the plain denoiser")


# ----------------------------------------------------------------------------- rendered state
@pytest.mark.parametrize("name,iterations", [(n, k) for n, k, _ in HS.rendered_cases()])
def test_rendered_hostile_state(tracer, name, iterations):
    scene, camera = S.scene(name)
    tracer.upload_scene(scene)
    tracer.history_reset()

    def frame():
        tracer.set_camera(camera)
        for spp in (8, 16):  # min_spp at the target: every pixel is traced, and the moments exist
            tracer.adaptive_pass(8, 0.0, spp, spp, 0.01, max_depth=14)
        state, mom = tracer.accum_export(), tracer.accum_export_moments()
        albedo, normal = tracer.denoise_guides()
        return dict(total=state["sum"], count=state["count"], mom=mom, albedo=albedo, normal=normal)

    s = frame()
    assert (s["count"] == 16).all() and (s["mom"][..., 2].view(U32) == 2).all()
    assert not np.isfinite(s["albedo"]).all(), "the guides hold no NaN or inf albedo"
    assert np.isnan(s["total"]).any() and not np.isfinite(s["total"]).all()
    p = dict(iterations=iterations, normal_power_log2=5)
    for demodulate in (True, False):
        want, want_var = R.denoise(s["total"], s["count"], s["mom"], s["albedo"], s["normal"], demodulate=demodulate, **p)
        share = float((~HS.nonfinite(want)).mean())
        print(f"{name}, {iterations} iterations, demodulate {int(demodulate)}: {share:.3f} of the denoised pixels finite")
        assert 0.0 < share < 1.0, share
        AR.assert_words_equal(tracer.denoise(demodulate=demodulate, **p), want, f"{name}: denoise, demodulate {demodulate}")
        AR.assert_words_equal(tracer.denoise_variance(), want_var, f"{name}: variance, demodulate {demodulate}")
    position = tracer.denoise_position()
    want, want_var, want_pend = TR.denoise_temporal(**s, position=position, history=None, **p)
    AR.assert_words_equal(tracer.denoise_temporal(**p), want, f"{name}: temporal, no history")
    pend = tracer.history_export(1)
    for key in ("color_var", "pos_len", "normal"):
        AR.assert_words_equal(pend[key], want_pend[key], f"{name}: pending {key}")
    assert not np.isfinite(pend["color_var"]).all()
    # the same view again: the rendered, non-finite record is the history now
    s2 = frame()
    hist = tracer.history_export(0)
    assert not np.isfinite(hist["color_var"]).all()
    tp = PARAMETER_SETS[1]
    m = TR.merge(**s2, position=position, history=hist, **tp)
    assert 0.02 < m["have"].mean() and (m["have"] & HS.nonfinite(m["cm"])).any()
    want, want_var, want_pend = TR.denoise_temporal(**s2, position=position, history=hist, **tp, **p)
    AR.assert_words_equal(tracer.denoise_temporal(**tp, **p), want, f"{name}: temporal with the rendered history")
    AR.assert_words_equal(tracer.denoise_variance(), want_var, f"{name}: variance with the rendered history")
    AR.assert_words_equal(tracer.history_export(1)["color_var"], want_pend["color_var"], f"{name}: pending with the rendered history")


# ----------------------------------------------------------------------------- chain into the display transform
def test_denoised_hostile_image_through_the_display(tracer, box_scene):
    w, h, k = 131, 37, 2
    s = hostile(w, h, "all")
    tracer.upload_scene(box_scene)
    load(tracer, s, camera_of(w, h))
    want, _ = restated(w, h, "all", k, True, 5, 1.0)
    tracer.denoise(iterations=k, demodulate=True, normal_power_log2=5, exposure=1.0)  # into the context's framebuffer
    assert np.isnan(want).any() and (~HS.nonfinite(want)).mean() > 0.5
    for p in (prt_amd.DisplayParams.make(tonemap=1, transfer=1, format=0, gain=0.8),
              prt_amd.DisplayParams.make(tonemap=0, transfer=0, format=0, meter=True, gain=1.25, adapt_rate=1.0)):
        tracer.display_reset()
        got = tracer.display(p)
        ref, state = D.display(want, p)
        assert np.array_equal(got, ref), (p.meter, int((got != ref).sum()))
        assert (got[np.isnan(want)] == 0).all()
        if p.meter:
            st = tracer.display_state()
            assert_state_equal(st, state, "meter of the denoised hostile image")
            assert st["metered"] + st["ignored"] == w * h and st["ignored"] >= int(np.isnan(want).all(-1).sum())
    # one NaN pixel, every channel: its whole square is black
    x, y = 70, 18
    one = HS.tame_state(w, h, 31, holes=False)
    one.state["sum"][y, x] = np.nan
    load(tracer, one, camera_of(w, h))
    img = tracer.denoise(iterations=k)
    sq = HS.square((h, w), x, y, k)
    assert np.isnan(img[sq]).all() and np.isfinite(img[~sq]).all()
    got = tracer.display(prt_amd.DisplayParams.make(tonemap=1, transfer=1, format=0, gain=1.0))
    assert (got[sq] == 0).all() and (got[~sq] != 0).any(-1).mean() > 0.9


# ----------------------------------------------------------------------------- a pure read
def test_everything_imported_is_exported_word_for_word(tracer, box_scene):
    w, h = 65, 5
    kw, s, cur = hostile_temporal(w, h, "all")
    words = s.state["sum"].view(U32)
    assert all((words == pattern).any() for pattern in HS.PAYLOADS)
    tracer.upload_scene(box_scene)
    load(tracer, s, cur)
    tracer.set_denoise_position(kw["position"])
    tracer.history_import(kw["history"])
    tracer.denoise()
    tracer.denoise_temporal(**PARAMETER_SETS[1])
    tracer.denoise(demodulate=False, iterations=1)
    tracer.denoise_temporal(demodulate=False, iterations=3)
    tracer.display(prt_amd.DisplayParams.make(meter=True))
    state = tracer.accum_export()
    strict_equal(state["sum"], s.state["sum"], "sums")
    strict_equal(state["count"], s.state["count"], "counts")
    strict_equal(state["rng"], s.state["rng"], "rng")
    strict_equal(tracer.accum_export_moments()[..., :3], s.mom[..., :3], "moments")
    hist = tracer.history_export(0)
    for key in ("color_var", "pos_len", "normal"):
        strict_equal(hist[key], kw["history"][key].astype(F), f"history {key}")
    albedo, normal = tracer.denoise_guides()
    strict_equal(albedo, s.albedo, "albedo guide")
    strict_equal(normal, s.normal, "normal guide")
    strict_equal(tracer.denoise_position(), kw["position"], "position guide")
