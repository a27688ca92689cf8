"""The adaptive estimator on the MI355X held to include/prt_hip.h ("adaptive sampling") word for word.  The moment records are
compared with the header's float32 Welford fold of EXACT packet sums (a pixel's packet depends only on its generator chain, so a
pass from a zeroed sum exports the packet's own sum); error, selection and resolve are run on synthetic accumulator states no
render produces (tests/prt_adaptive_ref.py: non-finite, denormal, negative, counts that are no multiple of 8, the 2^24 cap) and on
an image large enough for the grid-stride loops to repeat.  Every comparison is of uint32 words over every pixel; only NaN / NaN
pairs are excepted."""
import time

import numpy as np
import pytest

import prt_adaptive_ref as R
import prt_amd
import prt_testlib as T
from prt_gpukit import tracer  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
FLOOR = R.FLOOR
W = H = 64            # A and B: Cornell box + teapot
PACKETS = 12
SW, SH, SEED = 67, 61, 14  # C: 4087 pixels, the last block of 256 is ragged
SUB = (3, 5, 60, 50)


@pytest.fixture(autouse=True)
def tally(request):
    """Prints what a test compared and how long it took (-s shows it)."""
    before, t0 = R.words_compared, time.perf_counter()
    yield
    print(f"\n[{request.node.name}] {R.words_compared - before} words compared, {time.perf_counter() - t0:.2f} s")


# (differs from prt_gpukit.upload: takes the (scene, camera, exposure) tuple)
def upload(tracer, scene_camera):
    scene, camera, _ = scene_camera
    tracer.upload_scene(scene)
    tracer.set_camera(camera)


def make_state(tracer, rng, total, count):
    h, w = count.shape
    return dict(width=w, height=h, seed=tracer.seed, max_depth=tracer.max_depth, rr_depth=tracer.rr_depth, rng=rng, sum=total, count=count)


def import_state(tracer, s):
    tracer.accum_import(make_state(tracer, s.rng, s.sum, s.count))
    tracer.accum_import_moments(s.mom)


def m_of(mom):
    return mom[..., 2].view(U32)


# ---- A. exact packet sums
# (differs from prt_refit_ref.teapot_scene: a fixture, made once)
@pytest.fixture(scope="module")
def teapot_scene():
    return prt_amd.setup_cornell_box(W, H, teapot_mesh=T.teapot_product_mesh())


@pytest.fixture(scope="module")
def packets(tracer, teapot_scene):
    """P[j] (PACKETS, H, W, 3): the sum of packet j of every pixel, exactly.  color = sum + res, and res = +0 + r0 + ... + r7 is never
    -0, so a pass of 8 samples from a record whose sum was set to +0 (generator state and count kept) exports res itself."""
    upload(tracer, teapot_scene)
    tracer.accum_reset()
    P = np.zeros((PACKETS, H, W, 3), dtype=F32)
    for j in range(PACKETS):
        tracer.accumulate(8)
        st = tracer.accum_export()
        assert (st["count"] == 8 * (j + 1)).all()
        P[j] = st["sum"]
        st["sum"] = np.zeros_like(st["sum"])
        tracer.accum_import(st)
    tracer.accum_reset()
    P.setflags(write=False)
    return P


def test_packet_sums_are_exact(tracer, teapot_scene, packets):
    upload(tracer, teapot_scene)
    P0 = packets[0]
    assert (R.bits(packets) != 0x80000000).all(), "a packet sum is never -0"
    tiny = (P0 != 0) & (np.abs(P0) < F32(2.0 ** -120))
    assert not tiny.any(), "a component near underflow: / 8 and * 8 would not be exact"
    R.assert_words_equal(tracer.render(8, exposure=8.0), P0, "P[0] vs render(8) at exposure 8")
    rect = (24, 30, 39, 45)
    scene, camera, _ = teapot_scene
    ref, _ = T.OracleScene(T.scene_desc_from_product(scene, camera, 8.0)).render_rect(rect, 8, threads=16, stats=False)
    assert ref.shape == (16, 16, 3) and (ref != 0).any()
    R.assert_words_equal(P0[30:46, 24:40], ref, "P[0] vs the oracle's 8 samples at exposure 8")
    # the chain: the in-order sum of the first k packets is the accumulator of one pass of 8k samples, and the packets differ
    tracer.accum_reset()
    tracer.accumulate(40)
    R.assert_words_equal(tracer.accum_export()["sum"], R.ordered_sum(packets, np.full((H, W), 5)), "accumulate(40) vs P[0] + ... + P[4]")
    tracer.accum_reset()
    lum = R.luminance(packets)  # (most pixels of this box are black in most packets: its light is small and found by chance only)
    assert ((lum[1:] != lum[:-1]).mean(axis=(1, 2)) > 0.05).all(), "consecutive packets must differ: the generator chain moved on"


# ---- B. moments at tolerance 0
ALL = dict(thr=0.0, lo=8 * PACKETS, hi=8 * PACKETS)  # min = max: every pixel of the pass is active
MEDIAN = "the median of the reference's nonzero errors"
PART = dict(thr=MEDIAN, lo=16, hi=8 * PACKETS)
SCHEDULES = {
    "single packets": [dict(samples=8, **ALL)] * 4,
    "3 and 5 folds in one launch": [dict(samples=24, **ALL), dict(samples=40, **ALL)],
    "partly active": [dict(samples=8, **ALL)] * 2 + [dict(samples=8, share=True, **PART), dict(samples=8, **PART), dict(samples=24, **PART),
                                                     dict(samples=8, **PART)],
    "rectangle off the tile grid": [dict(samples=8, rect=(5, 7, 50, 41), **ALL)] * 2 +
                                   [dict(samples=8, rect=(5, 7, 50, 41), **PART), dict(samples=24, rect=(5, 7, 50, 41), **PART),
                                    dict(samples=8, rect=(0, 0, 30, 63), **PART)],
    "3 ranks, tile 8": [dict(samples=8, nranks=3, tile=8, **ALL), dict(samples=8, nranks=3, tile=8, **ALL),
                        dict(samples=16, nranks=3, tile=8, **PART), dict(samples=8, nranks=3, tile=8, rect=(5, 7, 50, 41), **PART)],
    "3 ranks, tile 32": [dict(samples=8, nranks=3, tile=32, **ALL), dict(samples=8, nranks=3, tile=32, **ALL),
                         dict(samples=16, nranks=3, tile=32, **PART), dict(samples=8, nranks=3, tile=32, rect=(5, 7, 50, 41), **PART)],
}


def check_share(err, want, scope, thr):
    """The first partly active pass really is one, counted on the reference.  Its threshold, the median of the nonzero errors after
    two packets, decides only about the pixels that HAVE a nonzero error: err > threshold >= 0 is false for every pixel whose two
    packets agree, and in this box (a small light, found by chance only) that is 82.2 % of the 4096 pixels, so no threshold could
    make a quarter of ALL pixels active here (the median makes 0.085 of them active: 348 pixels, 0.476 of the 731 it decides about).  Between a quarter and three
    quarters is therefore asked of the pixels the threshold decides about -- ties on the median, which a render produces in
    numbers, could still break that -- and both sides have to hold at least 256 pixels, four rows of 64 work items, so that the
    compacted launch has several rows and the pixels left out outnumber them."""
    decided = scope & np.isfinite(err) & (err > 0)
    share = want[decided].mean()
    print(f"\nnonzero errors: {decided.sum()} of {scope.sum()} pixels; above their median {thr!r}: {want.sum()} pixels, "
          f"{share:.3f} of the nonzero ones, {want.sum() / scope.sum():.3f} of all")
    assert not want[scope & ~decided].any() and decided.sum() >= 512
    assert 0.25 < share < 0.75, f"{share:.3f} of the pixels with a nonzero error are active at the median threshold"
    assert want.sum() >= 256 and (scope & ~want).sum() >= 256, (int(want.sum()), int((scope & ~want).sum()))


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_moments_are_the_headers_fold(tracer, teapot_scene, packets, name):
    """After every pass of the schedule, every pixel's exported moment record equals welford_fold of its first count / 8 exact packet
    sums, its sum their in-order float32 sum, and its count the reference's; the reference also decides who is active (the rule on
    the restated error of the restated moments).  A pixel the pass leaves out -- inactive, outside the rectangle, another rank's --
    keeps its words."""
    upload(tracer, teapot_scene)
    tracer.accum_reset()
    count = np.zeros((H, W), dtype=U32)
    thr_median = None
    partial = 0
    for k, ps in enumerate(SCHEDULES[name]):
        x0, y0, x1, y1 = ps.get("rect", (0, 0, W - 1, H - 1))
        inside = np.zeros((H, W), dtype=bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        nranks, tile = ps.get("nranks", 1), ps.get("tile", 16)
        thr = ps["thr"]
        if thr is MEDIAN:
            if thr_median is None:
                e = R.error(count, R.welford_fold(packets, count // 8), 1.0, FLOOR)[inside]
                thr_median = float(np.median(e[np.isfinite(e) & (e > 0)]))
            thr = thr_median
        for rank in range(nranks):
            mom_before, st_before = tracer.accum_export_moments(), tracer.accum_export()
            ref_mom = R.welford_fold(packets, count // 8)
            R.assert_words_equal(mom_before, ref_mom, f"{name}, before pass {k} rank {rank}: moments")
            err = R.error(count, ref_mom, 1.0, FLOOR)
            scope = inside & prt_amd.owned_pixel_mask(W, H, rank, nranks, tile)
            want = R.active(count, err, ps["samples"], thr, ps["lo"], ps["hi"]) & scope
            partial += int(0 < want.sum() < scope.sum())
            if ps.get("share"):
                check_share(err, want, scope, thr)
            _, active = tracer.adaptive_pass(ps["samples"], thr, ps["lo"], ps["hi"], FLOOR, x0, y0, x1, y1, exposure=1.0, rank=rank,
                                             nranks=nranks, tile=tile)
            assert active == int(want.sum()) == tracer.last_stats["nPx"], (name, k, rank, active, int(want.sum()))
            count = count + np.where(want, U32(ps["samples"]), U32(0)).astype(U32)
            mom, st = tracer.accum_export_moments(), tracer.accum_export()
            assert (st["count"] == count).all(), (name, k, rank, int((st["count"] != count).sum()))
            R.assert_words_equal(mom, R.welford_fold(packets, count // 8), f"{name}, pass {k} rank {rank}: moments vs welford_fold")
            R.assert_words_equal(st["sum"], R.ordered_sum(packets, count // 8), f"{name}, pass {k} rank {rank}: sums vs the in-order packet sum")
            assert (mom.view(U32)[~want] == mom_before.view(U32)[~want]).all(), f"{name}, pass {k} rank {rank}: a left-out pixel's moments moved"
            assert (st["rng"][~want] == st_before["rng"][~want]).all() and (st["rng"][want] != st_before["rng"][want]).sum() > 0.99 * want.sum()
    if name not in ("single packets", "3 and 5 folds in one launch"):
        assert partial >= 2, "the schedule never ran a pass with some pixels active and some not"
        assert len(np.unique(count)) >= 2, np.unique(count)


def test_accumulate_passes_leave_the_moments_alone(tracer, teapot_scene, packets):
    """Adaptive 16, accumulate 8, adaptive 8: the record folds packets 0, 1 and 3 and never packet 2, while the error uses the full
    n = 32 (n >> 3 = 4 packets under the square root, not the record's 3)."""
    upload(tracer, teapot_scene)
    tracer.accum_reset()
    tracer.adaptive_pass(16, 0.0, 96, 96, FLOOR)
    before = tracer.accum_export_moments()
    R.assert_words_equal(before, R.welford_fold(packets, np.full((H, W), 2)), "after two adaptive packets")
    tracer.accumulate(8)
    R.assert_words_equal(tracer.accum_export_moments(), before, "moments after an accumulate pass")
    _, active = tracer.adaptive_pass(8, 0.0, 96, 96, FLOOR)
    assert active == W * H
    mom, st = tracer.accum_export_moments(), tracer.accum_export()
    assert (st["count"] == 32).all() and (m_of(mom) == 3).all()
    R.assert_words_equal(mom, R.welford_fold(packets[[0, 1, 3]], np.full((H, W), 3)), "moments over packets 0, 1 and 3")
    R.assert_words_equal(st["sum"], R.ordered_sum(packets, np.full((H, W), 4)), "sums over packets 0 .. 3")
    for e in R.EXPOSURES:
        got = tracer.accum_error(e, FLOOR)
        R.assert_words_equal(got, R.error(st["count"], mom, e, FLOOR), f"accum_error at exposure {e}: the full n")
        lit = np.isfinite(got) & (got != 0)  # (with the record's own 3 packets under the root every error that is not 0 would differ)
        assert lit.sum() > 256 and (got != R.error(np.full((H, W), 24, dtype=U32), mom, e, FLOOR))[lit].all()
    tracer.accum_reset()


# ---- C. error, selection and resolve on synthetic states
@pytest.fixture(scope="module")
def synthetic():
    return R.synthetic_state(SW, SH, SEED)


@pytest.fixture(scope="module")
def synthetic_scene():
    return prt_amd.setup_cornell_box(SW, SH, teapot_mesh=T.teapot_product_mesh())


def whole_framebuffer(tracer, w, h):
    return tracer._download_rect(0, 0, w - 1, h - 1, stats=False)


def check_error_and_resolve(tracer, s, sub):
    """accum_error and accum_resolve of the imported state s over the whole image and over the rectangle sub, by words."""
    h, w = s.count.shape
    x0, y0, x1, y1 = sub
    cut = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    for e in R.EXPOSURES:
        want = R.error(s.count, s.mom, e, FLOOR)
        R.assert_words_equal(tracer.accum_error(e, FLOOR), want, f"accum_error at exposure {e}", s.label)
        R.assert_words_equal(tracer.accum_error(e, FLOOR, *sub), want[cut], f"accum_error at exposure {e} over {sub}", s.label[cut])
    for e in (1.0, 2.5, 0.0):
        R.assert_words_equal(tracer.accum_resolve(e), R.resolve(s.sum, s.count, e), f"accum_resolve at exposure {e}", s.label)
    # a rectangle's resolve leaves every pixel outside it as it was
    tracer.accum_resolve(1.0)
    R.assert_words_equal(tracer.accum_resolve(2.5, *sub), R.resolve(s.sum, s.count, 2.5)[cut], f"accum_resolve over {sub}", s.label[cut])
    want = R.resolve(s.sum, s.count, 1.0)
    want[cut] = R.resolve(s.sum, s.count, 2.5)[cut]
    R.assert_words_equal(whole_framebuffer(tracer, w, h), want, f"the framebuffer after a resolve over {sub}", s.label)


def test_error_and_resolve_on_synthetic_states(tracer, synthetic, synthetic_scene):
    upload(tracer, synthetic_scene)
    import_state(tracer, synthetic)
    st, mom = tracer.accum_export(), tracer.accum_export_moments()
    assert (st["count"] == synthetic.count).all() and (st["rng"] == synthetic.rng).all()
    assert (R.bits(st["sum"]) == R.bits(synthetic.sum)).all() and (R.bits(mom) == R.bits(synthetic.mom)).all()  # imports keep every word
    check_error_and_resolve(tracer, synthetic, SUB)


@pytest.fixture(scope="module")
def traced_rng(tracer, synthetic, synthetic_scene):
    """The generator state every pixel of the synthetic state has after 8 more samples: a pixel's chain depends on its state (its
    seed where the count is 0) and on nothing else of its record, so an accumulate pass from finite sums gives it."""
    upload(tracer, synthetic_scene)
    count = np.where(synthetic.count == 0, 0, 8).astype(U32)
    tracer.accum_import(make_state(tracer, synthetic.rng, np.zeros_like(synthetic.sum), count))
    tracer.accumulate(8)
    rng = tracer.accum_export()["rng"]
    tracer.accum_reset()
    return rng


def check_selection(tracer, s, traced, case, what, rank=0, nranks=1, samples=8):
    """One adaptive pass over the imported state s against the restated rule: who is active, what an active pixel gains, and what
    every other pixel shows."""
    thr, lo, hi = case
    h, w = s.count.shape
    import_state(tracer, s)
    fill = tracer.accum_resolve(R.FILL_EXPOSURE)
    err = R.error(s.count, s.mom, R.SELECT_EXPOSURE, FLOOR)
    owned = prt_amd.owned_pixel_mask(w, h, rank, nranks)
    want = R.active(s.count, err, samples, thr, lo, hi) & owned
    img, active = tracer.adaptive_pass(samples, thr, lo, hi, FLOOR, exposure=R.SELECT_EXPOSURE, rank=rank, nranks=nranks)
    assert active == int(want.sum()) == tracer.last_stats["nPx"], (what, active, int(want.sum()), tracer.last_stats["nPx"])
    st, mom = tracer.accum_export(), tracer.accum_export_moments()
    grew = st["count"] != s.count
    wrong = np.argwhere(grew != want)
    assert len(wrong) == 0, f"{what}: {len(wrong)} pixels selected against the rule, first {tuple(wrong[0])} [{s.label[tuple(wrong[0])]}] err {err[tuple(wrong[0])]!r}"
    assert (st["count"] == s.count + np.where(want, U32(samples), U32(0))).all(), what
    assert (m_of(mom) == m_of(s.mom) + np.where(want, U32(samples // 8), U32(0))).all(), what
    assert (st["rng"] == np.where(want, traced, s.rng)).all(), f"{what}: generator states"
    assert (R.bits(st["sum"])[~want] == R.bits(s.sum)[~want]).all() and (R.bits(mom)[~want] == R.bits(s.mom)[~want]).all(), what
    shown = owned & ~want
    R.assert_words_equal(img[shown], R.resolve(s.sum, s.count, R.SELECT_EXPOSURE)[shown], f"{what}: owned inactive pixels vs resolve", s.label[shown])
    R.assert_words_equal(img[~owned], fill[~owned], f"{what}: pixels of other ranks keep the fill", s.label[~owned])
    return int(want.sum())


def test_selection_on_synthetic_states(tracer, synthetic, synthetic_scene, traced_rng):
    upload(tracer, synthetic_scene)
    pixel, cases = R.selection_cases(synthetic)
    e = R.error(synthetic.count, synthetic.mom, R.SELECT_EXPOSURE, FLOOR)[pixel]
    sizes = set()
    for case in cases:
        sizes.add(check_selection(tracer, synthetic, traced_rng, case, f"threshold {case[0]!r} min {case[1]} max {case[2]}"))
        grew = tracer.accum_export()["count"][pixel] != synthetic.count[pixel]
        assert bool(grew) == (case[0] < float(e)), f"the pixel on the threshold, case {case}"  # err > threshold, not >=
    assert len(sizes) >= 6, sizes
    total = 0
    for rank in range(3):
        total += check_selection(tracer, synthetic, traced_rng, cases[3], f"rank {rank} of 3, case {cases[3]}", rank=rank, nranks=3)
    assert total == int(R.active(synthetic.count, R.error(synthetic.count, synthetic.mom, R.SELECT_EXPOSURE, FLOOR), 8, *cases[3]).sum())
    tracer.accum_reset()


# ---- D. beyond one trip of the stride loops
def test_beyond_one_trip_of_the_stride_loops(tracer, synthetic):
    """accum_resolve_kernel, adapt_select_kernel and accum_error_kernel run min(ceil(n / 256), 8 * CUs) blocks of 256: above
    8 * 256 * CUs items their loops repeat, and the compaction behind the selection sees as many items."""
    _, cus = tracer.device_info()
    trip = 8 * 256 * cus
    size = next(((w, h) for w, h in ((1031, 521), (1543, 701), (2053, 1031)) if w * h > trip), None)
    if size is None:
        pytest.skip(f"{cus} compute units: no image of the list has more than {trip} pixels")
    w, h = size
    n = w * h
    upload(tracer, prt_amd.setup_cornell_box(w, h))
    big = R.tile_state(synthetic, w, h)
    # about a thousand scattered pixels with count 0, among them the first, the last and those around the loop's second trip; no other
    g = np.random.default_rng(SEED)
    chosen = np.unique(np.concatenate([[0, n - 1, trip - 1, trip, trip + 1, trip + 255, trip + 256], g.choice(n, 1000, replace=False)]))
    chosen = chosen[chosen < n]
    count = np.where(big.count == 0, U32(8), big.count).reshape(-1)
    count[chosen] = 0
    big = big._replace(count=count.reshape(h, w))
    assert int((big.count == 0).sum()) == len(chosen) and (chosen >= trip).any() and (chosen < trip).sum() > 900
    import_state(tracer, big)
    check_error_and_resolve(tracer, big, (7, 3, w - 5, h - 2))  # (the rectangle, too, has more than `trip` pixels)
    assert (w - 11) * (h - 4) > trip
    # nobody active: maxSamples below every count + 8
    tracer.accum_resolve(R.FILL_EXPOSURE)
    img, active = tracer.adaptive_pass(8, 0.0, 0, 0, FLOOR, exposure=R.SELECT_EXPOSURE)
    stats = tracer.last_stats
    assert active == 0 and stats["nPx"] == 0 and stats["kernelLaunches"] == 0 and stats["raysTraced"] == 0
    R.assert_words_equal(img, R.resolve(big.sum, big.count, R.SELECT_EXPOSURE), "a pass without active pixels vs resolve", big.label)
    # the chosen pixels and nobody else: n + 8 <= maxSamples = 8 holds where the count is 0, and n < minSamples = 8 makes those active
    tracer.accum_resolve(R.FILL_EXPOSURE)
    err = R.error(big.count, big.mom, R.SELECT_EXPOSURE, FLOOR)
    want = R.active(big.count, err, 8, 0.0, 8, 8)
    assert (np.flatnonzero(want) == chosen).all()
    img, active = tracer.adaptive_pass(8, 0.0, 8, 8, FLOOR, exposure=R.SELECT_EXPOSURE)
    assert active == len(chosen) == tracer.last_stats["nPx"]
    st, mom = tracer.accum_export(), tracer.accum_export_moments()
    assert (st["count"] == big.count + np.where(want, U32(8), U32(0))).all()
    assert (m_of(mom) == m_of(big.mom) + want.astype(U32)).all()
    assert (st["rng"][~want] == big.rng[~want]).all() and (st["rng"][want] != big.rng[want]).any()
    assert (R.bits(st["sum"])[~want] == R.bits(big.sum)[~want]).all() and (R.bits(mom)[~want] == R.bits(big.mom)[~want]).all()
    R.assert_words_equal(img[~want], R.resolve(big.sum, big.count, R.SELECT_EXPOSURE)[~want], "inactive pixels vs resolve", big.label[~want])
    # the active ones started empty: they hold render(8) of the bare box
    one = tracer.render(8, exposure=R.SELECT_EXPOSURE)
    R.assert_words_equal(img[want], one[want], "the traced pixels vs render(8)")
    tracer.accum_reset()
