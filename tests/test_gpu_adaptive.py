"""Adaptive sampling on the MI355X (include/prt_hip.h "adaptive sampling").  An adaptive pass gives the pixels it selects exactly the
samples an accumulate pass would give them, so every pixel holds, bit for bit, the one-shot render of its own sample count: the images,
accumulator records and statistics below are compared with tolerance 0.  The selection is restated in numpy float32 (the build has no
FMA, tests/prt_adaptive_ref.py) and must pick exactly the pixels the library picks; the moment records are compared word for word with
the header's fold of exact packet sums, each exported by a pass that starts from a zeroed sum (test_gpu_adaptive_exact.py goes further:
partly active passes, ranks, synthetic states)."""
import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_adaptive_ref import active_set, luminance, np_error
from prt_gpukit import assert_bits_equal, upload
from prt_gpukit import c1_scene, tracer  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
EXPOSURE, FLOOR = 1.0, 0.01


def run_passes(t, passes, adaptive, **kw):
    """passes of (samples, threshold, min, max) as adaptive passes or as plain accumulate passes; returns per pass (image, active,
    stats) and the final export."""
    out = []
    for s, thr, lo, hi in passes:
        if adaptive:
            img, active = t.adaptive_pass(s, thr, lo, hi, FLOOR, exposure=EXPOSURE, **kw)
        else:
            img, active = t.accumulate(s, exposure=EXPOSURE, **kw), None
        out.append((img, active, dict(t.last_stats)))
    return out, t.accum_export()


def check_all_active_equals_accumulate(t, size, **kw):
    passes = [(8, 0.0, 32, 32), (8, 0.0, 32, 32), (16, 0.0, 32, 32)]
    t.accum_reset()
    ad, ad_state = run_passes(t, passes, True, **kw)
    t.accum_reset()
    acc, acc_state = run_passes(t, passes, False, **kw)
    for k, ((ia, active, sa), (ib, _, sb)) in enumerate(zip(ad, acc)):
        assert active == size, (k, active)
        assert_bits_equal(ia, ib, f"pass {k}: adaptive (all active) vs accumulate")
        assert (sa["raysTraced"], sa["occludedTraced"], sa["nPx"]) == (sb["raysTraced"], sb["occludedTraced"], sb["nPx"]), k
        assert sa["nPx"] == active
    assert (ad_state["rng"] == acc_state["rng"]).all() and (ad_state["count"] == acc_state["count"]).all()
    assert_bits_equal(ad_state["sum"], acc_state["sum"], "accumulator sums")
    assert (ad_state["count"] == 32).all()


def test_all_active_equals_accumulate(tracer, c1_scene):
    scene, camera, _ = c1_scene
    upload(tracer, scene, camera)
    check_all_active_equals_accumulate(tracer, 512 * 512)


def test_all_active_equals_accumulate_env_light(tracer):
    scene, camera, _ = prt_amd.setup_cornell_box(128, 128, teapot_mesh=T.teapot_product_mesh())
    scene.set_infinite_area_light(T.sky_env(48, 24, black_rows=True))
    upload(tracer, scene, camera)
    check_all_active_equals_accumulate(tracer, 128 * 128, max_depth=8)


@pytest.fixture(scope="module")
def c1_adaptive_run(tracer, c1_scene):
    """From empty: one 16-spp pass (min 16, max 128, threshold 0) gives every pixel two packets; the threshold is then the median of the
    nonzero errors, and 16-spp passes run until none is active.  Records the state before and the result after every pass."""
    scene, camera, exposure = c1_scene
    upload(tracer, scene, camera)
    lo, hi = 16, 128
    records, thr = [], 0.0
    for k in range(20):
        before, mom = tracer.accum_export(), tracer.accum_export_moments()
        err = tracer.accum_error(EXPOSURE, FLOOR)
        img, active = tracer.adaptive_pass(16, thr, lo, hi, FLOOR, exposure=EXPOSURE)
        records.append(dict(before=before, mom=mom, err=err, thr=thr, img=img, active=active, stats=dict(tracer.last_stats),
                            resolve=tracer.accum_resolve(EXPOSURE)))
        if k == 0:  # (a pixel whose two packets agree exactly has err 0 and stops at any threshold: the median of the others)
            e = tracer.accum_error(EXPOSURE, FLOOR)
            thr = float(np.median(e[e > 0]))
        elif active == 0:
            break
    assert records[-1]["active"] == 0, "the run did not converge"
    final = tracer.accum_export()
    return dict(scene=scene, camera=camera, exposure=exposure, records=records, final=final, img=records[-1]["img"], lo=lo, hi=hi)


def test_each_pixel_is_the_one_shot_render_of_its_own_count(tracer, c1_adaptive_run):
    R = c1_adaptive_run
    counts, img = R["final"]["count"], R["img"]
    assert np.isfinite(R["records"][1]["err"]).all() and (R["records"][1]["mom"][..., 2].view(np.uint32) == 2).all()
    classes = sorted(int(k) for k in np.unique(counts))
    assert len(classes) >= 3, (classes, R["records"][1]["thr"], float((R["records"][1]["err"] == 0).mean()))
    assert classes[0] < R["hi"], classes
    upload(tracer, R["scene"], R["camera"])
    for k in classes:
        sel = counts == k
        one = tracer.render(k, exposure=EXPOSURE)
        assert_bits_equal(img[sel], one[sel], f"pixels with {k} samples vs render({k})")
        tracer.accum_reset()
        tracer.accumulate(k, exposure=EXPOSURE)
        ref = tracer.accum_export()
        assert (ref["rng"][sel] == R["final"]["rng"][sel]).all(), k
        assert_bits_equal(R["final"]["sum"][sel], ref["sum"][sel], f"accumulator sums of the pixels with {k} samples")
    # one class straight against the oracle: a 16x16 rectangle, its most frequent count
    x0, y0 = 240, 300
    rect = (x0, y0, x0 + 15, y0 + 15)
    sub = counts[y0:y0 + 16, x0:x0 + 16]
    vals, freq = np.unique(sub, return_counts=True)
    k = int(vals[np.argmax(freq)])
    ref, _ = T.OracleScene(T.scene_desc_from_product(R["scene"], R["camera"], EXPOSURE)).render_rect(rect, k, threads=16, stats=False)
    sel = sub == k
    assert_bits_equal(img[y0:y0 + 16, x0:x0 + 16][sel], ref[sel], f"{int(sel.sum())} pixels with {k} samples vs the oracle")


def test_selection_is_the_documented_rule(c1_adaptive_run):
    R = c1_adaptive_run
    recs = R["records"]
    for k, r in enumerate(recs):
        count = r["before"]["count"]
        err = np_error(count, r["mom"])
        assert_bits_equal(err, r["err"], f"pass {k}: accum_error vs numpy")
        want = active_set(count, err, 16, r["thr"], R["lo"], R["hi"])
        after = recs[k + 1]["before"]["count"] if k + 1 < len(recs) else R["final"]["count"]
        grew = after != count
        assert (grew == want).all(), f"pass {k}: {int((grew != want).sum())} pixels selected against the rule"
        assert (after[grew] - count[grew] == 16).all()
        assert r["active"] == int(want.sum()) == r["stats"]["nPx"], (k, r["active"], int(want.sum()), r["stats"]["nPx"])
        assert_bits_equal(r["img"], r["resolve"], f"pass {k}: image vs accum_resolve")
    assert recs[-1]["stats"]["raysTraced"] == 0 and recs[-1]["stats"]["kernelLaunches"] == 0


def test_moments(tracer, c1_scene):
    scene, camera, _ = c1_scene
    rect = (100, 200, 227, 327)
    x0, y0, x1, y1 = rect
    upload(tracer, scene, camera)
    tracer.adaptive_pass(8, 0.0, 64, 64, FLOOR, *rect, exposure=EXPOSURE)  # min = max: every pixel of the rectangle is active
    mom, st = tracer.accum_export_moments(), tracer.accum_export()
    inside = np.zeros((512, 512), dtype=bool)
    inside[y0:y1 + 1, x0:x1 + 1] = True
    assert_bits_equal(mom[inside][:, 0], luminance(st["sum"][inside]), "mean after one packet = L(sum)")
    assert (mom[inside][:, 1] == 0).all() and (mom[inside][:, 2].view(np.uint32) == 1).all() and (mom[inside][:, 3] == 0).all()
    assert (mom[~inside] == 0).all()
    for s in (8, 16, 8):
        tracer.adaptive_pass(s, 0.0, 64, 64, FLOOR, *rect, exposure=EXPOSURE)
    mom = tracer.accum_export_moments()[y0:y1 + 1, x0:x1 + 1]
    # the same 40 samples in packets: an accumulate run of 8-spp passes, each from a sum set to +0 (state and count kept), so that the
    # exported sum is the packet's own sum exactly
    tracer.accum_reset()
    mean = np.zeros((y1 - y0 + 1, x1 - x0 + 1), dtype=np.float32)
    m2 = np.zeros_like(mean)
    for m in range(1, 6):
        tracer.accumulate(8, *rect, exposure=EXPOSURE)
        st = tracer.accum_export()
        L = luminance(st["sum"][y0:y1 + 1, x0:x1 + 1])
        d = L - mean
        mean = mean + d / np.float32(m)
        m2 = m2 + d * (L - mean)
        st["sum"] = np.zeros_like(st["sum"])
        tracer.accum_import(st)
    assert (mom[..., 2].view(np.uint32) == 5).all()
    assert_bits_equal(mom[..., 0], mean, "mean over five packets vs the header's fold")
    assert_bits_equal(mom[..., 1], m2, "M2 over five packets vs the header's fold")
    # plain accumulate passes neither read nor change the moments
    tracer.accum_reset()
    tracer.adaptive_pass(16, 0.0, 64, 64, FLOOR, *rect, exposure=EXPOSURE)
    before = tracer.accum_export_moments()
    tracer.accumulate(8, *rect, exposure=EXPOSURE)
    tracer.accumulate(8, exposure=EXPOSURE)
    assert_bits_equal(tracer.accum_export_moments(), before, "moments after accumulate passes")


def test_ranks(tracer, c1_scene):
    scene, camera, _ = c1_scene
    upload(tracer, scene, camera)
    W = H = 512
    tracer.adaptive_pass(16, 0.0, 16, 64, FLOOR)
    e = tracer.accum_error(EXPOSURE, FLOOR)
    thr = float(np.quantile(e[e > 0], 0.4))
    seq = [(16, 0.0, 16, 64)] + [(16, thr, 16, 64)] * 3
    tracer.accum_reset()
    one = [tracer.adaptive_pass(*p, FLOOR, exposure=EXPOSURE) for p in seq]
    one_counts = tracer.accum_counts()
    tracer.accum_reset()
    union = np.zeros((H, W, 3), dtype=np.float32)
    for k, p in enumerate(seq):
        total = 0
        for r in range(3):
            prev = tracer._download_rect(0, 0, W - 1, H - 1, stats=False)
            img, active = tracer.adaptive_pass(*p, FLOOR, exposure=EXPOSURE, rank=r, nranks=3)
            total += active
            mask = prt_amd.owned_pixel_mask(W, H, r, 3)
            assert_bits_equal(img[~mask], prev[~mask], f"pass {k} rank {r}: pixels of other ranks")
            union[mask] = img[mask]
        assert total == one[k][1], (k, total, one[k][1])
    assert_bits_equal(union, one[-1][0], "ranks 0..2 of 3 vs one rank")
    assert (tracer.accum_counts() == one_counts).all()


def test_checkpoint(c1_scene):
    scene, camera, _ = c1_scene
    seq = [(16, 0.0, 16, 96)] + [(16, 0.02, 16, 96)] * 5
    t = prt_amd.PathTracer()
    try:
        upload(t, scene, camera)
        full = [t.adaptive_pass(*p, FLOOR, exposure=EXPOSURE) for p in seq]
        full_counts = t.accum_counts()
        t.accum_reset()
        for p in seq[:2]:
            t.adaptive_pass(*p, FLOOR, exposure=EXPOSURE)
        state, mom = t.accum_export(), t.accum_export_moments()
    finally:
        t.close()
    assert len({a for _, a in full}) > 1, [a for _, a in full]
    t = prt_amd.PathTracer()
    try:
        upload(t, scene, camera)
        t.accum_import(state)
        t.accum_import_moments(mom)
        rest = [t.adaptive_pass(*p, FLOOR, exposure=EXPOSURE) for p in seq[2:]]
        assert [a for _, a in rest] == [a for _, a in full[2:]]
        assert_bits_equal(rest[-1][0], full[-1][0], "resumed run vs uninterrupted run")
        assert (t.accum_counts() == full_counts).all()
    finally:
        t.close()


def test_rules(tracer):
    scene, camera, exposure = prt_amd.setup_cornell_box(64, 64)
    upload(tracer, scene, camera)
    E = prt_amd.PrtError
    for kw, msg in ((dict(threshold=float("nan")), "threshold"), (dict(threshold=-0.1), "threshold"), (dict(threshold=float("inf")), "threshold"),
                    (dict(floor=0.0), "floor"), (dict(floor=-1.0), "floor"), (dict(min_spp=64, max_spp=32), "minSamples must not exceed"),
                    (dict(min_spp=12), "multiples of 8"), (dict(max_spp=100), "multiples of 8"), (dict(max_spp=(1 << 24) + 8), "2\\^24"),
                    (dict(samples=12), "multiple of 8"), (dict(samples=2048), "multiple of 8")):
        a = dict(samples=8, threshold=0.1, min_spp=16, max_spp=64, floor=FLOOR)
        a.update(kw)
        with pytest.raises(E, match=msg):
            tracer.adaptive_pass(a["samples"], a["threshold"], a["min_spp"], a["max_spp"], a["floor"])
    with pytest.raises(E, match="floor"):
        tracer.accum_error(1.0, 0.0)
    # the estimator binding holds across adaptive and accumulate passes
    tracer.adaptive_pass(8, 0.0, 16, 64, FLOOR)
    with pytest.raises(E, match="seed, maxDepth and rrDepth"):
        tracer.adaptive_pass(8, 0.0, 16, 64, FLOOR, max_depth=8)
    with pytest.raises(E, match="seed, maxDepth and rrDepth"):
        tracer.accumulate(8, max_depth=8)
    # moments: import refusals, and every reset zeroes them
    with pytest.raises(E, match="accum_import_moments"):
        tracer.accum_import_moments(np.zeros((32, 32, 4), dtype=np.float32))
    big = tracer.accum_export_moments()
    big[..., 2] = np.uint32((1 << 21) + 1).view(np.float32)
    with pytest.raises(E, match="2\\^21"):
        tracer.accum_import_moments(big)
    state = tracer.accum_export()
    for reset in (lambda: tracer.set_camera(camera), lambda: tracer.upload_scene(scene), tracer.accum_reset, lambda: tracer.accum_import(state)):
        tracer.adaptive_pass(16, 0.0, 16, 64, FLOOR)
        assert (tracer.accum_export_moments() != 0).any()
        reset()
        assert (tracer.accum_export_moments() == 0).all()
    # 2^24: an adaptive run up to maxSamples = 2^24 is never refused; a pass beyond it selects nobody and launches nothing
    top = 1 << 24
    state = tracer.accum_export()
    state["count"][:] = top - 8
    tracer.accum_import(state)
    _, active = tracer.adaptive_pass(8, 0.0, 0, top, FLOOR)
    assert active == 64 * 64 and (tracer.accum_counts() == top).all()
    tracer.accum_resolve(1.0)  # the framebuffer now holds exposure 1
    img, active = tracer.adaptive_pass(8, 0.0, 0, top, FLOOR, exposure=2.5)
    st = tracer.last_stats
    assert active == 0 and st["kernelLaunches"] == 0 and st["raysTraced"] == 0 and st["nPx"] == 0
    assert_bits_equal(img, tracer.accum_resolve(2.5), "a pass without active pixels writes the resolved image")
    with pytest.raises(E, match="2\\^24"):
        tracer.accumulate(8)
    # render_adaptive: the viewer's loop
    seen = []
    img, counts = tracer.render_adaptive(0.05, min_spp=16, max_spp=64, step=16, callback=lambda im, a: seen.append(a))
    assert seen[-1] == 0 and seen[0] == 64 * 64 and len(seen) <= 5
    assert counts.min() >= 16 and counts.max() <= 64
    assert_bits_equal(img, tracer.accum_resolve(1.0), "render_adaptive's image")
    _, counts = tracer.render_adaptive(0.0, min_spp=16, max_spp=1024, step=16, budget_ms=0.0)
    assert (counts == 16).all()  # a pass always runs; the budget is checked after it
