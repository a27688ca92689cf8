"""Temporal reprojection on the MI355X (include/prt_hip.h "temporal reprojection").  The stage is specified exactly in float32, so
every comparison below is at tolerance 0 against the numpy restatement of the header (prt_temporal_ref): the position guide, the
image, the filtered variance and the pending record, on synthetic state (imported accumulator, moments, guides, position and history)
and on rendered camera paths.  Only the last test is about quality: after a camera move, the 8-spp preview that carries the last
view's 64 samples along is closer to a converged render than the one that starts again."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_temporal_ref as TR
import prt_testlib as T
from prt_denoise_ref import DEFAULTS
from prt_gpucases import camera_equal, check, exported, record_equal
from prt_gpukit import assert_bits_equal, bits, synthetic_state
from prt_gpukit import box_scene, dev, rows, tracer  # noqa: F401  (fixtures)
from prt_temporal_ref import PARAMETER_SETS, TDEFAULTS

pytestmark = pytest.mark.gpu
F = np.float32
VIEW_A = ((0.0, 0.965, 2.6), (0.0, 0.0, -1.0))
VIEW_B = ((0.15, 0.965, 2.5), (-0.05, 0.0, -1.0))
VIEW_C = ((0.4, 1.1, 2.3), (-0.15, -0.05, -1.0))


def view(v, width, height):
    return prt_amd.Camera().create(v[0], v[1], width, height)


# ----------------------------------------------------------------------------- 4. the position guide
def centre_rays(camera):
    w, h = camera.width, camera.height
    d = TR.centre_directions(camera.desc, w, h)
    org = np.broadcast_to(np.array(list(camera.desc.pos), F), (h, w, 3))
    return np.ascontiguousarray(org).reshape(-1, 3), d.reshape(-1, 3)


def test_position_guide_is_the_centre_ray_hit(tracer, rows):
    scene, camera, exposure = prt_amd.setup_cornell_box(64, 64, teapot_mesh=T.teapot_product_mesh())
    org, d = centre_rays(camera)
    for t in (tracer, rows):
        t.upload_scene(scene)
        t.set_camera(camera)
    got = tracer.denoise_position()
    hits = rows.trace_rays(0, org, d, 100000.0)
    want = TR.position_plane(camera.desc, 64, 64, hits["t"].reshape(64, 64))
    assert_bits_equal(got, want, "position against trace_rays")
    assert_bits_equal(rows.denoise_position(), want, "position, test library")
    oracle_t = T.OracleScene(T.scene_desc_from_product(scene, camera, exposure)).intersect_single(org, d, 100000.0)[0]["t"]
    assert_bits_equal(got, TR.position_plane(camera.desc, 64, 64, oracle_t.reshape(64, 64)), "position against the oracle")
    # the box from further away and off the axis, so that some rays pass it: misses are {0, 0, 0, -1}
    cam2 = prt_amd.Camera().create((0.0, 1.0, 6.0), (0.3, 0.0, -1.0), 64, 64)
    org2, d2 = centre_rays(cam2)
    for t in (tracer, rows):
        t.set_camera(cam2)
    got2 = tracer.denoise_position()
    t2 = rows.trace_rays(0, org2, d2, 100000.0)["t"].reshape(64, 64)
    assert_bits_equal(got2, TR.position_plane(cam2.desc, 64, 64, t2), "position after set_camera")
    miss = t2 == -1
    assert miss.any() and (~miss).any()
    assert (bits(got2[miss]) == bits(np.array([0, 0, 0, -1], F))).all()
    assert (bits(got2) != bits(got)).any()  # stale with set_camera


def test_position_guide_alpha_masked_atrium(tracer, rows):
    scene, camera, _ = prt_amd.setup_atrium_standin(96, 54, tris=20000)
    org, d = centre_rays(camera)
    for t in (tracer, rows):
        t.upload_scene(scene)
        t.set_camera(camera)
    got = tracer.denoise_position()
    t0 = rows.trace_rays(0, org, d, 100000.0)["t"].reshape(54, 96)
    assert_bits_equal(got, TR.position_plane(camera.desc, 96, 54, t0), "atrium position")
    # stale with upload_scene: the same camera in another scene, without a set_camera in between
    scene2 = prt_amd.setup_cornell_box(96, 54)[0]
    tracer.upload_scene(scene2)
    rows.upload_scene(scene2)
    got2 = tracer.denoise_position()
    t1 = rows.trace_rays(0, org, d, 100000.0)["t"].reshape(54, 96)
    assert_bits_equal(got2, TR.position_plane(camera.desc, 96, 54, t1), "the atrium's camera in the Cornell box")
    assert (t0 != t1).any()
    tracer.upload_scene(scene)
    assert_bits_equal(tracer.denoise_position(), got, "position after upload_scene")
    # a host plane round-trips, and None returns to the library's
    mine = np.random.default_rng(1).normal(size=(54, 96, 4)).astype(F)
    mine[0, 0] = np.nan
    tracer.set_denoise_position(mine)
    assert_bits_equal(tracer.denoise_position(), mine, "host position")
    tracer.set_denoise_position(None)
    assert_bits_equal(tracer.denoise_position(), got, "library position again")
    with pytest.raises(prt_amd.PrtError, match="shape"):
        tracer.set_denoise_position(mine[:10])


# ----------------------------------------------------------------------------- 5. synthetic state
def random_camera(rng, width, height, around=None, pixels=0.0):
    """A camera near the Cornell view, or `around` moved sideways by about `pixels` pixel footprints at depth 4 and turned a little."""
    if around is None:
        pos = np.array([0.0, 1.0, 3.0]) + rng.uniform(-0.2, 0.2, 3)
        d = np.array([0.0, 0.0, -1.0]) + np.append(rng.uniform(-0.1, 0.1, 2), 0.0)
    else:
        foot = 1.2 * 4.0 / height
        pos = around.pos_arg + rng.uniform(-1, 1, 3) * pixels * foot
        d = around.dir_arg + np.append(rng.uniform(-1, 1, 2) * pixels * foot / 8.0, 0.0)
    return prt_amd.Camera().create(tuple(float(v) for v in pos), tuple(float(v) for v in d), width, height)


def plane_positions(camera):
    """{X, t} of a tilted plane around z = -1 seen through the pixel centres (host data: any values do)."""
    w, h = camera.width, camera.height
    d = TR.centre_directions(camera.desc, w, h).astype(np.float64)
    n = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    pos = np.array(list(camera.desc.pos), np.float64)
    t = ((-1.0 - n @ pos) / (d @ n)).astype(F)
    return TR.position_plane(camera.desc, w, h, t)


def synthetic_temporal(width, height, seed, cur, hist_cam, normal):
    """Position plane and history with every special case in them: misses, NaN and inf positions, points behind the history camera,
    hLen 0 and above the cap, unknown history variances, taps around the distance and the normal thresholds, radiance over nine
    decades."""
    rng = np.random.default_rng(seed + 17)
    shape = (height, width)
    pos = plane_positions(cur)
    r = rng.random(shape)
    pos[r < 0.08] = (0, 0, 0, -1)                       # misses
    pos[(r >= 0.08) & (r < 0.09), :3] = np.nan          # NaN position, t >= 0
    pos[(r >= 0.09) & (r < 0.095), 3] = np.nan          # NaN t
    pos[(r >= 0.095) & (r < 0.10), 0] = np.inf
    behind = (r >= 0.10) & (r < 0.11)                   # behind the history camera: z <= 0
    hp, hd = np.array(list(hist_cam.desc.pos), F), np.array(list(hist_cam.desc.dir), F)
    pos[behind, :3] = hp - hd
    pos[behind, 3] = 1.0
    hpos = plane_positions(hist_cam)
    tq = hpos[..., 3:4]
    jitter = np.where(rng.random(shape + (1,)) < 0.5, 1e-4, 0.012) * tq * rng.normal(size=shape + (3,)) / np.sqrt(3.0)
    hX = (hpos[..., :3] + jitter).astype(F)
    hX[rng.random(shape) < 0.01] = np.nan
    hlen = rng.choice(np.array([0.0, 8.0, 64.0, 300.0, 1e4, 12.5], F), shape, p=[0.1, 0.3, 0.3, 0.1, 0.1, 0.1]).astype(F)
    hlen[rng.random(shape) < 0.01] = -8.0
    hC = (rng.random(shape + (3,)) * 10.0 ** rng.uniform(-6, 3, shape + (1,))).astype(F)
    hV = (rng.random(shape) * 10.0 ** rng.uniform(-6, 2, shape)).astype(F)
    hV[rng.random(shape) < 0.3] = -1.0
    hV[rng.random(shape) < 0.05] = 0.0
    G = np.asarray(normal, dtype=F)
    N = np.where((G == 0).all(-1, keepdims=True), F(0), (G - F(0.5)) * F(2.0)).astype(F)
    length = np.linalg.norm(N, axis=-1, keepdims=True)
    hN = np.where(length > 0, N / np.maximum(length * length, 1e-9), 0.0) + rng.normal(0, 0.05, shape + (3,))  # dot3(N_p, hN_p) ~ 1
    hN[rng.random(shape) < 0.1] *= -1.0
    hist = dict(camera=hist_cam.desc, color_var=np.concatenate([hC, hV[..., None]], -1).astype(F),
                pos_len=np.concatenate([hX, hlen[..., None]], -1).astype(F),
                normal=np.concatenate([hN, np.zeros(shape + (1,))], -1).astype(F))
    return pos.astype(F), hist


def load_synthetic(t, scene, width, height, seed, pixels=1.5):
    rng = np.random.default_rng(seed + 5)
    cur = random_camera(rng, width, height)
    hist_cam = random_camera(rng, width, height, around=cur, pixels=pixels)
    t.upload_scene(scene)
    t.set_camera(cur)
    state, mom, albedo, normal = synthetic_state(width, height, seed)
    position, hist = synthetic_temporal(width, height, seed, cur, hist_cam, normal)
    t.accum_import(state)
    t.accum_import_moments(mom)
    t.set_denoise_guides(albedo, normal)
    t.set_denoise_position(position)
    t.history_import(hist)
    return dict(total=state["sum"], count=state["count"], mom=mom, albedo=albedo, normal=normal, position=position, history=hist)


@pytest.mark.parametrize("size", [(97, 61), (33, 200), (1, 1), (5, 3)])
def test_synthetic_state_matches_the_restatement(tracer, box_scene, size):
    w, h = size
    s = load_synthetic(tracer, box_scene, w, h, seed=w * 1000 + h, pixels=1.5 if w * h > 100 else 0.0)  # tiny images: the same view
    if w * h > 100:
        for tp in PARAMETER_SETS:
            m = TR.merge(s["total"], s["count"], s["mom"], s["albedo"], s["normal"], s["position"], s["history"], **tp)
            frac = m["have"].mean()
            print(f"{w}x{h} {tp}: {frac:.3f} of the pixels take history")
            assert 0.02 < frac < 0.98, (tp, frac)  # both branches are exercised
    for iterations in (1, 2, 3, 4, 5):
        for demodulate in (False, True):
            check(tracer, s, exposure=1.0 if demodulate else 0.75, what=f"{w}x{h}", iterations=iterations, demodulate=demodulate,
                  temporal=PARAMETER_SETS[iterations % 3])
    for tp in PARAMETER_SETS:
        check(tracer, s, what=f"{w}x{h} defaults", temporal=tp)
        check(tracer, s, what=f"{w}x{h} sigmas", temporal=tp, sigma_luminance=0.5, sigma_albedo=2.0, normal_power_log2=3, demodulate=False)
    # the history is untouched by all of it
    record_equal(tracer.history_export(0), s["history"], "history after the denoises")


def test_synthetic_state_1080p(tracer, box_scene):
    s = load_synthetic(tracer, box_scene, 1920, 1080, seed=77)
    check(tracer, s, what="1920x1080")
    check(tracer, s, what="1920x1080", temporal=PARAMETER_SETS[1], iterations=3, demodulate=False, normal_power_log2=7, exposure=2.0)


# ----------------------------------------------------------------------------- 6. no history => the plain denoiser
def test_without_history_it_is_the_plain_denoiser(tracer, box_scene):
    s = load_synthetic(tracer, box_scene, 97, 61, seed=9)
    fresh = prt_amd.PathTracer()
    try:
        fresh.upload_scene(box_scene)
        fresh.set_camera(tracer._camera)
        fresh.accum_import(tracer.accum_export())
        fresh.accum_import_moments(s["mom"])
        fresh.set_denoise_guides(s["albedo"], s["normal"])
        fresh.set_denoise_position(s["position"])
        for kw in (dict(), dict(demodulate=False, iterations=2)):
            plain = fresh.denoise(**dict(DEFAULTS, **kw))
            plain_var = fresh.denoise_variance()
            assert_bits_equal(fresh.denoise_temporal(**dict(DEFAULTS, **kw)), plain, f"fresh context {kw}")
            assert_bits_equal(fresh.denoise_variance(), plain_var, f"fresh context {kw}: variance")
    finally:
        fresh.close()
    plain = tracer.denoise(**DEFAULTS)
    with_history = tracer.denoise_temporal(**DEFAULTS)
    assert (bits(with_history) != bits(plain)).any()  # the imported history does something
    assert_bits_equal(tracer.denoise(**DEFAULTS), plain, "denoise ignores history and pending")
    assert_bits_equal(tracer.denoise_temporal(max_history=0.0, **DEFAULTS), plain, "maxHistory = 0")
    tracer.history_reset()
    assert_bits_equal(tracer.denoise_temporal(**DEFAULTS), plain, "after history_reset")
    with pytest.raises(prt_amd.PrtError, match="no history"):
        tracer.history_export(0)
    # upload_scene drops both
    tracer.history_import(s["history"])
    state = tracer.accum_export()
    tracer.upload_scene(box_scene)
    tracer.accum_import(state)
    tracer.accum_import_moments(s["mom"])
    tracer.set_denoise_guides(s["albedo"], s["normal"])
    tracer.set_denoise_position(s["position"])
    assert_bits_equal(tracer.denoise_temporal(**DEFAULTS), plain, "after upload_scene")
    # a set_camera to another size drops both
    tracer.history_import(s["history"])
    tracer.denoise_temporal(**DEFAULTS)
    s2 = synthetic_state(40, 30, 5)
    tracer.set_camera(prt_amd.setup_cornell_box(40, 30)[1])
    for which in (0, 1):
        with pytest.raises(prt_amd.PrtError):
            tracer.history_export(which)
    tracer.accum_import(s2[0])
    tracer.accum_import_moments(s2[1])
    tracer.set_denoise_guides(s2[2], s2[3])
    tracer.set_denoise_position(np.ones((30, 40, 4), F))
    plain2 = tracer.denoise(**DEFAULTS)
    assert_bits_equal(tracer.denoise_temporal(**DEFAULTS), plain2, "after a set_camera to another size")


# ----------------------------------------------------------------------------- 7. / 8. rendered chains and the life cycle


def history_or_none(t):
    try:
        return t.history_export(0)
    except prt_amd.PrtError:
        return None


def step(t, camera, passes, exposure, what, target=None):
    """set_camera, `passes` adaptive passes of 8 samples on every pixel, temporal denoise; everything against the restatement fed with
    the states exported before the denoise."""
    if camera is not None:
        t.set_camera(camera)
    have = int(t.accum_counts().max()) if camera is None else 0
    for k in range(passes):
        spp = have + 8 * (k + 1)
        t.adaptive_pass(8, 0.0, spp, spp, 0.01)
    s = exported(t)
    s["history"] = history_or_none(t)
    img, pend = check(t, s, exposure=exposure, what=what)
    return s, img, pend


def test_rendered_chain(tracer):
    scene, _, exposure = prt_amd.setup_cornell_box(256, 256, teapot_mesh=T.teapot_product_mesh())
    tracer.upload_scene(scene)
    sa, _, pend_a = step(tracer, view(VIEW_A, 256, 256), 8, exposure, "view A")
    assert sa["history"] is None and (sa["count"] == 64).all()
    assert (pend_a["pos_len"][..., 3] == np.where(sa["position"][..., 3] >= 0, 64, 0)).all()
    sb, img_b, pend_b = step(tracer, view(VIEW_B, 256, 256), 1, exposure, "view B")
    record_equal(sb["history"], pend_a, "history of B = pending of A")
    assert camera_equal(sb["history"]["camera"], view(VIEW_A, 256, 256).desc)
    hit = sb["position"][..., 3] >= 0
    took = hit & (pend_b["pos_len"][..., 3] > 8)
    print(f"view B: {took.sum() / hit.sum():.3f} of the hit pixels take history")
    assert took.sum() > 0.5 * hit.sum() and np.isfinite(img_b).all()
    sc, img_c, pend_c = step(tracer, view(VIEW_C, 256, 256), 1, exposure, "view C")
    record_equal(sc["history"], pend_b, "history of C = pending of B")
    took_c = (sc["position"][..., 3] >= 0) & (pend_c["pos_len"][..., 3] > 8)
    assert took_c.any() and pend_c["pos_len"][..., 3].max() > 72  # samples of A reach C through B


def test_life_cycle(tracer):
    scene, _, exposure = prt_amd.setup_cornell_box(128, 128, teapot_mesh=T.teapot_product_mesh())
    cams = [view(v, 128, 128) for v in (VIEW_A, VIEW_B, VIEW_C)]
    tracer.upload_scene(scene)
    step(tracer, cams[0], 2, exposure, "A")
    sb, _, pend1 = step(tracer, cams[1], 1, exposure, "B, first denoise")
    hist = tracer.history_export(0)
    # a second denoise of the same view after another pass: the history is bit-identical, pending is overwritten, nothing counts twice
    sb2, _, pend2 = step(tracer, None, 1, exposure, "B, second denoise")
    record_equal(tracer.history_export(0), hist, "history after two denoises of one view")
    assert (sb2["count"] == 16).all() and (bits(pend2["pos_len"]) != bits(pend1["pos_len"])).any()
    hit = sb2["position"][..., 3] >= 0
    assert pend2["pos_len"][..., 3][hit].max() <= 16 + 16 and (pend2["pos_len"][..., 3][~hit] == 0).all()
    # an undenoised view keeps the history: C is set and left without a denoise, then B again
    tracer.set_camera(cams[2])
    record_equal(tracer.history_export(0), pend2, "set_camera promotes")
    with pytest.raises(prt_amd.PrtError, match="no pending"):
        tracer.history_export(1)
    tracer.adaptive_pass(8, 0.0, 8, 8, 0.01)
    tracer.set_camera(cams[1])
    kept = tracer.history_export(0)
    record_equal(kept, pend2, "an undenoised view keeps the history")
    assert camera_equal(kept["camera"], cams[1].desc)
    # accum_reset and accum_import touch neither
    tracer.adaptive_pass(8, 0.0, 8, 8, 0.01)
    tracer.denoise_temporal(exposure=exposure, **DEFAULTS)
    pend3 = tracer.history_export(1)
    state, mom = tracer.accum_export(), tracer.accum_export_moments()
    tracer.accum_reset()
    record_equal(tracer.history_export(0), pend2, "history after accum_reset")
    record_equal(tracer.history_export(1), pend3, "pending after accum_reset")
    tracer.accum_import(state)
    tracer.accum_import_moments(mom)
    record_equal(tracer.history_export(0), pend2, "history after accum_import")
    # export -> fresh context -> import continues the chain bit for bit
    tracer.set_camera(cams[2])
    carried = tracer.history_export(0)
    tracer.adaptive_pass(8, 0.0, 8, 8, 0.01)
    want = tracer.denoise_temporal(exposure=exposure, **DEFAULTS)
    want_pend = tracer.history_export(1)
    fresh = prt_amd.PathTracer()
    try:
        fresh.upload_scene(scene)
        fresh.set_camera(cams[2])
        fresh.history_import(carried)
        fresh.adaptive_pass(8, 0.0, 8, 8, 0.01)
        assert_bits_equal(fresh.denoise_temporal(exposure=exposure, **DEFAULTS), want, "continued in a fresh context")
        record_equal(fresh.history_export(1), want_pend, "pending in a fresh context")
        record_equal(fresh.history_export(0), carried, "imported history")
    finally:
        fresh.close()


# ----------------------------------------------------------------------------- 9. a pure read
def test_temporal_denoise_is_a_pure_read(tracer):
    scene, camera, exposure = prt_amd.setup_cornell_box(256, 256, teapot_mesh=T.teapot_product_mesh())
    tracer.upload_scene(scene)
    tracer.set_camera(view(VIEW_A, 256, 256))
    tracer.adaptive_pass(16, 0.0, 16, 16, 0.01)
    tracer.denoise_temporal(exposure=exposure)
    tracer.set_camera(camera)
    before_render = tracer.render(16)
    tracer.adaptive_pass(16, 0.0, 32, 32, 0.01)
    tracer.adaptive_pass(16, 0.0, 32, 32, 0.01)
    state, mom, resolve = tracer.accum_export(), tracer.accum_export_moments(), tracer.accum_resolve(exposure)
    plain = tracer.denoise(exposure=exposure)
    got = tracer.denoise_temporal(exposure=exposure)
    assert (bits(got) != bits(plain)).any()
    tracer.denoise_temporal(exposure=exposure, demodulate=False)
    after, mom_after = tracer.accum_export(), tracer.accum_export_moments()
    for key in ("rng", "count", "seed", "max_depth", "rr_depth"):
        assert np.array_equal(state[key], after[key]), key
    assert_bits_equal(state["sum"], after["sum"], "sums")
    assert_bits_equal(mom, mom_after, "moments")
    assert_bits_equal(resolve, tracer.accum_resolve(exposure), "resolve")
    assert_bits_equal(plain, tracer.denoise(exposure=exposure), "denoise after temporal denoises")
    assert_bits_equal(before_render, tracer.render(16), "render after a temporal denoise")
    img = tracer.accumulate(8)
    tracer.accum_reset()
    tracer.accumulate(32)
    assert_bits_equal(img, tracer.accumulate(8), "continued accumulation")


def test_explicit_target_on_a_callers_stream(tracer, box_scene, dev):
    s = load_synthetic(tracer, box_scene, 97, 61, seed=3)
    want, _, _ = TR.denoise_temporal(**s, **TDEFAULTS, **DEFAULTS)
    tracer.accum_resolve(1.0)
    fb_before = np.zeros((61, 97, 3), F)
    tracer._download(fb_before, 0, 0, 96, 60)
    nbytes = 61 * 97 * 3 * 4
    stream, target = dev.stream(), dev.alloc(nbytes)
    dev.fill_async(target, 0xff, nbytes, stream)
    tracer.denoise_temporal_async(d_rgb=target, stream=stream, **TDEFAULTS, **DEFAULTS)
    got = np.zeros((61, 97, 3), F)
    dev.download_async(got, target, stream)
    dev.synchronize(stream)
    assert_bits_equal(got, want, "caller's buffer")
    fb_after = np.zeros((61, 97, 3), F)
    tracer._download(fb_after, 0, 0, 96, 60)
    assert_bits_equal(fb_after, fb_before, "the context's framebuffer")


# ----------------------------------------------------------------------------- 10. refusals
def test_refusals(tracer, box_scene):
    EINVAL, ESTATE = "(-2)", "(-5)"
    s = load_synthetic(tracer, box_scene, 16, 16, seed=1)
    inf, nan = float("inf"), float("nan")
    bad = [(dict(position_tolerance=0.0), "positionTolerance"), (dict(position_tolerance=-0.01), "positionTolerance"),
           (dict(position_tolerance=inf), "positionTolerance"), (dict(position_tolerance=nan), "positionTolerance"),
           (dict(normal_cos=1.5), "normalCos"), (dict(normal_cos=-1.01), "normalCos"), (dict(normal_cos=nan), "normalCos"),
           (dict(normal_cos=inf), "normalCos"), (dict(max_history=-1.0), "maxHistory"), (dict(max_history=inf), "maxHistory"),
           (dict(max_history=nan), "maxHistory"), (dict(iterations=0), "iterations"), (dict(iterations=6), "iterations"),
           (dict(normal_power_log2=8), "normalPowerLog2"), (dict(sigma_luminance=0.0), "sigmaLuminance"),
           (dict(sigma_albedo=nan), "sigmaAlbedo"), (dict(guide_samples=3), "guideSamples")]
    for kw, field in bad:
        with pytest.raises(prt_amd.PrtError) as e:
            tracer.denoise_temporal(**{**DEFAULTS, **TDEFAULTS, **kw})
        assert EINVAL in str(e.value) and field in str(e.value), (kw, str(e.value))
    for kw in (dict(normal_cos=1.0), dict(normal_cos=-1.0), dict(max_history=0.0)):
        tracer.denoise_temporal(**{**DEFAULTS, **TDEFAULTS, **kw})  # the ends of the ranges are inside
    L = tracer._L
    assert L.prt_hip_accum_denoise_temporal(tracer._ctx, None, None, 1.0, None, None) == -2
    cam = prt_amd.CameraDesc()
    buf = np.zeros((16, 16, 4), F).ctypes.data_as(C.c_void_p)
    assert L.prt_hip_history_export(tracer._ctx, 2, C.byref(cam), buf, buf, buf) == -2
    # a wrong-size import
    wrong = dict(s["history"], camera=prt_amd.setup_cornell_box(32, 16)[1].desc)
    with pytest.raises(prt_amd.PrtError) as e:
        tracer.history_import(wrong)
    assert EINVAL in str(e.value) and "size" in str(e.value)
    with pytest.raises(prt_amd.PrtError, match="shape"):
        tracer.history_import(dict(s["history"], color_var=s["history"]["color_var"][:8]))
    record_equal(tracer.history_export(0), s["history"], "history after refused imports")
    tracer.accum_reset()
    with pytest.raises(prt_amd.PrtError) as e:
        tracer.denoise_temporal()
    assert ESTATE in str(e.value) and "empty" in str(e.value)
    fresh = prt_amd.PathTracer()
    try:
        with pytest.raises(prt_amd.PrtError) as e:
            fresh.denoise_temporal_async()
        assert ESTATE in str(e.value)
        assert L.prt_hip_denoise_get_position(fresh._ctx, buf) == -5
        assert L.prt_hip_history_import(fresh._ctx, C.byref(cam), buf, buf, buf) == -5
        fresh.upload_scene(box_scene)
        fresh.set_camera(prt_amd.setup_cornell_box(16, 16)[1])
        with pytest.raises(prt_amd.PrtError) as e:
            fresh.denoise_temporal()
        assert ESTATE in str(e.value) and "empty" in str(e.value)
        for which in (0, 1):
            with pytest.raises(prt_amd.PrtError) as e:
                fresh.history_export(which)
            assert ESTATE in str(e.value)
        fresh.denoise_position()  # needs scene and camera only
    finally:
        fresh.close()


# ----------------------------------------------------------------------------- 11. it helps
def figures(x, ref, mask):
    """mean squared error, mean of |x - ref|^2 / (|ref|^2 + 0.01) per pixel, median absolute error (test_gpu_denoise.error_ratios)."""
    d = x.astype(np.float64)[mask] - ref[mask]
    sq = (d * d).sum(-1)
    return sq.mean(), (sq / ((ref[mask] * ref[mask]).sum(-1) + 0.01)).mean(), np.median(np.abs(d))


@pytest.mark.parametrize("move", ["small", "larger"])
def test_it_helps_after_a_camera_move(tracer, move):
    """Cornell box with teapot, 128x128.  View A gets 64 spp in eight adaptive passes and a temporal denoise; view B one 8-spp pass.
    Against a 1024-spp render of B, on the hit pixels that took history (pending len above their count): (a) they are at least half
    of the hit pixels, (b) the temporal result's mean squared error and mean relative error are both below the plain denoiser's.
    The conditions are for this view pair ("small"); the larger move is run and printed the same way.  Printed without a condition:
    the whole-image ratios temporal / plain, and the same after a second pass in B (16 spp), where a few view-dependent pixels
    (the specular teapot's reflections) can take the mean squared error above 1 -- the bias the header names.
    CPU prototype of the design, small (larger) move: accepted 0.89 (0.83), mse ratio 0.075 (0.075), relative 0.67 (0.51) on the
    pixels with history; whole image mse 0.39 (0.16), relative 0.90 (0.80), median 0.79 (0.82); at 16 spp relative 0.74, median 0.66,
    mse 1.13.  On the MI355X, 8 spp in B: accepted 0.894 (0.829); on the pixels with history mse 0.054 (0.124), relative 0.521
    (0.407); whole image mse 0.070 (0.139), relative 0.840 (0.750), median 0.674 (0.671).  16 spp in B: on the pixels with history
    mse 0.979 (1.538), relative 0.380 (0.393); whole image mse 1.001 (1.472), relative 0.615 (0.671), median 0.579 (0.576)."""
    scene, _, exposure = prt_amd.setup_cornell_box(128, 128, teapot_mesh=T.teapot_product_mesh())
    cam_a = view(VIEW_A, 128, 128)
    cam_b = view(VIEW_B if move == "small" else VIEW_C, 128, 128)
    tracer.upload_scene(scene)
    tracer.set_camera(cam_b)
    ref = tracer.render(1024, exposure=exposure).astype(np.float64)
    tracer.history_reset()
    tracer.set_camera(cam_a)
    for k in range(8):
        tracer.adaptive_pass(8, 0.0, 8 * (k + 1), 8 * (k + 1), 0.01, exposure=exposure)
    assert (tracer.accum_counts() == 64).all()
    tracer.denoise_temporal(exposure=exposure)
    tracer.set_camera(cam_b)
    everything = np.ones((128, 128), bool)
    for spp in (8, 16):
        tracer.adaptive_pass(8, 0.0, spp, spp, 0.01, exposure=exposure)
        assert (tracer.accum_counts() == spp).all()
        temporal = tracer.denoise_temporal(exposure=exposure)
        pend = tracer.history_export(1)
        plain = tracer.denoise(exposure=exposure)
        hit = tracer.denoise_position()[..., 3] >= 0
        took = hit & (pend["pos_len"][..., 3] > spp)
        accepted = took.sum() / hit.sum()
        on_with = [a / b for a, b in zip(figures(temporal, ref, took), figures(plain, ref, took))]
        whole = [a / b for a, b in zip(figures(temporal, ref, everything), figures(plain, ref, everything))]
        print(f"{move} move, {spp} spp in B: accepted {accepted:.3f}; temporal / plain on the pixels with history: mse {on_with[0]:.3f}, "
              f"relative {on_with[1]:.3f}; whole image: mse {whole[0]:.3f}, relative {whole[1]:.3f}, median abs {whole[2]:.3f}")
        if spp == 8 and move == "small":
            assert accepted >= 0.5, accepted
            assert on_with[0] < 1.0 and on_with[1] < 1.0, on_with
