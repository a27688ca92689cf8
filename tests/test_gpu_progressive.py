"""Progressive rendering on the MI355X (include/prt_hip.h "progressive rendering"): after accumulate passes of s1, ..., sk samples
the image is, bit for bit, the one-shot render of s1 + ... + sk samples -- so every check below compares bit patterns (tolerance
0) with a one-shot render, the oracle, or the oracle's whole-frame digests."""
import hashlib
import os

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_gpukit import assert_bits_equal, bits, upload
from prt_gpukit import c1_scene, dev, tracer  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
G = T.GOLDEN


def assert_frame_equals_digests(img, rays, occluded, name, spp, depth, exposure):
    """The whole frame against the oracle's, tile by tile (the check of test_gpu_parity.assert_frame_equals_oracle_digests)."""
    z = np.load(os.path.join(G, name))
    H, W, _ = img.shape
    assert (int(z["width"]), int(z["height"]), int(z["spp"]), int(z["max_depth"]), float(z["exposure"]), int(z["seed"])) == (W, H, spp, depth, float(exposure), 12345)
    ty, tx = (H + 15) // 16, (W + 15) // 16
    assert z["sha"].shape == (ty, tx, 32)
    differing = [(c, r) for r in range(ty) for c in range(tx)
                 if hashlib.sha256(np.ascontiguousarray(img[r * 16:r * 16 + 16, c * 16:c * 16 + 16]).view(np.uint32).tobytes()).digest()
                 != z["sha"][r, c].tobytes()]
    assert not differing, f"{len(differing)} of {ty * tx} tiles differ from the oracle's frame ({name}), first {differing[:4]}"
    assert (rays, occluded) == (int(z["rays"]), int(z["occluded"]))


def test_c1_passes_equal_one_shot_renders_of_the_running_total(tracer, c1_scene):
    scene, camera, _ = c1_scene
    upload(tracer, scene, camera)
    total, rays, occl = 0, 0, 0
    for s in (8, 8, 16, 32):
        img = tracer.accumulate(s)
        total += s
        rays += tracer.last_stats["raysTraced"]
        occl += tracer.last_stats["occludedTraced"]
        assert tracer.last_stats["nPx"] == 512 * 512
        assert (tracer.accum_counts() == total).all()
        one = tracer.render(total)
        assert_bits_equal(img, one, f"accumulated {total} spp vs render({total})")
    st = tracer.last_stats
    assert (rays, occl) == (st["raysTraced"], st["occludedTraced"])


def test_c3_whole_frame_in_eight_passes_equals_the_oracles_frame(tracer):
    W, H, spp, depth = 1920, 1080, 64, 8
    scene, camera, exposure = prt_amd.setup_atrium_standin(W, H, tris=262000, seed=1)
    upload(tracer, scene, camera)
    rays = occl = 0
    for _ in range(spp // 8):
        img = tracer.accumulate(8, max_depth=depth, exposure=exposure)
        rays += tracer.last_stats["raysTraced"]
        occl += tracer.last_stats["occludedTraced"]
    assert_frame_equals_digests(img, rays, occl, "frame_digests_c3.npz", spp, depth, exposure)


def test_4096_samples_beyond_the_one_launch_cap_equal_the_oracle(tracer):
    scene, camera, exposure = prt_amd.setup_bunny_standin(64, 64, tris=3000)
    upload(tracer, scene, camera)
    rect = (24, 24, 39, 39)
    with pytest.raises(prt_amd.PrtError):
        tracer.trace_block(*rect, 4096)
    for s in (2040, 2040, 16):
        img = tracer.accumulate(s, *rect)
    counts = tracer.accum_counts()
    assert (counts[24:40, 24:40] == 4096).all() and counts.sum() == 4096 * 256
    ref, _ = T.OracleScene(T.scene_desc_from_product(scene, camera, exposure)).render_rect(rect, 4096, threads=16, stats=False)
    assert_bits_equal(img, ref, "2 x 2040 + 16 spp vs the oracle's 4096 spp")


def test_ranks_and_rectangles(tracer, c1_scene):
    scene, camera, _ = c1_scene
    upload(tracer, scene, camera)
    W, H = 512, 512
    one = tracer.render(32)
    rays_one = tracer.last_stats["raysTraced"]
    tracer.accum_reset()
    union = np.zeros_like(one)
    rays = 0
    for r in range(3):
        for s in (8, 24):
            part = tracer.accumulate(s, rank=r, nranks=3)
            rays += tracer.last_stats["raysTraced"]
        mask = prt_amd.owned_pixel_mask(W, H, r, 3)
        union[mask] = part[mask]
    assert_bits_equal(union, one, "ranks 0..2 of 3, 8 + 24 spp each, vs render(32)")
    assert rays == rays_one and (tracer.accum_counts() == 32).all()
    # two rectangles (not on tile boundaries) at different totals
    tracer.accum_reset()
    a, b = (5, 7, 130, 99), (200, 301, 511, 420)
    tracer.accumulate(8, *a)
    tracer.accumulate(16, *b)
    img_a = tracer.accumulate(16, *a)
    img_b = tracer.accumulate(24, *b)
    assert_bits_equal(img_a, tracer.trace_block(*a, 24), "rectangle a at 24 spp")
    assert_bits_equal(img_b, tracer.trace_block(*b, 40), "rectangle b at 40 spp")
    counts = tracer.accum_counts()
    assert (counts[7:100, 5:131] == 24).all() and (counts[301:421, 200:512] == 40).all()
    assert counts.sum() == 24 * 93 * 126 + 40 * 120 * 312


def test_checkpoint_export_import_resume(c1_scene):
    scene, camera, _ = c1_scene
    t = prt_amd.PathTracer()
    try:
        upload(t, scene, camera)
        t.accumulate(16)
        state = t.accum_export()
    finally:
        t.close()
    assert (state["width"], state["height"], state["seed"], state["max_depth"], state["rr_depth"]) == (512, 512, 12345, 14, 4)
    assert (state["count"] == 16).all()
    t = prt_amd.PathTracer()
    try:
        upload(t, scene, camera)
        t.accum_import(state)
        img = t.accumulate(16)
        assert_bits_equal(img, t.render(32), "16 spp, checkpoint, fresh context, 16 spp vs render(32)")
        assert_bits_equal(t.accum_resolve(2.5), t.render(32, exposure=2.5), "resolve at another exposure")
        back = t.accum_export()
        assert (back["count"] == 32).all()
    finally:
        t.close()


def test_environment_light(tracer):
    scene, camera, exposure = prt_amd.setup_cornell_box(128, 128, teapot_mesh=T.teapot_product_mesh())
    scene.set_infinite_area_light(T.sky_env(48, 24, black_rows=True))
    upload(tracer, scene, camera)
    tracer.accumulate(8, max_depth=8)
    img = tracer.accumulate(8, max_depth=8)
    assert_bits_equal(img, tracer.render(16, max_depth=8), "env-lit, 8 + 8 spp vs render(16)")


def test_rules(tracer, c1_scene):
    scene, camera, _ = c1_scene
    upload(tracer, scene, camera)
    tracer.accumulate(8)
    # a one-shot render between passes neither reads nor changes the accumulator
    tracer.render(24)
    assert_bits_equal(tracer.accumulate(8), tracer.render(16), "a render() between passes")
    # set_camera / upload_scene reset: the next pass is a one-shot of that pass alone
    tracer.set_camera(camera)
    assert (tracer.accum_counts() == 0).all()
    assert_bits_equal(tracer.accumulate(8), tracer.render(8), "after set_camera")
    tracer.upload_scene(scene)
    assert_bits_equal(tracer.accumulate(16), tracer.render(16), "after upload_scene")
    # refusals
    for bad in (12, 4, 2048):
        with pytest.raises(prt_amd.PrtError, match="multiple of 8"):
            tracer.accumulate(bad)
    seed = tracer.seed
    tracer.seed = seed + 1
    try:
        with pytest.raises(prt_amd.PrtError, match="seed, maxDepth and rrDepth"):
            tracer.accumulate(8)
    finally:
        tracer.seed = seed
    with pytest.raises(prt_amd.PrtError, match="seed, maxDepth and rrDepth"):
        tracer.accumulate(8, max_depth=8)
    state = tracer.accum_export()
    state["count"][:] = (1 << 24) - 8
    tracer.accum_import(state)
    tracer.accumulate(8)  # exactly 2^24
    with pytest.raises(prt_amd.PrtError, match="2\\^24"):
        tracer.accumulate(8)
    small = dict(state, width=256, height=256, rng=state["rng"][:256, :256], sum=state["sum"][:256, :256], count=state["count"][:256, :256])
    with pytest.raises(prt_amd.PrtError, match="accum_import"):
        tracer.accum_import(small)
    # render_progressive: the viewer's loop
    seen = []
    img, reached = tracer.render_progressive(32, step=8, callback=lambda im, n: seen.append(n))
    assert seen == [8, 16, 24, 32] and reached == 32
    assert_bits_equal(img, tracer.render(32), "render_progressive(32)")
    _, reached = tracer.render_progressive(64, step=8, budget_ms=0.0)
    assert reached == 8  # a pass always runs; the budget is checked after it


def test_passes_on_a_callers_stream(tracer, dev):
    """Accumulate, adaptive, resolve and G-buffer into an explicit target on a caller's stream: each result is there when that
    stream gets to its copy, bit for bit the one of the same step on the context's own stream and framebuffer."""
    W = H = 64
    scene, camera, _ = prt_amd.setup_cornell_box(W, H)
    upload(tracer, scene, camera)
    tracer.seed = 12345
    L, ctx = prt_amd.lib(), tracer._ctx
    nbytes = H * W * 3 * 4
    stream, target = dev.stream(), dev.alloc(nbytes)
    got = [np.zeros((H, W, 3), np.float32) for _ in range(4)]

    def copy_out(k):  # queued on the caller's stream only
        dev.download_async(got[k], target, stream)

    dev.fill_async(target, 0xff, nbytes, stream)
    tracer.accumulate_async(16, d_rgb=target, stream=stream, tile=16)
    copy_out(0)
    active = tracer.adaptive_pass_async(16, 0.0, 16, 64, d_rgb=target, stream=stream, tile=16)
    copy_out(1)
    assert L.prt_hip_accum_resolve(ctx, 0, 0, W - 1, H - 1, 1.0, target, stream) == 0, L.prt_hip_last_error()
    copy_out(2)
    assert L.prt_hip_render_gbuffer(ctx, 0, 0, W - 1, H - 1, 0, tracer.seed, 1.0, target, stream) == 0, L.prt_hip_last_error()
    copy_out(3)
    dev.synchronize(stream)
    assert active > 0  # the launch path of the adaptive pass, not the empty one
    tracer.accum_reset()
    want = [tracer.accumulate(16, tile=16)]
    img, active_own = tracer.adaptive_pass(16, 0.0, 16, 64, tile=16)
    want += [img, tracer.accum_resolve(1.0), tracer.gbuffer(0)]
    assert active_own == active
    for k, what in enumerate(("accumulate", "adaptive", "resolve", "gbuffer")):
        assert not (bits(got[k]) == 0xffffffff).any(), f"{what}: the caller's buffer still holds its fill"
        assert_bits_equal(got[k], want[k], f"{what} on a caller's stream")


def _everything_at_this_size(t):
    """Every call that (re)allocates a context buffer, at the tracer's current camera; returns what the calls returned."""
    W, H = t._camera.width, t._camera.height
    out = {}
    out["pass 1"] = t.accumulate(8)
    out["pass 2"] = t.accumulate(8)
    out["rays of pass 2"] = t.last_stats["raysTraced"]
    out["resolve"] = t.accum_resolve()
    out["adaptive"], out["active"] = t.adaptive_pass(8, 0.02, 16, 64)
    out["error 5x3"] = t.accum_error(x0=2, y0=1, x1=6, y1=3)
    out["error"] = t.accum_error()
    out["denoise"] = t.denoise()
    out["temporal"] = t.denoise_temporal()
    t.display_reset()  # the adaptation state outlives a camera change on purpose
    out["display"] = t.display(prt_amd.DisplayParams.make(meter=True))
    out["gbuffer"] = t.gbuffer(0)
    for n in (64, 1000, 8):  # the staging buffers grow, then are kept
        k = np.arange(n)
        rays = prt_amd.pixel_centre_rays(t._camera.desc, k % W, (k // W) % H)
        out[f"hits {n}"], out[f"surfaces {n}"] = t.query_nearest(rays["org"], rays["dir"], rays["tMax"], surface=True)
    out["stats"] = {k: v for k, v in t.stats().items() if not k.startswith("kernel")}  # (the times are not results)
    return out


def test_one_context_walked_through_camera_sizes_equals_fresh_contexts():
    """The context's buffers follow the camera: at each of 48x32, 32x48 (as many pixels, another shape), 64x40 (more, and no multiple
    of the 16-pixel tile) and 48x32 again, one tracer returns bit for bit what a fresh tracer returns that only ever saw that size.
    Before anything is rendered at a new size, the framebuffer of the old size is refused, not read."""
    scene, _, _ = prt_amd.setup_cornell_box(48, 32)
    camera_of = lambda w, h: prt_amd.Camera().create((0, 0.965, 2.6), (0, 0, -1.0), w, h)  # noqa: E731
    walked = prt_amd.PathTracer()
    try:
        walked.upload_scene(scene)
        for W, H in ((48, 32), (32, 48), (64, 40), (48, 32)):
            walked.set_camera(camera_of(W, H))
            if (W, H) == (64, 40):
                with pytest.raises(prt_amd.PrtError) as e:
                    walked._download_rect(0, 0, W - 1, H - 1, stats=False)
                assert "(-5)" in str(e.value) and "nothing rendered into the context framebuffer" in str(e.value)  # PRT_HIP_ESTATE
            got = _everything_at_this_size(walked)
            fresh = prt_amd.PathTracer()
            try:
                fresh.upload_scene(scene)
                fresh.set_camera(camera_of(W, H))
                want = _everything_at_this_size(fresh)
            finally:
                fresh.close()
            assert got.keys() == want.keys()
            assert want["rays of pass 2"] > 0 and "raysTraced" in want["stats"]
            for k in want:
                if isinstance(want[k], np.ndarray):
                    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (W, H, k)
                    assert got[k].tobytes() == want[k].tobytes(), f"{W}x{H}: {k} differs from a fresh context's"
                else:
                    assert got[k] == want[k], (W, H, k, got[k], want[k])
    finally:
        walked.close()
