"""The display transform on the MI355X (include/prt_hip.h "display transform").  It is specified exactly, so every comparison is at
tolerance 0: against the same header run on the host (prt_amd.display_host), against its numpy restatement (prt_display_ref) and
against the pixel block prt_amd.save_ppm writes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import prt_amd
import prt_display_ref as R
from prt_display_ref import BAD_FIELDS, assert_state_equal, frame
from prt_gpukit import camera_of, fetch
from prt_gpukit import dev, tracer  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
P = prt_amd.DisplayParams.make
F = np.float32


def ppm_block(tmp_path, img, tonemap):
    path = tmp_path / "o.ppm"
    prt_amd.save_ppm(str(path), img, tonemap=tonemap)
    h, w, _ = img.shape
    return np.frombuffer(open(path, "rb").read()[-w * h * 3:], np.uint8).reshape(h, w, 3)


def test_hostile_image_in_every_combination(tracer, tmp_path):
    """61 x 37 through upload_image -> display for the 2 x 2 x 3 combinations of tone map, transfer and format: the device's bytes equal
    the host's.  The whole image is one span of 2257 = 4 x 564 + 1 pixels (vector path, then one scalar pixel); in the narrower
    rectangle every row is a span, and since 61 is no multiple of 4 the rows start at every alignment: groups of four cut by a row's
    ends take the scalar path, the others the vector path."""
    img = R.hostile_image()
    tracer.set_camera(camera_of(61, 37))
    tracer.upload_image(img)
    for tonemap, transfer, fmt in itertools.product((0, 1), (0, 1), (0, 1, 2)):
        p = P(tonemap=tonemap, transfer=transfer, format=fmt, gain=1.0)
        got = tracer.display(p)
        want, _ = prt_amd.display_host(img, p)
        assert got.shape == want.shape and np.array_equal(got, want), (tonemap, transfer, fmt, int((got != want).sum()))
        if transfer == 0 and fmt == 0:
            assert np.array_equal(got, ppm_block(tmp_path, img, bool(tonemap))), ("save_ppm", tonemap)
    # a rectangle narrower than the image: every row is a span of its own
    p = P(tonemap=1, transfer=1, format=0, gain=0.37)
    got = tracer.display(p, 2, 1, 59, 35)
    assert np.array_equal(got, prt_amd.display_host(img, p)[0][1:36, 2:60])


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rectangles_into_a_callers_buffer(tracer, dev, fmt):
    """Rectangles (3,5)-(57,30), a 1 x 1 and the full image into a caller's d_out prefilled with 0xA5: the bytes outside the rectangle
    stay, and the meter covers the rectangle only."""
    img = R.hostile_image()
    tracer.set_camera(camera_of(61, 37))
    tracer.upload_image(img)
    p = P(tonemap=1, transfer=1, format=fmt, meter=True, gain=1.25, adapt_rate=1.0)
    nbytes = 61 * 37 * p.bpp
    buf = dev.alloc(nbytes)
    for rect in ((3, 5, 57, 30), (17, 9, 17, 9), (0, 0, 60, 36)):
        dev.fill(buf, 0xA5, nbytes)
        tracer.display_reset()
        tracer.display_async(p, *rect, d_out=buf)
        st = tracer.display_state()
        got = fetch(dev, buf, nbytes, np.uint8).reshape(37, 61, p.bpp)
        want, ws = prt_amd.display_host(img, p, x0=rect[0], y0=rect[1], x1=rect[2], y1=rect[3], out=np.full((37, 61, p.bpp), 0xA5, np.uint8))
        assert np.array_equal(got, want), (rect, int((got != want).sum()))
        assert_state_equal(st, ws.as_dict(), str(rect))
        assert st["metered"] + st["ignored"] == (rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1)
        outside = np.ones((37, 61), bool)
        outside[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1] = False
        assert (got[outside] == 0xA5).all()
    # a d_out that is only 4-byte (RGB8: 1-byte) aligned: the scalar path alone, same bytes
    shifted = dev.alloc(nbytes + 4)
    q = P(tonemap=0, transfer=0, format=fmt, gain=1.0)
    tracer.display_async(q, d_out=shifted + (1 if fmt == 0 else 4))
    tracer.display_state()  # synchronises
    raw = fetch(dev, shifted, nbytes + 4, np.uint8)
    off = 1 if fmt == 0 else 4
    assert np.array_equal(raw[off:off + 61 * 37 * p.bpp].reshape(37, 61, p.bpp), prt_amd.display_host(img, q)[0])


def test_callers_image_and_stream_behind_a_queued_render(tracer, dev, tmp_path):
    """A render into the caller's image on the caller's stream, then the display of that image on the same stream, then the copy: all
    three queued before anything is waited for."""
    scene, camera, exposure = prt_amd.setup_cornell_box(48, 40)
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    want_rgb = tracer.render(8, exposure=exposure)
    p = P(tonemap=1, transfer=0, format=0, gain=1.0)
    fb_display_before = tracer.display(p)
    stream = dev.stream()
    rgb, out = dev.alloc(48 * 40 * 12), dev.alloc(48 * 40 * 3)
    dev.fill_async(rgb, 0, 48 * 40 * 12, stream)
    dev.fill_async(out, 0xA5, 48 * 40 * 3, stream)
    tracer.render_async(0, 0, 47, 39, 8, d_rgb=rgb, stream=stream, exposure=exposure)
    tracer.display_async(p, d_rgb=rgb, d_out=out, stream=stream)
    got = np.zeros((40, 48, 3), np.uint8)
    dev.download_async(got, out, stream)
    dev.synchronize(stream)
    tracer.stats()
    assert np.array_equal(got, ppm_block(tmp_path, want_rgb, True))
    assert np.array_equal(got, fb_display_before)  # (the framebuffer held the same render)


def test_auto_exposure_over_three_frames(tracer):
    """meter 1 at adaptRate 0.25 over three frames of different brightness: histogram, ignored, octaves, target and gain equal the
    restatement's; display_reset makes the next frame jump; a set_camera in between keeps the state."""
    tracer.set_camera(camera_of(40, 24))
    tracer.display_reset()
    p = P(meter=True, adapt_rate=0.25, tonemap=1, transfer=1, format=1, gain=1.0)
    ws = None
    for n, level in enumerate((1.0, 30.0, 0.02)):
        img = frame(level, 10 + n)
        img[n, 0] = np.nan
        img[n, 1] = np.inf
        img[n, 2] = 0.0
        if n == 2:
            tracer.set_camera(camera_of(40, 24))  # the state survives a new view
        tracer.upload_image(img)
        got = tracer.display(p)
        want, ws = R.display(img, p, state=ws)
        assert_state_equal(tracer.display_state(), ws, f"frame {n}")
        assert np.array_equal(got, want), n
    assert ws["gain"] != ws["target"] and ws["ignored"] == 2 and ws["hist"][255] >= 1
    tracer.display_reset()
    st = tracer.display_state()
    assert st["valid"] == 0 and st["gain"] == ws["gain"]
    tracer.display(p)
    st = tracer.display_state()
    assert st["valid"] == 1 and st["gain"] == st["target"] == ws["target"]


def test_beyond_one_trip_of_the_grid_stride_loops(tracer):
    """1920 x 1080 against display_host.  The grid rule (prt_display.hip): the histogram kernel runs min(work items, 8 x CUs) blocks of
    256 threads, one pixel per thread -- 8100 items here against 2048 blocks on 256 CUs; the transform kernel min(work items, 4 x CUs)
    blocks of 256 threads, four pixels per thread -- 2026 items against 1024 blocks: both loops take more than one trip.  A second
    display of a rectangle whose rows are spans of their own (1917 wide) does the same with 2 items per row."""
    rng = np.random.default_rng(5)
    img = (rng.random((1080, 1920, 3), dtype=F) * np.exp2(rng.uniform(-18, 17, (1080, 1920, 1)).astype(F))).astype(F)
    img[rng.random((1080, 1920)) < 0.01] = 0.0
    img[5, 5] = np.nan
    img[1079, 1919] = np.inf
    tracer.set_camera(camera_of(1920, 1080))
    tracer.upload_image(img)
    name, cus = tracer.device_info()
    assert 8100 > 8 * cus and 2026 > 4 * cus, (name, cus)
    tracer.display_reset()
    p = P(tonemap=1, transfer=1, format=1, meter=True, gain=1.0, adapt_rate=1.0)
    got = tracer.display(p)
    want, ws = prt_amd.display_host(img, p)
    assert np.array_equal(got, want), int((got != want).sum())
    assert_state_equal(tracer.display_state(), ws.as_dict())
    assert (ws.as_dict()["hist"] > 0).all()  # every bin is in use
    q = P(tonemap=0, transfer=0, format=0, meter=True, gain=1.0, adapt_rate=0.5)
    got = tracer.display(q, 1, 2, 1917, 1077)
    want, ws = prt_amd.display_host(img, q, state=ws, x0=1, y0=2, x1=1917, y1=1077)
    assert np.array_equal(got, want[2:1078, 1:1918])
    assert_state_equal(tracer.display_state(), ws.as_dict())


def test_end_to_end_cornell_box(tracer, tmp_path):
    """render -> display: the bytes are save_ppm's of the downloaded floats; the accumulator and the statistics do not notice."""
    scene, camera, exposure = prt_amd.setup_cornell_box(64, 64)
    tracer.upload_scene(scene)
    tracer.set_camera(camera)
    rgb = tracer.accumulate(8, exposure=exposure)
    before = tracer.accum_export()
    tracer.render_async(0, 0, 63, 63, 8, exposure=exposure)
    tracer.display_async(P(tonemap=1, transfer=0, format=0, gain=1.0))
    tracer.display_async(P(meter=True))
    stats = tracer.stats()
    assert stats["kernelLaunches"] == 1 and stats["nPx"] == 64 * 64
    got = tracer.display(P(tonemap=1, transfer=0, format=0, gain=1.0))
    again = tracer.stats()
    assert again["kernelLaunches"] == 0 and again["kernelMsSum"] == 0.0
    assert {k: v for k, v in again.items() if not k.startswith("kernel")} == {k: v for k, v in stats.items() if not k.startswith("kernel")}
    one_shot = np.zeros((64, 64, 3), F)
    tracer._download(one_shot, 0, 0, 63, 63)
    assert np.array_equal(one_shot.view(np.uint32), rgb.view(np.uint32))  # (8 samples either way)
    assert np.array_equal(got, ppm_block(tmp_path, one_shot, True))
    after = tracer.accum_export()
    for k in ("rng", "sum", "count"):
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    assert (before["seed"], before["max_depth"], before["rr_depth"]) == (after["seed"], after["max_depth"], after["rr_depth"])


def test_refusals_change_nothing(tracer):
    EINVAL, ESTATE = "(-2)", "(-5)"
    fresh = prt_amd.PathTracer()
    try:
        for call in (lambda: fresh._L.prt_hip_display(fresh._ctx, 0, 0, 0, 0, C.byref(P()), None, None, None),
                     lambda: fresh._L.prt_hip_upload(fresh._ctx, np.zeros(3, F).ctypes.data_as(C.c_void_p), 0, 0, 0, 0),
                     lambda: fresh._L.prt_hip_download_display(fresh._ctx, np.zeros(3, np.uint8).ctypes.data_as(C.c_void_p), 0, 0, 0, 0)):
            assert call() == -5, fresh._L.prt_hip_last_error()
        assert fresh.display_state()["valid"] == 0
        fresh.display_reset()
        fresh.set_camera(camera_of(16, 16))
        with pytest.raises(prt_amd.PrtError) as e:  # a camera, but no image yet
            fresh.display()
        assert ESTATE in str(e.value)
    finally:
        fresh.close()
    img = frame(1.0, 3, (16, 16))
    tracer.set_camera(camera_of(16, 16))
    tracer.upload_image(img)
    good = P(meter=True, adapt_rate=0.5, format=1)
    shown = tracer.display(good)
    state = tracer.display_state()
    for field, kw in BAD_FIELDS:
        with pytest.raises(prt_amd.PrtError) as e:
            tracer.display(P(**dict(dict(format=1), **kw)))
        assert EINVAL in str(e.value) and field in str(e.value), (kw, str(e.value))
    for rect in ((0, 0, 16, 15), (0, 0, 15, 16), (5, 0, 4, 15), (0, 5, 15, 4)):
        with pytest.raises(prt_amd.PrtError) as e:
            tracer.display_async(good, *rect)
        assert EINVAL in str(e.value) and "rectangle" in str(e.value)
    with pytest.raises(prt_amd.PrtError, match="shape"):
        tracer.upload_image(img[:8])
    assert_state_equal(tracer.display_state(), state)
    out = np.zeros((16, 16, 4), np.uint8)
    tracer._chk(tracer._L.prt_hip_download_display(tracer._ctx, out.ctypes.data_as(C.c_void_p), 0, 0, 15, 15), "prt_hip_download_display")
    assert np.array_equal(out, shown)
