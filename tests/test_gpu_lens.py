"""Lens renders on the MI355X (include/prt_hip.h "lens renders"; the CPU half is tests/test_lens_cpu.py): prt_hip_lens_rays and
prt_hip_lens_accumulate of the PRODUCT library against the numpy restatement tests/prt_lens_ref.py, and prt_hip_lens_render against
lens_accumulate(query_radiance(lens_rays)) with the merged prt_hip_query_radiance under the seeds the header gives.  Everything at
tolerance 0, compared as bytes (a NaN of the restatement asks for a NaN: prt_bake_ref.same_bytes says why), on the plain, sky and
box_rr stages of tests/prt_hostile_shade.py at depth 8 and 8 samples per ray."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
import prt_bake_ref as BR
import prt_hostile_shade as HS
import prt_lens_ref as LR
import prt_probe_ref as PR
from prt_gpukit import SCENES, SENTINEL, TAIL, fetch, ptr, sentinel, stage_tracers
from prt_gpukit import dev  # noqa: F401  (fixture: device memory and streams for one test)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
DEPTH = 8
SPP = 8
W, H = 13, 7            # 91 pixels: no multiple of 64, so the last wave of either kernel is partial
BANDS = ((0, 7), (2, 5), (6, 7))
BLOCKS_PER_CU = 8       # PRT_LENS_BLOCKS_PER_CU (prt_lens.hip): blocks of 256 lanes either kernel is launched with at the most
HOST = prt_amd.QUERY_HOST
tracers = stage_tracers(SCENES, max_depth=DEPTH)


def make_lens(kind, K=3, box=False, **kw):
    """A 13 x 7 lens of every kind, in front of the stage's patches or inside the box."""
    pos, at = ((0.0, 0.1, 0.6), (0.0, -0.3, -0.4)) if box else ((0.1, 1.2, 3.0), (0.0, 0.4, 0.0))
    up = (0.0, 1.0, 0.0)
    kw.setdefault("jitter_seed", 0x51ed270b)
    if kind == "pinhole":
        return prt_amd.lens_pinhole(pos, at, up, 0.9, W, H, K=K, **kw)
    if kind == "thin":
        return prt_amd.lens_pinhole(pos, at, up, 0.9, W, H, K=K, lens_radius=0.06, focus=3.0, **kw)
    if kind == "ortho":
        return prt_amd.lens_ortho(pos, at, up, 1.1, W, H, K=K, **kw)
    if kind == "equirect":
        return prt_amd.lens_equirect(pos, W, H, K=K, **kw)
    return prt_amd.lens_fisheye(pos, at, up, 3.0, W, H, K=K, **kw)


# ----------------------------------------------------------------------------- 1. rays
def run_rays(t, dev, lens, y0, y1, device):
    """prt_hip_lens_rays on host or device arrays: the rays of the band followed by the sentinel words."""
    out = sentinel((y1 - y0) * lens.width * lens.K * 8 + TAIL)
    if not device:
        rc = t._L.prt_hip_lens_rays(t._ctx, C.byref(lens), y0, y1, ptr(out), HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return out
    d_out = dev.upload(out)
    rc = t._L.prt_hip_lens_rays(t._ctx, C.byref(lens), y0, y1, d_out, 0, None)
    assert rc == 0, t._L.prt_hip_last_error()
    return fetch(dev, d_out, out.size)


def check_rays(got, lens, y0, y1, what):
    want = LR.rays(lens, y0, y1)
    words = len(want) * 8
    nans = BR.same_bytes(got[:words], want, what)
    assert (got[words:] == SENTINEL).all(), f"{what}: words behind the rays were written"
    return nans


@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("kind", ["pinhole", "thin", "ortho", "equirect", "fisheye"])
def test_rays_equal_the_restatement(tracers, dev, kind, K):
    t = tracers("none")  # prt_hip_lens_rays needs no scene
    for p in (0, 5):
        for flags in (0, LR.CENTRE):
            lens = make_lens(kind, K, pass_=p, flags=flags)
            for y0, y1 in BANDS:
                what = f"{kind} K={K} pass={p} flags={flags} rows [{y0}, {y1})"
                host = run_rays(t, dev, lens, y0, y1, device=False)
                assert check_rays(host, lens, y0, y1, what + ", host arrays") == 0
                on_device = run_rays(t, dev, lens, y0, y1, device=True)
                assert on_device.tobytes() == host.tobytes(), what + ": device and host pointers give different bytes"


def hostile_lenses():
    nan = np.array([PR.NAN_PAYLOAD], dtype=U).view(F)[0]
    inf = float("inf")
    out = [("zero right", make_lens("ortho").copy(right=(0, 0, 0))),
           ("zero right, pinhole", make_lens("pinhole").copy(right=(0, 0, 0))),
           ("zero up with a lens", make_lens("thin").copy(up=(0, 0, 0))),
           ("NaN in pos", make_lens("equirect").copy(pos=(0.0, nan, 1.0))),
           ("NaN in pos with a lens", make_lens("thin").copy(pos=(nan, 1.0, 1.0))),
           ("fwd 3e20 long", make_lens("fisheye").copy(fwd=(0.0, 3e20, 0.0))),
           ("fwd 1e-30 long", make_lens("pinhole").copy(fwd=(0.0, 0.0, -1e-30))),
           ("fwd 3e20 long with a lens", make_lens("thin").copy(fwd=(3e20, 0.0, 0.0))),
           ("right 3e20 long with a lens", make_lens("thin").copy(right=(3e20, 0.0, 0.0))),
           ("up 1e-30 long with a lens", make_lens("thin").copy(up=(0.0, 1e-30, 0.0)))]
    out += [(f"lensRadius {r}", make_lens("thin").copy(lensRadius=r)) for r in (0.0, -1.0, nan, inf)]
    out += [(f"focus {f}", make_lens("thin").copy(focus=f)) for f in (0.0, inf, -2.0, nan)]
    out += [(f"fov {f}", make_lens("fisheye").copy(fov=f)) for f in (0.0, float(np.pi), float(2 * np.pi), 7.0, -3.0)]
    return out


def test_hostile_records_give_what_the_arithmetic_gives(tracers, dev):
    t = tracers("none")
    nans = 0
    for what, lens in hostile_lenses():
        got = run_rays(t, dev, lens, 0, H, device=False)
        n = check_rays(got, lens, 0, H, what)
        print(f"{what}: {n} NaN words")
        nans += n
    assert nans > 0


def test_rays_beyond_one_trip_of_the_grid_stride_loop(tracers, dev):
    """256 x 256 with K = 9: 589 824 rays, more than the 8 blocks of 256 lanes per CU cover in one trip.  Rays only: nothing is traced.
    (A jittered pinhole: the restatement's sinf and cosf go through ctypes one value at a time.)"""
    t = tracers("none")
    lens = prt_amd.lens_pinhole((0.1, 1.2, 3.0), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 0.9, 256, 256, K=9, jitter_seed=3, pass_=2)
    one_trip = t.device_info()[1] * BLOCKS_PER_CU * 256
    assert 256 * 256 * 9 > one_trip + 256
    got = run_rays(t, dev, lens, 0, 256, device=True)
    check_rays(got, lens, 0, 256, "256 x 256 x 9")


# ----------------------------------------------------------------------------- 2. accumulate
# (differs from test_gpu_bake.py's: +-0, infinities of both signs and a sum that depends on its order, each in a pixel of its own)
def synthetic_radiance(n, K, seed=3):
    """(n*K, 3): ordinary values, +-0, infinities of both signs, NaN and 1e-45, each in pixels of its own; one pixel whose sum depends on
    its order."""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, K, 3)).astype(F)
    L[rng.random((n, K, 3)) < 0.05] = -0.0
    L[rng.random((n, K, 3)) < 0.05] = 0.0
    L[rng.random((n, K, 3)) < 0.05] = 1e-45
    L[3] = -0.0                      # a sum of negative zeros is -0 only if S does not start there: +0 + -0 = +0
    L[5, K // 2, 1] = np.nan
    L[6, K - 1] = np.inf
    L[7, 0, 0], L[7, K - 1, 0] = np.inf, -np.inf
    if K >= 3:
        L[8, :3, 2] = (3e38, 3e38, -3e38)  # inf in this order, 3e38 in another
    return L.reshape(n * K, 3)


def run_accumulate(t, dev, lens, y0, y1, L, prior, device):
    """prt_hip_lens_accumulate over `prior` (the whole image), followed by sentinel words."""
    img = np.concatenate([prior.view(U).reshape(-1), sentinel(TAIL)])
    if not device:
        rc = t._L.prt_hip_lens_accumulate(t._ctx, C.byref(lens), y0, y1, ptr(L), ptr(img), HOST, None)
        assert rc == 0, t._L.prt_hip_last_error()
        return img
    d_L, d_img = dev.upload(L), dev.upload(img)
    rc = t._L.prt_hip_lens_accumulate(t._ctx, C.byref(lens), y0, y1, d_L, d_img, 0, None)
    assert rc == 0, t._L.prt_hip_last_error()
    return fetch(dev, d_img, img.size)


@pytest.mark.parametrize("K", [1, 3, 64])
def test_accumulate_equals_the_restatement(tracers, dev, K):
    t = tracers("none")
    prior = np.random.default_rng(8).normal(size=(H, W, 3)).astype(F)
    prior[2, 4] = (np.inf, -0.0, np.nan)
    for flags in (0, LR.ACCUMULATE):
        lens = make_lens("pinhole", K, flags=flags)
        for y0, y1 in BANDS:
            L = synthetic_radiance((y1 - y0) * W, K)
            want = LR.accumulate(lens, L, prior, y0, y1)
            what = f"K={K} flags={flags} rows [{y0}, {y1})"
            assert want[:y0].tobytes() == prior[:y0].tobytes() and want[y1:].tobytes() == prior[y1:].tobytes()
            assert np.isnan(want[y0, 5, 1]) and want[y0, 6, 0] == np.inf and (K == 1 or np.isnan(want[y0, 7, 0]))
            if not flags:
                assert want[y0, 3].tobytes() == np.zeros(3, F).tobytes(), "S starts at +0"
            host = run_accumulate(t, dev, lens, y0, y1, L, prior, device=False)
            words = H * W * 3
            BR.same_bytes(host[:words], want, what + ", host arrays")
            assert (host[words:] == SENTINEL).all(), "words behind the image were written"
            rows = host[:words].reshape(H, W * 3)
            assert rows[:y0].tobytes() == prior[:y0].tobytes() and rows[y1:].tobytes() == prior[y1:].tobytes(), "rows outside the band"
            on_device = run_accumulate(t, dev, lens, y0, y1, L, prior, device=True)
            assert on_device.tobytes() == host.tobytes(), what + ": device and host pointers give different bytes"
    # the Python wrapper is the same call
    lens = make_lens("pinhole", K, flags=LR.ACCUMULATE)
    L = synthetic_radiance(3 * W, K)
    BR.same_bytes(t.lens_accumulate(lens, L, prior, 2, 5), LR.accumulate(lens, L, prior, 2, 5), "lens_accumulate()")
    assert t.lens_rays(lens, 2, 5).tobytes() == LR.rays(lens, 2, 5).tobytes()


# ----------------------------------------------------------------------------- 3. the fused call
def composition(t, lens, seed, image=None):
    """lens_accumulate(query_radiance(lens_rays)) band by band as LR.bands cuts the image, with the merged query under the header's
    seeds: (image, [statistics of every band's query])."""
    stats = []
    for y0, y1 in LR.bands(lens):
        r = LR.rays(lens, y0, y1)
        L = t.query_radiance(r["org"], r["dir"], SPP, seed=LR.band_seed(lens, seed, y0))
        stats.append(t.last_stats)
        image = LR.accumulate(lens, L, image, y0, y1)
    return image, stats


def run_render(t, lens, seed, flags=HOST, image=None, use_lens=True, use_params=True, use_image=True, **fields):
    """prt_hip_lens_render itself on host arrays: (code, image followed by sentinel words); fields override render parameters."""
    p = t.params(SPP, max_depth=DEPTH)
    p.seed = seed
    for k, v in fields.items():
        setattr(p, k, v)
    out = sentinel(lens.width * lens.height * 3 + TAIL) if image is None else image
    rc = t._L.prt_hip_lens_render(t._ctx, C.byref(lens) if use_lens else None, C.byref(p) if use_params else None,
                                  ptr(out) if use_image else None, flags, None)
    return rc, out


@pytest.mark.parametrize("name,kind", [("plain", "pinhole"), ("plain", "thin"), ("sky", "equirect"), ("sky", "ortho"), ("box_rr", "fisheye")])
def test_render_equals_accumulate_of_query_radiance_of_rays(tracers, name, kind):
    t = tracers(name)
    lens = make_lens(kind, 3, box=name == "box_rr")
    seed = 7000
    words = W * H * 3
    want, one = composition(t, lens, seed)
    assert len(one) == 1 and one[0]["nPx"] == W * H * 3 and not np.isnan(want).any()
    lit = int((want != 0).any(axis=2).sum())
    print(f"{name} {kind}: {lit} of {W * H} pixels are not black")
    assert lit >= 10
    # the image does not depend on how it is cut into bands; every band is a launch, and the event counters are the last band's
    for rows, launches in ((0, 1), (1, 7), (3, 3)):
        cut = lens.copy(bandRows=rows)
        _, per_band = composition(t, cut, seed)
        assert len(per_band) == launches and sum(s["raysTraced"] for s in per_band) == one[0]["raysTraced"]
        t.stats()
        rc, got = run_render(t, cut, seed)
        assert rc == 0, t._L.prt_hip_last_error()
        st = t.stats()
        BR.same_bytes(got[:words], want, f"{name} {kind} bandRows={rows}")
        assert (got[words:] == SENTINEL).all()
        assert st["kernelLaunches"] == launches and st["stackOverflow"] == 0
        assert (st["raysTraced"], st["nPx"]) == (per_band[-1]["raysTraced"], per_band[-1]["nPx"])
    # two accumulated passes are the f32 sum of the two single passes
    second, _ = composition(t, lens.copy(pass_=1), seed)
    assert second.tobytes() != want.tobytes()
    rc, first = run_render(t, lens, seed)
    rc2, both = run_render(t, lens.copy(pass_=1, flags=LR.ACCUMULATE, bandRows=3), seed, image=first)
    assert rc == 0 and rc2 == 0
    BR.same_bytes(both[:words], want + second, "two accumulated passes")
    assert (both[words:] == SENTINEL).all()
    # the Python wrapper is the same two calls and one division
    t.stats()
    mean = t.render_lens(lens, SPP, passes=2, seed=seed)
    assert mean.shape == (H, W, 3) and mean.tobytes() == ((want + second) / F(6)).tobytes()
    assert t.last_stats["kernelLaunches"] == 2


# ----------------------------------------------------------------------------- 4. nothing else moves
def test_a_lens_render_leaves_the_context_alone():
    prt_amd.build()
    scene, camera = HS.scene("plain")
    t = prt_amd.PathTracer(max_depth=DEPTH)
    try:
        t.upload_scene(scene)
        t.set_camera(camera)
        want16 = t.render(16)
        t.accumulate(8)
        t.display(prt_amd.DisplayParams.make(meter=True))
        cw, ch = camera.width, camera.height
        org, d = PR.stage_probes(100, seed=23)
        probes = t.query_radiance(org, d, 8, seed=5)  # (the staging arena holds this batch)

        def snapshot():
            acc = t.accum_export()
            return dict(rng=acc["rng"], sum=acc["sum"], count=acc["count"], bound=np.array([acc["seed"], acc["max_depth"], acc["rr_depth"]]),
                        display=np.frombuffer(repr(sorted(t.display_state().items())).encode(), np.uint8),
                        framebuffer=t._download_rect(0, 0, cw - 1, ch - 1, stats=False))
        before = snapshot()
        assert before["count"].any() and before["framebuffer"].any()
        lens = make_lens("thin", 3, band_rows=3)
        want, _ = composition(t, lens, 77)
        before = snapshot()
        rc, got = run_render(t, lens, 77)
        assert rc == 0, t._L.prt_hip_last_error()
        BR.same_bytes(got[:want.size], want, "the lens render between the passes")
        after = snapshot()
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        assert t.accumulate(8).tobytes() == want16.tobytes(), "the accumulate pass behind the lens render continues the one-shot render"
        assert t.render(16).tobytes() == want16.tobytes(), "the render digest"
        assert t.query_radiance(org, d, 8, seed=5).tobytes() == probes.tobytes()
    finally:
        t.close()


# ----------------------------------------------------------------------------- 5. refusals and state
def test_refusals_queue_nothing_and_leave_the_outputs_untouched(tracers, dev):
    t, bare = tracers("plain"), tracers("none")
    L = t._L
    lens = make_lens("pinhole", 3)
    rad = np.zeros((W * H * 3, 3), F)
    t.stats()
    # without a scene: the render is refused, the two halves work
    rc, out = run_render(bare, lens, 1)
    assert rc == -5 and b"upload a scene" in bare._L.prt_hip_last_error() and (out == SENTINEL).all()
    check_rays(run_rays(bare, dev, lens, 0, H, device=False), lens, 0, H, "without a scene")
    img = bare.lens_accumulate(lens, rad + F(1))
    assert (img == 3).all()
    # the record and the flags: all three calls
    outs = {"rays": sentinel(W * H * 3 * 8), "accumulate": sentinel(W * H * 3), "render": sentinel(W * H * 3)}
    bad = [dict(model=4), dict(model=0xffffffff), dict(width=0), dict(width=8193), dict(height=0), dict(height=8193), dict(K=0), dict(K=65),
           dict(bandRows=H + 1), dict(flags=4), dict(flags=0x80000001), dict(reserved=1)]
    cases = [dict(lens=lens.copy(**kw)) for kw in bad] + [dict(flags=HOST | 2), dict(flags=0x80000000)]
    for kw in cases:
        d, flags = kw.get("lens", lens), kw.get("flags", HOST)
        y1 = min(H, d.height) if d.height else 1
        assert L.prt_hip_lens_rays(t._ctx, C.byref(d), 0, y1, ptr(outs["rays"]), flags, None) == -2 and L.prt_hip_last_error(), kw
        assert L.prt_hip_lens_accumulate(t._ctx, C.byref(d), 0, y1, ptr(rad), ptr(outs["accumulate"]), flags, None) == -2 and L.prt_hip_last_error(), kw
        rc, _ = run_render(t, d, 1, flags=flags, image=outs["render"])
        assert rc == -2 and L.prt_hip_last_error(), (kw, rc)
    # the band of the two halves
    wide = lens.copy(width=8192, height=64, K=64)  # 2^19 rays per row: 32 rows are 2^24 rays, 33 are too many
    for d, y0, y1 in ((lens, 3, 3), (lens, 4, 3), (lens, 0, H + 1), (lens, H, H + 1), (lens, 0xffffffff, 0), (wide, 0, 33), (wide, 31, 64)):
        assert L.prt_hip_lens_rays(t._ctx, C.byref(d), y0, y1, ptr(outs["rays"]), HOST, None) == -2 and L.prt_hip_last_error(), (y0, y1)
        assert L.prt_hip_lens_accumulate(t._ctx, C.byref(d), y0, y1, ptr(rad), ptr(outs["accumulate"]), HOST, None) == -2, (y0, y1)
    # what prt_hip_query_radiance refuses of the parameters
    for kw in (dict(samples=0), dict(samples=12), dict(samples=2048), dict(nranks=2), dict(rank=1, nranks=2), dict(countTraffic=1), dict(maxDepth=256)):
        rc, _ = run_render(t, lens, 1, image=outs["render"], **kw)
        assert rc == -2 and L.prt_hip_last_error(), (kw, rc)
    # NULL pointers
    assert L.prt_hip_lens_rays(t._ctx, None, 0, H, ptr(outs["rays"]), HOST, None) == -2
    assert L.prt_hip_lens_rays(t._ctx, C.byref(lens), 0, H, None, HOST, None) == -2
    assert L.prt_hip_lens_accumulate(t._ctx, None, 0, H, ptr(rad), ptr(outs["accumulate"]), HOST, None) == -2
    assert L.prt_hip_lens_accumulate(t._ctx, C.byref(lens), 0, H, None, ptr(outs["accumulate"]), HOST, None) == -2
    assert L.prt_hip_lens_accumulate(t._ctx, C.byref(lens), 0, H, ptr(rad), None, HOST, None) == -2
    for kw in (dict(use_lens=False), dict(use_params=False), dict(use_image=False)):
        assert run_render(t, lens, 1, image=outs["render"], **kw)[0] == -2, kw
    # device pointers that are not aligned
    base = dev.upload(np.zeros(1 << 16, np.uint8))
    p = t.params(SPP, max_depth=DEPTH)
    assert L.prt_hip_lens_rays(t._ctx, C.byref(lens), 0, H, base + 8, 0, None) == -2 and b"16-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_lens_accumulate(t._ctx, C.byref(lens), 0, H, base + 2, base + 32768, 0, None) == -2 and b"4-byte aligned" in L.prt_hip_last_error()
    assert L.prt_hip_lens_accumulate(t._ctx, C.byref(lens), 0, H, base, base + 32768 + 1, 0, None) == -2
    assert L.prt_hip_lens_render(t._ctx, C.byref(lens), C.byref(p), base + 2, 0, None) == -2 and b"4-byte aligned" in L.prt_hip_last_error()
    assert not fetch(dev, base, 1 << 16, np.uint8).any(), "a refused call wrote device memory"
    assert t.stats()["kernelLaunches"] == 0
    for k, o in outs.items():
        assert (o == SENTINEL).all(), f"a refused {k} call wrote its output"
    rc, out = run_render(t, lens, 1)  # and the same arguments are accepted
    assert rc == 0 and not (out[:W * H * 3] == SENTINEL).any()


# ----------------------------------------------------------------------------- 6. a caller's stream
def test_device_memory_on_a_callers_stream_with_copies_around(tracers, dev):
    """The prior image arrives on the caller's stream, the accumulating render is queued behind it and a device copy of the answer
    behind the render: the answer must hold prior + render, so the call waited for the first copy and the second waited for it."""
    t = tracers("sky")
    lens = make_lens("equirect", 3, flags=LR.ACCUMULATE, band_rows=3)
    seed, words = 31, W * H * 3
    prior = np.concatenate([np.random.default_rng(9).normal(size=words).astype(F).view(U), sentinel(TAIL)])
    rc, want = run_render(t, lens, seed, image=prior.copy())
    assert rc == 0
    stream = dev.stream()
    d_image, d_copy = dev.upload(np.zeros_like(prior)), dev.upload(sentinel(words + TAIL))
    got = np.zeros(words + TAIL, U)
    dev.upload_async(prior, stream, d_image)
    t.stats()
    t.render_lens_async(lens, d_image, SPP, seed=seed, stream=stream)
    dev.copy_async(d_copy, d_image, (words + TAIL) * 4, stream)
    dev.download_async(got, d_copy, stream)
    dev.synchronize(stream)
    assert got.tobytes() == want.tobytes()
    st = t.stats()
    assert st["kernelLaunches"] == 3 and st["nPx"] == 1 * W * 3
