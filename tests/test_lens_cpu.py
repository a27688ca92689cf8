"""Lens renders without a GPU (include/prt_hip.h "lens renders"; the GPU half is tests/test_gpu_lens.py): the three entry points are
declared and exported, the numpy restatement the GPU tests hold the product to (tests/prt_lens_ref.py) equals, word for word, a
stand-alone host program compiled from the text the kernel compiles (prt_amd/csrc/prt_lens.h, tests/lens_main.cpp), and the
restatement has the properties the definition promises."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_bake_ref as BR
import prt_lens_ref as LR
import prt_testlib as T

F = np.float32
U = np.uint32
NAMES = ("prt_hip_lens_rays", "prt_hip_lens_accumulate", "prt_hip_lens_render")
HERE = os.path.dirname(os.path.abspath(__file__))


def pinhole(W=13, H=7, K=3, **kw):
    return prt_amd.lens_pinhole((0.25, 0.9, 2.5), (0.3, 0.7, 0.0), (0.0, 1.0, 0.0), 0.9, W, H, K=K, jitter_seed=77, **kw)


# ----------------------------------------------------------------------------- the interface
def test_the_entry_points_are_exported_and_wrapped():
    prt_amd.build()
    for name in NAMES:
        assert name in prt_amd.EXPORTS
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in NAMES:
            assert f" T {name}\n" in syms, (path, name)
    assert "prt_lens.hip" in prt_amd._build.SOURCES and "prt_lens.h" in prt_amd._build.KERNEL_HEADERS
    for method in ("lens_rays", "lens_accumulate", "render_lens", "render_lens_async"):
        assert callable(getattr(prt_amd.PathTracer, method))
    D = prt_amd.LensDesc
    assert C.sizeof(D) == 96
    assert (D.pass_.offset, D.bandRows.offset, D.pos.offset, D.lensRadius.offset, D.fwd.offset, D.focus.offset, D.right.offset,
            D.fov.offset, D.up.offset, D.reserved.offset) == (16, 28, 32, 44, 48, 60, 64, 76, 80, 92)
    assert (prt_amd.LENS_PINHOLE, prt_amd.LENS_ORTHO, prt_amd.LENS_EQUIRECT, prt_amd.LENS_FISHEYE) == (0, 1, 2, 3)
    assert (prt_amd.LENS_CENTRE, prt_amd.LENS_ACCUMULATE) == (LR.CENTRE, LR.ACCUMULATE) == (1, 2)


def test_header_declares_the_entry_points_and_carries_the_rules():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    section = src[src.index("---- lens renders"):]
    flat = re.sub(r"\s+", " ", section)
    for decl in ("int prt_hip_lens_rays(prt_hip_ctx* ctx, const prt_lens_desc* lens, uint32_t y0, uint32_t y1 /* rows [y0, y1) */, "
                 "prt_ray* rays /* (y1-y0)*W*K */, uint32_t flags, void* stream);",
                 "int prt_hip_lens_accumulate(prt_hip_ctx* ctx, const prt_lens_desc* lens, uint32_t y0, uint32_t y1, "
                 "const float* radiance /* 3*(y1-y0)*W*K */, float* image /* 3*W*H, the WHOLE image */, uint32_t flags, void* stream);",
                 "int prt_hip_lens_render(prt_hip_ctx* ctx, const prt_lens_desc* lens, const prt_render_params* params, "
                 "float* image /* 3*W*H */, uint32_t flags, void* stream);"):
        assert decl in flat, decl
    text = re.sub(r"[\s*]+", " ", section)
    for rule in ("s = mix(mix(pix + jitterSeed) + j) | 1", "a = 2.0f sx - 1.0f, b = 1.0f - 2.0f sy", "HALF A PIXEL",
                 "fwd' = dir - right'/W + up'/H", "d = (fwd + a right) + b up per component", "dir = F - org",
                 "org = (pos + a right) + b up, dir = fwd", "l = (ct sp, st, ct cp)", "if !(rr <= 1.0f): org = pos, dir = 0",
                 "q = rr > 0.0f ? st / rr : 0.0f", "tMax = 0, pad = 0", "params->seed + pass (W H K) + g",
                 "image[3 pix + h] = ACCUMULATE ? image[3 pix + h] + S : S", "A cube map is six PINHOLE calls",
                 "K outside 1 .. 64", "reserved != 0", "(y1 - y0) W K > 2^24", "Not built: filters other than the box; motion blur"):
        assert rule in text, rule


# ----------------------------------------------------------------------------- the host program
def parse(out):
    """[(LensDesc, y0, y1, rays (n, 8) uint32)] of the program's output."""
    entries, cur = [], None
    for line in out.splitlines():
        t = line.split()
        if t[0] == "lens":
            words = np.array([int(w, 16) for w in t[3:]], dtype=U)
            assert len(words) == 24
            cur = [prt_amd.LensDesc.from_buffer_copy(words.tobytes()), int(t[1]), int(t[2]), []]
            entries.append(cur)
        else:
            cur[3].append([int(w, 16) for w in t])
    return [(d, y0, y1, np.array(r, dtype=U)) for d, y0, y1, r in entries]


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    """tests/lens_main.cpp compiled against prt_lens.h for the CPU, under AddressSanitizer and UBSan with their runtimes linked
    statically (a program of its own: nothing of it is loaded into Python), without FMA contraction, as the kernels are built."""
    exe = str(tmp_path_factory.mktemp("lens") / "lens_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "lens_main.cpp"), "-o", exe, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return parse(r.stdout)


def test_the_restatement_equals_the_host_program_word_for_word(program_output):
    assert len(program_output) == 29
    models, nans = set(), 0
    for i, (d, y0, y1, got) in enumerate(program_output):
        want = LR.rays(d, y0, y1)
        assert got.shape == (len(want), 8), i
        nans += BR.same_bytes(got, want, f"lens {i} (model {d.model}, K {d.K}, pass {d.pass_}, flags {d.flags}, rows [{y0}, {y1}))")
        models.add((d.model, d.flags & 1))
    assert len(models) == 8, "every model with and without CENTRE"
    assert nans > 0, "the hostile records reach the invalid operations"


# ----------------------------------------------------------------------------- properties of the restatement
def test_the_middle_pixel_of_an_odd_centre_pinhole_looks_along_fwd():
    d = pinhole(13, 7, 3, flags=LR.CENTRE)
    r = LR.rays(d).reshape(7, 13, 3)
    assert r["dir"][3, 6].tobytes() == np.tile(np.array(list(d.fwd), F), (3, 1)).tobytes()
    assert r["org"][3, 6].tobytes() == np.tile(np.array(list(d.pos), F), (3, 1)).tobytes()
    assert not r["tMax"].view(U).any() and not r["pad"].any()


def test_all_draws_lie_in_the_unit_interval():
    d = pinhole(64, 64, 16, pass_=3)
    x, y, k = LR.band_index(d, 0, 64)
    u = LR.draws(d, x, y, k)
    assert u.dtype == F and (u >= 0).all() and (u < 1).all()
    assert 0.45 < u.mean() < 0.55 and len(np.unique(u[0])) > 0.99 * 65536 * 0.99
    # the two jitter draws fill the pixel
    a, b = LR.film(d, x, y, u)
    assert (a >= -1).all() and (a <= 1).all() and (b >= -1).all() and (b <= 1).all()


@pytest.mark.parametrize("model", [LR.PINHOLE, LR.ORTHO, LR.EQUIRECT, LR.FISHEYE])
def test_the_rays_of_a_band_are_a_slice_of_the_image(model):
    d = pinhole(13, 7, 3, lens_radius=0.05).copy(model=model, fov=3.0)
    whole = LR.rays(d)
    for y0, y1 in ((0, 7), (2, 5), (6, 7)):
        assert LR.rays(d, y0, y1).tobytes() == whole[y0 * 13 * 3:y1 * 13 * 3].tobytes()


def test_two_passes_of_two_rays_are_one_pass_of_four():
    four = LR.rays(pinhole(13, 7, 4, lens_radius=0.05)).reshape(7 * 13, 4)
    for p in (0, 1):
        two = LR.rays(pinhole(13, 7, 2, lens_radius=0.05, pass_=p)).reshape(7 * 13, 2)
        assert two.tobytes() == np.ascontiguousarray(four[:, 2 * p:2 * p + 2]).tobytes()
    assert four[:, 0].tobytes() != four[:, 1].tobytes()


def test_a_fisheye_pixel_outside_the_image_circle_has_no_direction():
    d = prt_amd.lens_fisheye((0, 1, 2), (0, 1, 0), (0, 1, 0), 3.0, 13, 7, K=3, jitter_seed=5)
    x, y, k = LR.band_index(d, 0, 7)
    a, b = LR.film(d, x, y, LR.draws(d, x, y, k))
    outside = ~(np.sqrt(a * a + b * b) <= F(1))
    r = LR.rays(d)
    assert 10 < outside.sum() < len(r) - 10
    assert not r["dir"][outside].view(U).any()
    assert (r["dir"][~outside] != 0).any(axis=1).all()
    assert (r["org"] == np.array(list(d.pos), F)).all()


def test_every_thin_lens_ray_of_a_centre_pixel_passes_through_its_focus_point():
    """dir = F - org, so org + dir misses F only by rounding.  Against F in float64 from the float32 d, three roundings lie between:
    the product focus*d (at most 2^-24 of the rounded product p), the sum pos + p (2^-24 of the rounded F) and the difference
    F - org (2^-24 of the rounded dir), each half an ulp of its result; org + dir itself is evaluated in float64, whose own
    rounding (2^-53 of the sum) is covered by rounding the total up by a part in 2^20."""
    d = pinhole(13, 7, 64, lens_radius=0.08, focus=2.75, flags=LR.CENTRE)
    r = LR.rays(d)
    x, y, k = LR.band_index(d, 0, 7)
    a, b = LR.film(d, x, y, LR.draws(d, x, y, k))
    pos, fwd, right, up = (np.array(list(getattr(d, n)), F) for n in ("pos", "fwd", "right", "up"))
    dd = (fwd + a[:, None] * right) + b[:, None] * up
    p32 = F(d.focus) * dd
    F32 = pos + p32
    assert F32.tobytes() == LR.focus_points(d).tobytes()
    F64 = pos.astype(np.float64) + np.float64(d.focus) * dd.astype(np.float64)
    err = np.abs(r["org"].astype(np.float64) + r["dir"].astype(np.float64) - F64)
    bound = 2.0 ** -24 * (np.abs(p32) + np.abs(F32) + np.abs(r["dir"])).astype(np.float64) * (1 + 2.0 ** -20)
    print(f"thin lens: largest miss {err.max():.3e}, smallest slack {(bound - err).min():.3e}")
    assert (err <= bound).all()
    # and the origins lie on the lens disc: all rays of a CENTRE pixel share F, and no two share an origin
    pix = r.reshape(7 * 13, 64)
    assert len(np.unique(F32.reshape(7 * 13, 64, 3)[5], axis=0)) == 1 and len(np.unique(pix["org"][5], axis=0)) == 64
    R = (right / np.linalg.norm(right)).astype(np.float64)
    Uv = (up / np.linalg.norm(up)).astype(np.float64)
    off = r["org"].astype(np.float64) - pos
    assert (np.hypot(off @ R, off @ Uv) <= 0.08 * (1 + 1e-6)).all()


def test_lens_from_camera_frames_what_the_camera_frames():
    """camera.cpp:54-56 at zero jitter in float64: v = nx*right + ny*up + dir with nx = 2*(x/W - 0.5)*0.6*(W/H) and ny = -2*(y/H -
    0.5)*0.6; the CENTRE lens gives d = (fwd' + a*right') + b*up' in float32.  Per component, with |a|, |b| <= 1 and M = |fwd'| +
    |right'| + |up'|: the three basis vectors are rounded once from float64 (2^-24 M); a carries the roundings of 1/W, of the product
    (2^-23 together on sx <= 1, doubled by the factor 2) and of the subtraction (2^-24): 1.25 * 2^-22 = 5 * 2^-24, times |right'|,
    and b the same times |up'|; the two products round (2^-24 (|right'| + |up'|)) and so do the two sums (2 * 2^-24 M).  In all at
    most 2^-24 (3 M + 6 (|right'| + |up'|)) <= 9 * 2^-24 M."""
    for W, H, pos, direction in ((13, 7, (0, 0.965, 2.6), (0, 0, -1.0)), (64, 48, (1.0, 2.0, 3.0), (-0.3, -0.4, -0.8)), (7, 13, (0, 0, 0), (1, 0.2, 0))):
        cam = prt_amd.Camera().create(pos, direction, W, H)
        d = prt_amd.lens_from_camera(cam, flags=LR.CENTRE)
        assert (d.model, d.width, d.height, d.K, d.lensRadius) == (LR.PINHOLE, W, H, 1, 0.0)
        r = LR.rays(d)
        x, y, _ = LR.band_index(d, 0, H)
        c = cam.desc
        right, up, fwd = (np.array(list(getattr(c, n)), np.float64) for n in ("right", "up", "dir"))
        nx = 2.0 * (x.astype(np.float64) / W - 0.5) * 0.6 * (W / H)
        ny = -2.0 * (y.astype(np.float64) / H - 0.5) * 0.6
        v = nx[:, None] * right + ny[:, None] * up + fwd
        M = sum(np.abs(np.array(list(getattr(d, n)), np.float64)) for n in ("fwd", "right", "up"))
        err = np.abs(r["dir"].astype(np.float64) - v)
        print(f"{W}x{H}: largest difference {err.max():.3e}, bound {(9 * 2.0 ** -24 * M).min():.3e} .. {(9 * 2.0 ** -24 * M).max():.3e}")
        assert (err <= 9 * 2.0 ** -24 * M).all()
        assert (r["org"] == np.array(list(c.pos), F)).all()
        # half a pixel is far outside the bound: the plain basis without the correction misses it
        plain = d.copy(fwd=list(c.dir))
        assert (np.abs(LR.rays(plain)["dir"].astype(np.float64) - v) > 9 * 2.0 ** -24 * M).any()


def test_the_constructors_give_the_bases_they_promise():
    p = prt_amd.lens_pinhole((0, 0, 0), (0, 0, -2), (0, 1, 0), np.pi / 2, 8, 4)
    assert np.allclose(list(p.fwd), (0, 0, -1)) and np.allclose(list(p.right), (2, 0, 0)) and np.allclose(list(p.up), (0, 1, 0))
    o = prt_amd.lens_ortho((0, 0, 0), (0, 0, -2), (0, 1, 0), 1.5, 8, 4)
    assert o.model == LR.ORTHO and np.allclose(list(o.right), (3, 0, 0)) and np.allclose(list(o.up), (0, 1.5, 0))
    e = prt_amd.lens_equirect((1, 2, 3), 16, 8, K=2)
    assert e.model == LR.EQUIRECT and np.allclose(list(e.fwd), (0, 0, -1)) and np.allclose(list(e.right), (1, 0, 0)) and e.K == 2
    # the centre column of a panorama looks along fwd, its left edge backwards, its top row up
    r = LR.rays(prt_amd.lens_equirect((0, 0, 0), 17, 9, flags=LR.CENTRE)).reshape(9, 17)
    assert np.allclose(r["dir"][4, 8], (0, 0, -1), atol=1e-6) and np.allclose(r["dir"][4, 0, [0, 1]], (np.sin(-np.pi * 16 / 17), 0), atol=1e-6)
    assert r["dir"][0, 8, 1] > 0.9
    f = prt_amd.lens_fisheye((0, 0, 0), (0, 0, -1), (0, 1, 0), np.pi, 9, 9, flags=LR.CENTRE)
    rf = LR.rays(f).reshape(9, 9)
    assert np.allclose(rf["dir"][4, 4], (0, 0, -1), atol=1e-6) and f.fov == F(np.pi)
    faces = prt_amd.lens_cube_faces((0, 1, 0), 5, flags=LR.CENTRE)
    assert len(faces) == 6
    fw = np.array([list(c.fwd) for c in faces])
    assert (fw == [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]).all()
    for c in faces:  # a 90 degree basis: the corner rays of the faces meet the cube's corners, and the middle ray is fwd
        assert abs(np.dot(list(c.fwd), list(c.right))) + abs(np.dot(list(c.fwd), list(c.up))) + abs(np.dot(list(c.right), list(c.up))) == 0
        assert np.linalg.norm(list(c.right)) == 1 and np.linalg.norm(list(c.up)) == 1 and c.width == c.height == 5
        assert LR.rays(c).reshape(5, 5)["dir"][2, 2].tolist() == list(c.fwd)


def test_accumulate_sums_in_order_and_leaves_the_other_rows():
    d = pinhole(13, 7, 3)
    rng = np.random.default_rng(1)
    L = rng.normal(size=(3 * 13 * 3, 3)).astype(F)
    L[0] = (3e38, -3e38, np.nan)
    L[1] = (3e38, 3e38, 0)
    L[2] = (-3e38, 3e38, 0)
    prior = rng.normal(size=(7, 13, 3)).astype(F)
    out = LR.accumulate(d, L, prior, 2, 5)
    assert out[:2].tobytes() == prior[:2].tobytes() and out[5:].tobytes() == prior[5:].tobytes()
    assert out[2, 0, 0] == np.inf and out[2, 0, 1] == F(3e38) and np.isnan(out[2, 0, 2])  # (3e38 + 3e38) - 3e38; (-3e38 + 3e38) + 3e38
    want = (L[3] + L[4]) + L[5]
    assert out[2, 1].tobytes() == want.tobytes()
    acc = LR.accumulate(d.copy(flags=LR.ACCUMULATE), L, prior, 2, 5)
    assert acc[2, 1].tobytes() == (prior[2, 1] + want).tobytes() and acc[0].tobytes() == prior[0].tobytes()


def test_band_seeds_and_bands():
    d = pinhole(13, 7, 3, pass_=5)
    assert LR.band_seed(d, 100, 0) == 100 + 5 * 273 and LR.band_seed(d, 100, 2) == 100 + 5 * 273 + 78
    assert LR.band_seed(d, 0xffffffff, 0) == 5 * 273 - 1
    assert LR.bands(d) == [(0, 7)] and LR.bands(d.copy(bandRows=3)) == [(0, 3), (3, 6), (6, 7)] and len(LR.bands(d.copy(bandRows=1))) == 7
    big = pinhole(3840, 2160, 8)
    assert LR.bands(big)[0] == (0, 546) and LR.bands(big)[-1][1] == 2160 and all((y1 - y0) * 3840 * 8 <= 1 << 24 for y0, y1 in LR.bands(big))
    assert LR.bands(pinhole(1920, 1080, 8)) == [(0, 1080)]


def test_the_calls_fail_loudly_without_a_context():
    """As the baker: PRT_HIP_ENODEVICE where no device exists, PRT_HIP_EINVAL for a NULL context where one does."""
    prt_amd.build()
    L = prt_amd.lib()
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    d = pinhole(2, 2, 1)
    params = prt_amd.RenderParams(samples=8, maxDepth=8, rrDepth=4, seed=1, exposure=1.0, tileSize=16, rank=0, nranks=1, countTraffic=0)
    assert L.prt_hip_lens_rays(None, C.byref(d), 0, 2, p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_lens_accumulate(None, C.byref(d), 0, 2, p, p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_lens_render(None, C.byref(d), C.byref(params), p, prt_amd.QUERY_HOST, None) == want
    assert not buf.any()
