"""The lightmap filter without a GPU (include/prt_hip.h "lightmap filter"; the GPU half is tests/test_gpu_atlas_filter.py): the entry
point is declared, exported and wrapped, the numpy restatement the GPU tests hold the product to (tests/prt_atlas_filter_ref.py)
equals, word for word, a stand-alone host program compiled from the text the kernels compile (prt_amd/csrc/prt_atlas_filter.h,
tests/atlas_filter_main.cpp) over the cases of the GPU tests, the restatement has the properties a lightmap filter must have, and
the compiled kernels use no scratch memory."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_atlas_filter_cases as AC
import prt_atlas_filter_ref as AF
import prt_bake_ref as BR
import prt_testlib as T

F = np.float32
U = np.uint32
B = prt_amd._build
HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "prt_hip_atlas_filter"
DEFAULTS = (5, 5, 4.0, 4.0)


# ----------------------------------------------------------------------------- the interface
def test_the_entry_point_is_exported_and_wrapped():
    prt_amd.build()
    assert NAME in prt_amd.EXPORTS
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert f" T {NAME}\n" in syms, path
    assert "prt_atlas_filter.hip" in B.SOURCES and "prt_atlas_filter.h" in B.KERNEL_HEADERS
    P = prt_amd.AtlasFilterParams
    assert C.sizeof(P) == 32
    assert (P.iterations.offset, P.normalPowerLog2.offset, P.sigmaLuminance.offset, P.sigmaPosition.offset, P.reserved.offset) == (0, 4, 8, 12, 16)
    p = P()
    assert (p.iterations, p.normalPowerLog2, p.sigmaLuminance, p.sigmaPosition, list(p.reserved)) == (5, 5, 4.0, 4.0, [0, 0, 0, 0])
    assert P(iterations=2, sigmaPosition=0.5).sigmaPosition == 0.5
    for method in ("atlas_filter", "atlas_filter_async"):
        assert callable(getattr(prt_amd.PathTracer, method))
    last = list(inspect.signature(prt_amd.PathTracer.lightmap).parameters.values())[-1]
    assert last.name == "filter" and last.default is None


def test_header_declares_the_call_and_carries_the_rules():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    section = src[src.index("---- lightmap filter"):]
    assert src.index("---- lightmap filter") > src.index("---- lens renders") > src.index("---- lightmap atlases")
    flat = re.sub(r"\s+", " ", section)
    for decl in ("typedef struct { uint32_t iterations; /* 1 .. 5 */ uint32_t normalPowerLog2; /* 0 .. 7 */ float sigmaLuminance; /* finite, > 0 */ "
                 "float sigmaPosition; /* finite, > 0; in texel footprints */ uint32_t reserved[4]; /* 0 */ } prt_atlas_filter_params; /* 32 bytes */",
                 "int prt_hip_atlas_filter(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, "
                 "const prt_bake_point* points, const float* values /* n*stride */, uint32_t stride /* 3*C, C 1 .. 16 */, "
                 "const prt_atlas_filter_params* params, float* out /* n*stride */, uint32_t flags, void* stream);"):
        assert decl in flat, decl
    text = re.sub(r"[\s*]+", " ", section)
    for rule in ("y = 0.125f x; r = 1.0f/((1.0f + y) + (0.5f y) y), then r = r r three times", "(x, y) = (t % W, t / W)",
                 "points[q].set != 0xffffffff", "map[t] is the smallest eligible q with texels[q] == t", "PLACED iff it is eligible and map[texels[q]] == q",
                 "out gets the bytes of values as they are", "never a tap", "d2(q,r) = (ex ex + ey ey) + ez ez with e = P_r - P_q",
                 "(dx,dy) = (-1,0), (1,0), (0,-1), (0,1) in that order", "d2 > 0 and d2 < f2_q", "If nothing was taken, f2_q = 0",
                 "dn = (Nq.x Nr.x + Nq.y Nr.y) + Nq.z Nr.z", "wn = dn > 0 ? dn : 0", "invP = 1.0f / ((sigP2 (float)(s s)) f2_q)",
                 "wp = d2 == 0 ? 1.0f : f(d2 invP)", "geo = wn wp", "per point and per launch, not per tap", "m1 = sl/sw", "d = lum_r - m1; sv = sv + g (d d)",
                 "V0 = sv/sw", "(dx==0 ? 0.5f : 0.25f) (dy==0 ? 0.5f : 0.25f)", "invDen = 1.0f / (sigmaLuminance sqrtf(a/b) + 1e-6f)",
                 "w = 0.375f 0.375f", "w = ((hy hx) geo(q,r,s)) f(fabsf(lum(C_q) - lum(C_r)) invDen)", "sumV = sumV + (w w) V_r",
                 "C'_q[j] = S_j/sumW, V'_q = sumV/(sumW sumW)", "The weights come from channel 0", "a stride that is not a multiple of 3",
                 "reserved != 0", "ranges of values and out that overlap", "needs no scene", "not a launch for prt_hip_get_stats",
                 "Not built: a per-sample variance output from the baker", "seam stitching; albedo demodulation; filtering camera or lens images; ranks"):
        assert rule in text, rule


def test_the_call_fails_loudly_without_a_context():
    """As the atlas calls: PRT_HIP_ENODEVICE where no device exists, PRT_HIP_EINVAL for a NULL context where one does."""
    prt_amd.build()
    L = prt_amd.lib()
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    params = prt_amd.AtlasFilterParams()
    assert L.prt_hip_atlas_filter(None, 4, 4, 4, p, p, p, 3, C.byref(params), p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_last_error()
    assert not buf.any()


# ----------------------------------------------------------------------------- the host program
def program_cases():
    """The cases of tests/test_gpu_atlas_filter.py: (name, (W, H, texels, points, values, iterations, npl2, sigma_l, sigma_p))."""
    cases = []
    for Cc in (1, 3, 16):
        t, pts, v, _, _ = AC.two_charts(C=Cc)
        for it in (1, 5):
            for npl2 in (0, 7):
                cases.append((f"two charts C={Cc} it={it} npl2={npl2}", (AC.W2, AC.H2, t, pts, v, it, npl2, 4.0, 4.0)))
    t, pts, v, _, _ = AC.two_charts(C=2)
    cases.append(("two charts, other sigmas", (AC.W2, AC.H2, t, pts, v, 3, 2, 0.7, 1.5)))
    for W, H in ((129, 5), (1, 1)):
        cases.append((f"{W} x {H}", (W, H) + AC.owned(W, H, C=2) + DEFAULTS))
    t, pts, v = AC.owned(129, 5)
    cases.append(("n = 1", (129, 5, t[300:301], pts[300:301], v[300:301]) + DEFAULTS))
    for kind in AC.HOSTILE + AC.REF_ONLY:
        (t, pts, v), _, _ = AC.hostile(kind)
        cases.append((kind, (AC.W2, AC.H2, t, pts, v) + DEFAULTS))
    t, pts, v, _, _ = AC.two_charts(C=3, seed=4)
    order = np.random.default_rng(8).permutation(len(t))
    cases.append(("shuffled", (AC.W2, AC.H2, t[order], pts[order], v[order]) + DEFAULTS))
    cases.append(("1024 x 513", (1024, 513) + AC.owned(1024, 513) + (1, 5, 4.0, 4.0)))
    return cases


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/atlas_filter_main.cpp compiled against prt_atlas_filter.h for the CPU, under AddressSanitizer and UBSan with their
    runtimes linked statically (a program of its own: nothing of it is loaded into Python), without FMA contraction, as the kernels
    are built; run once over all the cases."""
    tmp = tmp_path_factory.mktemp("atlas_filter")
    exe, cases_path, results = str(tmp / "atlas_filter_main"), str(tmp / "cases.bin"), str(tmp / "results.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "atlas_filter_main.cpp"), "-o", exe, "-lm"])
    cases = program_cases()
    AC.write_cases(cases_path, [c for _, c in cases])
    r = subprocess.run([exe, cases_path, results], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    return cases, AC.read_results(results, [c for _, c in cases])


def test_the_restatement_equals_the_host_program_word_for_word(program):
    cases, results = program
    assert len(cases) == 12 + 1 + 3 + len(AC.HOSTILE) + len(AC.REF_ONLY) + 2
    nans = {}
    for (name, (W, H, t, pts, v, it, npl2, sl, sp)), got in zip(cases, results):
        want = AF.filter(t, pts, v, W, H, it, npl2, sl, sp)
        assert got.shape == want.shape, name
        nans[name] = BR.same_bytes(got, want, name)
        assert want.tobytes() != np.ascontiguousarray(v, F).tobytes() or name in ("1 x 1", "n = 1"), f"{name}: nothing was filtered"
    assert nans["nan_c0"] == 1 and nans["nan_later"] == 1 and nans["huge_values"] > 0 and nans["two charts C=3 it=5 npl2=7"] == 0, nans


# ----------------------------------------------------------------------------- properties of the restatement
def rel(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b)))


def test_constant_charts_come_back_and_nothing_leaks():
    t, pts, v, clean, chart = AC.two_charts(C=1, noise=0.0, floor=1.0, wall=5.0)
    assert set(np.unique(v)) == {F(1.0), F(5.0)}
    out = AF.filter(t, pts, v, AC.W2, AC.H2, *DEFAULTS)
    err = rel(out, clean.astype(np.float64))
    print(f"constant charts: largest relative error {err:.3e}")
    assert err <= 1e-5
    # into the hole: a point there that is not eligible keeps its bytes, and one that is sees the floor only
    t2, p2, v2 = AC._append(t, pts, v, AC.HOLE_CENTRE, P=(0.8, 1.0, 0.0), values=[np.nan, 7.0, 7.0])
    out2 = AF.filter(t2, p2, v2, AC.W2, AC.H2, *DEFAULTS)
    assert out2[:-1].tobytes() == out.tobytes() and out2[-1].tobytes() == v2[-1].tobytes()
    t3, p3, v3 = AC._append(t, pts, v, AC.HOLE_CENTRE, P=(0.8, 1.0, 0.0), values=[1.0, 1.0, 1.0])
    assert rel(AF.filter(t3, p3, v3, AC.W2, AC.H2, *DEFAULTS), np.concatenate([clean, clean[:1]]).astype(np.float64)) <= 1e-5


def test_noise_falls():
    t, pts, v, clean, _ = AC.two_charts(C=1, noise=0.25)
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - clean) ** 2)))  # noqa: E731
    e = {it: rmse(AF.filter(t, pts, v, AC.W2, AC.H2, it, 5, 4.0, 4.0)) for it in (1, 3, 5)}
    print(f"RMSE against the clean signal: unfiltered {rmse(v):.3f}, after 1, 3, 5 iterations {e[1]:.3f} {e[3]:.3f} {e[5]:.3f}")
    assert e[1] < rmse(v) and e[5] < rmse(v) and e[5] <= e[1]


def test_the_scale_of_the_scene_does_not_matter():
    t, pts, v, _, _ = AC.two_charts(C=2)
    big = pts.copy()
    big["P"] = pts["P"] * F(1000.0)
    a, b = AF.filter(t, pts, v, AC.W2, AC.H2, *DEFAULTS), AF.filter(t, big, v, AC.W2, AC.H2, *DEFAULTS)
    err = rel(b, a.astype(np.float64))
    print(f"positions x 1000: largest relative difference {err:.3e}")
    assert err <= 1e-5


def test_permuting_the_points_permutes_the_output():
    t, pts, v, _, _ = AC.two_charts(C=2)
    order = np.random.default_rng(2).permutation(len(t))
    a = AF.filter(t, pts, v, AC.W2, AC.H2, *DEFAULTS)
    assert AF.filter(t[order], pts[order], v[order], AC.W2, AC.H2, *DEFAULTS).tobytes() == a[order].tobytes()


def test_hostile_points_leave_the_others_as_a_run_without_them():
    """The property the GPU tests check on the product, here on the restatement."""
    for kind in AC.HOSTILE:
        with_, without, keep = AC.hostile(kind)
        a, b = AF.filter(*with_, AC.W2, AC.H2, *DEFAULTS), AF.filter(*without, AC.W2, AC.H2, *DEFAULTS)
        assert a[keep].tobytes() == b.tobytes(), kind
        assert np.isfinite(a[keep]).all(), kind


# ----------------------------------------------------------------------------- resources
def test_the_kernels_use_no_scratch():
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC", "-pthread", "-ldl")]
    cmd = [B.hipcc()] + flags + ["--cuda-device-only", "-c", os.path.join(B.CSRC, "prt_atlas_filter.hip"), "-o", os.devnull,
                                 "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, check=True).stderr
    res, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
        elif cur is not None:
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
            if m:
                cur[m.group(1).strip()] = int(m.group(2))
    names = " ".join(res)
    for k in ("af_index_kernel", "af_prepare_kernel", "af_iter_kernelILb0ELb0E", "af_iter_kernelILb0ELb1E", "af_iter_kernelILb1ELb0E", "af_iter_kernelILb1ELb1E"):
        assert k in names, (k, names)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["LDS Size"] == 0, (name, r)
        assert r["Occupancy"] >= 4, (name, r)  # what DESIGN.md section 7 states
