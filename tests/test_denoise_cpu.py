"""Denoised previews without a GPU: the product exports the entry points, the header documents them and carries the filter's rules
(include/prt_hip.h "denoised previews"), Python binds them, the compiled denoise kernels use no scratch, and the numpy restatement
the GPU tests compare against (prt_denoise_ref) gives, on a hand-made case, the answer a plain double loop works out."""
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_denoise_ref as R
import prt_testlib as T
from prt_amd import _build as B

ENTRY_POINTS = ("prt_hip_denoise_set_guides", "prt_hip_denoise_get_guides", "prt_hip_accum_denoise", "prt_hip_denoise_variance")


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def test_product_exports_the_denoise_entry_points(L):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    for name in ENTRY_POINTS:
        assert re.search(rf" T {name}$", syms, re.M), name
        assert name in prt_amd.EXPORTS, name
        assert hasattr(L, name), name


def test_header_documents_the_filter():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", src), name
    block = src[src.index("denoised previews"):]
    assert "prt_denoise_params" in block
    for rule in ("lum(c) = 0.2126f*c.x + 0.7152f*c.y + 0.0722f*c.z",
                 "y = 0.125f*x; r = 1.0f / ((1.0f + y) + (0.5f*y)*y); r = r*r; r = r*r; r = r*r;",
                 "h[-2..2] = {1/16, 1/4, 3/8, 1/4, 1/16}",
                 "w = (((h[dy]*h[dx]) * wn) * wa) * wl",
                 "(M2 / (float)(m - 1)) / (float)(n >> 3) when m >= 2, else -1", '"unknown"',
                 "a tap outside the image or with !valid_q is skipped",
                 "exactly (0,0,0) per miss", "NOT renormalised", "every jitter missed",
                 "max(A_p, 0.015625f)", "V0_p = v_p < 0 ? -1 : v_p / (lum(d_p)*lum(d_p))",
                 "den = sigmaLuminance * sqrtf(g) + 1e-6f",
                 "dn = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z; wn = max(dn, 0.0f)",
                 "wa = f(((da.x*da.x + da.y*da.y) + da.z*da.z) / (sigmaAlbedo*sigmaAlbedo))",
                 "wl = V_p < 0 ? 1.0f : f(fabsf(L_p - lum(C_q)) / den)",
                 "sumV += (w*w) * (V_q >= 0 ? V_q : V_p)", "V'_p = V_p < 0 ? -1 : sumV / (sumW*sumW)",
                 "d_rgb_p = exposure * (C_final_p * d_p)", "g = g_0; g = g + g_k (k = 1..K-1); g = g * (1.0f / K)",
                 "seed boundSeed + k", "BIASED", "no FMA", "PRT_HIP_ESTATE", "PRT_HIP_EINVAL", "1, 2, 4, 8 or 16",
                 "Every comparison is the IEEE comparison and false for NaN", "max(a, b) means a > b ? a : b",
                 "a NaN albedo channel demodulates by 0.015625f", "a NaN dn gives wn = 0", "a NaN V_p is unknown",
                 "What follows for non-finite state", "|dx|, |dy| <= 2*(2^k - 1)", "125 x 125", "0 * NaN is NaN",
                 "a NaN V is unknown (-1) for good", "A +inf V spreads", "count < 8 with m >= 2", "A NaN normal channel is harmless",
                 "there is\n * no upper clamp", "length 40", "shows a NaN as 0"):
        assert rule in block, rule


def test_python_host_binds_the_denoise_api():
    assert [n for n, _ in prt_amd.DenoiseParams._fields_] == ["iterations", "normalPowerLog2", "sigmaLuminance", "sigmaAlbedo",
                                                               "demodulate", "guideSamples"]
    for m in ("denoise", "denoise_async", "denoise_guides", "set_denoise_guides", "denoise_variance"):
        assert callable(getattr(prt_amd.PathTracer, m)), m
    assert "prt_denoise.hip" in B.SOURCES


def denoise_kernel_resources():
    """{kernel name: {VGPRs, ScratchSize, ...}} of prt_denoise.hip, from the compiler's resource-usage remarks (product flags)."""
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC", "-pthread", "-ldl")]
    cmd = [B.hipcc()] + flags + ["--cuda-device-only", "-c", os.path.join(B.CSRC, "prt_denoise.hip"), "-o", os.devnull,
                                 "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, check=True).stderr
    out, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        elif cur is not None:
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
            if m:
                cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_denoise_kernels_use_no_scratch():
    res = denoise_kernel_resources()
    names = " ".join(res)
    for k in ("dn_guide_sum_kernel", "dn_prepare_kernel", "dn_iter_kernelILb0E", "dn_iter_kernelILb1E"):
        assert k in names, (k, names)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 64 and r["Occupancy"] == 8, (name, r)  # what DESIGN.md section 7 states


def test_restatement_on_a_hand_made_case():
    """8x8, one iteration, every variance unknown (wl = 1), one albedo (wa = f(0) = 1), left half with normal +x and right half with
    normal +y: wn is exactly 0 across the border and exactly 1 within a half, so every pixel is the h-weighted mean of the taps of its
    own half that lie inside the image -- worked out here by a plain double loop in double precision."""
    n = 8
    rng = np.random.default_rng(7)
    count = np.full((n, n), 16, np.uint32)
    c = rng.integers(1, 64, (n, n, 3)).astype(np.float32)  # small integers: the sums below are exact in either precision
    total = c * np.float32(16)
    mom = np.zeros((n, n, 4), np.float32)
    albedo = np.full((n, n, 3), 0.5, np.float32)
    normal = np.zeros((n, n, 3), np.float32)
    normal[:, :4] = (1.0, 0.5, 0.5)  # 0.5*n + 0.5 of n = +x
    normal[:, 4:] = (0.5, 1.0, 0.5)  # n = +y
    for power in (0, 7):
        img, var = R.denoise(total, count, mom, albedo, normal, iterations=1, normal_power_log2=power, demodulate=False)
        assert (var == -1).all()
        h = {-2: 1 / 16, -1: 1 / 4, 0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
        want = np.zeros((n, n, 3))
        for y in range(n):
            for x in range(n):
                sw, sc = 0.0, np.zeros(3)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + dx, y + dy
                        if 0 <= qx < n and 0 <= qy < n and (qx < 4) == (x < 4):
                            sw += h[dy] * h[dx]
                            sc += h[dy] * h[dx] * c[qy, qx].astype(np.float64)
                want[y, x] = sc / sw
        # weights are multiples of 1/256 and values integers below 64: every partial sum is exact in float32, so only the final
        # division rounds
        assert (img == want.astype(np.float32)).all(), np.abs(img - want).max()


def test_restatement_rules():
    """The special cases of the header on tiny inputs: an invalid pixel gives +0 and V -1 and is never a tap; a pixel whose guide
    normals all missed keeps its own value; demodulation divides by max(A, 1/64) and multiplies back."""
    count = np.array([[8, 0, 8]], np.uint32)
    total = np.array([[[8, 16, 24], [1e9, 1e9, 1e9], [80, 80, 80]]], np.float32)
    mom = np.zeros((1, 3, 4), np.float32)
    albedo = np.zeros((1, 3, 3), np.float32)
    normal = np.full((1, 3, 3), 0.5, np.float32)
    normal[0, :, 2] = 1.0  # +z everywhere
    img, var = R.denoise(total, count, mom, albedo, normal, iterations=1, normal_power_log2=0, demodulate=True)
    assert (var == -1).all() and (img[0, 1] == 0).all() and not np.signbit(img[0, 1]).any()
    # pixels 0 and 2 see each other at dx = +-2 (weight 3/8 * 1/16 against 9/64 for the centre), never pixel 1
    w0, w2 = 9 / 64, 3 / 128
    assert np.allclose(img[0, 0], (w0 * np.array([1, 2, 3]) + w2 * 10) / (w0 + w2), rtol=1e-6)
    normal[0, 0] = 0  # every jitter missed
    img, _ = R.denoise(total, count, mom, albedo, normal, iterations=3, normal_power_log2=2, demodulate=False)
    assert (img[0, 0] == np.array([1, 2, 3], np.float32)).all() and (img[0, 2] == 10).all()
