"""Adaptive sampling without a GPU: the adaptive frame kernel keeps the budget the frame kernel's design rests on, the product exports
the new entry points, the header documents them and their rules (include/prt_hip.h "adaptive sampling") and Python binds them."""
import os
import re
import subprocess
import sys

import pytest

import prt_amd
import prt_testlib as T

ACC = "_Z16frame_kernel_accILb0ELb{env}EEv12FrameAccArgs"
ADAPT = "_Z18frame_kernel_adaptILb0ELb{env}EEv14FrameAdaptArgs"
ENTRY_POINTS = ("prt_hip_render_adaptive", "prt_hip_accum_error", "prt_hip_accum_export_moments", "prt_hip_accum_import_moments")


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


@pytest.mark.parametrize("env", [0, 1])
def test_adaptive_frame_kernel_keeps_the_frame_kernels_budget(env):
    """frame_kernel_adapt<false, ENV>: at most 64 VGPRs and 80 SGPRs (8 waves per SIMD), the accumulating kernel's LDS, call-stack
    scratch within 16 bytes of frame_kernel_acc's, and calls to the same four traversal functions."""
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    import step_loop_isa as S
    acc, ad = S.kernel_resources(kernel=ACC.format(env=env)), S.kernel_resources(kernel=ADAPT.format(env=env))
    assert ad, "frame_kernel_adapt is not in the compiled kernels"
    assert ad["VGPRs"] <= 64 and ad["TotalSGPRs"] <= 80 and ad["Occupancy"] == 8, ad
    assert ad["LDS Size"] == acc["LDS Size"], (ad, acc)
    assert ad["ScratchSize"] <= acc["ScratchSize"] + 16, (ad, acc)
    body = S.function_body(S.device_asm(), ADAPT.format(env=env))
    calls = set(re.findall(r"(_Z11trace_queueILi[0-3]ELb0EEvm)", "\n".join(body)))
    assert len(calls) == 4, calls


def test_product_exports_the_adaptive_entry_points(L):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    for name in ENTRY_POINTS:
        assert re.search(rf" T {name}$", syms, re.M), name
        assert name in prt_amd.EXPORTS, name


def test_header_documents_adaptive_sampling():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", src), name
    block = src[src.index("adaptive sampling"):]
    assert "prt_adaptive_params" in block
    for rule in ("L = (0.2126f*res.x + 0.7152f*res.y + 0.0722f*res.z) * 0.125f",
                 "m += 1; d = L - mean; mean += d / (float)m; M2 += d * (L - mean);",
                 "var = M2 / (float)(m - 1); se = sqrtf(var / (float)(n >> 3)); err = (exposure * se) / (floor + exposure * mean)",
                 "n + samples <= maxSamples and (n < minSamples or err > threshold)", "NaN error counts as converged",
                 "bit for bit", "2^24", "2^21", "multiple of 8", "seed, maxDepth and rrDepth", "neither reads nor updates the moments",
                 "prt_hip_set_camera", "prt_hip_upload_scene", "prt_hip_accum_reset", "left untouched", "*active"):
        assert rule in block, rule


def test_python_host_binds_the_adaptive_api():
    assert [n for n, _ in prt_amd.AdaptiveParams._fields_] == ["threshold", "floor", "minSamples", "maxSamples"]
    for m in ("adaptive_pass", "adaptive_pass_async", "render_adaptive", "accum_error", "accum_export_moments", "accum_import_moments"):
        assert callable(getattr(prt_amd.PathTracer, m)), m
