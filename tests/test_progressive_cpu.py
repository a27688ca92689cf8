"""Progressive rendering without a GPU: the accumulating frame kernel keeps the occupancy the frame kernel's design rests on, the
product exports the new entry points and the header documents them (include/prt_hip.h "progressive rendering")."""
import os
import re
import subprocess
import sys

import pytest

import prt_amd
import prt_testlib as T

ONE_SHOT = "_Z12frame_kernelILb0ELb{env}EEv9FrameArgs"
ACC = "_Z16frame_kernel_accILb0ELb{env}EEv12FrameAccArgs"
ENTRY_POINTS = ("prt_hip_accum_reset", "prt_hip_render_accumulate", "prt_hip_accum_resolve", "prt_hip_accum_export", "prt_hip_accum_import")


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


@pytest.mark.parametrize("env", [0, 1])
def test_accumulating_frame_kernel_keeps_the_frame_kernels_occupancy(env):
    """frame_kernel_acc<false, ENV>: at most 64 VGPRs and 80 SGPRs (8 waves per SIMD), the one-shot kernel's LDS, and the same
    traversal functions (so the same scratch-free step loop, test_step_loop_has_no_scratch_access).  Its call-stack scratch (the
    shade functions' spills, which the one-shot kernel has too) stays within 16 bytes of the one-shot kernel's."""
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    import step_loop_isa as S
    one, acc = S.kernel_resources(kernel=ONE_SHOT.format(env=env)), S.kernel_resources(kernel=ACC.format(env=env))
    assert acc, "frame_kernel_acc is not in the compiled kernels"
    assert acc["VGPRs"] <= 64 and acc["TotalSGPRs"] <= 80 and acc["Occupancy"] == 8, acc
    assert acc["LDS Size"] == one["LDS Size"] and 2 * acc["LDS Size"] <= 160 * 1024, (acc, one)
    assert acc["ScratchSize"] <= one["ScratchSize"] + 16, (acc, one)
    asm = S.device_asm()
    body = S.function_body(asm, ACC.format(env=env))
    calls = set(re.findall(r"(_Z11trace_queueILi[0-3]ELb0EEvm)", "\n".join(body)))
    assert len(calls) == 4, calls


def test_product_exports_the_progressive_entry_points(L):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    for name in ENTRY_POINTS:
        assert re.search(rf" T {name}$", syms, re.M), name
        assert name in prt_amd.EXPORTS, name


def test_header_documents_progressive_rendering():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", src), name
    assert "prt_accum_info" in src
    block = src[src.index("progressive rendering"):]
    for rule in ("bit for bit", "2^24", "multiple of 8", "seed, maxDepth and rrDepth", "prt_hip_set_camera and prt_hip_upload_scene"):
        assert rule in block, rule


def test_python_host_binds_the_accumulator_structure():
    assert [n for n, _ in prt_amd.AccumInfo._fields_] == ["width", "height", "seed", "maxDepth", "rrDepth"]
    for m in ("accumulate", "accumulate_async", "accum_reset", "accum_counts", "accum_resolve", "accum_export", "accum_import",
              "render_progressive"):
        assert callable(getattr(prt_amd.PathTracer, m)), m
