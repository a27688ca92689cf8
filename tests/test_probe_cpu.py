"""Radiance queries without a GPU (include/prt_hip.h "radiance"; the GPU half is tests/test_gpu_probe.py): the entry point is exported,
declared and refused without a context as the other queries are; the helper that states the oracle's answer (tests/prt_probe_ref.py)
is pinned against OracleScene.trace_block; the hostile probes terminate in the oracle and give the answers the header documents."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import prt_amd
import prt_hostile_shade as HS
import prt_probe_ref as PR
import prt_testlib as T

F = np.float32
NAME = "prt_hip_query_radiance"
PROBE_KERNEL = "_Z18frame_kernel_probeILb{env}EEv14FrameProbeArgs"
ONE_SHOT = "_Z12frame_kernelILb0ELb{env}EEv9FrameArgs"


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def test_both_libraries_export_the_entry_point(L):
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert f" T {NAME}\n" in syms, path
    assert NAME in prt_amd.EXPORTS
    assert callable(prt_amd.PathTracer.query_radiance) and callable(prt_amd.PathTracer.query_radiance_async)


def test_header_declares_and_documents_the_contract():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    section = src[src.index("---- ray queries"):]
    assert re.search(rf"\bint {NAME}\(prt_hip_ctx\* ctx, uint32_t n, const prt_ray\* rays, const prt_render_params\* params,\s*"
                     r"float\* radiance /\* 3\*n floats \*/, uint32_t flags, void\* stream\);", section)
    text = re.sub(r"[\s*]+", " ", section)
    for sentence in ("Probe q (0-based) is, bit for bit, pixel (0, 0) of prt_hip_render under the camera",
                     "up = right = (0, 0, 0)", "width = height = 1", "seed is seed + q (uint32 wrap)",
                     "radiance[3q .. 3q+2] = exposure colour / samples",  # (the normalisation above drops the '*')
                     "rays[q].tMax and pad are ignored",
                     "A direction whose squared length overflows or underflows in float",
                     "normalises to zero or to non-finite components",
                     "samples a multiple of 8 from 8 to 2040", "rank must be 0 and nranks 1", "countTraffic must be 0", "tileSize is ignored",
                     "n: 1 .. 2^24 probes", "rays 16-byte aligned and radiance 4-byte aligned",
                     "needs a scene and NO camera", "nPx = n", "One persistent launch whatever n is"):
        assert sentence in text, sentence


def test_the_call_fails_loudly_without_a_context(L):
    """As the other queries (tests/test_query_cpu.py): PRT_HIP_ENODEVICE where no device exists, PRT_HIP_EINVAL for a NULL context where
    one does; NULL rays, params and radiance are refused the same way."""
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(96, np.uint8).ctypes.data_as(C.c_void_p)
    p = prt_amd.RenderParams()
    p.samples, p.nranks = 8, 1
    for args in ((None, 1, buf, C.byref(p), buf), (None, 1, None, C.byref(p), buf), (None, 1, buf, None, buf), (None, 1, buf, C.byref(p), None)):
        rc = L.prt_hip_query_radiance(*args, prt_amd.QUERY_HOST, None)
        assert rc == want, (rc, L.prt_hip_last_error())
        if want == -1:
            assert b"no HIP device" in L.prt_hip_last_error()


def test_probe_kernels_keep_the_frame_kernels_occupancy_and_step_loop():
    """frame_kernel_probe<ENV>: at most 64 VGPRs and 80 SGPRs (8 waves per SIMD) and the one-shot kernel's LDS; its primary rays are
    traced by an instantiation of their own (the origin is the probe's) whose step loop touches no scratch memory and is as long as
    the camera's, its other rays by the frame kernel's three functions."""
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    import step_loop_isa as S
    asm, res = S.device_asm_and_resources()
    for env in (0, 1):
        one, probe = res[ONE_SHOT.format(env=env)], res.get(PROBE_KERNEL.format(env=env))
        assert probe, "frame_kernel_probe is not in the compiled kernels"
        print(f"frame_kernel_probe<{env}>: {probe}; frame_kernel<false, {env}>: {one}")
        assert probe["VGPRs"] <= 64 and probe["TotalSGPRs"] <= 80 and probe["Occupancy"] == 8, probe
        assert probe["LDS Size"] == one["LDS Size"], (probe, one)
        body = "\n".join(S.function_body(asm, PROBE_KERNEL.format(env=env)))
        assert set(re.findall(r"(_Z11trace_queueILi\dELb0EEvm)", body)) == {f"_Z11trace_queueILi{m}ELb0EEvm" for m in (4, 1, 2, 3)}
    sizes = {}
    for mode in (0, 4):  # the camera's packet traversal and the probes'
        loop, lines = S.step_loop(S.function_body(asm, f"_Z11trace_queueILi{mode}ELb0EEvm"))
        sizes[mode], kinds, scratch = S.summary(lines)
        assert not scratch, (mode, scratch)
    print("step loop instructions (camera, probe):", sizes)
    assert sizes[4] == sizes[0] > 100


# ----------------------------------------------------------------------------- the helper
@pytest.fixture(scope="module")
def stage():
    prt_amd.build()
    return T.OracleScene(HS.desc("plain"))


def test_helper_is_trace_block_on_a_camera_zeroed_by_hand(stage):
    """Pins tests/prt_probe_ref.py, not the product: a REAL 1 x 1 camera from orc_camera_create whose up and right are then zeroed and whose
    dir is set to the probe's, traced by OracleScene.trace_block with seed + q, gives the helper's radiance and ray counts."""
    org, d = PR.stage_probes(24, seed=5)
    spp, depth, seed = 16, 6, 777
    got, rays, occl = PR.trace(stage, org, d, spp, depth, seed, exposure=1.5)
    o = T.OracleScene(T.SceneDesc(stage.desc.meshes, org[0], d[0], 1, 1, light=stage.desc.light, exposure=1.5))
    want_rays = want_occl = 0
    for q in range(len(org)):
        o.L.orc_camera_create(C.byref(o.camera), T.f3(org[q]), T.f3(d[q]), 1, 1)
        assert (o.camera.width, o.camera.height, o.camera.invWidth, o.camera.invHeight) == (1, 1, 1.0, 1.0)
        assert tuple(o.camera.pos) == tuple(org[q])
        o.camera.up[:] = o.camera.right[:] = (0.0, 0.0, 0.0)
        o.camera.dir[:] = [float(v) for v in d[q]]  # (orc_camera_create normalises; the probe's direction is as given)
        rgb, st = o.trace_block(0, 0, 0, 0, spp, max_depth=depth, seed=(seed + q) & 0xffffffff)
        assert rgb.reshape(3).tobytes() == got[q].tobytes(), q
        want_rays += st["raysTraced"]
        want_occl += st["occludedTraced"]
    assert (rays, occl) == (want_rays, want_occl)
    assert (got != 0).any(axis=1).sum() > len(org) // 4
    # a subset keeps its indices, and so its seeds
    sub, _, _ = PR.trace(stage, org, d, spp, depth, seed, exposure=1.5, which=[3, 17])
    assert sub[[3, 17]].tobytes() == got[[3, 17]].tobytes() and not sub[0].any()


def test_threads_do_not_change_the_helpers_answer(stage):
    org, d = PR.stage_probes(1024, seed=6)
    a = PR.trace(stage, org, d, 8, 4, 99, workers=1)
    b = PR.trace(stage, org, d, 8, 4, 99, workers=4)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


# ----------------------------------------------------------------------------- hostile probes
@pytest.mark.parametrize("name", ["plain", "box_rr"])
def test_hostile_probes_terminate_in_the_oracle_with_the_documented_answers(name):
    """A direction that normalises to zero or to non-finite components, and a NaN origin: black (+0), with the rays the reference
    counts for such a camera ray -- the packet's 8 primary rays and nothing else.  Probes with -0.0 components, an origin on a
    surface and an origin no ray leaves the scene from are ordinary probes; so are their neighbours."""
    prt_amd.build()
    o = T.OracleScene(HS.desc(name))
    org, d, at = PR.hostile_case(name)
    spp, depth, seed = 16, 8, 4242
    rad, rays, occl = PR.trace(o, org, d, spp, depth, seed)
    for k, hname in enumerate(PR.HOSTILE):
        one, r1, o1 = PR.trace(o, org, d, spp, depth, seed, which=[at[k]])
        assert one[at[k]].tobytes() == rad[at[k]].tobytes()
        print(f"{name} {hname}: radiance {rad[at[k]]}, raysTraced {r1}, occludedTraced {o1}")
        if hname in PR.DEGENERATE or hname == "nan_org":
            assert rad[at[k]].tobytes() == np.zeros(3, F).tobytes(), hname
            assert (r1, o1) == (spp, 0), hname
    rest = np.ones(64, bool)
    rest[at] = False
    assert (rad[rest] != 0).any(axis=1).sum() > rest.sum() // 4
    for hname in ("neg_zero", "neg_zero_axis", "on_surface", "inside"):
        assert rad[at[PR.HOSTILE.index(hname)]].any(), hname
