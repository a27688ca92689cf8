"""Ray queries without a GPU (include/prt_hip.h "ray queries"; the GPU half is tests/test_gpu_query.py): the four entry points are
exported by both builds and documented, the numpy records have the layout of the C structs, the calls fail loudly without a device,
and the ray PathTracer.pick shoots is the position guide's pixel-centre ray, float32 operation by float32 operation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_testlib as T

F = np.float32
ENTRY_POINTS = ("prt_hip_query_nearest", "prt_hip_query_any", "prt_hip_query_surface", "prt_hip_query_get_counts")


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def test_both_libraries_export_the_four_entry_points(L):
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in ENTRY_POINTS:
            assert f" T {name}\n" in syms, (path, name)
    assert set(ENTRY_POINTS) <= set(prt_amd.EXPORTS)
    assert "prt_query.hip" in prt_amd._build.SOURCES


def test_header_documents_the_contract():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    section = src[src.index("---- ray queries"):]
    text = re.sub(r"[\s*]+", " ", section)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(prt_hip_ctx\*", section), name
    for sentence in ("A ray with a NaN in org, dir or tMax is answered as a miss / not occluded without a walk",
                     "The library never stores a NaN t",
                     "Every index read from caller memory is range-checked on the device before it is used as an address",
                     "meshId < the scene's mesh count, primId < that mesh's primitive count",
                     "With PRT_HIP_QUERY_HOST in flags all array pointers are HOST pointers",
                     "rays and surfaces must be 16-byte aligned, hits 4-byte aligned",
                     "There is no tMin"):
        assert sentence in text, sentence
    assert re.search(r"#define PRT_HIP_QUERY_HOST 1u", section)


def test_numpy_records_have_the_layout_of_the_c_structs():
    r, s = prt_amd.RAY_DTYPE, prt_amd.SURFACE_DTYPE
    assert r.itemsize == 32 and s.itemsize == 80 and prt_amd.HIT_DTYPE.itemsize == 24
    assert {k: r.fields[k][1] for k in r.names} == dict(org=0, tMax=12, dir=16, pad=28)
    assert {k: s.fields[k][1] for k in s.names} == dict(P=0, t=12, normal=16, material=28, shadingNormal=32, meshMaterial=44, uv=48,
                                                       primId=56, meshId=60, diffuse=64, pad=76)
    rays = prt_amd.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [0, 1, 0]], [7.0, np.nan])
    w = rays.view(np.uint32).reshape(2, 8)
    assert (w[0, :3].view(F) == (1, 2, 3)).all() and w[0, 3].view(F) == 7 and (w[1, 4:7].view(F) == (0, 1, 0)).all() and np.isnan(w[1, 3].view(F))
    assert (prt_amd.make_rays(np.zeros((5, 3)), np.ones((5, 3)), 2.5)["tMax"] == F(2.5)).all()


def test_calls_fail_loudly_without_a_device(L):
    """Without a device no context can exist (PathTracer() raises "no HIP device"), and the entry points say the same: PRT_HIP_ENODEVICE.
    With a device a NULL context is PRT_HIP_EINVAL."""
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(80, np.uint8).ctypes.data_as(C.c_void_p)
    n = C.c_uint64()
    for rc in (L.prt_hip_query_nearest(None, 1, buf, buf, None, prt_amd.QUERY_HOST, None),
               L.prt_hip_query_any(None, 1, buf, buf, prt_amd.QUERY_HOST, None),
               L.prt_hip_query_surface(None, 1, buf, buf, buf, prt_amd.QUERY_HOST, None),
               L.prt_hip_query_get_counts(None, C.byref(n))):
        assert rc == want, (rc, L.prt_hip_last_error())
        if want == -1:
            assert b"no HIP device" in L.prt_hip_last_error()


def test_pick_ray_is_the_position_guides_centre_ray(L):
    """Three pixels of a 64 x 48 camera, two corners included, against the header's text ("temporal reprojection": nx, ny, v, dirp) written
    out here in float32 scalars."""
    cam = prt_amd.Camera().create((0.3, 0.965, 2.6), (0.1, -0.05, -1.0), 64, 48)
    d = cam.desc
    right, up, fwd, pos = ([F(v) for v in getattr(d, k)] for k in ("right", "up", "dir", "pos"))
    pixels = [(0, 0), (63, 47), (17, 30)]
    rays = prt_amd.pixel_centre_rays(d, [p[0] for p in pixels], [p[1] for p in pixels])
    assert rays.dtype == prt_amd.RAY_DTYPE and len(rays) == 3
    for r, (x, y) in zip(rays, pixels):
        k_aspect = F(64) / F(48)
        nx = F(F(F(F(2.0) * F(F(F(F(x) * F(d.invWidth)) - F(0.5)) + F(0.0))) * F(0.6)) * k_aspect)
        ny = F(F(F(-2.0) * F(F(F(F(y) * F(d.invHeight)) - F(0.5)) + F(0.0))) * F(0.6))
        v = [F(F(F(nx * right[k]) + F(ny * up[k])) + fwd[k]) for k in range(3)]
        inv = F(F(1.0) / np.sqrt(F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2]))))
        want = np.array([F(inv * v[k]) for k in range(3)], dtype=F)
        assert r["dir"].tobytes() == want.tobytes(), (x, y, r["dir"], want)
        assert r["org"].tobytes() == np.array(pos, dtype=F).tobytes() and r["tMax"] == F(100000.0) and r["pad"] == 0
