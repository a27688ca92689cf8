"""Visibility baking without a GPU (include/prt_hip.h "visibility baking"; the GPU half is tests/test_gpu_visibility.py): the two entry
points are declared, documented, exported and wrapped, the numpy restatement the GPU tests hold the product to
(tests/prt_visibility_ref.py) has the properties the header states, and the compiled kernels use what the design says they use."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_bake_ref as BR
import prt_testlib as T
import prt_visibility_ref as VR

F = np.float32
U = np.uint32
B = prt_amd._build
NAMES = ("prt_hip_bake_visibility", "prt_hip_bake_visibility_reduce")


# ----------------------------------------------------------------------------- the interface
def test_the_entry_points_are_exported_and_wrapped():
    prt_amd.build()
    for name in NAMES:
        assert name in prt_amd.EXPORTS
    for path in (prt_amd.LIB_PATH, prt_amd.TEST_LIB_PATH):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in NAMES:
            assert f" T {name}\n" in syms, (path, name)
    assert "prt_visibility.hip" in B.SOURCES and "prt_bake_ray.h" in B.KERNEL_HEADERS
    P = prt_amd.VisibilityParams
    assert C.sizeof(P) == 16 and (P.maxDistance.offset, P.flags.offset, P.reserved.offset) == (0, 4, 8)
    p = P()
    assert (p.maxDistance, p.flags, list(p.reserved)) == (np.inf, 0, [0, 0]) and prt_amd.VIS_TRIPLE == 1
    assert P(2.5, prt_amd.VIS_TRIPLE).maxDistance == 2.5
    for method in ("bake_visibility", "bake_visibility_async", "bake_visibility_reduce", "lightmap_visibility"):
        assert callable(getattr(prt_amd.PathTracer, method))
    sig = inspect.signature(prt_amd.PathTracer.bake_visibility).parameters
    assert list(sig)[1:] == ["points", "normals", "dirs", "weights", "max_distance", "bias", "sets", "triple", "return_bytes"]
    assert (sig["max_distance"].default, sig["bias"].default, sig["triple"].default, sig["return_bytes"].default) == (np.inf, 1e-4, False, False)
    sig = inspect.signature(prt_amd.PathTracer.lightmap_visibility).parameters
    assert list(sig)[1:] == ["uvs_per_mesh", "W", "H", "dirs", "weights", "max_distance", "bias", "set_tile", "gutter", "filter"]
    last = list(inspect.signature(prt_amd.PathTracer.lightmap).parameters.values())[-1]
    assert last.name == "filter" and last.default is None  # lightmap() keeps its signature


def test_header_declares_the_calls_and_carries_the_rules():
    src = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    assert src.index("---- visibility baking") > src.index("---- lightmap filter")
    section = src[src.index("---- visibility baking"):]
    flat = re.sub(r"\s+", " ", section)
    for decl in ("#define PRT_HIP_VIS_TRIPLE 1u",
                 "typedef struct { float maxDistance; /* > 0 or +inf, in units of the ray's dir */ uint32_t flags; /* PRT_HIP_VIS_TRIPLE; other "
                 "bits refused */ uint32_t reserved[2]; /* 0 */ } prt_visibility_params; /* 16 bytes, host memory, read before the call returns */",
                 "int prt_hip_bake_visibility(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, "
                 "const prt_visibility_params* vis, float* out /* n*C, or 3*n*C under TRIPLE */, uint8_t* occluded /* n*K, may be NULL */, "
                 "uint32_t flags, void* stream);",
                 "int prt_hip_bake_visibility_reduce(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, "
                 "const prt_visibility_params* vis, const uint8_t* occluded /* n*K */, float* out, uint32_t flags, void* stream);"):
        assert decl in flat, decl
    text = re.sub(r"[\s*]+", " ", section)
    for rule in ("Ray r = i K + k has the org and dir of prt_hip_bake_rays for the same points and table", "its tMax is vis->maxDistance",
                 "occ[r] is the answer of prt_hip_query_any for that ray, with all of that call's rules: alpha tests apply",
                 'a NaN in org, dir or tMax gives "not occluded" (0) without a walk',
                 "A point with set >= nSets (0xffffffff included) is never traced: its K bytes are 0",
                 "for lane l = 0..63, for channel c: a_l = +0",
                 "for k = l, l+64, l+128, ... < K: if occ[r] == 0 then a_l = a_l + weights[(s K + k) C + c]",
                 "for step = 32, 16, 8, 4, 2, 1, for l < step: a_l = a_l + a_(l+step)",
                 "out[i C + c] = a_0; under PRT_HIP_VIS_TRIPLE out[(i C + c) 3 + h] = a_0 for h = 0, 1, 2",
                 "Any non-zero byte counts as occluded", "An occluded direction's weight is not read into the sum",
                 "A point with set >= nSets writes +0 to all its floats",
                 "K 1 .. 4096, C 1 .. 16, nSets 1 .. 1024, n >= 1, n K <= 2^30", "The 2^24 cap of prt_hip_bake does not apply",
                 "a NULL pointer other than `occluded` in prt_hip_bake_visibility", "maxDistance NaN or <= 0", "unknown bits in vis->flags or flags",
                 "reserved != 0", "a misaligned device pointer", "prt_hip_bake_visibility without a scene is PRT_HIP_ESTATE", "needs no scene",
                 "raysTraced = occludedTraced = n K", "the reduce is not a launch for prt_hip_get_stats",
                 "Not built: distance falloff (needs nearest hits); back-face and validity counts; ranks; a per-ray tMax"):
        assert rule in text, rule


def test_the_calls_fail_loudly_without_a_context():
    """As the baker: PRT_HIP_ENODEVICE where no device exists, PRT_HIP_EINVAL for a NULL context where one does."""
    prt_amd.build()
    L = prt_amd.lib()
    want = -1 if L.prt_hip_device_count() == 0 else -2
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    table = prt_amd.BakeSets(K=1, C=1, nSets=1, reserved=0, dirs=buf.ctypes.data, weights=buf.ctypes.data)
    v = prt_amd.VisibilityParams()
    assert L.prt_hip_bake_visibility(None, 1, p, C.byref(table), C.byref(v), p, p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_bake_visibility_reduce(None, 1, p, C.byref(table), C.byref(v), p, p, prt_amd.QUERY_HOST, None) == want
    assert L.prt_hip_last_error()
    assert not buf.any()


# ----------------------------------------------------------------------------- the restatement
def zero_points(n, sets=0):
    return BR.points(np.zeros((n, 3)), np.zeros((n, 3)), 0, sets)


def one_channel(w, occ):
    """reduce for one point and one channel, by hand: (K,) weights, (K,) bytes."""
    a = []
    for l in range(64):
        s = F(0.0)
        for k in range(l, len(w), 64):
            if occ[k] == 0:
                s = F(s + F(w[k]))
        a.append(s)
    for step in (32, 16, 8, 4, 2, 1):
        a[:step] = [F(a[l] + a[l + step]) for l in range(step)]
    return a[0]


@pytest.mark.parametrize("K", [1, 64, 65, 300])
def test_reduce_equals_the_hand_written_version(K):
    rng = np.random.default_rng(K)
    n, Cc = 3, 2
    w = rng.normal(size=(1, K, Cc)).astype(F)
    occ = (rng.random((n, K)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (n, K)).astype(np.uint8)
    got = VR.reduce(zero_points(n), BR.Sets(np.zeros((1, K, 3)), w), occ)
    assert got.shape == (n, Cc) and got.dtype == F
    for i in range(n):
        for c in range(Cc):
            assert got[i, c].tobytes() == one_channel(w[0, :, c], occ[i]).tobytes(), (i, c)
    triple = VR.reduce(zero_points(n), BR.Sets(np.zeros((1, K, 3)), w), occ, triple=True)
    assert triple.shape == (n, Cc, 3) and all(triple[:, :, h].tobytes() == got.tobytes() for h in range(3))


@pytest.mark.parametrize("K", [1, 2, 64, 128, 4096])
def test_an_open_point_is_exactly_one_and_a_closed_one_plus_zero(K):
    """K a power of two and weights 1/K: every partial sum is a multiple of 1/K below 2^24/K, so no addition rounds."""
    sets = BR.Sets(np.zeros((1, K, 3)), np.full((1, K, 1), 1.0 / K, F))
    assert VR.reduce(zero_points(2), sets, np.zeros((2, K), np.uint8)).tobytes() == np.ones((2, 1), F).tobytes()
    closed = VR.reduce(zero_points(2), sets, np.ones((2, K), np.uint8))
    assert closed.tobytes() == np.zeros((2, 1), F).tobytes(), "+0, not -0"
    sets.weights[:] = -0.0
    assert VR.reduce(zero_points(1), sets, np.zeros((1, K), np.uint8)).tobytes() == np.zeros((1, 1), F).tobytes(), "+0 + -0 = +0"


def test_a_nan_weight_counts_only_where_its_direction_escapes():
    K = 70
    rng = np.random.default_rng(5)
    w = rng.uniform(0.1, 1.0, size=(2, K, 3)).astype(F)
    w[1, 69, 1] = np.nan
    pts = zero_points(4, [0, 1, 1, 0])
    occ = np.zeros((4, K), np.uint8)
    occ[1, 69] = 7  # point 1: the NaN direction is occluded; point 2: it escapes
    got = VR.reduce(pts, BR.Sets(np.zeros((2, K, 3)), w), occ)
    assert np.isfinite(got[[0, 1, 3]]).all(), "an occluded direction's weight is no operand"
    assert np.isnan(got[2, 1]) and np.isfinite(got[2, [0, 2]]).all(), "a visible NaN weight: that point's channel and no other"
    assert got[3].tobytes() == got[0].tobytes()


def test_a_set_outside_the_table_is_plus_zero():
    K = 9
    sets = BR.Sets(np.zeros((2, K, 3)), np.ones((2, K, 2), F))
    got = VR.reduce(zero_points(3, [2, 0xffffffff, 1]), sets, np.zeros((3, K), np.uint8))
    assert got[:2].tobytes() == np.zeros((2, 2), F).tobytes() and (got[2] == 9).all()


def test_the_order_depends_on_K_alone():
    """Two tables whose weights are equal direction for direction, one of 1 set and C = 1, one of 3 sets and C = 4 with the same column
    in channel 2 of set 1: the same bits, whatever n, nSets and C are; and it is within the bound of an f64 sum."""
    K = 300
    rng = np.random.default_rng(9)
    col = (rng.uniform(0.0, 1.0, K) * 10.0 ** rng.uniform(-6, 3, K)).astype(F)
    occ = (rng.random(K) < 0.3).astype(np.uint8)
    a = VR.reduce(zero_points(1), BR.Sets(np.zeros((1, K, 3)), col.reshape(1, K, 1)), occ[None])[0, 0]
    big = rng.normal(size=(3, K, 4)).astype(F)
    big[1, :, 2] = col
    b = VR.reduce(zero_points(5, [0, 2, 1, 1, 0]), BR.Sets(np.zeros((3, K, 3)), big), np.tile(occ, (5, 1)))
    assert b[2, 2].tobytes() == a.tobytes() and b[3, 2].tobytes() == a.tobytes()
    exact = col.astype(np.float64)[occ == 0].sum()
    assert abs(float(a) - exact) <= K * 2.0 ** -24 * exact  # (at most K additions of positive terms, each rounding 2^-24 of a partial sum)


def test_rays_are_the_bakers_with_tmax_set():
    rng = np.random.default_rng(3)
    sets = BR.Sets(rng.normal(size=(2, 5, 3)), np.ones((2, 5, 1)))
    pts = BR.points(rng.normal(size=(4, 3)), rng.normal(size=(4, 3)), 0.01, [0, 1, 2, 1])
    r, base = VR.rays(pts, sets, 2.5), BR.rays(pts, sets)
    assert (r["tMax"] == F(2.5)).all() and r["org"].tobytes() == base["org"].tobytes() and r["dir"].tobytes() == base["dir"].tobytes()
    assert np.isinf(VR.rays(pts, sets, np.inf)["tMax"]).all()


# ----------------------------------------------------------------------------- resources
def resources(source):
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC", "-pthread", "-ldl")]
    cmd = [B.hipcc()] + flags + ["--cuda-device-only", "-c", os.path.join(B.CSRC, source), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
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
    return res


def kernel(res, name):
    found = [r for k, r in res.items() if name in k]
    assert len(found) == 1, (name, sorted(res))
    return found[0]


def test_the_kernels_use_what_the_any_hit_query_uses():
    vis, query = resources("prt_visibility.hip"), resources("prt_query.hip")
    reduce_, trace, any_ = kernel(vis, "vis_reduce_kernel"), kernel(vis, "vis_trace_kernel"), kernel(query, "query_any_kernel")
    print("vis_reduce_kernel", reduce_, "\nvis_trace_kernel", trace, "\nquery_any_kernel", any_)
    assert reduce_["ScratchSize"] == 0 and reduce_["LDS Size"] == 0
    assert trace["ScratchSize"] <= any_["ScratchSize"]
    assert trace["Occupancy"] >= any_["Occupancy"]
