// prt_atlas_filter.hip -- the lightmap filter (include/prt_hip.h "lightmap filter"): an edge-avoiding a-trous filter over the baked
// values of an atlas, guided by the world position and normal of every texel's bake point.  Between prt_hip_bake and
// prt_hip_atlas_resolve, as one call:
//     prt_hip_atlas_filter  af_index_kernel    one lane per point: a 32-bit atomic min of q into map[texels[q]] for eligible points
//                           af_prepare_kernel  one lane per point: placed, the footprint f2 and the variance V0, 16 bytes per point
//                           af_iter_kernel     one lane per point, one launch per iteration between two planes: the first reads the
//                                              caller's values, the last writes the caller's out
// The arithmetic is prt_atlas_filter.h, which tests/atlas_filter_main.cpp compiles for the host.  A wavefront is 64 consecutive
// points, and the rasteriser's ascending texels make every tap of a wave a near-contiguous gather: 16-byte loads of the two halves
// of a prt_bake_point, served by L1 / L2 over the 25-fold reuse.  In a translation unit of its own, as prt_atlas.hip and
// prt_bake.hip are, so that the code objects of every other kernel do not move.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "prt_internal.h"
#include "prt_atlas_filter.h"
#ifdef PRT_TEST_ENTRY_POINTS
#include "../../include/prt_hip_test.h"
#endif

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define PRT_AF_MAX_DIM 8192u
#define PRT_AF_MAX_POINTS (1u << 26)
#define PRT_AF_MAX_CHANNELS 16u
#define PRT_AF_BLOCKS_PER_CU 8 // blocks of 256 lanes a kernel is launched with at the most, as in prt_atlas.hip: all are grid-stride loops

static_assert(sizeof(prt_bake_point) == 32 && sizeof(PrtAfQuad) == 16 && sizeof(float4) == 16 && sizeof(prt_atlas_filter_params) == 32,
              "record sizes of the filter kernels");

__global__ __launch_bounds__(256) void af_index_kernel(PrtAfArgs A)
{
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < A.n; q += gridDim.x * 256u)
        if (prt_af_eligible(A, q)) atomicMin(A.map + A.texels[q], q); // (texels[q] < W*H: eligible)
}

__global__ __launch_bounds__(256) void af_prepare_kernel(PrtAfArgs A)
{
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < A.n; q += gridDim.x * 256u) prt_af_prepare(A, q);
}

template <bool LAST, bool MULTI> __global__ __launch_bounds__(256) void af_iter_kernel(PrtAfArgs A)
{
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < A.n; q += gridDim.x * 256u) prt_af_iterate<LAST, MULTI>(A, q);
}

int check_params(const prt_atlas_filter_params& p)
{
    if (p.iterations < 1 || p.iterations > 5) return fail(PRT_HIP_EINVAL, "atlas_filter: iterations must be 1 .. 5");
    if (p.normalPowerLog2 > 7) return fail(PRT_HIP_EINVAL, "atlas_filter: normalPowerLog2 must be 0 .. 7");
    if (!std::isfinite(p.sigmaLuminance) || !(p.sigmaLuminance > 0.0f)) return fail(PRT_HIP_EINVAL, "atlas_filter: sigmaLuminance must be finite and > 0");
    if (!std::isfinite(p.sigmaPosition) || !(p.sigmaPosition > 0.0f)) return fail(PRT_HIP_EINVAL, "atlas_filter: sigmaPosition must be finite and > 0");
    for (uint32_t r : p.reserved)
        if (r != 0) return fail(PRT_HIP_EINVAL, "atlas_filter: reserved must be 0");
    return PRT_HIP_OK;
}

// The map, the records and the planes, then the 2 + iterations launches on the context's stream.  A carries the caller's arrays
// (device memory) and the parameters.  tm (optional, iterations + 3 marks): before the map is cleared and after every launch.
int launch_filter(prt_hip_ctx* c, PrtAfArgs A, uint32_t iterations, float* out, StageTimer* tm)
{
    hipStream_t s = c->stream;
    const size_t total = (size_t)A.W * A.H, floats = (size_t)A.n * A.stride;
    HIP_TRY(c->afMap.grow(total, s));
    HIP_TRY(c->afRec.grow(A.n, s));
    for (uint32_t k = 0; k + 1 < std::min(iterations, 3u); k++) HIP_TRY(c->afPlane[k].grow(floats + A.n, s)); // (two launches need one plane)
    A.map = c->afMap;
    A.rec = (PrtAfQuad*)(float4*)c->afRec;
    if (tm) HIP_TRY(tm->mark(s));
    HIP_TRY(hipMemsetAsync(A.map, 0xff, total * sizeof(uint32_t), s));
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((A.n + 255u) / 256u, (uint64_t)std::max(c->computeUnits, 1) * PRT_AF_BLOCKS_PER_CU));
    int rc;
    hipLaunchKernelGGL(af_index_kernel, dim3(blocks), dim3(256), 0, s, A);
    if ((rc = prt_launched("af_index_kernel"))) return rc;
    if (tm) HIP_TRY(tm->mark(s));
    hipLaunchKernelGGL(af_prepare_kernel, dim3(blocks), dim3(256), 0, s, A);
    if ((rc = prt_launched("af_prepare_kernel"))) return rc;
    if (tm) HIP_TRY(tm->mark(s));
    const bool multi = A.stride > 3;
    A.cin = A.values;
    A.vin = &A.rec->z;
    A.vinStride = 4;
    for (uint32_t i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations;
        float* plane = c->afPlane[i & 1];
        A.step = 1u << i;
        A.cout = last ? out : plane;
        A.vout = last ? nullptr : plane + floats;
        auto kernel = last ? (multi ? af_iter_kernel<true, true> : af_iter_kernel<true, false>)
                           : (multi ? af_iter_kernel<false, true> : af_iter_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, A);
        if ((rc = prt_launched("af_iter_kernel"))) return rc;
        if (tm) HIP_TRY(tm->mark(s));
        A.cin = A.cout;
        A.vin = A.vout;
        A.vinStride = 1;
    }
    return PRT_HIP_OK;
}

// Every refusal of the call but a misaligned device pointer (prt_run_io's)
int filter_checks(prt_hip_ctx* c, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, const prt_bake_point* points, const float* values,
                  uint32_t stride, const prt_atlas_filter_params* params, float* out, uint32_t flags)
{
    if (!c || !texels || !points || !values || !params || !out) return prt_null_argument("atlas_filter");
    int rc = prt_check_flags(flags, "atlas_filter");
    if (rc) return rc;
    if (W < 1 || W > PRT_AF_MAX_DIM || H < 1 || H > PRT_AF_MAX_DIM) return fail(PRT_HIP_EINVAL, "atlas_filter: W and H must be 1 .. 8192");
    if (n < 1 || n > PRT_AF_MAX_POINTS) return fail(PRT_HIP_EINVAL, "atlas_filter: n must be 1 .. 2^26");
    if (stride < 3 || stride > 3 * PRT_AF_MAX_CHANNELS || stride % 3 != 0) return fail(PRT_HIP_EINVAL, "atlas_filter: stride must be 3*C, C 1 .. 16");
    if ((rc = check_params(*params))) return rc;
    const size_t bytes = (size_t)n * stride * sizeof(float);
    const uintptr_t v0 = (uintptr_t)values, o0 = (uintptr_t)out;
    if (v0 < o0 + bytes && o0 < v0 + bytes) return fail(PRT_HIP_EINVAL, "atlas_filter: the ranges of values and out overlap");
    return PRT_HIP_OK;
}

PrtAfArgs filter_args(uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, const prt_bake_point* points, const float* values, uint32_t stride,
                      const prt_atlas_filter_params& p)
{
    PrtAfArgs A{};
    A.W = W;
    A.H = H;
    A.n = n;
    A.stride = stride;
    A.texels = texels;
    A.points = points;
    A.values = values;
    A.npl2 = p.normalPowerLog2;
    A.sigL = p.sigmaLuminance;
    A.sigP2 = p.sigmaPosition * p.sigmaPosition;
    return A;
}

} // namespace

extern "C" {

int prt_hip_atlas_filter(prt_hip_ctx* c, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, const prt_bake_point* points,
                         const float* values, uint32_t stride, const prt_atlas_filter_params* params, float* out, uint32_t flags, void* stream)
{
    int rc = filter_checks(c, W, H, n, texels, points, values, stride, params, out, flags);
    if (rc) return rc;
    const size_t bytes = (size_t)n * stride * sizeof(float);
    PrtIoArray io[4] = {prt_io_in(texels, (size_t)n * sizeof(uint32_t), 4), prt_io_in(points, (size_t)n * sizeof(prt_bake_point), 16),
                        prt_io_in(values, bytes, 4), prt_io_out(out, bytes, 4)};
    return prt_run_io(c, flags, stream, "atlas_filter: points must be 16-byte aligned, texels, values and out 4-byte aligned", io, 4, [&]() {
        return launch_filter(c, filter_args(W, H, n, io[0].as<uint32_t>(), io[1].as<prt_bake_point>(), io[2].as<float>(), stride, *params),
                             params->iterations, io[3].as<float>(), nullptr);
    });
}

} // extern "C"

#ifdef PRT_TEST_ENTRY_POINTS
extern "C" {

// tools/query_bench.py --atlas-filter: the filter on DEVICE arrays between two events, then once more with an event after every launch
int prt_hip_test_atlas_filter_profile(prt_hip_ctx* c, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, const prt_bake_point* points,
                                      const float* values, uint32_t stride, const prt_atlas_filter_params* params, float* out, float* ms)
{
    if (!ms) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = filter_checks(c, W, H, n, texels, points, values, stride, params, out, 0);
    if (rc) return rc;
    if (((uintptr_t)points & 15) || (((uintptr_t)texels | (uintptr_t)values | (uintptr_t)out) & 3)) return fail(PRT_HIP_EINVAL, "atlas_filter_profile: a misaligned pointer");
    HIP_TRY(hipSetDevice(c->device));
    const PrtAfArgs A = filter_args(W, H, n, texels, points, values, stride, *params);
    const uint32_t it = params->iterations;
    StageTimer whole(1), each(it + 2);
    HIP_TRY(whole.mark(c->stream));
    if ((rc = launch_filter(c, A, it, out, nullptr))) return rc;
    HIP_TRY(whole.mark(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(whole.lap());
    HIP_TRY(whole.median(0, &ms[7]));
    if ((rc = launch_filter(c, A, it, out, &each))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(each.lap());
    for (uint32_t k = 0; k < 7; k++) ms[k] = 0.0f;
    for (uint32_t k = 0; k < it + 2; k++) HIP_TRY(each.median(k, &ms[k]));
    return PRT_HIP_OK;
}

} // extern "C"
#endif // PRT_TEST_ENTRY_POINTS
