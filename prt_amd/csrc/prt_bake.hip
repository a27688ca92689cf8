// prt_bake.hip -- baking (include/prt_hip.h "baking"): points and direction sets in, weighted radiance sums out.  What every baker
// wrote around prt_hip_query_radiance on the host -- a tangent frame per point, K local directions rotated into it, n*K rays up,
// n*K radiances down, a weighted mean -- as two kernels around the frame kernel's probe launch (prt_frame_probe, as it stands):
//     bake_rays_kernel    one lane per ray: bake_ray of prt_bake_ray.h, which the visibility baker (prt_visibility.hip) traces too
//     bake_reduce_kernel  one wave per point: per lane a strided sum over k, then a shuffle tree, in an order fixed by K alone
// The rays and the per-ray radiances of prt_hip_bake live in the context (bkRays, bkRad) and never leave the device.  In a translation
// unit of its own, as prt_query.hip is, so that the code objects of every other kernel do not move.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "prt_bake_ray.h"
#include "prt_internal.h"

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define PRT_BAKE_MAX_RAYS (1u << 24) // the probes of one frame-kernel launch (prt_hip_query_radiance)
#define PRT_BAKE_MAX_K 4096u
#define PRT_BAKE_MAX_C 16u
#define PRT_BAKE_MAX_SETS 1024u
#define PRT_BAKE_BLOCKS_PER_CU 8 // blocks of 256 lanes either kernel is launched with at the most: both are grid-stride loops
#define PRT_BAKE_HELD 4          // radiance rows a lane of the reduce keeps in registers: K <= 64 * PRT_BAKE_HELD

static_assert(sizeof(prt_bake_point) == 32 && sizeof(prt_ray) == 32, "record sizes of the bake kernels");

// ============================================================================ rays
struct BakeRaysArgs {
    const float4* points; // 2 x float4 per point: {P, bias} {N, set}
    const float* dirs;    // nSets * K * 3
    float4* rays;         // 2 x float4 per ray: {org, tMax = 0} {dir, pad = 0}
    uint32_t n, K, nSets;
};

// Ray r = i*K + k.  A wave reads 64 consecutive rays' directions (768 contiguous bytes within a set) and writes 2 KB contiguously.
__global__ __launch_bounds__(256) void bake_rays_kernel(BakeRaysArgs A)
{
    const uint32_t total = A.n * A.K; // <= 2^24: checked by the host
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < total; r += gridDim.x * 256u) {
        const uint32_t i = r / A.K, k = r - i * A.K;
        Vec3 org, dir;
        bake_ray(A.points, A.dirs, A.K, A.nSets, i, k, org, dir); // (a set outside the table: org = dir = 0)
        gst4(A.rays + 2 * (size_t)r, make_float4(org.x, org.y, org.z, 0.0f));
        gst4(A.rays + 2 * (size_t)r + 1, make_float4(dir.x, dir.y, dir.z, asf(0u)));
    }
}

// ============================================================================ reduce
struct BakeReduceArgs {
    const float4* points;
    const float* weights; // nSets * K * C
    const float* L;       // 3 * n * K
    float* out;           // 3 * C * n
    uint32_t n, K, C, nSets;
};

// step = 32 .. 1, a_l = a_l + a_(l + step) for l < step: lane 0 ends with the tree of the header (the lanes at and above `step` hold
// values nothing reads)
__device__ __forceinline__ float bake_tree(float a)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) a = a + __shfl_down(a, step, 64);
    return a;
}

// One wave per point, four per block.  Lane l sums k = l, l + 64, ...: a wave reads 64 consecutive radiance rows (768 contiguous
// bytes) per trip.  With K <= 256 the lane's rows stay in registers over the C channels; a larger K reads them again per channel
// (they are in the cache by then).  Every trip count is uniform over the wave, so all 64 lanes reach every shuffle.
__global__ __launch_bounds__(256) void bake_reduce_kernel(BakeReduceArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < A.n; i += gridDim.x * 4u) {
        const uint32_t set = asu(gld4(A.points + 2 * (size_t)i + 1).w);
        float* o = A.out + (size_t)i * 3u * A.C;
        if (set >= A.nSets) {
            if (lane < 3u * A.C) o[lane] = 0.0f; // (3 * C <= 48)
            continue;
        }
        const float* w = A.weights + (size_t)set * A.K * A.C;
        const float* L = A.L + 3 * (size_t)i * A.K;
        if (A.K <= 64u * PRT_BAKE_HELD) {
            float l[PRT_BAKE_HELD][3];
#pragma unroll
            for (uint32_t j = 0; j < PRT_BAKE_HELD; j++) {
                const uint32_t k = lane + 64u * j;
                const bool in = k < A.K;
                l[j][0] = in ? L[3 * (size_t)k] : 0.0f;
                l[j][1] = in ? L[3 * (size_t)k + 1] : 0.0f;
                l[j][2] = in ? L[3 * (size_t)k + 2] : 0.0f;
            }
            for (uint32_t c = 0; c < A.C; c++) {
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < PRT_BAKE_HELD; j++) {
                    const uint32_t k = lane + 64u * j;
                    if (k < A.K) {
                        const float wt = w[(size_t)k * A.C + c];
                        a0 = a0 + wt * l[j][0];
                        a1 = a1 + wt * l[j][1];
                        a2 = a2 + wt * l[j][2];
                    }
                }
                a0 = bake_tree(a0);
                a1 = bake_tree(a1);
                a2 = bake_tree(a2);
                if (lane == 0) {
                    o[3 * c] = a0;
                    o[3 * c + 1] = a1;
                    o[3 * c + 2] = a2;
                }
            }
        } else {
            for (uint32_t c = 0; c < A.C; c++) {
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
                for (uint32_t k = lane; k < A.K; k += 64u) {
                    const float wt = w[(size_t)k * A.C + c];
                    a0 = a0 + wt * L[3 * (size_t)k];
                    a1 = a1 + wt * L[3 * (size_t)k + 1];
                    a2 = a2 + wt * L[3 * (size_t)k + 2];
                }
                a0 = bake_tree(a0);
                a1 = bake_tree(a1);
                a2 = bake_tree(a2);
                if (lane == 0) {
                    o[3 * c] = a0;
                    o[3 * c + 1] = a1;
                    o[3 * c + 2] = a2;
                }
            }
        }
    }
}

// ============================================================================ host side
// What the three calls ask of n, the table and the flags; *rays = n * K.  Refused before anything is queued.
int check_bake(uint32_t n, const prt_bake_sets* t, uint32_t flags, const char* what, uint32_t* rays)
{
    int rc = prt_check_flags(flags, what);
    if (rc) return rc;
    if (t->K < 1 || t->K > PRT_BAKE_MAX_K) return fail(PRT_HIP_EINVAL, std::string(what) + ": sets->K must be 1 .. 4096");
    if (t->C < 1 || t->C > PRT_BAKE_MAX_C) return fail(PRT_HIP_EINVAL, std::string(what) + ": sets->C must be 1 .. 16");
    if (t->nSets < 1 || t->nSets > PRT_BAKE_MAX_SETS) return fail(PRT_HIP_EINVAL, std::string(what) + ": sets->nSets must be 1 .. 1024");
    if (t->reserved != 0) return fail(PRT_HIP_EINVAL, std::string(what) + ": sets->reserved must be 0");
    if (n == 0 || (uint64_t)n * t->K > PRT_BAKE_MAX_RAYS) return fail(PRT_HIP_EINVAL, std::string(what) + ": n must be at least 1 and n*K at most 2^24");
    *rays = n * t->K;
    return PRT_HIP_OK;
}

uint32_t bake_blocks(const prt_hip_ctx* c, uint32_t wanted)
{
    return std::max(1u, std::min(wanted, (uint32_t)std::max(c->computeUnits, 1) * PRT_BAKE_BLOCKS_PER_CU));
}

int launch_rays(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets& t, const float* dirs, prt_ray* rays)
{
    BakeRaysArgs A{(const float4*)points, dirs, (float4*)rays, n, t.K, t.nSets};
    hipLaunchKernelGGL(bake_rays_kernel, dim3(bake_blocks(c, (n * t.K + 255u) / 256u)), dim3(256), 0, c->stream, A);
    return prt_launched("bake_rays_kernel");
}

int launch_reduce(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets& t, const float* weights, const float* radiance,
                  float* out)
{
    BakeReduceArgs A{(const float4*)points, weights, radiance, out, n, t.K, t.C, t.nSets};
    hipLaunchKernelGGL(bake_reduce_kernel, dim3(bake_blocks(c, (n + 3u) / 4u)), dim3(256), 0, c->stream, A);
    return prt_launched("bake_reduce_kernel");
}

// Where the arrays of the three calls stand in the table; an entry a call has no array for stays null.
enum { B_POINTS, B_DIRS, B_WEIGHTS, B_RAYS /* bake_rays: written */, B_RADIANCE /* bake_reduce: read */, B_OUT, B_ARRAYS };

// What the three calls share behind their checks.  The table is copied: the caller may reuse it as soon as the call returns.
// rays: bake_rays; radiance: bake_reduce; params: prt_hip_bake, which traces between the two kernels, its rays and their radiances in
// the context's buffers.  The directions go to the rays kernel and the weights to the reduce, so a call without one stages neither.
int run_bake(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, prt_ray* rays, const float* radiance, float* out,
             const prt_render_params* params, uint32_t flags, void* stream, const char* what)
{
    const prt_bake_sets t = *sets;
    const size_t nRays = (size_t)n * t.K, entries = (size_t)t.nSets * t.K;
    PrtIoArray io[B_ARRAYS] = {prt_io_in(points, (size_t)n * sizeof(prt_bake_point), 16),
                               prt_io_in(rays || params ? t.dirs : nullptr, entries * 3 * sizeof(float), 4),
                               prt_io_in(out ? t.weights : nullptr, entries * t.C * sizeof(float), 4),
                               prt_io_out(rays, nRays * sizeof(prt_ray), 16),
                               prt_io_in(radiance, 3 * nRays * sizeof(float), 4),
                               prt_io_out(out, (size_t)n * 3 * t.C * sizeof(float), 4)};
    return prt_run_io(c, flags, stream, std::string(what) + ": points and rays must be 16-byte aligned, float arrays 4-byte aligned", io, B_ARRAYS, [&]() {
        const prt_bake_point* pts = io[B_POINTS].as<prt_bake_point>();
        const float *dirs = io[B_DIRS].as<float>(), *weights = io[B_WEIGHTS].as<float>();
        if (rays) return launch_rays(c, n, pts, t, dirs, io[B_RAYS].as<prt_ray>());
        if (!params) return launch_reduce(c, n, pts, t, weights, io[B_RADIANCE].as<float>(), io[B_OUT].as<float>());
        int rc;
        HIP_TRY(c->bkRays.grow(nRays, c->stream));
        HIP_TRY(c->bkRad.grow(3 * nRays, c->stream));
        if ((rc = launch_rays(c, n, pts, t, dirs, c->bkRays)) || (rc = prt_frame_probe(c, (uint32_t)nRays, c->bkRays, params, c->bkRad))) return rc;
        return launch_reduce(c, n, pts, t, weights, c->bkRad, io[B_OUT].as<float>());
    });
}

} // namespace

extern "C" {

int prt_hip_bake_rays(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, prt_ray* rays, uint32_t flags,
                      void* stream)
{
    if (!c || !points || !sets || !sets->dirs || !rays) return prt_null_argument("bake_rays");
    uint32_t nRays;
    int rc = check_bake(n, sets, flags, "bake_rays", &nRays);
    if (rc) return rc;
    return run_bake(c, n, points, sets, rays, nullptr, nullptr, nullptr, flags, stream, "bake_rays");
}

int prt_hip_bake_reduce(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, const float* radiance, float* out,
                        uint32_t flags, void* stream)
{
    if (!c || !points || !sets || !sets->weights || !radiance || !out) return prt_null_argument("bake_reduce");
    uint32_t nRays;
    int rc = check_bake(n, sets, flags, "bake_reduce", &nRays);
    if (rc) return rc;
    return run_bake(c, n, points, sets, nullptr, radiance, out, nullptr, flags, stream, "bake_reduce");
}

int prt_hip_bake(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, const prt_render_params* params, float* out,
                 uint32_t flags, void* stream)
{
    if (!c || !points || !sets || !sets->dirs || !sets->weights || !params || !out) return prt_null_argument("bake");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "bake: upload a scene first");
    uint32_t nRays;
    int rc;
    if ((rc = check_bake(n, sets, flags, "bake", &nRays)) || (rc = prt_check_radiance(c, nRays, params, flags, "bake"))) return rc;
    return run_bake(c, n, points, sets, nullptr, nullptr, out, params, flags, stream, "bake");
}

} // extern "C"
