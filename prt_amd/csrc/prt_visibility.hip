// prt_visibility.hip -- visibility baking (include/prt_hip.h "visibility baking"): points and direction sets in, the summed weights of
// the directions that escape out.  Ambient occlusion, sky visibility, bent normals and SH9 visibility probes are this one sum under
// other weights.  Two kernels:
//     vis_trace_kernel    trace_batch<PRT_MODE_OCC_SINGLE> (prt_batch.h) behind a ray source that builds ray i*K + k in registers
//                         from the point and its direction (bake_ray, prt_bake_ray.h): the rays never exist in memory.  One byte out.
//     vis_reduce_kernel   one wave per point: per lane a strided sum over k of the weights of the directions whose byte is 0, then
//                         the shuffle tree of bake_reduce_kernel, in an order fixed by K alone
// The bytes of a call whose caller wants none live in the context (vsOcc): 1 byte per ray.  In a translation unit of its own, as
// prt_query.hip and prt_bake.hip are, so that the code objects of every other kernel do not move.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "prt_bake_ray.h"
#include "prt_internal.h"

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define PRT_VIS_MAX_RAYS (1u << 30) // the limit of the ray queries (prt_query.hip)
#define PRT_VIS_MAX_K 4096u
#define PRT_VIS_MAX_C 16u
#define PRT_VIS_MAX_SETS 1024u
#define PRT_VIS_TRACE_BLOCKS_PER_CU 2  // as query_any_kernel: a workgroup is 16 waves and a CU holds 32
#define PRT_VIS_REDUCE_BLOCKS_PER_CU 8 // blocks of 256 lanes the reduce is launched with at the most: a grid-stride loop
#define PRT_VIS_HELD 4                 // bytes a lane of the reduce keeps in a register: K <= 64 * PRT_VIS_HELD

static_assert(sizeof(prt_bake_point) == 32 && sizeof(prt_visibility_params) == 16, "record sizes of the visibility kernels");

// ============================================================================ trace
struct VisTraceArgs {
    DevScene sc;
    const float4* points; // 2 x float4 per point: {P, bias} {N, set}
    const float* dirs;    // nSets * K * 3
    uint8_t* occ;         // n * K
    uint32_t rays;        // n * K <= 2^30
    uint32_t K, nSets;
    float maxT;           // > 0 or +inf: checked by the host
    BatchCtl ctl;
};

// Ray r = i*K + k.  The 64 rays of a wave share one or two points when K >= 64 (same-address loads of the two float4), and their
// directions lie 12 bytes apart within a set.
struct VisSrc {
    const VisTraceArgs* A;
    __device__ __forceinline__ uint32_t count() const { return A->rays; }
    __device__ __forceinline__ uint32_t* cursor() const { return A->ctl.cursor; }
    __device__ __forceinline__ void load(uint32_t r, Vec3& org, Vec3& dir, float& maxT, uint32_t& rev) const
    {
        const uint32_t i = r / A->K, k = r - i * A->K;
        // a set outside the table is never followed and never traced: trace_loop answers a NaN origin without a walk
        if (!bake_ray(A->points, A->dirs, A->K, A->nSets, i, k, org, dir)) org.x = asf(0x7fc00000u);
        maxT = A->maxT;
        rev = 0;
    }
    __device__ __forceinline__ void store_hit(uint32_t, const DevHit&) const {}
    __device__ __forceinline__ void store_occ(uint32_t r, bool occ) const { A->occ[r] = occ ? 1 : 0; }
};

__global__ __launch_bounds__(PRT_BLOCK) void vis_trace_kernel(VisTraceArgs A)
{
    VisSrc src{&A};
    trace_batch<PRT_MODE_OCC_SINGLE>(A.sc, src, A.ctl);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&A.ctl.counters[PRT_STAT_RAYS], (unsigned long long)A.rays);
        atomicAdd(&A.ctl.counters[PRT_STAT_OCCL], (unsigned long long)A.rays);
    }
}

// ============================================================================ reduce
struct VisReduceArgs {
    const float4* points;
    const float* weights; // nSets * K * C
    const uint8_t* occ;   // n * K
    float* out;           // n * C, or 3 * n * C
    uint32_t n, K, C, nSets;
    uint32_t rep;         // floats written per channel: 1, or 3 under PRT_HIP_VIS_TRIPLE
};

// step = 32 .. 1, a_l = a_l + a_(l + step) for l < step: the tree of bake_reduce_kernel (prt_bake.hip)
__device__ __forceinline__ float vis_tree(float a)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) a = a + __shfl_down(a, step, 64);
    return a;
}

// One wave per point, four per block.  Lane l sums k = l, l + 64, ...: a wave reads 64 consecutive bytes per trip.  With K <= 256 the
// lane's bytes stay in one register over the C channels; a larger K reads them again per channel (they are in the cache by then).
// The weight of an occluded direction is not loaded.  Every trip count is uniform over the wave, so all 64 lanes reach every shuffle.
__global__ __launch_bounds__(256) void vis_reduce_kernel(VisReduceArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < A.n; i += gridDim.x * 4u) {
        const uint32_t set = asu(gld4(A.points + 2 * (size_t)i + 1).w);
        const uint32_t floats = A.C * A.rep; // <= 48
        float* o = A.out + (size_t)i * floats;
        if (set >= A.nSets) {
            if (lane < floats) o[lane] = 0.0f;
            continue;
        }
        const float* w = A.weights + (size_t)set * A.K * A.C;
        const uint8_t* b = A.occ + (size_t)i * A.K;
        if (A.K <= 64u * PRT_VIS_HELD) {
            uint32_t open = 0; // bit j: direction lane + 64 j exists and escapes
#pragma unroll
            for (uint32_t j = 0; j < PRT_VIS_HELD; j++) {
                const uint32_t k = lane + 64u * j;
                if (k < A.K && gld(b + k) == 0u) open |= 1u << j;
            }
            for (uint32_t c = 0; c < A.C; c++) {
                float a = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < PRT_VIS_HELD; j++)
                    if (open & (1u << j)) a = a + w[(size_t)(lane + 64u * j) * A.C + c];
                a = __shfl(vis_tree(a), 0, 64); // lane 0's sum, for the lanes that write it
                if (lane < A.rep) o[c * A.rep + lane] = a;
            }
        } else {
            for (uint32_t c = 0; c < A.C; c++) {
                float a = 0.0f;
                for (uint32_t k = lane; k < A.K; k += 64u)
                    if (gld(b + k) == 0u) a = a + w[(size_t)k * A.C + c];
                a = __shfl(vis_tree(a), 0, 64); // lane 0's sum, for the lanes that write it
                if (lane < A.rep) o[c * A.rep + lane] = a;
            }
        }
    }
}

// ============================================================================ host side
// What both calls ask of n, the table, the parameters and the flags.  Refused before anything is queued.
int check_visibility(uint32_t n, const prt_bake_sets* t, const prt_visibility_params* v, uint32_t flags, const char* what)
{
    int rc = prt_check_flags(flags, what);
    if (rc) return rc;
    const std::string w(what);
    if (t->K < 1 || t->K > PRT_VIS_MAX_K) return fail(PRT_HIP_EINVAL, w + ": sets->K must be 1 .. 4096");
    if (t->C < 1 || t->C > PRT_VIS_MAX_C) return fail(PRT_HIP_EINVAL, w + ": sets->C must be 1 .. 16");
    if (t->nSets < 1 || t->nSets > PRT_VIS_MAX_SETS) return fail(PRT_HIP_EINVAL, w + ": sets->nSets must be 1 .. 1024");
    if (t->reserved != 0) return fail(PRT_HIP_EINVAL, w + ": sets->reserved must be 0");
    if (n == 0 || (uint64_t)n * t->K > PRT_VIS_MAX_RAYS) return fail(PRT_HIP_EINVAL, w + ": n must be at least 1 and n*K at most 2^30");
    if (!(v->maxDistance > 0.0f)) return fail(PRT_HIP_EINVAL, w + ": vis->maxDistance must be > 0 or +inf"); // (a NaN compares false)
    if (v->flags & ~PRT_HIP_VIS_TRIPLE) return fail(PRT_HIP_EINVAL, w + ": unknown bits in vis->flags");
    if (v->reserved[0] != 0 || v->reserved[1] != 0) return fail(PRT_HIP_EINVAL, w + ": vis->reserved must be 0");
    return PRT_HIP_OK;
}

// One launch of the traversal over the n*K rays on the context's stream, timed as a render: launch_trace of prt_query.hip
int launch_vis_trace(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets& t, const float* dirs, float maxT, uint8_t* occ)
{
    const uint32_t rays = n * t.K;
    BatchLaunch L;
    int rc = prt_batch_begin(c, rays, (uint32_t)c->computeUnits * PRT_VIS_TRACE_BLOCKS_PER_CU, true, &L);
    if (rc) return rc;
    VisTraceArgs A{c->sc, (const float4*)points, dirs, occ, rays, t.K, t.nSets, maxT, L.ctl};
    hipLaunchKernelGGL(vis_trace_kernel, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    return prt_batch_end(c, L, "vis_trace_kernel");
}

int launch_vis_reduce(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets& t, const float* weights, const uint8_t* occ,
                      float* out, uint32_t rep)
{
    VisReduceArgs A{(const float4*)points, weights, occ, out, n, t.K, t.C, t.nSets, rep};
    const uint32_t blocks = std::max(1u, std::min((n + 3u) / 4u, (uint32_t)std::max(c->computeUnits, 1) * PRT_VIS_REDUCE_BLOCKS_PER_CU));
    hipLaunchKernelGGL(vis_reduce_kernel, dim3(blocks), dim3(256), 0, c->stream, A);
    return prt_launched("vis_reduce_kernel");
}

enum { V_POINTS, V_DIRS, V_WEIGHTS, V_OCC, V_OUT, V_ARRAYS };

// What the two calls share behind their checks.  The table and the parameters are copied: the caller may reuse them as soon as the
// call returns.  trace: prt_hip_bake_visibility, whose bytes go to the caller's array or, without one, to the context's.
int run_visibility(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, const prt_visibility_params* vis, bool trace,
                   uint8_t* occ, float* out, uint32_t flags, void* stream, const char* what)
{
    const prt_bake_sets t = *sets;
    const prt_visibility_params v = *vis;
    const size_t nRays = (size_t)n * t.K, entries = (size_t)t.nSets * t.K;
    const uint32_t rep = (v.flags & PRT_HIP_VIS_TRIPLE) ? 3u : 1u;
    PrtIoArray io[V_ARRAYS] = {prt_io_in(points, (size_t)n * sizeof(prt_bake_point), 16),
                               prt_io_in(trace ? t.dirs : nullptr, entries * 3 * sizeof(float), 4),
                               prt_io_in(t.weights, entries * t.C * sizeof(float), 4),
                               trace ? prt_io_out(occ, nRays, 1) : prt_io_in(occ, nRays, 1),
                               prt_io_out(out, (size_t)n * t.C * rep * sizeof(float), 4)};
    return prt_run_io(c, flags, stream, std::string(what) + ": points must be 16-byte aligned, float arrays 4-byte aligned", io, V_ARRAYS, [&]() {
        const prt_bake_point* pts = io[V_POINTS].as<prt_bake_point>();
        uint8_t* bytes = io[V_OCC].as<uint8_t>();
        if (trace) {
            if (!bytes) {
                HIP_TRY(c->vsOcc.grow(nRays, c->stream));
                bytes = c->vsOcc;
            }
            int rc = launch_vis_trace(c, n, pts, t, io[V_DIRS].as<float>(), v.maxDistance, bytes);
            if (rc) return rc;
        }
        return launch_vis_reduce(c, n, pts, t, io[V_WEIGHTS].as<float>(), bytes, io[V_OUT].as<float>(), rep);
    });
}

} // namespace

extern "C" {

int prt_hip_bake_visibility(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, const prt_visibility_params* vis,
                            float* out, uint8_t* occluded, uint32_t flags, void* stream)
{
    if (!c || !points || !sets || !sets->dirs || !sets->weights || !vis || !out) return prt_null_argument("bake_visibility");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "bake_visibility: upload a scene first");
    int rc = check_visibility(n, sets, vis, flags, "bake_visibility");
    if (rc) return rc;
    return run_visibility(c, n, points, sets, vis, true, occluded, out, flags, stream, "bake_visibility");
}

int prt_hip_bake_visibility_reduce(prt_hip_ctx* c, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets,
                                   const prt_visibility_params* vis, const uint8_t* occluded, float* out, uint32_t flags, void* stream)
{
    if (!c || !points || !sets || !sets->weights || !vis || !occluded || !out) return prt_null_argument("bake_visibility_reduce");
    int rc = check_visibility(n, sets, vis, flags, "bake_visibility_reduce");
    if (rc) return rc;
    return run_visibility(c, n, points, sets, vis, false, const_cast<uint8_t*>(occluded), out, flags, stream, "bake_visibility_reduce");
}

} // extern "C"
