// prt_kernels.hip -- libprt_hip.so: HIP kernels of PRT's per-pixel path-tracing loop for MI355X
// (gfx950, wave64) and the entry points of include/prt_hip.h that launch them: one-shot, accumulate and adaptive renders, the
// accumulator and the G-buffer.  The context, the shared scaffold of an entry point and the read-backs are prt_context.hip, the
// scene upload prt_upload.hip; the kernels and entry points of the row-level tests (test build only) are prt_rowtests.hip.
//
// Execution mapping (DESIGN.md "Kernel"): the reference traces a pixel as samples/8 packets of 8
// paths that share one xorshift32 stream (path_tracer.cpp:57-75).  Here one pixel is owned by 8
// consecutive lanes (one lane = one of the 8 path slots), so a wave64 holds 8 pixels; groups pull
// pixels from an atomic counter in tile-major order.  Every random-number phase of the reference
// draws a statically known number of values per alive slot in slot order, so a lane obtains its
// values by stepping the shared state "number of draws owed by lower slots" times (wave ballot +
// popcount); the ordered compaction of alive paths (path_tracer.cpp:255-293) is a ballot/prefix
// rank followed by an 8-lane gather.  BVH traversal is one lane = one ray with a per-lane stack in
// LDS.  No MFMA: there is no dense contraction on this path.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "prt_frame.h"
#include "prt_lanes.h"

// ============================================================================ G-buffer visualiser
// GbufferVisualizer::TraceBlock (gbuffer_visualizer.cpp:17-51): per pixel ONE jittered single ray (Camera::GenerateJitteredRay,
// camera.cpp:12-33: two generateMinus1to1 draws from the pixel's generator), the single-ray nearest traversal, then the
// surface's diffuse colour (type 0) or bump-mapped normal * 0.5 + 0.5 (types 1, 2).  Same persistent wave loop as the trace
// kernels; the ray source makes the camera ray, the hit sink shades and writes the pixel (Image::writePixel, image.cpp:44-50).
struct GbufArgs {
    DevScene sc;
    DevCamera cam;
    uint32_t x0, y0, rw, rh, type, seed;
    float exposure;
    float* rgb;
    BatchCtl ctl;
};

struct GbufSrc {
    const GbufArgs* A;
    __device__ __forceinline__ uint32_t count() const { return A->rw * A->rh; }
    __device__ __forceinline__ uint32_t* cursor() const { return A->ctl.cursor; }
    __device__ __forceinline__ void load(uint32_t i, Vec3& org, Vec3& dir, float& maxT, uint32_t& rev) const
    {
        const uint32_t x = A->x0 + i % A->rw, y = A->y0 + i / A->rw;
        const uint32_t s1 = xorshift32(pixel_seed(x, y, A->cam.width, A->seed)), s2 = xorshift32(s1);
        org = mk3(A->cam.pos[0], A->cam.pos[1], A->cam.pos[2]);
        dir = camera_dir(A->cam, x, y, s1, s2);
        maxT = 100000.0f; // camera.cpp:26
        rev = 0;
    }
    __device__ __forceinline__ void store_hit(uint32_t i, const DevHit& h) const
    {
        const uint32_t x = A->x0 + i % A->rw, y = A->y0 + i / A->rw;
        Vec3 color = mk3(0.0f, 0.0f, 0.0f);
        if (h.t != -1.0f) {
            Traffic tr{};
            Surface s;
            get_surface<false>(A->sc, h, s, tr);
            if (A->type == 0u) color = sample_diffuse<false>(A->sc, s.mat, s.uv, tr);
            else color = add3(scale3(0.5f, sample_bump<false>(A->sc, s.mat, s, tr)), mk3(0.5f, 0.5f, 0.5f));
        }
        float* px = A->rgb + ((size_t)x + (size_t)y * A->cam.width) * 3;
        px[0] = A->exposure * color.x;
        px[1] = A->exposure * color.y;
        px[2] = A->exposure * color.z;
    }
    __device__ __forceinline__ void store_occ(uint32_t, bool) const {}
};

__global__ __launch_bounds__(PRT_BLOCK) void gbuffer_kernel(GbufArgs A)
{
    GbufSrc src{&A};
    trace_batch<PRT_MODE_SINGLE>(A.sc, src, A.ctl);
}

// ============================================================================ host side of the C-ABI
namespace {
int fail(int code, const std::string& msg) { return prt_fail(code, msg); }
} // namespace

extern "C" {

// ---- frame kernel (prt_frame.h): resident blocks, pool state carved out of one allocation, one launch per render
static int frame_blocks(prt_hip_ctx* c)
{
    if (c->frameBlocksPerCU == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, frame_kernel<false, false>, PRT_BLOCK, 0) != hipSuccess || nb <= 0) nb = 4;
        // No block waits for another one, so a block the hardware admits later than the query says only starts later.
        c->frameBlocksPerCU = std::min(nb, 8);
#ifdef PRT_TUNING_ENV // tuning builds only (tools/build_variants.py): the product reads no tuning variable
        if (const char* e = getenv("PRT_FRAME_BPC")) c->frameBlocksPerCU = std::max(1, std::min(8, atoi(e)));
#endif
    }
    return c->computeUnits * c->frameBlocksPerCU;
}

static int frame_layout(prt_hip_ctx* c, uint32_t blocks, bool env, FrameArgs& A)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t groups = (size_t)blocks * PRT_POOL_GROUPS, slots = groups * 8;
    size_t need = 3 * al(groups * sizeof(uint32_t)) + al(groups * sizeof(float4));
    need += (env ? 7 : 5) * al(slots * sizeof(float4));
    need += al(slots * sizeof(float4)) + al(slots * sizeof(uint2)) + al(slots * sizeof(uint32_t));
    need += al((size_t)blocks * Q_COUNT * PRT_POOL_SLOTS * sizeof(uint32_t));
    HIP_TRY(c->wfBuffer.grow(need, c->stream));
    char* p = c->wfBuffer;
    auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return r; };
    A.gRng = (uint32_t*)take(groups * sizeof(uint32_t));
    A.gInfo = (uint32_t*)take(groups * sizeof(uint32_t));
    A.gPixel = (uint32_t*)take(groups * sizeof(uint32_t));
    A.gColor = (float4*)take(groups * sizeof(float4));
    A.S0 = (float4*)take(slots * sizeof(float4));
    A.S1 = (float4*)take(slots * sizeof(float4));
    A.S2 = (float4*)take(slots * sizeof(float4));
    A.S3 = (float4*)take(slots * sizeof(float4));
    A.S4 = (float4*)take(slots * sizeof(float4));
    A.S5 = env ? (float4*)take(slots * sizeof(float4)) : nullptr;
    A.S6 = env ? (float4*)take(slots * sizeof(float4)) : nullptr;
    A.hitA = (float4*)take(slots * sizeof(float4));
    A.hitB = (uint2*)take(slots * sizeof(uint2));
    A.occl = (uint32_t*)take(slots * sizeof(uint32_t));
    A.qE = (uint32_t*)take((size_t)blocks * Q_COUNT * PRT_POOL_SLOTS * sizeof(uint32_t));
    return PRT_HIP_OK;
}

enum FrameKind { FRAME_ONE_SHOT, FRAME_ACC, FRAME_ADAPT, FRAME_PROBE }; // frame_kernel, frame_kernel_acc, frame_kernel_adapt, frame_kernel_probe
static const char* const kFrameKernelName[] = {"frame_kernel", "frame_kernel_acc", "frame_kernel_adapt", "frame_kernel_probe"};

// probeRays: FRAME_PROBE only, the totalWork rays of the launch (device memory)
static int render_frame_kernel(prt_hip_ctx* c, FrameArgs& A, uint64_t totalWork, hipStream_t s, FrameKind kind, const prt_ray* probeRays = nullptr)
{
    const prt_render_params* p = &A.p;
    A.totalWork = (uint32_t)totalWork;
    A.totalChunks = (uint32_t)((totalWork + PRT_CHUNK - 1) / PRT_CHUNK);
    A.counters = c->counters;
    A.ctrl = c->work;
    const uint32_t resident = (uint32_t)frame_blocks(c);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(resident, A.totalChunks));
    // a block holds at most rowsPerBlock rows at a time and takes one row per visit to the shade role: all of a small launch's
    // rows are in flight at once (a row that starts late costs a whole chain of rounds), spread evenly over the blocks
    A.rowsPerBlock = std::max<uint32_t>(1, std::min<uint32_t>(PRT_POOL_CHUNKS, (A.totalChunks + blocks - 1) / blocks));
    A.spreadRows = (A.totalChunks < (uint64_t)blocks * PRT_POOL_CHUNKS * 2 && totalWork % PRT_CHUNK == 0) ? 1u : 0u;
#ifdef PRT_TUNING_ENV
    if (const char* e = getenv("PRT_SPREAD")) A.spreadRows = atoi(e) && totalWork % PRT_CHUNK == 0;
    if (const char* e = getenv("PRT_ROWS")) A.rowsPerBlock = std::max<uint32_t>(1, std::min<uint32_t>(PRT_POOL_CHUNKS, (uint32_t)atoi(e)));
#endif
    int rc = prt_launch_resources(c, resident);
    if (rc) return rc;
    A.spill = c->spill;
    A.spillStride = c->spillThreads();
    if ((rc = frame_layout(c, resident, c->sc.hasEnv != 0, A))) return rc;
    HIP_TRY(hipMemsetAsync(c->work, 0, PRT_WORK_WORDS * sizeof(uint32_t), s));
    if (A.totalChunks == 0) return PRT_HIP_OK;
    const bool env = c->sc.hasEnv != 0;
// the four instantiations of frame kernel K on (countTraffic, env)
#define PRT_LAUNCH_FRAME(K, ARGS)                                                                              \
    do {                                                                                                       \
        if (p->countTraffic) {                                                                                 \
            if (env) hipLaunchKernelGGL((K<true, true>), dim3(blocks), dim3(PRT_BLOCK), 0, s, ARGS);           \
            else hipLaunchKernelGGL((K<true, false>), dim3(blocks), dim3(PRT_BLOCK), 0, s, ARGS);              \
        } else {                                                                                               \
            if (env) hipLaunchKernelGGL((K<false, true>), dim3(blocks), dim3(PRT_BLOCK), 0, s, ARGS);          \
            else hipLaunchKernelGGL((K<false, false>), dim3(blocks), dim3(PRT_BLOCK), 0, s, ARGS);             \
        }                                                                                                      \
    } while (0)
    if (kind == FRAME_PROBE) { // a batch of probes: the caller's rays behind the arguments (no counting build: prt_hip_query_radiance)
        const FrameProbeArgs dAP{A, probeRays};
        if (env) hipLaunchKernelGGL(frame_kernel_probe<true>, dim3(blocks), dim3(PRT_BLOCK), 0, s, dAP);
        else hipLaunchKernelGGL(frame_kernel_probe<false>, dim3(blocks), dim3(PRT_BLOCK), 0, s, dAP);
    } else if (kind == FRAME_ADAPT) { // an adaptive pass: the accumulate launch with the pixel list and the moments behind its arguments
        const FrameAdaptArgs dAD{FrameAccArgs{A, c->accRng, c->accSum}, c->adList, c->accMom};
        PRT_LAUNCH_FRAME(frame_kernel_adapt, dAD);
    } else if (kind == FRAME_ACC) { // a progressive pass: the same launch with the accumulator behind the arguments
        const FrameAccArgs dAA{A, c->accRng, c->accSum};
        PRT_LAUNCH_FRAME(frame_kernel_acc, dAA);
    } else {
        const FrameArgs& dA = A;
        PRT_LAUNCH_FRAME(frame_kernel, dA);
    }
#undef PRT_LAUNCH_FRAME
    return PRT_HIP_OK;
}

// The set-up of a frame-kernel launch over a checked rectangle, shared by the one-shot, accumulate and adaptive passes: the caller's
// stream is ordered before the context's, the framebuffer is resolved and the launch's geometry and work items are laid out.
struct FrameLaunch {
    FrameArgs A{};
    uint64_t totalWork = 0; // tile-major work items of the rectangle (or of the rank's tiles in it)
    hipStream_t caller = nullptr; // to order behind the launch (prt_stream_leave), or null
};

static int frame_setup(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p, float* d_rgb,
                       void* stream, FrameLaunch& F)
{
    const uint32_t W = c->cam.width;
    HIP_TRY(hipSetDevice(c->device));
    int rc = prt_stream_enter(c, stream, &F.caller);
    if (rc) return rc;
    if ((rc = prt_own_framebuffer(c, &d_rgb))) return rc;
    FrameArgs& A = F.A;
    A.sc = c->sc;
    A.cam = c->cam;
    A.p = *p;
    A.x0 = x0; A.y0 = y0; A.x1 = x1; A.y1 = y1;
    const uint32_t T = p->tileSize;
    if ((uint64_t)T * T > (1u << 20)) return fail(PRT_HIP_EINVAL, "tile too large");
    A.tilesXImage = (W + T - 1) / T;
    A.rtx0 = x0 / T; A.rty0 = y0 / T;
    A.rtnx = x1 / T - A.rtx0 + 1;
    A.rtny = y1 / T - A.rty0 + 1;
    A.fullWidth = (x0 == 0 && x1 == W - 1) ? 1u : 0u;
    const uint32_t tilesInRect = A.rtnx * A.rtny;
    uint64_t totalWork;
    if (A.fullWidth) {
        // tile ids rty0*TX .. (rty0+rtny)*TX - 1 are contiguous; this rank owns ids == rank (mod nranks)
        uint32_t lo = A.rty0 * A.tilesXImage, hi = lo + tilesInRect;
        uint32_t first = lo + ((p->rank + p->nranks - lo % p->nranks) % p->nranks);
        A.firstOwned = first;
        uint32_t owned = first < hi ? (hi - first + p->nranks - 1) / p->nranks : 0;
        totalWork = (uint64_t)owned * T * T;
    } else {
        totalWork = (uint64_t)tilesInRect * T * T;
    }
    if (totalWork > 0xffffffffull) return fail(PRT_HIP_EINVAL, "rectangle too large");
    A.rgb = d_rgb;
    F.totalWork = totalWork;
    return PRT_HIP_OK;
}

// The frame's output has been written (by a launch or, in an adaptive pass without active pixels, by the selection alone): remember
// the output for the gathers and order the caller's stream behind it.
static int frame_finish(prt_hip_ctx* c, const FrameLaunch& F)
{
    c->lastRank = F.A.p.rank;
    c->lastNranks = F.A.p.nranks;
    c->lastTile = F.A.p.tileSize;
    return prt_stream_leave(c, F.caller);
}

// The launch itself, over `totalWork` work items, timed by the context's event ring.
static int frame_launch_timed(prt_hip_ctx* c, FrameArgs& A, uint64_t totalWork, FrameKind kind, const prt_ray* probeRays = nullptr)
{
    hipStream_t s = c->stream;
    HIP_TRY(hipMemsetAsync(c->counters, 0, PRT_STAT_SHARDS * PRT_STAT_STRIDE * sizeof(unsigned long long), s));
    hipEvent_t ev0, ev1;
    int rc = prt_timing_pair(c, &ev0, &ev1);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev0, s));
    if ((rc = render_frame_kernel(c, A, totalWork, s, kind, probeRays)) || (rc = prt_launched(kFrameKernelName[kind]))) return rc;
    HIP_TRY(hipEventRecord(ev1, s));
    return PRT_HIP_OK;
}

static int frame_launch(prt_hip_ctx* c, FrameLaunch& F, uint64_t totalWork, FrameKind kind)
{
    int rc = frame_launch_timed(c, F.A, totalWork, kind);
    return rc ? rc : frame_finish(c, F);
}

// One launch of the frame kernel over a checked rectangle (prt_hip_render, prt_hip_render_accumulate).
static int frame_render(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p, float* d_rgb,
                        void* stream, FrameKind kind)
{
    FrameLaunch F;
    int rc = frame_setup(c, x0, y0, x1, y1, p, d_rgb, stream, F);
    if (rc) return rc;
    return frame_launch(c, F, F.totalWork, kind);
}

int prt_hip_render(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p, float* d_rgb,
                   void* stream)
{
    if (!c || !p) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene || !c->haveCamera) return fail(PRT_HIP_ESTATE, "upload a scene and set a camera first");
    const uint32_t W = c->cam.width, H = c->cam.height;
    int rc = prt_check_rect(c, x0, y0, x1, y1);
    if (rc) return rc;
    if (p->samples == 0 || p->tileSize == 0 || p->nranks == 0 || p->rank >= p->nranks) return fail(PRT_HIP_EINVAL, "bad render params");
    if (W > 65535 || H > 65535 || p->samples / 8 > 255 || p->maxDepth > 255) return fail(PRT_HIP_EINVAL, "image, sample count or depth too large");
    return frame_render(c, x0, y0, x1, y1, p, d_rgb, stream, FRAME_ONE_SHOT);
}

int prt_hip_render_gbuffer(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t type, uint32_t seed, float exposure,
                           float* d_rgb, void* stream)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene || !c->haveCamera) return fail(PRT_HIP_ESTATE, "upload a scene and set a camera first");
    int rc = prt_check_rect(c, x0, y0, x1, y1);
    if (rc) return rc;
    if (type > 2) return fail(PRT_HIP_EINVAL, "type must be 0 (diffuse), 1 (mesh normal) or 2 (normal)");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = prt_own_framebuffer(c, &d_rgb))) return rc;
    const uint32_t rw = x1 - x0 + 1, rh = y1 - y0 + 1;
    if ((uint64_t)rw * rh > 0xffffffffull) return fail(PRT_HIP_EINVAL, "rectangle too large");
    BatchLaunch L; // not timed: a guide launch adds nothing to the statistics of the renders
    if ((rc = prt_batch_begin(c, (uint64_t)rw * rh, (uint32_t)c->computeUnits * PRT_BATCH_BLOCKS_PER_CU, false, &L))) return rc;
    GbufArgs A{c->sc, c->cam, x0, y0, rw, rh, type, seed, exposure, d_rgb, L.ctl};
    hipLaunchKernelGGL(gbuffer_kernel, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    if ((rc = prt_batch_end(c, L, "gbuffer_kernel"))) return rc;
    return prt_stream_leave(c, caller);
}

// ---- progressive rendering (include/prt_hip.h): the accumulator, one (state, sum, count) record per camera pixel
#define PRT_ACC_MAX_COUNT (1u << 24) // a pixel's count as a float is exact up to here

// Allocates the accumulator at the camera's size and zeroes it when a reset is pending (on the context's stream, ahead of
// whatever uses it next).
static int accum_ready(prt_hip_ctx* c)
{
    const size_t n = (size_t)c->cam.width * c->cam.height;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->accRng.fit(n, c->stream, &c->accClear));
    HIP_TRY(c->accSum.fit(n, c->stream, &c->accClear));
    if (c->accClear) {
        HIP_TRY(hipMemsetAsync(c->accRng, 0, n * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->accSum, 0, n * sizeof(float4), c->stream));
        c->accClear = false;
        c->accMax = 0;
    }
    return PRT_HIP_OK;
}

// What an accumulate and an adaptive pass (`who`) ask of the context, the rectangle and the render parameters alike.
static int check_pass(const prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p, const char* who)
{
    if (!c->haveScene || !c->haveCamera) return fail(PRT_HIP_ESTATE, "upload a scene and set a camera first");
    int rc = prt_check_rect(c, x0, y0, x1, y1);
    if (rc) return rc;
    if (p->tileSize == 0 || p->nranks == 0 || p->rank >= p->nranks) return fail(PRT_HIP_EINVAL, "bad render params");
    if (p->samples < 8 || p->samples % 8 != 0 || p->samples / 8 > 255)
        return fail(PRT_HIP_EINVAL, std::string(who) + ": samples must be a multiple of 8 from 8 to 2040 per pass");
    if (c->cam.width > 65535 || c->cam.height > 65535 || p->maxDepth > 255) return fail(PRT_HIP_EINVAL, "image or depth too large");
    return PRT_HIP_OK;
}

// Samples accumulate only under the estimator the accumulated ones came from.
static int check_bound(const prt_hip_ctx* c, const prt_render_params* p, const char* who)
{
    if (c->accMax > 0 && !c->accClear && (p->seed != c->accSeed || p->maxDepth != c->accMaxDepth || p->rrDepth != c->accRrDepth))
        return fail(PRT_HIP_EINVAL, std::string(who) + ": seed, maxDepth and rrDepth must be those of the accumulated samples (reset the accumulator first)");
    return PRT_HIP_OK;
}

static void accum_bind(prt_hip_ctx* c, uint32_t seed, uint32_t maxDepth, uint32_t rrDepth)
{
    c->accSeed = seed;
    c->accMaxDepth = maxDepth;
    c->accRrDepth = rrDepth;
}

int prt_hip_accum_reset(prt_hip_ctx* c)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    prt_accum_forget(c);
    return PRT_HIP_OK;
}

int prt_hip_render_accumulate(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p,
                              float* d_rgb, void* stream)
{
    if (!c || !p) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_pass(c, x0, y0, x1, y1, p, "accumulate")) || (rc = check_bound(c, p, "accumulate")) || (rc = accum_ready(c))) return rc;
    if ((uint64_t)c->accMax + p->samples > PRT_ACC_MAX_COUNT)
        return fail(PRT_HIP_EINVAL, "accumulate: a pixel's total would exceed 2^24 samples");
    if ((rc = frame_render(c, x0, y0, x1, y1, p, d_rgb, stream, FRAME_ACC))) return rc;
    c->accMax += p->samples;
    accum_bind(c, p->seed, p->maxDepth, p->rrDepth);
    return PRT_HIP_OK;
}

int prt_hip_accum_resolve(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float exposure, float* d_rgb, void* stream)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    const uint32_t W = c->cam.width;
    int rc;
    if ((rc = prt_check_rect(c, x0, y0, x1, y1)) || (rc = accum_ready(c))) return rc;
    hipStream_t s = c->stream, caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = prt_own_framebuffer(c, &d_rgb))) return rc;
    const uint32_t rw = x1 - x0 + 1, rh = y1 - y0 + 1; // rw * rh < 2^32: both are at most 65535 (checked by the passes)
    const uint64_t n = (uint64_t)rw * rh;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->computeUnits * 8);
    hipLaunchKernelGGL(accum_resolve_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)c->accSum, W, x0, y0, rw, rh, exposure, d_rgb);
    if ((rc = prt_launched("accum_resolve_kernel"))) return rc;
    return prt_stream_leave(c, caller);
}

int prt_hip_accum_export(prt_hip_ctx* c, prt_accum_info* info, uint32_t* rng, float* sum, uint32_t* count)
{
    if (!c || !info || !rng || !sum || !count) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    int rc = accum_ready(c);
    if (rc) return rc;
    const size_t n = c->accSum.size();
    std::vector<float4> rec(n);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(rng, c->accRng, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rec.data(), c->accSum, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        sum[3 * i] = rec[i].x;
        sum[3 * i + 1] = rec[i].y;
        sum[3 * i + 2] = rec[i].z;
        memcpy(&count[i], &rec[i].w, sizeof(uint32_t));
    }
    const bool bound = c->accMax > 0;
    *info = prt_accum_info{c->cam.width, c->cam.height, bound ? c->accSeed : 0u, bound ? c->accMaxDepth : 0u, bound ? c->accRrDepth : 0u};
    return PRT_HIP_OK;
}

int prt_hip_accum_import(prt_hip_ctx* c, const prt_accum_info* info, const uint32_t* rng, const float* sum, const uint32_t* count)
{
    if (!c || !info || !rng || !sum || !count) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    if (info->width != c->cam.width || info->height != c->cam.height)
        return fail(PRT_HIP_EINVAL, "accum_import: the accumulator is " + std::to_string(info->width) + "x" + std::to_string(info->height) +
                                        ", the camera " + std::to_string(c->cam.width) + "x" + std::to_string(c->cam.height));
    if (info->maxDepth > 255) return fail(PRT_HIP_EINVAL, "accum_import: maxDepth too large");
    const size_t n = (size_t)c->cam.width * c->cam.height;
    std::vector<float4> rec(n);
    uint32_t most = 0;
    for (size_t i = 0; i < n; i++) {
        if (count[i] > PRT_ACC_MAX_COUNT) return fail(PRT_HIP_EINVAL, "accum_import: a count exceeds 2^24");
        float w;
        memcpy(&w, &count[i], sizeof(float));
        rec[i] = make_float4(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2], w);
        most = std::max(most, count[i]);
    }
    int rc = accum_ready(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->accRng, rng, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->accSum, rec.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    c->accMax = most;
    accum_bind(c, info->seed, info->maxDepth, info->rrDepth);
    c->momClear = true; // the moments of the imported samples, if any, come with prt_hip_accum_import_moments
    return PRT_HIP_OK;
}

// ---- adaptive sampling (include/prt_hip.h): the moment records, the selection and the compacted pixel list
#define PRT_ADAPT_MAX_PACKETS (PRT_ACC_MAX_COUNT / 8u) // a moment record counts packets of 8 samples

// Allocates the accumulator and the moment records at the camera's size and zeroes what is stale (on the context's stream).
static int moments_ready(prt_hip_ctx* c)
{
    int rc = accum_ready(c);
    if (rc) return rc;
    const size_t n = c->accSum.size();
    HIP_TRY(c->accMom.fit(n, c->stream, &c->momClear));
    if (c->momClear) {
        HIP_TRY(hipMemsetAsync(c->accMom, 0, n * sizeof(float4), c->stream));
        c->momClear = false;
    }
    return PRT_HIP_OK;
}

// The selection's per-item buffers for `items` work items (the list padded to a multiple of PRT_CHUNK), the compaction's scratch and
// the active count with its pinned host copy.
static int adapt_buffers(prt_hip_ctx* c, uint64_t items)
{
    HIP_TRY(c->adCount.fit(1, c->stream));
    HIP_TRY(c->adCountHost.fit(1));
    const size_t padded = (size_t)((items + PRT_CHUNK - 1) / PRT_CHUNK * PRT_CHUNK);
    HIP_TRY(c->adCode.grow(padded, c->stream));
    HIP_TRY(c->adList.grow(padded, c->stream));
    HIP_TRY(c->adFlag.grow(padded, c->stream));
    size_t bytes = 0;
    HIP_TRY(prt_select_flagged(nullptr, bytes, c->adCode, c->adFlag, c->adList, c->adCount, items, c->stream));
    HIP_TRY(c->adTemp.grow(bytes, c->stream));
    return PRT_HIP_OK;
}

static int check_floor(float floor, const char* who)
{
    if (!(floor > 0.0f) || std::isinf(floor)) return fail(PRT_HIP_EINVAL, std::string(who) + ": floor must be finite and > 0");
    return PRT_HIP_OK;
}

int prt_hip_render_adaptive(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p,
                            const prt_adaptive_params* a, uint32_t* active, float* d_rgb, void* stream)
{
    if (!c || !p || !a || !active) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = check_pass(c, x0, y0, x1, y1, p, "adaptive");
    if (rc) return rc;
    if (!(a->threshold >= 0.0f) || std::isinf(a->threshold)) return fail(PRT_HIP_EINVAL, "adaptive: threshold must be finite and >= 0");
    if ((rc = check_floor(a->floor, "adaptive"))) return rc;
    if (a->minSamples % 8 != 0 || a->maxSamples % 8 != 0)
        return fail(PRT_HIP_EINVAL, "adaptive: minSamples and maxSamples must be multiples of 8");
    if (a->minSamples > a->maxSamples) return fail(PRT_HIP_EINVAL, "adaptive: minSamples must not exceed maxSamples");
    if (a->maxSamples > PRT_ACC_MAX_COUNT) return fail(PRT_HIP_EINVAL, "adaptive: maxSamples must not exceed 2^24");
    if ((rc = check_bound(c, p, "adaptive")) || (rc = moments_ready(c))) return rc;
    FrameLaunch F;
    if ((rc = frame_setup(c, x0, y0, x1, y1, p, d_rgb, stream, F))) return rc;
    if (F.totalWork >= (1ull << 31)) return fail(PRT_HIP_EINVAL, "adaptive: rectangle too large");
    if ((rc = adapt_buffers(c, F.totalWork))) return rc;
    hipStream_t s = c->stream;
    // ---- selection: flag the active items, resolve the others into d_rgb; then compact the active pixels' codes, in work-item order
    uint32_t n = 0;
    if (F.totalWork > 0) {
        F.A.totalWork = (uint32_t)F.totalWork;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((F.totalWork + 255) / 256, (uint64_t)c->computeUnits * 8);
        hipLaunchKernelGGL(adapt_select_kernel, dim3(blocks), dim3(256), 0, s, F.A, (const float4*)c->accSum, (const float4*)c->accMom, *a,
                           c->adCode, c->adFlag);
        if ((rc = prt_launched("adapt_select_kernel"))) return rc;
        size_t bytes = c->adTemp.size();
        HIP_TRY(prt_select_flagged(c->adTemp, bytes, c->adCode, c->adFlag, c->adList, c->adCount, F.totalWork, s));
        HIP_TRY(hipMemcpyAsync(c->adCountHost, c->adCount, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); // the pass's one synchronisation: the launch is sized by the active count
        n = *c->adCountHost;
    }
    *active = n;
    if (n == 0) { // nothing to trace: the selection has written the whole image; the statistics count no rays
        HIP_TRY(hipMemsetAsync(c->counters, 0, PRT_STAT_SHARDS * PRT_STAT_STRIDE * sizeof(unsigned long long), s));
        return frame_finish(c, F);
    }
    // the list padded to whole rows with the "no pixel" code, so that a small launch spreads its rows (render_frame_kernel)
    const uint64_t padded = ((uint64_t)n + PRT_CHUNK - 1) / PRT_CHUNK * PRT_CHUNK;
    if (padded > n) HIP_TRY(hipMemsetAsync(c->adList + n, 0xff, (size_t)(padded - n) * sizeof(uint32_t), s));
    if ((rc = frame_launch(c, F, padded, FRAME_ADAPT))) return rc;
    // no pixel went above maxSamples: the bound stays tight enough for an adaptive run up to 2^24
    c->accMax = std::min<uint32_t>(c->accMax + p->samples, std::max(c->accMax, a->maxSamples));
    accum_bind(c, p->seed, p->maxDepth, p->rrDepth);
    return PRT_HIP_OK;
}

int prt_hip_accum_error(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float exposure, float floor, float* err)
{
    if (!c || !err) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    const uint32_t W = c->cam.width;
    int rc;
    if ((rc = prt_check_rect(c, x0, y0, x1, y1)) || (rc = check_floor(floor, "accum_error")) || (rc = moments_ready(c))) return rc;
    const uint32_t rw = x1 - x0 + 1, rh = y1 - y0 + 1;
    const size_t n = (size_t)rw * rh;
    if (n > 0xffffffffull) return fail(PRT_HIP_EINVAL, "rectangle too large");
    HIP_TRY(c->adErr.grow(n, c->stream)); // the context keeps the buffer: a viewer may ask once per pass
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->computeUnits * 8);
    hipLaunchKernelGGL(accum_error_kernel, dim3(blocks), dim3(256), 0, c->stream, (const float4*)c->accSum, (const float4*)c->accMom, W, x0, y0,
                       rw, rh, exposure, floor, c->adErr);
    if ((rc = prt_launched("accum_error_kernel"))) return rc;
    std::vector<float> h(n);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(h.data(), c->adErr, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) err[(size_t)(x0 + i % rw) + (size_t)(y0 + i / rw) * W] = h[i];
    return PRT_HIP_OK;
}

int prt_hip_accum_export_moments(prt_hip_ctx* c, float* mom)
{
    if (!c || !mom) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    int rc = moments_ready(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(mom, c->accMom, c->accMom.size() * sizeof(float4), hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_accum_import_moments(prt_hip_ctx* c, const float* mom)
{
    if (!c || !mom) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    const size_t n = (size_t)c->cam.width * c->cam.height;
    std::vector<float4> rec(n);
    for (size_t i = 0; i < n; i++) {
        uint32_t m;
        memcpy(&m, &mom[4 * i + 2], sizeof(uint32_t));
        if (m > PRT_ADAPT_MAX_PACKETS) return fail(PRT_HIP_EINVAL, "accum_import_moments: a packet count exceeds 2^21");
        rec[i] = make_float4(mom[4 * i], mom[4 * i + 1], mom[4 * i + 2], 0.0f);
    }
    int rc = moments_ready(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->accMom, rec.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    return PRT_HIP_OK;
}

} // extern "C"

// ---- radiance queries (prt_hip_query_radiance, prt_query.hip): one timed launch of frame_kernel_probe over n probes on the context's
// stream.  The camera of the launch is the degenerate one of the header's definition -- 1 x 1, up = right = 0 -- whose position and
// direction the kernel takes from d_rays; the image is d_radiance.  Neither the context's camera nor its framebuffer, nor what a
// render leaves for the gathers, is read or written.
int prt_frame_probe(prt_hip_ctx* c, uint32_t n, const prt_ray* d_rays, const prt_render_params* p, float* d_radiance)
{
    FrameArgs A{};
    A.sc = c->sc;
    A.cam.width = A.cam.height = 1;
    A.cam.invWidth = A.cam.invHeight = 1.0f;
    A.p = *p;
    A.rgb = d_radiance;
    return frame_launch_timed(c, A, n, FRAME_PROBE, d_rays);
}
