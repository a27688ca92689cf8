// prt_temporal.hip -- temporal reprojection for the denoised previews (include/prt_hip.h "temporal reprojection"): a first-hit
// position guide per pixel, and a gather kernel that merges the history of the previous view into the current pixel's radiance and
// variance before the a-trous iterations of prt_denoise.hip run.  In a translation unit of its own, as prt_select.hip and
// prt_denoise.hip are, so that the code objects of every other kernel do not move.  Every operation of the merge is the header's, in
// the header's order: f32, no FMA (-ffp-contract=off), correctly rounded divide and sqrt, subnormals kept.  The tests compare the
// output with a numpy restatement of that text at tolerance 0, so nothing here may be reassociated or "simplified".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "prt_internal.h"
#ifdef PRT_TEST_ENTRY_POINTS
#include "../../include/prt_hip_test.h"
#endif

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

// ============================================================================ the position guide
// One ray per pixel through the pixel's centre (camera.cpp:46-56 with both jitter terms 0.0f), the single-ray nearest traversal of
// the G-buffer kernel (alpha tests included), and a hit sink that writes {pos + t*dir, t} -- no surface fetch, no texture tap.
struct PosArgs {
    DevScene sc;
    DevCamera cam;
    float4* xyzt;
    BatchCtl ctl;
};

__device__ __forceinline__ Vec3 centre_dir(const DevCamera& cam, uint32_t x, uint32_t y)
{
    const float kAspect = (float)cam.width / (float)cam.height;
    const float nx = 2.0f * ((float)x * cam.invWidth - 0.5f + 0.0f) * 0.6f * kAspect;
    const float ny = -2.0f * ((float)y * cam.invHeight - 0.5f + 0.0f) * 0.6f;
    const Vec3 right = mk3(cam.right[0], cam.right[1], cam.right[2]);
    const Vec3 up = mk3(cam.up[0], cam.up[1], cam.up[2]);
    const Vec3 fwd = mk3(cam.dir[0], cam.dir[1], cam.dir[2]);
    const Vec3 v = add3(add3(scale3(nx, right), scale3(ny, up)), fwd);
    const float inv = 1.0f / sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    return scale3(inv, v);
}

struct PosSrc {
    const PosArgs* A;
    __device__ __forceinline__ uint32_t count() const { return A->cam.width * A->cam.height; }
    __device__ __forceinline__ uint32_t* cursor() const { return A->ctl.cursor; }
    __device__ __forceinline__ void load(uint32_t i, Vec3& org, Vec3& dir, float& maxT, uint32_t& rev) const
    {
        org = mk3(A->cam.pos[0], A->cam.pos[1], A->cam.pos[2]);
        dir = centre_dir(A->cam, i % A->cam.width, i / A->cam.width);
        maxT = 100000.0f;
        rev = 0;
    }
    __device__ __forceinline__ void store_hit(uint32_t i, const DevHit& h) const
    {
        float4 o = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (h.t != -1.0f) {
            const Vec3 d = centre_dir(A->cam, i % A->cam.width, i / A->cam.width);
            o = make_float4(A->cam.pos[0] + h.t * d.x, A->cam.pos[1] + h.t * d.y, A->cam.pos[2] + h.t * d.z, h.t);
        }
        A->xyzt[i] = o;
    }
    __device__ __forceinline__ void store_occ(uint32_t, bool) const {}
};

__global__ __launch_bounds__(PRT_BLOCK) void position_kernel(PosArgs A)
{
    PosSrc src{&A};
    trace_batch<PRT_MODE_SINGLE>(A.sc, src, A.ctl);
}

// ============================================================================ the merge kernel
#define TP_TILE_X 64 // the tiles of dn_iter_kernel: one wavefront = 64 consecutive pixels of a row
#define TP_TILE_Y 4

__device__ __forceinline__ float tp_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
__device__ __forceinline__ float tp_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

struct MergeArgs {
    const float4* acc;    // {sum.xyz, bits(count)}
    const float4* mom;    // {mean, M2, bits(m), 0} or nullptr: every variance unknown
    const float* albedo;  // guide planes, 3 floats per pixel
    const float* normal;
    const float4* pos;    // {X.xyz, t}
    const float4* hC;     // history, or nullptr: no history exists (or maxHistory is 0)
    const float4* hX;
    const float4* hN;
    float4* cv;           // {C0, V0}: the iterations' input
    float4* ga;           // {A, valid}
    float4* gn;           // {N, 0}
    float4* pC;           // pending
    float4* pX;
    float4* pN;
    uint32_t W, H;
    int demod;
    float hcPos[3], hcRight[3], hcUp[3], hcDir[3]; // the history's camera
    float tol2;           // positionTolerance * positionTolerance
    float normalCos, maxHistory;
};

// One pixel per thread: the work of dn_prepare_kernel plus the reprojection gather (up to four taps of the three history planes) and
// the pending record.
__global__ __launch_bounds__(TP_TILE_X * TP_TILE_Y) void tp_merge_kernel(MergeArgs a)
{
    const uint32_t x = blockIdx.x * TP_TILE_X + (threadIdx.x & (TP_TILE_X - 1));
    const uint32_t y = blockIdx.y * TP_TILE_Y + (threadIdx.x / TP_TILE_X);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const float4 A4 = a.acc[p];
    const uint32_t cnt = __float_as_uint(A4.w);
    const bool valid = cnt > 0;
    const float ax = a.albedo[3 * p], ay = a.albedo[3 * p + 1], az = a.albedo[3 * p + 2];
    const float gx = a.normal[3 * p], gy = a.normal[3 * p + 1], gz = a.normal[3 * p + 2];
    const bool miss = gx == 0.0f && gy == 0.0f && gz == 0.0f;
    const float Nx = miss ? 0.0f : (gx - 0.5f) * 2.0f, Ny = miss ? 0.0f : (gy - 0.5f) * 2.0f, Nz = miss ? 0.0f : (gz - 0.5f) * 2.0f;
    const float4 P = a.pos[p];
    const float fc = (float)cnt;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, v = -1.0f;
    if (valid) {
        cx = A4.x / fc;
        cy = A4.y / fc;
        cz = A4.z / fc;
        if (a.mom) {
            const float4 m4 = a.mom[p];
            const uint32_t m = __float_as_uint(m4.z);
            if (m >= 2) v = (m4.y / (float)(m - 1)) / (float)(cnt >> 3);
        }
    }
    const bool geom = valid && P.w >= 0.0f;
    bool have = false;
    float sumW = 0.0f, sumL = 0.0f, sumVh = 0.0f, sumWv = 0.0f, sumX = 0.0f, sumY = 0.0f, sumZ = 0.0f;
    if (geom && a.hC) {
        const float ex = P.x - a.hcPos[0], ey = P.y - a.hcPos[1], ez = P.z - a.hcPos[2];
        const float ra = tp_dot(ex, ey, ez, a.hcRight[0], a.hcRight[1], a.hcRight[2]);
        const float rb = tp_dot(ex, ey, ez, a.hcUp[0], a.hcUp[1], a.hcUp[2]);
        const float z = tp_dot(ex, ey, ez, a.hcDir[0], a.hcDir[1], a.hcDir[2]);
        if (z > 0.0f) {
            const float kAspect = (float)a.W / (float)a.H;
            const float fW = (float)a.W, fH = (float)a.H;
            const float fx = ((ra / z) / ((2.0f * 0.6f) * kAspect) + 0.5f) * fW;
            const float fy = (0.5f - (rb / z) / (2.0f * 0.6f)) * fH;
            if (fx >= -1.0f && fx < fW && fy >= -1.0f && fy < fH) {
                const float fix = floorf(fx), fiy = floorf(fy);
                const float tx = fx - fix, ty = fy - fiy;
                const int ix = (int)fix, iy = (int)fiy;
                const float lim = a.tol2 * (P.w * P.w);
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = ix + i, qy = iy + j;
                        if (qx < 0 || qy < 0 || qx >= (int)a.W || qy >= (int)a.H) continue;
                        const size_t q = (size_t)qy * a.W + qx;
                        const float4 Xq = a.hX[q];
                        if (!(Xq.w > 0.0f)) continue;
                        const float4 Nq = a.hN[q];
                        const float dx = P.x - Xq.x, dy = P.y - Xq.y, dz = P.z - Xq.z;
                        if (!(tp_dot(dx, dy, dz, dx, dy, dz) <= lim && tp_dot(Nx, Ny, Nz, Nq.x, Nq.y, Nq.z) >= a.normalCos)) continue;
                        const float4 Cq = a.hC[q];
                        const float wb = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        sumW = sumW + wb;
                        sumX = sumX + wb * Cq.x;
                        sumY = sumY + wb * Cq.y;
                        sumZ = sumZ + wb * Cq.z;
                        sumL = sumL + wb * Xq.w;
                        if (Cq.w >= 0.0f) {
                            sumVh = sumVh + wb * Cq.w;
                            sumWv = sumWv + wb;
                        }
                    }
                }
                have = sumW > 0.015625f;
            }
        }
    }
    float mx = cx, my = cy, mz = cz, vm = v, len = valid ? fc : 0.0f;
    if (have) {
        const float Hx = sumX / sumW, Hy = sumY / sumW, Hz = sumZ / sumW;
        const float ql = sumL / sumW;
        const float Hl = ql < a.maxHistory ? ql : a.maxHistory;
        const float Hv = sumWv > 0.0f ? sumVh / sumWv : -1.0f;
        const float tot = fc + Hl;
        mx = (fc * cx + Hl * Hx) / tot;
        my = (fc * cy + Hl * Hy) / tot;
        mz = (fc * cz + Hl * Hz) / tot;
        if (v >= 0.0f && Hv >= 0.0f) vm = ((fc * fc) * v + (Hl * Hl) * Hv) / (tot * tot);
        else if (v >= 0.0f) vm = (v * fc) / tot;
        else if (Hv >= 0.0f) vm = (Hv * Hl) / tot;
        else vm = -1.0f;
        len = tot;
    }
    float4 o = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (valid) {
        float ox = mx, oy = my, oz = mz, ov = vm;
        if (a.demod) {
            const float dx = ax > 0.015625f ? ax : 0.015625f, dy = ay > 0.015625f ? ay : 0.015625f, dz = az > 0.015625f ? az : 0.015625f;
            ox = mx / dx;
            oy = my / dy;
            oz = mz / dz;
            const float ld = tp_lum(dx, dy, dz);
            ov = vm < 0.0f ? -1.0f : vm / (ld * ld);
        }
        o = make_float4(ox, oy, oz, ov);
    }
    a.cv[p] = o;
    a.ga[p] = make_float4(ax, ay, az, valid ? 1.0f : 0.0f);
    a.gn[p] = make_float4(Nx, Ny, Nz, 0.0f);
    a.pC[p] = make_float4(mx, my, mz, vm);
    a.pX[p] = make_float4(P.x, P.y, P.z, geom ? len : 0.0f);
    a.pN[p] = make_float4(Nx, Ny, Nz, 0.0f);
}

// ============================================================================ host side
int check_temporal(const prt_temporal_params* t)
{
    if (!std::isfinite(t->positionTolerance) || !(t->positionTolerance > 0.0f))
        return fail(PRT_HIP_EINVAL, "denoise_temporal: positionTolerance must be finite and > 0");
    if (!(t->normalCos >= -1.0f && t->normalCos <= 1.0f)) return fail(PRT_HIP_EINVAL, "denoise_temporal: normalCos must be in [-1, 1]");
    if (!std::isfinite(t->maxHistory) || !(t->maxHistory >= 0.0f))
        return fail(PRT_HIP_EINVAL, "denoise_temporal: maxHistory must be finite and >= 0");
    return PRT_HIP_OK;
}

// The six record planes at the camera's size.  Records of another size were dropped when the camera changed, so nothing is lost.
int records_ready(prt_hip_ctx* c)
{
    const size_t n = (size_t)c->cam.width * c->cam.height;
    HIP_TRY(hipSetDevice(c->device));
    bool fresh = false;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3; k++) {
        if (e == hipSuccess) e = c->tpHist[k].fit(n, c->stream, &fresh);
        if (e == hipSuccess) e = c->tpPend[k].fit(n, c->stream, &fresh);
    }
    if (fresh) c->tpHaveHist = c->tpHavePend = false;
    HIP_TRY(e);
    return PRT_HIP_OK;
}

int position_plane(prt_hip_ctx* c)
{
    const size_t n = (size_t)c->cam.width * c->cam.height;
    HIP_TRY(hipSetDevice(c->device));
    bool fresh = false;
    hipError_t e = c->tpPos.fit(n, c->stream, &fresh);
    if (fresh) c->tpPosValid = c->tpHostPos = false;
    HIP_TRY(e);
    return PRT_HIP_OK;
}

// The position guide of the current view on the context's stream: the host's own, or one launch of the position kernel over the
// whole image when it is stale (force: also when it is not).  Launched as the G-buffer is: as many workgroups, not timed.
int position_ready(prt_hip_ctx* c, bool force = false)
{
    if (!c->haveScene || !c->haveCamera) return fail(PRT_HIP_ESTATE, "upload a scene and set a camera first");
    int rc = position_plane(c);
    if (rc) return rc;
    if (!force && (c->tpHostPos || c->tpPosValid)) return PRT_HIP_OK;
    const uint32_t W = c->cam.width, H = c->cam.height;
    if ((uint64_t)W * H > 0xffffffffull) return fail(PRT_HIP_EINVAL, "image too large");
    BatchLaunch L;
    if ((rc = prt_batch_begin(c, (uint64_t)W * H, (uint32_t)c->computeUnits * PRT_BATCH_BLOCKS_PER_CU, false, &L))) return rc;
    PosArgs A{c->sc, c->cam, c->tpPos, L.ctl};
    hipLaunchKernelGGL(position_kernel, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    if ((rc = prt_batch_end(c, L, "position_kernel"))) return rc;
    c->tpPosValid = true;
    return PRT_HIP_OK;
}

// The merge kernel on the context's stream: accumulator + moments + guides + position + history -> the iterations' planes and pending.
int run_merge(prt_hip_ctx* c, const prt_denoise_params* d, const prt_temporal_params* t)
{
    const uint32_t W = c->cam.width, H = c->cam.height;
    const size_t n = (size_t)W * H;
    MergeArgs A{};
    A.acc = (const float4*)c->accSum;
    A.mom = (c->accMom.size() == n && !c->momClear) ? c->accMom : nullptr;
    A.albedo = c->dnAlbedo;
    A.normal = c->dnNormal;
    A.pos = c->tpPos;
    if (c->tpHaveHist && t->maxHistory > 0.0f) {
        A.hC = c->tpHist[0];
        A.hX = c->tpHist[1];
        A.hN = c->tpHist[2];
    }
    A.cv = c->dnPlane[0];
    A.ga = c->dnGuideA;
    A.gn = c->dnGuideN;
    A.pC = c->tpPend[0];
    A.pX = c->tpPend[1];
    A.pN = c->tpPend[2];
    A.W = W;
    A.H = H;
    A.demod = (int)d->demodulate;
    for (int k = 0; k < 3; k++) {
        A.hcPos[k] = c->tpHistCam.pos[k];
        A.hcRight[k] = c->tpHistCam.right[k];
        A.hcUp[k] = c->tpHistCam.up[k];
        A.hcDir[k] = c->tpHistCam.dir[k];
    }
    A.tol2 = t->positionTolerance * t->positionTolerance;
    A.normalCos = t->normalCos;
    A.maxHistory = t->maxHistory;
    const dim3 grid((W + TP_TILE_X - 1) / TP_TILE_X, (H + TP_TILE_Y - 1) / TP_TILE_Y);
    hipLaunchKernelGGL(tp_merge_kernel, grid, dim3(TP_TILE_X * TP_TILE_Y), 0, c->stream, A);
    int rc = prt_launched("tp_merge_kernel");
    if (rc) return rc;
    c->tpHavePend = true;
    memcpy(&c->tpPendCam, &c->cam, sizeof(prt_camera_desc));
    return PRT_HIP_OK;
}

int temporal_checks(prt_hip_ctx* c, const prt_denoise_params* d, const prt_temporal_params* t)
{
    if (!c || !d || !t) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = check_temporal(t);
    if (rc) return rc;
    return prt_denoise_checks(c, d);
}

// guides, position, records: everything the merge kernel reads or writes, on the context's stream
int temporal_inputs(prt_hip_ctx* c, const prt_denoise_params* d)
{
    int rc;
    if ((rc = prt_denoise_guides_ready(c, d->guideSamples)) || (rc = position_ready(c)) || (rc = records_ready(c))) return rc;
    return PRT_HIP_OK;
}

} // namespace

void prt_temporal_camera_change(prt_hip_ctx* c, const prt_camera_desc* next)
{
    c->tpPosValid = false;
    c->tpHostPos = false;
    const bool sameSize = c->haveCamera && next->width == c->cam.width && next->height == c->cam.height;
    if (!sameSize) {
        c->tpHaveHist = c->tpHavePend = false;
        return;
    }
    if (c->tpHavePend) { // work already queued on the context's stream keeps its pointers; later work sees the swapped ones
        for (int k = 0; k < 3; k++) c->tpHist[k].swap(c->tpPend[k]);
        c->tpHistCam = c->tpPendCam;
        c->tpHaveHist = true;
        c->tpHavePend = false;
    }
}

void prt_temporal_forget(prt_hip_ctx* c)
{
    c->tpPosValid = false;
    c->tpHostPos = false;
    c->tpHaveHist = c->tpHavePend = false;
}

extern "C" {

int prt_hip_denoise_get_position(prt_hip_ctx* c, float* xyzt)
{
    if (!c || !xyzt) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = position_ready(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(xyzt, c->tpPos, c->tpPos.size() * sizeof(float4), hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_denoise_set_position(prt_hip_ctx* c, const float* xyzt)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!xyzt) { // back to the library's own, rendered on its next use
        c->tpHostPos = false;
        c->tpPosValid = false;
        return PRT_HIP_OK;
    }
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    int rc = position_plane(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream)); // a denoise may still be reading the old plane
    HIP_TRY(hipMemcpy(c->tpPos, xyzt, c->tpPos.size() * sizeof(float4), hipMemcpyHostToDevice));
    c->tpHostPos = true;
    c->tpPosValid = false;
    return PRT_HIP_OK;
}

int prt_hip_accum_denoise_temporal(prt_hip_ctx* c, const prt_denoise_params* d, const prt_temporal_params* t, float exposure, float* d_rgb,
                                   void* stream)
{
    int rc = temporal_checks(c, d, t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = temporal_inputs(c, d)) || (rc = prt_own_framebuffer(c, &d_rgb)) ||
        (rc = run_merge(c, d, t)) || (rc = prt_denoise_iterations(c, d, exposure, d_rgb, nullptr)))
        return rc;
    return prt_stream_leave(c, caller);
}

int prt_hip_history_reset(prt_hip_ctx* c)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    c->tpHaveHist = c->tpHavePend = false;
    return PRT_HIP_OK;
}

int prt_hip_history_export(prt_hip_ctx* c, uint32_t which, prt_camera_desc* camera, float* colorVar, float* posLen, float* normal)
{
    if (!c || !camera || !colorVar || !posLen || !normal) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (which > 1) return fail(PRT_HIP_EINVAL, "history_export: which must be 0 (history) or 1 (pending)");
    if (which == 0 ? !c->tpHaveHist : !c->tpHavePend)
        return fail(PRT_HIP_ESTATE, which == 0 ? "history_export: there is no history" : "history_export: there is no pending record");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const DevBuf<float4>* pl = which == 0 ? c->tpHist : c->tpPend;
    const size_t bytes = c->tpHist[0].size() * sizeof(float4);
    HIP_TRY(hipMemcpy(colorVar, pl[0], bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(posLen, pl[1], bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(normal, pl[2], bytes, hipMemcpyDeviceToHost));
    *camera = which == 0 ? c->tpHistCam : c->tpPendCam;
    return PRT_HIP_OK;
}

int prt_hip_history_import(prt_hip_ctx* c, const prt_camera_desc* camera, const float* colorVar, const float* posLen, const float* normal)
{
    if (!c || !camera || !colorVar || !posLen || !normal) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    if (camera->width != c->cam.width || camera->height != c->cam.height)
        return fail(PRT_HIP_EINVAL, "history_import: the history's size is not the camera's");
    int rc = records_ready(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream)); // a denoise may still be reading the old history
    const size_t bytes = c->tpHist[0].size() * sizeof(float4);
    HIP_TRY(hipMemcpy(c->tpHist[0], colorVar, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->tpHist[1], posLen, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->tpHist[2], normal, bytes, hipMemcpyHostToDevice));
    c->tpHistCam = *camera;
    c->tpHaveHist = true;
    return PRT_HIP_OK;
}

} // extern "C"

#ifdef PRT_TEST_ENTRY_POINTS
extern "C" {

// tools/temporal_bench.py: ms[0] the merge kernel alone, ms[1] the whole temporal denoise (merge + iterations), ms[2] one position
// pass, ms[3] one prt_hip_render_gbuffer launch (type 0) of the same view; HIP events on the context's stream.
int prt_hip_test_temporal_profile(prt_hip_ctx* c, const prt_denoise_params* d, const prt_temporal_params* t, float exposure, float* ms)
{
    if (!ms) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = temporal_checks(c, d, t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    float* rgb = nullptr;
    if ((rc = temporal_inputs(c, d)) || (rc = prt_own_framebuffer(c, &rgb))) return rc;
    StageTimer denoise(2), position(1), gbuffer(1);
    hipStream_t s = c->stream;
    HIP_TRY(denoise.mark(s));
    if ((rc = run_merge(c, d, t))) return rc;
    HIP_TRY(denoise.mark(s));
    if ((rc = run_merge(c, d, t)) || (rc = prt_denoise_iterations(c, d, exposure, rgb, nullptr))) return rc;
    HIP_TRY(denoise.mark(s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(denoise.lap());
    HIP_TRY(denoise.median(0, &ms[0]));
    HIP_TRY(denoise.median(1, &ms[1]));
    ms[2] = 0.0f;
    if (!c->tpHostPos) { // a host's plane is left alone (ms[2] = 0)
        HIP_TRY(position.mark(s));
        if ((rc = position_ready(c, true))) return rc;
        HIP_TRY(position.mark(s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(position.lap());
        HIP_TRY(position.median(0, &ms[2]));
    }
    // the G-buffer launch writes the iterations' spare plane, never the image; both figures include the two small memsets of a launch
    HIP_TRY(gbuffer.mark(s));
    if ((rc = prt_hip_render_gbuffer(c, 0, 0, c->cam.width - 1, c->cam.height - 1, 0, c->accSeed, 1.0f, (float*)(float4*)c->dnPlane[1], nullptr))) return rc;
    HIP_TRY(gbuffer.mark(s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(gbuffer.lap());
    HIP_TRY(gbuffer.median(0, &ms[3]));
    c->dnLast = -1; // dnPlane[1] was overwritten
    return PRT_HIP_OK;
}

} // extern "C"
#endif // PRT_TEST_ENTRY_POINTS
