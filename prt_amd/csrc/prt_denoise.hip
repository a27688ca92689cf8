// prt_denoise.hip -- denoised previews of the accumulator (include/prt_hip.h "denoised previews"): an edge-avoiding a-trous wavelet
// filter guided by first-hit albedo, normal and the variance of the moment records.  In a translation unit of its own, as
// prt_select.hip is, so that the frame kernels' code objects (prt_kernels.hip) do not move.  Every operation below is the header's,
// in the header's order: f32, no FMA (-ffp-contract=off), correctly rounded divide and sqrt, subnormals kept.  The tests compare
// the output with a numpy restatement of that text at tolerance 0, so nothing here may be reassociated or "simplified".
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

#define DN_TILE_X 64 // one wavefront = 64 consecutive pixels of a row: every tap of a wavefront is one contiguous 1 KiB run
#define DN_TILE_Y 4

__device__ __forceinline__ float dn_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// f(x): the eighth power of 1 / (1 + y + y*y/2), y = x/8 -- exp(-x)-like and made of exactly rounded operations only
__device__ __forceinline__ float dn_f(float x)
{
    const float y = 0.125f * x;
    float r = 1.0f / ((1.0f + y) + (0.5f * y) * y);
    r = r * r;
    r = r * r;
    r = r * r;
    return r;
}

// g = first ? t : g + t; the last launch also scales by 1/K (K = 1: g = t * 1.0f = t)
__global__ __launch_bounds__(256) void dn_guide_sum_kernel(float* __restrict__ g, const float* __restrict__ t, size_t n, int first, int last,
                                                           float inv)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = first ? t[i] : g[i] + t[i];
        if (last) v = v * inv;
        g[i] = v;
    }
}

// accumulator + moments + guides -> {C0, V0}, {A, valid}, {N, 0}.  mom == nullptr: no pixel has moments (every variance unknown).
__global__ __launch_bounds__(256) void dn_prepare_kernel(const float4* __restrict__ acc, const float4* __restrict__ mom,
                                                         const float* __restrict__ albedo, const float* __restrict__ normal, size_t n,
                                                         int demod, float4* __restrict__ cv, float4* __restrict__ ga, float4* __restrict__ gn)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float4 a = acc[i];
        const uint32_t cnt = __float_as_uint(a.w);
        const float ax = albedo[3 * i], ay = albedo[3 * i + 1], az = albedo[3 * i + 2];
        const float gx = normal[3 * i], gy = normal[3 * i + 1], gz = normal[3 * i + 2];
        const bool miss = gx == 0.0f && gy == 0.0f && gz == 0.0f;
        const float4 N = miss ? make_float4(0.0f, 0.0f, 0.0f, 0.0f)
                              : make_float4((gx - 0.5f) * 2.0f, (gy - 0.5f) * 2.0f, (gz - 0.5f) * 2.0f, 0.0f);
        float4 o = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (cnt > 0) {
            const float fc = (float)cnt;
            float cx = a.x / fc, cy = a.y / fc, cz = a.z / fc;
            float v = -1.0f;
            if (mom) {
                const float4 m4 = mom[i];
                const uint32_t m = __float_as_uint(m4.z);
                if (m >= 2) v = (m4.y / (float)(m - 1)) / (float)(cnt >> 3);
            }
            if (demod) {
                const float dx = ax > 0.015625f ? ax : 0.015625f, dy = ay > 0.015625f ? ay : 0.015625f, dz = az > 0.015625f ? az : 0.015625f;
                cx = cx / dx;
                cy = cy / dy;
                cz = cz / dz;
                const float ld = dn_lum(dx, dy, dz);
                v = v < 0.0f ? -1.0f : v / (ld * ld);
            }
            o = make_float4(cx, cy, cz, v);
        }
        cv[i] = o;
        ga[i] = make_float4(ax, ay, az, cnt > 0 ? 1.0f : 0.0f);
        gn[i] = N;
    }
}

struct DnIterArgs {
    const float4* in;  // {C, V}; V is -1 at every invalid pixel
    float4* out;
    const float4* ga;  // {A, valid}
    const float4* gn;  // {N, 0}
    uint32_t W, H;
    int step;
    uint32_t npl2;
    float sigL, sigA2; // sigmaLuminance, sigmaAlbedo * sigmaAlbedo
    int demod;         // LAST only
    float exposure;
    float* rgb;
};

// One a-trous iteration, one pixel per thread, taps straight from global memory: the 64 lanes of a wavefront read 64 consecutive
// float4 of a row per tap (row-coalesced 16-byte loads), and the 25-fold reuse is served by L1 / L2.  The kernel is bound by its
// arithmetic (up to four correctly rounded divisions per tap), not by these loads: DESIGN.md section 7 has the measurements.
template <bool LAST>
__global__ __launch_bounds__(DN_TILE_X * DN_TILE_Y) void dn_iter_kernel(DnIterArgs a)
{
    const uint32_t x = blockIdx.x * DN_TILE_X + (threadIdx.x & (DN_TILE_X - 1));
    const uint32_t y = blockIdx.y * DN_TILE_Y + (threadIdx.x / DN_TILE_X);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const float4 Ap = a.ga[p];
    if (Ap.w == 0.0f) { // invalid: C' = 0, V' = -1, +0 in the image
        a.out[p] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (LAST) {
            a.rgb[3 * p] = 0.0f;
            a.rgb[3 * p + 1] = 0.0f;
            a.rgb[3 * p + 2] = 0.0f;
        }
        return;
    }
    const float4 Cp = a.in[p];
    const float4 Np = a.gn[p];
    const bool known = Cp.w >= 0.0f;
    const float Lp = dn_lum(Cp.x, Cp.y, Cp.z);
    float den = 1.0f;
    if (known) {
        // 3x3 average of V at stride 1 over the taps inside the image with V >= 0 (an invalid pixel's V is -1), row-major
        float sumVW = 0.0f, sumWt = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = (int)x + dx, qy = (int)y + dy;
                if (qx < 0 || qy < 0 || qx >= (int)a.W || qy >= (int)a.H) continue;
                const float Vq = (dx == 0 && dy == 0) ? Cp.w : a.in[(size_t)qy * a.W + qx].w;
                if (!(Vq >= 0.0f)) continue;
                const float wt = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f); // 1/4, 1/8, 1/16
                sumVW = sumVW + wt * Vq;
                sumWt = sumWt + wt;
            }
        }
        const float g = sumVW / sumWt;
        den = a.sigL * sqrtf(g) + 1e-6f;
    }
    float sumW = 0.0f, sumX = 0.0f, sumY = 0.0f, sumZ = 0.0f, sumV = 0.0f;
    const int s = a.step;
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = (int)y + dy * s;
        if (qy < 0 || qy >= (int)a.H) continue;
        const float hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
        const size_t row = (size_t)qy * a.W;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = (int)x + dx * s;
            if (qx < 0 || qx >= (int)a.W) continue;
            const float4 Aq = a.ga[row + qx];
            const float4 Cq = a.in[row + qx];
            const float4 Nq = a.gn[row + qx];
            if (Aq.w == 0.0f) continue;
            const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
            float w;
            if (dx == 0 && dy == 0) {
                w = 0.375f * 0.375f;
            } else {
                const float dn = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
                float wn = dn > 0.0f ? dn : 0.0f;
                for (uint32_t k = 0; k < a.npl2; k++) wn = wn * wn;
                const float ex = Ap.x - Aq.x, ey = Ap.y - Aq.y, ez = Ap.z - Aq.z;
                const float wa = dn_f(((ex * ex + ey * ey) + ez * ez) / a.sigA2);
                const float wl = known ? dn_f(fabsf(Lp - dn_lum(Cq.x, Cq.y, Cq.z)) / den) : 1.0f;
                w = (((hy * hx) * wn) * wa) * wl;
            }
            sumW = sumW + w;
            sumX = sumX + w * Cq.x;
            sumY = sumY + w * Cq.y;
            sumZ = sumZ + w * Cq.z;
            if (known) sumV = sumV + (w * w) * (Cq.w >= 0.0f ? Cq.w : Cp.w);
        }
    }
    const float ox = sumX / sumW, oy = sumY / sumW, oz = sumZ / sumW;
    const float ov = known ? sumV / (sumW * sumW) : -1.0f;
    a.out[p] = make_float4(ox, oy, oz, ov);
    if (LAST) {
        float dx = 1.0f, dy = 1.0f, dz = 1.0f;
        if (a.demod) {
            dx = Ap.x > 0.015625f ? Ap.x : 0.015625f;
            dy = Ap.y > 0.015625f ? Ap.y : 0.015625f;
            dz = Ap.z > 0.015625f ? Ap.z : 0.015625f;
        }
        a.rgb[3 * p] = a.exposure * (ox * dx);
        a.rgb[3 * p + 1] = a.exposure * (oy * dy);
        a.rgb[3 * p + 2] = a.exposure * (oz * dz);
    }
}

int check_params(const prt_denoise_params* d)
{
    if (d->iterations < 1 || d->iterations > 5) return fail(PRT_HIP_EINVAL, "denoise: iterations must be 1..5");
    if (d->normalPowerLog2 > 7) return fail(PRT_HIP_EINVAL, "denoise: normalPowerLog2 must be 0..7");
    if (!std::isfinite(d->sigmaLuminance) || !(d->sigmaLuminance > 0.0f))
        return fail(PRT_HIP_EINVAL, "denoise: sigmaLuminance must be finite and > 0");
    if (!std::isfinite(d->sigmaAlbedo) || !(d->sigmaAlbedo > 0.0f)) return fail(PRT_HIP_EINVAL, "denoise: sigmaAlbedo must be finite and > 0");
    if (d->demodulate > 1) return fail(PRT_HIP_EINVAL, "denoise: demodulate must be 0 or 1");
    return PRT_HIP_OK;
}

int check_guide_samples(uint32_t k)
{
    if (k != 1 && k != 2 && k != 4 && k != 8 && k != 16) return fail(PRT_HIP_EINVAL, "denoise: guideSamples must be 1, 2, 4, 8 or 16");
    return PRT_HIP_OK;
}

// The planes at the camera's size; new planes hold neither guides nor a filtered image.
int planes_ready(prt_hip_ctx* c)
{
    const size_t n = (size_t)c->cam.width * c->cam.height;
    HIP_TRY(hipSetDevice(c->device));
    bool fresh = false;
    hipError_t e = c->dnAlbedo.fit(n * 3, c->stream, &fresh);
    if (e == hipSuccess) e = c->dnNormal.fit(n * 3, c->stream, &fresh);
    for (auto* b : {&c->dnGuideA, &c->dnGuideN, &c->dnPlane[0], &c->dnPlane[1]})
        if (e == hipSuccess) e = b->fit(n, c->stream, &fresh);
    if (fresh) prt_denoise_forget(c);
    HIP_TRY(e);
    return PRT_HIP_OK;
}

uint32_t grid1d(prt_hip_ctx* c, size_t n) { return (uint32_t)std::min<size_t>((n + 255) / 256, (size_t)c->computeUnits * 16); }

} // namespace

// The guide planes a denoise with K jitters uses, on the context's stream: the host's own, or the average of K launches of the
// G-buffer kernel per plane (seed boundSeed + k), rendered when they are stale.  dnPlane[1] is the launches' target in between.
int prt_denoise_guides_ready(prt_hip_ctx* c, uint32_t K)
{
    if (!c->haveScene || !c->haveCamera) return fail(PRT_HIP_ESTATE, "upload a scene and set a camera first");
    int rc = planes_ready(c);
    if (rc) return rc;
    if (c->dnHostGuides) return PRT_HIP_OK;
    if (c->accMax == 0 || c->accClear)
        return fail(PRT_HIP_ESTATE, "denoise: the accumulator is empty, so there is no bound seed to render guides with");
    if (c->dnGuidesValid && c->dnGuideSeed == c->accSeed && c->dnGuideK == K) return PRT_HIP_OK;
    c->dnGuidesValid = false;
    const uint32_t W = c->cam.width, H = c->cam.height;
    const size_t nf = (size_t)W * H * 3;
    float* tmp = (float*)(float4*)c->dnPlane[1];
    for (int plane = 0; plane < 2; plane++) {
        float* g = plane == 0 ? c->dnAlbedo : c->dnNormal;
        for (uint32_t k = 0; k < K; k++) {
            if ((rc = prt_hip_render_gbuffer(c, 0, 0, W - 1, H - 1, plane == 0 ? 0u : 2u, c->accSeed + k, 1.0f, tmp, nullptr))) return rc;
            hipLaunchKernelGGL(dn_guide_sum_kernel, dim3(grid1d(c, nf)), dim3(256), 0, c->stream, g, (const float*)tmp, nf, k == 0 ? 1 : 0,
                               k == K - 1 ? 1 : 0, 1.0f / (float)K);
            if ((rc = prt_launched("dn_guide_sum_kernel"))) return rc;
        }
    }
    c->dnGuidesValid = true;
    c->dnGuideSeed = c->accSeed;
    c->dnGuideK = K;
    c->dnLast = -1; // dnPlane[1] was overwritten
    return PRT_HIP_OK;
}

namespace {

// Prepare + iterations on the context's stream.  tm (optional, iterations + 2 marks): before the prepare kernel and after every
// launch.
int run_filter(prt_hip_ctx* c, const prt_denoise_params* d, float exposure, float* d_rgb, StageTimer* tm)
{
    const uint32_t W = c->cam.width, H = c->cam.height;
    const size_t n = (size_t)W * H;
    hipStream_t s = c->stream;
    const float4* mom = (c->accMom.size() == n && !c->momClear) ? c->accMom : nullptr;
    int rc;
    if (tm) HIP_TRY(tm->mark(s));
    hipLaunchKernelGGL(dn_prepare_kernel, dim3(grid1d(c, n)), dim3(256), 0, s, (const float4*)c->accSum, mom, (const float*)c->dnAlbedo,
                       (const float*)c->dnNormal, n, (int)d->demodulate, c->dnPlane[0], c->dnGuideA, c->dnGuideN);
    if ((rc = prt_launched("dn_prepare_kernel"))) return rc;
    if (tm) HIP_TRY(tm->mark(s));
    return prt_denoise_iterations(c, d, exposure, d_rgb, tm);
}

} // namespace

// The iterations on dnPlane[0] (what a prepare step left there) into d_rgb.  tm (optional, `iterations` marks): one after every launch.
int prt_denoise_iterations(prt_hip_ctx* c, const prt_denoise_params* d, float exposure, float* d_rgb, StageTimer* tm)
{
    const uint32_t W = c->cam.width, H = c->cam.height;
    hipStream_t s = c->stream;
    int rc;
    const dim3 grid((W + DN_TILE_X - 1) / DN_TILE_X, (H + DN_TILE_Y - 1) / DN_TILE_Y);
    int cur = 0;
    for (uint32_t i = 0; i < d->iterations; i++) {
        DnIterArgs A{c->dnPlane[cur], c->dnPlane[cur ^ 1], c->dnGuideA, c->dnGuideN, W, H, 1 << i, d->normalPowerLog2, d->sigmaLuminance,
                     d->sigmaAlbedo * d->sigmaAlbedo, (int)d->demodulate, exposure, d_rgb};
        if (i + 1 == d->iterations)
            hipLaunchKernelGGL(dn_iter_kernel<true>, grid, dim3(DN_TILE_X * DN_TILE_Y), 0, s, A);
        else
            hipLaunchKernelGGL(dn_iter_kernel<false>, grid, dim3(DN_TILE_X * DN_TILE_Y), 0, s, A);
        if ((rc = prt_launched("dn_iter_kernel"))) return rc;
        if (tm) HIP_TRY(tm->mark(s));
        cur ^= 1;
    }
    c->dnLast = cur;
    return PRT_HIP_OK;
}

int prt_denoise_checks(prt_hip_ctx* c, const prt_denoise_params* d)
{
    if (!c || !d) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = check_params(d);
    if (rc) return rc;
    if ((rc = check_guide_samples(d->guideSamples))) return rc;
    if (!c->haveScene || !c->haveCamera) return fail(PRT_HIP_ESTATE, "upload a scene and set a camera first");
    if (c->accMax == 0 || c->accClear || !c->accSum || c->accSum.size() != (size_t)c->cam.width * c->cam.height)
        return fail(PRT_HIP_ESTATE, "denoise: the accumulator is empty (render or import samples first)");
    if (c->cam.width > 65535 || c->cam.height > 65535) return fail(PRT_HIP_EINVAL, "image too large");
    return PRT_HIP_OK;
}

void prt_denoise_forget(prt_hip_ctx* c)
{
    c->dnGuidesValid = false;
    c->dnHostGuides = false;
    c->dnLast = -1;
}

extern "C" {

int prt_hip_denoise_set_guides(prt_hip_ctx* c, const float* albedo, const float* normal)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!albedo && !normal) { // back to the library's own, rendered by the next denoise
        c->dnHostGuides = false;
        c->dnGuidesValid = false;
        return PRT_HIP_OK;
    }
    if (!albedo || !normal) return fail(PRT_HIP_EINVAL, "denoise_set_guides: both planes or neither");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    int rc = planes_ready(c);
    if (rc) return rc;
    const size_t bytes = c->dnAlbedo.size() * sizeof(float);
    HIP_TRY(hipStreamSynchronize(c->stream)); // a denoise may still be reading the old planes
    HIP_TRY(hipMemcpy(c->dnAlbedo, albedo, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->dnNormal, normal, bytes, hipMemcpyHostToDevice));
    c->dnHostGuides = true;
    c->dnGuidesValid = false;
    return PRT_HIP_OK;
}

int prt_hip_denoise_get_guides(prt_hip_ctx* c, uint32_t guideSamples, float* albedo, float* normal)
{
    if (!c || !albedo || !normal) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = check_guide_samples(guideSamples);
    if (rc) return rc;
    if ((rc = prt_denoise_guides_ready(c, guideSamples))) return rc;
    const size_t bytes = c->dnAlbedo.size() * sizeof(float);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(albedo, c->dnAlbedo, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(normal, c->dnNormal, bytes, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_accum_denoise(prt_hip_ctx* c, const prt_denoise_params* d, float exposure, float* d_rgb, void* stream)
{
    int rc = prt_denoise_checks(c, d);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = prt_denoise_guides_ready(c, d->guideSamples)) || (rc = prt_own_framebuffer(c, &d_rgb)) ||
        (rc = run_filter(c, d, exposure, d_rgb, nullptr)))
        return rc;
    return prt_stream_leave(c, caller);
}

int prt_hip_denoise_variance(prt_hip_ctx* c, float* var)
{
    if (!c || !var) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    const size_t n = (size_t)c->cam.width * c->cam.height;
    if (c->dnLast < 0 || c->dnPlane[0].size() != n) return fail(PRT_HIP_ESTATE, "denoise_variance: no denoise of this view yet");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float4> h(n);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(h.data(), c->dnPlane[c->dnLast], n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) var[i] = h[i].w;
    return PRT_HIP_OK;
}

} // extern "C"

#ifdef PRT_TEST_ENTRY_POINTS
namespace {

// The yardstick of tools/denoise_bench.py: every thread reads one element of each input plane and writes one of each output plane
// (16-byte planes as float4, 12-byte planes as three floats, as the filter's kernels access them); the inputs are summed so
// that no load can be dropped.
struct CopyArgs {
    const float4* r16[6];
    const float* r12[2];
    float4* w16[6];
    float* w12;
    int nr16, nr12, nw16, nw12;
    size_t n;
};
__global__ __launch_bounds__(256) void dn_copy_kernel(CopyArgs a)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (size_t)gridDim.x * 256) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = 0; k < a.nr16; k++) {
            const float4 t = a.r16[k][i];
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        for (int k = 0; k < a.nr12; k++) {
            v.x += a.r12[k][3 * i]; v.y += a.r12[k][3 * i + 1]; v.z += a.r12[k][3 * i + 2];
        }
        for (int k = 0; k < a.nw16; k++) a.w16[k][i] = v;
        if (a.nw12) {
            a.w12[3 * i] = v.x; a.w12[3 * i + 1] = v.y; a.w12[3 * i + 2] = v.z;
        }
    }
}

} // namespace

extern "C" {

int prt_hip_test_denoise_profile(prt_hip_ctx* c, const prt_denoise_params* d, float exposure, float* ms)
{
    if (!ms) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = prt_denoise_checks(c, d);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    float* rgb = nullptr;
    if ((rc = prt_denoise_guides_ready(c, d->guideSamples)) || (rc = prt_own_framebuffer(c, &rgb))) return rc;
    // the whole filter between two events, then the same again with an event after every launch
    StageTimer whole(1), each(d->iterations + 1);
    HIP_TRY(whole.mark(c->stream));
    if ((rc = run_filter(c, d, exposure, rgb, nullptr))) return rc;
    HIP_TRY(whole.mark(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(whole.lap());
    HIP_TRY(whole.median(0, &ms[6]));
    if ((rc = run_filter(c, d, exposure, rgb, &each))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(each.lap());
    for (uint32_t k = 0; k < 6; k++) ms[k] = 0.0f;
    for (uint32_t k = 0; k <= d->iterations; k++) HIP_TRY(each.median(k, &ms[k]));
    return PRT_HIP_OK;
}

int prt_hip_test_copy_yardstick(prt_hip_ctx* c, uint64_t pixels, int read16, int read12, int write16, int write12, float* ms)
{
    if (!c || !ms || pixels == 0) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (read16 < 0 || read16 > 6 || read12 < 0 || read12 > 2 || write16 < 0 || write16 > 6 || write12 < 0 || write12 > 1)
        return fail(PRT_HIP_EINVAL, "copy_yardstick: at most 6 + 2 input and 6 + 1 output planes");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)pixels;
    const size_t bytes = n * (size_t)(16 * (read16 + write16) + 12 * (read12 + write12));
    DevBuf<char> buf;
    HIP_TRY(buf.fit(bytes, c->stream));
    HIP_TRY(hipMemsetAsync(buf, 0, bytes, c->stream));
    CopyArgs A{};
    char* q = buf;
    for (int k = 0; k < read16; k++, q += n * 16) A.r16[k] = (const float4*)q;
    for (int k = 0; k < write16; k++, q += n * 16) A.w16[k] = (float4*)q;
    for (int k = 0; k < read12; k++, q += n * 12) A.r12[k] = (const float*)q;
    if (write12) A.w12 = (float*)q;
    A.nr16 = read16; A.nr12 = read12; A.nw16 = write16; A.nw12 = write12; A.n = n;
    StageTimer tm(1);
    hipLaunchKernelGGL(dn_copy_kernel, dim3(grid1d(c, n)), dim3(256), 0, c->stream, A); // warm-up
    HIP_TRY(tm.mark(c->stream));
    hipLaunchKernelGGL(dn_copy_kernel, dim3(grid1d(c, n)), dim3(256), 0, c->stream, A);
    HIP_TRY(tm.mark(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(tm.lap());
    HIP_TRY(tm.median(0, ms));
    return prt_launched("dn_copy_kernel");
}

} // extern "C"
#endif // PRT_TEST_ENTRY_POINTS
