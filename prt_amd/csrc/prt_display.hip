// prt_display.hip -- the display transform (include/prt_hip.h "display transform"): a float RGB image of the camera's size becomes
// 8-bit display-referred pixels on the device, under a manual gain or under an exposure metered from the image's own luminance
// histogram.  Three kernels -- histogram, resolve, transform -- whose arithmetic is prt_display.h, the text the host check runs too.
// A translation unit of its own: no kernel of another file moves when it changes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "prt_internal.h"

#include "prt_display.h"
#ifdef PRT_TEST_ENTRY_POINTS
#include "../../include/prt_hip_test.h"
#endif

namespace {
int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define DP_BLOCK 256
static_assert(DP_BLOCK == PRT_DISPLAY_BINS, "the flush of the histogram kernel gives every thread one bin");
#define DP_HIST_WORDS (PRT_DISPLAY_BINS + 2) // the bins, then the ignored count as 64 bits (8-byte aligned: 256 words in)

// The rectangle as the kernels see it: `rows` spans of `span` pixels, span r starting at linear pixel index first + r * pitch.  A
// rectangle as wide as the image is ONE span (its rows are contiguous), so that no row ends in a partly used block.
struct DpRect {
    uint64_t first, pitch;
    uint32_t span, rows;
    uint32_t chunks; // blocks per span
};

// Metering: one pixel per thread, a block per DP_BLOCK pixels of a span, grid-stride over those work items.  Each wave counts into
// an LDS histogram of its own (LDS atomics of one wave contend only with themselves); pixels outside the histogram are counted
// by a ballot, one add per wave; the block's four histograms are flushed with one global atomic per non-empty bin.
__global__ __launch_bounds__(DP_BLOCK) void display_hist_kernel(const float* __restrict__ in, DpRect R, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t lh[DP_BLOCK / 64][PRT_DISPLAY_BINS];
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t k = threadIdx.x; k < (DP_BLOCK / 64) * PRT_DISPLAY_BINS; k += DP_BLOCK) (&lh[0][0])[k] = 0u;
    __syncthreads();
    uint32_t ignored = 0; // of the wave, kept by every lane
    const uint64_t items = (uint64_t)R.rows * R.chunks;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t row = item / R.chunks;
        const uint32_t x = (uint32_t)(item - row * R.chunks) * DP_BLOCK + threadIdx.x;
        bool out = false;
        if (x < R.span) {
            const float* px = in + (R.first + row * R.pitch + x) * 3;
            const int32_t k = prt_display_bin(prt_display_lum(px[0], px[1], px[2]));
            if (k >= 0) atomicAdd(&lh[wave][k], 1u);
            out = k < 0;
        }
        ignored += (uint32_t)__popcll(__ballot(out));
    }
    __syncthreads();
    uint32_t n = 0;
    for (uint32_t w = 0; w < DP_BLOCK / 64; w++) n += lh[w][threadIdx.x];
    if (n) atomicAdd(&hist[threadIdx.x], n);
    if ((threadIdx.x & 63u) == 0 && ignored) atomicAdd((unsigned long long*)(hist + PRT_DISPLAY_BINS), (unsigned long long)ignored);
}

// One wave; its first lane walks the 256 bins and writes the state record.
__global__ __launch_bounds__(64) void display_resolve_kernel(const uint32_t* __restrict__ hist, prt_display_params p, prt_display_state* state)
{
    if (threadIdx.x == 0) prt_display_resolve(hist, *(const unsigned long long*)(hist + PRT_DISPLAY_BINS), &p, state);
}

// Transform: a thread owns one ALIGNED group of four consecutive pixels (linear pixel index 4q .. 4q + 3: 48 bytes in at a multiple
// of 48, 12 or 16 bytes out at a multiple of 12 or 16).  A group that lies wholly inside the span moves as three 16-byte loads and
// three dword stores (RGB8) or one 16-byte store; a group cut by the span's ends, and every group when a base pointer is not
// 16-byte aligned (vec = 0), goes pixel by pixel.  A block covers DP_BLOCK groups of a span; grid-stride over those work items.
__global__ __launch_bounds__(DP_BLOCK) void display_transform_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, DpRect R,
                                                                     prt_display_params p, const prt_display_state* __restrict__ state, uint32_t vec)
{
    const float g = p.meter ? p.gain * state->gain : p.gain;
    const uint64_t items = (uint64_t)R.rows * R.chunks;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t row = item / R.chunks;
        const uint64_t first = R.first + row * R.pitch, last = first + (R.span - 1);
        const uint64_t p0 = ((first >> 2) + (item - row * R.chunks) * DP_BLOCK + threadIdx.x) << 2;
        if (p0 > last) continue;
        if (vec && p0 >= first && p0 + 3 <= last) {
            const float4* src = (const float4*)(in + p0 * 3);
            const float4 a = src[0], b = src[1], c = src[2];
            const uint32_t w0 = prt_display_pixel(a.x, a.y, a.z, g, &p), w1 = prt_display_pixel(a.w, b.x, b.y, g, &p),
                           w2 = prt_display_pixel(b.z, b.w, c.x, g, &p), w3 = prt_display_pixel(c.y, c.z, c.w, g, &p);
            if (p.format == 0) {
                uint32_t* dst = (uint32_t*)(out + p0 * 3);
                dst[0] = w0 | (w1 << 24);
                dst[1] = (w1 >> 8) | (w2 << 16);
                dst[2] = (w2 >> 16) | (w3 << 8);
            } else {
                *(uint4*)(out + p0 * 4) = make_uint4(w0, w1, w2, w3);
            }
        } else {
            for (uint32_t k = 0; k < 4; k++) {
                const uint64_t q = p0 + k;
                if (q < first || q > last) continue;
                const float* px = in + q * 3;
                const uint32_t w = prt_display_pixel(px[0], px[1], px[2], g, &p);
                if (p.format == 0) {
                    uint8_t* dst = out + q * 3;
                    dst[0] = (uint8_t)w;
                    dst[1] = (uint8_t)(w >> 8);
                    dst[2] = (uint8_t)(w >> 16);
                } else {
                    *(uint32_t*)(out + q * 4) = w; // 4-byte aligned whenever the base is (checked by the host)
                }
            }
        }
    }
}

DpRect dp_rect(uint32_t W, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t perBlock, bool groups)
{
    DpRect R;
    R.first = (uint64_t)y0 * W + x0;
    R.pitch = W;
    R.span = x1 - x0 + 1;
    R.rows = y1 - y0 + 1;
    if (R.span == W && (uint64_t)W * R.rows <= 0xffffffffull) { // contiguous rows: one span
        R.span = W * R.rows;
        R.rows = 1;
    }
    // a span of n pixels touches at most (n - 1) / 4 + 2 aligned groups of four
    const uint64_t units = groups ? (uint64_t)(R.span - 1) / 4 + 2 : R.span;
    R.chunks = (uint32_t)((units + perBlock - 1) / perBlock);
    return R;
}

int dp_check(const prt_hip_ctx* c, const prt_display_params* p, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (!c || !p) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    if (const char* bad = prt_display_bad_field(p)) return fail(PRT_HIP_EINVAL, std::string("display: ") + bad + " is outside its range or not finite");
    return prt_check_rect(c, x0, y0, x1, y1);
}

// state and histogram, zeroed (valid = 0) on the context's stream when they are first needed
int dp_state_ready(prt_hip_ctx* c)
{
    bool fresh = false;
    HIP_TRY(c->dpHist.fit(DP_HIST_WORDS, c->stream));
    HIP_TRY(c->dpState.fit(1, c->stream, &fresh));
    if (fresh) HIP_TRY(hipMemsetAsync(c->dpState, 0, sizeof(prt_display_state), c->stream));
    return PRT_HIP_OK;
}

// The context's display buffer for the camera's image in `format`: reallocated (and cleared) when it has to grow.
int dp_own_buffer(prt_hip_ctx* c, uint32_t format, uint8_t** d_out)
{
    const size_t bytes = (size_t)c->cam.width * c->cam.height * prt_display_bpp(format);
    bool fresh = false;
    HIP_TRY(c->dpOut.grow(bytes, c->stream, &fresh));
    if (fresh) HIP_TRY(hipMemsetAsync(c->dpOut, 0, bytes, c->stream));
    c->dpOutW = c->cam.width;
    c->dpOutH = c->cam.height;
    c->dpOutFormat = format;
    *d_out = c->dpOut;
    return PRT_HIP_OK;
}

// The launches of one display on the context's stream; tm (optional, 4 marks): before the metering, after the histogram, after the
// resolve, after the transform (without metering the first three follow one another).
int dp_queue(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_display_params* p, const float* d_rgb, uint8_t* d_out,
             StageTimer* tm)
{
    int rc;
    hipStream_t s = c->stream;
    const uint32_t W = c->cam.width;
    if (tm) HIP_TRY(tm->mark(s));
    if (p->meter) {
        const DpRect R = dp_rect(W, x0, y0, x1, y1, DP_BLOCK, false);
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)R.rows * R.chunks, (uint64_t)c->computeUnits * 8);
        HIP_TRY(hipMemsetAsync(c->dpHist, 0, DP_HIST_WORDS * sizeof(uint32_t), s));
        hipLaunchKernelGGL(display_hist_kernel, dim3(blocks), dim3(DP_BLOCK), 0, s, d_rgb, R, c->dpHist);
        if ((rc = prt_launched("display_hist_kernel"))) return rc;
        if (tm) HIP_TRY(tm->mark(s));
        hipLaunchKernelGGL(display_resolve_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)c->dpHist, *p, c->dpState);
        if ((rc = prt_launched("display_resolve_kernel"))) return rc;
    } else if (tm) {
        HIP_TRY(tm->mark(s));
    }
    if (tm) HIP_TRY(tm->mark(s));
    const DpRect R = dp_rect(W, x0, y0, x1, y1, DP_BLOCK, true);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)R.rows * R.chunks, (uint64_t)c->computeUnits * 4);
    const uint32_t vec = ((uintptr_t)d_rgb % 16 == 0 && (uintptr_t)d_out % 16 == 0) ? 1u : 0u;
    hipLaunchKernelGGL(display_transform_kernel, dim3(blocks), dim3(DP_BLOCK), 0, s, d_rgb, d_out, R, *p, (const prt_display_state*)c->dpState, vec);
    if ((rc = prt_launched("display_transform_kernel"))) return rc;
    if (tm) HIP_TRY(tm->mark(s));
    return PRT_HIP_OK;
}
} // namespace

extern "C" {

int prt_hip_display(prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_display_params* p, const float* d_rgb,
                    uint8_t* d_out, void* stream)
{
    int rc = dp_check(c, p, x0, y0, x1, y1);
    if (rc) return rc;
    if (d_out && p->format != 0 && (uintptr_t)d_out % 4 != 0) return fail(PRT_HIP_EINVAL, "display: d_out of a 4-byte format must be 4-byte aligned");
    if (d_rgb && (uintptr_t)d_rgb % 4 != 0) return fail(PRT_HIP_EINVAL, "display: d_rgb must be 4-byte aligned");
    if (!d_rgb && !c->fb) return fail(PRT_HIP_ESTATE, "display: nothing rendered or uploaded into the context framebuffer");
    if (!d_rgb && c->fb.size() != (size_t)c->cam.width * c->cam.height * 3)
        return fail(PRT_HIP_ESTATE, "display: the context framebuffer holds an image of another camera's size");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = dp_state_ready(c))) return rc;
    if (!d_rgb) d_rgb = c->fb;
    if (!d_out && (rc = dp_own_buffer(c, p->format, &d_out))) return rc;
    if ((rc = dp_queue(c, x0, y0, x1, y1, p, d_rgb, d_out, nullptr))) return rc;
    return prt_stream_leave(c, caller);
}

int prt_hip_download_display(prt_hip_ctx* c, uint8_t* out_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (!c || !out_host) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    if (!c->dpOut || c->dpOutW != c->cam.width || c->dpOutH != c->cam.height)
        return fail(PRT_HIP_ESTATE, "nothing displayed into the context's display buffer at the camera's size");
    int rc = prt_check_rect(c, x0, y0, x1, y1);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t bpp = prt_display_bpp(c->dpOutFormat), pitch = (size_t)c->cam.width * bpp;
    const size_t off = ((size_t)y0 * c->cam.width + x0) * bpp;
    HIP_TRY(hipMemcpy2D(out_host + off, pitch, c->dpOut + off, pitch, (size_t)(x1 - x0 + 1) * bpp, y1 - y0 + 1, hipMemcpyDeviceToHost));
    return prt_sticky_error(c, false); // as prt_hip_download: reported, not cleared
}

int prt_hip_display_get_state(prt_hip_ctx* c, prt_display_state* out)
{
    if (!c || !out) return fail(PRT_HIP_EINVAL, "NULL argument");
    memset(out, 0, sizeof(*out));
    if (!c->dpState) return PRT_HIP_OK; // never displayed: valid = 0
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->dpState, sizeof(*out), hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_display_reset(prt_hip_ctx* c)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->dpState) return PRT_HIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    // valid = 0, ordered after the displays queued so far: the gain and the last metering's figures stay readable
    HIP_TRY(hipMemsetAsync(&c->dpState->valid, 0, sizeof(uint32_t), c->stream));
    return PRT_HIP_OK;
}

#ifdef PRT_TEST_ENTRY_POINTS
int prt_hip_test_display_host(uint32_t width, uint32_t height, const float* rgb, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                              const prt_display_params* p, prt_display_state* state, uint8_t* out)
{
    if (!rgb || !p || !state || !out || width == 0 || height == 0) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (const char* bad = prt_display_bad_field(p)) return fail(PRT_HIP_EINVAL, std::string("display: ") + bad + " is outside its range or not finite");
    if (x1 < x0 || y1 < y0 || x1 >= width || y1 >= height) return fail(PRT_HIP_EINVAL, "pixel rectangle outside the image");
    if (p->meter) {
        uint32_t hist[PRT_DISPLAY_BINS] = {0};
        uint64_t ignored = 0;
        for (uint32_t y = y0; y <= y1; y++)
            for (uint32_t x = x0; x <= x1; x++) {
                const float* px = rgb + ((size_t)y * width + x) * 3;
                const int32_t k = prt_display_bin(prt_display_lum(px[0], px[1], px[2]));
                if (k >= 0) hist[k]++;
                else ignored++;
            }
        prt_display_resolve(hist, ignored, p, state);
    }
    const float g = p->meter ? p->gain * state->gain : p->gain;
    const uint32_t bpp = prt_display_bpp(p->format);
    for (uint32_t y = y0; y <= y1; y++)
        for (uint32_t x = x0; x <= x1; x++) {
            const size_t q = (size_t)y * width + x;
            const uint32_t w = prt_display_pixel(rgb[3 * q], rgb[3 * q + 1], rgb[3 * q + 2], g, p);
            for (uint32_t k = 0; k < bpp; k++) out[q * bpp + k] = (uint8_t)(w >> (8 * k));
        }
    return PRT_HIP_OK;
}

// tools/display_bench.py: `reps` displays of the whole framebuffer into the context's display buffer with an event around every
// kernel; medians.  The adaptation state advances as by `reps` displays.
int prt_hip_test_display_profile(prt_hip_ctx* c, const prt_display_params* p, uint32_t reps, float* ms3)
{
    if (!ms3 || reps == 0) return fail(PRT_HIP_EINVAL, "NULL argument");
    int rc = dp_check(c, p, 0, 0, 0, 0);
    if (rc) return rc;
    if (!c->fb || c->fb.size() != (size_t)c->cam.width * c->cam.height * 3) return fail(PRT_HIP_ESTATE, "display profile: render or upload an image first");
    HIP_TRY(hipSetDevice(c->device));
    uint8_t* d_out = nullptr;
    if ((rc = dp_state_ready(c)) || (rc = dp_own_buffer(c, p->format, &d_out))) return rc;
    StageTimer tm(3);
    for (uint32_t r = 0; r <= reps; r++) { // the first is the warm-up
        if ((rc = dp_queue(c, 0, 0, c->cam.width - 1, c->cam.height - 1, p, c->fb, d_out, &tm))) return rc;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(PRT_HIP_ELAUNCH, "display profile: synchronise failed");
        HIP_TRY(tm.lap(r == 0));
    }
    for (uint32_t k = 0; k < 3; k++) HIP_TRY(tm.median(k, &ms3[k]));
    if (!p->meter) ms3[0] = ms3[1] = 0.0f;
    return PRT_HIP_OK;
}
#endif

} // extern "C"
