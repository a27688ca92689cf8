// prt_display.h -- the arithmetic of the display transform (include/prt_hip.h "display transform"), in ONE text that the kernels of
// prt_display.hip run on the device and prt_hip_test_display_host runs on the host: the luminance bin of the meter, the resolve of a
// histogram into the adaptation state, and the byte of one channel.  All of it is f32 without FMA (the build's -ffp-contract=off),
// with correctly rounded /, subnormals kept, in the order written; the only transcendental is powf, which is glibc's algorithm as
// prt_devmath.h restates it (double precision inside, so the device needs no libm).
#pragma once
#include <math.h>

#include "../../include/prt_hip.h"
#include "prt_devmath.h"

#define PRT_DISPLAY_BINS 256

// lum(c), left to right as in the denoiser
PRT_HD float prt_display_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The meter's bin of a luminance, or -1 for a pixel that is not counted (NaN, +-0, negative).  8 bins per octave from 2^-16: the
// exponent and the top three mantissa bits, a piecewise-linear log2; +inf and everything from 1.875 * 2^15 fall in bin 255.
PRT_HD int32_t prt_display_bin(float lum)
{
    if (!(lum > 0.0f)) return -1;
    const int32_t k = (int32_t)(prt_f2u(lum) >> 20) - 888;
    return k < 0 ? 0 : (k > PRT_DISPLAY_BINS - 1 ? PRT_DISPLAY_BINS - 1 : k);
}

// One metering's histogram (integers: exact whatever the order of the atomics that made it) into the adaptation state.  With an
// empty histogram the WHOLE record stays as it is, the last metering's figures included.
PRT_HD void prt_display_resolve(const uint32_t* hist, uint64_t ignored, const prt_display_params* p, prt_display_state* s)
{
    uint64_t N = 0;
    for (int k = 0; k < PRT_DISPLAY_BINS; k++) N += hist[k];
    if (N == 0) return;
    const uint64_t rlo = (uint64_t)p->lowPermille * N / 1000u, rhi = ((uint64_t)p->highPermille * N + 999u) / 1000u;
    uint64_t cum = 0, Nb = 0, S = 0;
    for (int k = 0; k < PRT_DISPLAY_BINS; k++) { // the pixels of rank [rlo, rhi) in the order of their bins
        const uint64_t a = cum > rlo ? cum : rlo, end = cum + hist[k], b = end < rhi ? end : rhi;
        if (b > a) {
            Nb += b - a;
            S += (b - a) * (uint64_t)(2 * k + 1);
        }
        cum = end;
    }
    const float m = (float)S / (float)Nb;           // mean of 2k + 1: twice the bin centre, Nb >= 1 since low < high
    const float octaves = m * 0.0625f - 16.0f;      // above 2^0
    const float i = floorf(octaves), f = octaves - i;
    const float two = prt_u2f((uint32_t)((int32_t)i + 127) << 23);
    const float L = (1.0f + f) * two;               // the inverse of the binning's log
    const float t = p->key / L;
    const float target = fminf(fmaxf(t, p->minGain), p->maxGain);
    s->gain = (s->valid && p->adaptRate < 1.0f) ? s->gain + (target - s->gain) * p->adaptRate : target;
    s->valid = 1u;
    s->octaves = octaves;
    s->target = target;
    s->metered = N;
    s->ignored = ignored;
    for (int k = 0; k < PRT_DISPLAY_BINS; k++) s->hist[k] = hist[k];
}

// The byte of one channel `in` under the gain g.  The clamp is fminf(fmaxf(x, 0.0f), 1.0f) written out, so that NaN becomes 0 on
// every target (+inf through the tone map is inf / inf = NaN and becomes 0 too: the reference's own behaviour, image.cpp:64).
PRT_HD uint8_t prt_display_byte(float in, float g, uint32_t tonemap, uint32_t transfer)
{
    float x = g * in;
    if (tonemap) x = x / (x + 1.0f);
    x = x > 0.0f ? x : 0.0f;
    x = x < 1.0f ? x : 1.0f;
    if (transfer == 0) return (uint8_t)(prt_powf_pos(x, 1 / 2.2f) * 255.0f); // image.cpp:65, truncated
    const float s = x <= 0.0031308f ? 12.92f * x : 1.055f * prt_powf_pos(x, 1 / 2.4f) - 0.055f;
    return (uint8_t)(s * 255.0f + 0.5f);
}

PRT_HD uint32_t prt_display_bpp(uint32_t format) { return format == 0 ? 3u : 4u; }

// The bytes of one pixel in `format` (0 RGB8, 1 RGBA8, 2 BGRA8; a = 255) as a little-endian word: byte k of the pixel is bits 8k..8k+7.
PRT_HD uint32_t prt_display_pixel(float r, float g, float b, float gain, const prt_display_params* p)
{
    const uint32_t R = prt_display_byte(r, gain, p->tonemap, p->transfer), G = prt_display_byte(g, gain, p->tonemap, p->transfer),
                   B = prt_display_byte(b, gain, p->tonemap, p->transfer);
    if (p->format == 0) return R | (G << 8) | (B << 16);
    if (p->format == 1) return R | (G << 8) | (B << 16) | 0xff000000u;
    return B | (G << 8) | (R << 16) | 0xff000000u;
}

// The field of *p that is out of its range or not finite, or NULL when every field is acceptable.
static inline const char* prt_display_bad_field(const prt_display_params* p)
{
    const auto finite = [](float v) { return (prt_f2u(v) & 0x7f800000u) != 0x7f800000u; };
    if (p->tonemap > 1) return "tonemap";
    if (p->transfer > 1) return "transfer";
    if (p->format > 2) return "format";
    if (p->meter > 1) return "meter";
    if (!finite(p->gain) || !(p->gain >= 0.0f)) return "gain";
    if (p->meter == 0) return nullptr;
    if (!finite(p->key) || !(p->key > 0.0f)) return "key";
    if (p->lowPermille >= 1000) return "lowPermille";
    if (p->highPermille > 1000 || p->highPermille <= p->lowPermille) return "highPermille";
    if (!finite(p->minGain) || !(p->minGain > 0.0f)) return "minGain";
    if (!finite(p->maxGain) || !(p->maxGain >= p->minGain)) return "maxGain";
    if (!finite(p->adaptRate) || !(p->adaptRate > 0.0f) || p->adaptRate > 1.0f) return "adaptRate";
    return nullptr;
}
