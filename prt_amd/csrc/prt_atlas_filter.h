// prt_atlas_filter.h -- the arithmetic of the lightmap filter (include/prt_hip.h "lightmap filter"), in ONE text that the kernels of
// prt_atlas_filter.hip run on the device and tests/atlas_filter_main.cpp runs on the host: eligibility, the footprint and the variance
// of a point, the geometric weight of a tap and one a-trous iteration of a point.  All of it is f32 without FMA (the build's
// -ffp-contract=off), every product rounded before the sum that uses it, sums left to right as written, sqrtf and / correctly rounded.
// Every operation is the header's, in the header's order: the tests compare the output with a numpy restatement of that text at
// tolerance 0, so nothing here may be reassociated or "simplified".  The tap loops are unrolled in full: the per-tap arrays are
// registers, not scratch memory.
#pragma once
#include <math.h>

#include "../../include/prt_hip.h"
#include "prt_devmath.h"

#define PRT_AF_NONE 0xffffffffu // map: no placed point at the texel (no q reaches it: n <= 2^26)

// 16 bytes moved as one: half a prt_bake_point ({P, bias}, {N, set}), or the record of a point
struct alignas(16) PrtAfQuad {
    float x, y, z, w;
};
PRT_HD PrtAfQuad prt_af_ld4(const void* p)
{
    PrtAfQuad q;
    __builtin_memcpy(&q, __builtin_assume_aligned(p, 16), 16);
    return q;
}
PRT_HD void prt_af_st4(void* p, PrtAfQuad q) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &q, 16); }

// What the three kernels share; the last block changes per iteration.
struct PrtAfArgs {
    uint32_t W, H, n, stride;
    const uint32_t* texels;
    const prt_bake_point* points; // 16-byte aligned
    const float* values;
    uint32_t* map;  // W*H: the smallest eligible q per texel, PRT_AF_NONE before the index kernel
    PrtAfQuad* rec; // per point {bits(placed ? 1 : 0), f2, V0, 0}
    uint32_t npl2;
    float sigL, sigP2; // sigmaLuminance, sigmaPosition * sigmaPosition
    // one iteration
    uint32_t step;
    const float* cin;   // n*stride: values in the first launch, a plane afterwards
    const float* vin;   // V of point r at vin[r * vinStride]: the records' V0 in the first launch (4), a plane afterwards (1)
    uint32_t vinStride;
    float* cout;        // n*stride: a plane, or out in the last launch
    float* vout;        // n (not written by the last launch)
};

PRT_HD bool prt_af_finite(float v) { return (prt_f2u(v) & 0x7f800000u) != 0x7f800000u; }
PRT_HD float prt_af_lum(const float* v) { return (0.2126f * v[0] + 0.7152f * v[1]) + 0.0722f * v[2]; }
// f(x): the eighth power of 1 / (1 + y + y*y/2), y = x/8 (dn_f of prt_denoise.hip)
PRT_HD float prt_af_f(float x)
{
    const float y = 0.125f * x;
    float r = 1.0f / ((1.0f + y) + (0.5f * y) * y);
    r = r * r;
    r = r * r;
    r = r * r;
    return r;
}
PRT_HD float prt_af_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

PRT_HD bool prt_af_eligible(const PrtAfArgs& A, uint32_t q)
{
    if (A.texels[q] >= A.W * A.H) return false;
    const PrtAfQuad P = prt_af_ld4(A.points + q), N = prt_af_ld4((const char*)(A.points + q) + 16);
    if (prt_f2u(N.w) == 0xffffffffu) return false;
    bool ok = prt_af_finite(P.x) && prt_af_finite(P.y) && prt_af_finite(P.z) && prt_af_finite(N.x) && prt_af_finite(N.y) && prt_af_finite(N.z);
    const float* v = A.values + (size_t)q * A.stride;
    for (uint32_t j = 0; j < A.stride; j++) ok = ok && prt_af_finite(v[j]);
    return ok;
}

// The placed point at texel (x + dx, y + dy), or PRT_AF_NONE
PRT_HD uint32_t prt_af_nb(const PrtAfArgs& A, int x, int y, int dx, int dy)
{
    const int nx = x + dx, ny = y + dy;
    if (nx < 0 || ny < 0 || nx >= (int)A.W || ny >= (int)A.H) return PRT_AF_NONE;
    return A.map[(size_t)ny * A.W + (uint32_t)nx];
}

PRT_HD float prt_af_d2(const PrtAfQuad& Pq, const PrtAfQuad& Pr)
{
    const float ex = Pr.x - Pq.x, ey = Pr.y - Pq.y, ez = Pr.z - Pq.z;
    return (ex * ex + ey * ey) + ez * ez;
}

// geo(q, r, s); invP carries s and f2_q
PRT_HD float prt_af_geo(const PrtAfQuad& Pq, const PrtAfQuad& Nq, const PrtAfQuad& Pr, const PrtAfQuad& Nr, float invP, uint32_t npl2)
{
    const float dn = (Nq.x * Nr.x + Nq.y * Nr.y) + Nq.z * Nr.z;
    float wn = dn > 0.0f ? dn : 0.0f;
    for (uint32_t k = 0; k < npl2; k++) wn = wn * wn;
    const float d2 = prt_af_d2(Pq, Pr);
    const float wp = d2 == 0.0f ? 1.0f : prt_af_f(d2 * invP);
    return wn * wp;
}

PRT_HD float prt_af_inv_p(const PrtAfArgs& A, uint32_t s, float f2) { return 1.0f / ((A.sigP2 * (float)(s * s)) * f2); }

// The record of point q: placed, f2 and V0.  The map is complete.
PRT_HD void prt_af_prepare(const PrtAfArgs& A, uint32_t q)
{
    const uint32_t t = A.texels[q];
    if (t >= A.W * A.H || A.map[t] != q) { // (the map holds eligible points only)
        prt_af_st4(A.rec + q, PrtAfQuad{0.0f, 0.0f, 0.0f, 0.0f});
        return;
    }
    const int x = (int)(t % A.W), y = (int)(t / A.W);
    const PrtAfQuad Pq = prt_af_ld4(A.points + q), Nq = prt_af_ld4((const char*)(A.points + q) + 16);
    float f2 = INFINITY;
    bool taken = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t r = prt_af_nb(A, x, y, k == 0 ? -1 : (k == 1 ? 1 : 0), k == 2 ? -1 : (k == 3 ? 1 : 0));
        if (r == PRT_AF_NONE) continue;
        const float d2 = prt_af_d2(Pq, prt_af_ld4(A.points + r));
        if (d2 > 0.0f && d2 < f2) {
            f2 = d2;
            taken = true;
        }
    }
    if (!taken) f2 = 0.0f;
    const float invP = prt_af_inv_p(A, 1u, f2);
    float g[25], l[25];
    uint32_t have = 0; // bit k: tap k exists
    float sw = 0.0f, sl = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int k = (dy + 2) * 5 + (dx + 2);
            g[k] = 0.0f;
            l[k] = 0.0f;
            const uint32_t r = prt_af_nb(A, x, y, dx, dy);
            if (r == PRT_AF_NONE) continue;
            have |= 1u << k;
            l[k] = prt_af_lum(A.values + (size_t)r * A.stride);
            g[k] = (dx == 0 && dy == 0) ? 1.0f
                                        : prt_af_geo(Pq, Nq, prt_af_ld4(A.points + r), prt_af_ld4((const char*)(A.points + r) + 16), invP, A.npl2);
            sw = sw + g[k];
            sl = sl + g[k] * l[k];
        }
    }
    const float m1 = sl / sw;
    float sv = 0.0f;
#pragma unroll
    for (int k = 0; k < 25; k++) {
        if (!(have & (1u << k))) continue;
        const float d = l[k] - m1;
        sv = sv + g[k] * (d * d);
    }
    prt_af_st4(A.rec + q, PrtAfQuad{prt_u2f(1u), f2, sv / sw, 0.0f});
}

// One iteration of point q.  LAST: the result goes to the caller's out, a point that is not placed gets the bytes of its values,
// and no variance is written.  MULTI: stride > 3; the 25 weights and tap indices are kept and the other channels loop over them.
template <bool LAST, bool MULTI> PRT_HD void prt_af_iterate(const PrtAfArgs& A, uint32_t q)
{
    const uint32_t stride = A.stride;
    const PrtAfQuad rec = prt_af_ld4(A.rec + q);
    if (prt_f2u(rec.x) == 0u) {
        if (LAST) {
            const float* v = A.values + (size_t)q * stride;
            float* o = A.cout + (size_t)q * stride;
            for (uint32_t j = 0; j < stride; j++) {
                uint32_t w;
                __builtin_memcpy(&w, v + j, 4);
                __builtin_memcpy(o + j, &w, 4);
            }
        }
        return;
    }
    const uint32_t t = A.texels[q];
    const int x = (int)(t % A.W), y = (int)(t / A.W), s = (int)A.step;
    const PrtAfQuad Pq = prt_af_ld4(A.points + q), Nq = prt_af_ld4((const char*)(A.points + q) + 16);
    const float invP = prt_af_inv_p(A, A.step, rec.y);
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const uint32_t r = prt_af_nb(A, x, y, dx, dy);
            if (r == PRT_AF_NONE) continue;
            const float wt = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            a = a + wt * A.vin[(size_t)r * A.vinStride];
            b = b + wt;
        }
    }
    const float invDen = 1.0f / (A.sigL * sqrtf(a / b) + 1e-6f);
    const float Lq = prt_af_lum(A.cin + (size_t)q * stride);
    float w[MULTI ? 25 : 1];
    uint32_t idx[MULTI ? 25 : 1];
    float sumW = 0.0f, sumV = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int k = MULTI ? (dy + 2) * 5 + (dx + 2) : 0;
            const uint32_t r = prt_af_nb(A, x, y, dx * s, dy * s);
            if (MULTI) {
                idx[k] = r;
                w[k] = 0.0f;
            }
            if (r == PRT_AF_NONE) continue;
            const float* cr = A.cin + (size_t)r * stride;
            float wk;
            if (dx == 0 && dy == 0) {
                wk = 0.375f * 0.375f;
            } else {
                const float geo = prt_af_geo(Pq, Nq, prt_af_ld4(A.points + r), prt_af_ld4((const char*)(A.points + r) + 16), invP, A.npl2);
                wk = ((prt_af_h(dy) * prt_af_h(dx)) * geo) * prt_af_f(fabsf(Lq - prt_af_lum(cr)) * invDen);
            }
            if (MULTI) w[k] = wk;
            sumW = sumW + wk;
            S0 = S0 + wk * cr[0];
            S1 = S1 + wk * cr[1];
            S2 = S2 + wk * cr[2];
            if (!LAST) sumV = sumV + (wk * wk) * A.vin[(size_t)r * A.vinStride];
        }
    }
    float* o = A.cout + (size_t)q * stride;
    o[0] = S0 / sumW;
    o[1] = S1 / sumW;
    o[2] = S2 / sumW;
    if (!LAST) A.vout[q] = sumV / (sumW * sumW);
    if (MULTI) {
        for (uint32_t c = 3; c < stride; c += 3) {
            S0 = 0.0f;
            S1 = 0.0f;
            S2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 25; k++) {
                if (idx[k] == PRT_AF_NONE) continue;
                const float* cr = A.cin + (size_t)idx[k] * stride + c;
                S0 = S0 + w[k] * cr[0];
                S1 = S1 + w[k] * cr[1];
                S2 = S2 + w[k] * cr[2];
            }
            o[c] = S0 / sumW;
            o[c + 1] = S1 / sumW;
            o[c + 2] = S2 / sumW;
        }
    }
}
