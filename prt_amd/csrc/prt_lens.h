// prt_lens.h -- the arithmetic of the lens renders (include/prt_hip.h "lens renders"), in ONE text that lens_rays_kernel
// (prt_lens.hip) runs on the device and tests/lens_main.cpp runs on the host: the four jitter draws of a ray, the film coordinates and
// the ray of each camera model.  All of it is f32 without FMA (the build's -ffp-contract=off), every product rounded before the sum
// that uses it, sums left to right as written, sqrtf and / correctly rounded; sine and cosine are prt_sincosf (prt_devmath.h: double
// precision inside, so the device needs no libm).  The integer steps restate pixel_seed, xorshift32 and rng_to_float of prt_device.h,
// which is device code only.
#pragma once
#include <math.h>

#include "../../include/prt_hip.h"
#include "prt_devmath.h"

struct PrtLensVec {
    float x, y, z;
};
struct PrtLensRay {
    PrtLensVec org, dir;
};
// What does not depend on the ray: computed once per lane, before the grid-stride loop
struct PrtLensFrame {
    float invW, invH;
    PrtLensVec R, U; // normalize3(right), normalize3(up): the lens disc's axes (PINHOLE with lensRadius > 0 reads them)
};

PRT_HD PrtLensVec prt_lens_v(const float* p) { return PrtLensVec{p[0], p[1], p[2]}; }
PRT_HD PrtLensVec prt_lens_add(PrtLensVec a, PrtLensVec b) { return PrtLensVec{a.x + b.x, a.y + b.y, a.z + b.z}; }
PRT_HD PrtLensVec prt_lens_sub(PrtLensVec a, PrtLensVec b) { return PrtLensVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
PRT_HD PrtLensVec prt_lens_scale(float f, PrtLensVec v) { return PrtLensVec{f * v.x, f * v.y, f * v.z}; }
// normalize3 of the baking section (vecmath.h:1200)
PRT_HD PrtLensVec prt_lens_normalize(PrtLensVec v)
{
    const float inv = 1.0f / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return prt_lens_scale(inv, v);
}

// the five steps of pixel_seed (prt_device.h) without the final | 1
PRT_HD uint32_t prt_lens_mix(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}
PRT_HD uint32_t prt_lens_xorshift32(uint32_t x)
{
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
}
PRT_HD float prt_lens_unit(uint32_t u) { return prt_u2f((u & 0x007fffffu) | 0x3f800000u) - 1.0f; } // rng_to_float

// The four draws of ray k of pixel (x, y): always all four, so the stream does not depend on the model.
PRT_HD void prt_lens_draws(const prt_lens_desc* d, uint32_t x, uint32_t y, uint32_t k, float u[4])
{
    const uint32_t pix = y * d->width + x, j = d->pass * d->K + k;
    uint32_t s = prt_lens_mix(prt_lens_mix(pix + d->jitterSeed) + j) | 1u;
    for (int i = 0; i < 4; i++) {
        s = prt_lens_xorshift32(s);
        u[i] = prt_lens_unit(s);
    }
}

PRT_HD PrtLensFrame prt_lens_frame(const prt_lens_desc* d)
{
    PrtLensFrame f;
    f.invW = 1.0f / (float)d->width;
    f.invH = 1.0f / (float)d->height;
    f.R = prt_lens_normalize(prt_lens_v(d->right));
    f.U = prt_lens_normalize(prt_lens_v(d->up));
    return f;
}

// dir = (l.x*right + l.y*up) + l.z*fwd: EQUIRECT and FISHEYE
PRT_HD PrtLensVec prt_lens_local(const prt_lens_desc* d, PrtLensVec l)
{
    return prt_lens_add(prt_lens_add(prt_lens_scale(l.x, prt_lens_v(d->right)), prt_lens_scale(l.y, prt_lens_v(d->up))),
                        prt_lens_scale(l.z, prt_lens_v(d->fwd)));
}

// Ray k of pixel (x, y), as the header defines it.  d->model has been checked.
PRT_HD PrtLensRay prt_lens_ray(const prt_lens_desc* d, const PrtLensFrame* f, uint32_t x, uint32_t y, uint32_t k)
{
    float u[4];
    prt_lens_draws(d, x, y, k, u);
    const bool centre = (d->flags & PRT_HIP_LENS_CENTRE) != 0;
    const float jx = centre ? 0.5f : u[0], jy = centre ? 0.5f : u[1];
    const float sx = ((float)x + jx) * f->invW, sy = ((float)y + jy) * f->invH;
    const float a = 2.0f * sx - 1.0f, b = 1.0f - 2.0f * sy;
    const PrtLensVec pos = prt_lens_v(d->pos), fwd = prt_lens_v(d->fwd), right = prt_lens_v(d->right), up = prt_lens_v(d->up);
    PrtLensRay r;
    r.org = pos;
    if (d->model == PRT_HIP_LENS_PINHOLE) {
        const PrtLensVec dd = prt_lens_add(prt_lens_add(fwd, prt_lens_scale(a, right)), prt_lens_scale(b, up));
        if (!(d->lensRadius > 0.0f)) {
            r.dir = dd;
        } else {
            const float rl = d->lensRadius * sqrtf(u[2]);
            float sn, cs;
            prt_sincosf(6.28318530717958647692f * u[3], &sn, &cs);
            r.org = prt_lens_add(prt_lens_add(pos, prt_lens_scale(rl * cs, f->R)), prt_lens_scale(rl * sn, f->U));
            const PrtLensVec F = prt_lens_add(pos, prt_lens_scale(d->focus, dd));
            r.dir = prt_lens_sub(F, r.org);
        }
    } else if (d->model == PRT_HIP_LENS_ORTHO) {
        r.org = prt_lens_add(prt_lens_add(pos, prt_lens_scale(a, right)), prt_lens_scale(b, up));
        r.dir = fwd;
    } else if (d->model == PRT_HIP_LENS_EQUIRECT) {
        float sp, cp, st, ct;
        prt_sincosf(a * 3.14159265358979323846f, &sp, &cp);
        prt_sincosf(b * 1.57079632679489661923f, &st, &ct);
        r.dir = prt_lens_local(d, PrtLensVec{ct * sp, st, ct * cp});
    } else { // PRT_HIP_LENS_FISHEYE
        const float rr = sqrtf(a * a + b * b);
        if (!(rr <= 1.0f)) { // outside the image circle (or a NaN): the probe rule answers a zero direction black
            r.dir = PrtLensVec{0.0f, 0.0f, 0.0f};
        } else {
            float st, ct;
            prt_sincosf(rr * (0.5f * d->fov), &st, &ct);
            const float q = rr > 0.0f ? st / rr : 0.0f;
            r.dir = prt_lens_local(d, PrtLensVec{a * q, b * q, ct});
        }
    }
    return r;
}
