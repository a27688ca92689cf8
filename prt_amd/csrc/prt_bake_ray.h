// prt_bake_ray.h -- the ray of a bake point and one direction of its set (include/prt_hip.h "baking", "Ray r = i*K + k"), once:
// bake_rays_kernel (prt_bake.hip) stores it, the ray source of vis_trace_kernel (prt_visibility.hip) hands it to trace_loop in
// registers.  The frame is the one of diffuse_dir (prt_lanes.h) through the cross3 and normalize3 of prt_device.h.
#pragma once
#include "prt_device.h"

// org and dir of ray k of point i; false, with org = dir = 0, for a set outside the table, which is never followed.
// points: 2 x float4 per point, {P, bias} {N, set}; dirs: nSets * K * 3.
__device__ __forceinline__ bool bake_ray(const float4* points, const float* dirs, uint32_t K, uint32_t nSets, uint32_t i, uint32_t k, Vec3& org,
                                         Vec3& dir)
{
    const float4 a = gld4(points + 2 * (size_t)i), b = gld4(points + 2 * (size_t)i + 1);
    const uint32_t set = asu(b.w);
    org = mk3(0.0f, 0.0f, 0.0f);
    dir = mk3(0.0f, 0.0f, 0.0f);
    if (set >= nSets) return false;
    const float* dp = dirs + ((size_t)set * K + k) * 3;
    const Vec3 d = mk3(dp[0], dp[1], dp[2]);
    const Vec3 P = mk3(a.x, a.y, a.z), N = mk3(b.x, b.y, b.z);
    if (N.x == 0.0f && N.y == 0.0f && N.z == 0.0f) { // (either zero) the identity frame
        org = P;
        dir = d;
    } else { // path_tracer.cpp:147-153, N as given
        const Vec3 u = (fabsf(N.x) > 0.1f) ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
        const Vec3 T = normalize3(cross3(N, u));
        const Vec3 B = normalize3(cross3(T, N));
        dir = add3(add3(scale3(d.x, B), scale3(d.y, T)), scale3(d.z, N));
        org = add3(P, scale3(a.w, N));
    }
    return true;
}
