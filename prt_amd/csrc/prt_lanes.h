// prt_lanes.h -- device helpers of the frame kernel's 8-lane pixel groups (prt_frame.h) that the G-buffer and row-test kernels
// (prt_kernels.hip) share: ballots and sums over a group or a wave, the camera ray of a lane, the queue and slot-flag names and the
// streaming loads and stores of the pool state.
#pragma once
#include "prt_device.h"

// ============================================================================ device: group helpers
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// ballot restricted to the caller's 8-lane group (bits 0..7)
__device__ __forceinline__ uint32_t group_ballot(bool p, uint32_t gbase)
{
    unsigned long long b = __ballot(p);
    return (uint32_t)(b >> gbase) & 0xffu;
}

__device__ __forceinline__ uint32_t nth_set(uint32_t m, uint32_t n)
{
    for (uint32_t k = 0; k < n; k++) m &= m - 1u;
    return m ? (uint32_t)__builtin_ctz(m) : 0u;
}

// sum over the wave's active lanes (all 64 lanes must call it); result valid in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ float shf(float v, uint32_t srcLane) { return __shfl(v, (int)srcLane, 64); }
__device__ __forceinline__ uint32_t shu(uint32_t v, uint32_t srcLane) { return (uint32_t)__shfl((int)v, (int)srcLane, 64); }
__device__ __forceinline__ Vec3 sh3(Vec3 v, uint32_t srcLane) { return mk3(shf(v.x, srcLane), shf(v.y, srcLane), shf(v.z, srcLane)); }

// path_tracer.cpp:143-153 (and :176-184): cosine-weighted direction about `normal`
__device__ __forceinline__ Vec3 diffuse_dir(Vec3 normal, float r2, float r1)
{
    const float kPi = 3.14159265358979323846f;
    float r2sq = sqrtf(r2);
    Vec3 u = (fabsf(normal.x) > 0.1f) ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
    Vec3 tangent = normalize3(cross3(normal, u));
    Vec3 binormal = normalize3(cross3(tangent, normal));
    float theta = 2.0f * kPi * r1;
    float sn, cs;
    prt_sincosf(theta, &sn, &cs);
    return add3(add3(scale3(r2sq * cs, binormal), scale3(r2sq * sn, tangent)), scale3(1.0f - r2, normal));
}

// camera.cpp:46-56 for one lane: consumes the two draws dxBits, dyBits
__device__ __forceinline__ Vec3 camera_dir(const DevCamera& cam, uint32_t x, uint32_t y, uint32_t dxBits, uint32_t dyBits)
{
    const float kScreenScale = 0.6f;
    const float kAspect = (float)cam.width / (float)cam.height;
    const float kScaleX = 0.5f * cam.invWidth;
    const float kScaleY = 0.5f * cam.invHeight;
    float dx = (2.0f * rng_to_float(dxBits) - 1.0f) * kScaleX;
    float dy = (2.0f * rng_to_float(dyBits) - 1.0f) * kScaleY;
    float nx = 2.0f * ((float)x * cam.invWidth - 0.5f + dx) * kScreenScale * kAspect;
    float ny = -2.0f * ((float)y * cam.invHeight - 0.5f + dy) * kScreenScale;
    Vec3 right = mk3(cam.right[0], cam.right[1], cam.right[2]);
    Vec3 up = mk3(cam.up[0], cam.up[1], cam.up[2]);
    Vec3 fwd = mk3(cam.dir[0], cam.dir[1], cam.dir[2]);
    return normalize3(add3(add3(scale3(nx, right), scale3(ny, up)), fwd));
}

// Camera::GenerateJitteredRayPacket (camera.cpp:35-73) across the 8 lanes of a group: lane s uses draws
// 2s and 2s+1 of the 16 the packet consumes; avgDir is the lane-ordered sum / 8.
__device__ __forceinline__ void camera_packet(const DevCamera& cam, uint32_t& rng, uint32_t x, uint32_t y, uint32_t slot, uint32_t gbase,
                                              DevRay& ray, Vec3& avgDir)
{
    uint32_t s = rng, dxb = 0, dyb = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        s = xorshift32(s);
        if (j == 2 * slot) dxb = s;
        if (j == 2 * slot + 1) dyb = s;
    }
    rng = s;
    ray.org = mk3(cam.pos[0], cam.pos[1], cam.pos[2]);
    ray.dir = camera_dir(cam, x, y, dxb, dyb);
    Vec3 avg = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (uint32_t l = 0; l < 8; l++) avg = add3(avg, sh3(ray.dir, gbase + l));
    avgDir = div3s(avg, 8.0f);
    prepare_soa(ray);
}

struct Surf5 { // what moves between slots at a compaction
    Vec3 normal;
    Vec2 uv;
    uint32_t mat, prim;
};

// ============================================================================ the per-pixel loop
// The loop of the reference is run as a state machine over pixel groups (a group = the 8 path slots of one pixel, one lane
// each); one round of a group = a shade pass (consume the hits of its last rays, run the bounce of path_tracer.cpp:124-293,
// emit the next rays) followed by the traversal of those rays.  A packet needs 1 + maxDepth rounds, a pixel
// (samples/8)*(1+maxDepth)+1.  Scheduling, queues and kernels: prt_frame.h.
enum { Q_PRIMARY = PRT_MODE_PACKET, Q_SCATTER = PRT_MODE_SINGLE, Q_OCC_PACKET = PRT_MODE_OCC_PACKET, Q_OCC_SINGLE = PRT_MODE_OCC_SINGLE, Q_COUNT = 4 };
enum { PH_START = 0, PH_WAIT_PRIMARY = 1, PH_WAIT_BOUNCE = 2, PH_DONE = 3 };
#define SLOT_HAS_SHADOW 1u
#define SLOT_SURVIVE 2u
#define SLOT_LIGHT_SET 4u


// streaming (touch-once-per-iteration) state goes around the caches' retention so that the BVH stays resident
typedef float f4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4* p)
{
    f4_t v = __builtin_nontemporal_load((const PRT_AS1 f4_t*)p);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store4(float4* p, float4 v)
{
    f4_t w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, (PRT_AS1 f4_t*)p);
}
__device__ __forceinline__ uint32_t nt_load(const uint32_t* p) { return __builtin_nontemporal_load((const PRT_AS1 uint32_t*)p); }
__device__ __forceinline__ void nt_store(uint32_t* p, uint32_t v) { __builtin_nontemporal_store(v, (PRT_AS1 uint32_t*)p); }
