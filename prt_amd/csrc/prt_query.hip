// prt_query.hip -- ray queries (include/prt_hip.h "ray queries"): nearest hit, any hit and surface records for batches of the caller's
// own rays.  The traversal is trace_loop of prt_device.h, unchanged, in the shell every batch kernel shares (prt_batch.h), behind a ray
// source that reads prt_ray records and a sink that writes prt_hit / prt_surface / one byte; the surface fetch is get_surface,
// sample_bump and sample_diffuse, unchanged.  In a translation unit of its own, as prt_temporal.hip and prt_display.hip are, so that
// the code objects of every other kernel -- the frame kernel's above all -- do not move.
// prt_hip_query_radiance (radiance along the caller's rays) has its checks and its array table here; its kernel is the frame kernel's probe
// instantiation, launched by prt_frame_probe (prt_kernels.hip), which shares the launch code of the renders.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "prt_internal.h"

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define PRT_QUERY_MAX_RAYS (1u << 30)
#define PRT_QUERY_BLOCKS_PER_CU 2 // a workgroup is 16 waves and a CU holds 32: two are resident, more would only queue behind them

static_assert(sizeof(prt_ray) == 32 && sizeof(prt_surface) == 80 && sizeof(prt_hit) == 24, "record sizes of the ray queries");

// What a query needs of the scene beside DevScene: per mesh the first global material and the number of triangles.
struct QueryMeshes {
    uint32_t matBase[PRT_MAX_BVH];
    uint32_t primCount[PRT_MAX_BVH];
};

struct QueryArgs {
    DevScene sc;
    QueryMeshes qm;
    uint32_t n;
    const float4* rays; // 2 x float4 per ray: {org, tMax} {dir, pad}
    prt_hit* hits;
    float4* surf;       // 5 x float4 per record, or nullptr
    uint8_t* occ;
    BatchCtl ctl;
};

__device__ __forceinline__ void store_miss(float4* q)
{
    gst4(q, make_float4(0.0f, 0.0f, 0.0f, -1.0f));
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    gst4(q + 1, z);
    gst4(q + 2, z);
    gst4(q + 3, z);
    gst4(q + 4, z);
}

// The record of hit h (primId = the triangle SLOT, as the traversal reports it) of the ray (org, dir); prim = its primId in its mesh.
__device__ __forceinline__ void store_surface(const DevScene& sc, const QueryMeshes& qm, Vec3 org, Vec3 dir, const DevHit& h, uint32_t prim, float4* q)
{
    Traffic tr{};
    Surface s;
    get_surface<false>(sc, h, s, tr);
    const Vec3 bn = sample_bump<false>(sc, s.mat, s, tr);
    const Vec3 kd = sample_diffuse<false>(sc, s.mat, s.uv, tr);
    gst4(q, make_float4(org.x + h.t * dir.x, org.y + h.t * dir.y, org.z + h.t * dir.z, h.t));
    gst4(q + 1, make_float4(s.normal.x, s.normal.y, s.normal.z, asf(s.mat)));
    gst4(q + 2, make_float4(bn.x, bn.y, bn.z, asf(s.mat - qm.matBase[h.meshId])));
    gst4(q + 3, make_float4(s.uv.x, s.uv.y, asf(prim), asf(h.meshId)));
    gst4(q + 4, make_float4(kd.x, kd.y, kd.z, 0.0f));
}

template <bool SURFACE>
struct QuerySrc {
    const QueryArgs* A;
    __device__ __forceinline__ uint32_t count() const { return A->n; }
    __device__ __forceinline__ uint32_t* cursor() const { return A->ctl.cursor; }
    __device__ __forceinline__ void load(uint32_t i, Vec3& org, Vec3& dir, float& maxT, uint32_t& rev) const
    {
        const float4 a = gld4(A->rays + 2 * (size_t)i), b = gld4(A->rays + 2 * (size_t)i + 1);
        org = mk3(a.x, a.y, a.z);
        dir = mk3(b.x, b.y, b.z);
        maxT = a.w;
        rev = 0;
        // trace_loop answers a ray with a NaN in org or dir without a walk; a NaN limit gets the same answer the same way (every
        // t < NaN is false, so the walk of the whole tree it would otherwise take records nothing)
        if (!(maxT == maxT)) org.x = maxT;
    }
    __device__ __forceinline__ void store_hit(uint32_t i, const DevHit& h) const
    {
        const bool hit = h.t != -1.0f && h.t == h.t; // (a NaN limit leaves hit.t NaN: never stored)
        prt_hit o;
        o.t = hit ? h.t : -1.0f; o.i = h.i; o.j = h.j; o.k = h.k;
        // the device names a hit triangle by its slot; the reference's primId is that triangle's index in its mesh
        o.primId = hit ? gld(A->sc.triPrim + h.primId) : h.primId;
        o.meshId = h.meshId;
        A->hits[i] = o;
        if (SURFACE) {
            float4* q = A->surf + 5 * (size_t)i;
            if (hit) {
                const float4 a = gld4(A->rays + 2 * (size_t)i), b = gld4(A->rays + 2 * (size_t)i + 1);
                store_surface(A->sc, A->qm, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), h, o.primId, q);
            } else {
                store_miss(q);
            }
        }
    }
    __device__ __forceinline__ void store_occ(uint32_t i, bool occ) const { A->occ[i] = occ ? 1 : 0; }
};

template <bool SURFACE>
__global__ __launch_bounds__(PRT_BLOCK) void query_nearest_kernel(QueryArgs A)
{
    QuerySrc<SURFACE> src{&A};
    trace_batch<PRT_MODE_SINGLE>(A.sc, src, A.ctl);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&A.ctl.counters[PRT_STAT_RAYS], (unsigned long long)A.n);
}

__global__ __launch_bounds__(PRT_BLOCK) void query_any_kernel(QueryArgs A)
{
    QuerySrc<false> src{&A};
    trace_batch<PRT_MODE_OCC_SINGLE>(A.sc, src, A.ctl);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&A.ctl.counters[PRT_STAT_RAYS], (unsigned long long)A.n);
        atomicAdd(&A.ctl.counters[PRT_STAT_OCCL], (unsigned long long)A.n);
    }
}

// ============================================================================ the inverse of triPrim
// inv[slotBase of the mesh + primId] = slot, for every slot that holds a triangle (a pad slot names no vertices: prt_upload.hip);
// the host has filled inv with 0xffffffff.  A triPrim beyond the mesh's slots cannot come from an accepted upload and is skipped.
struct IndexArgs {
    const uint32_t* triPrim;
    const uint32_t* slotVtx;
    uint32_t* inv;
    uint32_t slots, meshes;
    uint32_t slotBase[PRT_MAX_BVH], slotCount[PRT_MAX_BVH];
};

__global__ __launch_bounds__(256) void query_index_kernel(IndexArgs a)
{
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.slots; s += gridDim.x * blockDim.x) {
        if (a.slotVtx[3 * (size_t)s] == 0xffffffffu) continue;
        const uint32_t prim = a.triPrim[s];
        for (uint32_t m = 0; m < a.meshes; m++)
            if (s - a.slotBase[m] < a.slotCount[m] && prim < a.slotCount[m]) a.inv[a.slotBase[m] + prim] = s; // (s < slotBase wraps: false)
    }
}

// ============================================================================ surface records of the caller's hits
struct SurfaceArgs {
    DevScene sc;
    QueryMeshes qm;
    uint32_t n;
    const float4* rays;
    const prt_hit* hits;
    float4* surf;
    const uint32_t* inv;
    unsigned long long* invalid;
};

__global__ __launch_bounds__(256) void query_surface_kernel(SurfaceArgs A)
{
    uint32_t bad = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < A.n; r += gridDim.x * blockDim.x) {
        const prt_hit in = A.hits[r];
        float4* q = A.surf + 5 * (size_t)r;
        uint32_t slot = 0xffffffffu;
        // every index from caller memory is checked before it becomes an address
        if (in.meshId < A.sc.bvhCount && in.primId < A.qm.primCount[in.meshId]) slot = A.inv[A.sc.primBase[in.meshId] + in.primId];
        if (slot == 0xffffffffu) {
            bad++;
            store_miss(q);
        } else if (in.t == -1.0f || !(in.t == in.t)) {
            store_miss(q);
        } else {
            const float4 a = gld4(A.rays + 2 * (size_t)r), b = gld4(A.rays + 2 * (size_t)r + 1);
            DevHit h;
            h.t = in.t; h.i = in.i; h.j = in.j; h.k = in.k;
            h.primId = slot;
            h.meshId = in.meshId;
            store_surface(A.sc, A.qm, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), h, in.primId, q);
        }
    }
    if (bad) atomicAdd(A.invalid, (unsigned long long)bad);
}

// ============================================================================ host side
QueryMeshes query_meshes(const prt_hip_ctx* c)
{
    QueryMeshes qm{};
    for (uint32_t m = 0; m < c->sc.bvhCount && m < PRT_MAX_BVH; m++) qm.matBase[m] = m < c->ed.meshes.size() ? c->ed.meshes[m].matBase : 0u;
    prt_query_prim_counts(c, qm.primCount);
    return qm;
}

int check_batch(prt_hip_ctx* c, uint32_t n, uint32_t flags, const char* what)
{
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, std::string(what) + ": upload a scene first");
    if (n == 0 || n > PRT_QUERY_MAX_RAYS) return fail(PRT_HIP_EINVAL, std::string(what) + ": n must be 1 .. 2^30");
    return prt_check_flags(flags, what);
}

// One launch of a traversal kernel over the batch on the context's stream, timed as a render.
int launch_trace(prt_hip_ctx* c, uint32_t n, const prt_ray* rays, prt_hit* hits, prt_surface* surf, uint8_t* occ, bool any)
{
    hipStream_t s = c->stream;
    BatchLaunch L;
    int rc = prt_batch_begin(c, n, (uint32_t)c->computeUnits * PRT_QUERY_BLOCKS_PER_CU, true, &L);
    if (rc) return rc;
    QueryArgs A{c->sc, query_meshes(c), n, (const float4*)rays, hits, (float4*)surf, occ, L.ctl};
    if (any) hipLaunchKernelGGL(query_any_kernel, dim3(L.blocks), dim3(PRT_BLOCK), 0, s, A);
    else if (surf) hipLaunchKernelGGL(query_nearest_kernel<true>, dim3(L.blocks), dim3(PRT_BLOCK), 0, s, A);
    else hipLaunchKernelGGL(query_nearest_kernel<false>, dim3(L.blocks), dim3(PRT_BLOCK), 0, s, A);
    return prt_batch_end(c, L, any ? "query_any_kernel" : "query_nearest_kernel");
}

int launch_surface(prt_hip_ctx* c, uint32_t n, const prt_ray* rays, const prt_hit* hits, prt_surface* surf)
{
    int rc = prt_query_inverse_ready(c);
    if (rc) return rc;
    HIP_TRY(c->qCounts.fit(1, c->stream));
    HIP_TRY(hipMemsetAsync(c->qCounts, 0, sizeof(unsigned long long), c->stream));
    SurfaceArgs A{c->sc, query_meshes(c), n, (const float4*)rays, hits, (float4*)surf, c->qInv, c->qCounts};
    const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, (uint32_t)c->computeUnits * 8u);
    hipLaunchKernelGGL(query_surface_kernel, dim3(blocks), dim3(256), 0, c->stream, A);
    return prt_launched("query_surface_kernel");
}

// One query: what it launches, and where its arrays stand in the table; an entry the query has no array for stays null.
// Q_HITS_IN: the hits QUERY_SURFACE fetches records of (nothing is traced then).
enum QueryKind { QUERY_NEAREST, QUERY_ANY, QUERY_SURFACE };
enum { Q_RAYS, Q_HITS_IN, Q_HITS, Q_SURF, Q_OCC, Q_ARRAYS };

// What the three queries share behind their NULL checks.
int run_query(prt_hip_ctx* c, uint32_t n, QueryKind kind, const prt_ray* rays, const prt_hit* hitsIn, prt_hit* hits, prt_surface* surf, uint8_t* occ,
              uint32_t flags, void* stream, const char* what)
{
    int rc = check_batch(c, n, flags, what);
    if (rc) return rc;
    PrtIoArray io[Q_ARRAYS] = {prt_io_in(rays, (size_t)n * sizeof(prt_ray), 16), prt_io_in(hitsIn, (size_t)n * sizeof(prt_hit), 4),
                               prt_io_out(hits, (size_t)n * sizeof(prt_hit), 4), prt_io_out(surf, (size_t)n * sizeof(prt_surface), 16),
                               prt_io_out(occ, n, 1)};
    const bool records = hits || hitsIn || surf;
    return prt_run_io(c, flags, stream, std::string(what) + (records ? ": rays and surfaces must be 16-byte aligned, hits 4-byte aligned"
                                                                      : ": rays must be 16-byte aligned"), io, Q_ARRAYS, [&]() {
        if (kind == QUERY_SURFACE) return launch_surface(c, n, io[Q_RAYS].as<prt_ray>(), io[Q_HITS_IN].as<prt_hit>(), io[Q_SURF].as<prt_surface>());
        return launch_trace(c, n, io[Q_RAYS].as<prt_ray>(), io[Q_HITS].as<prt_hit>(), io[Q_SURF].as<prt_surface>(), io[Q_OCC].as<uint8_t>(),
                            kind == QUERY_ANY);
    });
}

} // namespace

// The inverse table of the uploaded scene on the context's stream (first use after an upload); prt_hip_atlas_points
// (prt_atlas.hip) needs it too.
int prt_query_inverse_ready(prt_hip_ctx* c)
{
    if (c->qInv) return PRT_HIP_OK;
    const PrtRefit& R = c->rf;
    const uint64_t slots = R.slotVtx.size() / 3;
    if (slots == 0 || slots > 0xffffffffull || !R.slotVtx || R.meshes.size() != c->sc.bvhCount)
        return fail(PRT_HIP_ESTATE, "query_surface: the scene holds no triangle slots");
    IndexArgs a{};
    a.triPrim = c->sc.triPrim;
    a.slotVtx = R.slotVtx;
    a.slots = (uint32_t)slots;
    a.meshes = c->sc.bvhCount;
    for (uint32_t m = 0; m < a.meshes; m++) {
        const PrtRefitMesh& rm = R.meshes[m];
        if ((uint64_t)rm.slotBase + rm.slotCount > slots || rm.slotBase != c->sc.primBase[m])
            return fail(PRT_HIP_ESTATE, "query_surface: slot range outside the scene");
        a.slotBase[m] = rm.slotBase;
        a.slotCount[m] = rm.slotCount;
    }
    HIP_TRY(c->qInv.fit(slots, c->stream));
    a.inv = c->qInv;
    HIP_TRY(hipMemsetAsync(c->qInv, 0xff, slots * sizeof(uint32_t), c->stream));
    const uint32_t blocks = std::min<uint32_t>((a.slots + 255u) / 256u, 65535u);
    hipLaunchKernelGGL(query_index_kernel, dim3(blocks), dim3(256), 0, c->stream, a);
    return prt_launched("query_index_kernel");
}

void prt_query_prim_counts(const prt_hip_ctx* c, uint32_t primCount[PRT_MAX_BVH])
{
    for (uint32_t m = 0; m < PRT_MAX_BVH; m++)
        primCount[m] = m < c->sc.bvhCount && m < c->rf.meshes.size() ? std::min(c->rf.meshes[m].primCount, c->rf.meshes[m].slotCount) : 0u;
}

// ENODEVICE on a machine without a device (where no context can exist), EINVAL otherwise
int prt_null_argument(const char* what)
{
    if (prt_hip_device_count() == 0) return fail(PRT_HIP_ENODEVICE, "no HIP device: libprt_hip has no CPU path (the GPU kernels are the product)");
    return fail(PRT_HIP_EINVAL, std::string(what) + ": NULL argument");
}

// ============================================================================ radiance along the caller's rays
#define PRT_QUERY_MAX_PROBES (1u << 24)

// What prt_hip_query_radiance asks of its scalar arguments, and prt_hip_bake (prt_bake.hip) of its n*K probes; everything is refused
// before anything is queued.
int prt_check_radiance(prt_hip_ctx* c, uint32_t n, const prt_render_params* p, uint32_t flags, const char* what)
{
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, std::string(what) + ": upload a scene first");
    if (n == 0 || n > PRT_QUERY_MAX_PROBES) return fail(PRT_HIP_EINVAL, std::string(what) + ": n must be 1 .. 2^24");
    int rc = prt_check_flags(flags, what);
    if (rc) return rc;
    if (p->samples < 8 || p->samples % 8 != 0 || p->samples / 8 > 255)
        return fail(PRT_HIP_EINVAL, std::string(what) + ": samples must be a multiple of 8 from 8 to 2040");
    if (p->maxDepth > 255) return fail(PRT_HIP_EINVAL, std::string(what) + ": maxDepth too large");
    if (p->rank != 0 || p->nranks != 1) return fail(PRT_HIP_EINVAL, std::string(what) + ": probes are not split over ranks (rank 0 of nranks 1)");
    if (p->countTraffic != 0) return fail(PRT_HIP_EINVAL, std::string(what) + ": countTraffic must be 0 (the probe kernel has no counting build)");
    return PRT_HIP_OK;
}

extern "C" {

int prt_hip_query_radiance(prt_hip_ctx* c, uint32_t n, const prt_ray* rays, const prt_render_params* p, float* radiance, uint32_t flags,
                           void* stream)
{
    if (!c || !rays || !p || !radiance) return prt_null_argument("query_radiance");
    int rc = prt_check_radiance(c, n, p, flags, "query_radiance");
    if (rc) return rc;
    PrtIoArray io[2] = {prt_io_in(rays, (size_t)n * sizeof(prt_ray), 16), prt_io_out(radiance, 3 * (size_t)n * sizeof(float), 4)};
    return prt_run_io(c, flags, stream, "query_radiance: rays must be 16-byte aligned, radiance 4-byte aligned", io, 2,
                      [&]() { return prt_frame_probe(c, n, io[0].as<prt_ray>(), p, io[1].as<float>()); });
}

int prt_hip_query_nearest(prt_hip_ctx* c, uint32_t n, const prt_ray* rays, prt_hit* hits, prt_surface* surfaces, uint32_t flags, void* stream)
{
    if (!c || !rays || !hits) return prt_null_argument("query_nearest");
    return run_query(c, n, QUERY_NEAREST, rays, nullptr, hits, surfaces, nullptr, flags, stream, "query_nearest");
}

int prt_hip_query_any(prt_hip_ctx* c, uint32_t n, const prt_ray* rays, uint8_t* occluded, uint32_t flags, void* stream)
{
    if (!c || !rays || !occluded) return prt_null_argument("query_any");
    return run_query(c, n, QUERY_ANY, rays, nullptr, nullptr, nullptr, occluded, flags, stream, "query_any");
}

int prt_hip_query_surface(prt_hip_ctx* c, uint32_t n, const prt_ray* rays, const prt_hit* hits, prt_surface* surfaces, uint32_t flags, void* stream)
{
    if (!c || !rays || !hits || !surfaces) return prt_null_argument("query_surface");
    return run_query(c, n, QUERY_SURFACE, rays, hits, nullptr, surfaces, nullptr, flags, stream, "query_surface");
}

int prt_hip_query_get_counts(prt_hip_ctx* c, uint64_t* invalidHits)
{
    if (!c || !invalidHits) return prt_null_argument("query_get_counts");
    *invalidHits = 0;
    if (!c->qCounts) return PRT_HIP_OK; // no query_surface yet
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, c->qCounts, sizeof(v), hipMemcpyDeviceToHost));
    *invalidHits = v;
    return PRT_HIP_OK;
}

} // extern "C"
