// prt_atlas.hip -- lightmap atlases (include/prt_hip.h "lightmap atlases"): per-corner lightmap UVs in, a lightmap image out.  The two
// ends every lightmapper wrote on the host around prt_hip_bake (prt_bake.hip, reused as it stands), as three calls:
//     prt_hip_atlas_rasterize  atlas_raster_kernel  one wave per UV triangle: integer edge functions over its texel box, 8 x 8 texels a
//                                                   trip, ownership by a 32-bit atomic min on the key (meshId << 28) | primId
//                              atlas_flag_kernel    owned texels flagged; prt_select_flagged (stable) compacts their indices
//                              atlas_hits_kernel    one lane per owned texel: the owner's barycentrics at the texel centre
//     prt_hip_atlas_points     atlas_points_kernel  one lane per record: P from the slot's tris record, N from get_surface
//     prt_hip_atlas_resolve    atlas_scatter_kernel values to their texels; atlas_gutter_kernel, one launch per gutter pass
// In a translation unit of its own, as prt_query.hip and prt_bake.hip are, so that the code objects of every other kernel do not move.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "prt_internal.h"

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define PRT_ATLAS_MAX_DIM 8192u
#define PRT_ATLAS_MAX_PRIMS (1u << 28)
#define PRT_ATLAS_MAX_RECORDS (1u << 26) // texels of the largest atlas
#define PRT_ATLAS_MAX_STRIDE 48u
#define PRT_ATLAS_MAX_GUTTER 64u
#define PRT_ATLAS_MAX_TILE 32u
#define PRT_ATLAS_BLOCKS_PER_CU 8 // blocks of 256 lanes a kernel is launched with at the most, as in prt_bake.hip: all are grid-stride loops
#define PRT_ATLAS_NO_OWNER 0xffffffffu // no key reaches it: meshId < 8 leaves bit 31 clear
#define PRT_ATLAS_SNAP_LIMIT 8388608.0f // 2^23: a snapped coordinate fits 24 bits and a sign, every edge function int64

static_assert(sizeof(prt_hit) == 24 && sizeof(prt_bake_point) == 32 && PRT_MAX_BVH == PRT_HIP_MAX_BVH && PRT_MAX_BVH <= 8,
              "record sizes of the atlas kernels; three bits of a key name the mesh");

// The meshes of a rasterise call BY meshId (ownership does not depend on the order of the caller's records): uv = null where the call
// names no such mesh; first[m] = triangles of the meshes below m, first[PRT_MAX_BVH] = all.
struct AtlasMeshes {
    const float* uv[PRT_MAX_BVH];
    uint64_t first[PRT_MAX_BVH + 1];
};

// ============================================================================ the definition, shared by the raster and the hits kernel
struct SnapTri {
    int32_t x[3], y[3];
};

// Corner (u, v) on the 1/256-texel grid; false: a coordinate beyond 2^23 in magnitude, or a NaN (the triangle is rejected)
__device__ __forceinline__ bool atlas_snap(const float* uv, float sx, float sy, SnapTri& t)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float fx = gld(uv + 2 * k) * sx, fy = gld(uv + 2 * k + 1) * sy;
        ok = ok && (fabsf(fx) <= PRT_ATLAS_SNAP_LIMIT) && (fabsf(fy) <= PRT_ATLAS_SNAP_LIMIT);
        t.x[k] = ok ? (int32_t)rintf(fx) : 0; // (ties to even)
        t.y[k] = ok ? (int32_t)rintf(fy) : 0;
    }
    return ok;
}

// E(a, b, c): every difference fits 26 bits, every product 52
__device__ __forceinline__ int64_t atlas_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t cx, int32_t cy)
{
    return (int64_t)(bx - ax) * (int64_t)(cy - ay) - (int64_t)(by - ay) * (int64_t)(cx - ax);
}

__device__ __forceinline__ int64_t atlas_area(const SnapTri& t) { return atlas_edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]); }

// w0, w1, w2 of the centre of texel (x, y), with the sign of A taken out
__device__ __forceinline__ void atlas_weights(const SnapTri& t, bool flip, int32_t x, int32_t y, int64_t& w0, int64_t& w1, int64_t& w2)
{
    const int32_t cx = 256 * x + 128, cy = 256 * y + 128;
    w0 = atlas_edge(t.x[1], t.y[1], t.x[2], t.y[2], cx, cy);
    w1 = atlas_edge(t.x[2], t.y[2], t.x[0], t.y[0], cx, cy);
    w2 = atlas_edge(t.x[0], t.y[0], t.x[1], t.y[1], cx, cy);
    if (flip) {
        w0 = -w0;
        w1 = -w1;
        w2 = -w2;
    }
}

// ============================================================================ rasterise
struct RasterArgs {
    AtlasMeshes M;
    uint32_t W, H;
    uint32_t* owner;            // W*H keys, PRT_ATLAS_NO_OWNER before the launch
    unsigned long long* counts; // [0] pairs, [1] rejected, [2] degenerate ([3]: n, written by the selection)
};

// One wave per triangle, four per block.  The wave's index is made a scalar, so the triangle, its mesh and its six UVs are the same
// for the 64 lanes by construction and every trip count below is uniform; lane l takes texel (l & 7, l >> 3) of an 8 x 8 tile.
__global__ __launch_bounds__(256) void atlas_raster_kernel(RasterArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float sx = (float)(256u * A.W), sy = (float)(256u * A.H); // exact: at most 2^21
    unsigned long long pairs = 0;
    uint32_t rejected = 0, degenerate = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * 4u + wave; g < A.M.first[PRT_MAX_BVH]; g += (uint64_t)gridDim.x * 4u) {
        uint32_t m = 0;
#pragma unroll
        for (uint32_t k = 1; k < PRT_MAX_BVH; k++) m += g >= A.M.first[k] ? 1u : 0u; // (first is non-decreasing)
        const uint32_t prim = (uint32_t)(g - A.M.first[m]);
        SnapTri t;
        if (!atlas_snap(A.M.uv[m] + 6 * (size_t)prim, sx, sy, t)) {
            rejected++;
            continue;
        }
        const int64_t area = atlas_area(t);
        if (area == 0) {
            degenerate++;
            continue;
        }
        // the texels whose centre 256x + 128 lies in the triangle's box, clipped to the atlas (>> floors a negative numerator)
        const int32_t loX = min(t.x[0], min(t.x[1], t.x[2])), hiX = max(t.x[0], max(t.x[1], t.x[2]));
        const int32_t loY = min(t.y[0], min(t.y[1], t.y[2])), hiY = max(t.y[0], max(t.y[1], t.y[2]));
        const int32_t x0 = max(0, (loX - 128 + 255) >> 8), x1 = min((int32_t)A.W - 1, (hiX - 128) >> 8);
        const int32_t y0 = max(0, (loY - 128 + 255) >> 8), y1 = min((int32_t)A.H - 1, (hiY - 128) >> 8);
        if (x0 > x1 || y0 > y1) continue;
        const uint32_t key = (m << 28) | prim;
        for (int32_t ty = y0; ty <= y1; ty += 8)
            for (int32_t tx = x0; tx <= x1; tx += 8) {
                const int32_t x = tx + lx, y = ty + ly;
                bool in = x <= x1 && y <= y1;
                if (in) {
                    int64_t w0, w1, w2;
                    atlas_weights(t, area < 0, x, y, w0, w1, w2);
                    in = w0 >= 0 && w1 >= 0 && w2 >= 0;
                    if (in) atomicMin(A.owner + (size_t)y * A.W + (uint32_t)x, key); // (x <= x1 < W, y <= y1 < H)
                }
                pairs += (unsigned long long)__popcll(__ballot(in));
            }
    }
    if (lane == 0) {
        if (pairs) atomicAdd(A.counts, pairs);
        if (rejected) atomicAdd(A.counts + 1, (unsigned long long)rejected);
        if (degenerate) atomicAdd(A.counts + 2, (unsigned long long)degenerate);
    }
}

// flag[t] = texel t is owned; index[t] = t, what the selection compacts
__global__ __launch_bounds__(256) void atlas_flag_kernel(const uint32_t* owner, uint8_t* flag, uint32_t* index, uint32_t total)
{
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
        flag[t] = gld(owner + t) != PRT_ATLAS_NO_OWNER ? 1 : 0;
        index[t] = t;
    }
}

struct HitsArgs {
    AtlasMeshes M;
    uint32_t W, H;
    const uint32_t* owner;
    const uint32_t* texels; // the selection's output and
    const uint32_t* n;      // its count
    prt_hit* hits;
};

// The owner's triangle once more, at the one texel centre the record is for: nothing but the key was kept of the sweep.
__global__ __launch_bounds__(256) void atlas_hits_kernel(HitsArgs A)
{
    const uint32_t n = min(gld(A.n), A.W * A.H);
    const float sx = (float)(256u * A.W), sy = (float)(256u * A.H);
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n; q += gridDim.x * 256u) {
        const uint32_t texel = gld(A.texels + q);
        if (texel >= A.W * A.H) continue; // (the selection writes indices below W*H only)
        const uint32_t key = gld(A.owner + texel);
        const uint32_t m = (key >> 28) & (PRT_MAX_BVH - 1), prim = key & (PRT_ATLAS_MAX_PRIMS - 1u);
        if (key == PRT_ATLAS_NO_OWNER || !A.M.uv[m] || prim >= A.M.first[m + 1] - A.M.first[m]) continue; // (a selected texel has an owner)
        SnapTri t;
        atlas_snap(A.M.uv[m] + 6 * (size_t)prim, sx, sy, t);
        const int64_t area = atlas_area(t);
        int64_t w0, w1, w2;
        atlas_weights(t, area < 0, (int32_t)(texel % A.W), (int32_t)(texel / A.W), w0, w1, w2);
        const float a = (float)(area < 0 ? -area : area); // int64 to f32: to nearest even
        prt_hit o;
        o.t = 0.0f; o.i = (float)w0 / a; o.j = (float)w1 / a; o.k = (float)w2 / a;
        o.primId = prim;
        o.meshId = m;
        A.hits[q] = o;
    }
}

// ============================================================================ points
struct PointsArgs {
    DevScene sc;
    uint32_t primCount[PRT_MAX_BVH]; // triangles per mesh: the range of a caller's primId
    uint32_t n, W, setTile;
    float bias;
    const uint32_t* texels;
    const prt_hit* hits;
    const uint32_t* inv;
    float4* points; // 2 x float4 per point: {P, bias} {N, set}
};

__global__ __launch_bounds__(256) void atlas_points_kernel(PointsArgs A)
{
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < A.n; r += gridDim.x * 256u) {
        const prt_hit in = A.hits[r];
        uint32_t slot = 0xffffffffu;
        // every index from caller memory is checked before it becomes an address, as query_surface_kernel checks it
        if (in.meshId < A.sc.bvhCount && in.primId < A.primCount[in.meshId]) slot = gld(A.inv + A.sc.primBase[in.meshId] + in.primId);
        float4* q = A.points + 2 * (size_t)r;
        if (slot == 0xffffffffu) { // the point prt_hip_bake never follows
            gst4(q, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            gst4(q + 1, make_float4(0.0f, 0.0f, 0.0f, asf(0xffffffffu)));
            continue;
        }
        const float* p = A.sc.tris + 9 * (size_t)slot;
        const Vec3 p0 = mk3(gld(p), gld(p + 1), gld(p + 2)), p1 = mk3(gld(p + 3), gld(p + 4), gld(p + 5)), p2 = mk3(gld(p + 6), gld(p + 7), gld(p + 8));
        const Vec3 P = add3(add3(scale3(in.i, p0), scale3(in.j, p1)), scale3(in.k, p2));
        DevHit h;
        h.t = 0.0f; h.i = in.i; h.j = in.j; h.k = in.k;
        h.primId = slot;
        h.meshId = in.meshId;
        Traffic tr{};
        Surface s;
        get_surface<false>(A.sc, h, s, tr);
        const uint32_t texel = gld(A.texels + r);
        const uint32_t x = texel % A.W, y = texel / A.W;
        const uint32_t set = (x % A.setTile) + A.setTile * (y % A.setTile);
        gst4(q, make_float4(P.x, P.y, P.z, A.bias));
        gst4(q + 1, make_float4(s.normal.x, s.normal.y, s.normal.z, asf(set)));
    }
}

// ============================================================================ resolve
struct ResolveArgs {
    uint32_t W, H, n, stride;
    const uint32_t* texels;
    const float* values;
    float* image;  // W*H*stride, +0 before the scatter
    uint8_t* mask; // W*H, 0 before the scatter
};

// One lane per float of values: a wave reads 256 contiguous bytes.  An index at or beyond W*H is ignored.
__global__ __launch_bounds__(256) void atlas_scatter_kernel(ResolveArgs A)
{
    const uint64_t floats = (uint64_t)A.n * A.stride;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < floats; e += (uint64_t)gridDim.x * 256u) {
        const uint32_t q = (uint32_t)(e / A.stride), f = (uint32_t)(e - (uint64_t)q * A.stride);
        const uint32_t texel = gld(A.texels + q);
        if (texel >= A.W * A.H) continue;
        A.image[(size_t)texel * A.stride + f] = gld(A.values + e);
        if (f == 0) A.mask[texel] = 1;
    }
}

// Pass g, in place, one lane per texel.  A texel is READ (mask and floats) only while its mask is in 1 .. g and WRITTEN only while
// its mask is 0, and a written texel's mask becomes g + 1: a lane that looks at a neighbour being filled in this pass sees 0 or
// g + 1, passes it over either way and never reads its floats.  So no lane reads what another writes, and no second buffer is needed.
__global__ __launch_bounds__(256) void atlas_gutter_kernel(ResolveArgs A, uint32_t g)
{
    const uint32_t total = A.W * A.H;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
        if (A.mask[t] != 0) continue;
        const int32_t x = (int32_t)(t % A.W), y = (int32_t)(t / A.W);
        uint32_t from = 0, count = 0; // bit 3 * (dy + 1) + (dx + 1)
#pragma unroll
        for (int32_t dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int32_t dx = -1; dx <= 1; dx++) {
                const int32_t nx = x + dx, ny = y + dy;
                if (nx < 0 || ny < 0 || nx >= (int32_t)A.W || ny >= (int32_t)A.H) continue;
                const uint32_t mk = A.mask[(size_t)ny * A.W + (uint32_t)nx];
                if (mk >= 1 && mk <= g) {
                    from |= 1u << (3 * (dy + 1) + (dx + 1));
                    count++;
                }
            }
        if (count == 0) continue;
        const float div = (float)count;
        for (uint32_t f = 0; f < A.stride; f++) {
            float s = 0.0f;
#pragma unroll
            for (int32_t dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int32_t dx = -1; dx <= 1; dx++)
                    if (from & (1u << (3 * (dy + 1) + (dx + 1)))) s = s + gld(A.image + ((size_t)(y + dy) * A.W + (uint32_t)(x + dx)) * A.stride + f);
            A.image[(size_t)t * A.stride + f] = s / div;
        }
        A.mask[t] = (uint8_t)(g + 1);
    }
}

// ============================================================================ host side
uint32_t atlas_blocks(const prt_hip_ctx* c, uint64_t wanted)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(wanted, (uint64_t)std::max(c->computeUnits, 1) * PRT_ATLAS_BLOCKS_PER_CU));
}

int check_size(uint32_t W, uint32_t H, const char* what)
{
    if (W < 1 || W > PRT_ATLAS_MAX_DIM || H < 1 || H > PRT_ATLAS_MAX_DIM) return fail(PRT_HIP_EINVAL, std::string(what) + ": W and H must be 1 .. 8192");
    return PRT_HIP_OK;
}

// ---------------------------------------------------------------------------- rasterise
// Every refusal of the mesh records; M->uv are the caller's pointers by meshId, M->first the running triangle counts.
int check_meshes(uint32_t count, const prt_atlas_mesh* meshes, AtlasMeshes* M)
{
    if (count < 1 || count > PRT_HIP_MAX_BVH) return fail(PRT_HIP_EINVAL, "atlas_rasterize: count must be 1 .. PRT_HIP_MAX_BVH");
    uint32_t prims[PRT_MAX_BVH] = {};
    *M = AtlasMeshes{};
    for (uint32_t k = 0; k < count; k++) {
        const prt_atlas_mesh& m = meshes[k];
        if (m.meshId >= PRT_HIP_MAX_BVH) return fail(PRT_HIP_EINVAL, "atlas_rasterize: meshId must be below PRT_HIP_MAX_BVH");
        if (M->uv[m.meshId]) return fail(PRT_HIP_EINVAL, "atlas_rasterize: a meshId may be named once");
        if (m.primCount < 1 || m.primCount > PRT_ATLAS_MAX_PRIMS) return fail(PRT_HIP_EINVAL, "atlas_rasterize: primCount must be 1 .. 2^28");
        if (!m.uv) return prt_null_argument("atlas_rasterize");
        M->uv[m.meshId] = m.uv;
        prims[m.meshId] = m.primCount;
    }
    for (uint32_t m = 0; m < PRT_MAX_BVH; m++) M->first[m + 1] = M->first[m] + prims[m];
    return PRT_HIP_OK;
}

// The four kernels and the selection on the context's stream, and the counters on their way to the pinned copy: M, texels and hits
// are device memory.
int launch_rasterize(prt_hip_ctx* c, uint32_t W, uint32_t H, const AtlasMeshes& M, uint32_t* texels, prt_hit* hits)
{
    hipStream_t s = c->stream;
    const uint32_t total = W * H;
    HIP_TRY(c->atOwner.grow(total, s));
    HIP_TRY(c->atFlag.grow(total, s));
    HIP_TRY(c->atIndex.grow(total, s));
    HIP_TRY(c->atCounts.fit(4, s));
    HIP_TRY(c->atCountsHost.fit(4));
    uint32_t* d_n = (uint32_t*)(c->atCounts + 3);
    size_t bytes = 0;
    HIP_TRY(prt_select_flagged(nullptr, bytes, c->atIndex, c->atFlag, texels, d_n, total, s));
    HIP_TRY(c->atTemp.grow(bytes, s));
    HIP_TRY(hipMemsetAsync(c->atOwner, 0xff, (size_t)total * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(c->atCounts, 0, 4 * sizeof(unsigned long long), s));
    int rc;
    RasterArgs R{M, W, H, c->atOwner, c->atCounts};
    hipLaunchKernelGGL(atlas_raster_kernel, dim3(atlas_blocks(c, (M.first[PRT_MAX_BVH] + 3) / 4)), dim3(256), 0, s, R);
    if ((rc = prt_launched("atlas_raster_kernel"))) return rc;
    const uint32_t perTexel = atlas_blocks(c, (total + 255u) / 256u);
    hipLaunchKernelGGL(atlas_flag_kernel, dim3(perTexel), dim3(256), 0, s, (const uint32_t*)c->atOwner, (uint8_t*)c->atFlag, (uint32_t*)c->atIndex, total);
    if ((rc = prt_launched("atlas_flag_kernel"))) return rc;
    bytes = c->atTemp.size();
    HIP_TRY(prt_select_flagged(c->atTemp, bytes, c->atIndex, c->atFlag, texels, d_n, total, s));
    HitsArgs Hh{M, W, H, c->atOwner, texels, d_n, hits};
    hipLaunchKernelGGL(atlas_hits_kernel, dim3(perTexel), dim3(256), 0, s, Hh);
    if ((rc = prt_launched("atlas_hits_kernel"))) return rc;
    HIP_TRY(hipMemcpyAsync(c->atCountsHost, c->atCounts, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return PRT_HIP_OK;
}

// After the stream has been synchronised behind launch_rasterize
void read_counts(const prt_hip_ctx* c, prt_atlas_counts* out)
{
    const unsigned long long* h = c->atCountsHost;
    out->n = (uint32_t)h[3];
    out->rejected = (uint32_t)h[1];
    out->degenerate = (uint32_t)h[2];
    out->reserved = 0;
    out->pairs = h[0];
}

// ---------------------------------------------------------------------------- points
int launch_points(prt_hip_ctx* c, uint32_t n, uint32_t W, const uint32_t* texels, const prt_hit* hits, const prt_atlas_point_params& p,
                  prt_bake_point* points)
{
    int rc = prt_query_inverse_ready(c);
    if (rc) return rc;
    PointsArgs A{};
    A.sc = c->sc;
    prt_query_prim_counts(c, A.primCount);
    A.n = n;
    A.W = W;
    A.setTile = p.setTile;
    A.bias = p.bias;
    A.texels = texels;
    A.hits = hits;
    A.inv = c->qInv;
    A.points = (float4*)points;
    hipLaunchKernelGGL(atlas_points_kernel, dim3(atlas_blocks(c, (n + 255u) / 256u)), dim3(256), 0, c->stream, A);
    return prt_launched("atlas_points_kernel");
}

// ---------------------------------------------------------------------------- resolve
int launch_resolve(prt_hip_ctx* c, const ResolveArgs& A, uint32_t gutter)
{
    hipStream_t s = c->stream;
    const size_t total = (size_t)A.W * A.H;
    HIP_TRY(hipMemsetAsync(A.image, 0, total * A.stride * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(A.mask, 0, total, s));
    int rc;
    hipLaunchKernelGGL(atlas_scatter_kernel, dim3(atlas_blocks(c, ((uint64_t)A.n * A.stride + 255u) / 256u)), dim3(256), 0, s, A);
    if ((rc = prt_launched("atlas_scatter_kernel"))) return rc;
    for (uint32_t g = 1; g <= gutter; g++) {
        hipLaunchKernelGGL(atlas_gutter_kernel, dim3(atlas_blocks(c, (total + 255u) / 256u)), dim3(256), 0, s, A, g);
        if ((rc = prt_launched("atlas_gutter_kernel"))) return rc;
    }
    return PRT_HIP_OK;
}

} // namespace

extern "C" {

int prt_hip_atlas_rasterize(prt_hip_ctx* c, uint32_t W, uint32_t H, uint32_t count, const prt_atlas_mesh* meshes, uint32_t* texels,
                            prt_hit* hits, prt_atlas_counts* counts, uint32_t flags, void* stream)
{
    if (!c || !meshes || !texels || !hits || !counts) return prt_null_argument("atlas_rasterize");
    AtlasMeshes M;
    int rc;
    if ((rc = prt_check_flags(flags, "atlas_rasterize")) || (rc = check_size(W, H, "atlas_rasterize")) || (rc = check_meshes(count, meshes, &M))) return rc;
    // texels and hits have room for W*H entries; the per-mesh uv arrays follow, by meshId
    PrtIoArray io[2 + PRT_MAX_BVH] = {prt_io_out(texels, (size_t)W * H * sizeof(uint32_t), 4), prt_io_out(hits, (size_t)W * H * sizeof(prt_hit), 4)};
    for (uint32_t m = 0; m < PRT_MAX_BVH; m++) io[2 + m] = prt_io_in(M.uv[m], 6 * (size_t)(M.first[m + 1] - M.first[m]) * sizeof(float), 4);
    return prt_run_io(c, flags, stream, "atlas_rasterize: uv, texels and hits must be 4-byte aligned", io, 2 + PRT_MAX_BVH, [&]() {
        for (uint32_t m = 0; m < PRT_MAX_BVH; m++) M.uv[m] = io[2 + m].as<float>();
        if (int e = launch_rasterize(c, W, H, M, io[0].as<uint32_t>(), io[1].as<prt_hit>())) return e;
        HIP_TRY(hipStreamSynchronize(c->stream)); // the one synchronous step: a bake needs n on the host
        read_counts(c, counts);
        io[0].bytes = (size_t)counts->n * sizeof(uint32_t); // entries at and beyond n stay as the caller left them
        io[1].bytes = (size_t)counts->n * sizeof(prt_hit);
        return PRT_HIP_OK;
    });
}

int prt_hip_atlas_points(prt_hip_ctx* c, uint32_t n, uint32_t W, const uint32_t* texels, const prt_hit* hits, const prt_atlas_point_params* params,
                         prt_bake_point* points, uint32_t flags, void* stream)
{
    if (!c || !texels || !hits || !params || !points) return prt_null_argument("atlas_points");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "atlas_points: upload a scene first");
    int rc = prt_check_flags(flags, "atlas_points");
    if (rc) return rc;
    if (n < 1 || n > PRT_ATLAS_MAX_RECORDS) return fail(PRT_HIP_EINVAL, "atlas_points: n must be 1 .. 2^26");
    if (W < 1 || W > PRT_ATLAS_MAX_DIM) return fail(PRT_HIP_EINVAL, "atlas_points: W must be 1 .. 8192");
    const prt_atlas_point_params p = *params;
    if (p.setTile < 1 || p.setTile > PRT_ATLAS_MAX_TILE) return fail(PRT_HIP_EINVAL, "atlas_points: setTile must be 1 .. 32");
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return fail(PRT_HIP_EINVAL, "atlas_points: reserved must be 0");
    PrtIoArray io[3] = {prt_io_in(texels, (size_t)n * sizeof(uint32_t), 4), prt_io_in(hits, (size_t)n * sizeof(prt_hit), 4),
                        prt_io_out(points, (size_t)n * sizeof(prt_bake_point), 16)};
    return prt_run_io(c, flags, stream, "atlas_points: points must be 16-byte aligned, texels and hits 4-byte aligned", io, 3,
                      [&]() { return launch_points(c, n, W, io[0].as<uint32_t>(), io[1].as<prt_hit>(), p, io[2].as<prt_bake_point>()); });
}

int prt_hip_atlas_resolve(prt_hip_ctx* c, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, const float* values, uint32_t stride,
                          uint32_t gutter, float* image, uint8_t* mask, uint32_t flags, void* stream)
{
    if (!c || !texels || !values || !image) return prt_null_argument("atlas_resolve");
    int rc;
    if ((rc = prt_check_flags(flags, "atlas_resolve")) || (rc = check_size(W, H, "atlas_resolve"))) return rc;
    if (n < 1 || n > PRT_ATLAS_MAX_RECORDS) return fail(PRT_HIP_EINVAL, "atlas_resolve: n must be 1 .. 2^26");
    if (stride < 1 || stride > PRT_ATLAS_MAX_STRIDE) return fail(PRT_HIP_EINVAL, "atlas_resolve: stride must be 1 .. 48");
    if (gutter > PRT_ATLAS_MAX_GUTTER) return fail(PRT_HIP_EINVAL, "atlas_resolve: gutter must be 0 .. 64");
    const size_t total = (size_t)W * H;
    PrtIoArray io[4] = {prt_io_in(texels, (size_t)n * sizeof(uint32_t), 4), prt_io_in(values, (size_t)n * stride * sizeof(float), 4),
                        prt_io_out(image, total * stride * sizeof(float), 4), prt_io_out(mask, total, 1)};
    return prt_run_io(c, flags, stream, "atlas_resolve: texels, values and image must be 4-byte aligned", io, 4, [&]() {
        ResolveArgs A{W, H, n, stride, io[0].as<uint32_t>(), io[1].as<float>(), io[2].as<float>(), io[3].as<uint8_t>()};
        if (!A.mask) { // the passes need one: the context's
            HIP_TRY(c->atScratchMask.grow(total, c->stream));
            A.mask = c->atScratchMask;
        }
        return launch_resolve(c, A, gutter);
    });
}

} // extern "C"
