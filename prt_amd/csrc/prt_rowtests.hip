// prt_rowtests.hip -- the kernels and entry points of the row-level parity tests (include/prt_hip_test.h): batches of the caller's rays
// through every traversal mode, single leaf / box / camera / math rows, texture taps and surface records.  Only in the test build of
// the library (-DPRT_TEST_ENTRY_POINTS -> libprt_hip_test.so): the product library exports neither these kernels nor their entry
// points, and the file is empty there.  In a translation unit of its own so that the frame kernel's (prt_kernels.hip) holds the same
// code in both builds.
#ifdef PRT_TEST_ENTRY_POINTS
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "prt_internal.h"
#include "prt_lanes.h"
#include "../../include/prt_hip_test.h"

namespace {
int fail(int code, const std::string& msg) { return prt_fail(code, msg); }
} // namespace

// ============================================================================ row-level test kernels
struct RaysArgs {
    DevScene sc;
    uint32_t n;
    const float* org;
    const float* dir;
    float maxT;
    prt_hit* hits;
    BatchCtl ctl;
};

struct ArraySrc {
    const RaysArgs* A;
    int mode;
    __device__ __forceinline__ uint32_t count() const { return A->n; }
    __device__ __forceinline__ uint32_t* cursor() const { return A->ctl.cursor; }
    __device__ __forceinline__ void load(uint32_t i, Vec3& org, Vec3& dir, float& maxT, uint32_t& rev) const
    {
        org = mk3(A->org[3 * i], A->org[3 * i + 1], A->org[3 * i + 2]);
        dir = mk3(A->dir[3 * i], A->dir[3 * i + 1], A->dir[3 * i + 2]);
        maxT = A->maxT;
        rev = 0;
        if (mode == PRT_MODE_PACKET) { // avgDir = lane-ordered sum of the packet's 8 directions / 8 (camera.cpp:56,70)
            uint32_t g = i & ~7u;
            Vec3 avg = mk3(0, 0, 0);
            for (uint32_t l = 0; l < 8; l++) avg = add3(avg, mk3(A->dir[3 * (g + l)], A->dir[3 * (g + l) + 1], A->dir[3 * (g + l) + 2]));
            avg = div3s(avg, 8.0f);
            rev = (avg.x < 0.0f ? 1u : 0u) | (avg.y < 0.0f ? 2u : 0u) | (avg.z < 0.0f ? 4u : 0u);
        }
    }
    __device__ __forceinline__ void store_hit(uint32_t i, const DevHit& h) const
    {
        prt_hit o;
        // the device names a hit triangle by its leaf-order index; the reference's primId is that triangle's index in its mesh
        // (a NaN limit keeps hit.t NaN: no triangle was recorded and primId is not an index)
        o.t = h.t; o.i = h.i; o.j = h.j; o.k = h.k;
        o.primId = (h.t != -1.0f && h.t == h.t) ? gld(A->sc.triPrim + h.primId) : h.primId;
        o.meshId = h.meshId;
        A->hits[i] = o;
    }
    __device__ __forceinline__ void store_occ(uint32_t i, bool occ) const
    {
        prt_hit o;
        o.t = occ ? 1.0f : 0.0f; o.i = o.j = o.k = 0.0f; o.primId = 0; o.meshId = 0;
        A->hits[i] = o;
    }
};

template <int MODE>
__global__ __launch_bounds__(PRT_BLOCK) void rays_kernel(RaysArgs A)
{
    ArraySrc src{&A, MODE};
    trace_batch<MODE>(A.sc, src, A.ctl);
}

__global__ void leaf_kernel(uint32_t n, const float* rec, float* out)
{
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float* p = rec + 22 * (size_t)r;
    float* q = out + 24 * (size_t)r;
    for (int k = 0; k < 24; k++) q[k] = 0.0f;
    DevRay rs, r1;
    rs.org = r1.org = mk3(p[0], p[1], p[2]);
    rs.dir = r1.dir = mk3(p[3], p[4], p[5]);
    Vec3 p0 = mk3(p[6], p[7], p[8]), p1 = mk3(p[9], p[10], p[11]), p2 = mk3(p[12], p[13], p[14]);
    Box b{mk3(p[15], p[16], p[17]), mk3(p[18], p[19], p[20])};
    float maxT = p[21];
    prepare_soa(rs);
    prepare_single(r1);
    float bi, bj, bk;
    float t = tri_intersect(rs, p0, p1, p2, bi, bj, bk);
    q[0] = t;
    if (t != -1.0f) { q[1] = bi; q[2] = bj; q[3] = bk; }
    t = tri_intersect(r1, p0, p1, p2, bi, bj, bk);
    q[4] = t;
    if (t != -1.0f) { q[5] = bi; q[6] = bj; q[7] = bk; }
    q[12] = box_t(b, r1);
    q[13] = box_bool(b, r1, maxT) ? 1.0f : 0.0f;
    q[14] = box_soa(b, rs, maxT) ? 1.0f : 0.0f;
    q[16] = rs.inv.x; q[17] = rs.inv.y; q[18] = rs.inv.z;
    q[19] = rs.swapXZ ? 1.0f : 0.0f;
    q[20] = rs.swapYZ ? 1.0f : 0.0f;
    q[21] = r1.swapXZ ? 1.0f : 0.0f;
    q[22] = r1.swapYZ ? 1.0f : 0.0f;
}

__global__ void sincos_kernel(uint32_t n, const float* theta, float* s, float* c)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sn, cs;
    prt_sincosf(theta[i], &sn, &cs);
    s[i] = sn;
    c[i] = cs;
}

__global__ void powf_kernel(uint32_t n, const float* x, float* y)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = prt_powf_2p2(x[i]);
}

__global__ void camera_kernel(DevCamera cam, uint32_t x, uint32_t y, uint32_t state, float* out)
{
    uint32_t lane = threadIdx.x & 63u, slot = lane & 7u, gbase = lane & ~7u;
    uint32_t rng = state;
    DevRay r;
    Vec3 avg;
    camera_packet(cam, rng, x, y, slot, gbase, r, avg);
    if (lane < 8) {
        float* q = out + 11 * slot;
        q[0] = r.org.x; q[1] = r.org.y; q[2] = r.org.z;
        q[3] = r.dir.x; q[4] = r.dir.y; q[5] = r.dir.z;
        q[6] = r.inv.x; q[7] = r.inv.y; q[8] = r.inv.z;
        q[9] = r.swapXZ ? 1.0f : 0.0f;
        q[10] = r.swapYZ ? 1.0f : 0.0f;
    }
    if (lane == 0) {
        out[88] = avg.x; out[89] = avg.y; out[90] = avg.z;
        out[91] = asf(rng);
    }
}

// Texture taps on the uploaded scene's own arrays (texture.cpp:31-183, material.cpp:87-96).  rec: {material (global), u, v, flags};
// out: 12 words per record (include/prt_hip_test.h).  classOf = per texture its first alpha class word (PrtEdit::classWordOf); the
// host has checked every record's material, maps and class words.  A grid-stride loop: any grid covers any n.
template <bool COUNT>
__global__ __launch_bounds__(256) void taps_kernel(DevScene sc, const uint32_t* classOf, uint32_t n, const uint32_t* rec, uint32_t* out)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t* p = rec + 4 * (size_t)r;
        uint32_t* q = out + 12 * (size_t)r;
        const uint32_t mat = p[0], flags = p[3];
        const Vec2 uv = Vec2{asf(p[1]), asf(p[2])};
        Traffic tr{};
        const float4* mp = sc.mats + PRT_MAT_STRIDE * (size_t)mat;
        const float4 m2 = gld4(mp + 2), m3 = gld4(mp + 3), m4 = gld4(mp + 4);
        const uint4 dd = make_uint4(asu(m3.x), asu(m3.y), asu(m3.z), asu(m3.w)), bd = make_uint4(asu(m4.x), asu(m4.y), asu(m4.z), asu(m4.w));
        for (int k = 0; k < 12; k++) q[k] = 0u;
        if (flags & 1u) {
            const Vec3 c = tex_sample3<COUNT>(sc, dd, uv, tr);
            q[0] = asu(c.x); q[1] = asu(c.y); q[2] = asu(c.z);
            q[3] = asu(tex_sample1<COUNT>(sc, bd, uv, tr));
            const Vec3 s = sample_diffuse<COUNT>(sc, mat, uv, tr);
            q[6] = asu(s.x); q[7] = asu(s.y); q[8] = asu(s.z);
        }
        if (flags & 2u) {
            const float base = asf(classOf[asu(m2.x)]);
            if (flags & 1u) q[4] = alpha_decide<false>(sc, dd, base, uv, tr) ? 1u : 0u;
            q[5] = alpha_decide<true>(sc, dd, base, uv, tr) ? 1u : 0u;
        }
        q[9] = COUNT ? tr.nTap : 0u;
    }
}

// Mesh::getSurfaceProperties + Material::sampleBump (mesh.cpp:311-364, material.cpp:98-114) on the uploaded scene's own records.
// rec: {mesh, triangle slot, i, j, k} (the host has turned the mesh-order primId into the slot and checked both); out: 20 words.
template <bool COUNT>
__global__ __launch_bounds__(256) void surface_kernel(DevScene sc, uint32_t anyBump, uint32_t n, const uint32_t* rec, uint32_t* out)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t* p = rec + 5 * (size_t)r;
        uint32_t* q = out + 20 * (size_t)r;
        Traffic tr{};
        DevHit h;
        h.t = 1.0f; h.i = asf(p[2]); h.j = asf(p[3]); h.k = asf(p[4]);
        h.primId = p[1]; h.meshId = p[0];
        Surface s;
        get_surface<COUNT>(sc, h, s, tr);
        for (int k = 0; k < 20; k++) q[k] = 0u;
        q[0] = asu(s.normal.x); q[1] = asu(s.normal.y); q[2] = asu(s.normal.z);
        q[3] = asu(s.uv.x); q[4] = asu(s.uv.y);
        q[5] = s.mat;
        if (anyBump) { // the bump record of the slot: dp01.xyz duv01.x | dp02.xyz duv01.y | duv02.xy (prt_upload.hip)
            const float4* bp = sc.bump + 3 * (size_t)s.prim;
            const float4 b0 = gld4(bp), b1 = gld4(bp + 1), b2 = gld4(bp + 2);
            q[6] = asu(b0.w); q[7] = asu(b1.w); q[8] = asu(b2.x); q[9] = asu(b2.y);
            q[10] = asu(b0.x); q[11] = asu(b0.y); q[12] = asu(b0.z);
            q[13] = asu(b1.x); q[14] = asu(b1.y); q[15] = asu(b1.z);
        }
        const Vec3 bn = sample_bump<COUNT>(sc, s.mat, s, tr);
        q[16] = asu(bn.x); q[17] = asu(bn.y); q[18] = asu(bn.z);
        q[19] = COUNT ? tr.nTap : 0u;
    }
}

// ============================================================================ host side of the C-ABI
// (the device scratch of a test call is a DevBuf of its own: freed on every return path)
extern "C" {

int prt_hip_test_occlusion_skipped(prt_hip_ctx* c, uint64_t* skipped)
{
    if (!c || !skipped) return fail(PRT_HIP_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> all((size_t)PRT_STAT_SHARDS * PRT_STAT_STRIDE);
    HIP_TRY(hipMemcpy(all.data(), c->counters, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (int sh = 0; sh < PRT_STAT_SHARDS; sh++) n += all[(size_t)sh * PRT_STAT_STRIDE + PRT_STAT_OCCL_SKIPPED];
    *skipped = n;
    return PRT_HIP_OK;
}

int prt_hip_trace_rays(prt_hip_ctx* c, int mode, uint32_t n, const float* org, const float* dir, float maxT, prt_hit* hits)
{
    if (!c || !org || !dir || !hits) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (n == 0 || (n & 7u) || mode < 0 || mode > 3) return fail(PRT_HIP_EINVAL, "n must be a positive multiple of 8, mode 0..3");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> dorg, ddir;
    DevBuf<prt_hit> dh;
    HIP_TRY(dorg.fit((size_t)n * 3, c->stream));
    HIP_TRY(ddir.fit((size_t)n * 3, c->stream));
    HIP_TRY(dh.fit(n, c->stream));
    HIP_TRY(hipMemcpy(dorg, org, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ddir, dir, (size_t)n * 12, hipMemcpyHostToDevice));
    // every workgroup of the batch at once; timed like a render (prt_hip_get_stats reports it as kernelMs):
    // tools/ray_order_experiment.py compares orders of one batch
    BatchLaunch L;
    int rc = prt_batch_begin(c, n, (n + PRT_BLOCK - 1) / PRT_BLOCK, true, &L);
    if (rc) return rc;
    RaysArgs A{c->sc, n, dorg, ddir, maxT, dh, L.ctl};
    if (mode == 0) hipLaunchKernelGGL(rays_kernel<PRT_MODE_SINGLE>, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    else if (mode == 1) hipLaunchKernelGGL(rays_kernel<PRT_MODE_PACKET>, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    else if (mode == 2) hipLaunchKernelGGL(rays_kernel<PRT_MODE_OCC_SINGLE>, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    else hipLaunchKernelGGL(rays_kernel<PRT_MODE_OCC_PACKET>, dim3(L.blocks), dim3(PRT_BLOCK), 0, c->stream, A);
    if ((rc = prt_batch_end(c, L, "rays_kernel"))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(hits, dh, (size_t)n * sizeof(prt_hit), hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_test_leaf(prt_hip_ctx* c, uint32_t n, const float* records, float* out)
{
    if (!c || !records || !out || n == 0) return fail(PRT_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> din, dout;
    HIP_TRY(din.fit((size_t)n * 22, c->stream));
    HIP_TRY(dout.fit((size_t)n * 24, c->stream));
    HIP_TRY(hipMemcpy(din, records, (size_t)n * 22 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(leaf_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, din, dout);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 24 * 4, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_test_sincos(prt_hip_ctx* c, uint32_t n, const float* theta, float* s, float* cs)
{
    if (!c || !theta || !s || !cs || n == 0) return fail(PRT_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> dt, ds, dc;
    HIP_TRY(dt.fit(n, c->stream));
    HIP_TRY(ds.fit(n, c->stream));
    HIP_TRY(dc.fit(n, c->stream));
    HIP_TRY(hipMemcpy(dt, theta, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dt, ds, dc);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(s, ds, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cs, dc, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_test_powf(prt_hip_ctx* c, uint32_t n, const float* x, float* y)
{
    if (!c || !x || !y || n == 0) return fail(PRT_HIP_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> dx, dy;
    HIP_TRY(dx.fit(n, c->stream));
    HIP_TRY(dy.fit(n, c->stream));
    HIP_TRY(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(powf_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dx, dy);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_test_camera(prt_hip_ctx* c, uint32_t x, uint32_t y, uint32_t state, float* out92)
{
    if (!c || !out92) return fail(PRT_HIP_EINVAL, "bad argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d;
    HIP_TRY(d.fit(92, c->stream));
    hipLaunchKernelGGL(camera_kernel, dim3(1), dim3(64), 0, c->stream, c->cam, x, y, state, d);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out92, d, 92 * 4, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

// blocks of a row-level launch: the caller's, or one thread per record; at most 65535
static uint32_t row_blocks(uint32_t n, uint32_t blocks)
{
    if (blocks == 0) blocks = (n + 255u) / 256u;
    return std::min<uint32_t>(blocks, 65535u);
}

int prt_hip_test_taps(prt_hip_ctx* c, uint32_t n, const uint32_t* records, int counting, uint32_t blocks, uint32_t* out)
{
    if (!c || !records || !out || n == 0) return fail(PRT_HIP_EINVAL, "bad argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    // every address the kernel forms is checked here: the material exists, the flavours asked for have their maps and class words
    std::vector<const prt_material*> matOf(c->arr.mats.size() / PRT_MAT_STRIDE, nullptr);
    for (const PrtEditMesh& m : c->ed.meshes)
        for (size_t k = 0; k < m.materials.size(); k++)
            if (m.matBase + k < matOf.size()) matOf[m.matBase + k] = &m.materials[k];
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t mat = records[4 * (size_t)r], flags = records[4 * (size_t)r + 3];
        if (mat >= matOf.size() || !matOf[mat] || (flags & ~3u)) return fail(PRT_HIP_EINVAL, "taps: bad material index or flags");
        const prt_material& mt = *matOf[mat];
        if ((flags & 1u) && (mt.diffuseMap < 0 || mt.bumpMap < 0)) return fail(PRT_HIP_EINVAL, "taps: the material lacks a diffuse or a bump map");
        if (flags & 2u) {
            if (mt.diffuseMap < 0 || (size_t)mt.diffuseMap >= c->ed.classWordOf.size() || c->ed.classWordOf[mt.diffuseMap] == 0xffffffffu ||
                c->ed.texDesc[mt.diffuseMap].w != 4u)
                return fail(PRT_HIP_EINVAL, "taps: alpha test asked of a material without a 4-component map whose cell classes were built");
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> din, dout, dcls;
    HIP_TRY(din.fit((size_t)n * 4, c->stream));
    HIP_TRY(dout.fit((size_t)n * 12, c->stream));
    HIP_TRY(dcls.fit(c->ed.classWordOf.size(), c->stream));
    HIP_TRY(hipMemcpy(din, records, (size_t)n * 16, hipMemcpyHostToDevice));
    if (!c->ed.classWordOf.empty()) HIP_TRY(hipMemcpy(dcls, c->ed.classWordOf.data(), c->ed.classWordOf.size() * 4, hipMemcpyHostToDevice));
    blocks = row_blocks(n, blocks);
    if (counting) hipLaunchKernelGGL(taps_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, c->sc, dcls, n, din, dout);
    else hipLaunchKernelGGL(taps_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, c->sc, dcls, n, din, dout);
    int rc = prt_launched("taps_kernel");
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 48, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}

int prt_hip_test_surface(prt_hip_ctx* c, uint32_t n, const uint32_t* records, int counting, uint32_t blocks, uint32_t* out)
{
    if (!c || !records || !out || n == 0) return fail(PRT_HIP_EINVAL, "bad argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // mesh-order primId -> triangle slot, from the arrays the upload left on the device (a pad slot names no vertices)
    const size_t slots = c->rf.slotVtx.size() / 3;
    std::vector<uint32_t> triPrim(slots), slotVtx(3 * slots);
    if (slots) {
        HIP_TRY(hipMemcpy(triPrim.data(), c->sc.triPrim, slots * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(slotVtx.data(), c->rf.slotVtx, slots * 12, hipMemcpyDeviceToHost));
    }
    std::vector<std::vector<uint32_t>> slotOf(c->rf.meshes.size());
    for (size_t m = 0; m < c->rf.meshes.size(); m++) {
        const PrtRefitMesh& rm = c->rf.meshes[m];
        if ((size_t)rm.slotBase + rm.slotCount > slots) return fail(PRT_HIP_ESTATE, "surface: slot range outside the scene");
        slotOf[m].assign(rm.slotCount, 0xffffffffu); // (primCount <= slotCount)
        for (uint32_t s = rm.slotBase; s < rm.slotBase + rm.slotCount; s++)
            if (slotVtx[3 * (size_t)s] != 0xffffffffu && triPrim[s] < rm.slotCount) slotOf[m][triPrim[s]] = s;
    }
    std::vector<uint32_t> rec(records, records + 5 * (size_t)n);
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t mesh = rec[5 * (size_t)r], prim = rec[5 * (size_t)r + 1];
        if (mesh >= slotOf.size() || mesh >= c->sc.bvhCount || prim >= slotOf[mesh].size() || slotOf[mesh][prim] == 0xffffffffu)
            return fail(PRT_HIP_EINVAL, "surface: bad mesh or primitive index");
        rec[5 * (size_t)r + 1] = slotOf[mesh][prim];
    }
    DevBuf<uint32_t> din, dout;
    HIP_TRY(din.fit((size_t)n * 5, c->stream));
    HIP_TRY(dout.fit((size_t)n * 20, c->stream));
    HIP_TRY(hipMemcpy(din, rec.data(), (size_t)n * 20, hipMemcpyHostToDevice));
    blocks = row_blocks(n, blocks);
    const uint32_t anyBump = c->arr.anyBump() ? 1u : 0u;
    if (counting) hipLaunchKernelGGL(surface_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, c->sc, anyBump, n, din, dout);
    else hipLaunchKernelGGL(surface_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, c->sc, anyBump, n, din, dout);
    int rc = prt_launched("surface_kernel");
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 80, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < n; r++) // the material as the reference names it: its index within the mesh
        out[20 * (size_t)r + 5] -= c->ed.meshes[records[5 * (size_t)r]].matBase;
    return PRT_HIP_OK;
}

} // extern "C"
#endif // PRT_TEST_ENTRY_POINTS
