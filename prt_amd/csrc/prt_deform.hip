// prt_deform.hip -- geometry updates from device memory (include/prt_hip.h "geometry updates from device memory"): the caller's vertex
// positions are read where a simulation or a skinning kernel left them, and what the host path (prt_hip_update_meshes) expects the
// caller to bring along is computed here:
//   keep     grid-stride over the vertices: the library's own copy of positions (and given normals) for prt_hip_get_mesh_vertices, and
//            the min / max of Mesh::calculateBounds, per block; a second one-block launch folds the per-block boxes.  min / max of
//            finite floats is exact and order independent (up to the sign of a zero, which the radius cannot see);
//   face     one lane per face: normalize(cross(p1 - p0, p2 - p0)), (0, 0, 0) when a component is NaN (mesh.cpp:120-126);
//   vertex   one lane per vertex: its incidence list in the order the reference's sequential loop reaches the vertex's corners
//            (faces descending, corners ascending), n = acc + fn; if (length(n) > 0) acc = n; then normalize(acc).  That loop touches
//            a vertex's accumulator at that vertex's corners only, so this is the same arithmetic in the same order;
//   sah      one lane per wide record of a mesh: the f32 areas of both child boxes into f64 sums (internal children, leaf children
//            times their triangle count), block tree in LDS, per-block partials, one final block: a fixed order, so a run repeats
//            itself bit for bit.
// The refit itself (gather, levels, finish) and everything the call invalidates are prt_refit.hip's, shared with the host path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/prt_hip.h"
#include "prt_device.h"
#include "prt_internal.h"
#ifdef PRT_TEST_ENTRY_POINTS
#include "../../include/prt_hip_test.h"
#endif

#define PRT_DEFORM_BLOCK 256
#define PRT_DEFORM_BOX_BLOCKS 512 // blocks of the keep kernel at the most (grid-stride beyond)

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

__device__ __forceinline__ void st3(float* p, uint32_t v, Vec3 a)
{
    float* q = p + 3 * (size_t)v;
    *(PRT_AS1 float*)q = a.x;
    *(PRT_AS1 float*)(q + 1) = a.y;
    *(PRT_AS1 float*)(q + 2) = a.z;
}

// the six planes of a box, one value per lane -> lane 0 holds the block's (tree over the lane index: a fixed order)
__device__ __forceinline__ void block_box(float (*sh)[PRT_DEFORM_BLOCK], Vec3& lo, Vec3& hi)
{
    const uint32_t t = threadIdx.x;
    sh[0][t] = lo.x; sh[1][t] = lo.y; sh[2][t] = lo.z;
    sh[3][t] = hi.x; sh[4][t] = hi.y; sh[5][t] = hi.z;
    __syncthreads();
    for (uint32_t w = PRT_DEFORM_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                sh[j][t] = fminf(sh[j][t], sh[j][t + w]);
                sh[3 + j][t] = fmaxf(sh[3 + j][t], sh[3 + j][t + w]);
            }
        }
        __syncthreads();
    }
    lo = mk3(sh[0][0], sh[1][0], sh[2][0]);
    hi = mk3(sh[3][0], sh[4][0], sh[5][0]);
}

// keepPos / keepNrm (either may be NULL): the library's copies; partial: 6 floats per block
__global__ __launch_bounds__(PRT_DEFORM_BLOCK) void deform_keep_kernel(const float* pos, float* keepPos, const float* nrm, float* keepNrm, uint32_t vertices,
                                                                       float* partial)
{
    __shared__ float sh[6][PRT_DEFORM_BLOCK];
    const float big = 3.402823466e+38f; // BBox::init (vecmath.cpp:46-52)
    Vec3 lo = mk3(big, big, big), hi = mk3(-big, -big, -big);
    for (uint32_t v = blockIdx.x * PRT_DEFORM_BLOCK + threadIdx.x; v < vertices; v += gridDim.x * PRT_DEFORM_BLOCK) {
        const Vec3 p = ld3(pos, v);
        lo = mk3(fminf(lo.x, p.x), fminf(lo.y, p.y), fminf(lo.z, p.z));
        hi = mk3(fmaxf(hi.x, p.x), fmaxf(hi.y, p.y), fmaxf(hi.z, p.z));
        if (keepPos) st3(keepPos, v, p);
        if (keepNrm) st3(keepNrm, v, ld3(nrm, v));
    }
    block_box(sh, lo, hi);
    if (threadIdx.x == 0) {
        float* q = partial + 6 * (size_t)blockIdx.x;
        q[0] = lo.x; q[1] = lo.y; q[2] = lo.z;
        q[3] = hi.x; q[4] = hi.y; q[5] = hi.z;
    }
}

__global__ __launch_bounds__(PRT_DEFORM_BLOCK) void deform_box_kernel(const float* partial, uint32_t blocks, float* out)
{
    __shared__ float sh[6][PRT_DEFORM_BLOCK];
    const float big = 3.402823466e+38f;
    Vec3 lo = mk3(big, big, big), hi = mk3(-big, -big, -big);
    for (uint32_t b = threadIdx.x; b < blocks; b += PRT_DEFORM_BLOCK) {
        const Vec3 l = ld3(partial, 2 * b), h = ld3(partial, 2 * b + 1);
        lo = mk3(fminf(lo.x, l.x), fminf(lo.y, l.y), fminf(lo.z, l.z));
        hi = mk3(fmaxf(hi.x, h.x), fmaxf(hi.y, h.y), fmaxf(hi.z, h.z));
    }
    block_box(sh, lo, hi);
    if (threadIdx.x == 0) {
        out[0] = lo.x; out[1] = lo.y; out[2] = lo.z;
        out[3] = hi.x; out[4] = hi.y; out[5] = hi.z;
    }
}

__global__ __launch_bounds__(PRT_DEFORM_BLOCK) void deform_face_kernel(const uint32_t* faceVtx, const float* pos, float* faceNrm, uint32_t faces)
{
    const uint32_t f = blockIdx.x * PRT_DEFORM_BLOCK + threadIdx.x;
    if (f >= faces) return;
    const Vec3 p0 = ld3(pos, gld(faceVtx + 3 * (size_t)f)), p1 = ld3(pos, gld(faceVtx + 3 * (size_t)f + 1)), p2 = ld3(pos, gld(faceVtx + 3 * (size_t)f + 2));
    Vec3 n = normalize3(cross3(sub3(p1, p0), sub3(p2, p0)));
    if (n.x != n.x || n.y != n.y || n.z != n.z) n = mk3(0.0f, 0.0f, 0.0f);
    st3(faceNrm, f, n);
}

__global__ __launch_bounds__(PRT_DEFORM_BLOCK) void deform_vertex_kernel(const uint32_t* off, const uint32_t* face, const float* faceNrm, float* nrm,
                                                                         uint32_t vertices)
{
    const uint32_t v = blockIdx.x * PRT_DEFORM_BLOCK + threadIdx.x;
    if (v >= vertices) return;
    Vec3 acc = mk3(0.0f, 0.0f, 0.0f);
    const uint32_t end = gld(off + v + 1);
    for (uint32_t k = gld(off + v); k < end; k++) {
        const Vec3 n = add3(acc, ld3(faceNrm, gld(face + k)));
        if (length3(n) > 0.0f) acc = n; // mesh.cpp:129-132
    }
    st3(nrm, v, normalize3(acc));
}

__device__ __forceinline__ float box_area(Box b) // vecmath.cpp:75-79
{
    const Vec3 e = sub3(b.hi, b.lo);
    return 2.0f * (e.x * e.y + e.y * e.z + e.z * e.x);
}

// three f64 values per lane -> lane 0 holds the block's sums (tree over the lane index)
__device__ __forceinline__ void block_sum3(double (*sh)[PRT_DEFORM_BLOCK], double& a, double& b, double& c)
{
    const uint32_t t = threadIdx.x;
    sh[0][t] = a; sh[1][t] = b; sh[2][t] = c;
    __syncthreads();
    for (uint32_t w = PRT_DEFORM_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            sh[0][t] += sh[0][t + w];
            sh[1][t] += sh[1][t + w];
            sh[2][t] += sh[2][t + w];
        }
        __syncthreads();
    }
    a = sh[0][0]; b = sh[1][0]; c = sh[2][0];
}

// list: the n records of one mesh; partial: per block {sum of area over internal children, sum of count * area over leaf children, leaf children}
__global__ __launch_bounds__(PRT_DEFORM_BLOCK) void deform_sah_kernel(const uint32_t* list, uint32_t n, const uint2* kids, const float4* wnodes, double* partial)
{
    __shared__ double sh[3][PRT_DEFORM_BLOCK];
    const uint32_t i = blockIdx.x * PRT_DEFORM_BLOCK + threadIdx.x;
    double inner = 0.0, leaf = 0.0, leaves = 0.0;
    if (i < n) {
        const uint32_t r = gld(list + i);
        const uint2 kid = gld2u(kids + r);
        const float4* rec = wnodes + 4 * (size_t)r;
        const float4 w0 = gld4(rec), w1 = gld4(rec + 1), w2 = gld4(rec + 2);
        const float a0 = box_area(Box{mk3(w0.x, w0.z, w1.x), mk3(w0.y, w0.w, w1.y)});
        const float a1 = box_area(Box{mk3(w2.x, w2.z, w1.z), mk3(w2.y, w2.w, w1.w)});
        if (kid.x & PRT_REF_LEAF) { leaf += (double)leaf_count(kid.x) * (double)a0; leaves += 1.0; } else inner += (double)a0;
        if (kid.y & PRT_REF_LEAF) { leaf += (double)leaf_count(kid.y) * (double)a1; leaves += 1.0; } else inner += (double)a1;
    }
    block_sum3(sh, inner, leaf, leaves);
    if (threadIdx.x == 0) {
        double* q = partial + 3 * (size_t)blockIdx.x;
        q[0] = inner; q[1] = leaf; q[2] = leaves;
    }
}

__global__ __launch_bounds__(PRT_DEFORM_BLOCK) void deform_sah_final_kernel(const double* partial, uint32_t blocks, double* out)
{
    __shared__ double sh[3][PRT_DEFORM_BLOCK];
    double inner = 0.0, leaf = 0.0, leaves = 0.0;
    for (uint32_t b = threadIdx.x; b < blocks; b += PRT_DEFORM_BLOCK) {
        inner += partial[3 * (size_t)b];
        leaf += partial[3 * (size_t)b + 1];
        leaves += partial[3 * (size_t)b + 2];
    }
    block_sum3(sh, inner, leaf, leaves);
    if (threadIdx.x == 0) {
        out[0] = inner; out[1] = leaf; out[2] = leaves;
    }
}

uint32_t blocks_of(uint32_t n) { return (n + PRT_DEFORM_BLOCK - 1) / PRT_DEFORM_BLOCK; }

uint32_t sah_blocks_max(const prt_hip_ctx* c) { return (uint32_t)(c->arr.wnodes.size() / 4 / PRT_DEFORM_BLOCK + 1); } // (4 float4 per record)

// the scratch arrays of this file (kept with the scene)
int scratch_ready(prt_hip_ctx* c)
{
    PrtRefit& R = c->rf;
    if (!R.vboxOut) HIP_TRY(R.vboxOut.fit(PRT_MAX_BVH * 6, c->stream));
    if (!R.boxPartial) HIP_TRY(R.boxPartial.fit(PRT_DEFORM_BOX_BLOCKS * 6, c->stream));
    if (!R.sahPartial) HIP_TRY(R.sahPartial.fit(3 * ((size_t)sah_blocks_max(c) + 1), c->stream)); // (the last three: the sums)
    HIP_TRY(R.vboxHost.fit(PRT_MAX_BVH * 6));
    return PRT_HIP_OK;
}

// keep + box of one mesh on s: the box of `pos` lands in vboxOut[mesh]
int queue_box(prt_hip_ctx* c, uint32_t mesh, const float* pos, float* keepPos, const float* nrm, float* keepNrm, hipStream_t s)
{
    PrtRefit& R = c->rf;
    const PrtRefitMesh& M = R.meshes[mesh];
    const uint32_t blocks = std::max(1u, std::min<uint32_t>(blocks_of(M.vertexCount), PRT_DEFORM_BOX_BLOCKS));
    hipLaunchKernelGGL(deform_keep_kernel, dim3(blocks), dim3(PRT_DEFORM_BLOCK), 0, s, pos, keepPos, nrm, keepNrm, M.vertexCount, R.boxPartial);
    int rc = prt_launched("deform_keep_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(deform_box_kernel, dim3(1), dim3(PRT_DEFORM_BLOCK), 0, s, R.boxPartial, blocks, R.vboxOut + 6 * mesh);
    return prt_launched("deform_box_kernel");
}

// {internal children's area, leaf children's count * area, leaf children} of the mesh's records as they stand; synchronises the context's stream
int sah_sums(prt_hip_ctx* c, uint32_t mesh, double out[3])
{
    PrtRefit& R = c->rf;
    const PrtRefitMesh& M = R.meshes[mesh];
    out[0] = out[1] = out[2] = 0.0;
    uint32_t n = 0;
    for (const auto& l : M.levels) n += l.second;
    if (n == 0) return PRT_HIP_OK; // the root is a leaf
    int rc = scratch_ready(c);
    if (rc) return rc;
    const uint32_t blocks = blocks_of(n);
    if (blocks > sah_blocks_max(c)) return fail(PRT_HIP_EINVAL, "internal: more records in a mesh than in the scene");
    double* sums = R.sahPartial + 3 * (size_t)sah_blocks_max(c);
    hipLaunchKernelGGL(deform_sah_kernel, dim3(blocks), dim3(PRT_DEFORM_BLOCK), 0, c->stream, R.levelList + M.levels[0].first, n, R.kids, c->sc.wnodes, R.sahPartial);
    if ((rc = prt_launched("deform_sah_kernel"))) return rc;
    hipLaunchKernelGGL(deform_sah_final_kernel, dim3(1), dim3(PRT_DEFORM_BLOCK), 0, c->stream, R.sahPartial, blocks, sums);
    if ((rc = prt_launched("deform_sah_final_kernel"))) return rc;
    HIP_TRY(hipMemcpyAsync(out, sums, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRT_HIP_OK;
}

float host_area(const float* b)
{
    const float ex = b[3] - b[0], ey = b[4] - b[1], ez = b[5] - b[2];
    return 2.0f * (ex * ey + ey * ez + ez * ex);
}

// {internalArea, leafArea, rootArea} and the node counts of the mesh's tree as it stands (the root's own box is added here)
int sah_of(prt_hip_ctx* c, uint32_t mesh, double area[3], uint32_t* internalNodes, uint32_t* leaves)
{
    const PrtRefitMesh& M = c->rf.meshes[mesh];
    double s[3];
    int rc = sah_sums(c, mesh, s);
    if (rc) return rc;
    const double root = (double)host_area(c->sc.rootBox[mesh]);
    uint32_t n = 0;
    for (const auto& l : M.levels) n += l.second;
    if (M.rootKid & PRT_REF_LEAF) {
        area[0] = 0.0;
        area[1] = (double)((M.rootKid & 7u) + 1u) * root;
        if (leaves) *leaves = 1;
    } else {
        area[0] = s[0] + root;
        area[1] = s[1];
        if (leaves) *leaves = (uint32_t)s[2];
    }
    area[2] = root;
    if (internalNodes) *internalNodes = n;
    return PRT_HIP_OK;
}

// The incidence list of the mesh, from the device's own tables: the index buffer is what the leaves' slots (slotVtx) say about the
// triangles they hold (triPrim).  PRT_HIP_EINVAL when the leaves do not name every triangle exactly once.
int csr_ready(prt_hip_ctx* c, uint32_t mesh)
{
    PrtRefit& R = c->rf;
    PrtRefitMesh& M = R.meshes[mesh];
    if (M.csrOff) return PRT_HIP_OK;
    std::vector<uint32_t> slotVtx((size_t)M.slotCount * 3), triPrim(M.slotCount);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (M.slotCount) {
        HIP_TRY(hipMemcpy(slotVtx.data(), R.slotVtx + 3 * (size_t)M.slotBase, slotVtx.size() * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(triPrim.data(), c->sc.triPrim + M.slotBase, triPrim.size() * 4, hipMemcpyDeviceToHost));
    }
    const std::string which = "mesh " + std::to_string(mesh) + ": ";
    std::vector<uint32_t> idx((size_t)M.primCount * 3, 0xffffffffu);
    for (uint32_t sl = 0; sl < M.slotCount; sl++) {
        if (slotVtx[3 * (size_t)sl] == 0xffffffffu) continue; // a pad slot
        const uint32_t prim = triPrim[sl];
        if (prim >= M.primCount) return fail(PRT_HIP_EINVAL, which + "a leaf names a triangle the mesh does not have: vertex normals cannot be recomputed");
        if (idx[3 * (size_t)prim] != 0xffffffffu) return fail(PRT_HIP_EINVAL, which + "two leaves name the same triangle: vertex normals cannot be recomputed");
        for (int j = 0; j < 3; j++) {
            const uint32_t v = slotVtx[3 * (size_t)sl + j];
            if (v >= M.vertexCount) return fail(PRT_HIP_EINVAL, which + "internal: vertex index out of range");
            idx[3 * (size_t)prim + j] = v;
        }
    }
    for (uint32_t p = 0; p < M.primCount; p++)
        if (idx[3 * (size_t)p] == 0xffffffffu) return fail(PRT_HIP_EINVAL, which + "no leaf names triangle " + std::to_string(p) + ": vertex normals cannot be recomputed");
    std::vector<uint32_t> off((size_t)M.vertexCount + 1, 0), face(idx.size());
    for (uint32_t v : idx) off[(size_t)v + 1]++;
    for (size_t v = 0; v < M.vertexCount; v++) off[v + 1] += off[v];
    std::vector<uint32_t> cursor(off.begin(), off.end() - 1);
    for (uint32_t f = M.primCount; f-- > 0;) // mesh.cpp:112: faces descending, corners ascending
        for (int j = 0; j < 3; j++) face[cursor[idx[3 * (size_t)f + j]]++] = f;
    DevBuf<uint32_t> dOff, dFace, dIdx; // the mesh's only once all of it is on the device: a failure frees them here
    DevBuf<float> dFn;
    int rc;
    if ((rc = prt_upload(dOff, off, c->stream)) || (rc = prt_upload(dFace, face, c->stream)) || (rc = prt_upload(dIdx, idx, c->stream))) return rc;
    HIP_TRY(dFn.fit(idx.size(), c->stream));
    M.csrFace = std::move(dFace);
    M.faceVtx = std::move(dIdx);
    M.faceNrm = std::move(dFn);
    M.csrOff = std::move(dOff);
    return PRT_HIP_OK;
}

const uint32_t kFlags = PRT_HIP_DEFORM_HOST | PRT_HIP_DEFORM_RADIUS_AUTO;

// every refusal of prt_hip_deform_meshes; nothing has changed when it returns non-zero.  as[k]: the update as prt_hip_update_meshes would take it
int check_deform(prt_hip_ctx* c, uint32_t count, const prt_mesh_deform* d, uint32_t flags, prt_mesh_update* as)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (count == 0 || !d) return fail(PRT_HIP_EINVAL, "no mesh update given");
    if (count > PRT_MAX_BVH) return fail(PRT_HIP_EINVAL, "more updates than a scene has meshes");
    if (flags & ~kFlags) return fail(PRT_HIP_EINVAL, "unknown flag bits");
    for (uint32_t k = 0; k < count; k++) {
        const std::string which = "update " + std::to_string(k) + ": ";
        if (d[k].normalsMode > PRT_HIP_NORMALS_RECOMPUTE) return fail(PRT_HIP_EINVAL, which + "unknown normalsMode " + std::to_string(d[k].normalsMode));
        if (d[k].normalsMode == PRT_HIP_NORMALS_GIVEN && !d[k].normals) return fail(PRT_HIP_EINVAL, which + "PRT_HIP_NORMALS_GIVEN with NULL normals");
        if (d[k].normalsMode != PRT_HIP_NORMALS_GIVEN && d[k].normals)
            return fail(PRT_HIP_EINVAL, which + "normals must be NULL unless normalsMode is PRT_HIP_NORMALS_GIVEN");
        if ((flags & PRT_HIP_DEFORM_RADIUS_AUTO) && d[k].radius != 0.0f)
            return fail(PRT_HIP_EINVAL, which + "radius must be 0 with PRT_HIP_DEFORM_RADIUS_AUTO (the library computes it)");
        as[k] = prt_mesh_update{d[k].mesh, d[k].vertexCount, d[k].positions, d[k].normals, d[k].radius};
    }
    int rc = prt_refit_check(c, count, as);
    if (rc) return rc;
    for (uint32_t k = 0; k < count; k++)
        if (d[k].normalsMode == PRT_HIP_NORMALS_RECOMPUTE && !c->rf.meshes[d[k].mesh].hasNormals)
            return fail(PRT_HIP_EINVAL, "update " + std::to_string(k) + ": normals cannot be recomputed for a mesh that was uploaded without vertex normals");
    return PRT_HIP_OK;
}

// allocations and tables a checked call needs; the tree as uploaded is measured before it goes
int prepare_deform(prt_hip_ctx* c, uint32_t count, const prt_mesh_deform* d, prt_mesh_update* as)
{
    int rc = scratch_ready(c);
    if (rc) return rc;
    for (uint32_t k = 0; k < count; k++)
        if (d[k].normalsMode == PRT_HIP_NORMALS_RECOMPUTE && (rc = csr_ready(c, d[k].mesh))) return rc;
    for (uint32_t k = 0; k < count; k++)
        if (d[k].normalsMode == PRT_HIP_NORMALS_RECOMPUTE) as[k].normals = d[k].positions; // (non-NULL: the mesh needs its normals buffer)
    if ((rc = prt_refit_staging(c, count, as))) return rc;
    for (uint32_t k = 0; k < count; k++)
        if ((rc = prt_deform_capture_sah(c, d[k].mesh))) return rc;
    return PRT_HIP_OK;
}

// The device work of a checked and prepared call on s.  tm (optional, 6 marks): before the keep kernels, after them, after the face
// kernels, and -- the three of prt_refit_queue -- after the vertex kernels, after the gathers, after the finish kernel.
int queue_deform(prt_hip_ctx* c, uint32_t count, const prt_mesh_deform* d, uint32_t flags, hipStream_t s, StageTimer* tm)
{
    PrtRefit& R = c->rf;
    const bool host = (flags & PRT_HIP_DEFORM_HOST) != 0;
    PrtRefitSrc src[PRT_MAX_BVH];
    for (uint32_t k = 0; k < count; k++) {
        PrtRefitMesh& M = R.meshes[d[k].mesh];
        const size_t bytes = (size_t)M.vertexCount * 3 * sizeof(float);
        const bool given = d[k].normalsMode == PRT_HIP_NORMALS_GIVEN;
        src[k] = PrtRefitSrc{d[k].mesh, d[k].positions, given ? d[k].normals : nullptr};
        if (host) { // staged and copied as prt_hip_update_meshes does
            HIP_TRY(hipMemcpyAsync(M.dPos, d[k].positions, bytes, hipMemcpyHostToDevice, s));
            if (given) HIP_TRY(hipMemcpyAsync(M.dNrm, d[k].normals, bytes, hipMemcpyHostToDevice, s));
            src[k].pos = M.dPos;
            if (given) src[k].nrm = M.dNrm;
        }
        if (d[k].normalsMode == PRT_HIP_NORMALS_RECOMPUTE) src[k].nrm = M.dNrm;
    }
    if (tm) HIP_TRY(tm->mark(s));
    int rc;
    for (uint32_t k = 0; k < count; k++) {
        PrtRefitMesh& M = R.meshes[d[k].mesh];
        const bool given = d[k].normalsMode == PRT_HIP_NORMALS_GIVEN;
        if ((rc = queue_box(c, d[k].mesh, src[k].pos, host ? nullptr : (float*)M.dPos, given ? src[k].nrm : nullptr, given && !host ? (float*)M.dNrm : nullptr, s))) return rc;
    }
    if (flags & PRT_HIP_DEFORM_RADIUS_AUTO) // meshes the host path changed since their box was taken
        for (uint32_t m = 0; m < R.meshes.size(); m++) {
            bool named = false;
            for (uint32_t k = 0; k < count; k++) named |= d[k].mesh == m;
            if (!named && !R.meshes[m].vboxValid && (rc = queue_box(c, m, R.meshes[m].dPos, nullptr, nullptr, nullptr, s))) return rc;
        }
    if (tm) HIP_TRY(tm->mark(s));
    for (uint32_t k = 0; k < count; k++) {
        const PrtRefitMesh& M = R.meshes[d[k].mesh];
        if (d[k].normalsMode != PRT_HIP_NORMALS_RECOMPUTE || M.primCount == 0) continue;
        hipLaunchKernelGGL(deform_face_kernel, dim3(blocks_of(M.primCount)), dim3(PRT_DEFORM_BLOCK), 0, s, M.faceVtx, src[k].pos, M.faceNrm, M.primCount);
        if ((rc = prt_launched("deform_face_kernel"))) return rc;
    }
    if (tm) HIP_TRY(tm->mark(s));
    for (uint32_t k = 0; k < count; k++) {
        const PrtRefitMesh& M = R.meshes[d[k].mesh];
        if (d[k].normalsMode != PRT_HIP_NORMALS_RECOMPUTE || M.vertexCount == 0) continue;
        hipLaunchKernelGGL(deform_vertex_kernel, dim3(blocks_of(M.vertexCount)), dim3(PRT_DEFORM_BLOCK), 0, s, M.csrOff, M.csrFace, M.faceNrm, M.dNrm, M.vertexCount);
        if ((rc = prt_launched("deform_vertex_kernel"))) return rc;
    }
    return prt_refit_queue(c, count, src, s, tm);
}

// after the synchronisation: the vertex boxes, the radius (AUTO) and what prt_hip_update_meshes commits
void commit_deform(prt_hip_ctx* c, uint32_t count, const prt_mesh_deform* d, uint32_t flags)
{
    PrtRefit& R = c->rf;
    uint32_t ids[PRT_MAX_BVH];
    float radius = 0.0f;
    for (uint32_t k = 0; k < count; k++) {
        ids[k] = d[k].mesh;
        if (d[k].radius != 0.0f) radius = d[k].radius;
        memcpy(R.meshes[d[k].mesh].vbox, R.vboxHost + 6 * d[k].mesh, 6 * sizeof(float));
        R.meshes[d[k].mesh].vboxValid = true;
    }
    if (flags & PRT_HIP_DEFORM_RADIUS_AUTO) {
        float lo[3], hi[3]; // scene.cpp:23-26
        for (int j = 0; j < 3; j++) {
            lo[j] = std::numeric_limits<float>::max();
            hi[j] = std::numeric_limits<float>::lowest();
        }
        for (uint32_t m = 0; m < R.meshes.size(); m++) {
            PrtRefitMesh& M = R.meshes[m];
            if (!M.vboxValid) {
                memcpy(M.vbox, R.vboxHost + 6 * m, 6 * sizeof(float));
                M.vboxValid = true;
            }
            for (int j = 0; j < 3; j++) {
                lo[j] = std::fmin(lo[j], M.vbox[j]);
                hi[j] = std::fmax(hi[j], M.vbox[3 + j]);
            }
        }
        float e[3];
        for (int j = 0; j < 3; j++) {
            const float centre = 0.5f * (hi[j] + lo[j]);
            e[j] = hi[j] - centre;
        }
        const float x = e[0] * e[0], y = e[1] * e[1], z = e[2] * e[2];
        radius = sqrtf(x + y + z);
    }
    prt_refit_commit(c, count, ids, radius);
}

} // namespace

int prt_deform_capture_sah(prt_hip_ctx* c, uint32_t mesh)
{
    PrtRefitMesh& M = c->rf.meshes[mesh];
    if (M.sahCaptured) return PRT_HIP_OK;
    int rc = sah_of(c, mesh, M.sahUpload, nullptr, nullptr);
    if (rc) return rc;
    M.sahCaptured = true;
    return PRT_HIP_OK;
}

extern "C" {

int prt_hip_deform_meshes(prt_hip_ctx* c, uint32_t count, const prt_mesh_deform* deforms, uint32_t flags, void* stream)
{
    prt_mesh_update as[PRT_MAX_BVH];
    int rc = check_deform(c, count, deforms, flags, as);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = prepare_deform(c, count, deforms, as))) return rc;
    hipStream_t s = c->stream, caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = queue_deform(c, count, deforms, flags, s, nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(c->rf.rootHost, c->rf.rootOut, PRT_MAX_BVH * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c->rf.vboxHost, c->rf.vboxOut, PRT_MAX_BVH * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
    if ((rc = prt_stream_leave(c, caller))) return rc;
    HIP_TRY(hipStreamSynchronize(s)); // the root boxes and the radius are part of DevScene, which every later launch takes by value
    commit_deform(c, count, deforms, flags);
    return PRT_HIP_OK;
}

int prt_hip_get_mesh_vertices(prt_hip_ctx* c, uint32_t mesh, float* positions, float* normals, uint32_t flags, void* stream)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (flags & ~PRT_HIP_DEFORM_HOST) return fail(PRT_HIP_EINVAL, "unknown flag bits");
    if (mesh >= c->rf.meshes.size()) return fail(PRT_HIP_EINVAL, "mesh index out of range");
    const PrtRefitMesh& M = c->rf.meshes[mesh];
    if (positions && !M.dPos) return fail(PRT_HIP_ESTATE, "no update yet: the caller still holds what it uploaded");
    if (normals && !M.dNrm) return fail(PRT_HIP_ESTATE, "no update of the normals yet: the caller still holds what it uploaded");
    HIP_TRY(hipSetDevice(c->device));
    const bool host = (flags & PRT_HIP_DEFORM_HOST) != 0;
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t bytes = (size_t)M.vertexCount * 3 * sizeof(float);
    hipStream_t s = c->stream, caller;
    int rc = prt_stream_enter(c, stream, &caller);
    if (rc) return rc;
    if (positions && bytes) HIP_TRY(hipMemcpyAsync(positions, M.dPos, bytes, kind, s));
    if (normals && bytes) HIP_TRY(hipMemcpyAsync(normals, M.dNrm, bytes, kind, s));
    if ((rc = prt_stream_leave(c, caller))) return rc;
    if (host) HIP_TRY(hipStreamSynchronize(s));
    return PRT_HIP_OK;
}

int prt_hip_mesh_info(prt_hip_ctx* c, uint32_t mesh, prt_mesh_info* out)
{
    if (!c || !out) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (mesh >= c->rf.meshes.size()) return fail(PRT_HIP_EINVAL, "mesh index out of range");
    HIP_TRY(hipSetDevice(c->device));
    PrtRefitMesh& M = c->rf.meshes[mesh];
    int rc;
    if (!M.vboxValid) { // last changed by prt_hip_update_meshes: the staged copy is reduced now (a cache: nothing a render sees changes)
        if ((rc = scratch_ready(c)) || (rc = queue_box(c, mesh, M.dPos, nullptr, nullptr, nullptr, c->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(c->rf.vboxHost + 6 * mesh, c->rf.vboxOut + 6 * mesh, 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        memcpy(M.vbox, c->rf.vboxHost + 6 * mesh, 6 * sizeof(float));
        M.vboxValid = true;
    }
    double area[3];
    prt_mesh_info info{};
    if ((rc = sah_of(c, mesh, area, &info.internalNodes, &info.leaves))) return rc;
    if (!M.sahCaptured) { // never updated: the tree is the uploaded one
        memcpy(M.sahUpload, area, sizeof(area));
        M.sahCaptured = true;
    }
    memcpy(info.vertexBox, M.vbox, sizeof(info.vertexBox));
    memcpy(info.rootBox, c->sc.rootBox[mesh], sizeof(info.rootBox));
    info.radius = c->sc.radius;
    info.internalArea = area[0];
    info.leafArea = area[1];
    info.rootArea = area[2];
    info.sahCost = (0.125 * area[0] + area[1]) / area[2];
    info.sahCostAtUpload = (0.125 * M.sahUpload[0] + M.sahUpload[1]) / M.sahUpload[2];
    *out = info;
    return PRT_HIP_OK;
}

#ifdef PRT_TEST_ENTRY_POINTS
// tools/refit_bench.py --device: the device work of prt_hip_deform_meshes queued `reps` times on the context's stream between HIP
// events; ms[0..4] = medians of keep + box, face normals, vertex normals, gather, levels + finish.  Ends with one real
// prt_hip_deform_meshes.  Synchronous.
int prt_hip_test_deform_profile(prt_hip_ctx* c, uint32_t count, const prt_mesh_deform* deforms, uint32_t flags, uint32_t reps, float* ms5)
{
    prt_mesh_update as[PRT_MAX_BVH];
    int rc = check_deform(c, count, deforms, flags, as);
    if (rc) return rc;
    if (!ms5 || reps == 0) return fail(PRT_HIP_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = prepare_deform(c, count, deforms, as))) return rc;
    StageTimer tm(5);
    for (uint32_t r = 0; r < reps; r++) {
        if ((rc = queue_deform(c, count, deforms, flags, c->stream, &tm))) return rc;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(PRT_HIP_ELAUNCH, "deform profile: synchronise failed");
        HIP_TRY(tm.lap());
    }
    for (uint32_t j = 0; j < 5; j++) HIP_TRY(tm.median(j, &ms5[j]));
    return prt_hip_deform_meshes(c, count, deforms, flags, nullptr);
}
#endif

} // extern "C"
