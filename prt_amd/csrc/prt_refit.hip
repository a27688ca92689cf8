// prt_refit.hip -- geometry updates (include/prt_hip.h "geometry updates"): new vertex positions for meshes of the uploaded scene,
// with everything prt_hip_upload_scene derives from positions rewritten on the device: leaf triangle corners, face / vertex
// normals, bump tangents, the child boxes of every wide record (a bottom-up refit of the unchanged tree), the hot-node copies,
// the root boxes.  Two kernels do the work:
//   gather  one lane per triangle slot: vertex ids -> corners (staged in LDS so that the 36-byte triangles leave as whole-wave
//           contiguous dword stores), normals into the shade records, dp01 / dp02 into the bump records, with the operations of
//           the host code of the upload (hsub / hcross / hnormalize = sub3 / cross3 / normalize3) in the same order;
//   level   one lane per wide record of one depth of one mesh: a leaf child's box is the min / max over its freshly written
//           corners, an internal child's box the union of the two boxes in that child's own record.  Launched per depth,
//           deepest first: the kernel boundary hands a level's boxes to the level above, so nothing inside a launch depends
//           on another workgroup.  min / max of finite floats is exact and order independent (up to the sign of a zero).
// The root boxes travel back to the host (DevScene is a by-value kernel argument), which costs the call one synchronisation.
// prt_hip_deform_meshes (prt_deform.hip) shares the checks, the staging buffers, the three kernels (prt_refit_queue reads device
// arrays wherever they lie) and the commit with prt_hip_update_meshes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prt_hip.h"
#include "prt_device.h"
#include "prt_internal.h"
#ifdef PRT_TEST_ENTRY_POINTS
#include "../../include/prt_hip_test.h"
#endif

#define PRT_REFIT_BLOCK 256

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

struct GatherArgs {
    const uint32_t* slotVtx; // 3 per slot, all slots of the scene
    const float* pos;        // the mesh's new positions
    const float* nrm;        // the mesh's new vertex normals, or NULL (keep / none)
    float* tris;
    float4* shade;
    float4* bump; // NULL when the scene has no bump map
    uint32_t slotBase, slotCount;
    uint32_t faceNormals; // the mesh has no vertex normals: n0 is the face normal
};

__device__ __forceinline__ void st3(float4* rec, Vec3 v) // the first three floats of a record; the fourth is not positional
{
    float* q = (float*)rec;
    *(PRT_AS1 float*)q = v.x;
    *(PRT_AS1 float*)(q + 1) = v.y;
    *(PRT_AS1 float*)(q + 2) = v.z;
}

__global__ __launch_bounds__(PRT_REFIT_BLOCK) void refit_gather_kernel(GatherArgs a)
{
    __shared__ float corners[PRT_REFIT_BLOCK * 9]; // stride 9 words per lane: odd, no bank conflict
    const uint32_t first = blockIdx.x * PRT_REFIT_BLOCK, i = first + threadIdx.x;
    Vec3 p0 = mk3(0.0f, 0.0f, 0.0f), p1 = p0, p2 = p0;
    if (i < a.slotCount) {
        const size_t g = (size_t)a.slotBase + i;
        const uint32_t v0 = gld(a.slotVtx + 3 * g), v1 = gld(a.slotVtx + 3 * g + 1), v2 = gld(a.slotVtx + 3 * g + 2);
        if (v0 != 0xffffffffu) { // (a pad slot keeps its zeros everywhere)
            p0 = ld3(a.pos, v0);
            p1 = ld3(a.pos, v1);
            p2 = ld3(a.pos, v2);
            float4* sh = a.shade + 4 * g;
            if (a.faceNormals) {
                st3(sh, normalize3(cross3(sub3(p1, p0), sub3(p2, p0)))); // mesh.cpp:335
            } else if (a.nrm) {
                st3(sh, ld3(a.nrm, v0));
                st3(sh + 1, ld3(a.nrm, v1));
                st3(sh + 2, ld3(a.nrm, v2));
            }
            if (a.bump) {
                float4* bp = a.bump + 3 * g;
                st3(bp, normalize3(sub3(p1, p0))); // mesh.cpp:360-361
                st3(bp + 1, normalize3(sub3(p2, p0)));
            }
        }
    }
    float* mine = corners + 9 * threadIdx.x;
    mine[0] = p0.x; mine[1] = p0.y; mine[2] = p0.z;
    mine[3] = p1.x; mine[4] = p1.y; mine[5] = p1.z;
    mine[6] = p2.x; mine[7] = p2.y; mine[8] = p2.z;
    __syncthreads();
    // the block's 256 triangles are 2304 contiguous floats: every store instruction of a wave covers 256 contiguous bytes
    const uint32_t left = a.slotCount > first ? a.slotCount - first : 0u;
    const uint32_t floats = 9u * (left < PRT_REFIT_BLOCK ? left : PRT_REFIT_BLOCK);
    float* out = a.tris + 9 * ((size_t)a.slotBase + first);
#pragma unroll
    for (uint32_t k = 0; k < 9u; k++) {
        const uint32_t f = k * PRT_REFIT_BLOCK + threadIdx.x;
        if (f < floats) *(PRT_AS1 float*)(out + f) = corners[f];
    }
}

// The box of a kid word: a leaf reference -> min / max over its triangles' corners; a record index -> the union of the record's
// two child boxes (that record belongs to a deeper level: written by an earlier launch).
__device__ __forceinline__ Box kid_box(uint32_t kid, const float* tris, const float4* wnodes)
{
    Box b;
    if (kid & PRT_REF_LEAF) {
        const uint32_t n = leaf_count(kid);
        const float* tp = tris + 9 * (size_t)leaf_first(kid);
        b.lo = b.hi = mk3(gld(tp), gld(tp + 1), gld(tp + 2));
        for (uint32_t k = 1; k < 3u * n; k++) {
            const Vec3 p = mk3(gld(tp + 3 * k), gld(tp + 3 * k + 1), gld(tp + 3 * k + 2));
            b.lo = mk3(fminf(b.lo.x, p.x), fminf(b.lo.y, p.y), fminf(b.lo.z, p.z));
            b.hi = mk3(fmaxf(b.hi.x, p.x), fmaxf(b.hi.y, p.y), fmaxf(b.hi.z, p.z));
        }
    } else {
        const float4* rec = wnodes + 4 * (size_t)kid;
        const float4 w0 = gld4(rec), w1 = gld4(rec + 1), w2 = gld4(rec + 2);
        b.lo = mk3(fminf(w0.x, w2.x), fminf(w0.z, w2.z), fminf(w1.x, w1.z));
        b.hi = mk3(fmaxf(w0.y, w2.y), fmaxf(w0.w, w2.w), fmaxf(w1.y, w1.w));
    }
    return b;
}

__global__ __launch_bounds__(PRT_REFIT_BLOCK) void refit_level_kernel(const uint32_t* list, uint32_t n, const uint2* kids, const float* tris, float4* wnodes)
{
    const uint32_t i = blockIdx.x * PRT_REFIT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = gld(list + i);
    const uint2 kid = gld2u(kids + r);
    const Box b0 = kid_box(kid.x, tris, wnodes), b1 = kid_box(kid.y, tris, wnodes);
    float4* rec = wnodes + 4 * (size_t)r; // the layout of prt_device.h; the fourth float4 (references, split axis) stays
    gst4(rec, make_float4(b0.lo.x, b0.hi.x, b0.lo.y, b0.hi.y));
    gst4(rec + 1, make_float4(b0.lo.z, b0.hi.z, b1.lo.z, b1.hi.z));
    gst4(rec + 2, make_float4(b1.lo.x, b1.hi.x, b1.lo.y, b1.hi.y));
}

struct RootArgs {
    uint32_t count;
    uint32_t mesh[PRT_MAX_BVH], kid[PRT_MAX_BVH];
};

// After the levels: the root boxes of the updated meshes (lane t < count) and the hot-node copies of the box part of their records
// (every hot slot: a record of a mesh that was not updated is copied onto equal bytes).
__global__ __launch_bounds__(PRT_REFIT_BLOCK) void refit_finish_kernel(RootArgs a, const float* tris, const float4* wnodes, float* rootOut,
                                                                       const uint32_t* hotOrder, uint32_t hotCount, float4* hot)
{
    const uint32_t t = blockIdx.x * PRT_REFIT_BLOCK + threadIdx.x;
    if (t < a.count) {
        const Box b = kid_box(a.kid[t], tris, wnodes);
        float* q = rootOut + 6 * a.mesh[t];
        q[0] = b.lo.x; q[1] = b.lo.y; q[2] = b.lo.z;
        q[3] = b.hi.x; q[4] = b.hi.y; q[5] = b.hi.z;
    }
    if (t < 3u * hotCount) {
        const uint32_t k = t / 3u, j = t - 3u * k;
        gst4(hot + 4 * (size_t)k + j, gld4(wnodes + 4 * (size_t)gld(hotOrder + k) + j));
    }
}

// Queues the copies of the caller's host arrays into the staging buffers, then the refit reading them (prt_refit_queue).
int queue_update(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* u, hipStream_t s, StageTimer* tm)
{
    PrtRefit& R = c->rf;
    PrtRefitSrc src[PRT_MAX_BVH];
    for (uint32_t k = 0; k < count; k++) { // the caller's arrays first (the library copies)
        PrtRefitMesh& M = R.meshes[u[k].mesh];
        const size_t bytes = (size_t)M.vertexCount * 3 * sizeof(float);
        HIP_TRY(hipMemcpyAsync(M.dPos, u[k].positions, bytes, hipMemcpyHostToDevice, s));
        if (u[k].normals) HIP_TRY(hipMemcpyAsync(M.dNrm, u[k].normals, bytes, hipMemcpyHostToDevice, s));
        M.vboxValid = false; // (the vertex box of the staged copy is reduced when a later call asks for it: prt_deform.hip)
        src[k] = PrtRefitSrc{u[k].mesh, M.dPos, u[k].normals ? (float*)M.dNrm : nullptr};
    }
    return prt_refit_queue(c, count, src, s, tm);
}

} // namespace

int prt_refit_queue(prt_hip_ctx* c, uint32_t count, const PrtRefitSrc* u, hipStream_t s, StageTimer* tm)
{
    PrtRefit& R = c->rf;
    PrtSceneArrays& A = c->arr; // the writable pointers are the owners'
    float* tris = A.tris;
    float4* wnodes = A.wnodes;
    if (tm) HIP_TRY(tm->mark(s));
    for (uint32_t k = 0; k < count; k++) {
        PrtRefitMesh& M = R.meshes[u[k].mesh];
        if (M.slotCount == 0) continue;
        GatherArgs g{R.slotVtx, u[k].pos, u[k].nrm, tris, A.shade, A.anyBump() ? (float4*)A.bump : nullptr, M.slotBase, M.slotCount, M.hasNormals ? 0u : 1u};
        hipLaunchKernelGGL(refit_gather_kernel, dim3((M.slotCount + PRT_REFIT_BLOCK - 1) / PRT_REFIT_BLOCK), dim3(PRT_REFIT_BLOCK), 0, s, g);
        int rc = prt_launched("refit_gather_kernel");
        if (rc) return rc;
    }
    if (tm) HIP_TRY(tm->mark(s));
    RootArgs ra{};
    for (uint32_t k = 0; k < count; k++) {
        const PrtRefitMesh& M = R.meshes[u[k].mesh];
        for (size_t d = M.levels.size(); d-- > 0;) { // deepest first
            const uint32_t first = M.levels[d].first, n = M.levels[d].second;
            hipLaunchKernelGGL(refit_level_kernel, dim3((n + PRT_REFIT_BLOCK - 1) / PRT_REFIT_BLOCK), dim3(PRT_REFIT_BLOCK), 0, s, R.levelList + first, n,
                               R.kids, tris, wnodes);
            int rc = prt_launched("refit_level_kernel");
            if (rc) return rc;
        }
        ra.mesh[ra.count] = u[k].mesh;
        ra.kid[ra.count] = M.rootKid;
        ra.count++;
    }
    const uint32_t lanes = std::max<uint32_t>(ra.count, 3u * R.hotCount);
    hipLaunchKernelGGL(refit_finish_kernel, dim3((lanes + PRT_REFIT_BLOCK - 1) / PRT_REFIT_BLOCK), dim3(PRT_REFIT_BLOCK), 0, s, ra, tris, wnodes, R.rootOut,
                       R.hotOrder, R.hotCount, A.hotNodes);
    int rc = prt_launched("refit_finish_kernel");
    if (rc) return rc;
    if (tm) HIP_TRY(tm->mark(s));
    return PRT_HIP_OK;
}

// every refusal of prt_hip_update_meshes; nothing has changed when it returns non-zero
int prt_refit_check(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* u)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (count == 0 || !u) return fail(PRT_HIP_EINVAL, "no mesh update given");
    if (count > PRT_MAX_BVH) return fail(PRT_HIP_EINVAL, "more updates than a scene has meshes");
    for (uint32_t k = 0; k < count; k++) {
        const std::string which = "update " + std::to_string(k) + ": ";
        if (u[k].mesh >= c->rf.meshes.size()) return fail(PRT_HIP_EINVAL, which + "mesh index out of range");
        const PrtRefitMesh& M = c->rf.meshes[u[k].mesh];
        if (u[k].vertexCount != M.vertexCount)
            return fail(PRT_HIP_EINVAL, which + "vertexCount " + std::to_string(u[k].vertexCount) + " differs from the uploaded mesh's " + std::to_string(M.vertexCount));
        if (!u[k].positions) return fail(PRT_HIP_EINVAL, which + "positions is NULL");
        if (u[k].normals && !M.hasNormals) return fail(PRT_HIP_EINVAL, which + "normals given for a mesh that was uploaded without vertex normals");
        if (!(u[k].radius >= 0.0f) || std::isinf(u[k].radius)) return fail(PRT_HIP_EINVAL, which + "radius must be finite and >= 0 (0 keeps the current one)");
        for (uint32_t j = 0; j < k; j++)
            if (u[j].mesh == u[k].mesh) return fail(PRT_HIP_EINVAL, which + "mesh " + std::to_string(u[k].mesh) + " is named twice in one call");
    }
    return PRT_HIP_OK;
}

// staging buffers of the named meshes (kept with the scene)
int prt_refit_staging(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* u)
{
    for (uint32_t k = 0; k < count; k++) {
        PrtRefitMesh& M = c->rf.meshes[u[k].mesh];
        const size_t floats = (size_t)M.vertexCount * 3;
        if (!M.dPos) HIP_TRY(M.dPos.fit(floats, c->stream));
        if (u[k].normals && !M.dNrm) HIP_TRY(M.dNrm.fit(floats, c->stream));
    }
    return PRT_HIP_OK;
}

void prt_refit_commit(prt_hip_ctx* c, uint32_t count, const uint32_t* meshes, float radius)
{
    for (uint32_t k = 0; k < count; k++) memcpy(c->sc.rootBox[meshes[k]], c->rf.rootHost + 6 * meshes[k], 6 * sizeof(float));
    if (radius != 0.0f) c->sc.radius = radius;
    // what was sampled or derived from the old geometry
    prt_accum_forget(c);
    prt_denoise_forget(c);
    if (c->haveCamera) {
        prt_camera_desc same;
        static_assert(sizeof(same) == sizeof(c->cam), "camera layouts must match");
        memcpy(&same, &c->cam, sizeof(same));
        prt_temporal_camera_change(c, &same); // the same promotion as a camera move of unchanged size
    } else {
        prt_temporal_forget(c);
    }
}

int prt_refit_build(prt_hip_ctx* c, const std::vector<float4>& wnodes, const std::vector<uint32_t>& hotOrder, std::vector<PrtRefitMesh>&& meshes,
                    const std::vector<uint32_t>& slotVtx)
{
    PrtRefit& R = c->rf;
    R = PrtRefit{};
    R.meshes = std::move(meshes);
    const size_t records = wnodes.size() / 4;
    R.hotCount = (uint32_t)hotOrder.size();
    auto bitsOf = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    auto resolve = [&](uint32_t ref) -> uint32_t {
        if (ref & PRT_REF_LEAF) return ref;
        return (ref & PRT_REF_HOT) ? hotOrder[ref & (PRT_HOT_NODES - 1u)] : ref;
    };
    std::vector<uint2> kids(records);
    for (size_t r = 0; r < records; r++) {
        const float4& refs = wnodes[r * 4 + 3];
        kids[r] = make_uint2(resolve(bitsOf(refs.x)), resolve(bitsOf(refs.y)));
    }
    std::vector<uint32_t> levelList;
    levelList.reserve(records);
    for (PrtRefitMesh& M : R.meshes) {
        M.rootKid = resolve(M.rootKid);
        std::vector<uint32_t> level, next;
        if (!(M.rootKid & PRT_REF_LEAF)) level.push_back(M.rootKid);
        while (!level.empty()) {
            M.levels.push_back({(uint32_t)levelList.size(), (uint32_t)level.size()});
            levelList.insert(levelList.end(), level.begin(), level.end());
            next.clear();
            for (uint32_t r : level)
                for (uint32_t k : {kids[r].x, kids[r].y})
                    if (!(k & PRT_REF_LEAF)) next.push_back(k);
            level.swap(next);
        }
    }
    if (levelList.size() != records) return fail(PRT_HIP_EINVAL, "internal: the wide records are not the trees of the scene's roots");
    int rc;
    if ((rc = prt_upload(R.slotVtx, slotVtx, c->stream))) return rc;
    if ((rc = prt_upload(R.kids, kids, c->stream))) return rc;
    if ((rc = prt_upload(R.levelList, levelList, c->stream))) return rc;
    if ((rc = prt_upload(R.hotOrder, hotOrder, c->stream))) return rc;
    HIP_TRY(R.rootOut.fit(PRT_MAX_BVH * 6, c->stream));
    HIP_TRY(R.rootHost.fit(PRT_MAX_BVH * 6));
    return PRT_HIP_OK;
}

void prt_refit_forget(prt_hip_ctx* c) { c->rf = PrtRefit{}; } // (the device arrays and the pinned copies go with their owners)

extern "C" {

int prt_hip_update_meshes(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* updates, void* stream)
{
    int rc = prt_refit_check(c, count, updates);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = prt_refit_staging(c, count, updates))) return rc;
    for (uint32_t k = 0; k < count; k++) // prt_hip_mesh_info compares against the tree as uploaded
        if ((rc = prt_deform_capture_sah(c, updates[k].mesh))) return rc;
    hipStream_t s = c->stream, caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = queue_update(c, count, updates, s, nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(c->rf.rootHost, c->rf.rootOut, PRT_MAX_BVH * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
    if ((rc = prt_stream_leave(c, caller))) return rc;
    HIP_TRY(hipStreamSynchronize(s)); // the root boxes are part of DevScene, which every later launch takes by value
    uint32_t ids[PRT_MAX_BVH];
    float radius = 0.0f; // with several updates the last non-zero one holds
    for (uint32_t k = 0; k < count; k++) {
        ids[k] = updates[k].mesh;
        if (updates[k].radius != 0.0f) radius = updates[k].radius;
    }
    prt_refit_commit(c, count, ids, radius);
    return PRT_HIP_OK;
}

#ifdef PRT_TEST_ENTRY_POINTS
int prt_hip_test_scene_arrays(prt_hip_ctx* c, uint64_t counts[5], float* wnodes, float* hot, float* tris, float* shade, float* bump,
                              float* rootBoxes, float* radius)
{
    if (!c || !counts) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    const PrtSceneArrays& A = c->arr;
    const uint64_t records = A.wnodes.size() / 4, slots = c->rf.slotVtx.size() / 3;
    counts[0] = records;
    counts[1] = PRT_HOT_NODES;
    counts[2] = slots;
    counts[3] = A.anyBump() ? slots : 0;
    counts[4] = c->sc.bvhCount;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (wnodes && records) HIP_TRY(hipMemcpy(wnodes, A.wnodes, records * 64, hipMemcpyDeviceToHost));
    if (hot) HIP_TRY(hipMemcpy(hot, A.hotNodes, (size_t)PRT_HOT_NODES * 64, hipMemcpyDeviceToHost));
    if (tris && slots) HIP_TRY(hipMemcpy(tris, A.tris, slots * 36, hipMemcpyDeviceToHost));
    if (shade && slots) HIP_TRY(hipMemcpy(shade, A.shade, slots * 64, hipMemcpyDeviceToHost));
    if (bump && counts[3]) HIP_TRY(hipMemcpy(bump, A.bump, slots * 48, hipMemcpyDeviceToHost));
    if (rootBoxes) memcpy(rootBoxes, c->sc.rootBox, sizeof(c->sc.rootBox));
    if (radius) *radius = c->sc.radius;
    return PRT_HIP_OK;
}

// tools/refit_bench.py: the update queued `reps` times on the context's stream between HIP events; ms[0] = median time of the gather
// kernels, ms[1] = median of the level launches + finish (the copies of the caller's arrays lie before both).  Synchronous;
// the context's state is that of one prt_hip_update_meshes.
int prt_hip_test_refit_profile(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* updates, uint32_t reps, float* ms2)
{
    int rc = prt_refit_check(c, count, updates);
    if (rc) return rc;
    if (!ms2 || reps == 0) return fail(PRT_HIP_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = prt_refit_staging(c, count, updates))) return rc;
    for (uint32_t k = 0; k < count; k++)
        if ((rc = prt_deform_capture_sah(c, updates[k].mesh))) return rc;
    StageTimer tm(2);
    for (uint32_t r = 0; r < reps; r++) {
        if ((rc = queue_update(c, count, updates, c->stream, &tm))) return rc;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(PRT_HIP_ELAUNCH, "refit profile: synchronise failed");
        HIP_TRY(tm.lap());
    }
    for (uint32_t k = 0; k < 2; k++) HIP_TRY(tm.median(k, &ms2[k]));
    return prt_hip_update_meshes(c, count, updates, nullptr);
}
#endif

} // extern "C"
