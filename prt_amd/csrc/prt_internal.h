// prt_internal.h -- what the translation units of libprt_hip.so share: the context behind the C-ABI handle, the error
// helpers and the build constants of the wavefront pipeline.  Not installed; include/prt_hip.h is the interface.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/prt_hip.h"
#include "prt_devbuf.h"
#include "prt_devres.h"
#include "prt_stage.h"
#include "prt_device.h"
#include "prt_batch.h"

#define PRT_WORK_WORDS 512 // control words of a launch (frame kernel: prt_frame.h PRT_CTRL_CURSORS; claim cursor of the G-buffer kernel)
#define PRT_STICKY_WORDS 160 // behind the control words and NEVER cleared by a render: [0] error flags of any earlier launch (1 watchdog, 2 stack
                             // overflow), [2] + [8..135] the first watchdog reports; read and cleared by prt_hip_get_stats, read by download / gather
#define PRT_TIMING_RING 32

// thread-local message behind prt_hip_last_error(); returns `code`
int prt_fail(int code, const std::string& msg);
const std::string& prt_last_error_string();

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return prt_fail(e_ == hipErrorOutOfMemory ? PRT_HIP_ENOMEM : PRT_HIP_ENODEVICE,             \
                            std::string(#expr) + ": " + hipGetErrorString(e_));                         \
    } while (0)

// Geometry updates (prt_refit.hip): what prt_hip_update_meshes needs beside the arrays of DevScene, kept at upload.  It lives in the
// context, not in DevScene, which is a by-value argument of the render kernels.
struct PrtRefitMesh {
    uint32_t slotBase = 0, slotCount = 0; // the mesh's triangle slots in tris / shade / bump
    uint32_t vertexCount = 0, hasNormals = 0;
    uint32_t primCount = 0;               // triangles of the mesh (slotCount minus the pad slots): the range of a caller's primId (prt_query.hip)
    uint32_t rootKid = 0;                 // the root as a kid word (see PrtRefit::kids)
    std::vector<std::pair<uint32_t, uint32_t>> levels; // per depth (root's record first): {first entry in levelList, entries}
    DevBuf<float> dPos;                   // staging of the caller's positions / normals (3 * vertexCount floats), allocated by the first update
    DevBuf<float> dNrm;
    // device-side deformation (prt_deform.hip)
    float vbox[6] = {};                   // Mesh::calculateBounds of the current positions (lower, upper), over ALL vertices
    bool vboxValid = false;               // false after prt_hip_update_meshes: reduced from dPos when next needed
    DevBuf<uint32_t> csrOff;              // incidence list, built by the first PRT_HIP_NORMALS_RECOMPUTE: vertexCount + 1 offsets,
    DevBuf<uint32_t> csrFace;             // one face per corner (faces descending, corners ascending within a face),
    DevBuf<uint32_t> faceVtx;             // the index buffer (3 per face, mesh order) and
    DevBuf<float> faceNrm;                // the face normals of the last recompute (3 per face)
    bool sahCaptured = false;             // sahUpload holds {internalArea, leafArea, rootArea} of the tree as uploaded
    double sahUpload[3] = {};
};
// One mesh of a refit whose arrays are already on the device (prt_refit_queue): pos / nrm are what the gather kernel reads
struct PrtRefitSrc {
    uint32_t mesh;
    const float* pos;
    const float* nrm; // NULL: the shade records keep their normals
};
struct PrtRefit {
    std::vector<PrtRefitMesh> meshes;
    DevBuf<uint32_t> slotVtx;      // 3 vertex ids (within the mesh) per triangle slot; 0xffffffff in a pad slot
    DevBuf<uint2> kids;            // per wide record: its two children -- a leaf reference as the record holds it, or the child's own
                                   // record index (a PRT_REF_HOT reference resolved)
    DevBuf<uint32_t> levelList;    // record indices by mesh and depth (PrtRefitMesh::levels)
    DevBuf<uint32_t> hotOrder;     // record index of every hot slot
    uint32_t hotCount = 0;
    DevBuf<float> rootOut;         // device: PRT_MAX_BVH x 6 floats, the refitted root boxes
    HostBuf<float> rootHost;       // pinned host copy of it
    // prt_deform.hip, allocated on first use: the vertex boxes of a call (PRT_MAX_BVH x 6 floats), their pinned host copy, and the
    // per-block partials of the box and SAH reductions
    DevBuf<float> vboxOut;
    HostBuf<float> vboxHost;
    DevBuf<float> boxPartial;
    DevBuf<double> sahPartial;
};

// Scene edits (prt_edit.hip): what the checks of prt_hip_update_materials / prt_hip_update_textures need from the upload, kept on the host.
struct PrtEditMesh {
    uint32_t matBase = 0;                // first record of the mesh in DevScene::mats
    std::vector<prt_material> materials; // as uploaded, then as last updated
};
struct PrtEdit {
    std::vector<PrtEditMesh> meshes;
    std::vector<uint4> texDesc;        // per texture: {offset in DevScene::texels, width, height, component}
    std::vector<uint32_t> classWordOf; // per texture: first word of its alpha cell classes, 0xffffffff = none were built
};

// The owners of the arrays DevScene points to (prt_device.h), under the names it gives them.  DevScene is the by-value kernel argument,
// a read-only view; host code that rewrites an array in place takes the pointer from here, and an array's size is its size().
struct PrtSceneArrays {
    DevBuf<float4> wnodes, hotNodes;
    DevBuf<float> tris;
    DevBuf<uint32_t> triAlpha, triPrim;
    DevBuf<float4> shade, bump, mats, alpha; // bump holds records exactly when some material of the scene names a bump map
    DevBuf<uint32_t> alphaClass;
    DevBuf<uint4> texDesc;
    DevBuf<uint8_t> texels;
    DevBuf<float4> envTexels; // the four of the environment light: empty without one
    DevBuf<float> envV, envHor;
    DevBuf<int32_t> envFirstX;
    bool anyBump() const { return bump.size() != 0; }
};

// Every event, device buffer and pinned buffer of the context is a member that owns it (DevEvent, DevBuf, HostBuf) and goes with
// `delete c`.  The stream alone stays a raw handle: created in prt_hip_create and destroyed in prt_hip_destroy, one place each.
struct prt_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // Timing: a fixed ring of event pairs, one pair per render launch.  When the ring is full the oldest launches are folded
    // into accMs (they have long finished), so a caller that renders in a loop without reading the stats holds no more than
    // PRT_TIMING_RING pairs.
    DevEvent evT0[PRT_TIMING_RING], evT1[PRT_TIMING_RING]; // each created when the ring first reaches it
    uint32_t ringUsed = 0;
    double accMs = 0.0, lastMs = 0.0;
    uint64_t accLaunches = 0;
    int computeUnits = 0;
    std::string name;
    // scene
    bool haveScene = false, haveCamera = false;
    DevScene sc{};
    DevCamera cam{};
    PrtSceneArrays arr;         // sc's pointers are prt_scene_view's copies of these
    PrtRefit rf;
    PrtEdit ed;
    // render resources.  Every device buffer of the context is a DevBuf (prt_devbuf.h): it is freed with the context, and a (re)allocation
    // synchronises the context's stream before the old memory goes.
    DevBuf<float> fb;           // the context's own framebuffer, at the size of the camera it was last rendered or uploaded for
    DevBuf<uint32_t> work;      // PRT_WORK_WORDS control words of a launch + PRT_STICKY_WORDS
    DevBuf<unsigned long long> counters;
    DevEvent evIn, evOut;       // order the pipeline against a caller's stream
    DevBuf<char> wfBuffer;      // the frame kernel's pool state and ray queues
    DevBuf<uint32_t> spill;     // spill columns of the traversal stacks: [entry][thread], two words per entry (prt_launch_resources)
    uint32_t spillThreads() const { return (uint32_t)(spill.size() / (2 * (PRT_STACK_MAX - PRT_STACK_LDS_PACKET))); }
    uint32_t lastRank = 0, lastNranks = 0, lastTile = 0; // of the last render (prt_hip_gather*)
    // image gather (prt_gather.hip): tile-major staging buffers and the RCCL communicator
    void* comm = nullptr;       // ncclComm_t
    bool commOwned = false;     // created by prt_hip_comm_init (destroyed with the context) or adopted from the host
    bool commBroken = false;    // a send / receive failed: the communicator is refused until it is replaced (prt_gather.hip)
    int commRank = 0, commSize = 0;
    DevBuf<float> packBuf;      // this rank's tiles, tile-major
    DevBuf<float> stageBuf;     // root: the other ranks' tiles as received
    int frameBlocksPerCU = 0;   // resident blocks per CU of the frame kernel
    // progressive rendering (prt_hip_render_accumulate): one record per camera pixel, allocated on first use
    DevBuf<uint32_t> accRng;     // generator state
    DevBuf<float4> accSum;       // colour sum, bits(count)
    bool accClear = true;        // the records must be zeroed before the next use (a reset since the last pass)
    uint32_t accMax = 0;         // upper bound of any pixel's count; 0 = empty, the estimator is not bound yet
    uint32_t accSeed = 0, accMaxDepth = 0, accRrDepth = 0; // the estimator the accumulated samples came from (accMax > 0)
    // adaptive sampling (prt_hip_render_adaptive): allocated on first use
    DevBuf<float4> accMom;       // per camera pixel: {mean, M2, bits(m), 0}
    bool momClear = true;        // the moment records must be zeroed before their next use
    DevBuf<uint32_t> adCode;     // per work item of a pass: its pixel code (the selection's output)
    DevBuf<uint32_t> adList;     // the compacted codes of the active pixels, padded to a multiple of 64 (the frame kernel's input)
    DevBuf<uint8_t> adFlag;      // per work item: 1 = active
    DevBuf<char> adTemp;         // hipcub scratch of the compaction
    DevBuf<uint32_t> adCount;    // active pixels of the last selection
    HostBuf<uint32_t> adCountHost; // pinned host copy of it
    DevBuf<float> adErr;         // prt_hip_accum_error: the rectangle's errors
    // denoised previews (prt_denoise.hip): guide and scratch planes at the camera's size, allocated on first use
    DevBuf<float> dnAlbedo;      // guide planes, 3 floats per pixel: the average of dnGuideK G-buffer launches, or the host's own
    DevBuf<float> dnNormal;
    DevBuf<float4> dnGuideA;     // packed for the taps: {A.xyz, valid ? 1 : 0}
    DevBuf<float4> dnGuideN;     // {N.xyz, 0}
    DevBuf<float4> dnPlane[2];   // ping-pong {C.xyz, V}
    bool dnGuidesValid = false;  // dnAlbedo / dnNormal hold the library's guides for (dnGuideSeed, dnGuideK) and the current view
    bool dnHostGuides = false;   // dnAlbedo / dnNormal hold planes the host supplied (prt_hip_denoise_set_guides)
    uint32_t dnGuideSeed = 0, dnGuideK = 0;
    int dnLast = -1;             // dnPlane[dnLast].w is V_final of the last denoise (-1: none yet)
    // temporal reprojection (prt_temporal.hip): the position guide and the history / pending records, allocated on first use
    DevBuf<float4> tpPos;        // {X.xyz, t} per camera pixel: the library's (tpPosValid) or the host's own (tpHostPos)
    bool tpPosValid = false, tpHostPos = false;
    DevBuf<float4> tpHist[3];    // {hC.xyz, hV}, {hX.xyz, hLen}, {hN.xyz, 0}
    DevBuf<float4> tpPend[3];
    bool tpHaveHist = false, tpHavePend = false;
    prt_camera_desc tpHistCam{}, tpPendCam{};
    // display transform (prt_display.hip): allocated on first use; neither the camera nor the scene touches any of it
    DevBuf<prt_display_state> dpState; // the adaptation state and the figures of the last metering
    DevBuf<uint32_t> dpHist;           // the histogram of the metering under way, then the ignored count (64 bits)
    DevBuf<uint8_t> dpOut;             // the context's display buffer
    uint32_t dpOutW = 0, dpOutH = 0, dpOutFormat = 0; // image it last held (prt_hip_download_display)
    // ray queries (prt_query.hip): allocated on first use
    DevBuf<uint32_t> qInv;             // with the scene: slot base of the mesh + mesh-order primId -> triangle slot (0xffffffff: none)
    DevBuf<unsigned long long> qCounts; // records the last prt_hip_query_surface refused
    PrtStage stage;                    // PRT_HIP_QUERY_HOST, every family: the caller's arrays and the answers of the call under way
    // baking (prt_bake.hip): allocated on first use
    DevBuf<prt_ray> bkRays;            // prt_hip_bake: the n*K rays and
    DevBuf<float> bkRad;               // their radiances, which never leave the device, in either flavour
    // lightmap atlases (prt_atlas.hip): allocated on first use
    DevBuf<uint32_t> atOwner;          // prt_hip_atlas_rasterize: per texel the smallest key (meshId << 28) | primId that covers it,
    DevBuf<uint8_t> atFlag;            // 1 = the texel is owned, and
    DevBuf<uint32_t> atIndex;          // its index: what the selection compacts
    DevBuf<char> atTemp;               // hipcub scratch of the selection
    DevBuf<unsigned long long> atCounts;    // {pairs, rejected, degenerate, n} of the last rasterise and
    HostBuf<unsigned long long> atCountsHost; // their pinned host copy
    DevBuf<uint8_t> atScratchMask;     // the mask the passes of a prt_hip_atlas_resolve work on when its caller wants none
    // lightmap filter (prt_atlas_filter.hip): allocated on first use
    DevBuf<uint32_t> afMap;            // per texel the placed point, and
    DevBuf<float4> afRec;              // per point {bits(placed), f2, V0, 0}
    DevBuf<float> afPlane[2];          // ping-pong between the launches: n*stride floats of C, then n of V
    // visibility baking (prt_visibility.hip): allocated on first use
    DevBuf<uint8_t> vsOcc;             // prt_hip_bake_visibility without a caller's array: the n*K occlusion bytes
};


// prt_gather.hip: ends an owned communicator
void prt_gather_release(prt_hip_ctx* c);
// prt_context.hip: 0, or the error code of a launch since the last prt_hip_get_stats whose image must not be trusted (the context's
// stream must be idle); `clear` consumes it (prt_hip_get_stats), download / gather only report it
int prt_sticky_error(prt_hip_ctx* c, bool clear);
// prt_context.hip, the scaffold of an entry point.  Each returns PRT_HIP_OK or the code of the error it has recorded.
// The rectangle lies inside the camera's image.
int prt_check_rect(const prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
// The work of an entry point runs on the context's own stream; a caller's stream is ordered around it with two events: work queued
// on it before prt_stream_enter is finished before the context's stream goes on, and whatever the caller queues after
// prt_stream_leave waits for it.  *caller = the stream to hand to prt_stream_leave, or null when there is nothing to order (no
// stream given, or the context's own).  An error return skips the leave.
int prt_stream_enter(prt_hip_ctx* c, void* stream, hipStream_t* caller);
int prt_stream_leave(prt_hip_ctx* c, hipStream_t caller);
// The scaffold of an entry point whose arrays are host memory under PRT_HIP_QUERY_HOST and device memory otherwise: io lists them
// (prt_stage.h), launch() queues the work on the context's stream and reads the device pointers out of io[].dev.  Host arrays are
// staged in the context's arena: copied in, launch(), copied out, and the stream is synchronised.  Device arrays are refused with
// PRT_HIP_EINVAL and alignmentMessage, before anything is queued or allocated, when a pointer misses its alignment; then launch()
// runs between prt_stream_enter and prt_stream_leave.  The parts that are no template: prt_context.hip.
int prt_io_begin(prt_hip_ctx* c, uint32_t flags, void* stream, const std::string& alignmentMessage, PrtIoArray* io, uint32_t count, hipStream_t* caller);
int prt_io_end(prt_hip_ctx* c, uint32_t flags, const PrtIoArray* io, uint32_t count, hipStream_t caller);
template <typename Launch>
int prt_run_io(prt_hip_ctx* c, uint32_t flags, void* stream, const std::string& alignmentMessage, PrtIoArray* io, uint32_t count, Launch launch)
{
    hipStream_t caller;
    int rc;
    if ((rc = prt_io_begin(c, flags, stream, alignmentMessage, io, count, &caller)) || (rc = launch())) return rc;
    return prt_io_end(c, flags, io, count, caller);
}
// EINVAL "<what>: unknown flag bits" for any bit but PRT_HIP_QUERY_HOST
int prt_check_flags(uint32_t flags, const char* what);
// *d_rgb == NULL becomes the context's own framebuffer, (re)allocated at the camera's size and cleared on the context's stream.
int prt_own_framebuffer(prt_hip_ctx* c, float** d_rgb);
// After a kernel launch: PRT_HIP_ELAUNCH "<kernel> launch: ..." when the runtime refused it.
int prt_launched(const char* kernel);
// The next event pair of the timing ring (prt_hip_ctx::evT0): record ev0 before and ev1 after the launch that prt_hip_get_stats is to time.
int prt_timing_pair(prt_hip_ctx* c, hipEvent_t* ev0, hipEvent_t* ev1);
// The spill columns of the traversal stacks for a launch of `blocks` workgroups.
int prt_launch_resources(prt_hip_ctx* c, uint32_t blocks);
// One launch of a batch kernel (prt_batch.h) over `items` rays on the context's stream, `resident` workgroups at the most.  begin
// sizes the spill columns, clears the statistics and the control words and fills L.ctl and L.blocks; the caller launches L.blocks
// workgroups of PRT_BLOCK threads with L.ctl in the kernel's arguments; end reports a refused launch under the kernel's name.
// timed: prt_hip_get_stats counts and times the launch as it does a render (an event pair of the timing ring around it).
struct BatchLaunch {
    BatchCtl ctl;
    uint32_t blocks;
    hipEvent_t ev1; // timed: recorded behind the launch; else null
};
int prt_batch_begin(prt_hip_ctx* c, uint64_t items, uint32_t resident, bool timed, BatchLaunch* L);
int prt_batch_end(prt_hip_ctx* c, const BatchLaunch& L, const char* kernel);
// prt_kernels.hip, for prt_hip_query_radiance (prt_query.hip): one launch of the frame kernel's probe instantiation over n checked
// probes on the context's stream, timed as a render: d_rays and d_radiance (3 * n floats) are device memory, p has been checked
int prt_frame_probe(prt_hip_ctx* c, uint32_t n, const prt_ray* d_rays, const prt_render_params* p, float* d_radiance);
// prt_query.hip, shared with prt_bake.hip: every refusal of prt_hip_query_radiance for n probes under p and flags, under the caller's
// name; and the answer to a NULL argument (ENODEVICE on a machine without a device, EINVAL otherwise)
int prt_check_radiance(prt_hip_ctx* c, uint32_t n, const prt_render_params* p, uint32_t flags, const char* what);
int prt_null_argument(const char* what);
// prt_query.hip, shared with prt_hip_atlas_points (prt_atlas.hip): the inverse of triPrim for the uploaded scene (prt_hip_ctx::qInv),
// built on the context's stream by the first use after an upload
int prt_query_inverse_ready(prt_hip_ctx* c);
// prt_query.hip, shared with the same: triangles per mesh of the uploaded scene, the range of a caller's primId
void prt_query_prim_counts(const prt_hip_ctx* c, uint32_t primCount[PRT_MAX_BVH]);
// prt_upload.hip: frees the scene's device arrays (prt_hip_destroy; a new upload)
void prt_free_scene(prt_hip_ctx* c);
// prt_upload.hip, the ONE place that writes a pointer of c->sc: each from its owner in c->arr (null where the owner is empty).  Called
// when owners have changed: the upload, an environment map handed over or removed (prt_edit.hip), prt_free_scene.
void prt_scene_view(prt_hip_ctx* c);
// v on the device in b, which holds exactly v.size() elements afterwards (synchronous; `stream` as for DevBuf::fit)
template <typename T> int prt_upload(DevBuf<T>& b, const std::vector<T>& v, hipStream_t stream)
{
    HIP_TRY(b.fit(v.size(), stream));
    if (!v.empty()) HIP_TRY(hipMemcpy(b, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PRT_HIP_OK;
}
// The ONE place that writes a material record (prt_hip_upload_scene, prt_hip_update_materials); its size is tied to the stride the
// kernels index with (sample_diffuse, sample_bump, shade_kernel: sc.mats + PRT_MAT_STRIDE * material).  A record count and an index
// stride that disagree read another material's fields as texture descriptors -- a wild texel address on the device.  texDesc: per
// texture {offset, width, height, component}; the caller has checked both map indices against it.
inline void prt_material_record(const prt_material& mt, const std::vector<uint4>& texDesc, float4* out)
{
    auto ubits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    const uint4 dd = mt.diffuseMap >= 0 ? texDesc[mt.diffuseMap] : make_uint4(0, 0, 0, 0);
    const uint4 bd = mt.bumpMap >= 0 ? texDesc[mt.bumpMap] : make_uint4(0, 0, 0, 0);
    const float4 record[] = {
        make_float4(mt.diffuse[0], mt.diffuse[1], mt.diffuse[2], ubits(mt.reflectionType)),
        make_float4(mt.emissive[0], mt.emissive[1], mt.emissive[2], ubits(mt.alphaTest)),
        make_float4(ubits((uint32_t)mt.diffuseMap), ubits((uint32_t)mt.bumpMap), 0.0f, 0.0f),
        make_float4(ubits(dd.x), ubits(dd.y), ubits(dd.z), ubits(dd.w)),
        make_float4(ubits(bd.x), ubits(bd.y), ubits(bd.z), ubits(bd.w)),
    };
    static_assert(sizeof(record) / sizeof(record[0]) == PRT_MAT_STRIDE, "material record size and PRT_MAT_STRIDE must agree");
    for (int k = 0; k < PRT_MAT_STRIDE; k++) out[k] = record[k];
}
// Progressive rendering: the accumulator holds no samples from here on (its records are zeroed before their next use).
inline void prt_accum_forget(prt_hip_ctx* c)
{
    c->accClear = true;
    c->accMax = 0;
    c->momClear = true; // and no moments (adaptive sampling)
}
// prt_refit.hip: called by prt_hip_upload_scene (prt_upload.hip) once the scene arrays are on the device, with the wide records as uploaded (hot
// references in place), the record of every hot slot, and per mesh its slot range, vertex count and root reference
// (PrtRefitMesh::rootKid = DevScene::rootRef on entry); prt_refit_forget drops the state with the scene
int prt_refit_build(prt_hip_ctx* c, const std::vector<float4>& wnodes, const std::vector<uint32_t>& hotOrder, std::vector<PrtRefitMesh>&& meshes,
                    const std::vector<uint32_t>& slotVtx);
void prt_refit_forget(prt_hip_ctx* c);
// prt_refit.hip, shared with prt_hip_deform_meshes (prt_deform.hip): every refusal of prt_hip_update_meshes; the staging buffers of the
// named meshes (normals too where `normals` is set); gather, levels and finish of the named meshes queued on s, reading device
// arrays (tm, optional, 3 marks: before the gathers, after them, after the finish kernel); and, once the context's stream has been
// synchronised behind the copy of rootOut to rootHost, the root boxes, the radius (0 keeps it) and everything the call invalidates
int prt_refit_check(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* u);
int prt_refit_staging(prt_hip_ctx* c, uint32_t count, const prt_mesh_update* u);
int prt_refit_queue(prt_hip_ctx* c, uint32_t count, const PrtRefitSrc* src, hipStream_t s, StageTimer* tm);
void prt_refit_commit(prt_hip_ctx* c, uint32_t count, const uint32_t* meshes, float radius);
// prt_deform.hip: the SAH sums of the mesh's tree as uploaded, kept before its first update (PrtRefitMesh::sahUpload)
int prt_deform_capture_sah(prt_hip_ctx* c, uint32_t mesh);
// prt_denoise.hip: the view or the scene changed, or the planes are new (guides of either origin are dropped)
void prt_denoise_forget(prt_hip_ctx* c);
// prt_denoise.hip, for the temporal stage (prt_temporal.hip), which replaces the prepare step and then runs the same iterations:
// the checks of prt_hip_accum_denoise; the guide planes for K jitters; the iterations on dnPlane[0] -> d_rgb (tm, optional: one
// mark after every launch)
int prt_denoise_checks(prt_hip_ctx* c, const prt_denoise_params* d);
int prt_denoise_guides_ready(prt_hip_ctx* c, uint32_t K);
int prt_denoise_iterations(prt_hip_ctx* c, const prt_denoise_params* d, float exposure, float* d_rgb, StageTimer* tm);
// prt_temporal.hip: the view changes to `next` (pending becomes history when the size stays, else both go; the position guide
// goes stale); the scene changed or prt_hip_history_reset (both records go)
void prt_temporal_camera_change(prt_hip_ctx* c, const prt_camera_desc* next);
void prt_temporal_forget(prt_hip_ctx* c);
// prt_select.hip: hipcub::DeviceSelect::Flagged of n pixel codes on stream s (stable: the selected codes keep their order); with
// temp == nullptr it only sets tempBytes
hipError_t prt_select_flagged(void* temp, size_t& tempBytes, const uint32_t* in, const uint8_t* flags, uint32_t* out, uint32_t* count,
                              uint64_t n, hipStream_t s);
