/*
 * prt_hip.h -- C-ABI of libprt_hip.so: the MI355X (gfx950) implementation of PRT's per-pixel
 * path-tracing loop.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * The reference (amada/PRT) has no FFI of its own: its hot path is entered through one C++
 * call, PathTracer::TraceBlock(Image&, x0,y0,x1,y1, const Scene&, const Camera&, samples)
 * (path_tracer.h:20, called from main.cpp:146-147), on data owned by Scene/Bvh/Mesh.  The entry
 * points below are what that call binds to when the loop runs on the GPU; each cites the
 * reference interface it replaces (file:line under /root/reference/src).  INTEGRATION.md shows the
 * host-side binding.
 *
 * Conventions: every function returns 0 on success or a negative PRT_HIP_E* code;
 * prt_hip_last_error() gives the message (thread local).  The caller owns all host pointers; the
 * library copies what it needs during the call.  One context per device; calls on one context are
 * serialised by the caller; contexts on different devices are independent.
 */
#ifndef PRT_HIP_H
#define PRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_HIP_OK 0
#define PRT_HIP_ENODEVICE (-1) /* no HIP device / HIP runtime failure: the product has no CPU path */
#define PRT_HIP_EINVAL (-2)
#define PRT_HIP_ENOMEM (-3)
#define PRT_HIP_ELAUNCH (-4)
#define PRT_HIP_ESTATE (-5)    /* scene or camera not uploaded */
#define PRT_HIP_ESTACK (-6)    /* traversal stack deeper than 64 entries (reference asserts, bvh.cpp:552) */
#define PRT_HIP_ECOMM (-7)     /* RCCL: library not found or a communicator call failed */

#define PRT_HIP_MAX_BVH 8

typedef struct prt_hip_ctx prt_hip_ctx;

/* Material fields the path reads (material.h:30-44).  reflectionType: 0 diffuse, 1 specular,
 * 2 refraction (material.h:24-28).  diffuseMap/bumpMap index prt_scene_desc.textures, -1 = none.
 * Any float is accepted in diffuse and emissive (and in a directional light); the image is what the reference computes from them.
 * Refraction is undefined in the reference (path_tracer.cpp never writes the path's next direction and normalises stack
 * contents); here it is defined: a refraction surface scatters along a ZERO direction in every bounce, i.e. it sends one
 * counted ray that misses, and the path's emission and its pending light addend still count. */
typedef struct {
    float diffuse[3];
    float emissive[3];
    uint32_t reflectionType;
    uint32_t alphaTest;
    int32_t diffuseMap;
    int32_t bumpMap;
} prt_material;

/* LinearBvhNode (bvh.h:49-60) with the bit-fields widened. */
typedef struct {
    float lower[3];
    float upper[3];
    uint32_t primOrSecondNodeIndex;
    uint32_t triVectorIndex;
    uint32_t primCount; /* 0xf = internal */
    uint32_t splitAxis;
} prt_bvh_node;

/* One Bvh and the Mesh it owns (bvh.h:113-119, mesh.h:87-104), as built by Bvh::build. */
typedef struct {
    uint32_t nodeCount;
    const prt_bvh_node* nodes;     /* Bvh::m_nodes, DFS order, first child = i+1 */
    uint32_t primCount;
    const uint32_t* primRemapping; /* Bvh::m_primRemapping */
    uint32_t vertexCount;
    const uint32_t* indices;       /* 3*primCount */
    const float* positions;        /* 3*vertexCount */
    const float* normals;          /* 3*vertexCount or NULL (Mesh::hasVertexNormal) */
    const float* texcoords;        /* 2*vertexCount or NULL (Mesh::m_hasTexcoord) */
    uint32_t materialCount;
    const uint32_t* primMaterial;  /* primCount */
    const prt_material* materials;
} prt_mesh_desc;

/* Texture (texture.h:15-24), 8-bit unorm texels, `component` bytes per texel. */
typedef struct {
    int32_t width, height, component;
    const uint8_t* texels;
} prt_texture_desc;

/* What Scene holds for the path (scene.h:61-71): BVHs in Scene::add order, lights, radius. */
typedef struct {
    uint32_t meshCount;
    const prt_mesh_desc* meshes;
    uint32_t textureCount;
    const prt_texture_desc* textures;
    uint32_t hasDirectionalLight; /* Scene::isLightAvailable(kDirectional) */
    float lightDir[3];
    float lightIntensity[3];
    float radius;                 /* Scene::getRadius() */
    /* InfiniteAreaLight (light.h:28-50), tested before the directional light (path_tracer.cpp:164-173): the float RGBA
     * image (Texture::loadExr: 4 floats per texel, row 0 first) and the two CDF tables InfiniteAreaLight::create builds
     * (light.cpp:30-84).  The library copies all three. */
    uint32_t hasInfiniteAreaLight; /* Scene::isLightAvailable(kInfiniteArea) */
    int32_t envWidth, envHeight;
    const float* envTexels;        /* 4*envWidth*envHeight */
    const float* envVerticalP;     /* m_verticalP[envHeight] */
    const float* envHorizontalP;   /* m_horizontalP[envWidth*envHeight] */
} prt_scene_desc;

/* Camera after Camera::create (camera.h:17-36, 46-53). */
typedef struct {
    float pos[3], dir[3], up[3], right[3];
    uint32_t width, height;
    float invWidth, invHeight;
} prt_camera_desc;

/* The literals of the reference's loop, as parameters (SURVEY.md 5 "Config / flags"). */
typedef struct {
    uint32_t samples;  /* kSamples, main.cpp:125; a multiple of 8 (path_tracer.cpp:65) */
    uint32_t maxDepth; /* 14, path_tracer.cpp:124 */
    uint32_t rrDepth;  /* Russian roulette when depth > rrDepth; 4, path_tracer.cpp:258 */
    uint32_t seed;     /* per-pixel generator state = lowbias32(x + y*W + seed) | 1 (replaces random.h:15-17) */
    float exposure;    /* Image::m_exposure, image.cpp:45 */
    uint32_t tileSize; /* 16, main.cpp:123-124; tile t is rendered when t % nranks == rank */
    uint32_t rank, nranks;
    uint32_t countTraffic; /* also count box/triangle/surface/tap events (slower; not for timing) */
} prt_render_params;

/* stats.h:10-16 + the algorithmic-traffic events of DESIGN.md */
typedef struct {
    uint64_t raysTraced;     /* path_tracer.cpp:62,219,242,276 */
    uint64_t occludedTraced; /* path_tracer.cpp:220,243 */
    uint64_t nBox, nTri, nHit, nTap, nPx;
    /* the traversal events again, per traversal (0 primary packets, 1 scatter rays, 2 packet / 3 single occlusion rays); the taps
     * here are the alpha tests inside leaves -- nTap minus their sum are the shading taps (countTraffic launches only) */
    uint64_t modeBox[4], modeTri[4], modeTap[4];
    uint64_t stackOverflow;  /* lanes that needed more than 64 stack entries (must be 0) */
    double kernelMs;         /* HIP-event time of the last render's kernel (events on the launch stream) */
    double kernelMsSum;      /* sum over the render launches since the previous prt_hip_get_stats */
    uint64_t kernelLaunches; /* number of those launches; the event counters above are of the LAST launch */
} prt_hip_stats;

/* RayHitT (ray.h:182-198) */
typedef struct {
    float t, i, j, k;
    uint32_t primId, meshId;
} prt_hit;

/* ---- context ---- */
int prt_hip_device_count(void);
int prt_hip_create(int device, prt_hip_ctx** out);
void prt_hip_destroy(prt_hip_ctx* ctx);
const char* prt_hip_last_error(void);
/* First 16 hex digits of the SHA-256 over the kernel sources THIS library was built from (stamped at build time): a host that
 * quotes measurements (bench.py, the counter summaries under profiles/) compares what is loaded, not what lies in the tree. */
const char* prt_hip_source_sha16(void);
/* fills name (<= cap bytes) and the CU count of the context's device */
int prt_hip_device_info(prt_hip_ctx* ctx, char* name, size_t cap, int* computeUnits);

/* ---- data: replaces the pointers PathTracer reaches through const Scene& / const Camera&
 *      (scene.h:61-71 -> bvh.h:113-119 -> mesh.h:87-104; camera.h:46-53) ---- */
int prt_hip_upload_scene(prt_hip_ctx* ctx, const prt_scene_desc* scene);
int prt_hip_set_camera(prt_hip_ctx* ctx, const prt_camera_desc* camera);

/* ---- Bvh::build on the GPU: the reference's binned-SAH build (bvh.cpp:31-171) and depth-first linearisation
 * (bvh.cpp:230-299) level by level on the device, producing the IDENTICAL node array (prt_bvh_node = LinearBvhNode),
 * leaf order and primRemapping that Bvh::build produces on the host -- a mesh descriptor built from them is interchangeable
 * with one from the host builder.  Host pointers: indices 3 * primCount, positions 3 * vertexCount; nodes_out has room for
 * 2 * primCount nodes, primRemapping_out for primCount entries; buildMs (may be NULL) = device time of the build. ---- */
int prt_hip_build_bvh(prt_hip_ctx* ctx, uint32_t primCount, const uint32_t* indices, uint32_t vertexCount, const float* positions,
                      prt_bvh_node* nodes_out, uint32_t* nodeCount_out, uint32_t* primRemapping_out, double* buildMs);

/* ---- the hot path: replaces PathTracer::TraceBlock (path_tracer.cpp:17-33; pixel rectangle
 * INCLUSIVE as there) + Image::writePixel (image.cpp:44-50).  d_rgb is a DEVICE pointer to
 * width*height*3 floats (pixel (x,y) at (x + y*width)*3), or NULL for the context's own
 * framebuffer.  stream is a hipStream_t (NULL = the context's stream): the render -- ONE persistent
 * kernel launch for the whole rectangle, whatever its size -- is ordered after the work already queued
 * on it and before what is queued on it next.  Asynchronous with respect to the host;
 * prt_hip_download / prt_hip_get_stats synchronise. ---- */
int prt_hip_render(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                   const prt_render_params* params, float* d_rgb, void* stream);
/* GbufferVisualizer::TraceBlock (gbuffer_visualizer.cpp:17-51): one jittered camera ray per pixel, the surface's diffuse colour
 * (type 0 = kDiffuse) or bump-mapped normal * 0.5 + 0.5 (1 = kMeshNormal, 2 = kNormal), times exposure.  Same rectangle,
 * framebuffer and stream conventions as prt_hip_render; the pixel's generator state is the same function of (x, y, seed). */
int prt_hip_render_gbuffer(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t type, uint32_t seed,
                           float exposure, float* d_rgb, void* stream);
/* copies the rectangle (inclusive) of the context's framebuffer into a host image of the camera's size */
int prt_hip_download(prt_hip_ctx* ctx, float* rgb_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
float* prt_hip_framebuffer(prt_hip_ctx* ctx); /* device pointer, width*height*3 floats */
/* ---- image gather: the ONE exchange of the multi-GPU path.  The reference has none (one process, one
 * Image, main.cpp:107-190); tiles are dealt to ranks by tile id % nranks (prt_render_params), every rank renders the
 * tiles it owns into its own camera-sized framebuffer and the owned tiles are moved to the root: each rank packs them
 * tile-major (1/nranks of the image: 3.1 MB at 1080p with 8 ranks), the packed tiles travel, the root de-interleaves them
 * into its frame.  No reduction, no full-frame traffic, nothing to zero between frames. ---- */
#define PRT_HIP_COMM_ID_BYTES 128
/* One process per GPU (RCCL over xGMI; librccl is loaded on first use).  Rank 0 makes an id and ships its 128 bytes to the
 * other ranks over any host channel; then EVERY rank calls prt_hip_comm_init (collective).  A host that already owns an
 * ncclComm_t for these ranks hands it over with prt_hip_comm_adopt instead (the library never destroys an adopted one). */
int prt_hip_comm_unique_id(void* id128);
int prt_hip_comm_init(prt_hip_ctx* ctx, const void* id128, int rank, int nranks);
int prt_hip_comm_adopt(prt_hip_ctx* ctx, void* ncclComm);
int prt_hip_comm_destroy(prt_hip_ctx* ctx);
/* Collective, after prt_hip_render(..., params.rank = the communicator's rank, params.nranks = its size, d_rgb, stream) on every
 * rank: grouped ncclSend (owners) / ncclRecv (root), so that each link into the root carries one peer's tiles, then the
 * de-interleave kernel on the root.  d_rgb / stream as in prt_hip_render (the same buffer the render wrote); afterwards the
 * root's buffer holds the whole image, the other ranks' buffers are unchanged.
 * A failing ncclSend / ncclRecv returns PRT_HIP_ECOMM with the RCCL group closed again and marks the communicator BROKEN (RCCL leaves
 * it in an error state): every later gather on this context is refused with PRT_HIP_ECOMM until prt_hip_comm_init or
 * prt_hip_comm_adopt replaces it on every rank (a broken communicator the context owns is ended with ncclCommAbort). */
int prt_hip_gather_rccl(prt_hip_ctx* ctx, float* d_rgb, int root, void* stream);
/* bytes the context's rank contributes to a gather of its last render (what travels over xGMI) */
int prt_hip_gather_payload_bytes(prt_hip_ctx* ctx, uint64_t* bytes);
/* One process driving several contexts: context i has rendered with params.rank = i, params.nranks = n into its own
 * framebuffer (d_rgb = NULL).  The same pack and de-interleave kernels with device-to-device copies in between assemble the
 * image in context 0's framebuffer; the rectangle of it is then copied to rgb_host (camera-sized). */
int prt_hip_gather(prt_hip_ctx* const* ctxs, int n, float* rgb_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
int prt_hip_get_stats(prt_hip_ctx* ctx, prt_hip_stats* stats);

/* ---- progressive rendering: resumable per-pixel sample accumulation.  The context keeps an ACCUMULATOR, one record per camera
 * pixel: the generator state after the pixel's last packet, the float RGB sum of its packets and its sample count.  Across
 * packets the reference carries exactly these two things per pixel (m_rand and color, path_tracer.cpp:57-75), so a pass that
 * resumes from them continues the pixel's one-shot render: after passes of s1, s2, ..., sk samples the image is, bit for bit,
 * the image of ONE prt_hip_render of s1 + ... + sk samples.  The total may exceed prt_hip_render's 2040-sample limit. ---- */
typedef struct {
    uint32_t width, height;           /* the camera's size */
    uint32_t seed, maxDepth, rrDepth; /* the estimator the accumulated samples came from (0 when the accumulator is empty) */
} prt_accum_info;
/* Empties the accumulator (every count 0) and unbinds the estimator.  prt_hip_set_camera and prt_hip_upload_scene do the same, and so
 * does prt_hip_update_meshes.  So do prt_hip_update_lights, prt_hip_update_materials and prt_hip_update_textures ("scene edits"). */
int prt_hip_accum_reset(prt_hip_ctx* ctx);
/* One pass: every pixel of the rectangle (or of rank's tiles in it) renders params->samples more samples, starting from its
 * record (a pixel with count 0 is seeded as prt_hip_render seeds it), stores its state, sum and count back and writes
 * exposure * sum / count to d_rgb.  Rectangle, rank / tile, framebuffer and stream rules are those of prt_hip_render, and
 * prt_hip_gather_rccl / prt_hip_gather work on the output unchanged; prt_hip_get_stats counts this pass's rays only.
 * params->samples: a multiple of 8 from 8 to 2040.  A pass that could take any pixel's count above 2^24 (where a count as a float
 * stops being exact) is refused.  The first pass after a reset binds seed, maxDepth and rrDepth; a pass with other values is
 * refused (mixing two estimators would be a silent error).  exposure may change from pass to pass.  All refusals are
 * PRT_HIP_EINVAL with a message.  The accumulator is allocated at the camera's size on first use; prt_hip_render neither
 * reads nor changes it. */
int prt_hip_render_accumulate(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                              const prt_render_params* params, float* d_rgb, void* stream);
/* Writes exposure * sum / count of the rectangle's records to d_rgb (+0.0 where count is 0) without tracing: the image of the
 * accumulated passes at another exposure.  Framebuffer and stream rules of prt_hip_render. */
int prt_hip_accum_resolve(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float exposure,
                          float* d_rgb, void* stream);
/* Checkpoint / resume.  export copies the whole accumulator to host arrays (waits for the context's stream): rng width*height
 * states, sum 3*width*height floats, count width*height; info gets the size and the bound estimator.  import loads such arrays
 * into a context whose camera has info's size (else PRT_HIP_EINVAL) and binds info's estimator; counts above 2^24 are refused.
 * A context that imports a checkpoint after uploading the same scene and camera continues it as if it had never stopped. */
int prt_hip_accum_export(prt_hip_ctx* ctx, prt_accum_info* info, uint32_t* rng, float* sum, uint32_t* count);
int prt_hip_accum_import(prt_hip_ctx* ctx, const prt_accum_info* info, const uint32_t* rng, const float* sum,
                         const uint32_t* count);

/* ---- adaptive sampling: passes that trace only the pixels whose noise is above a target.  Besides its accumulator record, every
 * pixel has a MOMENT record {mean, M2, bits(m), 0} (16 bytes): Welford's running mean and sum of squared deviations of the mean
 * luminance of its packets of 8 samples, over the m packets adaptive passes gave it.  Only adaptive passes update it: at each packet
 * end, with res the sum of the packet's 8 slot results (f32, no FMA, in this order)
 *     L = (0.2126f*res.x + 0.7152f*res.y + 0.0722f*res.z) * 0.125f;  m += 1; d = L - mean; mean += d / (float)m; M2 += d * (L - mean);
 * The ERROR of a pixel with count n (its accumulator count) at an exposure and a floor: +inf when m < 2, otherwise
 *     var = M2 / (float)(m - 1); se = sqrtf(var / (float)(n >> 3)); err = (exposure * se) / (floor + exposure * mean)
 * (correctly rounded f32 divide and sqrt): the relative standard error of the displayed pixel; floor, in displayed units, lets black
 * pixels converge.  A pass covers the work items of prt_hip_render_accumulate over the same rectangle and rank; an owned pixel is
 * ACTIVE iff n + samples <= maxSamples and (n < minSamples or err > threshold) -- a NaN error counts as converged, +inf as active.
 * Active pixels get params->samples more samples exactly as an accumulate pass gives them, so every pixel holds, bit for bit, the
 * one-shot render of its own count.  Every other owned pixel of the rectangle gets exposure * sum / count (+0 where the count is 0)
 * in d_rgb: after the pass d_rgb over the owned pixels equals prt_hip_accum_resolve at that exposure bit for bit; pixels the rank
 * does not own are left untouched.  prt_hip_render_accumulate neither reads nor updates the moments (after mixed passes a moment
 * covers only the adaptive packets; the error still uses the full n).  prt_hip_accum_reset, prt_hip_accum_import, prt_hip_set_camera
 * and prt_hip_upload_scene zero the moments.  The estimator binding (seed, maxDepth and rrDepth), the multiple of 8 from 8 to 2040
 * per pass and the 2^24 cap are those of prt_hip_render_accumulate.  All refusals are PRT_HIP_EINVAL with a message. ---- */
typedef struct {
    float threshold;     /* relative standard error target (>= 0, finite) */
    float floor;         /* > 0, displayed units: added to exposure*mean in the error's denominator */
    uint32_t minSamples; /* multiple of 8: a pixel below it is always traced */
    uint32_t maxSamples; /* multiple of 8, >= minSamples, <= 2^24: no pixel is taken above it */
} prt_adaptive_params;

/* One adaptive pass. Selection, then one frame-kernel launch over the active pixels only. Synchronises the context's stream
 * once, between the two, to read the active count: *active gets the number of pixels traced. With 0 active, nothing is
 * launched. Rectangle, rank/tile, d_rgb and stream rules are those of prt_hip_render_accumulate.  prt_hip_get_stats counts the
 * pass's rays, and its nPx is *active. */
int prt_hip_render_adaptive(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_render_params* p,
                            const prt_adaptive_params* a, uint32_t* active, float* d_rgb, void* stream);
/* err of every pixel of the rectangle (formula above) into a camera-sized host array at (x + y*width); synchronous.  floor > 0. */
int prt_hip_accum_error(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, float exposure, float floor, float* err);
/* Checkpoint / resume of the moment records: 4*width*height floats {mean, M2, bits(m), 0}. Import after prt_hip_accum_import (which
 * zeroes them); an m above 2^21 (2^24 samples in packets of 8) is refused. */
int prt_hip_accum_export_moments(prt_hip_ctx* ctx, float* mom);
int prt_hip_accum_import_moments(prt_hip_ctx* ctx, const float* mom);

/* ---- denoised previews: an edge-avoiding a-trous wavelet filter (B3 spline, 5x5 taps, hole size doubling per iteration) over the
 * whole camera image of the accumulator, guided by first-hit albedo, first-hit normal and the variance of the moment records, with
 * optional albedo demodulation.  A post-process: it reads the accumulator and the moments and changes neither.  It is specified
 * exactly, so that a restatement in any language gives the same bits: all arithmetic is f32, no FMA, correctly rounded / and sqrtf,
 * subnormals not flushed, in the order written.
 *     lum(c) = 0.2126f*c.x + 0.7152f*c.y + 0.0722f*c.z                                  (left to right)
 *     f(x):  y = 0.125f*x; r = 1.0f / ((1.0f + y) + (0.5f*y)*y); r = r*r; r = r*r; r = r*r;   result r
 *            (the eighth power of the reciprocal of e^(x/8)'s series cut after the square: an exp(-x)-like falloff made of exactly
 *            rounded operations only -- not expf, whose bits differ between libraries)
 *     h[-2..2] = {1/16, 1/4, 3/8, 1/4, 1/16}
 * Per pixel p:
 *     valid_p = count_p > 0
 *     A_p = albedo guide; G_p = normal guide in the G-buffer's encoding (0.5*n + 0.5 per hit, exactly (0,0,0) per miss, averaged
 *           over the guide jitters);  N_p = (0,0,0) if G_p is exactly (0,0,0) (every jitter missed), else (G_p - 0.5f) * 2.0f per
 *           component, NOT renormalised (a pixel straddling an edge has a short normal, hence a small wn to both sides)
 *     c_p = sum_p / (float)count_p per channel
 *     v_p = (M2 / (float)(m - 1)) / (float)(n >> 3) when m >= 2, else -1 ("unknown"): moment record {mean, M2, m}, n = count_p;
 *           the variance of the pixel's mean luminance (se squared, see "adaptive sampling")
 *     demodulate: d_p = max(A_p, 0.015625f) per channel; C0_p = c_p / d_p; V0_p = v_p < 0 ? -1 : v_p / (lum(d_p)*lum(d_p))
 *     otherwise:  d_p = 1; C0_p = c_p; V0_p = v_p
 * Iteration i = 0 .. iterations-1, step s = 1 << i, from planes (C, V) to (C', V').  For a valid p:
 *     L_p = lum(C_p).  If V_p >= 0: g = the 3x3 average of V around p at stride 1, weights {1/16,1/8,1/16; 1/8,1/4,1/8; 1/16,1/8,1/16},
 *         over the taps that are inside the image, valid and have V >= 0, row-major: g = sumVW / sumWt (sumVW += wt*V_q; sumWt += wt);
 *         den = sigmaLuminance * sqrtf(g) + 1e-6f
 *     taps q = p + s*(dx, dy), dy outer -2..2, dx inner -2..2; a tap outside the image or with !valid_q is skipped
 *         q == p:  w = h[0]*h[0]
 *         else     dn = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z; wn = max(dn, 0.0f); then wn = wn*wn, normalPowerLog2 times;
 *                  da = A_p - A_q; wa = f(((da.x*da.x + da.y*da.y) + da.z*da.z) / (sigmaAlbedo*sigmaAlbedo));
 *                  wl = V_p < 0 ? 1.0f : f(fabsf(L_p - lum(C_q)) / den);
 *                  w = (((h[dy]*h[dx]) * wn) * wa) * wl
 *         sumW += w; sumC += w * C_q per channel; if V_p >= 0: sumV += (w*w) * (V_q >= 0 ? V_q : V_p)
 *     C'_p = sumC / sumW per channel; V'_p = V_p < 0 ? -1 : sumV / (sumW*sumW)
 * An invalid p: C'_p = 0, V'_p = -1.
 * Output: d_rgb_p = exposure * (C_final_p * d_p) per channel; +0.0 for an invalid p.
 * What follows from these rules: a pixel all of whose guide jitters missed (background) only ever keeps its own value, since every
 * wn to or from it is 0.  The filter is BIASED where the guides cannot see an edge that the radiance has, most visibly around
 * directly seen emitters, whose HDR edge pixels dominate the absolute error once the noise is low: it is a preview filter for low
 * sample counts, not a substitute for convergence.  A pixel whose variance is unknown gets no luminance edge-stopping; a host
 * that wants it renders with adaptive passes (with minSamples at the target count every pixel below it is active whatever its
 * error: an accumulate pass that also keeps moments).  There is no depth or position guide.  In a multi-rank run it works on
 * whatever this context's accumulator holds: pixels the rank does not own (count 0) stay +0.
 *
 * Comparisons.  Every comparison is the IEEE comparison and false for NaN, here and in "temporal reprojection", and in both blocks
 * max(a, b) means a > b ? a : b, which is b when a is NaN: a NaN albedo channel demodulates by 0.015625f (in the prepare step, the
 * temporal stage and the multiply-back of the output alike), and a NaN dn gives wn = 0.  Within an iteration "V_p < 0" stands for
 * the negation of the test "V_p >= 0" above it: a NaN V_p is unknown (no g, wl = 1.0f, no sumV, V'_p = -1).  Only the prepare
 * step's V0_p = v_p < 0 ? -1 : ... is the literal test: a NaN v_p gives a NaN V0_p, which the first iteration reads as unknown.
 *
 * What follows for non-finite state.  The accumulator may hold NaN and infinite sums (a render of a scene with such materials or
 * lights produces them, and prt_hip_accum_import takes any bits), the moments and the guides likewise.  The filter does not contain
 * them.  Colour: a NaN or +-inf channel of the sum of ONE pixel of a fully valid image makes the output non-finite exactly on the
 * square |dx|, |dy| <= 2*(2^k - 1) around it after k iterations, clipped to the image: 5 x 5, 13 x 13, 29 x 29, 61 x 61 and
 * 125 x 125 pixels.  A weight of 0 does not protect a tap, because 0 * NaN is NaN and 0 * inf is NaN; only taps that are skipped
 * (outside the image, count 0) stop the spread, so a valid pixel among count-0 pixels at all its tap offsets keeps a finite value.
 * An infinity is still an infinity at its own pixel after the first iteration (every other tap there has wl = 0 or w finite) and
 * NaN on the rest of the square; from the second iteration on the whole square is NaN.  Variance: a NaN V is unknown (-1) for good
 * after one iteration and is never read as a tap, so it touches no neighbour.  A +inf V spreads: den becomes infinite and wl = 1
 * wherever the 3x3 average sees it, and sumV takes (w*w) * inf, which is inf, or NaN where w is 0, so every pixel with a known V that
 * taps it ends with an infinite or unknown V while all colours stay finite.  Such a V comes from an import with count < 8 with m >= 2
 * (n >> 3 is 0) or from an infinite M2.  A negative M2 is a negative v: unknown.  Guides: a NaN albedo channel is a source like a NaN
 * sum, with or without demodulation (wa is NaN to and from the pixel), except that a pixel with no other tap comes out as
 * exposure * ((c / 0.015625f) * 0.015625f).  A +inf albedo channel has wa = 0 to every finite neighbour and harms nobody else; with
 * demodulation its own channel is 0 * inf = NaN.  A negative (or -inf) albedo demodulates by 0.015625f, one above 1 by itself: there is
 * no upper clamp.  A NaN normal channel is harmless (every wn to and from the pixel is 0: it keeps its own value, as a miss does).
 * A long normal has wn above 1, and wn raised to 2^normalPowerLog2 can overflow: length 1.04 is finite at every setting, length 40
 * gives w = +inf, or NaN against a weight of 0, and is a source for the taps it has a positive dot product with.  The display
 * transform shows a NaN as 0, so a poisoned square is black on screen.  A host that imports accumulators or guides should check
 * them; prt_hip_accum_denoise does not.
 *
 * Guides: the context owns two camera-sized planes, albedo and normal.  Each is the average of K = guideSamples launches of the
 * G-buffer kernel (prt_hip_render_gbuffer type 0, respectively type 2, exposure 1; launch k = 0..K-1 with seed boundSeed + k, uint32
 * wrap-around, boundSeed = the accumulator's bound seed): g = g_0; g = g + g_k (k = 1..K-1); g = g * (1.0f / K), per float.  They
 * are rendered by the first denoise (or prt_hip_denoise_get_guides) after they became stale: prt_hip_set_camera,
 * prt_hip_upload_scene, another bound seed and another K make them stale (the first two also drop planes the host had set).
 * Rendering them is a G-buffer render for prt_hip_get_stats: read a pass's statistics before denoising it. ---- */
typedef struct {
    uint32_t iterations;      /* 1..5 */
    uint32_t normalPowerLog2; /* 0..7: wn is raised to 2^normalPowerLog2 */
    float sigmaLuminance;     /* > 0, finite */
    float sigmaAlbedo;        /* > 0, finite */
    uint32_t demodulate;      /* 0 or 1 */
    uint32_t guideSamples;    /* K: 1, 2, 4, 8 or 16 */
} prt_denoise_params;
/* The host's own guide planes (host pointers, 3*width*height floats each, pixel (x,y) at (x + y*width)*3; taken at the camera's size
 * on trust); NULL, NULL returns to the library's own.  Synchronous. */
int prt_hip_denoise_set_guides(prt_hip_ctx* ctx, const float* albedo, const float* normal);
/* The planes a denoise with this K uses, to host arrays: renders them if stale; the host's own if set.  Synchronous.
 * PRT_HIP_ESTATE without scene / camera, or with an empty accumulator (no bound seed) unless the host's planes are set. */
int prt_hip_denoise_get_guides(prt_hip_ctx* ctx, uint32_t guideSamples, float* albedo, float* normal);
/* Filters the whole image into d_rgb (d_rgb / stream rules of prt_hip_accum_resolve; asynchronous).  PRT_HIP_EINVAL with a message
 * for a parameter outside its range or a non-finite sigma; PRT_HIP_ESTATE without scene / camera or with an empty (never bound)
 * accumulator.  Scratch planes (88 bytes per pixel) are allocated at the camera's size on first use and freed with the context. */
int prt_hip_accum_denoise(prt_hip_ctx* ctx, const prt_denoise_params* params, float exposure, float* d_rgb, void* stream);
/* V_final of the last denoise into a host array of width*height floats (-1 = unknown or invalid): the variance of the filtered
 * luminance (demodulated if the denoise was).  Synchronous; PRT_HIP_ESTATE when this view has not been denoised. */
int prt_hip_denoise_variance(prt_hip_ctx* ctx, float* var);

/* ---- temporal reprojection: denoised previews that survive camera moves.  What was learnt in the last view is carried into the next
 * one wherever the same surface is still visible: the temporal stage of SVGF in front of the a-trous filter above.  It needs a
 * first-hit POSITION per pixel, which is the guide that filter lacks.  A post-process like the denoiser: it reads the accumulator and
 * the moments and changes neither, and prt_hip_accum_denoise ignores everything below and gives the bits it always gave.  All new
 * arithmetic is specified exactly, as for the filter: f32, no FMA, correctly rounded / and sqrtf, subnormals kept, in the order
 * written.  dot3(u, w) = (u.x*w.x + u.y*w.y) + u.z*w.z.
 *
 * Position guide: one ray per pixel (x, y) through the pixel's CENTRE -- camera_dir (camera.cpp:46-56) with both jitter terms 0.0f:
 *     kAspect = (float)W / (float)H
 *     nx = 2.0f * ((float)x * invWidth - 0.5f + 0.0f) * 0.6f * kAspect                   (left to right)
 *     ny = -2.0f * ((float)y * invHeight - 0.5f + 0.0f) * 0.6f
 *     v = (nx*right + ny*up) + dir per component
 *     dirp = (1.0f / sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)) * v
 * from pos with maxT = 100000.0f through the single-ray nearest-hit traversal: the G-buffer kernel's ray, alpha tests included,
 * without the jitter.  The plane holds {X.x, X.y, X.z, t} per pixel at (x + y*width)*4: for a hit X = pos + t*dirp per component
 * (the product is rounded, then the sum); a miss is {0, 0, 0, -1}.  It is a function of scene and camera only: rendered on first
 * use per view by one launch of a persistent traversal kernel with neither surface fetch nor texture tap, stale after
 * prt_hip_set_camera / prt_hip_upload_scene (which also drop a plane the host had set).  Rendering it is a G-buffer render for
 * prt_hip_get_stats (a stack overflow is reported there, as for prt_hip_render_gbuffer): read a pass's statistics first.
 *
 * Records: the context keeps a HISTORY and a PENDING record, each a camera plus three camera-sized float4 planes
 * {hC.xyz, hV}, {hX.xyz, hLen}, {hN.xyz, 0}: hC is radiance (sum / count, not demodulated, no exposure), hV the variance of its mean
 * luminance (-1 = unknown), hLen the number of samples it stands for, as a float (0 = nothing), hX and hN the position guide and
 * the guide normal N of that view.
 *
 * prt_hip_accum_denoise_temporal does, per pixel p = (x, y), with valid_p, c_p, v_p, N_p, A_p, d_p exactly as "denoised previews"
 * defines them (for an invalid p: c_p = (0,0,0), v_p = -1), {X_p, t_p} from the position guide, hc the history's camera and W, H the
 * image size, which is also the history's:
 *     have = false
 *     if valid_p and t_p >= 0 and a history exists and maxHistory > 0:
 *         e = X_p - hc.pos;  a = dot3(e, hc.right);  b = dot3(e, hc.up);  z = dot3(e, hc.dir)
 *         if z > 0:
 *             fx = ((a / z) / ((2.0f*0.6f) * kAspect) + 0.5f) * (float)W
 *             fy = (0.5f - (b / z) / (2.0f*0.6f)) * (float)H
 *             if fx >= -1.0f and fx < (float)W and fy >= -1.0f and fy < (float)H:          (false for NaN)
 *                 ix = floorf(fx); iy = floorf(fy); tx = fx - ix; ty = fy - iy
 *                 lim = (positionTolerance*positionTolerance) * (t_p*t_p)
 *                 sumW = sumL = sumVh = sumWv = 0; sumC = (0,0,0)
 *                 taps q = (ix + i, iy + j), j = 0,1 outer, i = 0,1 inner; skipped when outside the image or !(hLen_q > 0)
 *                     g = X_p - hX_q;  accepted iff dot3(g, g) <= lim and dot3(N_p, hN_q) >= normalCos
 *                     wb = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty)
 *                     sumW += wb; sumC += wb * hC_q (per channel); sumL += wb * hLen_q
 *                     if hV_q >= 0: sumVh += wb * hV_q; sumWv += wb
 *                 have = sumW > 0.015625f
 *     if have:
 *         Hc = sumC / sumW;  q = sumL / sumW;  Hl = q < maxHistory ? q : maxHistory;  Hv = sumWv > 0 ? sumVh / sumWv : -1
 *         n = (float)count_p;  tot = n + Hl
 *         cm = (n * c_p + Hl * Hc) / tot                                   (per channel)
 *         vm = v_p >= 0 and Hv >= 0 ? ((n*n)*v_p + (Hl*Hl)*Hv) / (tot*tot)
 *            : v_p >= 0 ? (v_p * n) / tot      (a history without a variance is taken to have the pixel's own per-sample variance)
 *            : Hv  >= 0 ? (Hv * Hl) / tot      (and the other way round: the first 8-spp pass of a new view gets its edge-stopping from the history)
 *            : -1
 *         len = tot
 *     else:
 *         cm = c_p;  vm = v_p;  len = valid_p ? (float)count_p : 0
 *     demodulate: C0_p = cm / d_p (per channel);  V0_p = vm < 0 ? -1 : vm / (lum(d_p)*lum(d_p))
 *     otherwise:  C0_p = cm;  V0_p = vm          (no division: lum(1,1,1) is not exactly 1.0f, and without a history these are the plain denoiser's bits)
 *     an invalid p: C0_p = (0,0,0), V0_p = -1, as in the plain denoiser
 *     pending_p = {cm, vm}, {X_p, (valid_p and t_p >= 0) ? len : 0}, {N_p, 0};  pending camera = the current camera
 * The iterations of "denoised previews" then run on (C0, V0) unchanged and write d_rgb.  The history is merged in RADIANCE space,
 * before demodulation (the albedo guide of one surface point differs between two views), and no material or primitive id is used.
 * An invalid pixel stays invalid.  A pixel whose centre ray misses never takes history and never becomes history.  Without a
 * history (fresh context, after a reset, maxHistory = 0) the result is prt_hip_accum_denoise's, bit for bit.
 *
 * Non-finite state (comparisons and max(a, b) as "denoised previews" states them: IEEE, false for NaN).  The merge contains
 * nothing either.  A tap with a NaN hLen is skipped (!(hLen_q > 0)); a +inf hLen is accepted and capped (q < maxHistory is false, so
 * Hl = maxHistory), a denormal one is accepted and weighs nothing.  A NaN hV is not summed (hV_q >= 0 is false); a +inf hV makes Hv and vm
 * infinite, and V spreads from there as an infinite V does.  A NaN v_p or Hv fails its >= 0 test and takes the next branch of vm.
 * A NaN in hX or hN fails the acceptance test; an infinite hN can pass it.  A non-finite history colour enters every merged pixel
 * whose accepted bilinear taps include it, whatever the tap's weight (0 * NaN is NaN): cm is non-finite there, the iterations
 * spread it over the square of "denoised previews", and cm is carried in the pending record into the next history, where it merges
 * again -- with an unchanged camera for as long as the view is denoised.  maxHistory caps the weight of a history, not of a NaN.
 * prt_hip_history_reset ends this (so do prt_hip_upload_scene and a camera of another size); prt_hip_accum_denoise never sees it.
 *
 * Life cycle (what keeps samples from being counted twice):
 *   - a temporal denoise merges with the HISTORY only, never with pending, and overwrites pending: denoising the same view again
 *     after more passes is idempotent in the history and never double counts;
 *   - prt_hip_set_camera with a pending record promotes it to history when the new camera has the same width and height, otherwise
 *     both are dropped; without a pending record (a view that was never denoised) it keeps the history under the same size rule;
 *   - prt_hip_upload_scene and prt_hip_history_reset drop both; prt_hip_accum_reset / prt_hip_accum_import touch neither;
 *   - prt_hip_update_meshes promotes a pending record as a prt_hip_set_camera of unchanged size does ("geometry updates");
 *   - prt_hip_accum_denoise ignores both.
 * The history is BIASED for view-dependent radiance (reflections, highlights): a first-hit position says where the surface is,
 * not what it reflects; maxHistory bounds the history's weight, so that new samples take over (once the noise is low a few such
 * pixels dominate the squared error, as the emitter edges do for the filter).  A host that sets the SAME camera again gets the
 * same per-pixel seeds and therefore the same samples: varying `seed` per view (allowed after the reset that prt_hip_set_camera
 * implies) makes the merged samples independent.  Memory: 16 bytes (position) plus 2 x 48 bytes (history, pending) per pixel,
 * allocated on first use.  In a multi-rank run the stage works on what this context holds, as the denoiser does.  With host guides
 * (prt_hip_denoise_set_guides) the position plane may be the host's too or the library's for the current view. ---- */
typedef struct {
    float positionTolerance; /* finite, > 0: a tap is accepted within positionTolerance * t_p of X_p (0.01) */
    float normalCos;         /* in [-1, 1]: least dot3 of the two guide normals (0.9) */
    float maxHistory;        /* finite, >= 0: cap of the history's length in samples; 0 disables the merge (256) */
} prt_temporal_params;
/* The position plane of the current view into a host array of 4*width*height floats: renders it if stale; the host's own if set.
 * Synchronous.  PRT_HIP_ESTATE without scene / camera. */
int prt_hip_denoise_get_position(prt_hip_ctx* ctx, float* xyzt);
/* The host's own position plane (4*width*height floats, taken at the camera's size on trust); NULL returns to the library's. */
int prt_hip_denoise_set_position(prt_hip_ctx* ctx, const float* xyzt);
/* prt_hip_accum_denoise with the temporal stage in place of its prepare step: parameters, d_rgb / stream rules, refusals and
 * prt_hip_denoise_variance as there; PRT_HIP_EINVAL with a message naming the field for a prt_temporal_params value outside its range
 * or non-finite, PRT_HIP_ESTATE without scene / camera / samples. */
int prt_hip_accum_denoise_temporal(prt_hip_ctx* ctx, const prt_denoise_params* params, const prt_temporal_params* temporal, float exposure,
                                   float* d_rgb, void* stream);
/* Drops history and pending. */
int prt_hip_history_reset(prt_hip_ctx* ctx);
/* Checkpoint and test access.  export: which 0 = history, 1 = pending, into host arrays of 4*width*height floats each ({hC, hV},
 * {hX, hLen}, {hN, 0}) and its camera; synchronous; PRT_HIP_ESTATE when there is none.  import: the arrays become the HISTORY seen
 * from `camera`, whose width and height must be the current camera's (else PRT_HIP_EINVAL); pending is left as it is. */
int prt_hip_history_export(prt_hip_ctx* ctx, uint32_t which, prt_camera_desc* camera, float* colorVar, float* posLen, float* normal);
int prt_hip_history_import(prt_hip_ctx* ctx, const prt_camera_desc* camera, const float* colorVar, const float* posLen,
                           const float* normal);

/* ---- geometry updates: move and deform meshes of the uploaded scene in place.  A mesh's TOPOLOGY stays (the tree's shape, primRemapping,
 * indices, materials, textures, lights); its vertex positions, and optionally its vertex normals, are replaced, and everything
 * prt_hip_upload_scene derives from positions is rewritten on the device by two kernels (prt_refit.hip): the leaf triangles, the face
 * normals of meshes without vertex normals, the vertex normals when given, dp01 / dp02 of the bump records, the child boxes of every
 * node record and their hot copies, the root boxes, the radius.  Node boxes are REFITTED bottom up, in f32:
 *     leaf:      lower = min, upper = max per component over the 3 x primCount vertices of its triangles
 *     internal:  lower = min(child0.lower, child1.lower), upper = max(child0.upper, child1.upper)
 * (min / max of finite floats: exact and order independent except for the sign of a zero).  After the call the context is in exactly
 * the state prt_hip_upload_scene produces from the descriptor with the same topology, the new positions and normals, the given radius
 * and node boxes refitted by this rule.  The reference's builder sets every node's box by the same rule (bvh.cpp:21-29), so for a
 * change that leaves the builder's decisions alone (a translation, a uniform scale by a power of two, ...) that is the state of a
 * rebuild.  A refit never improves a tree: after a large deformation build again (prt_hip_build_bvh) and upload.  Non-finite
 * positions are the caller's error, as they are for the upload.
 *
 * Refusals: PRT_HIP_ESTATE without a scene; PRT_HIP_EINVAL with a message for count 0, a mesh index out of range, a vertexCount other
 * than the uploaded mesh's, NULL positions, normals for a mesh uploaded without, a mesh named twice in one call, a negative or
 * non-finite radius.  A refused call changes nothing.
 *
 * What the call invalidates (the samples and guides of the old geometry):
 *   - the accumulator and the moments are emptied and the estimator unbound, as by prt_hip_accum_reset;
 *   - the denoise guides and the position plane go stale and are rendered again on next use; planes a host had set are dropped, as
 *     prt_hip_set_camera drops them;
 *   - temporal records: a pending record is promoted to the history exactly as prt_hip_set_camera with an unchanged size promotes it;
 *     without a pending record the history is kept.  The position and normal tests of the merge reject every pixel whose first hit
 *     moved, so untouched surfaces keep their history and moved ones start fresh; what the history cannot see -- shadows and
 *     reflections of the moved object on surfaces that did not move -- is biased as view-dependent radiance is, until new samples
 *     outweigh it (maxHistory);
 *   - prt_hip_render after the call renders the new geometry.
 * stream as in prt_hip_render: the update is ordered after the work queued on it.  The call then SYNCHRONISES the context's stream
 * once: the refitted root boxes come back to the host, which hands them to every later launch by value.  Memory: 12 bytes per triangle
 * slot and 12 bytes per internal node kept from the upload, plus 12 bytes per vertex (24 with normals) of every mesh ever updated. ---- */
typedef struct {
    uint32_t mesh;           /* index into prt_scene_desc.meshes of the uploaded scene */
    uint32_t vertexCount;    /* must equal the uploaded mesh's */
    const float* positions;  /* 3*vertexCount, host pointer (the library copies) */
    const float* normals;    /* 3*vertexCount, or NULL = keep the uploaded vertex normals; must be NULL for a mesh uploaded without */
    float radius;            /* Scene::getRadius() after the change (scene.cpp:23-26); 0 = keep the current one.  With several
                              * updates in one call the last non-zero one holds */
} prt_mesh_update;
int prt_hip_update_meshes(prt_hip_ctx* ctx, uint32_t count, const prt_mesh_update* updates, void* stream);

/* ---- geometry updates from device memory: prt_hip_update_meshes for callers that deform ON THE DEVICE (simulation, skinning, a
 * PyTorch kernel on the same card).  positions / normals are DEVICE pointers: the refit's gather kernel reads the caller's array where
 * it lies -- no staging copy in front of it -- ordered on `stream` after whatever the caller queued there (the kernel that wrote the
 * positions).  The caller's arrays may be reused when the call returns.  What the host path expects the caller to bring along, the
 * library computes (prt_deform.hip):
 *   - PRT_HIP_NORMALS_RECOMPUTE: Mesh::calculateVertexNormals (mesh.cpp:108-149) of the new positions, bit for bit, by two kernels.  One
 *     lane per face: fn = normalize(cross(p1 - p0, p2 - p0)), (0, 0, 0) when a component is NaN.  One lane per vertex walks the vertex's
 *     incidence list in the order the reference's sequential loop reaches that vertex's corners (faces descending, corners ascending
 *     within a face; a face that names the vertex twice appears twice): n = acc + fn; if (sqrtf(dot(n, n)) > 0) acc = n; the result
 *     is normalize(acc).  The sequential loop touches a vertex's accumulator at that vertex's own corners only, so the walk is the same
 *     arithmetic in the same order.  The incidence list (CSR) is built on the host at a mesh's first RECOMPUTE from the device's own
 *     leaf tables and kept with the scene (4 bytes per vertex + 36 bytes per triangle); PRT_HIP_EINVAL when the leaves of the uploaded
 *     tree do not name every triangle exactly once.
 *   - PRT_HIP_DEFORM_RADIUS_AUTO: the radius of Scene::add / Scene::updatePositions (scene.cpp:23-26): per mesh the box over ALL
 *     vertexCount positions (Mesh::calculateBounds: vertices no triangle uses count), merged over the meshes, center = 0.5f * (upper +
 *     lower), radius = length(upper - center) in f32.  The box of a deformed mesh is a min / max reduction over the new positions
 *     (exact and order independent up to the sign of a zero, which the radius cannot see); the box of a mesh never touched was taken
 *     from the descriptor at upload; a mesh last changed by prt_hip_update_meshes has its staged copy reduced when it is next needed.
 * The contract is prt_hip_update_meshes': afterwards the context is in exactly the state prt_hip_upload_scene produces from the same
 * topology with the new positions, normals and radius; the same things are invalidated; the call synchronises the context's stream
 * once (root boxes, vertex boxes).  Refusals (a refused call changes nothing): everything prt_hip_update_meshes refuses; an unknown
 * normalsMode or flag bit; GIVEN with NULL normals, KEEP / RECOMPUTE with non-NULL normals; GIVEN or RECOMPUTE for a mesh uploaded
 * without vertex normals; PRT_HIP_DEFORM_RADIUS_AUTO with a non-zero radius.  Without AUTO, radius is prt_mesh_update's.
 * Memory: 12 bytes per vertex (24 with normals) of every mesh ever updated, as for prt_hip_update_meshes: the library keeps its own
 * copy (written by the kernel that reduces the box) for prt_hip_get_mesh_vertices. ---- */
#define PRT_HIP_NORMALS_KEEP      0u  /* as normals == NULL in prt_hip_update_meshes */
#define PRT_HIP_NORMALS_GIVEN     1u  /* read `normals` */
#define PRT_HIP_NORMALS_RECOMPUTE 2u  /* Mesh::calculateVertexNormals (mesh.cpp:108-149) of the new positions, on the device */
#define PRT_HIP_DEFORM_HOST        1u /* positions / normals are HOST pointers (staged and copied as today); default: DEVICE pointers */
#define PRT_HIP_DEFORM_RADIUS_AUTO 2u /* radius = Scene radius of the updated scene, computed by the library; prt_mesh_deform.radius must be 0 */
typedef struct {
    uint32_t mesh, vertexCount;  /* as prt_mesh_update */
    const float* positions;      /* 3*vertexCount */
    const float* normals;        /* 3*vertexCount with PRT_HIP_NORMALS_GIVEN, else NULL */
    uint32_t normalsMode;        /* PRT_HIP_NORMALS_* */
    float radius;                /* as prt_mesh_update; 0 with PRT_HIP_DEFORM_RADIUS_AUTO */
} prt_mesh_deform;
int prt_hip_deform_meshes(prt_hip_ctx* ctx, uint32_t count, const prt_mesh_deform* deforms, uint32_t flags, void* stream);
/* The current positions and vertex normals of a mesh, from the copies the library keeps since the mesh's first update (either call);
 * either pointer may be NULL.  Targets are device pointers (the copies are queued, ordered with `stream`), or host pointers with
 * PRT_HIP_DEFORM_HOST (synchronous).  PRT_HIP_ESTATE for a mesh never updated, or whose normals never were ("no update yet: the caller
 * still holds what it uploaded").  With it a caller that deforms on the device brings a host Scene in step, or reads the recomputed normals. */
int prt_hip_get_mesh_vertices(prt_hip_ctx* ctx, uint32_t mesh, float* positions, float* normals, uint32_t flags, void* stream);
/* The tree readout: what a refit has cost in the builder's own terms.  area(box) = 2.0f * (ex*ey + ey*ez + ez*ex) in f32
 * (vecmath.cpp:75-79); internalArea = sum of area over the internal nodes, root included; leafArea = sum of primCount * area over the
 * leaves; both summed in f64 in a fixed order (one kernel over the mesh's node records: block tree, per-block partials, one final
 * block; the root's own box is added on the host), so a run repeats itself bit for bit.  sahCost = (0.125 * internalArea + leafArea) /
 * rootArea, 0.125 being the builder's traversal constant (bvh.cpp:111).  sahCostAtUpload is the same quantity of the tree as uploaded,
 * taken before the mesh's first update: sahCost / sahCostAtUpload is the number to watch, and to rebuild on.  vertexBox: lower, upper
 * of Mesh::calculateBounds; rootBox: the tree's; radius: the scene's.  Synchronous; changes nothing in the context. */
typedef struct {
    float vertexBox[6], rootBox[6], radius;
    double internalArea, leafArea, rootArea, sahCost, sahCostAtUpload;
    uint32_t internalNodes, leaves;
} prt_mesh_info;
int prt_hip_mesh_info(prt_hip_ctx* ctx, uint32_t mesh, prt_mesh_info* out);

/* ---- scene edits: the lights, single materials and the texels of single textures of the uploaded scene, replaced in place.  Everything
 * else that changes in a look-dev session -- the sun, the environment map, a material colour, a repainted texture -- without the
 * flattening and the copies of a whole prt_hip_upload_scene.  The contract of all three calls: after the call the context is in exactly
 * the state prt_hip_upload_scene produces from the uploaded descriptor with these fields replaced; every device array is the same
 * byte for byte.  Where the upload takes host-built environment tables, that is the state of the tables InfiniteAreaLight::create
 * builds (light.cpp:30-84).  stream as in prt_hip_update_meshes: the edit is ordered after the work queued on it; host pointers are
 * copied during the call, which SYNCHRONISES the context's stream once (an update of the directional fields alone does not).
 * Refusals: PRT_HIP_ESTATE without a scene, PRT_HIP_EINVAL with a message otherwise.  A refused call changes nothing.
 *
 * Lights.  The directional fields are always applied.  envMode:
 *     PRT_HIP_ENV_KEEP     leaves the environment light as it is, present or absent;
 *     PRT_HIP_ENV_NONE     removes it and releases its buffers;
 *     PRT_HIP_ENV_REPLACE  takes a new image of any size and builds the vertical table, the horizontal table and the first-step
 *                          constants of the bisection on the DEVICE (prt_edit.hip), from the texels alone, in the reference's arithmetic:
 *         l = sqrtf((r*r + g*g) + b*b);  hsum added in x order from 0.0f;  sinPhi = sin(kPi * (y + 0.5f) / height) (the kernels' own sine);
 *         vert[y] = hsum * sinPhi, vsum added in y order;  invH = 1.0f / hsum, ph = accumH + invH * l running in x order;
 *         invV = 1.0f / vsum, pv = accumV + invV * vert[y] running in y order
 *     all f32, no FMA, correctly rounded / and sqrtf.  The additions are SEQUENTIAL along a row and along the column: float addition is
 *     not associative, so neither a tree reduction nor a parallel scan is used for them; the parallelism is across rows, and within
 *     a row in the loads and the lengths.  The device refuses what the upload refuses in host-built tables -- a vertical table that is
 *     not non-decreasing, a partly NaN row, a row that is not non-decreasing (a NaN texel, a +inf texel and an all-black map end
 *     there) -- and accepts an all-NaN row (a black row), so the accepted maps are exactly the upload's; more than 2^28 texels and a NULL
 *     image are refused.  The tables are built into new buffers and swapped in once the flags are back, so a refused map leaves the old
 *     light in place.
 *
 * Materials.  The record of (mesh, material) is rewritten by the function that wrote it at upload.  Refused: count 0, an index out of
 * range, the same (mesh, material) twice in one call, an alphaTest other than the uploaded value, another diffuseMap for a
 * material uploaded with alphaTest (the alpha records and the leaf flags are per triangle and fixed at upload), a map index >=
 * textureCount, bumpMap >= 0 in a scene uploaded without any bump-mapped material (it has no bump records), reflectionType > 2.
 *
 * Textures.  The texels of texture `texture` are replaced; width, height and component must equal the uploaded ones.  The alpha cell
 * classes of a texture that an alpha-tested material names are rebuilt on the device by the upload's rule.  A texture may appear only
 * once per call.
 *
 * What the calls invalidate (the samples of the old radiance):
 *   - all three empty the accumulator and the moments and unbind the estimator, as prt_hip_accum_reset does;
 *   - all three drop the temporal history AND the pending record, as prt_hip_history_reset does: radiance changes everywhere the edit is
 *     seen, directly or indirectly, and the position and normal tests of the merge cannot see that.  A host that prefers the biased
 *     preview exports the history before the edit (prt_hip_history_export) and imports it afterwards;
 *   - prt_hip_update_lights leaves the denoise guides, the position plane and planes the host had set untouched: none depends on a light;
 *   - prt_hip_update_materials and prt_hip_update_textures treat them as prt_hip_update_meshes does: guides and position plane go stale
 *     and are rendered again on next use, planes a host had set are dropped;
 *   - prt_hip_render after any of the calls renders the edited scene. ---- */
#define PRT_HIP_ENV_KEEP 0     /* leave the environment light as it is (present or absent) */
#define PRT_HIP_ENV_NONE 1     /* remove it */
#define PRT_HIP_ENV_REPLACE 2  /* new image, any size; tables built on the device */
typedef struct {
    uint32_t hasDirectionalLight; /* as in prt_scene_desc; always applied */
    float lightDir[3];
    float lightIntensity[3];
    uint32_t envMode;             /* PRT_HIP_ENV_* */
    int32_t envWidth, envHeight;  /* PRT_HIP_ENV_REPLACE only */
    const float* envTexels;       /* host, 4*envWidth*envHeight floats, row 0 first; PRT_HIP_ENV_REPLACE only */
} prt_light_update;
int prt_hip_update_lights(prt_hip_ctx* ctx, const prt_light_update* update, void* stream);

typedef struct {
    uint32_t mesh, material; /* indices into prt_scene_desc.meshes and that mesh's materials */
    prt_material value;
} prt_material_update;
int prt_hip_update_materials(prt_hip_ctx* ctx, uint32_t count, const prt_material_update* updates, void* stream);

typedef struct {
    uint32_t texture;                 /* index into prt_scene_desc.textures of the uploaded scene */
    int32_t width, height, component; /* must equal the uploaded texture's */
    const uint8_t* texels;            /* host, width*height*component bytes (the library copies) */
} prt_texture_update;
int prt_hip_update_textures(prt_hip_ctx* ctx, uint32_t count, const prt_texture_update* updates, void* stream);

/* ---- display transform: 8-bit display-referred pixels and auto exposure on the device.  Every stage above ends in a camera-sized float
 * RGB image in device memory; a viewer shows bytes.  This stage turns such an image -- the context's framebuffer or a caller's -- into
 * RGB8 / RGBA8 / BGRA8 on the device, under a manual gain or under an exposure METERED from the image's own luminance histogram and
 * adapted over the frames.  It needs a camera (for the image size) and no scene, and it changes nothing else in the context: the
 * accumulator, the moments, the guides, the history and the statistics are untouched, it is not a render for prt_hip_get_stats and
 * takes no slot of the timing ring.  The only path to bytes without it is prt_hip_download (12 bytes per pixel) and the host loop of
 * Image::savePpm (image.cpp:52-80); with meter 0, gain 1.0f, transfer 0 and format 0 the bytes here ARE the pixel block
 * prt_host_save_ppm writes for the same floats.
 *
 * It is specified exactly, as the denoiser is: all arithmetic is f32, no FMA, correctly rounded /, subnormals kept, in the order
 * written (prt_amd/csrc/prt_display.h is that text for the device and for the host check).
 *     lum(c) = 0.2126f*c.x + 0.7152f*c.y + 0.0722f*c.z                                  (left to right)
 * Metering (meter 1), over the rectangle of the INPUT image:
 *     a pixel is counted iff lum > 0.0f (false for NaN, +-0 and negatives); every other pixel of the rectangle is `ignored`
 *     bin k = min(max((int32)(bits(lum) >> 20) - 888, 0), 255): 8 bins per octave from 2^-16, from the exponent and the top three
 *     mantissa bits -- a piecewise-linear log2 without a transcendental; +inf and everything from 1.875 * 2^15 falls in bin 255.
 *     The counts are integers: the histogram is exact whatever the order of the atomics.
 * Resolve, on the device:
 *     N = sum of hist; with N == 0 the whole state record stays as it is.  Otherwise, in u64:
 *     rlo = lowPermille*N/1000; rhi = (highPermille*N + 999)/1000
 *     bins upward with cum: bin k gives n = |[cum, cum + hist[k]) intersected with [rlo, rhi)| to Nb += n and S += n*(2k + 1)
 *     m = (float)S / (float)Nb                        (both conversions round to nearest even; Nb >= 1 follows from low < high)
 *     octaves = m*0.0625f - 16.0f
 *     i = floorf(octaves); f = octaves - i; two = the float with bits ((int32)i + 127) << 23; L = (1.0f + f) * two
 *     target = fminf(fmaxf(key / L, minGain), maxGain)
 *     gain = (valid && adaptRate < 1.0f) ? gain + (target - gain)*adaptRate : target;  valid = 1
 * Transform, of every pixel of the rectangle:
 *     g = meter ? params.gain * state.gain : params.gain      (once; with meter 1 read on the device after this call's resolve)
 *     per channel x = g * in;  tonemap 1: x = x / (x + 1.0f);  x = fminf(fmaxf(x, 0.0f), 1.0f)
 *         (NaN becomes 0, and +inf through the tone map -- inf / inf -- becomes 0 too: the reference's own behaviour)
 *     transfer 0: byte = (uint8_t)(powf(x, 1/2.2f) * 255.0f)
 *     transfer 1: s = x <= 0.0031308f ? 12.92f*x : 1.055f*powf(x, 1/2.4f) - 0.055f;  byte = (uint8_t)(s*255.0f + 0.5f)
 *     powf is glibc's algorithm (prt_devmath.h restates it; checked against libm over every float of [2^-24, 1] for both exponents).
 *
 * d_rgb: a device image of the camera's size (pixel (x,y) at (x + y*width)*3 floats), NULL = the context's framebuffer (PRT_HIP_ESTATE
 * when it holds no image of the camera's size).  d_out: a device buffer of width*height*bytesPerPixel, pixel (x,y) at
 * (x + y*width)*bpp, NULL = a display buffer the context owns, reallocated (and zeroed) when size or format make it grow.  Only the
 * bytes of the rectangle (inclusive) are written.  stream rules of prt_hip_accum_resolve; the call is asynchronous and never
 * synchronises the host, with meter 1 as well: the gain goes from the resolve to the transform through device memory.  Pointers that
 * are 16-byte aligned take the wide path (four pixels per thread); any 4-byte aligned d_rgb, and any d_out aligned to its format's
 * 1 or 4 bytes, is accepted.
 * Refusals: PRT_HIP_ESTATE without a camera; PRT_HIP_EINVAL with a message naming the field for every field out of range or not
 * finite (the meter's fields are only read with meter 1).  A refused call changes nothing.
 * The adaptation state survives prt_hip_set_camera, scene edits and uploads -- that is its purpose; only prt_hip_display_reset and
 * prt_hip_destroy end it. ---- */
typedef struct {
    uint32_t tonemap;   /* 0 none, 1 c/(c+1) per channel (Image::m_tonemap, image.cpp:64) */
    uint32_t transfer;  /* 0 the reference's: powf(c, 1/2.2f) * 255, truncated (image.cpp:65); 1 sRGB, rounded to nearest */
    uint32_t format;    /* 0 RGB8 (3 B/pixel: the body of the PPM), 1 RGBA8 (a = 255), 2 BGRA8 (a = 255) */
    uint32_t meter;     /* 0 manual gain only, 1 auto exposure */
    float gain;         /* finite, >= 0: manual multiplier; 1.0f with meter 0 gives savePpm's bytes */
    float key;          /* meter 1: finite, > 0: where the metered luminance lands (0.18) */
    uint32_t lowPermille, highPermille; /* meter 1: band of the lit pixels that is averaged, 0 <= low < high <= 1000 (500, 950) */
    float minGain, maxGain;             /* meter 1: finite, 0 < minGain <= maxGain */
    float adaptRate;    /* meter 1: in (0, 1]; 1 = jump to the target */
} prt_display_params;
typedef struct {
    float gain; uint32_t valid;     /* the adaptation state */
    float octaves, target;          /* of the last metering (0 before any) */
    uint64_t metered, ignored;      /* pixels of the last metering inside / outside the histogram */
    uint32_t hist[256];             /* its histogram */
} prt_display_state;
int prt_hip_display(prt_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const prt_display_params* params,
                    const float* d_rgb, uint8_t* d_out, void* stream);
/* Copies the rectangle (inclusive) of the context's display buffer into a host image of the camera's size in the format of the last
 * display into that buffer.  Synchronises; like prt_hip_download it reports a sticky launch error without clearing it. */
int prt_hip_download_display(prt_hip_ctx* ctx, uint8_t* out_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
/* The state record as it stands once the context's stream is idle (all zero before the first display).  Synchronous. */
int prt_hip_display_get_state(prt_hip_ctx* ctx, prt_display_state* state);
/* valid = 0, ordered behind the displays queued so far: the next metering jumps to its target. */
int prt_hip_display_reset(prt_hip_ctx* ctx);
/* The mirror of prt_hip_download: the rectangle (inclusive) of a host image of the camera's size goes into the context's framebuffer
 * (allocated and zeroed at the camera's size when there is none), behind the work queued on the context's stream.  Synchronous. */
int prt_hip_upload(prt_hip_ctx* ctx, const float* rgb_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);

/* ---- ray queries: nearest hit, any hit and surface records for batches of the caller's own rays.  Everything above answers "what
 * colour is this pixel"; these answer what else a ray tracer is asked: which mesh, triangle and material lies under the cursor, whether
 * two points see each other, what a probe or a lightmap texel sees, what a collision ray meets among the meshes prt_hip_update_meshes
 * moves.  The traversals are the frame kernel's own (prt_device.h trace_loop) behind a ray source that reads the caller's array; a
 * query reads the scene and changes nothing else: the accumulator, the moments, the guides, the history and the display state are
 * untouched.  It needs a scene and no camera (PRT_HIP_ESTATE without a scene).
 *
 * A ray is {org, tMax, dir}: 32 bytes, read as two 16-byte loads.  dir need not be normalised; t is in units of dir.  There is no
 * tMin: as in the reference, offsetting the origin is the caller's business.  pad is ignored.
 *
 * nearest: Scene::intersect<SingleRayHitPacket, SingleRayPacket> (scene.cpp:47-64) per ray with the ray's own tMax: the single-ray
 * nearest traversal of the G-buffer kernel, alpha tests included.  hits[r] is the reference's RayHitT: t, the barycentrics i, j, k,
 * primId = the triangle's index in its mesh, meshId = the mesh's index in the scene; a miss is {-1, 0, 0, 0, 0, 0}.
 * any: Scene::occluded<bool, SingleRayPacket> (scene.cpp:66-84): occluded[r] = 1 when any triangle is accepted below tMax, else 0.
 * A ray with a NaN in org, dir or tMax is answered as a miss / not occluded without a walk (under the reference's min / max such a ray
 * passes every box test and misses every triangle: the same answer after a walk of the whole tree).  The library never stores a NaN t.
 *
 * surfaces (nearest: may be NULL): the surface record of each ray's own hit, fetched by the same kernel:
 *     P = org + t*dir per component (the product is rounded, then the sum); t
 *     normal = Mesh::getSurfaceProperties' normal (mesh.cpp:311-364); material = the GLOBAL material index (the meshes' materials in order)
 *     shadingNormal = Material::sampleBump's normal (material.cpp:98-114); meshMaterial = the material's index within its mesh
 *     uv; primId, meshId as in the hit;  diffuse = Material::sampleDiffuse at uv (material.cpp:87-96)
 * A miss is the all-zero record with t = -1.
 * prt_hip_query_surface fetches the same records for hits the caller supplies (primId in mesh order, as nearest reports it), with
 * rays[r] giving org and dir of P.  Every index read from caller memory is range-checked on the device before it is used as an
 * address: meshId < the scene's mesh count, primId < that mesh's primitive count; the barycentrics are taken as they are.  A record
 * that fails the check, a record with t == -1 and a record with a NaN t all give the miss record, and nothing of the scene is read for
 * them; the records that failed the check are counted (prt_hip_query_get_counts, synchronous: those of the last query_surface).  The
 * call needs the inverse of the upload's triangle order, one word per triangle slot, built on the device by its first use after
 * prt_hip_upload_scene and kept until the next upload (prt_hip_update_meshes and the scene edits keep the topology, hence the table).
 *
 * n: 1 .. 2^30 rays, any count (PRT_HIP_EINVAL otherwise).  Pointers: DEVICE pointers by default; rays and surfaces must be 16-byte
 * aligned, hits 4-byte aligned, occluded any; anything else is refused with PRT_HIP_EINVAL and a message before anything is launched.
 * stream as in prt_hip_render: the query is ordered after the work queued on it and before what is queued next; asynchronous.  With
 * PRT_HIP_QUERY_HOST in flags all array pointers are HOST pointers: the arrays are staged in the one arena the context owns for the
 * host arrays of all its calls (grown to the largest call, freed with the context) and the call returns when the answers are in host
 * memory.  Other flag bits are refused.
 * For prt_hip_get_stats nearest and any are launches like the position pass, timed as a render: kernelMs, raysTraced = n
 * (occludedTraced = n too for any), and a stack overflow is reported there.  query_surface is not a launch for the statistics.
 * One persistent launch per call, a few workgroups per compute unit whatever n is. ---- */
typedef struct { float org[3]; float tMax; float dir[3]; uint32_t pad; } prt_ray;      /* 32 bytes, 16-byte aligned */
typedef struct { float P[3]; float t;                /* org + t*dir per component (product rounded, then the sum); t = -1: miss */
                 float normal[3]; uint32_t material; /* Mesh::getSurfaceProperties' normal; GLOBAL material index (meshes in order) */
                 float shadingNormal[3]; uint32_t meshMaterial; /* Material::sampleBump's normal; index within the mesh */
                 float uv[2]; uint32_t primId, meshId;
                 float diffuse[3]; uint32_t pad; } prt_surface;                        /* 80 bytes */
#define PRT_HIP_QUERY_HOST 1u  /* all array pointers are HOST pointers: staged in the context's arena, the call is synchronous */

int prt_hip_query_nearest(prt_hip_ctx* ctx, uint32_t n, const prt_ray* rays, prt_hit* hits, prt_surface* surfaces /* may be NULL */,
                          uint32_t flags, void* stream);
int prt_hip_query_any(prt_hip_ctx* ctx, uint32_t n, const prt_ray* rays, uint8_t* occluded, uint32_t flags, void* stream);
int prt_hip_query_surface(prt_hip_ctx* ctx, uint32_t n, const prt_ray* rays, const prt_hit* hits, prt_surface* surfaces,
                          uint32_t flags, void* stream);
int prt_hip_query_get_counts(prt_hip_ctx* ctx, uint64_t* invalidHits); /* synchronous: records of the last prt_hip_query_surface refused on the device */

/* radiance: what a baker asks instead of a hit record -- the path-traced radiance arriving along each ray (emission, sun and sky
 * light, every bounce): light probes and irradiance volumes, lightmap texels, reflection cube maps and panoramas, any camera model
 * the reference lacks.  The frame kernel itself (prt_frame.h) with a ray source that is the caller's array instead of the context's
 * camera, and an output that is the caller's array instead of a camera-sized image.
 *
 * Definition.  Probe q (0-based) is, bit for bit, pixel (0, 0) of prt_hip_render under the camera
 *     pos = rays[q].org,  dir = rays[q].dir (as given: the caller does not normalise it),  up = right = (0, 0, 0),
 *     width = height = 1,  invWidth = invHeight = 1
 * with params whose seed is seed + q (uint32 wrap).  So: the generator starts at lowbias32(q + seed) | 1; the eight primary rays of
 * every packet are the same ray, run through camera.cpp:46-56 (both jitter terms are multiplied by the zero vectors), avgDir is their
 * lane-ordered sum over 8, and each packet consumes 16 draws; the primary traversal (limit 100000, camera.cpp:64), the bounce loop,
 * Russian roulette, the shadow-ray skip, the environment light and the defined refraction are the frame kernel's own;
 *     radiance[3q .. 3q+2] = exposure * colour / samples.
 * rays[q].tMax and pad are ignored.  A direction whose squared length overflows or underflows in float -- zero, 1e-30 or 3e20 long,
 * or with an inf or NaN component -- normalises to zero or to non-finite components, and the probe returns what the reference returns
 * for such a camera ray -- black (+0) -- and counts what the reference counts for it, its `samples` primary rays and no others; it is
 * not refused and it does not disturb its neighbours.  A NaN in org is answered the same way.
 *
 * params: samples a multiple of 8 from 8 to 2040; maxDepth (<= 255), rrDepth, exposure as in prt_hip_render; rank must be 0 and
 * nranks 1 (probes are not split over ranks); countTraffic must be 0 (the probe kernel has no counting build); tileSize is ignored.
 * n: 1 .. 2^24 probes.  Anything else is PRT_HIP_EINVAL with a message, refused before anything is launched, radiance untouched.
 * Pointers, flags and stream as for the other queries: DEVICE pointers by default, rays 16-byte aligned and radiance 4-byte aligned;
 * with PRT_HIP_QUERY_HOST both are HOST pointers staged in the context's arena and the call is synchronous; other flag bits
 * are refused; the query is ordered after the work queued on stream and before what is queued next.
 * State: needs a scene and NO camera (PRT_HIP_ESTATE without a scene).  It reads the scene and changes nothing else: the camera, the
 * accumulator, the moments, the guides, the position plane, the history, the display state and the framebuffer are untouched, and so
 * is what the last render left for the gathers.  For prt_hip_get_stats it is a render launch: kernelMs, raysTraced, occludedTraced,
 * nPx = n, stackOverflow.  One persistent launch whatever n is.
 * Not built: probes do not accumulate over calls (a caller averages equal-sample calls with different seeds itself), the eight lanes
 * of a packet cannot carry distinct rays, and a batch is not split over ranks. */
int prt_hip_query_radiance(prt_hip_ctx* ctx, uint32_t n, const prt_ray* rays, const prt_render_params* params,
                           float* radiance /* 3*n floats */, uint32_t flags, void* stream);

/* ---- baking: points and direction sets in, weighted radiance sums out.  What every baker writes around prt_hip_query_radiance -- a
 * tangent frame per probe or texel, K local directions rotated into it, the origin tiled K times, n*K rays up and n*K radiances
 * down, a weighted mean -- as one call that takes 32 bytes per point and returns C*12 bytes per point: light probes, irradiance
 * volumes, lightmap texels.  The rays and the per-ray radiances never leave the device.
 *
 * A point is {P, bias, N, set}; the table holds nSets direction sets of K local directions (z along the normal) and, per direction,
 * C weights.  One set with C = 1, cosine-weighted directions and weights pi/K gives irradiance; directions on the sphere with C = 9
 * and weights 4pi/K * Y_c(d_k) give an SH9 probe (such points have N = 0: the frame is the identity); several sets, each point naming
 * its own, break up the pattern one shared set leaves across neighbouring texels.
 *
 * Definition.  Everything is f32, every product is rounded before the sum that uses it (no FMA).
 * Ray r = i*K + k of point i, with s = points[i].set and d = dirs[(s*K + k)*3 ..]:
 *     if all three components of N compare equal to 0:  org = P, dir = d
 *     otherwise the frame is the bounce loop's own (path_tracer.cpp:147-153):
 *         u = fabsf(N.x) > 0.1f ? (0,1,0) : (1,0,0)
 *         T = normalize3(cross3(N, u))
 *         B = normalize3(cross3(T, N))
 *         dir = (d.x*B + d.y*T) + d.z*N per component, with N as given and not normalised
 *         org = P + bias*N per component
 *     with cross3(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x) and normalize3(v) = (1.0f / sqrtf(v.x*v.x + v.y*v.y
 *     + v.z*v.z)) * v per component (vecmath.h:1200)
 *     tMax = 0, pad = 0
 * Hostile N (NaN, inf, 1e-30, 3e20) is not refused: the arithmetic gives what it gives, and the probe rule of prt_hip_query_radiance
 * makes a non-finite or unnormalisable direction black.  (Which NaN an invalid operation gives, its sign and payload, is the
 * processor's choice.)
 * set >= nSets is never followed: the point's K rays get org = dir = 0.
 * Radiance L[r] is prt_hip_query_radiance of those n*K rays under params: probe r under seed + r, with all of that call's rules.
 * Reduce, one wavefront per point, in an order fixed by K alone:
 *     1. for lane l = 0..63, for channel c and colour component h: a_l = +0
 *     2. for k = l, l+64, l+128, ... < K: a_l = a_l + (weights[(s*K + k)*C + c] * L[3r + h])
 *     3. for step = 32, 16, 8, 4, 2, 1, for l < step: a_l = a_l + a_(l+step)
 *     4. out[(i*C + c)*3 + h] = a_0
 * A point with set >= nSets writes +0 to all its 3*C floats.  Weights and radiance are taken as given: a NaN weight gives a NaN
 * output for that point and for no other.
 *
 * prt_hip_bake runs the ray kernel, the frame kernel's probe launch and the reduce kernel in order on the context's stream; the rays
 * and radiances live in buffers the context owns, grown on demand.  It is one persistent frame-kernel launch: prt_hip_get_stats
 * reports it as prt_hip_query_radiance of n*K probes would (nPx = n*K).  prt_hip_bake_rays and prt_hip_bake_reduce are the two
 * halves on the caller's arrays: bake_rays needs no scene, and bake_reduce lets a baker who kept the per-ray radiance project it
 * again under other weights without tracing again; neither is a launch for the statistics.  bake_rays reads no weights and
 * bake_reduce no directions: that pointer of the table may be NULL there.
 * Pointers: DEVICE pointers by default, sets->dirs and sets->weights included (the prt_bake_sets record itself is host memory, read
 * before the call returns); points and rays 16-byte aligned, floats 4-byte aligned; asynchronous, ordered after the work queued on
 * stream and before what is queued next, as the queries are.  With PRT_HIP_QUERY_HOST every array is HOST memory, staged in
 * the context's arena, and the call returns with the answer.  Other flag bits are refused.
 * Refused with PRT_HIP_EINVAL and a message, before anything is queued and with the outputs untouched: a NULL pointer; K outside
 * 1 .. 4096, C outside 1 .. 16, nSets outside 1 .. 1024; reserved != 0; n = 0 or n*K > 2^24; for prt_hip_bake whatever
 * prt_hip_query_radiance refuses of params.  prt_hip_bake without a scene is PRT_HIP_ESTATE.
 * State: prt_hip_bake reads the scene and changes nothing else: the camera, the accumulator, the moments, the guides, the history,
 * the display state and the framebuffer are untouched, and so is the staging arena of the host-array calls.
 * Not built: batches beyond 2^24 rays (the caller splits by points and passes seed + i0*K for the part that starts at point i0);
 * per-point validity or back-face counts; splitting over ranks. ---- */
typedef struct { float P[3]; float bias; float N[3]; uint32_t set; } prt_bake_point;   /* 32 bytes, 16-byte aligned */
typedef struct {
    uint32_t K;           /* directions per point, 1 .. 4096 */
    uint32_t C;           /* output channels per point, 1 .. 16 */
    uint32_t nSets;       /* direction sets, 1 .. 1024 */
    uint32_t reserved;    /* must be 0 */
    const float* dirs;    /* nSets*K*3: local directions (x, y, z), z along the normal */
    const float* weights; /* nSets*K*C: weights[(set*K + k)*C + c] */
} prt_bake_sets;
int prt_hip_bake_rays(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, prt_ray* rays /* n*K */,
                      uint32_t flags, void* stream);
int prt_hip_bake_reduce(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets,
                        const float* radiance /* 3*n*K */, float* out /* 3*C*n */, uint32_t flags, void* stream);
int prt_hip_bake(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets, const prt_render_params* params,
                 float* out /* 3*C*n */, uint32_t flags, void* stream);

/* ---- lightmap atlases: per-corner lightmap UVs in, a lightmap image out.  prt_hip_bake takes the world position and normal of every
 * lightmap texel; producing that array means rasterising the meshes in their lightmap UV space, and after the bake the n answers have
 * to go back into a W x H image whose chart borders are dilated, or bilinear taps bleed black into the charts.  Three calls around
 * prt_hip_bake, which is used as it stands:
 *     prt_hip_atlas_rasterize   UV triangles -> the covered texels and, per texel, a hit record of the triangle that owns it
 *     prt_hip_atlas_points      hit records -> bake points on the scene as it is now
 *     prt_hip_atlas_resolve     per-point values -> an image with a filled gutter
 * The UVs are the caller's LIGHTMAP channel, given per corner (texture UVs tile and overlap): 6 floats per triangle, (u, v) of corners
 * 0, 1, 2, triangles in mesh order.  u runs along x over W texels and v along y over H; texel (x, y) has the index y*W + x and its
 * centre at u = (x + 0.5) / W, v = (y + 0.5) / H.
 *
 * prt_hip_atlas_rasterize.  Integer arithmetic throughout, so it is watertight along shared edges and independent of the order in
 * which triangles are processed.  It needs no scene.
 *   Snap.  Corner (u, v) snaps to a 1/256-texel grid: fx = u * (float)(256*W) (one f32 product), X = rint(fx) (ties to even); Y the
 *     same with H.  A triangle with a corner where !(fabsf(fx) <= 8388608.0f) in either coordinate is not rasterised and counts in
 *     `rejected`: NaN, infinity and far-off UVs.
 *   Edge functions, in int64: E(a,b,c) = (b.x-a.x)*(c.y-a.y) - (b.y-a.y)*(c.x-a.x).  A = E(v0,v1,v2); a triangle with A == 0 counts in
 *     `degenerate` and covers nothing.  For texel (x, y) with c = (256x+128, 256y+128): w0 = E(v1,v2,c), w1 = E(v2,v0,c),
 *     w2 = E(v0,v1,c).  If A < 0, negate all four.
 *   Coverage.  The triangle covers the texel iff w0 >= 0 && w1 >= 0 && w2 >= 0: the edges are closed, and w0+w1+w2 == A exactly.
 *     Every (triangle, texel) pair that passes counts in `pairs`.
 *   Ownership.  A covered texel belongs to the smallest key (meshId << 28) | primId among its covering triangles.
 *   Outputs.  n = the number of owned texels; texels[0..n) are their indices y*W + x in ascending order;
 *     hits[q] = {t = 0, i = (float)w0/(float)A, j = (float)w1/(float)A, k = (float)w2/(float)A, primId, meshId} of the owner of
 *     texels[q], the int64 to f32 conversions rounding to nearest even and the divisions correctly rounded.  Entries at and beyond n
 *     are untouched.
 *   W, H: 1 .. 8192.  count: 1 .. PRT_HIP_MAX_BVH records; meshId below PRT_HIP_MAX_BVH, each at most once; primCount 1 .. 2^28.
 *   The prt_atlas_mesh records are host memory, read before the call returns; their uv pointers follow the flags.  counts is HOST
 *   memory and the call returns when it is filled: the one synchronous step (a bake needs n on the host anyway).  texels and hits have
 *   a capacity of W*H entries.
 *
 * prt_hip_atlas_points.  Needs a scene (PRT_HIP_ESTATE without one).  Record q is a hit (primId in mesh order, as the rasteriser and
 * prt_hip_query_nearest report it) and the texel it is for.  Every index read from caller memory is range-checked on the device as
 * prt_hip_query_surface checks it: meshId < the scene's mesh count, primId < that mesh's primitive count.
 *   A valid record gives the point
 *     P = (i*p0 + j*p1) + k*p2 per component, p0 p1 p2 the triangle's corners as the scene holds them now, every product rounded
 *         before the sums
 *     N = the normal of prt_hip_query_surface for that hit: the normalised interpolation of the vertex normals, or the face normal
 *         of a mesh without them
 *     bias as given
 *     set = (x % setTile) + setTile * (y % setTile) with x = texel % W, y = texel / W; setTile 1 .. 32.  A set at or above the
 *         table's nSets is the caller's business: prt_hip_bake never follows it.
 *   An invalid record gives the all-zero point with set = 0xffffffff, which prt_hip_bake answers with +0; nothing of the scene is
 *   read for it.  t of a hit is ignored.
 *   The call reads the scene as it is at that moment: after prt_hip_update_meshes, prt_hip_deform_meshes or an edit the same hits
 *   give the moved surface's points without rasterising again, which is why the atlas stores barycentrics and not positions.
 *   n: 1 .. 2^26 records; W: 1 .. 8192; reserved must be 0.
 *
 * prt_hip_atlas_resolve.  Needs no scene.
 *   Every texel starts at +0 with mask 0.  texels[q] < W*H gets values[q*stride ..] and mask 1; an index at or beyond W*H is ignored;
 *   with duplicate indices, which the rasteriser never produces, it is unspecified which value is stored.
 *   Pass g = 1 .. gutter: a texel with mask 0 that has at least one 8-neighbour inside the image with mask in 1 .. g takes, per float,
 *   the sum over those neighbours in the order dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, starting from +0, divided by (float)count;
 *   its mask becomes g + 1.  Texels filled in pass g are not read in pass g.  NaN values travel as given.
 *   stride: 1 .. 48 floats per texel (3*C of the bake); gutter: 0 .. 64; n: 1 .. 2^26; mask may be NULL.
 *
 * Pointers, flags and stream as for the queries and the baker: DEVICE pointers by default (points 16-byte aligned, everything else
 * 4-byte aligned, mask any), ordered after the work queued on stream and before what is queued next; points and resolve are
 * asynchronous.  With PRT_HIP_QUERY_HOST every array is HOST memory, staged in the context's arena, and the call returns
 * with the answer.  Other flag bits are refused.  Refused with PRT_HIP_EINVAL and a message, before anything is queued and with the
 * outputs untouched: a NULL pointer, a parameter outside its range, reserved != 0, a misaligned device pointer.
 * State: the calls read the scene (points only) and change nothing else in the context; none is a launch for prt_hip_get_stats.
 * Not built: unwrapping or packing charts; conservative rasterisation; supersampled texels; seam stitching; atlases over ranks; a
 * count of invalid records in atlas_points. ---- */
typedef struct { uint32_t meshId; uint32_t primCount; const float* uv; /* 6*primCount: (u,v) of corners 0,1,2, mesh order */ } prt_atlas_mesh;
typedef struct { uint32_t n; uint32_t rejected; uint32_t degenerate; uint32_t reserved; uint64_t pairs; } prt_atlas_counts;
typedef struct { float bias; uint32_t setTile; uint32_t reserved[2]; } prt_atlas_point_params;
int prt_hip_atlas_rasterize(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t count, const prt_atlas_mesh* meshes,
                            uint32_t* texels /* capacity W*H */, prt_hit* hits /* capacity W*H */,
                            prt_atlas_counts* counts /* HOST */, uint32_t flags, void* stream);
int prt_hip_atlas_points(prt_hip_ctx* ctx, uint32_t n, uint32_t W, const uint32_t* texels, const prt_hit* hits,
                         const prt_atlas_point_params* params, prt_bake_point* points, uint32_t flags, void* stream);
int prt_hip_atlas_resolve(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels,
                          const float* values /* n*stride */, uint32_t stride /* 1 .. 48: 3*C of the bake */, uint32_t gutter /* 0 .. 64 */,
                          float* image /* W*H*stride */, uint8_t* mask /* W*H, may be NULL */, uint32_t flags, void* stream);

/* ---- lens renders: a camera record in, an image of radiance sums out.  What a caller writes around prt_hip_query_radiance for any
 * camera the reference lacks -- a ray per pixel and sample built on the host, 32 bytes per ray up and 12 down, a sum, and a splitter for
 * every image beyond the 2^24 probes of one launch -- as one call that builds the rays on the device, traces them band by band and
 * adds the K radiances of every pixel into an image that can accumulate over calls: a perspective camera with a thin lens (depth of
 * field), an orthographic view, a 360 x 180 degree panorama and an equidistant fisheye.  A cube map is six PINHOLE calls with a 90
 * degree basis (|right| = |up| = |fwd|, width = height); it needs no model of its own.  The rays and the per-ray radiances never
 * leave the device.
 *
 * Definition.  Everything is f32, every product is rounded before the sum that uses it (no FMA), sums go left to right as written.
 * W = width, H = height.  Ray r = ((y - y0)*W + x)*K + k of pixel (x, y), k = 0 .. K-1, in the band of rows [y0, y1):
 *   Draws.  mix(v) is the five steps of the frame kernel's pixel seed without its final | 1:
 *         v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16
 *     pix = y*W + x, j = pass*K + k (uint32 wrap), s = mix(mix(pix + jitterSeed) + j) | 1; then four times in turn
 *         s = xorshift32(s) (s ^= s << 13; s ^= s >> 17; s ^= s << 5),  u_i = bits((s & 0x007fffff) | 0x3f800000) - 1.0f,  i = 0 .. 3
 *     All four draws are always made: the stream does not depend on the model, and pass p with K rays is rays p*K .. p*K + K-1 of the
 *     pixel's stream, whatever K is.
 *   Film.  jx = CENTRE ? 0.5f : u0, jy = CENTRE ? 0.5f : u1; invW = 1.0f / (float)W, invH = 1.0f / (float)H;
 *         sx = ((float)x + jx) * invW,  sy = ((float)y + jy) * invH,  a = 2.0f*sx - 1.0f,  b = 1.0f - 2.0f*sy
 *     so a runs from -1 at the left edge to +1 at the right, b from +1 at the top edge to -1 at the bottom, and the centre of pixel
 *     (x, y) sits at ((x + 0.5) / W, (y + 0.5) / H), as a texel's does in the atlas.  This is HALF A PIXEL off the footprint of
 *     prt_hip_render, which centres pixel x at x / W (camera.cpp:54-55): a PINHOLE record that frames what a prt_camera_desc frames
 *     has right' = 0.6*aspect*right, up' = 0.6*up and fwd' = dir - right'/W + up'/H.
 *   PINHOLE.  d = (fwd + a*right) + b*up per component.
 *     if !(lensRadius > 0):  org = pos, dir = d
 *     otherwise (a thin lens):
 *         rl = lensRadius * sqrtf(u2);  (sn, cs) = sincosf(6.28318530717958647692f * u3)
 *         R = normalize3(right), U = normalize3(up)   (the normalize3 of the baking section)
 *         org = (pos + (rl*cs)*R) + (rl*sn)*U;  F = pos + focus*d;  dir = F - org
 *     d is not normalised, so the plane in focus lies at focus * |fwd| along fwd for every pixel.
 *   ORTHO.  org = (pos + a*right) + b*up, dir = fwd.
 *   EQUIRECT.  (sp, cp) = sincosf(a * 3.14159265358979323846f), (st, ct) = sincosf(b * 1.57079632679489661923f),
 *         l = (ct*sp, st, ct*cp);  dir = (l.x*right + l.y*up) + l.z*fwd;  org = pos
 *   FISHEYE.  rr = sqrtf(a*a + b*b).  if !(rr <= 1.0f): org = pos, dir = 0 (outside the image circle: the probe rule of
 *     prt_hip_query_radiance answers such a ray black and counts its `samples` primary rays).  Otherwise
 *         (st, ct) = sincosf(rr * (0.5f*fov)),  q = rr > 0.0f ? st / rr : 0.0f,  l = (a*q, b*q, ct),  dir and org as for EQUIRECT
 *   All models: tMax = 0, pad = 0.  sincosf is glibc's sinf and cosf of the same argument, as the kernels restate them.  Nothing about
 *   the basis is checked or normalised beyond what is written: hostile pos, fwd, right, up, fov, lensRadius and focus (NaN, inf, 0,
 *   1e-30, 3e20, negative) give what the arithmetic gives, and the probe rule handles the rest.  (Which NaN an invalid operation
 *   gives, its sign and payload, is the processor's choice.)
 * Probe seeds.  The ray with the global index g = (y*W + x)*K + k is probe g under the seed params->seed + pass*(W*H*K) + g (uint32
 *   wrap, the product included): the band [y0, y1) is prt_hip_query_radiance of prt_hip_lens_rays(y0, y1) under
 *   seed + pass*W*H*K + y0*W*K, and the image does not depend on how it is cut into bands.
 * Accumulate.  For pixel pix of the band, whose first ray in the band is r0, and colour component h: S = +0, then for k = 0 .. K-1 in
 *   that order S = S + L[3*(r0 + k) + h];  image[3*pix + h] = ACCUMULATE ? image[3*pix + h] + S : S.  Rows outside the band are not
 *   touched; NaN and infinities travel as given.  The result is a SUM: the mean is sum / (passes*K), taken by the caller or by the
 *   manual gain of prt_hip_display.
 *
 * prt_hip_lens_render runs, for each band of rows in ascending y, on the context's stream: the rays kernel, the frame kernel's probe
 * launch with the band's seed, the accumulate kernel.  A band holds as many rows as fit the 2^24 probes of one launch, or bandRows
 * if that is fewer: bandRows caps the scratch (44 bytes per ray, in buffers the context owns and grows on demand).  For
 * prt_hip_get_stats every band is a render launch: kernelMsSum and kernelLaunches cover them all, the event counters (raysTraced,
 * nPx ...) are the last band's.  prt_hip_lens_rays and prt_hip_lens_accumulate are the two halves on the caller's arrays; they
 * need no scene and neither is a launch for the statistics.
 * Pointers: DEVICE pointers by default (the prt_lens_desc record itself is host memory, read before the call returns); rays 16-byte
 * aligned, floats 4-byte aligned; asynchronous, ordered after the work queued on stream and before what is queued next, as the
 * queries are.  With PRT_HIP_QUERY_HOST every array is HOST memory, staged in the context's arena (the image in both directions
 * under ACCUMULATE), and the call returns with the answer.  Other flag bits are refused.
 * Refused with PRT_HIP_EINVAL and a message, before anything is queued and with the outputs untouched: a NULL pointer; an unknown
 * model; width or height outside 1 .. 8192, K outside 1 .. 64, bandRows above height; unknown bits in lens->flags; reserved != 0;
 * for the two halves y0 >= y1, y1 > height or (y1 - y0)*W*K > 2^24; for prt_hip_lens_render whatever prt_hip_query_radiance
 * refuses of params.  prt_hip_lens_render without a scene is PRT_HIP_ESTATE.
 * State: the calls read the scene (the render only) and change nothing else in the context: the camera, the accumulator, the
 * moments, the guides, the history, the display state and the framebuffer are untouched.
 * Not built: filters other than the box; motion blur; splitting over ranks; a G-buffer or denoiser guides for lens images; distinct
 * rays in the eight lanes of a packet, so `samples` per ray stays at least 8. ---- */
#define PRT_HIP_LENS_PINHOLE  0u  /* perspective; a thin lens when lensRadius > 0 */
#define PRT_HIP_LENS_ORTHO    1u
#define PRT_HIP_LENS_EQUIRECT 2u  /* 360 x 180 degree panorama */
#define PRT_HIP_LENS_FISHEYE  3u  /* equidistant, full angle `fov` in radians across the image circle */
#define PRT_HIP_LENS_CENTRE     1u /* lens->flags: jx = jy = 0.5 (no pixel jitter; the draws are still made) */
#define PRT_HIP_LENS_ACCUMULATE 2u /* lens->flags: add to `image` instead of overwriting it */
typedef struct {
    uint32_t model, width, height;   /* width, height 1 .. 8192 */
    uint32_t K;                      /* rays per pixel and pass, 1 .. 64 */
    uint32_t pass;                   /* which K rays of the pixel's jitter stream, and the probe seeds' offset */
    uint32_t jitterSeed;
    uint32_t flags;                  /* PRT_HIP_LENS_CENTRE | PRT_HIP_LENS_ACCUMULATE, other bits refused */
    uint32_t bandRows;               /* 0: as many rows per frame-kernel launch as fit 2^24 probes; else 1 .. height, capped by that */
    float pos[3];   float lensRadius;
    float fwd[3];   float focus;
    float right[3]; float fov;
    float up[3];    uint32_t reserved; /* 0 */
} prt_lens_desc;                     /* 96 bytes, host memory, read before the call returns */
int prt_hip_lens_rays(prt_hip_ctx* ctx, const prt_lens_desc* lens, uint32_t y0, uint32_t y1 /* rows [y0, y1) */,
                      prt_ray* rays /* (y1-y0)*W*K */, uint32_t flags, void* stream);
int prt_hip_lens_accumulate(prt_hip_ctx* ctx, const prt_lens_desc* lens, uint32_t y0, uint32_t y1,
                            const float* radiance /* 3*(y1-y0)*W*K */, float* image /* 3*W*H, the WHOLE image */, uint32_t flags,
                            void* stream);
int prt_hip_lens_render(prt_hip_ctx* ctx, const prt_lens_desc* lens, const prt_render_params* params, float* image /* 3*W*H */,
                        uint32_t flags, void* stream);

/* ---- lightmap filter: an edge-avoiding a-trous filter over the baked values of an atlas, in atlas space.  A lightmap at a few
 * hundred paths per texel is noisy, and it cannot go through the camera denoiser: its texels are no camera pixels, and neighbouring
 * texels of different charts lie on unrelated surfaces.  Every texel carries exact guides, though: the world position and normal of
 * its prt_bake_point.  prt_hip_atlas_filter sits between prt_hip_bake and prt_hip_atlas_resolve, neither of which changes: the n
 * values of the bake in, n filtered values out, the points and their texel indices as guides.
 *
 * Definition.  All arithmetic is f32 with no FMA, every product is rounded before the sum that uses it, sums go left to right as
 * written, divisions and sqrtf are correctly rounded and subnormals are kept: the rules of the denoised previews.
 *   f(x):  y = 0.125f*x; r = 1.0f/((1.0f + y) + (0.5f*y)*y), then r = r*r three times (the previews' f).
 *   lum(v) = (0.2126f*v[0] + 0.7152f*v[1]) + 0.0722f*v[2] of the FIRST three floats of a point's values (the previews' lum).
 *   Texel t is (x, y) = (t % W, t / W).
 *   Eligibility.  Point q is eligible iff texels[q] < W*H, points[q].set != 0xffffffff, the six floats of P and N are finite and
 *     all `stride` floats of values[q] are finite.  map[t] is the smallest eligible q with texels[q] == t, or none.  Point q is
 *     PLACED iff it is eligible and map[texels[q]] == q.  For a point that is not placed, out gets the bytes of values as they are,
 *     and such a point is never a tap: a NaN texel is contained instead of spreading over +-62 texels in five iterations, and
 *     duplicate indices are deterministic.  Everything below is for a placed q, and every r is placed.
 *   nb(q, dx, dy) = map[(y+dy)*W + (x+dx)] if that texel is inside the image, else none.
 *   Distance.  d2(q,r) = (ex*ex + ey*ey) + ez*ez with e = P_r - P_q.
 *   Footprint.  f2_q = +inf; for (dx,dy) = (-1,0), (1,0), (0,-1), (0,1) in that order: if r = nb(q,dx,dy) exists, d2 > 0 and
 *     d2 < f2_q, then f2_q = d2.  If nothing was taken, f2_q = 0.  It is the squared world size of a texel measured inside the
 *     point's own chart, so sigmaPosition is in texel footprints and does not depend on the scene's scale.
 *   Geometric weight for step s.  dn = (Nq.x*Nr.x + Nq.y*Nr.y) + Nq.z*Nr.z;  wn = dn > 0 ? dn : 0, then wn = wn*wn repeated
 *     normalPowerLog2 times;  invP = 1.0f / ((sigP2 * (float)(s*s)) * f2_q) with sigP2 = sigmaPosition*sigmaPosition computed once
 *     on the host (invP is per point and per launch, not per tap);  wp = d2 == 0 ? 1.0f : f(d2 * invP);  geo = wn * wp.
 *   Variance V0_q.  Taps dy = -2..2 outer, dx = -2..2 inner at stride 1, r = nb(q,dx,dy); missing taps are skipped.  g = 1 for the
 *     centre, else geo(q,r,1).  First loop: sw = sw + g, sl = sl + g*lum_r, both from +0;  m1 = sl/sw.  Second loop in the same
 *     order: d = lum_r - m1; sv = sv + g*(d*d), from +0;  V0 = sv/sw.
 *   Iteration i = 0 .. iterations-1 (s = 1 << i) on (C, V), starting from (values, V0):
 *     a/b is the 3 x 3 stride-1 average of V over existing neighbours, weights (dx==0 ? 0.5f : 0.25f)*(dy==0 ? 0.5f : 0.25f),
 *       row-major: a = a + wt*V_r, b = b + wt, both from +0, exactly as in the previews' iteration.
 *     invDen = 1.0f / (sigmaLuminance*sqrtf(a/b) + 1e-6f).
 *     Taps dy = -2..2 outer, dx = -2..2 inner at stride s, r = nb(q, dx*s, dy*s); missing taps are skipped.  With h = 0.375, 0.25,
 *       0.0625 for |d| = 0, 1, 2: the centre has w = 0.375f*0.375f, other taps have
 *       w = ((hy*hx)*geo(q,r,s)) * f(fabsf(lum(C_q) - lum(C_r)) * invDen).
 *     sumW = sumW + w;  per float j: S_j = S_j + w*C_r[j];  sumV = sumV + (w*w)*V_r;  all from +0.
 *     C'_q[j] = S_j/sumW,  V'_q = sumV/(sumW*sumW).
 *   out = C after the last iteration.  The weights come from channel 0 (the first three floats) and apply to every channel.
 *   IEEE fixes every finite word; which NaN an invalid operation gives is the processor's choice.
 *
 * W, H: 1 .. 8192.  n: 1 .. 2^26.  stride: 3*C floats per point, C 1 .. 16.  iterations 1 .. 5, normalPowerLog2 0 .. 7,
 * sigmaLuminance and sigmaPosition finite and > 0, reserved 0.
 * Pointers, flags and stream as for the three atlas calls: DEVICE pointers by default (points 16-byte aligned, everything else
 * 4-byte aligned), asynchronous, ordered after the work queued on stream and before what is queued next; with PRT_HIP_QUERY_HOST
 * every array is HOST memory, staged in the context's arena, and the call returns with the answer.  The params record is host
 * memory, read before the call returns.
 * Refused with PRT_HIP_EINVAL and a message, before anything is queued and with out untouched: a NULL pointer; a parameter out
 * of range; a stride that is not a multiple of 3; reserved != 0; unknown flag bits; a misaligned device pointer; ranges of values
 * and out that overlap.
 * State: the call needs no scene and changes nothing in the context but scratch buffers of its own (the map, 16 bytes per point
 * and two planes of stride + 1 floats per point, grown on demand); it is not a launch for prt_hip_get_stats.
 * Not built: a per-sample variance output from the baker (the filter estimates variance spatially); seam stitching; albedo
 * demodulation; filtering camera or lens images; ranks. ---- */
typedef struct { uint32_t iterations;      /* 1 .. 5 */
                 uint32_t normalPowerLog2; /* 0 .. 7 */
                 float sigmaLuminance;     /* finite, > 0 */
                 float sigmaPosition;      /* finite, > 0; in texel footprints */
                 uint32_t reserved[4];     /* 0 */ } prt_atlas_filter_params;   /* 32 bytes */
int prt_hip_atlas_filter(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels,
                         const prt_bake_point* points, const float* values /* n*stride */, uint32_t stride /* 3*C, C 1 .. 16 */,
                         const prt_atlas_filter_params* params, float* out /* n*stride */, uint32_t flags, void* stream);

/* ---- visibility baking: points and direction sets in, the summed weights of the directions that escape out.  How much of a
 * hemisphere, or of the sky, a point can see is what a lightmapper asks for most often: ambient occlusion maps, sky-visibility masks
 * for a separately lit sky, bent normals and SH9 visibility probes are all one computation -- fire a direction set from each point and
 * sum the weights of the directions that escape.  The points and the table are those of prt_hip_bake; the rays are built in
 * registers from the point and its direction set and never exist in memory, and the answer per ray is one byte.
 *
 * Definition.  No new arithmetic: every piece is one defined above.
 * Ray r = i*K + k has the org and dir of prt_hip_bake_rays for the same points and table (the frame of path_tracer.cpp:147-153 with
 *     N as given, org = P + bias*N; the identity frame for N = 0); its tMax is vis->maxDistance, in units of the ray's dir.
 * Occlusion byte.  occ[r] is the answer of prt_hip_query_any for that ray, with all of that call's rules: alpha tests apply, and a
 *     NaN in org, dir or tMax gives "not occluded" (0) without a walk.  A point with set >= nSets (0xffffffff included) is never
 *     traced: its K bytes are 0.
 * Reduce, one wavefront per point, in the order of prt_hip_bake_reduce, fixed by K alone:
 *     1. for lane l = 0..63, for channel c: a_l = +0
 *     2. for k = l, l+64, l+128, ... < K: if occ[r] == 0 then a_l = a_l + weights[(s*K + k)*C + c]
 *     3. for step = 32, 16, 8, 4, 2, 1, for l < step: a_l = a_l + a_(l+step)
 *     4. out[i*C + c] = a_0; under PRT_HIP_VIS_TRIPLE out[(i*C + c)*3 + h] = a_0 for h = 0, 1, 2
 *     Any non-zero byte counts as occluded.  An occluded direction's weight is not read into the sum, so a NaN weight there
 *     changes nothing; a NaN weight of a direction that escapes gives a NaN in that point's channel and in no other point.
 *     A point with set >= nSets writes +0 to all its floats.
 * Recipes: cosine-weighted directions with weights 1/K give ambient occlusion (1 = open) under a finite maxDistance and sky
 * visibility under +inf; C = 3 with weights d_k/K, d_k in the local frame, gives the bent normal; uniform directions with
 * weights 4pi/K * Y_c(d_k) and N = 0 give an SH9 visibility probe.
 *
 * prt_hip_bake_visibility runs the trace and the reduce in order on the context's stream.  The bytes go to `occluded`, or, when it is
 * NULL, to a buffer the context owns, grown on demand: 1 byte per ray against the 44 bytes per ray of prt_hip_bake.
 * prt_hip_bake_visibility_reduce is the second half on the caller's bytes: a baker who kept them sums them again under other
 * weights without tracing again.  It reads no directions (sets->dirs may be NULL there) and needs no scene.
 * Limits: K 1 .. 4096, C 1 .. 16, nSets 1 .. 1024, n >= 1, n*K <= 2^30, the limit of the ray queries.  The 2^24 cap of prt_hip_bake
 * does not apply: no probe launch is involved.
 * Pointers, flags and stream as for the baker: DEVICE pointers by default, sets->dirs and sets->weights included (points 16-byte
 * aligned, floats 4-byte aligned, bytes as they come); asynchronous, ordered after the work queued on stream and before what is
 * queued next.  With PRT_HIP_QUERY_HOST every array is HOST memory, staged in the context's arena, and the call returns with the
 * answer.  The prt_bake_sets and prt_visibility_params records are host memory, read before the call returns.
 * Refused with PRT_HIP_EINVAL and a message, before anything is queued and with the outputs untouched: a NULL pointer other than
 * `occluded` in prt_hip_bake_visibility; a table out of range; maxDistance NaN or <= 0; unknown bits in vis->flags or flags;
 * reserved != 0; a misaligned device pointer.  prt_hip_bake_visibility without a scene is PRT_HIP_ESTATE.
 * State: the call reads the scene and changes nothing else in the context, apart from a scratch buffer of its own: the camera, the
 * accumulator, the moments, the guides, the history, the display state and the framebuffer are untouched.
 * Statistics: the trace is a launch like prt_hip_query_any's -- raysTraced = occludedTraced = n*K, and a stack overflow is reported
 * there; the reduce is not a launch for prt_hip_get_stats.
 * Not built: distance falloff (needs nearest hits); back-face and validity counts; ranks; a per-ray tMax. ---- */
#define PRT_HIP_VIS_TRIPLE 1u  /* vis->flags: every channel is written three times, the (n, C, 3) layout of prt_hip_bake */
typedef struct { float maxDistance;   /* > 0 or +inf, in units of the ray's dir */
                 uint32_t flags;      /* PRT_HIP_VIS_TRIPLE; other bits refused */
                 uint32_t reserved[2]; /* 0 */ } prt_visibility_params;   /* 16 bytes, host memory, read before the call returns */
int prt_hip_bake_visibility(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets,
                            const prt_visibility_params* vis, float* out /* n*C, or 3*n*C under TRIPLE */,
                            uint8_t* occluded /* n*K, may be NULL */, uint32_t flags, void* stream);
int prt_hip_bake_visibility_reduce(prt_hip_ctx* ctx, uint32_t n, const prt_bake_point* points, const prt_bake_sets* sets,
                                   const prt_visibility_params* vis, const uint8_t* occluded /* n*K */, float* out,
                                   uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
