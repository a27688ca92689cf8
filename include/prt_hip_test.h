/*
 * prt_hip_test.h -- row-level entry points of the TEST build of the library (libprt_hip_test.so = the product's sources
 * compiled with -DPRT_TEST_ENTRY_POINTS, plus the translation units only this build has: prt_amd/_build.py TEST_SOURCES).
 * They exist so that the parity tests can drive single rows of SURVEY.md 8(a) (leaf math, the four traversals, the camera
 * packet, sin/cos/pow) on the device; libprt_hip.so, the product, exports none of them and compiles none of their kernels.
 */
#ifndef PRT_HIP_TEST_H
#define PRT_HIP_TEST_H

#include "prt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the four traversals on caller-supplied rays (host pointers) ----
 * mode 0: Scene::intersect<SingleRayHitPacket,SingleRayPacket>   (scene.cpp:47, bvh.cpp:429 single branch)
 * mode 1: Scene::intersect<RayHitPacket,RayPacket>               (packet branch; rays in groups of 8, avgDir = sum/8)
 * mode 2: Scene::occluded<bool,SingleRayPacket>                  (scene.cpp:69, bvh.cpp:576); hit.t = 1 if occluded else 0
 * mode 3: Scene::occluded<RayPacketMask,RayPacket> with a full mask
 * n rays (multiple of 8); org/dir are n*3 floats. */
int prt_hip_trace_rays(prt_hip_ctx* ctx, int mode, uint32_t n, const float* org, const float* dir, float maxT,
                       prt_hit* hits);
/* leaf math on the device (triangle.cpp:90-166, vecmath.h:1402-1518, ray.h:26-71).  in: 22 floats per record =
 * org[3] dir[3] p0[3] p1[3] p2[3] lower[3] upper[3] maxT; out: 24 floats = [0..3] t,i,j,k with SoaRay::prepare swaps,
 * [4..7] with Ray::prepare swaps, [12] box t, [13] box bool(maxT), [14] box SoA mask(maxT), [16..18] invDir,
 * [19..22] swapXZ/swapYZ (SoA), swapXZ/swapYZ (single) */
int prt_hip_test_leaf(prt_hip_ctx* ctx, uint32_t n, const float* records, float* out);
/* sin/cos of theta[i] as the kernels compute them (prt_devmath.h) */
int prt_hip_test_sincos(prt_hip_ctx* ctx, uint32_t n, const float* theta, float* sin_out, float* cos_out);
/* powf(x, 2.2f) as material.cpp:24-28 (degamma) needs it */
int prt_hip_test_powf(prt_hip_ctx* ctx, uint32_t n, const float* x, float* y);
/* Camera::GenerateJitteredRayPacket + Random on the device: out = 8 x {org[3] dir[3] invDir[3] swapXZ swapYZ},
 * avgDir[3], state after (as float bits) = 92 floats */
int prt_hip_test_camera(prt_hip_ctx* ctx, uint32_t x, uint32_t y, uint32_t state, float* out92);
/* tools/denoise_bench.py: prt_hip_accum_denoise into the context's framebuffer twice, timed with HIP events; ms[0] = the prepare
 * kernel, ms[1..5] = the iterations (0 beyond params->iterations) of the second run, ms[6] = the whole first run (no events
 * inside).  Synchronous. */
int prt_hip_test_denoise_profile(prt_hip_ctx* ctx, const prt_denoise_params* params, float exposure, float* ms7);
/* tools/query_bench.py --atlas-filter: prt_hip_atlas_filter on DEVICE arrays twice, timed with HIP events; ms[0] = the map's clear and
 * the index kernel, ms[1] = the prepare kernel, ms[2..6] = the iterations (0 beyond params->iterations) of the second run, ms[7] = the
 * whole first run (no events inside).  Synchronous; refuses what the call refuses. */
int prt_hip_test_atlas_filter_profile(prt_hip_ctx* ctx, uint32_t W, uint32_t H, uint32_t n, const uint32_t* texels, const prt_bake_point* points,
                                      const float* values, uint32_t stride, const prt_atlas_filter_params* params, float* out, float* ms8);
/* the yardstick of the same tool: one launch (after a warm-up launch) of a plain copy kernel in which every thread reads one element
 * of read16 16-byte planes and read12 12-byte planes and writes one of write16 16-byte and write12 12-byte planes of `pixels`
 * elements, in buffers of its own; *ms = its time */
int prt_hip_test_copy_yardstick(prt_hip_ctx* ctx, uint64_t pixels, int read16, int read12, int write16, int write12, float* ms);
/* tools/temporal_bench.py: HIP-event times on the context's stream; ms[0] = the merge kernel alone, ms[1] = merge + iterations (a whole
 * prt_hip_accum_denoise_temporal into the context's framebuffer), ms[2] = one position pass (0 with a host's plane), ms[3] = one
 * prt_hip_render_gbuffer launch (type 0) of the same view; the last two include the two small memsets of a launch.  Synchronous. */
int prt_hip_test_temporal_profile(prt_hip_ctx* ctx, const prt_denoise_params* params, const prt_temporal_params* temporal, float exposure,
                                  float* ms4);

/* The device scene arrays as they stand, to host buffers (any of them may be NULL): counts[0] node records (16 floats each),
 * [1] hot copies (16 floats each), [2] triangle slots (tris: 9 floats each, shade: 16 floats each), [3] bump records (12 floats
 * each; 0 when the scene has no bump map), [4] meshes; rootBoxes: PRT_HIP_MAX_BVH x 6 floats, radius: 1 float.  Call it with NULL
 * buffers for the counts first.  Synchronous. */
int prt_hip_test_scene_arrays(prt_hip_ctx* ctx, uint64_t counts[5], float* wnodes, float* hot, float* tris, float* shade, float* bump,
                              float* rootBoxes, float* radius);
/* tools/refit_bench.py: prt_hip_update_meshes' device work queued `reps` times between HIP events on the context's stream; ms[0] =
 * median time of the gather kernels, ms[1] = median of the level launches and the finish kernel (the copies of the caller's arrays
 * lie before both).  Ends with one real prt_hip_update_meshes.  Synchronous. */
int prt_hip_test_refit_profile(prt_hip_ctx* ctx, uint32_t count, const prt_mesh_update* updates, uint32_t reps, float* ms2);
/* tools/refit_bench.py --device: prt_hip_deform_meshes' device work queued `reps` times between HIP events on the context's stream;
 * ms[0..4] = medians of keep + box, face normals, vertex normals, gather, level launches + finish.  Ends with one real
 * prt_hip_deform_meshes.  Synchronous. */
int prt_hip_test_deform_profile(prt_hip_ctx* ctx, uint32_t count, const prt_mesh_deform* deforms, uint32_t flags, uint32_t reps, float* ms5);
/* Occlusion rays of the context's last render (or accumulate / adaptive pass) that the frame kernel answered without a walk: the
 * surface faces away from the slot's light, so an unoccluded answer would add +-0.  They are part of
 * prt_hip_stats.occludedTraced and raysTraced, which count the reference's rays; 0 for a render with countTraffic, which walks every
 * ray.  Synchronous. */
int prt_hip_test_occlusion_skipped(prt_hip_ctx* ctx, uint64_t* skipped);
/* The device arrays a scene edit ("scene edits" in prt_hip.h) can change, as they stand, to host buffers (any of them may be NULL):
 * counts[0] material records (20 floats each), [1] alpha class words, [2] texel bytes, [3] / [4] width / height of the environment map
 * (0 without one: envTexels 4 floats, envHorizontal 1 float per texel, envVertical and envFirstX one entry per row); the scalars of
 * DevScene beside them.  Call it with NULL buffers for the counts first.  Synchronous. */
int prt_hip_test_shading_arrays(prt_hip_ctx* ctx, uint64_t counts[5], float* mats, uint32_t* alphaClass, uint8_t* texels, float* envTexels,
                                float* envVertical, float* envHorizontal, int32_t* envFirstX, int32_t* envFirstY, uint32_t* hasLight,
                                float* lightDir, float* lightIntensity, uint32_t* hasEnv);
/* The arithmetic the environment kernels run (prt_envcdf.h), on the HOST: the two tables, firstX[height], *firstY and the refusal flags
 * (1 vertical table not non-decreasing, 2 partly NaN row, 4 row not non-decreasing; 0 = the map is accepted) of a width x height
 * float RGBA image.  Takes no context and needs no device. */
int prt_hip_test_env_tables_host(int32_t width, int32_t height, const float* rgba, float* vertical, float* horizontal, int32_t* firstX,
                                 int32_t* firstY, uint32_t* flags);
/* tools/scene_edit_bench.py: HIP-event times on the context's stream, medians of `reps`: ms[0] = the two kernels that build the tables of
 * the context's own environment map again, into scratch buffers (0 without one); ms[1] = the class kernels of the named textures, whose
 * texels are copied first (count 0: ms[1] = 0).  Ends with one real update of those textures.  Synchronous. */
int prt_hip_test_edit_profile(prt_hip_ctx* ctx, uint32_t count, const prt_texture_update* updates, uint32_t reps, float* ms2);
/* The arithmetic of the display kernels (prt_display.h) on the HOST: metering over the rectangle (meter 1; *state is the adaptation
 * state going in and coming out) and the transform of the rectangle of a width x height float RGB image into `out` (width * height *
 * bytesPerPixel bytes; only the rectangle's are written).  Takes no context and needs no device; the refusals of the device call. */
int prt_hip_test_display_host(uint32_t width, uint32_t height, const float* rgb, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                              const prt_display_params* params, prt_display_state* state, uint8_t* out);
/* tools/display_bench.py: HIP-event times on the context's stream, medians of `reps` displays (after one warm-up) of the whole
 * framebuffer into the context's display buffer: ms[0] = the histogram kernel with its memset, ms[1] = the resolve kernel (both 0 with
 * meter 0), ms[2] = the transform kernel.  The adaptation state advances as by that many displays.  Synchronous. */
int prt_hip_test_display_profile(prt_hip_ctx* ctx, const prt_display_params* params, uint32_t reps, float* ms3);
/* Texture taps on the uploaded scene's own arrays (texture.cpp:31-183, material.cpp:87-96).  records: n x 4 words {material (global
 * index: the scene's materials in mesh order), f32 u, f32 v, flags}; flags 1: the single-ray flavours (uv must be finite; the material
 * needs both maps), 2: the alpha tests (the material is alpha-tested, its diffuse map has 4 components).  out: n x 12 words:
 * [0..2] tex_sample3 of the diffuse map, [3] tex_sample1 of the bump map, [4] the alpha decision of a leaf round for a single ray
 * (class word, then the blend -- alpha_decide, prt_device.h), [5] the same for a packet, [6..8] sample_diffuse, [9] taps counted
 * (counting form), [10..11] 0.  counting != 0 runs the kernels' counting form (prt_render_params.countTraffic).  blocks = workgroups of
 * 256 threads to launch (the kernel strides over the records), 0 = one thread per record.  Refuses what would read outside the scene's
 * arrays.  Synchronous. */
int prt_hip_test_taps(prt_hip_ctx* ctx, uint32_t n, const uint32_t* records, int counting, uint32_t blocks, uint32_t* out);
/* Mesh::getSurfaceProperties and Material::sampleBump (mesh.cpp:311-364, material.cpp:98-114) on the uploaded scene's own records.
 * records: n x 5 words {mesh, primId in mesh order, f32 i, j, k}; out: n x 20 words: [0..2] normal, [3..4] uv, [5] material (index within
 * the mesh), [6..9] duv01, duv02 and [10..15] dp01, dp02 as the bump record of the triangle holds them (0 in a scene without a bump
 * map), [16..18] sample_bump's normal, [19] taps counted (counting form).  counting, blocks: as above.  Synchronous. */
int prt_hip_test_surface(prt_hip_ctx* ctx, uint32_t n, const uint32_t* records, int counting, uint32_t blocks, uint32_t* out);
/* InfiniteAreaLight::sample (light.cpp:86-128) on the uploaded scene's own tables, texels and `first` constants (env_sample / cdf_find,
 * prt_device.h).  u: n x 2 floats {u.x, u.y}, each in [0, 1) as the generator gives them (anything else is refused: EINVAL); out: n x 8
 * words: [0..2] dir, [3..5] color, [6] taps counted (counting form: 1), [7] 0.  counting, blocks: as above.  ESTATE without a scene or
 * when the scene has no environment map.  Synchronous. */
int prt_hip_test_env_sample(prt_hip_ctx* ctx, uint32_t n, const float* u, uint32_t* out, int counting, uint32_t blocks);

#ifdef __cplusplus
}
#endif
#endif
