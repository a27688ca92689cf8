// prt_edit.hip -- scene edits (include/prt_hip.h "scene edits"): the lights, single material records and the texels of single
// textures of the uploaded scene are replaced in place, and what prt_hip_upload_scene derives from them is rebuilt on the device:
//   env     the two CDF tables of a new environment map (InfiniteAreaLight::create, light.cpp:30-84), with the first-step constants
//           and the refusals of the upload.  Every sum runs in index order (prt_envcdf.h), so the parallelism is ACROSS rows and,
//           within a row, in the loads and the lengths: one wavefront per row, whose 64 lanes load 64 consecutive float4 texels
//           (one coalesced KB), compute their lengths and park them in LDS, where lane 0 folds them in order -- once for the row
//           sum, once for the running table.  The column is one more wavefront doing the same two folds over `height` values.
//   class   the 2-bit alpha classes of a repainted texture's bilinear cells (prt_upload.hip classWord): one thread per 32-bit word
//           of 16 cells, no atomics.
// Nothing here touches the frame kernels: DevScene keeps its layout, and the launches after an edit take the edited copy by value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prt_hip.h"
#include "prt_device.h"
#include "prt_envcdf.h"
#include "prt_internal.h"
#ifdef PRT_TEST_ENTRY_POINTS
#include "../../include/prt_hip_test.h"
#endif

#define PRT_EDIT_BLOCK 256

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

// One wavefront per row y = blockIdx.x.  hor: the horizontal table (width * height); vertRaw[y] = hsum * sinPhi, the column's terms.
__global__ __launch_bounds__(PRT_ENV_CHUNK) void env_rows_kernel(const float4* texels, int32_t width, int32_t height, float* hor, float* vertRaw,
                                                                 int32_t* firstX, uint32_t* result)
{
    __shared__ float term[PRT_ENV_CHUNK];
    const uint32_t y = blockIdx.x, lane = threadIdx.x, W = (uint32_t)width;
    const float4* row = texels + (size_t)y * W;
    float* out = hor + (size_t)y * W;
    float hsum = 0.0f; // lane 0's
    for (uint32_t x0 = 0; x0 < W; x0 += PRT_ENV_CHUNK) {
        const uint32_t n = W - x0 < PRT_ENV_CHUNK ? W - x0 : PRT_ENV_CHUNK;
        if (lane < n) {
            const float4 t = row[x0 + lane];
            const float l = prt_env_length(t.x, t.y, t.z);
            term[lane] = l;
            out[x0 + lane] = l; // light.cpp:54: the table holds the lengths until the second pass
        }
        __syncthreads();
        if (lane == 0) hsum = prt_env_sum(hsum, term, n);
        __syncthreads();
    }
    float invH = 0.0f;
    if (lane == 0) {
        vertRaw[y] = hsum * prt_env_sin_phi(y, height);
        invH = 1.0f / hsum;
    }
    PrtEnvScan s = prt_env_scan_begin();
    for (uint32_t x0 = 0; x0 < W; x0 += PRT_ENV_CHUNK) {
        const uint32_t n = W - x0 < PRT_ENV_CHUNK ? W - x0 : PRT_ENV_CHUNK;
        if (lane < n) term[lane] = out[x0 + lane]; // this lane's own store of the first pass
        __syncthreads();
        if (lane == 0) prt_env_scan(&s, invH, term, n, PRT_ENV_BAD_ROW, PRT_ENV_PARTLY_NAN);
        __syncthreads();
        if (lane < n) out[x0 + lane] = term[lane];
    }
    if (lane == 0) {
        firstX[y] = prt_env_first_step(&s, width);
        if (s.flags) atomicOr(result, s.flags);
    }
}

// One wavefront: the vertical table from the rows' terms, in place.  result[0] |= flags, result[1] = envFirstY.
__global__ __launch_bounds__(PRT_ENV_CHUNK) void env_column_kernel(float* vert, int32_t height, uint32_t* result)
{
    __shared__ float term[PRT_ENV_CHUNK];
    const uint32_t lane = threadIdx.x, H = (uint32_t)height;
    float vsum = 0.0f;
    for (uint32_t y0 = 0; y0 < H; y0 += PRT_ENV_CHUNK) {
        const uint32_t n = H - y0 < PRT_ENV_CHUNK ? H - y0 : PRT_ENV_CHUNK;
        if (lane < n) term[lane] = vert[y0 + lane];
        __syncthreads();
        if (lane == 0) vsum = prt_env_sum(vsum, term, n);
        __syncthreads();
    }
    const float invV = 1.0f / vsum;
    PrtEnvScan s = prt_env_scan_begin();
    for (uint32_t y0 = 0; y0 < H; y0 += PRT_ENV_CHUNK) {
        const uint32_t n = H - y0 < PRT_ENV_CHUNK ? H - y0 : PRT_ENV_CHUNK;
        if (lane < n) term[lane] = vert[y0 + lane];
        __syncthreads();
        if (lane == 0) prt_env_scan(&s, invV, term, n, PRT_ENV_BAD_VERTICAL, 0u);
        __syncthreads();
        if (lane < n) vert[y0 + lane] = term[lane];
    }
    if (lane == 0) {
        if (s.flags) atomicOr(result, s.flags);
        result[1] = (uint32_t)prt_env_first_step(&s, height);
    }
}

// One thread per class word: the 16 cells cell = 16 * word + j of a w x h texture whose texels start at px (prt_upload.hip classWord).
__global__ __launch_bounds__(PRT_EDIT_BLOCK) void alpha_class_kernel(const uint8_t* px, int32_t w, int32_t h, int32_t comp, uint32_t* words, uint32_t wordCount)
{
    const uint32_t i = blockIdx.x * PRT_EDIT_BLOCK + threadIdx.x;
    if (i >= wordCount) return;
    const uint64_t cells = (uint64_t)w * (uint64_t)h;
    uint32_t word = 0u;
    for (uint32_t j = 0; j < 16u; j++) {
        const uint64_t cell = (uint64_t)i * 16u + j;
        if (cell >= cells) break;
        const int32_t x0 = (int32_t)(cell % (uint64_t)w), y0 = (int32_t)(cell / (uint64_t)w);
        const int32_t x1 = (x0 + 1 < w - 1) ? x0 + 1 : w - 1;
        const int32_t y1 = (y0 + 1 < h - 1) ? y0 + 1 : h - 1;
        auto alphaOf = [&](int32_t x, int32_t y) -> uint32_t { return px[(size_t)comp * ((size_t)x + (size_t)y * (size_t)w) + 3]; };
        const uint32_t a0 = alphaOf(x0, y0), a1 = alphaOf(x1, y0), a2 = alphaOf(x0, y1), a3 = alphaOf(x1, y1);
        const uint32_t lo = min(min(a0, a1), min(a2, a3)), hi = max(max(a0, a1), max(a2, a3));
        const uint32_t cls = lo >= 128u ? 1u : (hi <= 126u ? 2u : 0u);
        word |= cls << (j * 2u);
    }
    words[i] = word;
}

struct EnvBuild { // the buffers of a new environment map, not yet the scene's
    DevBuf<float4> texels;
    DevBuf<float> vert, hor;
    DevBuf<int32_t> firstX;
    DevBuf<uint32_t> result; // {flags, envFirstY}
};

// The scene's environment map becomes b's (an empty b: none), of W x H texels.  The old arrays are freed here: the stream is idle.
void set_env(prt_hip_ctx* c, EnvBuild&& b, int32_t W, int32_t H, int32_t firstY)
{
    c->sc.hasEnv = b.texels ? 1u : 0u;
    c->arr.envTexels = std::move(b.texels);
    c->arr.envV = std::move(b.vert);
    c->arr.envHor = std::move(b.hor);
    c->arr.envFirstX = std::move(b.firstX);
    prt_scene_view(c);
    c->sc.envW = W;
    c->sc.envH = H;
    c->sc.envFirstY = firstY;
}

// the samples of the old lights, materials or texels: accumulator, moments, estimator, history and pending record
void forget_radiance(prt_hip_ctx* c)
{
    prt_accum_forget(c);
    c->tpHaveHist = c->tpHavePend = false;
}

int env_alloc(EnvBuild& b, int32_t W, int32_t H, hipStream_t s)
{
    const size_t n = (size_t)W * H;
    hipError_t e = b.texels.fit(n, s);
    if (e == hipSuccess) e = b.vert.fit((size_t)H, s);
    if (e == hipSuccess) e = b.hor.fit(n, s);
    if (e == hipSuccess) e = b.firstX.fit((size_t)H, s);
    if (e == hipSuccess) e = b.result.fit(16, s);
    if (e != hipSuccess) // (what was allocated goes with b)
        return fail(e == hipErrorOutOfMemory ? PRT_HIP_ENOMEM : PRT_HIP_ENODEVICE, std::string("environment light buffers: ") + hipGetErrorString(e));
    return PRT_HIP_OK;
}

// the copy of the image and the two kernels on s; tm (optional, 2 marks) around the kernels
int env_queue(const EnvBuild& b, int32_t W, int32_t H, const float* texels, hipStream_t s, StageTimer* tm)
{
    if (texels) HIP_TRY(hipMemcpyAsync(b.texels, texels, (size_t)W * H * sizeof(float4), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b.result, 0, 64, s));
    if (tm) HIP_TRY(tm->mark(s));
    hipLaunchKernelGGL(env_rows_kernel, dim3((uint32_t)H), dim3(PRT_ENV_CHUNK), 0, s, b.texels, W, H, b.hor, b.vert, b.firstX, b.result);
    int rc = prt_launched("env_rows_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(env_column_kernel, dim3(1), dim3(PRT_ENV_CHUNK), 0, s, b.vert, H, b.result);
    if ((rc = prt_launched("env_column_kernel"))) return rc;
    if (tm) HIP_TRY(tm->mark(s));
    return PRT_HIP_OK;
}

int env_refusal(uint32_t flags)
{
    if (flags & PRT_ENV_BAD_VERTICAL) return fail(PRT_HIP_EINVAL, "environment light: vertical CDF is not non-decreasing (negative or non-finite radiance?)");
    if (flags & PRT_ENV_PARTLY_NAN) return fail(PRT_HIP_EINVAL, "environment light: partly NaN CDF row");
    if (flags & PRT_ENV_BAD_ROW) return fail(PRT_HIP_EINVAL, "environment light: horizontal CDF is not non-decreasing (negative or non-finite radiance?)");
    return PRT_HIP_OK;
}

int check_lights(prt_hip_ctx* c, const prt_light_update* u)
{
    if (!c || !u) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (u->envMode > PRT_HIP_ENV_REPLACE) return fail(PRT_HIP_EINVAL, "envMode must be PRT_HIP_ENV_KEEP, PRT_HIP_ENV_NONE or PRT_HIP_ENV_REPLACE");
    if (u->envMode == PRT_HIP_ENV_REPLACE) {
        if (u->envWidth <= 0 || u->envHeight <= 0) return fail(PRT_HIP_EINVAL, "incomplete environment light: width and height must be positive");
        if ((int64_t)u->envWidth * u->envHeight > (1 << 28)) return fail(PRT_HIP_EINVAL, "environment map too large");
        if (!u->envTexels) return fail(PRT_HIP_EINVAL, "incomplete environment light: envTexels is NULL");
    }
    return PRT_HIP_OK;
}

// every refusal of prt_hip_update_materials; nothing has changed when it returns non-zero
int check_materials(prt_hip_ctx* c, uint32_t count, const prt_material_update* u)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (count == 0 || !u) return fail(PRT_HIP_EINVAL, "no material update given");
    const PrtEdit& E = c->ed;
    const int32_t textures = (int32_t)E.texDesc.size();
    for (uint32_t k = 0; k < count; k++) {
        const std::string which = "update " + std::to_string(k) + ": ";
        if (u[k].mesh >= E.meshes.size()) return fail(PRT_HIP_EINVAL, which + "mesh index out of range");
        const PrtEditMesh& M = E.meshes[u[k].mesh];
        if (u[k].material >= M.materials.size()) return fail(PRT_HIP_EINVAL, which + "material index out of range");
        for (uint32_t j = 0; j < k; j++)
            if (u[j].mesh == u[k].mesh && u[j].material == u[k].material)
                return fail(PRT_HIP_EINVAL, which + "material " + std::to_string(u[k].material) + " of mesh " + std::to_string(u[k].mesh) + " is named twice in one call");
        const prt_material& was = M.materials[u[k].material];
        const prt_material& v = u[k].value;
        if (v.alphaTest != was.alphaTest)
            return fail(PRT_HIP_EINVAL, which + "alphaTest differs from the uploaded value (alpha records and leaf flags are fixed at upload)");
        if (v.diffuseMap >= textures || v.bumpMap >= textures) return fail(PRT_HIP_EINVAL, which + "material texture index out of range");
        if (was.alphaTest && v.diffuseMap != was.diffuseMap)
            return fail(PRT_HIP_EINVAL, which + "another diffuseMap for a material uploaded with alphaTest (its alpha records are fixed at upload)");
        if (v.bumpMap >= 0 && !c->arr.anyBump()) return fail(PRT_HIP_EINVAL, which + "bumpMap in a scene uploaded without bump-mapped materials (it has no bump records)");
        if (v.reflectionType > 2u) return fail(PRT_HIP_EINVAL, which + "reflectionType must be 0, 1 or 2");
        if ((uint64_t)M.matBase + u[k].material >= c->arr.mats.size() / PRT_MAT_STRIDE) return fail(PRT_HIP_EINVAL, which + "internal: material record outside the table");
    }
    return PRT_HIP_OK;
}

int check_textures(prt_hip_ctx* c, uint32_t count, const prt_texture_update* u)
{
    if (!c) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    if (count == 0 || !u) return fail(PRT_HIP_EINVAL, "no texture update given");
    const PrtEdit& E = c->ed;
    for (uint32_t k = 0; k < count; k++) {
        const std::string which = "update " + std::to_string(k) + ": ";
        if (u[k].texture >= E.texDesc.size()) return fail(PRT_HIP_EINVAL, which + "texture index out of range");
        const uint4 d = E.texDesc[u[k].texture];
        if (u[k].width != (int32_t)d.y || u[k].height != (int32_t)d.z || u[k].component != (int32_t)d.w)
            return fail(PRT_HIP_EINVAL, which + "size " + std::to_string(u[k].width) + " x " + std::to_string(u[k].height) + " x " + std::to_string(u[k].component) +
                                            " differs from the uploaded texture's " + std::to_string(d.y) + " x " + std::to_string(d.z) + " x " + std::to_string(d.w));
        if (!u[k].texels) return fail(PRT_HIP_EINVAL, which + "texels is NULL");
        for (uint32_t j = 0; j < k; j++)
            if (u[j].texture == u[k].texture) return fail(PRT_HIP_EINVAL, which + "texture " + std::to_string(u[k].texture) + " is named twice in one call");
        const uint64_t bytes = (uint64_t)d.y * d.z * d.w, words = ((uint64_t)d.y * d.z + 15) / 16;
        if ((uint64_t)d.x + bytes > c->arr.texels.size()) return fail(PRT_HIP_EINVAL, which + "internal: texture outside the texel array");
        const uint32_t first = E.classWordOf[u[k].texture];
        if (first != 0xffffffffu && (uint64_t)first + words > c->arr.alphaClass.size()) return fail(PRT_HIP_EINVAL, which + "internal: class words outside their array");
    }
    return PRT_HIP_OK;
}

// the copies of the caller's texels, then the class kernels, on s; tm (optional, 2 marks) around the kernels
int queue_textures(prt_hip_ctx* c, uint32_t count, const prt_texture_update* u, hipStream_t s, StageTimer* tm)
{
    const PrtEdit& E = c->ed;
    uint8_t* texels = c->arr.texels;
    for (uint32_t k = 0; k < count; k++) {
        const uint4 d = E.texDesc[u[k].texture];
        HIP_TRY(hipMemcpyAsync(texels + d.x, u[k].texels, (size_t)d.y * d.z * d.w, hipMemcpyHostToDevice, s));
    }
    if (tm) HIP_TRY(tm->mark(s));
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t first = E.classWordOf[u[k].texture];
        if (first == 0xffffffffu) continue; // no alpha-tested material names it
        const uint4 d = E.texDesc[u[k].texture];
        const uint32_t words = (uint32_t)(((uint64_t)d.y * d.z + 15) / 16);
        hipLaunchKernelGGL(alpha_class_kernel, dim3((words + PRT_EDIT_BLOCK - 1) / PRT_EDIT_BLOCK), dim3(PRT_EDIT_BLOCK), 0, s, texels + d.x, (int32_t)d.y,
                           (int32_t)d.z, (int32_t)d.w, c->arr.alphaClass + first, words);
        int rc = prt_launched("alpha_class_kernel");
        if (rc) return rc;
    }
    if (tm) HIP_TRY(tm->mark(s));
    return PRT_HIP_OK;
}

} // namespace

extern "C" {

int prt_hip_update_lights(prt_hip_ctx* c, const prt_light_update* u, void* stream)
{
    int rc = check_lights(c, u);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream, caller;
    if (u->envMode == PRT_HIP_ENV_REPLACE) {
        const int32_t W = u->envWidth, H = u->envHeight;
        EnvBuild b; // NEW buffers: a refused map leaves the scene's own untouched
        if ((rc = env_alloc(b, W, H, s))) return rc;
        uint32_t result[2] = {0u, 0u};
        hipError_t e = hipSuccess;
        if ((rc = prt_stream_enter(c, stream, &caller)) == PRT_HIP_OK && (rc = env_queue(b, W, H, u->envTexels, s, nullptr)) == PRT_HIP_OK) {
            e = hipMemcpyAsync(result, b.result, sizeof(result), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) rc = prt_stream_leave(c, caller);
            if (e == hipSuccess && rc == PRT_HIP_OK) e = hipStreamSynchronize(s); // the flags decide; envFirstY is part of DevScene
        }
        if (rc == PRT_HIP_OK && e != hipSuccess) rc = fail(PRT_HIP_ENODEVICE, std::string("environment light build: ") + hipGetErrorString(e));
        if (rc == PRT_HIP_OK) rc = env_refusal(result[0]);
        if (rc) {
            (void)hipStreamSynchronize(s); // then b's buffers go with it
            return rc;
        }
        set_env(c, std::move(b), W, H, (int32_t)result[1]); // (the stream is idle: no launch still reads the old buffers)
    } else if (u->envMode == PRT_HIP_ENV_NONE && c->sc.hasEnv) {
        if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = prt_stream_leave(c, caller))) return rc;
        HIP_TRY(hipStreamSynchronize(s)); // launches queued before the call still read the buffers
        set_env(c, EnvBuild{}, 0, 0, 0);
    }
    c->sc.hasLight = u->hasDirectionalLight ? 1u : 0u;
    memcpy(c->sc.lightDir, u->lightDir, 12);
    memcpy(c->sc.lightIntensity, u->lightIntensity, 12);
    forget_radiance(c); // guides and position plane do not depend on a light
    return PRT_HIP_OK;
}

int prt_hip_update_materials(prt_hip_ctx* c, uint32_t count, const prt_material_update* updates, void* stream)
{
    int rc = check_materials(c, count, updates);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float4> records((size_t)count * PRT_MAT_STRIDE);
    for (uint32_t k = 0; k < count; k++) prt_material_record(updates[k].value, c->ed.texDesc, &records[(size_t)k * PRT_MAT_STRIDE]);
    hipStream_t s = c->stream, caller;
    if ((rc = prt_stream_enter(c, stream, &caller))) return rc;
    float4* mats = c->arr.mats;
    for (uint32_t k = 0; k < count; k++) {
        const size_t at = ((size_t)c->ed.meshes[updates[k].mesh].matBase + updates[k].material) * PRT_MAT_STRIDE;
        HIP_TRY(hipMemcpyAsync(mats + at, &records[(size_t)k * PRT_MAT_STRIDE], PRT_MAT_STRIDE * sizeof(float4), hipMemcpyHostToDevice, s));
    }
    if ((rc = prt_stream_leave(c, caller))) return rc;
    HIP_TRY(hipStreamSynchronize(s)); // the records leave this frame's memory
    for (uint32_t k = 0; k < count; k++) c->ed.meshes[updates[k].mesh].materials[updates[k].material] = updates[k].value;
    forget_radiance(c);
    prt_denoise_forget(c);
    prt_temporal_forget(c);
    return PRT_HIP_OK;
}

int prt_hip_update_textures(prt_hip_ctx* c, uint32_t count, const prt_texture_update* updates, void* stream)
{
    int rc = check_textures(c, count, updates);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream, caller;
    if ((rc = prt_stream_enter(c, stream, &caller)) || (rc = queue_textures(c, count, updates, s, nullptr)) || (rc = prt_stream_leave(c, caller))) return rc;
    HIP_TRY(hipStreamSynchronize(s)); // the caller's texels have been copied when the call returns
    forget_radiance(c);
    prt_denoise_forget(c);
    prt_temporal_forget(c);
    return PRT_HIP_OK;
}

#ifdef PRT_TEST_ENTRY_POINTS
int prt_hip_test_shading_arrays(prt_hip_ctx* c, uint64_t counts[5], float* mats, uint32_t* alphaClass, uint8_t* texels, float* envTexels,
                                float* envVertical, float* envHorizontal, int32_t* envFirstX, int32_t* envFirstY, uint32_t* hasLight,
                                float* lightDir, float* lightIntensity, uint32_t* hasEnv)
{
    if (!c || !counts) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    const PrtSceneArrays& A = c->arr;
    const DevScene& sc = c->sc;
    counts[0] = A.mats.size() / PRT_MAT_STRIDE;
    counts[1] = A.alphaClass.size();
    counts[2] = A.texels.size();
    counts[3] = sc.hasEnv ? (uint64_t)sc.envW : 0;
    counts[4] = sc.hasEnv ? (uint64_t)sc.envH : 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)counts[3] * counts[4];
    if (mats && counts[0]) HIP_TRY(hipMemcpy(mats, sc.mats, counts[0] * PRT_MAT_STRIDE * sizeof(float4), hipMemcpyDeviceToHost));
    if (alphaClass && counts[1]) HIP_TRY(hipMemcpy(alphaClass, sc.alphaClass, counts[1] * 4, hipMemcpyDeviceToHost));
    if (texels && counts[2]) HIP_TRY(hipMemcpy(texels, sc.texels, counts[2], hipMemcpyDeviceToHost));
    if (envTexels && n) HIP_TRY(hipMemcpy(envTexels, sc.envTexels, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (envVertical && n) HIP_TRY(hipMemcpy(envVertical, sc.envV, (size_t)counts[4] * 4, hipMemcpyDeviceToHost));
    if (envHorizontal && n) HIP_TRY(hipMemcpy(envHorizontal, sc.envHor, n * 4, hipMemcpyDeviceToHost));
    if (envFirstX && n) HIP_TRY(hipMemcpy(envFirstX, sc.envFirstX, (size_t)counts[4] * 4, hipMemcpyDeviceToHost));
    if (envFirstY) *envFirstY = sc.hasEnv ? sc.envFirstY : 0;
    if (hasLight) *hasLight = sc.hasLight;
    if (lightDir) memcpy(lightDir, sc.lightDir, 12);
    if (lightIntensity) memcpy(lightIntensity, sc.lightIntensity, 12);
    if (hasEnv) *hasEnv = sc.hasEnv;
    return PRT_HIP_OK;
}

// The functions of prt_envcdf.h on the HOST, chunk by chunk as the kernels hand them over: no context, no device.
int prt_hip_test_env_tables_host(int32_t width, int32_t height, const float* rgba, float* vertical, float* horizontal, int32_t* firstX,
                                 int32_t* firstY, uint32_t* flags)
{
    if (width <= 0 || height <= 0 || !rgba || !vertical || !horizontal || !firstX || !firstY || !flags) return fail(PRT_HIP_EINVAL, "NULL argument");
    if ((int64_t)width * height > (1 << 28)) return fail(PRT_HIP_EINVAL, "environment map too large");
    const uint32_t W = (uint32_t)width, H = (uint32_t)height;
    uint32_t all = 0u;
    for (uint32_t y = 0; y < H; y++) {
        const float* row = rgba + 4 * (size_t)y * W;
        float* out = horizontal + (size_t)y * W;
        float hsum = 0.0f;
        for (uint32_t x0 = 0; x0 < W; x0 += PRT_ENV_CHUNK) {
            const uint32_t n = std::min(W - x0, PRT_ENV_CHUNK);
            for (uint32_t k = 0; k < n; k++) out[x0 + k] = prt_env_length(row[4 * (x0 + k)], row[4 * (x0 + k) + 1], row[4 * (x0 + k) + 2]);
            hsum = prt_env_sum(hsum, out + x0, n);
        }
        vertical[y] = hsum * prt_env_sin_phi(y, height);
        const float invH = 1.0f / hsum;
        PrtEnvScan s = prt_env_scan_begin();
        for (uint32_t x0 = 0; x0 < W; x0 += PRT_ENV_CHUNK) prt_env_scan(&s, invH, out + x0, std::min(W - x0, PRT_ENV_CHUNK), PRT_ENV_BAD_ROW, PRT_ENV_PARTLY_NAN);
        firstX[y] = prt_env_first_step(&s, width);
        all |= s.flags;
    }
    float vsum = 0.0f;
    for (uint32_t y0 = 0; y0 < H; y0 += PRT_ENV_CHUNK) vsum = prt_env_sum(vsum, vertical + y0, std::min(H - y0, PRT_ENV_CHUNK));
    const float invV = 1.0f / vsum;
    PrtEnvScan s = prt_env_scan_begin();
    for (uint32_t y0 = 0; y0 < H; y0 += PRT_ENV_CHUNK) prt_env_scan(&s, invV, vertical + y0, std::min(H - y0, PRT_ENV_CHUNK), PRT_ENV_BAD_VERTICAL, 0u);
    *firstY = prt_env_first_step(&s, height);
    *flags = all | s.flags;
    return PRT_HIP_OK;
}

// tools/scene_edit_bench.py: HIP-event times on the context's stream, medians of `reps`.  ms[0]: the two kernels that build the tables
// of the context's OWN environment map again, into scratch buffers (0 without one); ms[1]: the class kernels of the named textures
// (updates may be NULL with count 0: ms[1] = 0), whose texels are copied first, as by prt_hip_update_textures, which the call
// ends with.  Synchronous.
int prt_hip_test_edit_profile(prt_hip_ctx* c, uint32_t count, const prt_texture_update* updates, uint32_t reps, float* ms2)
{
    if (!c || !ms2 || reps == 0) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "upload a scene first");
    int rc = count ? check_textures(c, count, updates) : PRT_HIP_OK;
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    const bool hasEnv = c->sc.hasEnv != 0;
    StageTimer env(1), cls(1);
    EnvBuild b; // its buffers go with the scope: every return below follows a synchronisation of what was queued on them
    if (hasEnv && (rc = env_alloc(b, c->sc.envW, c->sc.envH, s))) return rc;
    for (uint32_t r = 0; r < reps; r++) {
        if (hasEnv) {
            if (hipMemcpyAsync(b.texels, c->sc.envTexels, (size_t)c->sc.envW * c->sc.envH * sizeof(float4), hipMemcpyDeviceToDevice, s) != hipSuccess)
                return fail(PRT_HIP_ENODEVICE, "edit profile: copy failed");
            rc = env_queue(b, c->sc.envW, c->sc.envH, nullptr, s, &env);
            if (hipStreamSynchronize(s) != hipSuccess) return fail(PRT_HIP_ELAUNCH, "edit profile: synchronise failed");
            if (rc) return rc;
            HIP_TRY(env.lap());
        }
        if (count) {
            if ((rc = queue_textures(c, count, updates, s, &cls))) return rc;
            if (hipStreamSynchronize(s) != hipSuccess) return fail(PRT_HIP_ELAUNCH, "edit profile: synchronise failed");
            HIP_TRY(cls.lap());
        }
    }
    ms2[0] = ms2[1] = 0.0f;
    if (hasEnv) HIP_TRY(env.median(0, &ms2[0]));
    if (count) HIP_TRY(cls.median(0, &ms2[1]));
    return count ? prt_hip_update_textures(c, count, updates, nullptr) : PRT_HIP_OK;
}
#endif

} // extern "C"
