// prt_lens.hip -- lens renders (include/prt_hip.h "lens renders"): a camera record in, an image of radiance sums out.  What a caller
// wrote around prt_hip_query_radiance on the host for any camera the reference lacks -- one ray per pixel and jitter built in numpy,
// the rays up, the radiances down, a sum, a splitter for images beyond 2^24 rays -- as two kernels around the frame kernel's probe
// launch (prt_frame_probe, as it stands), band by band:
//     lens_rays_kernel        one lane per ray: the arithmetic of prt_lens.h, which a host program compiles too
//     lens_accumulate_kernel  one lane per output float: the K radiances of its pixel summed in order, written or added to the image
// The rays and the per-ray radiances of prt_hip_lens_render live in the context (bkRays, bkRad: the baker's, one call runs at a time)
// and never leave the device.  In a translation unit of its own, as prt_bake.hip is, so that the code objects of every other kernel
// do not move.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "prt_internal.h"
#include "prt_lens.h"

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

#define PRT_LENS_MAX_RAYS (1u << 24) // the probes of one frame-kernel launch (prt_hip_query_radiance)
#define PRT_LENS_MAX_SIDE 8192u
#define PRT_LENS_MAX_K 64u
#define PRT_LENS_BLOCKS_PER_CU 8 // blocks of 256 lanes either kernel is launched with at the most (the baker's): both are grid-stride loops

static_assert(sizeof(prt_lens_desc) == 96 && sizeof(prt_ray) == 32, "record sizes of the lens kernels");

// ============================================================================ rays
struct LensRaysArgs {
    prt_lens_desc d; // by value: uniform over the launch, it stays in scalar registers
    float4* rays;    // 2 x float4 per ray: {org, tMax = 0} {dir, pad = 0}
    uint32_t y0, total; // first row of the band; (y1 - y0) * W * K <= 2^24
};

// Ray r = ((y - y0)*W + x)*K + k.  Consecutive lanes write consecutive rays: a wave writes 2 KB contiguously.  r becomes (x, y, k)
// by two 32-bit divisions with a uniform divisor (some thirty integer instructions each, no table and no second pass, next to
// the two 16-byte stores every ray costs anyway); prt_sincosf (fp64 inside) is called only under the branch of the model that needs
// it, and the model is uniform over the launch, so no wave pays for a branch it does not take.
__global__ __launch_bounds__(256) void lens_rays_kernel(LensRaysArgs A)
{
    const PrtLensFrame f = prt_lens_frame(&A.d);
    const uint32_t W = A.d.width, K = A.d.K;
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < A.total; r += gridDim.x * 256u) {
        const uint32_t p = r / K, k = r - p * K;
        const uint32_t row = p / W, x = p - row * W;
        const PrtLensRay ray = prt_lens_ray(&A.d, &f, x, A.y0 + row, k);
        gst4(A.rays + 2 * (size_t)r, make_float4(ray.org.x, ray.org.y, ray.org.z, 0.0f));
        gst4(A.rays + 2 * (size_t)r + 1, make_float4(ray.dir.x, ray.dir.y, ray.dir.z, asf(0u)));
    }
}

// ============================================================================ accumulate
struct LensAccArgs {
    const float* L; // 3 * pixels * K: the band's radiances
    float* image;   // the band's first row
    uint32_t floats; // 3 * pixels of the band (< 2^26)
    uint32_t K, add;
};

// One lane per output float e = 3*pix + h: S = +0, then S = S + L[3*(pix*K + k) + h] for k = 0 .. K-1.  Lanes 3*pix .. 3*pix + 2
// read the three floats of one radiance, so with K = 1 a wave reads 256 contiguous bytes per trip, and with a larger K its lanes walk
// 22 neighbouring strips of 12*K bytes whose cache lines every trip of the k loop uses again.  (The wave-cooperative layout of
// the baker's reduce would fix another order of the sum than the definition's.)
__global__ __launch_bounds__(256) void lens_accumulate_kernel(LensAccArgs A)
{
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < A.floats; e += gridDim.x * 256u) {
        const uint32_t pix = e / 3u, h = e - 3u * pix;
        const float* l = A.L + (3 * (size_t)pix * A.K + h);
        float S = 0.0f;
        for (uint32_t k = 0; k < A.K; k++) S = S + gld(l + 3 * (size_t)k);
        A.image[e] = A.add ? gld(A.image + e) + S : S;
    }
}

// ============================================================================ host side
// What the three calls ask of the record and the flags.  Refused before anything is queued.
int check_lens(const prt_lens_desc* d, uint32_t flags, const char* what)
{
    int rc = prt_check_flags(flags, what);
    if (rc) return rc;
    const std::string w(what);
    if (d->model > PRT_HIP_LENS_FISHEYE) return fail(PRT_HIP_EINVAL, w + ": unknown lens model");
    if (d->width < 1 || d->width > PRT_LENS_MAX_SIDE || d->height < 1 || d->height > PRT_LENS_MAX_SIDE)
        return fail(PRT_HIP_EINVAL, w + ": width and height must be 1 .. 8192");
    if (d->K < 1 || d->K > PRT_LENS_MAX_K) return fail(PRT_HIP_EINVAL, w + ": K must be 1 .. 64");
    if (d->flags & ~(PRT_HIP_LENS_CENTRE | PRT_HIP_LENS_ACCUMULATE)) return fail(PRT_HIP_EINVAL, w + ": unknown bits in lens->flags");
    if (d->bandRows > d->height) return fail(PRT_HIP_EINVAL, w + ": bandRows must be 0 or 1 .. height");
    if (d->reserved != 0) return fail(PRT_HIP_EINVAL, w + ": lens->reserved must be 0");
    return PRT_HIP_OK;
}

// The band [y0, y1) of the two halves; *rays = (y1 - y0) * W * K
int check_band(const prt_lens_desc* d, uint32_t y0, uint32_t y1, const char* what, uint32_t* rays)
{
    if (y0 >= y1 || y1 > d->height) return fail(PRT_HIP_EINVAL, std::string(what) + ": rows [y0, y1) must be inside the image and not empty");
    const uint64_t n = (uint64_t)(y1 - y0) * d->width * d->K;
    if (n > PRT_LENS_MAX_RAYS) return fail(PRT_HIP_EINVAL, std::string(what) + ": (y1 - y0)*width*K must be at most 2^24");
    *rays = (uint32_t)n;
    return PRT_HIP_OK;
}

// Rows per frame-kernel launch of prt_hip_lens_render: as many as fit 2^24 probes (at least 32: W*K <= 2^19), or bandRows if fewer
uint32_t band_rows(const prt_lens_desc& d)
{
    const uint32_t fit = std::min(d.height, PRT_LENS_MAX_RAYS / (d.width * d.K));
    return d.bandRows ? std::min(d.bandRows, fit) : fit;
}

uint32_t lens_blocks(const prt_hip_ctx* c, uint32_t lanes)
{
    return std::max(1u, std::min((lanes + 255u) / 256u, (uint32_t)std::max(c->computeUnits, 1) * PRT_LENS_BLOCKS_PER_CU));
}

int launch_rays(prt_hip_ctx* c, const prt_lens_desc& d, uint32_t y0, uint32_t y1, prt_ray* rays)
{
    LensRaysArgs A{d, (float4*)rays, y0, (y1 - y0) * d.width * d.K};
    hipLaunchKernelGGL(lens_rays_kernel, dim3(lens_blocks(c, A.total)), dim3(256), 0, c->stream, A);
    return prt_launched("lens_rays_kernel");
}

// band: the first of the `rows` rows of the image the radiances belong to
int launch_accumulate(prt_hip_ctx* c, const prt_lens_desc& d, uint32_t rows, const float* radiance, float* band)
{
    LensAccArgs A{radiance, band, 3u * rows * d.width, d.K, (d.flags & PRT_HIP_LENS_ACCUMULATE) ? 1u : 0u};
    hipLaunchKernelGGL(lens_accumulate_kernel, dim3(lens_blocks(c, A.floats)), dim3(256), 0, c->stream, A);
    return prt_launched("lens_accumulate_kernel");
}

// The image of a call in the table: read as well as written under ACCUMULATE
PrtIoArray io_image(const prt_lens_desc& d, float* p, size_t floats)
{
    return (d.flags & PRT_HIP_LENS_ACCUMULATE) ? prt_io_inout(p, floats * sizeof(float), 4) : prt_io_out(p, floats * sizeof(float), 4);
}

enum { L_RAYS /* lens_rays: written */, L_RADIANCE /* lens_accumulate: read */, L_IMAGE, L_ARRAYS };

// What the three calls share behind their checks.  The record is copied: the caller may reuse it as soon as the call returns.
// rays: lens_rays; radiance: lens_accumulate; params: prt_hip_lens_render, which traces between the two kernels, band by band, its
// rays and their radiances in the context's buffers.  The two halves stage the rows of their band only, so on host arrays too the
// rows outside it are never touched.
int run_lens(prt_hip_ctx* c, const prt_lens_desc* lens, uint32_t y0, uint32_t y1, prt_ray* rays, const float* radiance, float* image,
             const prt_render_params* params, uint32_t flags, void* stream, const char* what)
{
    const prt_lens_desc d = *lens;
    const size_t nRays = (size_t)(y1 - y0) * d.width * d.K;
    float* first = image ? (params ? image : image + 3 * (size_t)y0 * d.width) : nullptr; // the first float the call may touch
    PrtIoArray io[L_ARRAYS] = {prt_io_out(rays, nRays * sizeof(prt_ray), 16), prt_io_in(radiance, 3 * nRays * sizeof(float), 4),
                               io_image(d, first, 3 * (size_t)(y1 - y0) * d.width)};
    return prt_run_io(c, flags, stream, std::string(what) + ": rays must be 16-byte aligned, float arrays 4-byte aligned", io, L_ARRAYS, [&]() {
        if (rays) return launch_rays(c, d, y0, y1, io[L_RAYS].as<prt_ray>());
        float* img = io[L_IMAGE].as<float>(); // the band's first row (the halves) or the image's (the render)
        if (!params) return launch_accumulate(c, d, y1 - y0, io[L_RADIANCE].as<float>(), img);
        const uint32_t rows = band_rows(d), perRow = d.width * d.K;
        int rc;
        HIP_TRY(c->bkRays.grow((size_t)rows * perRow, c->stream));
        HIP_TRY(c->bkRad.grow(3 * (size_t)rows * perRow, c->stream));
        for (uint32_t b0 = 0; b0 < d.height; b0 += rows) { // ascending y; every band is a render launch for prt_hip_get_stats
            const uint32_t b1 = std::min(d.height, b0 + rows);
            prt_render_params p = *params;
            p.seed = params->seed + d.pass * (d.width * d.height * d.K) + b0 * perRow; // probe g under seed + pass*W*H*K + g (uint32 wrap)
            if ((rc = launch_rays(c, d, b0, b1, c->bkRays)) || (rc = prt_frame_probe(c, (b1 - b0) * perRow, c->bkRays, &p, c->bkRad)) ||
                (rc = launch_accumulate(c, d, b1 - b0, c->bkRad, img + 3 * (size_t)b0 * d.width)))
                return rc;
        }
        return PRT_HIP_OK;
    });
}

} // namespace

extern "C" {

int prt_hip_lens_rays(prt_hip_ctx* c, const prt_lens_desc* lens, uint32_t y0, uint32_t y1, prt_ray* rays, uint32_t flags, void* stream)
{
    if (!c || !lens || !rays) return prt_null_argument("lens_rays");
    uint32_t nRays;
    int rc;
    if ((rc = check_lens(lens, flags, "lens_rays")) || (rc = check_band(lens, y0, y1, "lens_rays", &nRays))) return rc;
    return run_lens(c, lens, y0, y1, rays, nullptr, nullptr, nullptr, flags, stream, "lens_rays");
}

int prt_hip_lens_accumulate(prt_hip_ctx* c, const prt_lens_desc* lens, uint32_t y0, uint32_t y1, const float* radiance, float* image,
                            uint32_t flags, void* stream)
{
    if (!c || !lens || !radiance || !image) return prt_null_argument("lens_accumulate");
    uint32_t nRays;
    int rc;
    if ((rc = check_lens(lens, flags, "lens_accumulate")) || (rc = check_band(lens, y0, y1, "lens_accumulate", &nRays))) return rc;
    return run_lens(c, lens, y0, y1, nullptr, radiance, image, nullptr, flags, stream, "lens_accumulate");
}

int prt_hip_lens_render(prt_hip_ctx* c, const prt_lens_desc* lens, const prt_render_params* params, float* image, uint32_t flags, void* stream)
{
    if (!c || !lens || !params || !image) return prt_null_argument("lens_render");
    if (!c->haveScene) return fail(PRT_HIP_ESTATE, "lens_render: upload a scene first");
    int rc;
    if ((rc = check_lens(lens, flags, "lens_render")) || (rc = prt_check_radiance(c, band_rows(*lens) * lens->width * lens->K, params, flags, "lens_render")))
        return rc;
    return run_lens(c, lens, 0, lens->height, nullptr, nullptr, image, params, flags, stream, "lens_render");
}

} // extern "C"
