// prt_rowtests_env.hip -- the row-level entry of environment-light sampling (prt_hip_test_env_sample, include/prt_hip_test.h): a batch
// of the caller's draws through env_sample / cdf_find (prt_device.h) on the uploaded scene's own tables.  A translation unit of the
// TEST build alone (prt_amd/_build.py TEST_SOURCES): the product library is not built from it, so it is no part of the stamp of the
// product's kernel sources either (prt_hip_source_sha16), and the frame kernel's translation unit holds the same code in both builds.
#include <algorithm>
#include <string>

#include "prt_internal.h"
#include "../../include/prt_hip_test.h"

// InfiniteAreaLight::sample (light.cpp:86-128) on the uploaded scene's own tables, texels and `first` constants.  u: {u.x, u.y} per
// draw; out: 8 words per draw (include/prt_hip_test.h).  A grid-stride loop: any grid covers any n.
template <bool COUNT>
__global__ __launch_bounds__(256) void env_sample_kernel(DevScene sc, uint32_t n, const float* u, uint32_t* out)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        uint32_t* q = out + 8 * (size_t)r;
        Traffic tr{};
        Vec3 dir, color;
        env_sample<COUNT>(sc, u[2 * (size_t)r], u[2 * (size_t)r + 1], dir, color, tr);
        q[0] = asu(dir.x); q[1] = asu(dir.y); q[2] = asu(dir.z);
        q[3] = asu(color.x); q[4] = asu(color.y); q[5] = asu(color.z);
        q[6] = COUNT ? tr.nTap : 0u;
        q[7] = 0u;
    }
}

extern "C" int prt_hip_test_env_sample(prt_hip_ctx* c, uint32_t n, const float* u, uint32_t* out, int counting, uint32_t blocks)
{
    if (!c || !u || !out || n == 0) return prt_fail(PRT_HIP_EINVAL, "bad argument");
    if (!c->haveScene) return prt_fail(PRT_HIP_ESTATE, "upload a scene first");
    if (!c->sc.hasEnv || c->sc.envW <= 0 || c->sc.envH <= 0) return prt_fail(PRT_HIP_ESTATE, "env_sample: the scene has no environment map");
    // a draw is a generator output, in [0, 1): only then is every index the search and the tap form inside the map's arrays
    for (size_t k = 0; k < 2 * (size_t)n; k++)
        if (!(u[k] >= 0.0f && u[k] < 1.0f)) return prt_fail(PRT_HIP_EINVAL, "env_sample: a draw outside [0, 1)");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> din;
    DevBuf<uint32_t> dout;
    HIP_TRY(din.fit((size_t)n * 2, c->stream));
    HIP_TRY(dout.fit((size_t)n * 8, c->stream));
    HIP_TRY(hipMemcpy(din, u, (size_t)n * 8, hipMemcpyHostToDevice));
    // the caller's workgroups, or one thread per draw; at most 65535 (as prt_hip_test_taps)
    blocks = std::min<uint32_t>(blocks ? blocks : (n + 255u) / 256u, 65535u);
    if (counting) hipLaunchKernelGGL(env_sample_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, c->sc, n, din, dout);
    else hipLaunchKernelGGL(env_sample_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, c->sc, n, din, dout);
    int rc = prt_launched("env_sample_kernel");
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 32, hipMemcpyDeviceToHost));
    return PRT_HIP_OK;
}
