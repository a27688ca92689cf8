// prt_context.hip -- the context behind the C-ABI handle (include/prt_hip.h): its lifetime, the last-error string, the camera, the
// scaffold every entry point shares and the host half of a batch launch (prt_internal.h), and what reads a context back: download, statistics and the sticky error
// words.  Host code only: no kernel is defined or launched here, so that the frame kernels' code objects (prt_kernels.hip) do not
// move when it changes.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "prt_internal.h"

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) { return prt_fail(code, msg); }
} // namespace
int prt_fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
const std::string& prt_last_error_string() { return g_err; }

// ============================================================================ the scaffold of an entry point
int prt_check_rect(const prt_hip_ctx* c, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    const uint32_t W = c->cam.width, H = c->cam.height;
    if (x1 < x0 || y1 < y0 || x1 >= W || y1 >= H) return fail(PRT_HIP_EINVAL, "pixel rectangle outside the image");
    return PRT_HIP_OK;
}

int prt_stream_enter(prt_hip_ctx* c, void* stream, hipStream_t* out)
{
    hipStream_t s = c->stream;
    hipStream_t caller = (stream && (hipStream_t)stream != c->stream) ? (hipStream_t)stream : nullptr;
    *out = caller;
    if (caller) {
        HIP_TRY(hipEventRecord(c->evIn, caller));
        HIP_TRY(hipStreamWaitEvent(s, c->evIn, 0));
    }
    return PRT_HIP_OK;
}

int prt_stream_leave(prt_hip_ctx* c, hipStream_t caller)
{
    hipStream_t s = c->stream;
    if (caller) {
        HIP_TRY(hipEventRecord(c->evOut, s));
        HIP_TRY(hipStreamWaitEvent(caller, c->evOut, 0));
    }
    return PRT_HIP_OK;
}

// The two halves of prt_run_io around its launch.
int prt_io_begin(prt_hip_ctx* c, uint32_t flags, void* stream, const std::string& alignmentMessage, PrtIoArray* io, uint32_t count, hipStream_t* caller)
{
    HIP_TRY(hipSetDevice(c->device));
    *caller = nullptr;
    if (flags & PRT_HIP_QUERY_HOST) {
        HIP_TRY(c->stage.place(io, count, c->stream));
        return PRT_HIP_OK;
    }
    if (!prt_io_on_device(io, count)) return fail(PRT_HIP_EINVAL, alignmentMessage);
    return prt_stream_enter(c, stream, caller);
}

int prt_io_end(prt_hip_ctx* c, uint32_t flags, const PrtIoArray* io, uint32_t count, hipStream_t caller)
{
    if (flags & PRT_HIP_QUERY_HOST) {
        HIP_TRY(c->stage.fetch(io, count, c->stream));
        return PRT_HIP_OK;
    }
    return prt_stream_leave(c, caller);
}

int prt_check_flags(uint32_t flags, const char* what)
{
    if (flags & ~PRT_HIP_QUERY_HOST) return fail(PRT_HIP_EINVAL, std::string(what) + ": unknown flag bits");
    return PRT_HIP_OK;
}

int prt_own_framebuffer(prt_hip_ctx* c, float** d_rgb)
{
    if (*d_rgb) return PRT_HIP_OK;
    const size_t n = (size_t)c->cam.width * c->cam.height;
    bool fresh = false;
    HIP_TRY(c->fb.fit(n * 3, c->stream, &fresh));
    if (fresh) HIP_TRY(hipMemsetAsync(c->fb, 0, n * 3 * sizeof(float), c->stream));
    *d_rgb = c->fb;
    return PRT_HIP_OK;
}

int prt_launched(const char* kernel)
{
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(PRT_HIP_ELAUNCH, std::string(kernel) + " launch: " + hipGetErrorString(le));
    return PRT_HIP_OK;
}

// Per-thread spill columns of the traversal stacks (entries beyond those kept in LDS): [entry][thread], two words per entry.
int prt_launch_resources(prt_hip_ctx* c, uint32_t blocks)
{
    HIP_TRY(c->spill.grow((size_t)blocks * PRT_BLOCK * 2 * (PRT_STACK_MAX - PRT_STACK_LDS_PACKET), c->stream));
    return PRT_HIP_OK;
}

// Folds the recorded launches of the timing ring into the context's totals (waits for them: they were queued long ago).
static void fold_timing(prt_hip_ctx* c)
{
    for (uint32_t i = 0; i < c->ringUsed; i++) {
        float ms = 0.0f;
        if (hipEventSynchronize(c->evT1[i]) == hipSuccess && hipEventElapsedTime(&ms, c->evT0[i], c->evT1[i]) == hipSuccess) {
            c->lastMs = ms;
            c->accMs += ms;
            c->accLaunches++;
        }
    }
    c->ringUsed = 0;
}

int prt_timing_pair(prt_hip_ctx* c, hipEvent_t* ev0, hipEvent_t* ev1)
{
    if (c->ringUsed == PRT_TIMING_RING) fold_timing(c);
    HIP_TRY(c->evT0[c->ringUsed].make());
    HIP_TRY(c->evT1[c->ringUsed].make());
    *ev0 = c->evT0[c->ringUsed];
    *ev1 = c->evT1[c->ringUsed];
    c->ringUsed++;
    return PRT_HIP_OK;
}

int prt_batch_begin(prt_hip_ctx* c, uint64_t items, uint32_t resident, bool timed, BatchLaunch* L)
{
    hipStream_t s = c->stream;
    int rc = prt_launch_resources(c, resident);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->counters, 0, PRT_STAT_SHARDS * PRT_STAT_STRIDE * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(c->work, 0, PRT_WORK_WORDS * sizeof(uint32_t), s));
    L->ctl = BatchCtl{c->work, c->spill, c->spillThreads(), c->counters};
    L->blocks = (uint32_t)std::min<uint64_t>((items + PRT_BLOCK - 1) / PRT_BLOCK, resident);
    L->ev1 = nullptr;
    if (timed) {
        hipEvent_t ev0;
        if ((rc = prt_timing_pair(c, &ev0, &L->ev1))) return rc;
        HIP_TRY(hipEventRecord(ev0, s));
    }
    return PRT_HIP_OK;
}

int prt_batch_end(prt_hip_ctx* c, const BatchLaunch& L, const char* kernel)
{
    int rc = prt_launched(kernel);
    if (rc) return rc;
    if (L.ev1) HIP_TRY(hipEventRecord(L.ev1, c->stream));
    return PRT_HIP_OK;
}

// Errors of launches since the last prt_hip_get_stats.  Every render clears its own control words and counters, so a watchdog
// abort or a stack overflow of an EARLIER frame of an asynchronous sequence (bench steps, render + gather loops) would be gone by
// the time anybody looks; the frame kernel therefore also ORs them into words no render clears.
int prt_sticky_error(prt_hip_ctx* c, bool clear)
{
    uint32_t S[PRT_STICKY_WORDS] = {0};
    if (!c->work) return PRT_HIP_OK;
    HIP_TRY(hipMemcpy(S, c->work + PRT_WORK_WORDS, sizeof(S), hipMemcpyDeviceToHost));
    if (S[0] == 0) return PRT_HIP_OK;
    if (clear) HIP_TRY(hipMemset(c->work + PRT_WORK_WORDS, 0, sizeof(S)));
    if (S[0] & 1u) {
        std::string msg = "frame kernel: scheduler watchdog fired in a launch since the last prt_hip_get_stats (a workgroup waited for work that never came; its image is incomplete);";
        for (uint32_t k = 0; k < std::min<uint32_t>(S[2], 8u); k++) {
            const uint32_t* D = S + 8 + 16 * k;
            char line[256];
            snprintf(line, sizeof(line), " [block %u wave %u: ready %u live %u exhausted %u lock %u, %u groups wait for %u rays, tails %u %u %u %u heads %u %u %u %u]",
                     D[0], D[1], D[2], D[3], D[4], D[5], D[6], D[7], D[8], D[9], D[10], D[11], D[12], D[13], D[14], D[15]);
            msg += line;
        }
        return fail(PRT_HIP_ELAUNCH, msg);
    }
    return fail(PRT_HIP_ESTACK, "BVH traversal needed more than 64 stack entries in a launch since the last prt_hip_get_stats (the reference asserts here, bvh.cpp:552)");
}

extern "C" {

const char* prt_hip_last_error(void) { return g_err.c_str(); }

#ifndef PRT_SOURCE_SHA16
#define PRT_SOURCE_SHA16 "unstamped"
#endif
const char* prt_hip_source_sha16(void) { return PRT_SOURCE_SHA16; }

int prt_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int create_resources(prt_hip_ctx* c)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->computeUnits = prop.multiProcessorCount;
    c->name = prop.name[0] ? prop.name : prop.gcnArchName;
    HIP_TRY(hipStreamCreate(&c->stream));
    HIP_TRY(c->evIn.make(hipEventDisableTiming));
    HIP_TRY(c->evOut.make(hipEventDisableTiming));
    HIP_TRY(c->work.fit(PRT_WORK_WORDS + PRT_STICKY_WORDS, c->stream));
    HIP_TRY(hipMemset(c->work, 0, (PRT_WORK_WORDS + PRT_STICKY_WORDS) * sizeof(uint32_t)));
    HIP_TRY(c->counters.fit(PRT_STAT_SHARDS * PRT_STAT_STRIDE, c->stream));
    HIP_TRY(hipMemset(c->counters, 0, PRT_STAT_SHARDS * PRT_STAT_STRIDE * sizeof(unsigned long long)));
    return PRT_HIP_OK;
}

// The library touches neither the process environment nor the HIP runtime's configuration: a render is one kernel on one
// stream of the context.
int prt_hip_create(int device, prt_hip_ctx** out)
{
    if (!out) return fail(PRT_HIP_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(PRT_HIP_ENODEVICE, "no HIP device: libprt_hip has no CPU path (the GPU kernels are the product)");
    if (device < 0 || device >= n) return fail(PRT_HIP_EINVAL, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    prt_hip_ctx* c = new prt_hip_ctx();
    c->device = device;
    int rc = create_resources(c);
    if (rc != PRT_HIP_OK) {
        std::string why = prt_last_error_string(); // prt_hip_destroy makes HIP calls of its own
        prt_hip_destroy(c);      // frees whatever was created before the failure
        return fail(rc, why);
    }
    *out = c;
    return PRT_HIP_OK;
}

void prt_hip_destroy(prt_hip_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    prt_free_scene(c);
    prt_gather_release(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // frees the context's buffers, events and pinned memory (DevBuf, DevEvent, HostBuf)
}

int prt_hip_device_info(prt_hip_ctx* c, char* name, size_t cap, int* computeUnits)
{
    if (!c) return fail(PRT_HIP_EINVAL, "ctx is NULL");
    if (name && cap) {
        strncpy(name, c->name.c_str(), cap - 1);
        name[cap - 1] = 0;
    }
    if (computeUnits) *computeUnits = c->computeUnits;
    return PRT_HIP_OK;
}

int prt_hip_set_camera(prt_hip_ctx* c, const prt_camera_desc* cam)
{
    if (!c || !cam) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (cam->width == 0 || cam->height == 0) return fail(PRT_HIP_EINVAL, "empty image");
    static_assert(sizeof(DevCamera) == sizeof(prt_camera_desc), "camera layouts must match");
    prt_temporal_camera_change(c, cam); // before the view goes: a pending record becomes the history
    memcpy(&c->cam, cam, sizeof(DevCamera));
    c->haveCamera = true;
    prt_accum_forget(c); // of another view (and perhaps another size)
    prt_denoise_forget(c);
    return PRT_HIP_OK;
}

float* prt_hip_framebuffer(prt_hip_ctx* c) { return c ? (float*)c->fb : nullptr; }

int prt_hip_download(prt_hip_ctx* c, float* rgb_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (!c || !rgb_host) return fail(PRT_HIP_EINVAL, "NULL argument");
    const uint32_t W = c->cam.width;
    if (!c->fb || c->fb.size() != (size_t)W * c->cam.height * 3) return fail(PRT_HIP_ESTATE, "nothing rendered into the context framebuffer");
    int rc = prt_check_rect(c, x0, y0, x1, y1);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    size_t rowBytes = (size_t)(x1 - x0 + 1) * 3 * sizeof(float);
    size_t off = ((size_t)y0 * W + x0) * 3;
    HIP_TRY(hipMemcpy2D(rgb_host + off, (size_t)W * 3 * sizeof(float), c->fb + off, (size_t)W * 3 * sizeof(float), rowBytes,
                        y1 - y0 + 1, hipMemcpyDeviceToHost));
    return prt_sticky_error(c, false); // the pixels are delivered, but a caller must learn that a launch behind them was cut short
}

// The mirror of prt_hip_download; ordered on the context's stream behind the work queued there.
int prt_hip_upload(prt_hip_ctx* c, const float* rgb_host, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    if (!c || !rgb_host) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (!c->haveCamera) return fail(PRT_HIP_ESTATE, "set a camera first");
    const uint32_t W = c->cam.width;
    int rc = prt_check_rect(c, x0, y0, x1, y1);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    float* fb = nullptr;
    if ((rc = prt_own_framebuffer(c, &fb))) return rc;
    size_t rowBytes = (size_t)(x1 - x0 + 1) * 3 * sizeof(float);
    size_t off = ((size_t)y0 * W + x0) * 3;
    HIP_TRY(hipMemcpy2DAsync(fb + off, (size_t)W * 3 * sizeof(float), rgb_host + off, (size_t)W * 3 * sizeof(float), rowBytes, y1 - y0 + 1,
                             hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the caller's array is free again on return
    return PRT_HIP_OK;
}

int prt_hip_get_stats(prt_hip_ctx* c, prt_hip_stats* st)
{
    if (!c || !st) return fail(PRT_HIP_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long h[PRT_STAT_STRIDE] = {0};
    {
        std::vector<unsigned long long> all((size_t)PRT_STAT_SHARDS * PRT_STAT_STRIDE);
        HIP_TRY(hipMemcpy(all.data(), c->counters, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int sh = 0; sh < PRT_STAT_SHARDS; sh++)
            for (int k = 0; k < PRT_STAT_STRIDE; k++) h[k] += all[(size_t)sh * PRT_STAT_STRIDE + k];
    }
    // errors of ANY launch since the last call (the last one included): see prt_sticky_error
    const int sticky = prt_sticky_error(c, true);
    prt_profile_report(h); // (the profile build only, prt_stats.h)
    st->raysTraced = h[PRT_STAT_RAYS];
    st->occludedTraced = h[PRT_STAT_OCCL];
    st->nBox = h[PRT_STAT_BOX];
    st->nTri = h[PRT_STAT_TRI];
    st->nHit = h[PRT_STAT_HIT];
    st->nTap = h[PRT_STAT_TAP];
    st->nPx = h[PRT_STAT_PIXELS];
    for (int m = 0; m < PRT_STAT_MODES; m++) { // (0 in the profile build, whose loop statistics overlay these words)
        st->modeBox[m] = prt_stat_mode_words_valid ? h[prt_stat_mode(m, PRT_STAT_MODE_BOX)] : 0;
        st->modeTri[m] = prt_stat_mode_words_valid ? h[prt_stat_mode(m, PRT_STAT_MODE_TRI)] : 0;
        st->modeTap[m] = prt_stat_mode_words_valid ? h[prt_stat_mode(m, PRT_STAT_MODE_TAP)] : 0;
    }
    st->stackOverflow = h[PRT_STAT_STACK_OVERFLOW];
    fold_timing(c);
    st->kernelMs = c->accLaunches ? c->lastMs : 0.0;
    st->kernelMsSum = c->accMs;
    st->kernelLaunches = c->accLaunches;
    c->accMs = c->lastMs = 0.0;
    c->accLaunches = 0;
    if (sticky) return sticky;
    if (h[PRT_STAT_STACK_OVERFLOW]) return fail(PRT_HIP_ESTACK, "BVH traversal needed more than 64 stack entries (the reference asserts here, bvh.cpp:552)");
    return PRT_HIP_OK;
}

} // extern "C"
