// prt_select.hip -- the stream compaction of adaptive sampling (prt_hip_render_adaptive, prt_kernels.hip): hipcub's stable
// DeviceSelect::Flagged, in a translation unit of its own so that the frame kernel's (prt_kernels.hip, whose gfx950 assembly
// tools/step_loop_isa.py and the resource tests read) carries no library kernels.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "prt_internal.h"

hipError_t prt_select_flagged(void* temp, size_t& tempBytes, const uint32_t* in, const uint8_t* flags, uint32_t* out, uint32_t* count,
                              uint64_t n, hipStream_t s)
{
    return hipcub::DeviceSelect::Flagged(temp, tempBytes, in, flags, out, count, (int64_t)n, s);
}
