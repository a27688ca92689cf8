// prt_batch.h -- the shell of a "ray batch" kernel: one ray per lane through trace_loop (prt_device.h), behind a ray source and a hit
// sink of the kernel's own.  gbuffer_kernel (prt_kernels.hip), position_kernel (prt_temporal.hip), query_nearest_kernel and
// query_any_kernel (prt_query.hip) and the test build's rays_kernel (prt_rowtests.hip) are each: make the source, call trace_batch.
// The host half is prt_batch_begin / prt_batch_end (prt_internal.h, prt_context.hip).
#pragma once
#include "prt_device.h"

// Workgroups launched per CU by the G-buffer and the position guide.  A workgroup is PRT_BLOCK = 1024 threads = 16 waves, and a CU
// runs as many at a time as the kernel's registers admit: two of position_kernel (74 VGPRs, 70 KB of LDS each), one of gbuffer_kernel
// (128 VGPRs: 4 waves per SIMD).  The others start as those end; no workgroup waits for another one.
#define PRT_BATCH_BLOCKS_PER_CU 4

// What a launch hands every batch kernel, filled by prt_batch_begin: the last member of the kernel's argument struct.
struct BatchCtl {
    uint32_t* cursor;            // the claim cursor (the context's control words, cleared for the launch)
    uint32_t* spill;             // spill columns of the traversal stacks
    uint32_t spillStride;        // threads the columns were sized for
    unsigned long long* counters; // the statistics (cleared for the launch, prt_stats.h)
};

// The body of a batch kernel.  Src: count(), cursor() (= ctl.cursor), load(), store_hit(), store_occ() as trace_loop asks for them.
// Only the packet traversal stores entry distances: half as many LDS entries, a distance with each; the other modes keep one row.
template <int MODE, class Src>
__device__ __forceinline__ void trace_batch(const DevScene& sc, Src& src, const BatchCtl& ctl)
{
    constexpr int NLDS = (MODE == PRT_MODE_PACKET) ? PRT_STACK_LDS_PACKET : PRT_STACK_LDS;
    __shared__ uint32_t ldsRef[NLDS * PRT_BLOCK];
    __shared__ float ldsT[(MODE == PRT_MODE_PACKET ? NLDS : 1) * PRT_BLOCK];
    const uint32_t tid = threadIdx.x;
    __shared__ uint32_t coopTbl[(PRT_BLOCK / 64) * PRT_COOP_STRIDE];
    const StackT<NLDS> st{(lds_u32*)&ldsRef[tid], (lds_f32*)&ldsT[tid], ctl.spill, ctl.spillStride, nullptr,
                          (lds_u32*)&coopTbl[(tid >> 6) * PRT_COOP_STRIDE]};
    Traffic tr{};
    uint32_t overflow = 0;
    trace_loop<MODE, false>(sc, src, st, tr, overflow);
    if (overflow) atomicAdd(&ctl.counters[PRT_STAT_STACK_OVERFLOW], 1ull);
}
