// prt_stage.h -- the arrays of a host-array entry point and the one arena they are staged in.  An entry point lists its arrays in a
// table of PrtIoArray; under PRT_HIP_QUERY_HOST PrtStage gives each a slice of one device allocation and copies it in before and out
// after the launch, otherwise the launch uses the caller's (device) pointers as they are (prt_run_io, prt_internal.h).  Includes
// prt_devbuf.h and nothing else of the project (tests/stage_main.cpp compiles it for the CPU against fakes that copy and log).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "prt_devbuf.h"

enum PrtIoDir { PRT_IO_IN, PRT_IO_OUT, PRT_IO_INOUT }; // IN: copied to the device before the launch; OUT: copied back after it; INOUT: both

// One array of a call.  p == null: the call has no such array, and every step skips it.
struct PrtIoArray {
    void* p;         // the caller's pointer
    size_t bytes;    // an OUT array is copied back at the size this holds AFTER the launch (which may trim it; 0 copies nothing)
    uintptr_t align; // what the kernels load and store it with: a power of two
    PrtIoDir dir;
    void* dev;       // what the launch is to use: the slice of the arena, or p itself on device arrays
    template <typename T> T* as() const { return (T*)dev; }
};
inline PrtIoArray prt_io_in(const void* p, size_t bytes, uintptr_t align) { return PrtIoArray{const_cast<void*>(p), bytes, align, PRT_IO_IN, nullptr}; }
inline PrtIoArray prt_io_out(void* p, size_t bytes, uintptr_t align) { return PrtIoArray{p, bytes, align, PRT_IO_OUT, nullptr}; }
// an array the launch updates in place (an image a lens render adds to): the same slice in both directions
inline PrtIoArray prt_io_inout(void* p, size_t bytes, uintptr_t align) { return PrtIoArray{p, bytes, align, PRT_IO_INOUT, nullptr}; }

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; } // (null is aligned)

// Device arrays: every pointer as the kernels need it?  Then the launch uses the caller's pointers.
inline bool prt_io_on_device(PrtIoArray* io, uint32_t count)
{
    for (uint32_t i = 0; i < count; i++)
        if (!aligned(io[i].p, io[i].align)) return false;
    for (uint32_t i = 0; i < count; i++) io[i].dev = io[i].p;
    return true;
}

// The staging of every host-array call of a context: one allocation, which lives as long as the context and grows to the largest
// call.  One call runs at a time on the context's stream, so the slices of a call are the arena's only tenants.
class PrtStage {
public:
    static constexpr size_t SLICE = 256; // every slice starts at a multiple of it: at least the alignment of any record

    // One grow to the sum of the sizes (memory that already serves is kept; a regrow synchronises `stream` first: DevBuf), a slice
    // for every array in table order, and the copies of the IN and INOUT arrays queued on `stream`.  After an error the arena may be empty.
    hipError_t place(PrtIoArray* io, uint32_t count, hipStream_t stream)
    {
        size_t total = 0;
        for (uint32_t i = 0; i < count; i++)
            if (io[i].p) total += rounded(io[i].bytes);
        hipError_t e = arena_.grow(total, stream);
        if (e != hipSuccess) return e;
        size_t at = 0;
        for (uint32_t i = 0; i < count; i++) {
            io[i].dev = io[i].p ? arena_ + at : nullptr;
            if (io[i].p) at += rounded(io[i].bytes);
        }
        for (uint32_t i = 0; i < count; i++)
            if (io[i].p && io[i].dir != PRT_IO_OUT && io[i].bytes) {
                e = hipMemcpyAsync(io[i].dev, io[i].p, io[i].bytes, hipMemcpyHostToDevice, stream);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    }
    // The copies of the OUT and INOUT arrays, then the wait for them: the answers are in the caller's memory on return.
    hipError_t fetch(const PrtIoArray* io, uint32_t count, hipStream_t stream)
    {
        for (uint32_t i = 0; i < count; i++)
            if (io[i].p && io[i].dir != PRT_IO_IN && io[i].bytes) {
                hipError_t e = hipMemcpyAsync(io[i].p, io[i].dev, io[i].bytes, hipMemcpyDeviceToHost, stream);
                if (e != hipSuccess) return e;
            }
        return hipStreamSynchronize(stream);
    }
    size_t size() const { return arena_.size(); } // bytes

private:
    static size_t rounded(size_t bytes) { return (bytes + SLICE - 1) / SLICE * SLICE; }
    DevBuf<char> arena_;
};
