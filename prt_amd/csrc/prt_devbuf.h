// prt_devbuf.h -- the one owner of a device allocation: `n` elements of T, freed with the object.  The count is zero whenever the
// pointer is null.  Includes nothing of the project (tests/devbuf_main.cpp compiles it for the CPU against a counting allocator).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

template <typename T> class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // Moving hands the memory over and leaves the source empty.  Assignment frees what the target held WITHOUT synchronising: as with
    // release(), the caller answers for the stream that used that memory being idle.
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            swap(o);
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T*() const { return p_; }
    T* operator->() const { return p_; } // for the address of a field on the device
    size_t size() const { return n_; } // elements

    void release()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    void swap(DevBuf& o) noexcept // the two exchange their memory (history and pending records, prt_temporal.hip)
    {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
    // Exactly n elements (fit) or at least n (grow).  Memory that already serves is kept.  Otherwise `stream`, which may still be using
    // the old memory, is synchronised, the old memory is freed and new memory of undefined contents takes its place; when that fails the
    // buffer is empty.  *fresh is set when the old contents are gone, whether or not the new memory came, and is left alone when the
    // memory is kept, so that one flag can serve several buffers.  n == 0 still yields a pointer.
    hipError_t fit(size_t n, hipStream_t stream, bool* fresh = nullptr) { return p_ && n_ == n ? hipSuccess : remake(n, stream, fresh); }
    hipError_t grow(size_t n, hipStream_t stream, bool* fresh = nullptr) { return p_ && n_ >= n ? hipSuccess : remake(n, stream, fresh); }

private:
    hipError_t remake(size_t n, hipStream_t stream, bool* fresh)
    {
        if (p_) {
            hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            release();
        }
        if (fresh) *fresh = true;
        hipError_t e = hipMalloc((void**)&p_, n * sizeof(T) > 64 ? n * sizeof(T) : 64); // (never fewer than 64 bytes)
        if (e == hipSuccess) n_ = n;
        else p_ = nullptr;
        return e;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};
