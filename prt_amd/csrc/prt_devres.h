// prt_devres.h -- the owners of the two other kinds of HIP resource, beside DevBuf (prt_devbuf.h): an event, pinned host memory, and the
// events and samples of a profile call.  Every hipEventCreate / hipEventDestroy / hipHostMalloc / hipHostFree of the library is in
// this file.  Includes nothing of the project (tests/devres_main.cpp compiles it for the CPU against counting fakes).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// One event, destroyed with the object.  Null until make() and after a failed make().
class DevEvent {
public:
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept { std::swap(e_, o.e_); }
    DevEvent& operator=(DevEvent&& o) noexcept
    {
        if (this != &o) {
            release();
            std::swap(e_, o.e_);
        }
        return *this;
    }
    ~DevEvent() { release(); }

    operator hipEvent_t() const { return e_; }

    // Creates the event on first use; an event that exists is kept, whatever its flags.
    hipError_t make(unsigned flags = hipEventDefault)
    {
        if (e_) return hipSuccess;
        hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    void release()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

// Pinned host memory, `n` elements of T, with DevBuf's vocabulary; the count is zero whenever the pointer is null.  It takes no
// stream: the call sites allocate once and keep the memory, and the caller answers for no copy into it being in flight when it is
// remade, released, moved onto or destroyed.
template <typename T> class HostBuf {
public:
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    HostBuf(HostBuf&& o) noexcept { swap(o); }
    HostBuf& operator=(HostBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            swap(o);
        }
        return *this;
    }
    ~HostBuf() { release(); }

    operator T*() const { return p_; }
    size_t size() const { return n_; } // elements

    void release()
    {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // Exactly n elements: memory of that size is kept, else the old memory is freed and new memory of undefined contents takes its
    // place; when that fails the buffer is empty.  n == 0 still yields a pointer.
    hipError_t fit(size_t n)
    {
        if (p_ && n_ == n) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T) > 64 ? n * sizeof(T) : 64, hipHostMallocDefault); // (as DevBuf: never fewer than 64 bytes)
        if (e == hipSuccess) n_ = n;
        else p_ = nullptr;
        return e;
    }

private:
    void swap(HostBuf& o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};

// The scaffold of a profile call: `stages` intervals between stages + 1 events on a stream, over any number of repetitions.  A
// repetition is stages + 1 calls of mark() around the queued work, a synchronisation of the stream by the caller, and one lap(),
// which takes the repetition's elapsed times into the samples of their stages.  The events are created by the first repetition's
// marks and destroyed with the timer, wherever the caller returns.
class StageTimer {
public:
    explicit StageTimer(uint32_t stages) : ev_(stages + 1), ms_(stages) {}

    // Records the next event of the repetition on s.  One mark too many is refused here and again by lap().
    hipError_t mark(hipStream_t s)
    {
        if (next_ >= ev_.size()) {
            next_ = ev_.size() + 1;
            return hipErrorInvalidValue;
        }
        hipError_t e = ev_[next_].make();
        if (e == hipSuccess) e = hipEventRecord(ev_[next_], s);
        if (e == hipSuccess) next_++;
        return e;
    }
    // After the stream has been synchronised: one sample per stage, and the next mark is the first of a repetition again.  discard
    // only rewinds (a warm-up repetition).  A repetition that did not mark exactly stages + 1 events gives no sample and is an error.
    hipError_t lap(bool discard = false)
    {
        const size_t marked = next_;
        next_ = 0;
        if (marked != ev_.size()) return hipErrorInvalidValue;
        if (discard) return hipSuccess;
        for (size_t k = 0; k < ms_.size(); k++) {
            float ms = 0.0f;
            hipError_t e = hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]);
            if (e != hipSuccess) return e;
            ms_[k].push_back(ms);
        }
        return hipSuccess;
    }
    // *ms = sorted[size / 2] of the stage's samples; an error without one.
    hipError_t median(uint32_t stage, float* ms) const
    {
        if (stage >= ms_.size() || ms_[stage].empty()) return hipErrorInvalidValue;
        std::vector<float> sorted = ms_[stage];
        std::sort(sorted.begin(), sorted.end());
        *ms = sorted[sorted.size() / 2];
        return hipSuccess;
    }

private:
    std::vector<DevEvent> ev_;
    std::vector<std::vector<float>> ms_;
    size_t next_ = 0; // event of the next mark
};
