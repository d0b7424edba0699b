// sydelta_stage.hpp — the pinned staging ring of the calls that upload host tables in pieces
// (sydelta_apply_delta_device and the five batch calls).  It includes only the HIP runtime API
// and the standard library, so a host program can include it alone (tests/csrc/stage_check.cpp
// drives it against recording stand-ins of the HIP calls).
//
// The protocol, once: use number k of a call takes slot k % slots.  The host may write a slot
// only after the slot's previous upload has landed, so acquire(k) waits for the event that
// uploaded(k - slots) recorded; the first `slots` uses of a call wait for nothing, because every
// call drains its stream before it returns.  A user fills the slot, queues its copies, and calls
// uploaded(k, stream).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

namespace sydelta {

// One per entry point and thread (thread_local): the pinned bytes are freed with the thread,
// the per-device events and copy stream are never destroyed (like thread_stream).
class StageRing {
public:
    explicit StageRing(uint32_t slots) : slots_(slots) {}
    ~StageRing() {
        if (p_) (void)hipHostFree(p_);
    }
    StageRing(const StageRing&) = delete;
    StageRing& operator=(const StageRing&) = delete;

    // The start of a call on `device`: the ring holds at least `bytes` in all (slots of
    // bytes / slots; it grows only here, where nothing is in flight) and the device's events exist.
    hipError_t open(int device, size_t bytes) {
        if (bytes > bytes_) {
            if (p_) (void)hipHostFree(p_);
            p_ = nullptr, bytes_ = 0;
            if (hipError_t e = hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault)) return p_ = nullptr, e;
            bytes_ = bytes;
        }
        dev_ = &devs_[device];
        dev_->up.resize(slots_, nullptr);
        for (hipEvent_t& ev : dev_->up)
            if (!ev)
                if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) return e;
        return hipSuccess;
    }
    uint8_t* base() const { return p_; }
    size_t slot_bytes() const { return bytes_ / slots_; }

    // The slot of use k, once its previous upload (use k - slots) has landed.
    hipError_t acquire(uint64_t k, void** slot) {
        const uint32_t i = (uint32_t)(k % slots_);
        if (k >= slots_)
            if (hipError_t e = hipEventSynchronize(dev_->up[i])) return e;
        *slot = p_ + i * slot_bytes();
        return hipSuccess;
    }
    // The copies of use k are queued on `s`; `waiter`, if any, runs on only after them.
    hipError_t uploaded(uint64_t k, hipStream_t s, hipStream_t waiter = nullptr) {
        const hipEvent_t ev = dev_->up[k % slots_];
        if (hipError_t e = hipEventRecord(ev, s)) return e;
        return waiter ? hipStreamWaitEvent(waiter, ev, 0) : hipSuccess;
    }
    // n elements of src to d_dst, a slot at a time; *k counts the call's uses.
    template <class T>
    hipError_t upload(const T* src, size_t n, T* d_dst, uint64_t* k, hipStream_t s) {
        const size_t per = slot_bytes() / sizeof(T);
        for (size_t i0 = 0; i0 < n; i0 += per, ++*k) {
            const size_t m = std::min(per, n - i0);
            void* h;
            if (hipError_t e = acquire(*k, &h)) return e;
            std::copy(src + i0, src + i0 + m, (T*)h);
            if (hipError_t e = hipMemcpyAsync(d_dst + i0, h, m * sizeof(T), hipMemcpyHostToDevice, s)) return e;
            if (hipError_t e = uploaded(*k, s)) return e;
        }
        return hipSuccess;
    }
    // The device's copy stream (made on first use), ordered behind what `after` holds now.
    hipError_t copy_stream(hipStream_t after, hipStream_t* cs) {
        if (!dev_->copy)
            if (hipError_t e = hipStreamCreateWithFlags(&dev_->copy, hipStreamNonBlocking)) return e;
        if (!dev_->ready)
            if (hipError_t e = hipEventCreateWithFlags(&dev_->ready, hipEventDisableTiming)) return e;
        *cs = dev_->copy;
        if (hipError_t e = hipEventRecord(dev_->ready, after)) return e;
        return hipStreamWaitEvent(dev_->copy, dev_->ready, 0);
    }

private:
    struct Dev {
        std::vector<hipEvent_t> up;
        hipStream_t copy = nullptr;
        hipEvent_t ready = nullptr;
    };
    const uint32_t slots_;
    uint8_t* p_ = nullptr;
    size_t bytes_ = 0;
    std::map<int, Dev> devs_;
    Dev* dev_ = nullptr;
};

}  // namespace sydelta
