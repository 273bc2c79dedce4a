// eslam_buf.h -- host-only owners of the HIP resources the context keeps: device and pinned
// buffers, events and the timing rings.  Each frees what it holds when it is reset, assigned
// over or destroyed, so a lifetime is written once, at the member's declaration.  The structs
// kernels take by value (eslam_internal.h) keep raw pointers and are filled from these.  Also
// the Carver, which lays the arrays of one block out in order.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/eslam_gpu.h"        // the error codes

namespace eslam_buf {

enum class Mem { Device, Pinned };

// A move-only buffer of T in device or pinned host memory, with its capacity: in bytes after
// alloc() and grow(), in the caller's units after grow_keep().
template <typename T, Mem M = Mem::Device>
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    template <typename U> U* as() const { return reinterpret_cast<U*>(p_); }
    uint64_t cap() const { return cap_; }

    void reset()
    {
        if (p_) (void)(M == Mem::Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }

    // exactly `bytes`, whatever was held freed first; empty on failure
    hipError_t alloc(uint64_t bytes)
    {
        reset();
        return take(bytes, bytes);
    }
    // ... with the block's address also in `field` (of a struct kernels take by value)
    hipError_t alloc(uint64_t bytes, T** field)
    {
        const hipError_t e = alloc(bytes);
        *field = p_;
        return e;
    }

    // at least `bytes`, contents not kept: nothing to do when they fit; otherwise the stream's
    // work completes, the old block goes first (the peak stays one block) and the new one has a
    // quarter's headroom.  Empty on failure.
    hipError_t grow(uint64_t bytes, hipStream_t stream)
    {
        if (bytes <= cap_) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        return e != hipSuccess ? e : alloc(bytes + bytes / 4 + 4096);
    }

    // at least `bytes`, capacity counted in units of `unit` bytes, contents not kept: the new
    // block exists before the old one goes, so a failed growth leaves the buffer as it was.  A
    // quarter's headroom, or the exact size when the device has no room for that.
    // ESLAM_OK, ESLAM_ERR_OUT_OF_MEMORY, or ESLAM_ERR_HIP with *hip the stream's error.
    int grow_keep(uint64_t bytes, uint64_t unit, hipStream_t stream, hipError_t* hip)
    {
        if (bytes <= cap_ * unit) return ESLAM_OK;
        if ((*hip = hipStreamSynchronize(stream)) != hipSuccess) return ESLAM_ERR_HIP;
        Buf nb;
        uint64_t want = (bytes + bytes / 4 + unit - 1) / unit;
        if (nb.take(want * unit, want) != hipSuccess) {
            (void)hipGetLastError();
            want = (bytes + unit - 1) / unit;
            if (nb.take(want * unit, want) != hipSuccess) {
                (void)hipGetLastError();
                return ESLAM_ERR_OUT_OF_MEMORY;
            }
        }
        *this = std::move(nb);
        return ESLAM_OK;
    }

private:
    // (empty) a new block of `bytes`, recorded with capacity `cap`
    hipError_t take(uint64_t bytes, uint64_t cap)
    {
        void* v = nullptr;
        const hipError_t e = M == Mem::Pinned ? hipHostMalloc(&v, bytes, hipHostMallocDefault) : hipMalloc(&v, bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(v);
        cap_ = cap;
        return hipSuccess;
    }

    T* p_ = nullptr;
    uint64_t cap_ = 0;
};

template <typename T> using Dev = Buf<T, Mem::Device>;
template <typename T> using Pinned = Buf<T, Mem::Pinned>;

// Arrays carved one after another from a block that starts at `base`, each rounded up to `align`
// bytes (hipMalloc's blocks are 256-byte aligned, so every array is).  With a null base it only
// measures: take() returns nullptr and bytes() is the block's size.  A layout is one function
// of a Carver, run once to size the block and once to place the arrays.
class Carver {
public:
    explicit Carver(void* base, uint64_t align = 256) : base_(static_cast<char*>(base)), align_(align) {}

    void* take_bytes(uint64_t bytes)
    {
        void* p = base_ ? base_ + off_ : nullptr;
        off_ += (bytes + align_ - 1) / align_ * align_;
        return p;
    }
    template <class T> T* take(uint64_t count) { return static_cast<T*>(take_bytes(count * sizeof(T))); }
    uint64_t bytes() const { return off_; }     // taken so far

private:
    char* base_;
    uint64_t align_, off_ = 0;
};

// A move-only event, created on first use.
class Event {
public:
    operator hipEvent_t() const { return e_.get(); }
    void reset() { e_.reset(); }
    // nothing to do when the event exists
    hipError_t create(bool timing)
    {
        if (e_) return hipSuccess;
        hipEvent_t e = nullptr;
        const hipError_t r = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
        e_.reset(e);
        return r;
    }

private:
    struct Destroy {
        void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
    };
    std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> e_;
};

// Timing mode: the events of up to kRingSteps recorded steps, `per_step` each, kept in a ring so
// a whole timed region of back-to-back steps is measured without synchronising between steps.
// Timing is diagnostic: the events are created on first use, best effort.
static constexpr uint32_t kRingSteps = 2048;

class EventRing {
public:
    // the event index `closing` ends a step
    EventRing(uint32_t per_step, uint32_t closing) : per_(per_step), closing_(closing) {}

    // event k of the current step
    void record(bool timing, uint32_t k, hipStream_t stream)
    {
        if (!timing) return;
        if (ev_.empty()) {
            ev_.resize((size_t)per_ * kRingSteps);
            for (auto& e : ev_) (void)e.create(true);
        }
        if (steps_ >= kRingSteps) return;
        (void)hipEventRecord(ev_[(size_t)per_ * steps_ + k], stream);
        if (k == closing_) steps_++;
    }

    uint32_t steps() const { return steps_; }   // whole steps recorded
    void clear() { steps_ = 0; }                // the events are kept

    // over the recorded steps: the summed times (ms) from each event to the next and, in
    // acc[per_step - 1], from the first to the last; returns the steps, and the ring starts over
    uint32_t sums(double* acc)
    {
        for (uint32_t j = 0; j < per_; ++j) acc[j] = 0;
        for (uint32_t s = 0; s < steps_; ++s) {
            const Event* e = &ev_[(size_t)per_ * s];
            for (uint32_t j = 0; j < per_; ++j) {
                float ms = 0;
                (void)hipEventElapsedTime(&ms, e[j + 1 < per_ ? j : 0], e[j + 1 < per_ ? j + 1 : j]);
                acc[j] += ms;
            }
        }
        return std::exchange(steps_, 0);
    }

private:
    std::vector<Event> ev_;
    uint32_t per_, closing_, steps_ = 0;
};

}  // namespace eslam_buf
