// rtx_mem.hpp -- the owners of everything the library allocates on a device: memory (DeviceBuf), pinned host memory (PinnedBuf),
// the counters kernels write and the host reads back (Counter), events and streams.  Move-only; a destructor releases.  Nothing else in
// csrc/ allocates or frees (rtx_host_alloc / rtx_host_free apart: that memory is the caller's).  DESIGN.md, "Ownership".
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace rtxmem {

// What must have finished before outgrown storage is freed: the caller says it, at the call, because only the caller knows who
// may still read the old storage.
struct BeforeFree {
    enum Kind { kNothing, kStream, kDevice } kind;
    hipStream_t stream;
};
inline BeforeFree nothing() { return {BeforeFree::kNothing, nullptr}; }                 // every reader has been waited for already
inline BeforeFree after_stream(hipStream_t s) { return {BeforeFree::kStream, s}; }      // all readers were queued on this one stream
inline BeforeFree after_device() { return {BeforeFree::kDevice, nullptr}; }             // readers on streams the library does not know

inline void wait(BeforeFree w)
{
    if (w.kind == BeforeFree::kStream) (void)hipStreamSynchronize(w.stream);
    if (w.kind == BeforeFree::kDevice) (void)hipDeviceSynchronize();
}

// `Pinned`: host memory of hipHostMalloc (hipHostMallocDefault) instead of device memory.  Capacities are in elements of T.
template <class T, bool Pinned>
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            release();
            swap(o);
        }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }

    T* get() const { return p_; }
    size_t capacity() const { return cap_; }

    // Room for n elements.  Within the capacity: no call at all.  Outgrown: the wait, the free, then exactly n elements, contents
    // not kept.  A failed allocation leaves the buffer empty (capacity 0) and HIP's last error cleared; the caller decides what
    // it means.
    hipError_t reserve(size_t n, BeforeFree w)
    {
        if (n <= cap_) return hipSuccess;
        if (p_) wait(w);
        release();
        void* raw = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&raw, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&raw, n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e;
        }
        p_ = static_cast<T*>(raw);
        cap_ = n;
        return hipSuccess;
    }

    // ... with the capacity doubled from `floor` (or from what the buffer holds) until it covers n.
    hipError_t reserve_doubling(size_t n, size_t floor, BeforeFree w)
    {
        if (n <= cap_) return hipSuccess;
        size_t cap = cap_ ? cap_ : floor;
        while (cap < n) cap *= 2;
        return reserve(cap, w);
    }

    // Takes the storage of `fresh` (which is left empty) in place of its own, which is freed after the wait: grow-by-copy, where
    // the new array exists before the old one goes.
    void adopt(Buf&& fresh, BeforeFree w)
    {
        if (p_) wait(w);
        *this = std::move(fresh);
    }

    void release()
    {
        if (p_) (void)(Pinned ? hipHostFree((void*)p_) : hipFree((void*)p_));
        p_ = nullptr;
        cap_ = 0;
    }

    void swap(Buf& o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T>
using DeviceBuf = Buf<T, false>;
template <class T>
using PinnedBuf = Buf<T, true>;

// n words of device memory -> the host, after everything queued on the device: the one place the library reads counters back.
template <class T>
hipError_t read_words(int device, const T* d_src, size_t n, T* out)
{
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e != hipSuccess ? e : hipMemcpy(out, d_src, n * sizeof(T), hipMemcpyDeviceToHost);
}

// N words that kernels count into, allocated on first use.  `valid` says whether the words belong to the launch set queued last:
// whoever queues launches sets it, and a counter that is not valid, or has never been allocated, reads 0 without touching the device.
template <class T, size_t N>
class Counter {
public:
    explicit Counter(bool valid_ = true) : valid(valid_) {}
    bool valid;

    hipError_t ensure() { return buf_.reserve(N, nothing()); }
    hipError_t zero(hipStream_t s) const { return hipMemsetAsync(buf_.get(), 0, N * sizeof(T), s); }
    T* get() const { return buf_.get(); }
    hipError_t read(int device, T (&out)[N]) const
    {
        for (T& w : out) w = 0;
        return buf_.get() && valid ? read_words(device, buf_.get(), N, out) : hipSuccess;
    }

private:
    DeviceBuf<T> buf_;
};

// An event, created on first use.  Converts to its handle (nullptr until ensure has succeeded).
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept
    {
        if (this != &o) {
            release();
            std::swap(e_, o.e_);
        }
        return *this;
    }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { release(); }

    hipError_t ensure(unsigned flags = hipEventDisableTiming)
    {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }
    void release()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

// A stream, created on first use (when a stream comes into being matters: a process's streams share four hardware queues).
class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept
    {
        if (this != &o) {
            release();
            std::swap(s_, o.s_);
        }
        return *this;
    }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { release(); }

    hipError_t ensure(unsigned flags) { return s_ ? hipSuccess : created(hipStreamCreateWithFlags(&s_, flags)); }
    hipError_t ensure_with_priority(unsigned flags, int priority) { return s_ ? hipSuccess : created(hipStreamCreateWithPriority(&s_, flags, priority)); }
    hipStream_t get() const { return s_; }
    operator hipStream_t() const { return s_; }
    void release()
    {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }

private:
    hipError_t created(hipError_t e)
    {
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    hipStream_t s_ = nullptr;
};

} // namespace rtxmem
