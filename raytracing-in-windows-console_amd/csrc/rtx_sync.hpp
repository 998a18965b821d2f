// rtx_sync.hpp -- ordering across streams: a table keyed by stream, and Shared, the one protocol for a thing on the device that one
// stream writes and launches on any stream read (the coarse-cell list sets, the world grid).  DESIGN.md 3, "Ordering across streams".
#pragma once

#include "rtx_mem.hpp"

#include <vector>

namespace rtxsync {

// A small vector of entries with a `stream` member, at most one per stream.  What a full table means is the caller's business.
template <class T>
T* find(std::vector<T>& v, hipStream_t s)
{
    for (auto& e : v) {
        if (e.stream == s) return &e;
    }
    return nullptr;
}

// A fresh entry for `s` at the back, or nullptr when the table holds `capacity` entries already.
template <class T>
T* add(std::vector<T>& v, hipStream_t s, size_t capacity)
{
    if (v.size() >= capacity) return nullptr;
    v.emplace_back();
    v.back().stream = s;
    return &v.back();
}

// Between end_write and the next begin_write the thing is read: a launch on `r` that reads it is queued after read(r); close(r)
// says that r's launches queued so far are the last that read it for now (it costs one event record; an open reader is closed
// by the next begin_write at the latest).  A write is begin_write(w), the work queued on w, end_write(w, ..).  Then every read
// queued before begin_write finishes before the work starts, and every read queued after end_write starts after the work.
class Shared {
public:
    static constexpr size_t kMaxReaders = 32;

    hipError_t begin_write(hipStream_t w)
    {
        hipError_t e = ev_write_.ensure();
        if (e != hipSuccess) return e;
        const Reader* me = find(readers_, w);
        if (written_ && !(me && me->ordered) && (e = hipStreamWaitEvent(w, ev_write_, 0)) != hipSuccess) return e;
        for (Reader& r : readers_) {
            if (r.stream != w) {
                close(r);
                if (r.state == kClosed && (e = hipStreamWaitEvent(w, r.ev, 0)) != hipSuccess) return e;
            }
            r.state = kIdle; // (w's own reads are in front of the work on w)
        }
        return hipSuccess;
    }

    // readers_on_w_are_ordered: launches queued on w from now on come after the work without a wait (not so for a side stream,
    // whose handle a caller's render stream never is)
    hipError_t end_write(hipStream_t w, bool readers_on_w_are_ordered)
    {
        const hipError_t e = hipEventRecord(ev_write_, w);
        if (e != hipSuccess) return e;
        for (Reader& r : readers_) r.ordered = false;
        if (readers_on_w_are_ordered) entry(w).ordered = true;
        written_ = true;
        ready_ = false;
        return hipSuccess;
    }

    hipError_t read(hipStream_t r)
    {
        Reader& me = entry(r);
        if (!me.ordered) {
            const hipError_t e = hipStreamWaitEvent(r, ev_write_, 0);
            if (e != hipSuccess) return e;
            me.ordered = true;
        }
        me.state = kOpen;
        return hipSuccess;
    }

    void close(hipStream_t r)
    {
        if (Reader* me = find(readers_, r)) close(*me);
    }

    bool written() const { return written_; }
    hipEvent_t last_write() const { return ev_write_; }

    // the last write is known to have finished (asked of the event until it says so once)
    bool ready()
    {
        if (written_ && !ready_) {
            if (hipEventQuery(ev_write_) == hipSuccess) ready_ = true;
            else (void)hipGetLastError(); // hipErrorNotReady
        }
        return ready_;
    }

    // the caller has just waited for the whole device
    void forget_readers()
    {
        for (Reader& r : readers_) r.state = kIdle;
    }

private:
    enum State { kIdle, kOpen, kClosed }; // open: launches that read, no event behind them yet; closed: `ev` is behind the last of them
    struct Reader {
        hipStream_t stream = nullptr;
        rtxmem::Event ev;     // one per stream, re-recorded at every close: streams run in order, a later record covers the earlier
        State state = kIdle;
        bool ordered = false; // the stream is ordered after the last write
    };

    // An open reader gets its event now.  A stream the caller has destroyed since cannot be recorded on: then the whole device is
    // waited for instead.
    void close(Reader& r)
    {
        if (r.state != kOpen) return;
        if (r.ev.ensure() == hipSuccess && hipEventRecord(r.ev, r.stream) == hipSuccess) {
            r.state = kClosed;
        } else {
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
            r.state = kIdle;
        }
    }

    // Entries outlive writes, so that their events are reused.  A caller that keeps creating streams: settle everything, start over.
    Reader& entry(hipStream_t s)
    {
        Reader* r = find(readers_, s);
        if (!r && !(r = add(readers_, s, kMaxReaders))) {
            (void)hipDeviceSynchronize();
            readers_.clear();
            r = add(readers_, s, kMaxReaders);
        }
        return *r;
    }

    rtxmem::Event ev_write_;
    bool written_ = false, ready_ = false;
    std::vector<Reader> readers_;
};

} // namespace rtxsync
