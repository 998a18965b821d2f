// rtx_update.cpp -- RayTracingManager::Update (RayTracingManager.cu:76-154) in one call, and its family: rtx_update, the pipelined
// rtx_update_begin / rtx_update_end, rtx_update_delta, rtx_update_half and rtx_update_half_delta.  Every one of them is the same sequence:
//   0. the call's plan (rtxplan::plan_update, rtx_plan.hpp): its refusal, what it traces and encodes, how it tries to deliver
//   1. the physics step (rtx_update_objects)
//   2. trace: pixel words or records into a buffer of the context's, of an update slot's or of the delta pair's
//   3. encode: Minimize, or its delta or half-block form (rtx_post.hip), into a device buffer or into the caller's host buffer itself
//   4. deliver: the wait for the stream's length, and the copy of the stream where the form has one
// The steps are written once below; an entry point is its argument checks, its plan and the steps in its order.  The blocking forms
// wait at once; rtx_update_begin stops where nothing more can be queued without a wait for the copy, and rtx_update_end finishes.
#include "rtx_ctx.h"
#include "rtx_group.h"

#include <vector>

namespace {

using rtxplan::UpdatePlan;
using UpdateSlot = rtx_ctx::UpdateSlot;

// ---- 0 and 1: the plan of a call, then its refusal and the physics step (RayTracingManager.cu:89-107) in the order the plan says;
// the device is the context's afterwards.  (A pipelined call's step comes behind its slot: rtx_update_begin.)
int enter(rtx_ctx* ctx, rtxplan::UpdateEntry entry, const rtx_params* p, int mode, const void* host_out, double dt, int run_physics, UpdatePlan* plan, bool unknown_flags = false)
{
    const bool aligned = ((uintptr_t)host_out & 15u) == 0;
    *plan = rtxplan::plan_update({entry, mode, p->x, p->y, ctx->capacity, unknown_flags, ctx->opt.update_words, ctx->opt.min_fused, ctx->opt.update_host_write, ctx->group != nullptr, rtxgroup::update_direct_wanted(ctx), aligned});
    int rc;
    if (plan->physics_first && run_physics && (rc = rtx_update_objects(ctx, dt)) != RTX_OK) return rc;
    if (plan->refusal != RTX_OK) return rtx_fail(ctx, plan->refusal, plan->message);
    if (!plan->physics_first && entry != rtxplan::kUpdatePipelined && run_physics && (rc = rtx_update_objects(ctx, dt)) != RTX_OK) return rc;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    return RTX_OK;
}

// ---- 2: trace

int ensure_words_buffer(rtx_ctx* ctx, DeviceBuf<uint32_t>& buf, size_t need)
{
    return buf.reserve(need, rtxmem::after_stream(ctx->stream)) == hipSuccess ? RTX_OK : rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the pixel-word buffer");
}

// The frame of `p` as W*H pixel words, complete in stream order on the context's stream, as *in, Minimize's input: sharded over the
// group's devices and gathered into the group's buffer, or one launch into `own` (grown as needed).  `keep`: the words are wanted
// in `own` whoever traced them (a delta's next call compares with them), so a group's gathered words are copied into it.
int trace_words(rtx_ctx* ctx, const rtx_params* p, int mode, DeviceBuf<uint32_t>& own, bool keep, MinInput* in)
{
    const size_t W = (size_t)p->x, H = (size_t)p->y;
    const uint32_t* d_words = nullptr;
    int rc;
    if ((!ctx->group || keep) && (rc = ensure_words_buffer(ctx, own, W * H)) != RTX_OK) return rc;
    if (!ctx->group) {
        rc = rtx_render_rows(ctx, p, mode, 0, H, own.get(), 0, ctx->stream, RTX_RENDER_COMPACT);
    } else if ((rc = rtxgroup::render_words(ctx, p, mode, &d_words)) == RTX_OK && keep) {
        RTX_HIP(ctx, hipMemcpyAsync(own.get(), d_words, W * H * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    }
    *in = words_input(mode, W, H, ctx->group && !keep ? d_words : own.get());
    return rc;
}

// ---- 3: encode.  The copy forms encode into a device buffer (launch_minimize, minimize_and_wait); the host-write form
// (RTX_OPT_UPDATE_HOST_WRITE) has the Minimize launch store the stream straight into the caller's buffer -- pinned host memory,
// addressed by the device -- and its length into a pinned pair, so that no copy is queued and nothing is waited for twice.  A
// console-sized frame's Update is three launches, two small copies and two waits -- 45 us of which the kernels are 11 -- and this
// takes a copy, the stream's copy and a wait out of it.

// Tried once the frame is traced.  *written stays false where host_out is not device-addressable (pageable memory): the copy form
// then.  Else the launch is queued -- it is what RTX_STAT_UPDATE_HOST_WRITES counts -- and nothing is waited for: after a wait
// `pair` holds the two result words of `run`.
int queue_host_write(rtx_ctx* ctx, void* host_out, PinnedBuf<uint64_t>& pair, void* d_scan, const MinInput& in, MinRun* run, bool* written)
{
    void *d_host = nullptr, *d_pair = nullptr;
    if (hipHostGetDevicePointer(&d_host, host_out, 0) != hipSuccess || d_host == nullptr) {
        (void)hipGetLastError();
        return RTX_OK;
    }
    if (pair.reserve(2, rtxmem::nothing()) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipHostMalloc failed for the stream's length");
    RTX_HIP(ctx, hipHostGetDevicePointer(&d_pair, pair.get(), 0));
    pair.get()[0] = pair.get()[1] = 0; // (whoever used the pair last has been waited for)
    const int rc = launch_minimize(ctx, d_scan, in, (uint8_t*)d_host, run, (uint64_t*)d_pair);
    if (rc == RTX_OK) ctx->stat_host_writes++;
    *written = rc == RTX_OK;
    return rc;
}

// ---- 4: deliver

// The length of `run`'s stream from the two result words a wait has brought to the host.  (Blocks that gave up: the chain, into the
// same buffer -- the caller's, in the host-write form -- and its length read back the usual way.)
int settle_bytes(rtx_ctx* ctx, const MinRun& run, const uint64_t* pair, size_t* bytes)
{
    uint64_t total = 0;
    const int rc = settle_minimize(ctx, run, pair, &total);
    if (rc == RTX_OK) *bytes = (size_t)total;
    return rc;
}

// Steps 3 and 4 of the copy form for a call that waits at once: Minimize of `in` into d_stream (nullptr: the context's own buffer),
// the wait for its length, the copy of that many bytes to host_out and the wait for them.  `too_long`: the refusal of a stream of
// more than host_capacity bytes.
int encode_copy_wait(rtx_ctx* ctx, const MinInput& in, uint8_t* d_stream, void* host_out, size_t host_capacity, const char* too_long, size_t* out_bytes)
{
    RTX_HIP(ctx, hipSetDevice(ctx->device)); // (a group's trace may have left another member's device current)
    size_t n = 0;
    const int rc = minimize_and_wait(ctx, in, d_stream, &n);
    if (rc != RTX_OK) return rc;
    if (n > host_capacity) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, too_long);
    if (n) {
        RTX_HIP(ctx, hipMemcpyAsync(host_out, d_stream ? d_stream : ctx->d_min.get(), n, hipMemcpyDeviceToHost, ctx->stream));
        RTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out_bytes = n;
    return RTX_OK;
}

// rtx_update on a device group WITHOUT a gather (RTX_OPT_GROUP_UPDATE): the whole Update is bound by the copy of the minimised
// stream over one PCIe link, and a group has one link per device.  Every rank traces its rows as pixel words -- and the row above
// them, whose last pixel is the colour its first pixel is compared with (RayTracingManager.cu:181-319 carries the last emitted colour
// across rows) -- minimises its own rows (launch_minimize with `lead` = W) and, once the lengths of the ranks before it are
// known on the host, copies its part of the stream to its place in host_out from its own device.  The ranks' parts, in rank
// order, are the bytes the root would have made of the gathered frame.
int update_group_direct(rtx_ctx* root, const rtx_params* p, int mode, void* host_out, size_t* out_bytes)
{
    const int N = rtx_group_size(root);
    const size_t W = (size_t)p->x, H = (size_t)p->y;
    struct Part {
        size_t row0 = 0, rows = 0, bytes = 0, offset = 0;
    };
    std::vector<Part> part((size_t)N);
    std::vector<MinRun> runs((size_t)N);
    for (int r = 0; r < N; r++) {
        const rtxplan::Slab s = rtxplan::slab_of(H, r, N);
        part[(size_t)r].row0 = (size_t)s.row0;
        part[(size_t)r].rows = (size_t)s.rows;
    }
    auto wait_for = [](rtx_ctx* m) -> int {
        RTX_HIP(m, hipSetDevice(m->device));
        RTX_HIP(m, hipStreamSynchronize(m->stream));
        return RTX_OK;
    };
    // a rank's device work: trace (its rows and the one above), minimise, the two words of the result on their way to the host
    auto queue_rows = [&](int r, rtx_ctx* m) -> int {
        Part& q = part[(size_t)r];
        if (q.rows == 0) return RTX_OK;
        RTX_HIP(m, hipSetDevice(m->device));
        const size_t above = q.row0 > 0 ? 1u : 0u;
        int rc2 = ensure_words_buffer(m, m->d_words, (q.rows + above) * W);
        if (rc2 != RTX_OK) return rc2;
        if (m->h_pair.reserve(2, rtxmem::nothing()) != hipSuccess) return rtx_fail(m, RTX_ERR_OUT_OF_MEMORY, "hipHostMalloc failed for a rank's stream length");
        if ((rc2 = rtx_render_rows(m, p, mode, q.row0 - above, q.rows + above, m->d_words.get(), q.row0 - above, m->stream, RTX_RENDER_COMPACT)) != RTX_OK) return rc2;
        if ((rc2 = ensure_min_buffers(m, (uint64_t)W * q.rows, true)) != RTX_OK) return rc2;
        MinRun& run = runs[(size_t)r];
        if ((rc2 = launch_minimize(m, m->d_scan.get(), words_input(mode, W, q.rows, m->d_words.get() + above * W, (uint32_t)(above * W)), m->d_min.get(), &run)) != RTX_OK) return rc2;
        RTX_HIP(m, hipMemcpyAsync(m->h_pair.get(), run.d_total, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
        return RTX_OK;
    };
    auto await_rows = [&](int r, rtx_ctx* m) -> int {
        Part& q = part[(size_t)r];
        if (q.rows == 0) return RTX_OK;
        const int rc2 = wait_for(m);
        return rc2 != RTX_OK ? rc2 : settle_bytes(m, runs[(size_t)r], m->h_pair.get(), &q.bytes);
    };
    auto queue_copy = [&](int r, rtx_ctx* m) -> int {
        const Part& q = part[(size_t)r];
        if (q.bytes == 0) return RTX_OK;
        RTX_HIP(m, hipSetDevice(m->device));
        RTX_HIP(m, hipMemcpyAsync((uint8_t*)host_out + q.offset, m->d_min.get(), q.bytes, hipMemcpyDeviceToHost, m->stream));
        return RTX_OK;
    };
    auto await_copy = [&](int r, rtx_ctx* m) -> int { return part[(size_t)r].bytes ? wait_for(m) : RTX_OK; };
    int rc = rtxgroup::run_phases(root, queue_rows, await_rows);
    if (rc != RTX_OK) {
        (void)hipSetDevice(root->device);
        return rc;
    }
    size_t at = 0;
    for (int r = 0; r < N; r++) {
        part[(size_t)r].offset = at;
        at += part[(size_t)r].bytes;
    }
    rc = rtxgroup::run_phases(root, queue_copy, await_copy);
    RTX_HIP(root, hipSetDevice(root->device));
    if (rc != RTX_OK) return rc;
    *out_bytes = at;
    return RTX_OK;
}

// One attempt at it.  true: host_out holds the frame, *out_bytes its length.  false: nothing was delivered, the group gathers on
// its root from now on, and this frame goes the next way the plan has.
bool deliver_group_direct(rtx_ctx* ctx, const rtx_params* p, int mode, void* host_out, size_t* out_bytes)
{
    const bool ok = update_group_direct(ctx, p, mode, host_out, out_bytes) == RTX_OK;
    rtxgroup::update_direct_done(ctx, ok);
    if (!ok) (void)hipGetLastError();
    return ok;
}

// ---- the pipelined form's slots

// What a slot needs for a frame of n_slots.  Every member under its own null check: a call that fails half-way (out of memory)
// leaves a slot the next call completes, instead of one that looks initialised with null buffers behind it.
int prepare_slot(rtx_ctx* ctx, UpdateSlot& sl, bool records, uint64_t n_slots)
{
    if (!ctx->copy_stream) {
        // A stream of another priority than the render streams': the runtime spreads a process's streams of one priority over four
        // hardware queues, and a copy that lands in the queue of the context's own stream holds back the next frame's kernels until
        // it is done -- the pipelined Update then costs copy + kernels (0.376 ms) instead of the copy alone (0.326), which is what
        // bench.py's default line measured whenever four render streams had been created first.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest ||
            ctx->copy_stream.ensure_with_priority(hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();
            RTX_HIP(ctx, ctx->copy_stream.ensure(hipStreamNonBlocking));
        }
    }
    if (records && !sl.d_frame.get()) {
        if (sl.d_frame.reserve(ctx->capacity, rtxmem::nothing()) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for an update slot's frame");
        const hipError_t me = hipMemsetAsync(sl.d_frame.get(), 0, ctx->capacity, ctx->stream);
        if (me != hipSuccess) {
            sl.d_frame.release();
            return rtx_hip_fail(ctx, me, "hipMemsetAsync(update slot frame)");
        }
    }
    if (!sl.d_min.get() && sl.d_min.reserve(ctx->capacity, rtxmem::nothing()) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for an update slot's minimise buffer");
    if (sl.h_total.reserve(2, rtxmem::nothing()) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipHostMalloc failed for an update slot");
    RTX_HIP(ctx, sl.ev_ready.ensure());
    RTX_HIP(ctx, sl.ev_copied.ensure());
    // (the slot is not busy: the launch that used the old scratch has been waited for)
    RTX_HIP(ctx, sl.d_scan.reserve(min_scan_bytes(n_slots), rtxmem::nothing()));
    return RTX_OK;
}

// Steps 2 to 4 of a pipelined frame, as far as they go without a wait for the frame's last byte; rtx_update_end waits for
// sl.ev_ready (the host-write form) or sl.ev_copied (the others).
int queue_frame(rtx_ctx* ctx, const UpdatePlan& plan, UpdateSlot& sl, const rtx_params* p, int mode, void* host_out)
{
    sl.host_write = false;
    if (plan.try_group_direct && deliver_group_direct(ctx, p, mode, host_out, &sl.bytes)) {
        // N links carry the stream at once, which is worth more than the overlap of one link's copy with the next trace: the frame is
        // complete already.  (The copy stream carries nothing; the event is recorded because rtx_update_end waits on it.)
        RTX_HIP(ctx, hipEventRecord(sl.ev_copied, ctx->copy_stream));
        return RTX_OK;
    }
    MinInput in;
    int rc;
    if (plan.source == rtxplan::kUpdateWords) {
        // pixel words into the slot's own buffer (a group: into the group's, gathered), minimised from there
        if ((rc = trace_words(ctx, p, mode, sl.d_words, false, &in)) != RTX_OK) return rc;
    } else {
        // the slot's frame buffer is caller-style memory for rtx_render_rows: whole frame, with the zero semantics of the per-frame
        // memset (the buffer starts zeroed; SDL frames write nothing, so clear)
        const size_t W = (size_t)p->x, H = (size_t)p->y;
        const unsigned flags = mode >= RTX_RGB_ASCII ? RTX_RENDER_DEFAULT : RTX_RENDER_ZERO_TAIL;
        if (mode == RTX_SDL) RTX_HIP(ctx, hipMemsetAsync(sl.d_frame.get(), 0, 20 * W * H, ctx->stream));
        rc = ctx->group ? rtxgroup::render_frame(ctx, p, mode, sl.d_frame.get(), flags) : rtx_render_rows(ctx, p, mode, 0, H, sl.d_frame.get(), 0, ctx->stream, flags);
        if (rc != RTX_OK) return rc;
        in = records_input(mode, W, H, sl.d_frame.get());
    }
    // a small frame: NOTHING is waited for here.  (At console sizes the copy form's two waits per frame were what the pipelined Update cost.)
    if (plan.try_host_write && (rc = queue_host_write(ctx, host_out, sl.h_total, sl.d_scan.get(), in, &sl.run, &sl.host_write)) != RTX_OK) return rc;
    if (sl.host_write) {
        RTX_HIP(ctx, hipEventRecord(sl.ev_ready, ctx->stream));
        return RTX_OK;
    }
    if ((rc = launch_minimize(ctx, sl.d_scan.get(), in, sl.d_min.get(), &sl.run)) != RTX_OK) return rc;
    RTX_HIP(ctx, hipMemcpyAsync(sl.h_total.get(), sl.run.d_total, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    RTX_HIP(ctx, hipEventRecord(sl.ev_ready, ctx->stream));
    // the length is needed on the host to size the copy: wait for this frame's kernels (the previous frame's copy keeps running on
    // the copy stream meanwhile)
    RTX_HIP(ctx, hipEventSynchronize(sl.ev_ready));
    if ((rc = settle_bytes(ctx, sl.run, sl.h_total.get(), &sl.bytes)) != RTX_OK) return rc;
    if (sl.bytes) RTX_HIP(ctx, hipMemcpyAsync(host_out, sl.d_min.get(), sl.bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
    RTX_HIP(ctx, hipEventRecord(sl.ev_copied, ctx->copy_stream));
    return RTX_OK;
}

} // namespace

extern "C" {

int rtx_update(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, void* host_out, size_t* out_bytes)
{
    if (!ctx || !params || !host_out || !out_bytes) return RTX_ERR_INVALID_ARGUMENT;
    ctx->delta_valid = false; // (the consumer's screen is about to show this frame: the next rtx_update_delta gives a key frame)
    UpdatePlan plan;
    int rc = enter(ctx, rtxplan::kUpdateBlocking, params, mode, host_out, dt, run_physics, &plan);
    if (rc != RTX_OK) return rc;
    if (plan.source == rtxplan::kUpdateRecords) {
        // :86 + :120-134: zero semantics and trace into the context's frame buffer -- rtx_render refuses what the plan of this form
        // does not look at; :146: minimise on the device; :143 then only moves the minimised stream across PCIe
        if ((rc = rtx_render(ctx, params, mode)) != RTX_OK) return rc;
        return encode_copy_wait(ctx, records_input(mode, (size_t)params->x, (size_t)params->y, ctx->d_frame.get()), nullptr, host_out, ~(size_t)0, "", out_bytes);
    }
    // :120-134 + :146 on 4-byte pixel words: the trace stores words, the minimise pass reads them and writes the very stream it
    // would have made of the records (which are never written: the context's frame buffer keeps what it held)
    if (plan.try_group_direct && deliver_group_direct(ctx, params, mode, host_out, out_bytes)) return RTX_OK;
    MinInput in;
    MinRun run;
    bool written = false; // (a group that gathers on its root takes this way too: the root's Minimize launch writes the host buffer)
    if ((rc = trace_words(ctx, params, mode, ctx->d_words, false, &in)) != RTX_OK) return rc;
    if (plan.try_host_write && (rc = ensure_min_buffers(ctx, (uint64_t)in.w * in.h, false)) != RTX_OK) return rc;
    if (plan.try_host_write && (rc = queue_host_write(ctx, host_out, ctx->h_pair, ctx->d_scan.get(), in, &run, &written)) != RTX_OK) return rc;
    if (!written) return encode_copy_wait(ctx, in, nullptr, host_out, ~(size_t)0, "", out_bytes);
    // ONE host wait, at any size in this blocking form -- 1080p: 0.370 ms against 0.395 with the copy queued after a wait for the length
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return settle_bytes(ctx, run, ctx->h_pair.get(), out_bytes);
}

// ---- pipelined Update: the frame sequence of RayTracingManager::Update split in two calls so
// that the copy of frame k's minimised stream to the host overlaps the trace of frame k+1.
int rtx_update_begin(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, void* host_out, int* ticket)
{
    if (!ctx || !params || !host_out || !ticket) return RTX_ERR_INVALID_ARGUMENT;
    ctx->delta_valid = false; // (as rtx_update: the next rtx_update_delta gives a key frame)
    UpdatePlan plan;
    int rc = enter(ctx, rtxplan::kUpdatePipelined, params, mode, host_out, dt, run_physics, &plan);
    if (rc != RTX_OK) return rc;
    const unsigned si = ctx->upd_next;
    UpdateSlot& sl = ctx->upd[si];
    if (sl.busy) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_update_begin: both slots are in flight; call rtx_update_end first");
    if ((rc = prepare_slot(ctx, sl, plan.source == rtxplan::kUpdateRecords, params->x * params->y)) != RTX_OK) return rc;
    if (run_physics && (rc = rtx_update_objects(ctx, dt)) != RTX_OK) return rc;
    if ((rc = queue_frame(ctx, plan, sl, params, mode, host_out)) != RTX_OK) return rc;
    // the slot is in flight
    sl.busy = true;
    *ticket = (int)si;
    ctx->upd_next = si ^ 1u;
    return RTX_OK;
}

int rtx_update_end(rtx_ctx* ctx, int ticket, size_t* out_bytes)
{
    if (!ctx || !out_bytes || ticket < 0 || ticket > 1) return RTX_ERR_INVALID_ARGUMENT;
    UpdateSlot& sl = ctx->upd[ticket];
    if (!sl.busy) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_update_end: no frame in flight under this ticket");
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    RTX_HIP(ctx, hipEventSynchronize(sl.host_write ? sl.ev_ready : sl.ev_copied));
    sl.busy = false;
    if (sl.host_write) {
        sl.host_write = false;
        return settle_bytes(ctx, sl.run, sl.h_total.get(), out_bytes);
    }
    *out_bytes = sl.bytes;
    return RTX_OK;
}

int rtx_update_delta(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, unsigned flags, void* host_out, size_t host_capacity,
                     size_t* out_bytes, int* kind)
{
    if (!ctx || !params || !host_out || !out_bytes || !kind) return RTX_ERR_INVALID_ARGUMENT;
    UpdatePlan plan;
    int rc = enter(ctx, rtxplan::kUpdateDelta, params, mode, host_out, dt, run_physics, &plan, (flags & ~(unsigned)RTX_DELTA_KEYFRAME) != 0);
    if (rc != RTX_OK) return rc;
    const size_t W = (size_t)params->x, H = (size_t)params->y;
    // (delta_half: the consumer's screen shows a half-block frame, rtx_update_half_delta's)
    const bool key = !ctx->delta_valid || ctx->delta_half || ctx->delta_w != W || ctx->delta_h != H || ctx->delta_mode != mode || (flags & RTX_DELTA_KEYFRAME) != 0;
    const unsigned at = ctx->delta_at ^ 1u; // the buffer that does NOT hold the frame handed out last: nothing of this call reads it before it is written
    ctx->delta_valid = false;               // until this call has handed its frame out
    // the words: traced straight into the pair's buffer; a group's gathered words are copied into it.  A key frame is what rtx_update
    // makes of them: Minimize into the context's buffer
    MinInput in;
    uint8_t* d_stream = nullptr;
    if ((rc = trace_words(ctx, params, mode, ctx->d_delta_words[at], true, &in)) != RTX_OK) return rc;
    if (!key) {
        if (ctx->d_delta_out.reserve(rtx_delta_bound(mode, W, H), rtxmem::after_stream(ctx->stream)) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the delta buffer");
        unsigned long long* counts = nullptr;
        if ((rc = rtx_delta_counters(ctx, &counts)) != RTX_OK) return rc;
        in = delta_input(mode, W, H, in.data, ctx->d_delta_words[at ^ 1u].get(), counts);
        d_stream = ctx->d_delta_out.get();
    }
    if ((rc = encode_copy_wait(ctx, in, d_stream, host_out, host_capacity, "rtx_update_delta: the stream is longer than host_capacity (the next call gives a key frame)", out_bytes)) != RTX_OK) return rc;
    ctx->delta_at = at;
    ctx->delta_valid = true;
    ctx->delta_half = false;
    ctx->delta_w = W;
    ctx->delta_h = H;
    ctx->delta_mode = mode;
    ctx->stat_delta_frames++;
    if (key) ctx->stat_delta_keyframes++;
    *kind = key ? RTX_DELTA_KEY : RTX_DELTA_DIFF;
    return RTX_OK;
}

int rtx_update_half(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, void* host_out, size_t host_capacity, size_t* out_bytes)
{
    if (!ctx || !params || !host_out || !out_bytes) return RTX_ERR_INVALID_ARGUMENT;
    ctx->delta_valid = false; // (the consumer's screen is about to show this frame: the next rtx_update_delta gives a key frame)
    UpdatePlan plan;
    int rc = enter(ctx, rtxplan::kUpdateHalf, params, mode, host_out, dt, run_physics, &plan);
    if (rc != RTX_OK) return rc;
    const size_t W = (size_t)params->x, H = (size_t)params->y;
    // the sample frame: two pixel rows per console row, under the same field of view (ray generation divides by y)
    rtx_params sample = *params;
    sample.y = 2u * (uint64_t)H;
    MinInput in;
    if ((rc = trace_words(ctx, &sample, mode, ctx->d_words, false, &in)) != RTX_OK) return rc;
    // (every earlier launch into the buffer has been waited for by the call that queued it)
    if (ctx->d_half_out.reserve((rtx_half_bound(mode, W, H) + 15u) & ~(size_t)15u, rtxmem::nothing()) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the half-block buffer");
    rc = encode_copy_wait(ctx, half_input(mode, W, H, in.data), ctx->d_half_out.get(), host_out, host_capacity, "rtx_update_half: the stream is longer than host_capacity", out_bytes);
    if (rc == RTX_OK) ctx->stat_half_frames++;
    return rc;
}

// rtx_update_delta's sequence over rtx_update_half's frame: the delta pair holds W x 2H words, a key frame is rtx_update_half's stream.
int rtx_update_half_delta(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, unsigned flags, void* host_out, size_t host_capacity,
                          size_t* out_bytes, int* kind)
{
    if (!ctx || !params || !host_out || !out_bytes || !kind) return RTX_ERR_INVALID_ARGUMENT;
    UpdatePlan plan;
    int rc = enter(ctx, rtxplan::kUpdateHalfDelta, params, mode, host_out, dt, run_physics, &plan, (flags & ~(unsigned)RTX_DELTA_KEYFRAME) != 0);
    if (rc != RTX_OK) return rc;
    const size_t W = (size_t)params->x, H = (size_t)params->y;
    const bool key = !ctx->delta_valid || !ctx->delta_half || ctx->delta_w != W || ctx->delta_h != H || ctx->delta_mode != mode || (flags & RTX_DELTA_KEYFRAME) != 0;
    const unsigned at = ctx->delta_at ^ 1u; // the buffer that does NOT hold the frame handed out last
    ctx->delta_valid = false;               // until this call has handed its frame out
    // the sample frame: two pixel rows per console row, under the same field of view (ray generation divides by y)
    rtx_params sample = *params;
    sample.y = 2u * (uint64_t)H;
    MinInput in;
    if ((rc = trace_words(ctx, &sample, mode, ctx->d_delta_words[at], true, &in)) != RTX_OK) return rc;
    // (every earlier launch into the buffer has been waited for by the call that queued it)
    if (ctx->d_half_out.reserve((rtx_half_delta_bound(mode, W, H) + 15u) & ~(size_t)15u, rtxmem::nothing()) != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the half-block buffer");
    if (key) {
        in = half_input(mode, W, H, in.data);
    } else {
        unsigned long long* counts = nullptr;
        if ((rc = rtx_delta_counters(ctx, &counts)) != RTX_OK) return rc;
        in = half_delta_input(mode, W, H, in.data, ctx->d_delta_words[at ^ 1u].get(), counts);
    }
    if ((rc = encode_copy_wait(ctx, in, ctx->d_half_out.get(), host_out, host_capacity, "rtx_update_half_delta: the stream is longer than host_capacity (the next call gives a key frame)", out_bytes)) != RTX_OK) return rc;
    ctx->delta_at = at;
    ctx->delta_valid = true;
    ctx->delta_half = true;
    ctx->delta_w = W;
    ctx->delta_h = H;
    ctx->delta_mode = mode;
    ctx->stat_half_delta_frames++;
    if (key) ctx->stat_half_delta_keyframes++;
    *kind = key ? RTX_DELTA_KEY : RTX_DELTA_DIFF;
    return RTX_OK;
}

} // extern "C"
