// rtx_post.hip -- what RayTracingManager::Update runs around the trace kernel, on the GPU:
// UpdateObjects (RayTracingManager.cu:10-44, 89-107) and Minimize (RayTracingManager.cu:167-319) with its delta, half-block and
// half-block delta encoders.  (The whole of Update in one call -- rtx_update and its family -- is rtx_update.cpp, which drives the launches here.)
// Also the edits of scene objects in place (rtx_scene_set_spheres, rtx_scene_set_spheres_device, rtx_scene_set_plane) and their removal
// (rtx_scene_remove_objects, rtx_scene_remove_marked_device): their kernels sit beside the physics step's, which moves the same arrays.
#include "rtx_ctx.h"
#include "rtx_group.h"
#include "rtx_device.hpp"
#include "rtx_records.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rtx_post_kernels.inc" // namespace rtx: the kernels launched below

namespace {

uint64_t min_blocks(uint64_t n_slots) { return (n_slots + rtx::kSlotsPerBlock - 1) / rtx::kSlotsPerBlock; }

} // namespace

// Bytes of Minimize scratch for a frame of n_slots: [total u64 x 8][offsets u64 x blocks][sums u32 x blocks]
size_t min_scan_bytes(uint64_t n_slots) { return (size_t)min_blocks(n_slots) * (sizeof(uint32_t) + sizeof(uint64_t)) + 64; }

int ensure_min_buffers(rtx_ctx* ctx, uint64_t n_slots, bool need_out)
{
    // (every minimise launch that used the old scratch has been waited for by the call that queued it)
    if (ctx->d_scan.reserve(min_scan_bytes(n_slots), rtxmem::nothing()) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the minimise scratch");
    }
    // m_minimizedResultArray is as large as the frame (RayTracingManager.cu:66)
    if (need_out && !ctx->d_min.get() && ctx->d_min.reserve(ctx->capacity, rtxmem::nothing()) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the minimise buffer");
    }
    return RTX_OK;
}

namespace {

// f(Src()) with the slot source (rtx_post_kernels.inc) of `in`: the one place where a mode and an input form pick the kernels.
template <class F>
int with_source(rtx_ctx* ctx, const MinInput& in, F f)
{
    if (!in.words) {
        const bool rgb = !(in.mode == RTX_BIT_ASCII || in.mode == RTX_BIT_PIXEL); // MinimizeResults, RayTracingManager.cu:167-179
        if (rgb) {
            f(rtx::RecordSource<20>());
        } else {
            f(rtx::RecordSource<12>());
        }
        return RTX_OK;
    }
    if (in.half) {
        if (in.mode < RTX_BIT_ASCII || in.mode >= RTX_SDL) return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "no pixel words in this mode");
        // the family alone decides: the glyph byte of a word is ignored
        if (in.prev) {
            if (in.mode >= RTX_RGB_ASCII) {
                f(rtx::HalfDeltaSource<true>());
            } else {
                f(rtx::HalfDeltaSource<false>());
            }
        } else if (in.mode >= RTX_RGB_ASCII) {
            f(rtx::HalfSource<true>());
        } else {
            f(rtx::HalfSource<false>());
        }
        return RTX_OK;
    }
    if (in.prev) {
        switch (in.mode) {
        case RTX_BIT_ASCII: f(rtx::DeltaSource<RTX_K_BIT_ASCII>()); break;
        case RTX_BIT_PIXEL: f(rtx::DeltaSource<RTX_K_BIT_PIXEL>()); break;
        case RTX_RGB_ASCII: f(rtx::DeltaSource<RTX_K_RGB_ASCII>()); break;
        case RTX_RGB_PIXEL: f(rtx::DeltaSource<RTX_K_RGB_PIXEL>()); break;
        case RTX_RGB_NORMALS: f(rtx::DeltaSource<RTX_K_RGB_NORMALS>()); break;
        default: return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "no pixel words in this mode");
        }
        return RTX_OK;
    }
    switch (in.mode) {
    case RTX_BIT_ASCII: f(rtx::WordSource<RTX_K_BIT_ASCII>()); break;
    case RTX_BIT_PIXEL: f(rtx::WordSource<RTX_K_BIT_PIXEL>()); break;
    case RTX_RGB_ASCII: f(rtx::WordSource<RTX_K_RGB_ASCII>()); break;
    case RTX_RGB_PIXEL: f(rtx::WordSource<RTX_K_RGB_PIXEL>()); break;
    case RTX_RGB_NORMALS: f(rtx::WordSource<RTX_K_RGB_NORMALS>()); break;
    default: return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "no pixel words in this mode");
    }
    return RTX_OK;
}

// The chain of `run` on the context's stream: count, offsets, scatter; the stream's length lands at run.d_scan.
int launch_minimize_chain(rtx_ctx* ctx, const MinRun& run)
{
    const MinInput& in = run.input;
    const uint64_t n_slots = (uint64_t)in.w * in.h;
    const unsigned n_blocks = (unsigned)min_blocks(n_slots);
    uint64_t* total = (uint64_t*)run.d_scan;
    uint64_t* offsets = total + 8;
    uint32_t* sums = (uint32_t*)(offsets + n_blocks);
    hipStream_t st = ctx->stream;
    if (in.counts) RTX_HIP(ctx, hipMemsetAsync(in.counts, 0, 2 * sizeof(unsigned long long), st)); // (a delta's counters: the scatter pass adds to them)
    const int rc = with_source(ctx, in, [&](auto src) {
        using Src = decltype(src);
        const typename Src::In p = Src::input(in.data, in.prev, in.counts);
        hipLaunchKernelGGL((rtx::rtx_min_count<Src>), dim3(n_blocks), dim3(rtx::kThreads), 0, st, p, n_slots, (uint32_t)in.w, in.lead, sums);
        hipLaunchKernelGGL(rtx::rtx_min_offsets, dim3(1), dim3(rtx::kThreads), 0, st, sums, n_blocks, offsets, total);
        hipLaunchKernelGGL((rtx::rtx_min_scatter<Src>), dim3(n_blocks), dim3(rtx::kThreads), 0, st, p, n_slots, (uint32_t)in.w, in.lead, offsets, run.out);
    });
    if (rc != RTX_OK) return rc;
    RTX_HIP(ctx, hipGetLastError());
    return RTX_OK;
}

// The look-back tables of rtx_min_fused: agg (one entry per block) then 64 replicas of grp (one entry per 64 blocks); zeroed when allocated, tagged by
// epoch afterwards.  One set per context: every minimise launch runs on the context's stream, one after the other.
int ensure_look_tables(rtx_ctx* ctx, size_t n_blocks)
{
    if (ctx->look_blocks() >= n_blocks) return RTX_OK;
    // agg[cap], then 64 replicas of grp[cap / 64]: 2 cap words, cap doubled from 4096
    if (ctx->d_look.reserve_doubling(2 * n_blocks, 2 * 4096, rtxmem::after_stream(ctx->stream)) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the minimise look-back tables");
    }
    RTX_HIP(ctx, hipMemsetAsync(ctx->d_look.get(), 0, ctx->d_look.capacity() * sizeof(uint64_t), ctx->stream));
    return RTX_OK;
}

} // namespace

// Minimize of `in` into d_out on the context's stream (scratch d_scan: min_scan_bytes): one launch (rtx_min_fused,
// RTX_OPT_MINIMIZE_FUSED) or the chain.  run->d_total[0] will hold the stream's length; after a fused launch (run->epoch != 0)
// run->d_total[1] == run->epoch says that blocks gave up: settle_minimize then redoes the frame as the chain.
// (`pair`: where the one-launch form leaves the two result words instead of at d_scan -- pinned host memory as the device addresses it,
// for a caller that reads them after a synchronisation without a copy; the chain does not take it)
int launch_minimize(rtx_ctx* ctx, void* d_scan, const MinInput& in, uint8_t* d_out, MinRun* run, uint64_t* pair)
{
    *run = MinRun{in, d_out, d_scan, (uint64_t*)d_scan, 0u};
    const uint64_t n_slots = (uint64_t)in.w * in.h;
    const uint64_t n_blocks = min_blocks(n_slots);
    if (ctx->opt.min_fused == 0 || n_blocks > (1u << 24)) return launch_minimize_chain(ctx, *run);
    int rc = ensure_look_tables(ctx, (size_t)n_blocks);
    if (rc != RTX_OK) return rc;
    if (++ctx->look_epoch == 0u) {
        // the tags have wrapped: forget every entry
        RTX_HIP(ctx, hipMemsetAsync(ctx->d_look.get(), 0, 2 * ctx->look_blocks() * sizeof(uint64_t), ctx->stream));
        ctx->look_epoch = 1u;
    }
    const uint32_t epoch = ctx->look_epoch;
    uint64_t* total = pair ? pair : (uint64_t*)d_scan;
    uint64_t* agg = ctx->d_look.get();
    uint64_t* grp = agg + ctx->look_blocks();
    const uint32_t ng = (uint32_t)(ctx->look_blocks() / rtx::kLookGroup);
    const uint32_t polls = ctx->opt.min_fused == 2 ? 0u : rtx::kLookPolls;
    if (in.counts) RTX_HIP(ctx, hipMemsetAsync(in.counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
    rc = with_source(ctx, in, [&](auto src) {
        using Src = decltype(src);
        hipLaunchKernelGGL((rtx::rtx_min_fused<Src>), dim3((unsigned)n_blocks), dim3(rtx::kThreads), 0, ctx->stream, Src::input(in.data, in.prev, in.counts), n_slots,
                           (uint32_t)in.w, in.lead, agg, grp, ng, epoch, polls, d_out, total);
    });
    if (rc != RTX_OK) return rc;
    RTX_HIP(ctx, hipGetLastError());
    run->d_total = total;
    run->epoch = epoch;
    return RTX_OK;
}

// got[0], got[1]: the two words at run.d_total as the host read them after launch_minimize.  A fused launch whose blocks gave up
// is redone here as the chain (the stream is synchronised again); *total = the stream's length.
int settle_minimize(rtx_ctx* ctx, const MinRun& run, const uint64_t got[2], uint64_t* total)
{
    *total = got[0];
    if (run.epoch == 0u || got[1] != (uint64_t)run.epoch) return RTX_OK;
    ctx->stat_min_fallbacks++;
    int rc = launch_minimize_chain(ctx, run);
    if (rc != RTX_OK) return rc;
    RTX_HIP(ctx, hipMemcpyAsync(total, run.d_scan, sizeof *total, hipMemcpyDeviceToHost, ctx->stream));
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTX_OK;
}

// Minimize of `in` into d_out (nullptr: the context's buffer) with the context's scratch, the host waiting for the length.
int minimize_and_wait(rtx_ctx* ctx, const MinInput& in, void* d_out, size_t* out_bytes)
{
    int rc = ensure_min_buffers(ctx, (uint64_t)in.w * in.h, d_out == nullptr);
    if (rc != RTX_OK) return rc;
    if (!d_out) d_out = ctx->d_min.get();
    MinRun run;
    if ((rc = launch_minimize(ctx, ctx->d_scan.get(), in, (uint8_t*)d_out, &run)) != RTX_OK) return rc;
    uint64_t got[2] = {0, 0}, total = 0;
    RTX_HIP(ctx, hipMemcpyAsync(got, run.d_total, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = settle_minimize(ctx, run, got, &total)) != RTX_OK) return rc;
    *out_bytes = (size_t)total;
    return RTX_OK;
}

namespace {

// rtx_scene_set_spheres*: is [first, first + n) a run of spheres?  (Then it is a run of consecutive sphere indices too.)
int check_sphere_range(rtx_ctx* ctx, const char* who, unsigned first, size_t n)
{
    if (first > ctx->next_gidx || n > (size_t)(ctx->next_gidx - first)) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": the range goes past rtx_scene_count");
    }
    for (size_t i = 0; i < n; i++) {
        if (ctx->kind_of[first + i] != 2) {
            return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": object " + std::to_string(first + i) + " is not a sphere");
        }
    }
    return RTX_OK;
}

// an edit waits for its result: not inside a graph capture, on either stream
int check_not_capturing(rtx_ctx* ctx, const char* who, hipStream_t other)
{
    for (hipStream_t s : {ctx->stream.get(), other}) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        RTX_HIP(ctx, hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) {
            return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": not inside a graph capture (the call waits for the edit)");
        }
    }
    return RTX_OK;
}

} // namespace

int rtx_edit_spheres_here(rtx_ctx* ctx, unsigned first, size_t n, const float* rows, int src_device, bool stage, hipEvent_t after)
{
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = rtx_sync_scene(ctx);
    if (rc != RTX_OK) return rc;
    if ((rc = rtx_wait_side_builds(ctx)) != RTX_OK) return rc; // (as a physics step does)
    if (after) RTX_HIP(ctx, hipStreamWaitEvent(ctx->stream, after, 0));
    RTX_HIP(ctx, ctx->d_edit_result.reserve(2, rtxmem::nothing()));
    RTX_HIP(ctx, ctx->h_edit_result.reserve(2, rtxmem::nothing()));
    const float* d_rows = rows;
    if (src_device < 0 || stage) {
        const size_t need = 7 * n;
        // (every earlier edit has been waited for: nothing reads the old scratch)
        if (ctx->d_edit_rows.reserve_doubling(need, 7 * 1024, rtxmem::nothing()) != hipSuccess) {
            return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed while growing the scene edit scratch");
        }
        if (src_device < 0) {
            RTX_HIP(ctx, hipMemcpyAsync(ctx->d_edit_rows.get(), rows, need * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        } else {
            RTX_HIP(ctx, hipMemcpyPeerAsync(ctx->d_edit_rows.get(), ctx->device, rows, src_device, need * sizeof(float), ctx->stream));
        }
        d_rows = ctx->d_edit_rows.get();
    }
    const uint32_t k0 = ctx->local_of[first];
    const bool sorted = ctx->sorted_gen == ctx->scene_gen && ctx->d_sorted_geom.get() != nullptr;
    RTX_HIP(ctx, hipMemsetAsync(ctx->d_edit_result.get(), 0, 2 * sizeof(uint32_t), ctx->stream));
    const unsigned blocks = (unsigned)((n + rtx::kThreads - 1) / rtx::kThreads);
    hipLaunchKernelGGL(rtx::rtx_write_spheres, dim3(blocks), dim3(rtx::kThreads), 0, ctx->stream, d_rows, k0, (uint32_t)n,
                       ctx->d_sph_geom.get(), ctx->d_sph_color.get(), ctx->d_sph_od.get(),
                       sorted ? ctx->d_sorted_geom.get() : nullptr, sorted ? ctx->d_sorted_od.get() : nullptr,
                       sorted ? ctx->d_pos_of.get() : nullptr, ctx->d_edit_result.get());
    RTX_HIP(ctx, hipGetLastError());
    RTX_HIP(ctx, hipMemcpyAsync(ctx->h_edit_result.get(), ctx->d_edit_result.get(), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the one wait: the edit is applied, the rows are free, the words are here
    const uint32_t* const result = ctx->h_edit_result.get();
    const uint32_t flags = result[1];
    const rtxplan::EditEffect eff = rtxplan::edit_effect(bits_to_float(result[0]), flags);
    ctx->qgrid.dirty = true; // (the world grid lists spheres where they were)
    ctx->ns_moved_since_build = true;
    ctx->stat_scene_edits++;
    if (eff.invalidate_lists) {
        // the branch rtx_update_objects takes for its first step after an edit; scene_gen stays: object counts and array addresses
        // are what they were, recorded graphs stay valid and replay with the new values
        ctx->lists_gen++;
        ctx->cell_policy.invalidate();
        ctx->stat_edit_move_bits = 0x7f800000u;
    } else {
        ctx->stat_edit_move_bits = result[0];
    }
    ctx->scene_drift += eff.drift_add;
    if (eff.unsettle_physics) ctx->physics_settled = false;
    if (src_device < 0) {
        // the sort's input at the next re-sort.  The device form leaves h_centres as they are: the order is a speed matter only
        // (ties are broken by creation index in any order), and the rows never come to the host
        for (size_t i = 0; i < n && (size_t)k0 + i < ctx->h_centres.size(); i++) {
            ctx->h_centres[(size_t)k0 + i] = make_float4(rows[7 * i], rows[7 * i + 1], rows[7 * i + 2], rows[7 * i + 3]);
        }
    }
    return RTX_OK;
}

// Everything of a removal that can fail for want of memory, before anything is moved: pending appends uploaded, the second set of
// arrays and the list buffer large enough.  Changes nothing a launch reads; a device group prepares every member before the first
// one compacts, so that running out of memory leaves every replica as it was.
int rtx_remove_prepare(rtx_ctx* ctx, const std::vector<uint32_t>& ascending)
{
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = rtx_sync_scene(ctx); // every pending append is on the device: ns_uploaded == ns, np_uploaded == np
    if (rc != RTX_OK) return rc;
    const size_t n = ascending.size();
    const DeviceBuf<float4>* const live[8] = {&ctx->d_sph_geom, &ctx->d_sph_motion, &ctx->d_sph_color, &ctx->d_sph_od,
                                              &ctx->d_pl_a,     &ctx->d_pl_b,       &ctx->d_pl_c,      &ctx->d_pl_od};
    for (int a = 0; a < 8; a++) {
        // (every earlier removal has been waited for, and no launch reads a spare set)
        if (ctx->d_spare[a].reserve(live[a]->capacity(), rtxmem::nothing()) != hipSuccess) {
            return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed while growing the second set of scene arrays");
        }
    }
    // the lists: R, then the removed sphere locals, then the removed plane locals -- 2 |R| words
    if (ctx->d_remove_lists.reserve_doubling(2 * n, 1024, rtxmem::nothing()) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed while growing the removal lists");
    }
    return RTX_OK;
}

int rtx_remove_objects_here(rtx_ctx* ctx, const std::vector<uint32_t>& ascending)
{
    int rc = rtx_remove_prepare(ctx, ascending); // (nothing left to do where a group has prepared this member already)
    if (rc != RTX_OK) return rc;
    if ((rc = rtx_wait_side_builds(ctx)) != RTX_OK) return rc; // (as an edit does)
    rtxplan::RemovalPlan plan = rtxplan::plan_removal(ctx->kind_of, ascending);
    const size_t n = ascending.size();
    // the kernel's argument order: the two plain arrays of a kind, then the two that carry the creation index in .w
    DeviceBuf<float4>* const live[8] = {&ctx->d_sph_geom, &ctx->d_sph_motion, &ctx->d_sph_color, &ctx->d_sph_od,
                                        &ctx->d_pl_a,     &ctx->d_pl_b,       &ctx->d_pl_c,      &ctx->d_pl_od};
    const bool moves[2] = {plan.ns > 0, plan.np > 0}; // (a kind without survivors has nothing to move: its count drops to 0)
    std::vector<uint32_t> lists(ascending);
    lists.insert(lists.end(), plan.removed_spheres.begin(), plan.removed_spheres.end());
    lists.insert(lists.end(), plan.removed_planes.begin(), plan.removed_planes.end());
    const uint32_t* d_gidx = ctx->d_remove_lists.get();
    const uint32_t* d_local[2] = {d_gidx + n, d_gidx + n + plan.removed_spheres.size()};
    const uint32_t n_local[2] = {(uint32_t)plan.removed_spheres.size(), (uint32_t)plan.removed_planes.size()};
    const uint32_t count[2] = {ctx->ns, ctx->np};
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_remove_lists.get(), lists.data(), lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    for (int kind = 0; kind < 2; kind++) {
        if (!moves[kind]) continue;
        DeviceBuf<float4>* const* from = live + 4 * kind;
        const DeviceBuf<float4>* to = ctx->d_spare + 4 * kind;
        hipLaunchKernelGGL(rtx::rtx_compact_objects, dim3((count[kind] + rtx::kThreads - 1) / rtx::kThreads), dim3(rtx::kThreads), 0, ctx->stream,
                           (const float4*)from[0]->get(), (const float4*)from[1]->get(), (const float4*)from[2]->get(), (const float4*)from[3]->get(),
                           to[0].get(), to[1].get(), to[2].get(), to[3].get(), count[kind], d_gidx, (uint32_t)n,
                           d_local[kind], n_local[kind]);
        RTX_HIP(ctx, hipGetLastError());
    }
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the one wait: the survivors are in the second set, the lists are free
    for (int a = 0; a < 8; a++) {
        if (moves[a / 4]) live[a]->swap(ctx->d_spare[a]);
    }
    // the books, all in one place: what a context holds to which the survivors were added in their order
    ctx->materials.remove(ascending); // (no reflective object left: the mirror path is simply not taken any more)
    if (ctx->h_centres.size() == ctx->ns) {
        // the sort's input at the next re-sort, by sphere index
        size_t kept = 0, gone = 0;
        for (size_t k = 0; k < ctx->h_centres.size(); k++) {
            if (gone < plan.removed_spheres.size() && plan.removed_spheres[gone] == k) {
                gone++;
            } else {
                ctx->h_centres[kept++] = ctx->h_centres[k];
            }
        }
        ctx->h_centres.resize(kept);
    }
    ctx->kind_of.swap(plan.kind_of);
    ctx->local_of.swap(plan.local_of);
    ctx->ns = ctx->ns_uploaded = plan.ns;
    ctx->np = ctx->np_uploaded = plan.np;
    ctx->next_gidx = plan.ns + plan.np;
    ctx->scene_drift += 1.0e3; // (an edit: every dispatch order is stale)
    // scene and list generations, view density, physics bound, cell policy, world grid: counts and addresses changed, so the sorted
    // copy is re-sorted, cell lists and grid are rebuilt and recorded graphs are refused, exactly as after rtx_scene_add_*
    rtx_scene_edited(ctx);
    ctx->stat_scene_removed += n;
    return RTX_OK;
}

namespace {

// R is checked and not empty: the context itself, then the other members of its group
int remove_checked(rtx_ctx* ctx, const std::vector<uint32_t>& ascending)
{
    // on a group: every member's memory first, then the moves -- running out of memory touches no replica
    int rc = ctx->group ? rtxgroup::scene_remove_prepare(ctx, ascending) : RTX_OK;
    if (rc != RTX_OK) return rc;
    if ((rc = rtx_remove_objects_here(ctx, ascending)) != RTX_OK) return rc;
    return ctx->group ? rtxgroup::scene_remove_objects(ctx, ascending) : RTX_OK;
}

} // namespace

extern "C" {

int rtx_scene_remove_objects(rtx_ctx* ctx, size_t n, const unsigned* indices)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    if (n && !indices) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_remove_objects: the indices are NULL");
    if (n == 0) return RTX_OK;
    // all or nothing: the set is checked before anything is touched (and, on a group, before any rank is)
    std::vector<uint32_t> ascending;
    const size_t bad = rtxplan::removal_fault(ctx->next_gidx, n, indices, ascending);
    if (bad < n) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT,
                        "rtx_scene_remove_objects: index " + std::to_string(indices[bad]) + " (entry " + std::to_string(bad) + ") " +
                            (indices[bad] >= ctx->next_gidx ? "is past rtx_scene_count" : "is listed twice"));
    }
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = check_not_capturing(ctx, "rtx_scene_remove_objects", ctx->stream);
    if (rc != RTX_OK) return rc;
    return remove_checked(ctx, ascending);
}

int rtx_scene_remove_marked_device(rtx_ctx* ctx, const uint8_t* d_marks, void* stream_v, size_t* n_removed)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    const size_t count = ctx->next_gidx;
    if (count == 0) {
        if (n_removed) *n_removed = 0;
        return RTX_OK;
    }
    if (!d_marks) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_remove_marked_device: the marks are NULL");
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_v ? (hipStream_t)stream_v : ctx->stream;
    int rc = check_not_capturing(ctx, "rtx_scene_remove_marked_device", st);
    if (rc != RTX_OK) return rc;
    // (every earlier copy of marks has been waited for)
    if (ctx->h_remove_marks.reserve_doubling(count, 4096, rtxmem::nothing()) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipHostMalloc failed while growing the removal marks");
    }
    // after everything queued so far on the caller's stream (the kernel that wrote the marks); the first of the two waits
    RTX_HIP(ctx, hipMemcpyAsync(ctx->h_remove_marks.get(), d_marks, count, hipMemcpyDeviceToHost, st));
    RTX_HIP(ctx, hipStreamSynchronize(st));
    std::vector<uint32_t> ascending;
    for (size_t i = 0; i < count; i++) {
        if (ctx->h_remove_marks.get()[i]) ascending.push_back((uint32_t)i);
    }
    if (!ascending.empty() && (rc = remove_checked(ctx, ascending)) != RTX_OK) return rc;
    if (n_removed) *n_removed = ascending.size();
    return RTX_OK;
}

int rtx_scene_set_spheres(rtx_ctx* ctx, unsigned first, size_t n, const float* xyzr_rgb)
{
    if (!ctx || (n && !xyzr_rgb)) return ctx ? rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_spheres: the rows are NULL") : RTX_ERR_INVALID_ARGUMENT;
    // all or nothing: the range is checked before anything is touched (and, on a group, before any rank is)
    int rc = check_sphere_range(ctx, "rtx_scene_set_spheres", first, n);
    if (rc != RTX_OK || n == 0) return rc;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = check_not_capturing(ctx, "rtx_scene_set_spheres", ctx->stream)) != RTX_OK) return rc;
    if ((rc = rtx_edit_spheres_here(ctx, first, n, xyzr_rgb, -1, false, nullptr)) != RTX_OK) return rc;
    return ctx->group ? rtxgroup::scene_set_spheres(ctx, first, n, xyzr_rgb) : RTX_OK;
}

int rtx_scene_set_spheres_device(rtx_ctx* ctx, unsigned first, size_t n, const float* d_xyzr_rgb, void* stream_v)
{
    if (!ctx || (n && !d_xyzr_rgb)) return ctx ? rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_spheres_device: the rows are NULL") : RTX_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_xyzr_rgb & 3u) != 0) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_spheres_device: the rows must be 4-byte aligned");
    int rc = check_sphere_range(ctx, "rtx_scene_set_spheres_device", first, n);
    if (rc != RTX_OK || n == 0) return rc;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_v ? (hipStream_t)stream_v : ctx->stream;
    if ((rc = check_not_capturing(ctx, "rtx_scene_set_spheres_device", st)) != RTX_OK) return rc;
    // after everything queued so far on the caller's stream (the kernel that wrote the rows); a group's members wait for it too
    hipEvent_t after = nullptr;
    if (st != ctx->stream || ctx->group) {
        RTX_HIP(ctx, ctx->ev_edit.ensure());
        RTX_HIP(ctx, hipEventRecord(ctx->ev_edit, st));
        after = ctx->ev_edit;
    }
    if ((rc = rtx_edit_spheres_here(ctx, first, n, d_xyzr_rgb, ctx->device, false, st != ctx->stream ? after : nullptr)) != RTX_OK) return rc;
    return ctx->group ? rtxgroup::scene_set_spheres_device(ctx, first, n, d_xyzr_rgb, after) : RTX_OK;
}

int rtx_scene_set_plane(rtx_ctx* ctx, unsigned index, const float pos[3], const float normal[3], const float rgb[3], float width, float height)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    if (!pos || !normal || !rgb) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_plane: a NULL argument");
    if (index >= ctx->next_gidx || ctx->kind_of[index] != 1) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_plane: object " + std::to_string(index) + " is not a plane");
    }
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = check_not_capturing(ctx, "rtx_scene_set_plane", ctx->stream);
    if (rc != RTX_OK) return rc;
    if ((rc = rtx_sync_scene(ctx)) != RTX_OK) return rc;
    // what rtx_scene_add_plane stores: the safe host normalise of Plane::Plane (Plane.cu:6-12, MyMath.h:117-123), od by the same
    // IEEE division, the creation index kept in the .w words
    const float length = std::sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
    const float divider = length < 0.000001f ? 0.0f : 1.0f / length;
    const float4 a = make_float4(pos[0], pos[1], pos[2], width);
    const float4 b = make_float4(normal[0] * divider, normal[1] * divider, normal[2] * divider, height);
    const float4 c = make_float4(rgb[0], rgb[1], rgb[2], bits_to_float(index));
    const float4 od = make_float4(rgb[0] / 255.0f, rgb[1] / 255.0f, rgb[2] / 255.0f, bits_to_float(index));
    const uint32_t k = ctx->local_of[index];
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_pl_a.get() + k, &a, sizeof a, hipMemcpyHostToDevice, ctx->stream));
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_pl_b.get() + k, &b, sizeof b, hipMemcpyHostToDevice, ctx->stream));
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_pl_c.get() + k, &c, sizeof c, hipMemcpyHostToDevice, ctx->stream));
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_pl_od.get() + k, &od, sizeof od, hipMemcpyHostToDevice, ctx->stream));
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // Cell lists hold spheres only and stay valid; the dispatch orders' estimates are stale.  qgrid.dirty is left as it is: the
    // world grid (rtx_grid.hpp, the build in rtx_query.cpp) lists spheres and takes its bounds from spheres alone -- the query and
    // shadow kernels read the plane arrays themselves at every launch, so nothing of a plane is cached in it.
    ctx->scene_drift += 1.0e3;
    ctx->stat_scene_edits++;
    return ctx->group ? rtxgroup::scene_set_plane(ctx, index, pos, normal, rgb, width, height) : RTX_OK;
}

int rtx_update_objects(rtx_ctx* ctx, double dt)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = rtx_sync_scene(ctx);
    if (rc != RTX_OK) return rc;
    if (ctx->ns == 0) return RTX_OK;
    if ((rc = rtx_wait_side_builds(ctx)) != RTX_OK) return rc;
    const unsigned blocks = (ctx->ns + rtx::kThreads - 1) / rtx::kThreads;
    const bool sorted = ctx->sorted_gen == ctx->scene_gen && ctx->d_sorted_geom.get() != nullptr;
    hipLaunchKernelGGL(rtx::rtx_update_spheres, dim3(blocks), dim3(rtx::kThreads), 0, ctx->stream,
                       ctx->d_sph_geom.get(), ctx->d_sph_motion.get(), ctx->ns, dt, sorted ? ctx->d_sorted_geom.get() : nullptr,
                       sorted ? ctx->d_pos_of.get() : nullptr);
    RTX_HIP(ctx, hipGetLastError());
    ctx->ns_moved_since_build = true;
    ctx->qgrid.dirty = true; // (the world grid lists spheres where they were)
    // How far a sphere can have moved (dispatch orders age with it; cell lists are valid within it: rtx_plan.hpp).  A step
    // moves a sphere by at most |speed dt| -- the clamp to [-10, 10] only shortens the move -- once it has been through one
    // step; the FIRST step after an edit may pull a sphere from anywhere onto +-10 (Sphere.cu:18-22), so it counts as
    // an edit.  A dt that is not a number moves spheres to NaN: an edit as well.
    const double step = std::fabs(dt) * (double)ctx->max_speed;
    if (!ctx->physics_settled || !(step == step) || !(step < 1.0e30)) {
        ctx->lists_gen++; // (object counts and array addresses are what they were: recorded graphs stay valid)
        ctx->cell_policy.invalidate();
        ctx->physics_settled = (step == step) && (step < 1.0e30);
        ctx->scene_drift += 1.0e3;
    } else {
        ctx->scene_drift += step + 2.0e-6; // (+ the rounding of y to float: half an ulp of 10)
    }
    return ctx->group ? rtxgroup::update_objects(ctx, dt) : RTX_OK; // every rank steps its replica: the same arithmetic on the same values
}

void* rtx_minimized_device_ptr(rtx_ctx* ctx) { return ctx ? ctx->d_min.get() : nullptr; }

int rtx_ansi256_map(rtx_ctx* ctx, uint32_t first_rgb, size_t count, void* d_out, void* stream_v)
{
    if (!ctx || (count && !d_out)) return RTX_ERR_INVALID_ARGUMENT;
    if ((uint64_t)first_rgb + (uint64_t)count > (1ull << 24)) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_ansi256_map: range exceeds 2^24 colours");
    if (count == 0) return RTX_OK;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_v ? (hipStream_t)stream_v : ctx->stream;
    const uint64_t threads = ((uint64_t)count + 3u) / 4u;
    const unsigned blocks = (unsigned)((threads + rtx::kThreads - 1) / rtx::kThreads);
    hipLaunchKernelGGL(rtx::rtx_ansi_map, dim3(blocks), dim3(rtx::kThreads), 0, st, first_rgb, (uint64_t)count, ctx->d_grey.get(), (uint8_t*)d_out);
    RTX_HIP(ctx, hipGetLastError());
    return RTX_OK;
}

int rtx_minimize(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_in, void* d_out, size_t* out_bytes)
{
    if (!ctx || !out_bytes) return RTX_ERR_INVALID_ARGUMENT;
    if (mode < RTX_BIT_ASCII || mode > RTX_SDL) return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "invalid rendering mode");
    if (w == 0 || h == 0 || w >= (1ull << 31) || h >= (1ull << 31)) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "w/h must be in [1, 2^31)");
    if (!d_in) {
        if (20 * w * h > ctx->capacity) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, "frame larger than the context was created for");
        d_in = ctx->d_frame.get();
    }
    if (((uintptr_t)d_in & 15u) != 0 || (d_out && ((uintptr_t)d_out & 15u) != 0)) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "minimise buffers must be 16-byte aligned");
    }
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    if (!d_out && 20 * w * h > ctx->capacity) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, "minimise output larger than the context's buffer");
    return minimize_and_wait(ctx, records_input(mode, w, h, d_in), d_out, out_bytes);
}

int rtx_minimize_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_words, void* d_out, size_t* out_bytes)
{
    if (!ctx || !out_bytes || !d_words) return RTX_ERR_INVALID_ARGUMENT;
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL) return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "rtx_minimize_words: not a character mode");
    if (w == 0 || h == 0 || w >= (1ull << 31) || h >= (1ull << 31)) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "w/h must be in [1, 2^31)");
    if (((uintptr_t)d_words & 3u) != 0 || (d_out && ((uintptr_t)d_out & 15u) != 0)) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_minimize_words: words must be 4-byte, the output 16-byte aligned");
    }
    if (!d_out && 20 * w * h > ctx->capacity) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, "minimise output larger than the context's buffer");
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    return minimize_and_wait(ctx, words_input(mode, w, h, d_words), d_out, out_bytes);
}

size_t rtx_delta_bound(int mode, size_t w, size_t h)
{
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL || w == 0 || h == 0 || w - 1 > rtxplan::kDeltaMaxIndex || h > rtxplan::kDeltaMaxIndex) return 0;
    const size_t S = mode >= RTX_RGB_ASCII ? RTX_SIZE_RGB : RTX_SIZE_8BIT;
    return std::max(rtxplan::delta_bound(S, w, h), S * w * h); // (a key frame of rtx_update_delta: Minimize's S W H)
}

int rtx_delta_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_cur, const void* d_prev, void* d_out, size_t out_capacity, size_t* out_bytes)
{
    if (!ctx || !out_bytes || !d_cur || !d_prev || !d_out) return RTX_ERR_INVALID_ARGUMENT;
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL) return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "rtx_delta_words: not a character mode");
    if (w == 0 || h == 0 || w - 1 > rtxplan::kDeltaMaxIndex || h > rtxplan::kDeltaMaxIndex) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_delta_words: w - 1 and h must be in [0, 99999], h and w at least 1");
    }
    if ((((uintptr_t)d_cur | (uintptr_t)d_prev) & 3u) != 0 || ((uintptr_t)d_out & 15u) != 0) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_delta_words: words must be 4-byte, the output 16-byte aligned");
    }
    if (out_capacity < rtx_delta_bound(mode, w, h)) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, "rtx_delta_words: the output holds less than rtx_delta_bound");
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long* counts = nullptr;
    const int rc = rtx_delta_counters(ctx, &counts);
    if (rc != RTX_OK) return rc;
    return minimize_and_wait(ctx, delta_input(mode, w, h, d_cur, d_prev, counts), d_out, out_bytes);
}

size_t rtx_half_bound(int mode, size_t w, size_t h)
{
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL || w == 0 || h == 0 || w >= (1ull << 31) || h >= (1ull << 30)) return 0;
    return rtxplan::half_bound(mode >= RTX_RGB_ASCII ? rtxplan::kHalfEscRgb : rtxplan::kHalfEsc8, w, h); // (0 where it does not fit size_t)
}

int rtx_half_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_words, void* d_out, size_t out_capacity, size_t* out_bytes)
{
    if (!ctx || !out_bytes || !d_words || !d_out) return RTX_ERR_INVALID_ARGUMENT;
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL) return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "rtx_half_words: not a character mode");
    const size_t bound = rtx_half_bound(mode, w, h);
    if (bound == 0) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_half_words: w and 2 h must be in [1, 2^31)");
    if (((uintptr_t)d_words & 3u) != 0 || ((uintptr_t)d_out & 15u) != 0) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_half_words: words must be 4-byte, the output 16-byte aligned");
    }
    if (out_capacity < bound) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, "rtx_half_words: the output holds less than rtx_half_bound");
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    return minimize_and_wait(ctx, half_input(mode, w, h, d_words), d_out, out_bytes);
}

size_t rtx_half_delta_bound(int mode, size_t w, size_t h)
{
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL) return 0;
    return rtxplan::half_delta_bound(mode >= RTX_RGB_ASCII ? rtxplan::kHalfEscRgb : rtxplan::kHalfEsc8, w, h); // (0 for what the calls refuse)
}

int rtx_half_delta_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_cur, const void* d_prev, void* d_out, size_t out_capacity, size_t* out_bytes)
{
    if (!ctx || !out_bytes || !d_cur || !d_prev || !d_out) return RTX_ERR_INVALID_ARGUMENT;
    if (mode < RTX_BIT_ASCII || mode >= RTX_SDL) return rtx_fail(ctx, RTX_ERR_INVALID_MODE, "rtx_half_delta_words: not a character mode");
    const size_t bound = rtx_half_delta_bound(mode, w, h);
    if (bound == 0) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_half_delta_words: w - 1 and h must be in [0, 99999], h and w at least 1");
    if ((((uintptr_t)d_cur | (uintptr_t)d_prev) & 3u) != 0 || ((uintptr_t)d_out & 15u) != 0) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_half_delta_words: words must be 4-byte, the output 16-byte aligned");
    }
    if (out_capacity < bound) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, "rtx_half_delta_words: the output holds less than rtx_half_delta_bound");
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long* counts = nullptr;
    const int rc = rtx_delta_counters(ctx, &counts);
    if (rc != RTX_OK) return rc;
    return minimize_and_wait(ctx, half_delta_input(mode, w, h, d_cur, d_prev, counts), d_out, out_bytes);
}

} // extern "C"


// ---- the direction-sorted copy of the sphere array (what KArgs::sph_geom and sph_od point at for the trace kernels): spheres ordered by a Morton code of the direction
// (azimuth, elevation) in which they lie from `origin` -- the camera's position at the first launch after a scene edit -- so that
// the spheres of a coarse cell, or of a macro tile's pyramid, are neighbours in memory.  Host-side sort (rtxplan::direction_order)
// over the positions the spheres were created with (physics moves them by a few units at most: the order stays good enough),
// then one gather on the device from the live arrays.
int rtx_sort_scene(rtx_ctx* ctx, const float origin[3])
{
    const uint32_t ns = ctx->ns;
    if (ns == 0 || ctx->h_centres.size() != ns) return RTX_OK;
    std::vector<uint32_t> order, pos_of;
    rtxplan::direction_order(&ctx->h_centres[0].x, sizeof(float4) / sizeof(float), ns, origin, order, pos_of);
    // (a scene edit: nothing may still read the old copy)
    RTX_HIP(ctx, hipDeviceSynchronize());
    // no sorted copy where memory is short: staging reads the scene array (sorted_gen stays behind)
    if (ctx->d_sorted_geom.reserve_doubling(ns, 1024, rtxmem::nothing()) != hipSuccess || ctx->d_sorted_od.reserve_doubling(ns, 1024, rtxmem::nothing()) != hipSuccess ||
        ctx->d_sorted_idx.reserve_doubling(ns, 1024, rtxmem::nothing()) != hipSuccess || ctx->d_pos_of.reserve_doubling(ns, 1024, rtxmem::nothing()) != hipSuccess) {
        return RTX_OK;
    }
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_sorted_idx.get(), order.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    RTX_HIP(ctx, hipMemcpyAsync(ctx->d_pos_of.get(), pos_of.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(rtx::rtx_gather_spheres, dim3((ns + rtx::kThreads - 1) / rtx::kThreads), dim3(rtx::kThreads), 0, ctx->stream,
                       ctx->d_sph_geom.get(), ctx->d_sph_od.get(), ctx->d_sorted_idx.get(),
                       ctx->d_sorted_geom.get(), ctx->d_sorted_od.get(), ns);
    RTX_HIP(ctx, hipGetLastError());
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the staging vectors go out of scope; other streams may render next)
    ctx->sorted_gen = ctx->scene_gen;
    ctx->h_sorted_idx.swap(order);
    ctx->materials.order_changed(); // the attributes by sorted position follow this order (rtx_render.cpp, upload_materials)
    return RTX_OK;
}
