// rtx_ctx.h -- the context behind the C ABI, shared by rtx_api.cpp, rtx_post.hip, rtx_update.cpp and the other host files.
#pragma once

#include "../../include/rtx.h"
#include "rtx_kernels.h"
#include "rtx_materials.hpp"
#include "rtx_mem.hpp"
#include "rtx_options.hpp"
#include "rtx_plan.hpp"
#include "rtx_sync.hpp"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

using rtxmem::Counter;
using rtxmem::DeviceBuf;
using rtxmem::Event;
using rtxmem::PinnedBuf;
using rtxmem::Stream;

struct HostPlane {
    float4 a, b, c, od;
};

// RayTracing.cu:143-157: the one light of the reference, a constant at the BlinnPhongShading call site
inline rtx_light rtx_reference_light()
{
    rtx_light l;
    l.pos[0] = 1.0f;
    l.pos[1] = 50.0f;
    l.pos[2] = 0.0f;
    for (int k = 0; k < 3; k++) l.diffuse_rgb[k] = l.specular_rgb[k] = 1.0f;
    l.diffuse_power = 2000.0f;
    l.specular_power = 3000.0f;
    return l;
}

struct rtx_group; // rtx_group.cpp: the device group a context is the root of

// One Minimize (rtx_post.hip): its input, a W*H frame as records or as pixel words (`lead`: how many words before `data` belong to
// the same frame: rtx_post_kernels.inc) ...
struct MinInput {
    int mode = 0;
    size_t w = 0, h = 0;
    bool words = false; // data: pixel words, else S-byte records
    const void* data = nullptr;
    uint32_t lead = 0;
    // a delta (rtx_delta_words): `data` is the current frame's words, `prev` the previous frame's, `counts` the launch's two counters
    const void* prev = nullptr;
    void* counts = nullptr;
    // a half-block frame (rtx_half_words): `data` is W * 2h pixel words, w x h the cells
    bool half = false;
};

// ... and, once launched, where it writes and where its result words are.
struct MinRun {
    MinInput input;
    uint8_t* out = nullptr;
    void* d_scan = nullptr;      // the chain's scratch
    uint64_t* d_total = nullptr; // [0] the stream's length, [1] the failure word of a fused launch
    uint32_t epoch = 0;          // not 0: a fused launch under this epoch
};

inline MinInput records_input(int mode, size_t w, size_t h, const void* d_records) { return MinInput{mode, w, h, false, d_records, 0u}; }

inline MinInput words_input(int mode, size_t w, size_t h, const void* d_words, uint32_t lead = 0) { return MinInput{mode, w, h, true, d_words, lead}; }

inline MinInput delta_input(int mode, size_t w, size_t h, const void* d_cur, const void* d_prev, void* d_counts) { return MinInput{mode, w, h, true, d_cur, 0u, d_prev, d_counts}; }

// (w x h: the cells; d_words: w x 2h pixel words)
inline MinInput half_input(int mode, size_t w, size_t h, const void* d_words) { return MinInput{mode, w, h, true, d_words, 0u, nullptr, nullptr, true}; }

// (a delta of two half-block frames, rtx_half_delta_words: both marks -- `half` with `prev` and `counts`)
inline MinInput half_delta_input(int mode, size_t w, size_t h, const void* d_cur, const void* d_prev, void* d_counts) { return MinInput{mode, w, h, true, d_cur, 0u, d_prev, d_counts, true}; }

// bit casts (the creation index of an object travels in the .w of its float4s)
inline float bits_to_float(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

inline uint32_t float_to_bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// Every buffer, event and stream below is an owner (rtx_mem.hpp): it goes with the context, or with the set it is a member of.  Who
// waits for what before outgrown storage is freed is said where it grows; DESIGN.md 3, "Ownership".
struct rtx_ctx {
    int device = 0;
    rtx_group* group = nullptr;     // not null: this context is the root of a device group (rtx_group_create)
    Stream stream;                  // (declared first: destroyed after everything that was queued on it is gone)
    Event ev_start, ev_stop;        // (with timing: rtx_timer_*)
    size_t max_w = 0, max_h = 0, capacity = 0;
    rtxopt::Options opt;            // what rtx_set_option stores (rtx_options.hpp; a group's own four: rtx_group.cpp)
    DeviceBuf<uint8_t> d_frame;
    DeviceBuf<uint8_t> d_min;       // minimise output (allocated on first use)
    DeviceBuf<uint8_t> d_scan;      // minimise scratch (bytes)
    DeviceBuf<uint32_t> d_words;    // rtx_update's pixel words (W * H; allocated on first use)
    uint64_t stat_host_writes = 0;
    PinnedBuf<uint64_t> h_pair;     // two pinned words: a rank's stream length and failure word (rtx_update on a group, RTX_OPT_GROUP_UPDATE)
    DeviceBuf<uint64_t> d_look;     // rtx_min_fused's look-back tables (agg, grp: rtx_post.hip), zeroed when allocated
    size_t look_blocks() const { return d_look.capacity() / 2; } // ... sized for this many blocks
    uint32_t look_epoch = 0;        // of the last fused launch (0: none yet; never used as a tag)
    uint64_t stat_min_fallbacks = 0; // fused minimise launches that gave up and were redone as three launches
    DeviceBuf<uint8_t> d_grey;
    size_t dirty_hi = 0;            // bytes of d_frame that may be non-zero

    // scene: host staging for objects not yet uploaded + device SoA (the device copy is the truth
    // once uploaded, because UpdateObjects moves spheres there)
    std::vector<float4> h_sph_geom, h_sph_color, h_sph_od, h_sph_motion;
    std::vector<HostPlane> h_planes;
    uint32_t ns = 0, np = 0, next_gidx = 0;
    uint32_t ns_uploaded = 0, np_uploaded = 0;
    DeviceBuf<float4> d_sph_geom, d_sph_color, d_sph_od, d_sph_motion, d_pl_a, d_pl_b, d_pl_c, d_pl_od;
    // the direction-sorted copy of the sphere array that staging reads (rtx_sort_scene): geometry by sorted position, sorted
    // position -> sphere index, sphere index -> sorted position; valid while sorted_gen == scene_gen
    DeviceBuf<float4> d_sorted_geom, d_sorted_od;
    DeviceBuf<uint32_t> d_sorted_idx, d_pos_of;
    std::vector<float4> h_centres;  // cx cy cz r as created, by sphere index (the sort's input; the device copy moves under physics)
    uint64_t sorted_gen = 0;
    std::vector<uint8_t> kind_of;   // per creation index: 1 plane, 2 sphere (Object3D.h:14)
    std::vector<uint32_t> local_of; // per creation index: index within its kind

    // two-level culling scratch, one set per stream that renders (launches on one stream are ordered, so a
    // set is never shared by frames in flight on different streams)
    struct CellScratch {
        hipStream_t stream = nullptr;
        DeviceBuf<uint32_t> list;                 // cells x capacity sphere indices
        DeviceBuf<uint32_t> count;                // two alternating buffers of one counter per cell
        uint32_t n_cells = 0;                     // the cell grid the counters were last zeroed for
        uint32_t flip = 0;                        // which counter buffer the next launch accumulates into
    };
    std::vector<CellScratch> cell_scratch;

    // dispatch order of the macro tiles, one set per (render stream, tile grid): everything that touches a set is queued
    // on that one stream, in order (trace writes the estimates, rtx_order_tiles turns them into the order the following
    // traces read) or on the context's side stream behind events (rtx_balance_tiles).  The decisions are
    // rtxplan::DispatchOrder's; this holds the buffers and events.
    struct TileOrder {
        hipStream_t stream = nullptr;
        uint64_t key[3] = {0, 0, 0}; // identifies the tile grid the buffers describe
        DeviceBuf<uint32_t> cost;
        DeviceBuf<uint32_t> order;   // two orders of `cap` tiles: the one in use and the one a balancing pass writes
        DeviceBuf<float> factor;     // per-tile correction of the estimate (rtx_balance_tiles)
        Event ev_rec, ev_done;
        size_t cap() const { return factor.capacity(); } // tiles the buffers hold
        uint64_t last_use = 0;       // ctx->order_clock at the last launch (least recently used set is recycled)
        bool frozen = false;         // a recorded (HIP graph) launch reads the order in use: nothing is derived for this set any more
        uint32_t frozen_refs = 0;    // ... by this many live graphs (rtx_graph_destroy of the last one releases the set)
        uint64_t id = 0;             // stable name of the set (the vector's entries move)
        bool batch = false;          // the set of a batched launch (rtx_trace_batch): plain heaviest first, nothing dealt
        const uint32_t* base = nullptr; // the static XCD-aware order of the launch in hand, or nullptr (rtx_order_tiles sorts per XCD label within it)
        rtxplan::DispatchOrder plan;
    };
    std::vector<TileOrder> tile_orders;
    uint64_t order_clock = 0, next_order_id = 1;
    std::vector<uint64_t> capture_frozen; // ids of the sets the capture in progress has frozen (handed to the graph by rtx_graph_end)

    // Coarse-cell lists that outlive a frame (two-level culling): two sets, shared by all render streams, each valid for
    // cameras within the motion budget it was binned with (rtxplan::CellCachePolicy).  A set is (re)built on the render
    // stream that missed, or ahead of time on the side stream; who waits for whom is `sync`'s contract (rtx_sync.hpp): a rebuild
    // waits for each stream's last launch that read the set -- not for everything the render streams have queued since, which
    // would drain the frames in flight at every rebuild.
    struct CellCacheSlot {
        DeviceBuf<uint32_t> list, count;
        rtxsync::Shared sync;
        bool built_on_aux = false;              // the last build ran on the side stream
    };
    CellCacheSlot cell_cache[2];
    rtxplan::CellCachePolicy cell_policy;
    // capacity feedback: the binning passes keep the longest list needed in d_cell_max; it is copied to the pinned word
    // h_cell_max after a build (and now and then on the per-frame path) and read, unsynchronised, when the next launch is planned
    DeviceBuf<uint32_t> d_cell_max;
    PinnedBuf<volatile uint32_t> h_cell_max;
    uint32_t cell_cap_floor = 0;                // capacity the lists of the current grid are planned with at least
    uint64_t cell_grid_id[3] = {0, 0, 0};       // the grid (and scene generation) the two words above belong to
    uint64_t per_frame_bins = 0;
    struct XcdOrder {                           // static dispatch order of a two-level grid: a cell's tiles share an XCD
        DeviceBuf<uint32_t> p;
        uint64_t key[2] = {0, 0};               // (tile grid, cell shape)
        uint64_t last_use = 0;
    };
    XcdOrder xcd_orders[4];                     // the grids seen last (least recently used is replaced)
    // view-density feedback (rtxplan::ViewDensity): the longest candidate list the trace workgroups of an epoch (8 culling
    // launches) report, copied to the pinned word when the epoch ends and taken as an observation once that copy has landed
    DeviceBuf<uint32_t> d_longest;              // three words in rotation: the epoch being filled, the next one (zeroed), the one before (being copied)
    PinnedBuf<volatile uint32_t> h_longest;
    Event ev_longest;
    bool longest_copy_pending = false;
    uint32_t longest_epoch = 0, longest_launches = 0;
    rtxplan::ViewDensity view_density;
    uint64_t stat_density_switches = 0;
    hipStream_t recent_streams[16] = {nullptr}; // the render streams of the last two-level launches
    unsigned recent_pos = 0, render_streams_seen = 0;
    Event ev_physics;                           // orders a build on the side stream after the physics steps queued so far
    bool ns_moved_since_build = false;          // rtx_update_objects ran since the last such ordering
    uint64_t scene_gen = 1;                     // bumped by every scene edit: object counts / array addresses (recorded graphs belong to one)
    uint64_t lists_gen = 1;                     // ... and by the first physics step after one: what cell lists belong to
    bool physics_settled = false;               // every sphere has been through Sphere::Update since the last edit (|y| <= 10)
    uint64_t stat_order_passes = 0;
    uint64_t stat_cell_builds = 0, stat_cell_prefetches = 0, stat_cell_hits = 0, stat_cell_per_frame = 0;

    Stream aux_stream;                // the balancing passes' stream (created with the first pass)
    double scene_drift = 0.0;        // how far any sphere can have moved since the context was created (rtx_update_objects:
                                     // |dt| x the largest |speed x mover|; rtx_scene_set_spheres: the largest move; other scene edits and removals add 1e3):
                                     // dispatch orders go stale with it
    float max_speed = 0.0f;          // largest |speed * mover| any sphere was given: what a physics step moves it by per unit of dt
    uint64_t stat_batched_launches = 0;
    int n_cu = 0;                   // compute units of the device

    // events of rtx_submit_slabs' fork/join: one for `after`, one per distinct render stream seen
    Event ev_fork;
    struct JoinEvent {
        hipStream_t stream = nullptr;
        Event ev;
    };
    std::vector<JoinEvent> join_events;

    // pipelined Update (rtx_update_begin / rtx_update_end; rtx_update.cpp): two slots, each with its own frame, minimise
    // buffer, scan scratch and events; the copy of slot k's stream to the host runs on copy_stream while slot
    // k^1 is being traced
    struct UpdateSlot {
        DeviceBuf<uint8_t> d_frame;  // (the record form only)
        DeviceBuf<uint32_t> d_words; // (the word form only)
        DeviceBuf<uint8_t> d_min;
        DeviceBuf<uint8_t> d_scan;   // (bytes)
        PinnedBuf<uint64_t> h_total;
        Event ev_ready, ev_copied;
        size_t bytes = 0;
        bool busy = false;
        // a small frame whose Minimize launch writes the caller's buffer itself (RTX_OPT_UPDATE_HOST_WRITE): nothing was waited for in
        // rtx_update_begin; rtx_update_end waits for ev_ready, reads the length from h_total and settles `run`
        bool host_write = false;
        MinRun run; // the Minimize launch of the slot's frame
    };
    UpdateSlot upd[2];
    Stream copy_stream;
    unsigned upd_next = 0;

    // light and hard shadows (RTX_OPT_SHADOWS, rtx_scene_set_light): with shadows off and the reference's light every launch is
    // today's one-pass trace; otherwise rtx_render_rows traces the closest hit into a hit buffer (8 bytes per pixel) and
    // rtx_shadow_shade shades from it.  One hit buffer per render stream (launches on one stream are ordered; frames on two
    // streams never share one), for at most kMaxHitStreams streams.
    // the lights (rtx_scene_set_lights; rtx_scene_set_light sets a set of one).  A set of one launches what it always has; two or
    // more (or RTX_OPT_LIGHTS_CHECK 1) shade with rtx_lights_shade / rtx_lights_reflect_shade, which get the set by value.
    rtx_light lights[RTX_MAX_LIGHTS] = {rtx_reference_light()};
    size_t n_lights = 1;
    rtxspot::Block spots = {}; // the cones of the set (rtx_scene_set_spots), as stored: all zero while every light is a point light
    uint64_t stat_spot_frames = 0;
    uint64_t stat_shadow_frames = 0;
    static constexpr int kMaxHitStreams = 64;
    struct HitScratch {
        hipStream_t stream = nullptr;
        DeviceBuf<uint8_t> p;
        bool recorded = false; // a launch recorded into a graph reads this buffer
    };
    std::vector<HitScratch> hit_scratch;
    std::vector<DeviceBuf<uint8_t>> hit_retired; // outgrown buffers that a recorded graph may still read

    // surface attributes by creation index (rtx_materials.hpp): the reflectivity k, the slot in the pattern table, the index of
    // refraction, the finish and the shadow-casting flag, with their counts, the upload flag and the generations that tell recorded graphs they are stale.  While an object
    // has k > 0 (or under RTX_OPT_REFLECT_CHECK 2) rtx_render_rows traces the closest hits, rtx_reflect_hit the secondary hits of the
    // reflective pixels and rtx_reflect_shade shades and blends: 16 bytes per pixel of the stream's hit buffer.
    rtxmat::Book materials;
    rtx_pattern patterns[RTX_MAX_PATTERNS] = {}; // the table (rtx_scene_set_patterns): context state, like the lights
    size_t n_patterns = 0;
    uint64_t stat_pattern_frames = 0, stat_refract_frames = 0, stat_finish_frames = 0;
    struct MaterialBufs { // the device copies, all uploaded at the next launch that reads any of them after a change (upload_materials)
        rtxmat::Orders<DeviceBuf<float>> k, ior;
        rtxmat::Orders<DeviceBuf<uint8_t>> slot;
        rtxmat::Orders<DeviceBuf<rtx_finish>> finish;
        rtxmat::Orders<DeviceBuf<uint8_t>> cast;
        DeviceBuf<uint8_t> cast_gidx; // the same flags by creation index, for the grid's lists (GridShadowArgs::list_gidx)
        DeviceBuf<rtxpattern::Entry> table;
        DeviceBuf<uint32_t> pos; // rtxmat::position_map, for rtx_grid_reflect (RTX_OPT_REFLECT_GRID)
    } d_mat;
    std::vector<uint32_t> h_sorted_idx; // sorted position -> sphere index of the sorted copy (valid while sorted_gen == scene_gen)
    uint64_t stat_reflect_frames = 0;
    // mirrors that see mirrors (RTX_OPT_REFLECT_DEPTH): at depth 1 with the check option 0 every launch is the one-bounce path's;
    // otherwise rtx_reflect_chain traces every level in one launch and rtx_lights_chain_shade folds the chain, through 8 (depth + 1)
    // bytes per pixel of the stream's hit buffer.  The depth travels in the kernel arguments.
    // shadows seen in mirrors (RTX_OPT_REFLECT_SHADOWS): in effect while RTX_OPT_SHADOWS is 1 and the mirror path is taken; then the
    // chain kernels at any depth, rtx_chain_shadow between them, and 4 more bytes per pixel of the hit buffer (the dark words)

    // The counters kernels write and rtx_get_option reads back (rtxmem::Counter): one word or one array per context, which the
    // launch set queued last has zeroed on its stream, behind its closest-hit launch.  When each reads its words and when 0:
    //  - the two longest lists and the two fallback counters: whenever the buffer exists (it keeps the last launch set's words
    //    that wrote it);
    //  - reflect_rays: on the mirror path launch_frame sets valid to whether the plan counts rays (the chain kernels or
    //    rtx_grid_reflect; else RTX_STAT_REFLECT_RAYS reads 0).  The shaded path without a mirror and the direct path leave flag
    //    and buffer alone: the words of the last mirror frame stay readable;
    //  - reflect_shadow_points: cleared at the top of launch_frame by every frame off the mirror path, the direct path included,
    //    and by every batched launch (never the mirror path's); on the mirror path valid is whether rtx_chain_shadow runs (plan.deep);
    //  - delta_counts (changed cells, runs): valid from the first delta launch queued on (rtx_delta_counters, below).
    Counter<uint32_t, 1> shadow_longest;          // the longest occluder list of the last two-pass launch
    Counter<uint32_t, 1> reflect_longest;         // the longest candidate list of the last launch set on the mirror path
    Counter<uint32_t, RTX_MAX_REFLECT_DEPTH> reflect_rays{false};          // secondary rays per level
    Counter<uint32_t, RTX_MAX_REFLECT_DEPTH> reflect_shadow_points{false}; // hit points shadow-tested per level
    Counter<uint32_t, 1> shadow_grid_fallback;    // segments of the last launch set through the grid that tested every sphere
    Counter<uint32_t, 1> reflect_grid_fallback;   // rays of the last launch set through the grid that tested every sphere
    Counter<unsigned long long, 2> delta_counts{false};

    // ray queries (rtx_query_rays, rtx_pick; rtx_query.cpp): the world grid over the scene arrays in creation order, rebuilt on the
    // context's stream by the first query after a scene edit or a physics step (qgrid.dirty).  The build is the writer of `sync`
    // (rtx_sync.hpp); queries and the render launches that read the lists (RTX_OPT_SHADOW_GRID), on whatever stream, are its readers.
    struct QueryGrid {
        rtxgrid::Grid plan;
        bool dirty = true;            // the scene changed since the last build
        bool brute = false;           // the last build gave up (more than kLargeCap large spheres): queries test every sphere
        uint32_t n_cells = 0, n_large = 0, pairs = 0;
        DeviceBuf<uint32_t> cell_count, cell_fill, pair_tmp, list_gidx;
        DeviceBuf<uint8_t> is_large;
        DeviceBuf<float4> list_geom;
        DeviceBuf<uint32_t> d_large;  // kLargeCap sphere indices
        DeviceBuf<uint32_t> d_words;  // [0] pairs, [1] large spheres, [2] fallback rays of the last call, [4..10] bounds
        DeviceBuf<uint8_t> d_ray;     // rtx_pick's ray and hit (48 bytes)
        rtxsync::Shared sync;
    };
    QueryGrid qgrid;
    uint64_t stat_query_builds = 0;

    // shadow tests through that grid (RTX_OPT_SHADOW_GRID): in effect while RTX_OPT_SHADOWS is 1, RTX_OPT_SHADOW_CHECK 0, the scene has
    // a sphere and the build found a usable grid; then rtx_grid_shadow decides every level's dark lights per pixel and the
    // rtx_grid_*shade family shades from its words: 4 more bytes per pixel of the stream's hit buffer
    uint64_t stat_shadow_grid_frames = 0;

    // mirror rays through that grid (RTX_OPT_REFLECT_GRID): in effect on the mirror path while RTX_OPT_REFLECT_CHECK is 0, the scene has a
    // sphere and the build found a usable grid; then rtx_grid_reflect writes the hit arrays in place of rtx_reflect_hit /
    // rtx_reflect_chain, finding spheres through d_mat.pos.
    uint64_t stat_reflect_grid_frames = 0;

    // supersampling (RTX_OPT_SUPERSAMPLE): with S > 1 rtx_render_rows runs its launches for the S W x S H sample frame in values form
    // into the render stream's sample buffer (32 S^2 W rows bytes; one per render stream as the hit buffers, for at most
    // kMaxHitStreams streams; it grows on demand, never shrinks and goes with the context) and rtx_resolve folds it into the target
    uint64_t stat_supersample_frames = 0;
    struct SampleScratch {
        hipStream_t stream = nullptr;
        DeviceBuf<uint8_t> p;
    };
    std::vector<SampleScratch> sample_scratch;

    // objects edited in place (rtx_scene_set_spheres, rtx_scene_set_spheres_device, rtx_scene_set_plane; rtx_post.hip): rows that
    // come from the host, or from another member of a device group, are staged in d_edit_rows (floats);
    // rtx_write_spheres leaves its two result words in d_edit_result, which the call copies to the pinned pair and waits for
    DeviceBuf<float> d_edit_rows;
    DeviceBuf<uint32_t> d_edit_result;
    PinnedBuf<uint32_t> h_edit_result;
    Event ev_edit;                      // orders a device-form edit after what the caller's stream holds
    uint64_t stat_scene_edits = 0;      // edit calls that changed something
    uint32_t stat_edit_move_bits = 0;   // RTX_STAT_SCENE_EDIT_MOVE

    // objects removed in place (rtx_scene_remove_objects, rtx_scene_remove_marked_device; rtx_post.hip): rtx_compact_objects moves the
    // survivors into the spare set of the eight scene arrays (sphere geom / color / od / motion, plane a / b / c / od: as large as the
    // live ones), which is then swapped with the live set; the removed indices travel in d_remove_lists (words), a device form's marks
    // arrive in the pinned h_remove_marks
    DeviceBuf<float4> d_spare[8];
    DeviceBuf<uint32_t> d_remove_lists;
    PinnedBuf<uint8_t> h_remove_marks;
    uint64_t stat_scene_removed = 0;    // RTX_STAT_SCENE_REMOVED

    // delta frames (rtx_delta_words: rtx_post.hip; rtx_update_delta: rtx_update.cpp): the previous and the current frame's pixel words in two
    // buffers that swap roles (delta_at: the one the last successful call handed out), the delta's own output buffer (sized by
    // rtx_delta_bound at first use) and the two counters of the last delta launch (changed cells, runs)
    DeviceBuf<uint32_t> d_delta_words[2];
    unsigned delta_at = 0;
    bool delta_valid = false;           // delta_words[delta_at] is the frame the consumer shows: W, H, mode and kind as below
    bool delta_half = false;            // ... as a half-block frame (rtx_update_half_delta: W x 2H words), else as plain cells (rtx_update_delta)
    size_t delta_w = 0, delta_h = 0;
    int delta_mode = -1;
    DeviceBuf<uint8_t> d_delta_out;
    uint64_t stat_delta_frames = 0, stat_delta_keyframes = 0;
    uint64_t stat_half_delta_frames = 0, stat_half_delta_keyframes = 0; // RTX_STAT_HALF_DELTA_FRAMES, _KEYFRAMES

    // half-block frames (rtx_update_half; rtx_update.cpp): the stream's own buffer, grown on demand to rtx_half_bound bytes (d_min
    // holds 20 W 2H, a half-block stream can take 41 W H)
    DeviceBuf<uint8_t> d_half_out;
    uint64_t stat_half_frames = 0;      // RTX_STAT_HALF_FRAMES

    std::string error;
    const char* last_kernel = "";
};


// rtx_api.cpp
int rtx_fail(rtx_ctx* ctx, int status, const std::string& msg);
int rtx_hip_fail(rtx_ctx* ctx, hipError_t e, const char* what);
// the two counters for a delta launch about to be queued: from now on RTX_STAT_DELTA_CELLS and _RUNS read them
inline int rtx_delta_counters(rtx_ctx* ctx, unsigned long long** out)
{
    if (ctx->delta_counts.ensure() != hipSuccess) return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "hipMalloc failed for the delta counters");
    ctx->delta_counts.valid = true;
    *out = ctx->delta_counts.get();
    return RTX_OK;
}
int rtx_sync_scene(rtx_ctx* ctx);
void rtx_scene_edited(rtx_ctx* ctx);
int rtx_sort_scene(rtx_ctx* ctx, const float origin[3]); // rtx_post.hip
// rtx_post.hip: Minimize as rtx_update.cpp drives it.  launch_minimize queues the Minimize of `in` into d_out on the context's stream
// (scratch d_scan: min_scan_bytes of it; `pair`: pinned host words, as the device addresses them, that receive the result instead of
// d_scan); settle_minimize takes the two result words as the host read them after a wait and redoes a launch whose blocks gave up;
// minimize_and_wait is both with the context's scratch, the wait in between, d_out = nullptr being the context's d_min.
size_t min_scan_bytes(uint64_t n_slots);
int ensure_min_buffers(rtx_ctx* ctx, uint64_t n_slots, bool need_out);
int launch_minimize(rtx_ctx* ctx, void* d_scan, const MinInput& in, uint8_t* d_out, MinRun* run, uint64_t* pair = nullptr);
int settle_minimize(rtx_ctx* ctx, const MinRun& run, const uint64_t got[2], uint64_t* total);
int minimize_and_wait(rtx_ctx* ctx, const MinInput& in, void* d_out, size_t* out_bytes);
// rtx_post.hip: the rows of an edit in place -> spheres first .. first+n-1 of THIS context alone (a validated range of creation
// indices, n > 0, not inside a capture), blocking.  `rows` is host memory (src_device < 0; h_centres follows) or device memory of
// src_device: read in place, or copied into the context's scratch first (`stage`: a group member's copy of the root's rows).
// `after`, if not null, is an event the edit is ordered behind.
int rtx_edit_spheres_here(rtx_ctx* ctx, unsigned first, size_t n, const float* rows, int src_device, bool stage, hipEvent_t after);
// rtx_post.hip: removes the objects of a validated, ascending, non-empty list of creation indices from THIS context alone (not
// inside a capture), blocking: the device arrays are compacted on the device, then the host's books follow
int rtx_remove_objects_here(rtx_ctx* ctx, const std::vector<uint32_t>& ascending);
// ... and its first half alone: uploads pending appends and allocates what the removal needs (the second set of arrays, the list
// buffer); moves nothing.  A group prepares every member before any of them compacts.
int rtx_remove_prepare(rtx_ctx* ctx, const std::vector<uint32_t>& ascending);
// rtx_query.cpp: the world grid for a launch on `stream` that reads its lists -- the one grid object the queries use, brought up to date
// if the scene changed since its last build (a build blocks, as a query's does, and counts in RTX_STAT_QUERY_GRID_BUILDS); `stream` is
// ordered after the build.  Not inside a graph capture.  Then rtx_grid_read, behind the launches: a later rebuild waits for them.
int rtx_grid_ensure(rtx_ctx* ctx, hipStream_t stream);
void rtx_grid_read(rtx_ctx* ctx, hipStream_t stream);
// rtx_render.cpp: whoever is about to write the sphere arrays on the context's stream waits for a cell-list build in flight on the side stream
int rtx_wait_side_builds(rtx_ctx* ctx);
bool rtx_query_stat(const rtx_ctx* ctx, int option, int64_t* value, int* status); // rtx_query.cpp: the RTX_STAT_QUERY_* values
// the zero-fill bookkeeping of the context's own frame buffer for a frame of `mode` whose records something other than
// rtx_render_rows is about to write there (a group's gathered slabs, its expanded words), on the context's stream
extern "C" int rtx_frame_zero_semantics(rtx_ctx* ctx, int mode, uint64_t W, uint64_t H, unsigned flags); // (hidden: not part of the ABI)
bool rtx_group_stat(const rtx_ctx* ctx, int option, int64_t* value); // rtx_group.cpp

#define RTX_HIP(ctx, call)                          \
    do {                                            \
        hipError_t e__ = (call);                    \
        if (e__ != hipSuccess) {                    \
            return rtx_hip_fail((ctx), e__, #call); \
        }                                           \
    } while (0)
