/*
 * rtx.h -- C ABI of the MI355X (gfx950) ray-trace hot path.
 *
 * This is the drop-in boundary for ONE path of EmilHogstedt/Raytracing-in-Windows-Console:
 * RayTracingManager::Update -> RayTracing::RayTrace -> RayTrace_<MODE> kernels
 * (primary-ray generation, sphere/plane closest hit, Blinn-Phong shading, ANSI record
 * write) plus the Minimize pass and the UpdateObjects step that Update runs around it.
 * Plain pointers and sizes only; every entry point returns an int status (0 = RTX_OK) and
 * never exits the process.  Reference citations are file:line under ConsoleProject/.
 *
 * The reference has no FFI layer: its seams are in-process C++.  Each entry
 * point below names the reference interface it replaces; include/rtx_compat.hpp rebuilds
 * the reference's classes (RayTracingManager, RayTracing, Scene3D, ...) on top of this ABI,
 * and INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Threading: one caller per context, blocking unless a call says otherwise (the reference
 * drives the path from its main thread only, Engine3D.cpp:81-107).
 */
#ifndef RTX_H
#define RTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden; only this header's entry points are exported */
#pragma GCC visibility push(default)

typedef struct rtx_ctx rtx_ctx;

/* Status codes. */
enum rtx_status {
    RTX_OK = 0,
    RTX_ERR_INVALID_ARGUMENT = 1,
    RTX_ERR_INVALID_MODE = 2,    /* RayTracing.cu:863-865 asserts; this ABI reports */
    RTX_ERR_HIP = 3,             /* a HIP runtime call failed: rtx_last_error() has the text (pch.h:45-53 exits instead) */
    RTX_ERR_OUT_OF_MEMORY = 4,
    RTX_ERR_NO_DEVICE = 5,       /* no gfx950 device visible: the product never falls back to a CPU path */
    RTX_ERR_TOO_LARGE = 6        /* frame larger than the context was created for */
};

/* enum RenderingMode, RayTracingManager.h:21 (same values). */
enum rtx_mode {
    RTX_BIT_ASCII = 0,
    RTX_BIT_PIXEL = 1,
    RTX_RGB_ASCII = 2,
    RTX_RGB_PIXEL = 3,
    RTX_RGB_NORMALS = 4,
    RTX_SDL = 5
};

/* Bytes per pixel record: SIZE_8BIT / SIZE_RGB, RayTracing.h:120-124. */
#define RTX_SIZE_8BIT 12
#define RTX_SIZE_RGB 20

/* struct RayTracingCPUToGPUData, RayTracingManager.h:9-19: the logical payload without the
 * six vptrs the reference's Matrix/Vector classes carry.  inv_v is row-major (row1..row4). */
typedef struct rtx_params {
    float inv_v[16];
    float cam_pos[3];
    float element1;  /* projection matrix [0][0], Engine3D.cpp:94 */
    float element2;  /* projection matrix [1][1], Engine3D.cpp:95 */
    float cam_far;   /* Engine3D.cpp:96 */
    uint64_t x;      /* console width  W, Engine3D.cpp:92 */
    uint64_t y;      /* console height H, Engine3D.cpp:93 */
} rtx_params;

/* Which kernel family renders (RTX_OPT_KERNEL). */
enum rtx_kernel {
    RTX_KERNEL_AUTO = 0,   /* binned when it pays, brute otherwise */
    RTX_KERNEL_BRUTE = 1,  /* every pixel tests every object, scene tiles staged in LDS */
    RTX_KERNEL_BINNED = 2  /* per-workgroup conservative frustum culling, then the same exact tests */
};

enum rtx_option {
    RTX_OPT_KERNEL = 1,       /* enum rtx_kernel */
    RTX_OPT_TILE_LOG2_W = 2,  /* log2 of the sub-tile width in pixels (2..6; a sub-tile is 256 pixels); 0 = choose from the camera */
    RTX_OPT_SUBTILES = 3,     /* sub-tiles per workgroup in the binned kernel (1, 2, 4, 8, 16); 0 = default */
    RTX_OPT_TWO_LEVEL = 4,    /* coarse-cell pre-pass before the binned kernel (one launch: blocks of 4x4 cells, then the cells):
                               * -1 auto (from 2048 spheres; from 256 while the view is locally dense, RTX_OPT_VIEW_ADAPT; smaller
                               * scenes get exact lists while camera and scene rest, see RTX_OPT_CELL_REUSE), 0 off, 1 on (2 is
                               * accepted and means 1) */
    RTX_OPT_CELL_CAPACITY = 7, /* entries per coarse-cell list of that pre-pass; 0 = auto (4 * spheres / cells + 1024, so that the
                               * scratch is O(spheres)).  A cell whose list does not fit falls back to the whole scene: slower,
                               * the same frame */
    RTX_OPT_TILE_ORDER = 6,   /* binned kernel: dispatch the macro tiles heaviest first and dealt evenly over the CUs, from the work
                               * estimates (and, for grids of one dispatch round, the measured durations) that earlier frames of
                               * the same tile grid on the same stream left behind.  Speed only: the frame is the same in any
                               * order.  -1 = auto (default): on for tile grids whose workgroups are all resident at once (5 or 6
                               * sub-tiles per workgroup are chosen to make that so, e.g. at 1080p); those are balanced by
                               * rtx_balance_tiles on a stream of the library's own, every 4th frame for the first 64 frames of a
                               * grid, then every 64th (one 1080p launch alone: 29.3 -> 25.9 us).  Larger grids (several dispatch
                               * rounds, up to six): heaviest first only while the caller renders on a single stream -- then nothing
                               * overlaps the end of a launch, and the workgroups dispatched last should be the light ones (a dense
                               * 1080p scene alone 44.6 -> 41.4 us); with frames in flight on several streams the order gains
                               * nothing, costs 1-2 % and at 8K 10 % by separating tiles that share 128-byte lines: off.
                               * 0 = frame order; k > 0 = on for every grid, the order re-derived every k-th frame */
    RTX_OPT_CELL_REUSE = 8,   /* coarse-cell lists of that pre-pass outlive the frame: binned with every sphere's culling margin grown by a
                               * motion budget (about sixteen frames of the camera's and the spheres' current motion), the lists serve
                               * every later frame whose camera stays within it -- for a static view: all of them -- and are rebuilt
                               * ahead of time, beside the frames, on the library's side stream.  A camera too fast for that (a
                               * quarter of a cell in under four frames) gets the per-frame pre-pass.  Scenes under 2048 spheres, for
                               * which a pre-pass per frame does not pay, get exact lists while camera and scene rest (two launches
                               * in a row without motion) and none otherwise.  Same frames either way: a list is always a superset
                               * of what a pixel ray of its cell can hit.  -1 auto (on), 0 off, 1 on */
    RTX_OPT_XCD_ORDER = 9,    /* two-level grids: dispatch the macro tiles so that a cell's tiles (and neighbouring cells) run on one
                               * XCD, whose L2 then holds that part of the scene alone.  Speed only.  -1 auto (on), 0 off, 1 on */
    RTX_OPT_VIEW_ADAPT = 10,  /* a scene that is sparse by its numbers can be locally dense from where the camera stands (config 2 seen along
                               * its long axis: 95 candidates on one macro tile instead of 9, one launch alone 63 us instead of 27).  The
                               * trace workgroups report their longest candidate list; when it passes 28 the following launches are
                               * planned as for a dense scene (2 sub-tiles per workgroup, two-level culling, per-wave refinement: 23-27 us
                               * on those views), and as before again once it has stayed short.  Same frames either way.
                               * -1 auto (on), 0 off, 1 on */
    RTX_OPT_SORTED_STORE = 11,/* staging reads a copy of the sphere array sorted by direction (Morton code of azimuth and elevation as seen
                               * from the camera of the first launch after a scene edit), kept in step by rtx_update_objects: the spheres
                               * of a coarse cell are then neighbours in memory (config 5: a quarter of the lines per launch).  Speed
                               * only; ties are still broken by creation order.  Scenes from 256 spheres.  -1 auto (on), 0 off, 1 on */
    RTX_OPT_BATCH = 14,       /* rtx_submit_slabs: consecutive slabs on ONE stream are traced by one launch (up to 16 frames' rows per launch; the
                               * frames' cameras and output buffers travel in the kernel arguments), instead of a launch each -- a rank's slab of
                               * a sharded 1080p frame is 255 workgroups, far too few to fill 256 CUs.  Taken where the plan has neither
                               * two-level culling nor per-wave refinement and the frames differ in camera only.  -1 auto (on), 0 off, 1 on */
    RTX_OPT_UPDATE_WORDS = 15, /* rtx_update / rtx_update_begin trace 4-byte pixel words (RTX_RENDER_COMPACT) and minimise from them instead of
                               * writing the 12 / 20-byte records and reading them back twice: the same minimised stream with a fifth of the
                               * memory traffic (1080p RGB: 8.3 MB written + 16.6 MB read instead of 41.5 + 83).  The context's frame buffer
                               * is then not written by an Update (it keeps what the last rtx_render left).  -1 auto (on), 0 off (records:
                               * the frame buffer holds the frame after every Update, as the reference's m_deviceResultArray does), 1 on */
    RTX_OPT_MINIMIZE_FUSED = 17, /* Minimize -- from pixel words (rtx_minimize_words, rtx_update with RTX_OPT_UPDATE_WORDS) and from records (rtx_minimize) -- as ONE launch: every block counts
                               * its slots, publishes its length and finds its place in the stream by a two-level look-back over the lengths of
                               * the blocks before it, instead of three launches (count, offsets, scatter; two for records) that read their input twice.  A launch
                               * whose blocks gave up waiting (bounded polling; never seen) is redone as three launches: RTX_STAT_MINIMIZE_FALLBACKS.
                               * -1 auto (on), 0 off, 1 on, 2 on with blocks that give up on purpose (tests of that path) */
    RTX_OPT_GROUP_EXCHANGE = 12, /* device groups (rtx_group_create): enum rtx_group_exchange -- how the slabs reach the root */
    RTX_OPT_GROUP_THREADS = 16, /* device groups: a submission thread per rank other than the root queues that rank's launch and copy while the
                               * caller's thread queues the root's (a rank's share is ~15 us of host work; on one thread 8 ranks cost 132 us per
                               * 1080p frame).  The call still returns only when everything is queued.  -1 auto (on where the list names two or
                               * more distinct devices; with all ranks on one GPU the threads were measured to change nothing), 0 off, 1 on */
    RTX_OPT_UPDATE_HOST_WRITE = 19, /* rtx_update / rtx_update_begin (word form, one device) when the caller's buffer is pinned, device-addressable memory
                               * (rtx_host_alloc's is): the Minimize launch stores the stream and its length straight into host memory instead of
                               * leaving them to two copies.  The blocking form then waits for the device ONCE (console-sized frames 45 -> 27 us per
                               * Update, 1080p 0.395 -> 0.370 ms); the pipelined form does not wait at all before rtx_update_end (console sizes 35 ->
                               * 19 us).  The same bytes; a pageable buffer quietly takes the copy form.  -1 auto (blocking: always; pipelined: frames
                               * up to 2^17 slots -- beyond that a launch that runs at PCIe speed delays the next frame's kernels), 0 off, 1 on */
    RTX_OPT_GROUP_UPDATE = 18, /* device groups: how rtx_update / rtx_update_begin hand the minimised stream to the host.  0: the ranks' pixel words
                               * are gathered on the root, which minimises the frame and copies the stream over ITS PCIe link (the whole Update is
                               * bound by that copy: 0.33 ms per 1080p RGB frame).  1: no gather -- every rank traces its rows and the row above them,
                               * minimises its own rows (the colour carried over from the last pixel above) and copies its part of the stream to its
                               * place in the host buffer over its OWN link, N links at once (SURVEY.md 8(e)'s alternative).  The same bytes either
                               * way.  -1 auto: 1 where the list names two or more distinct devices.  A HIP error on the direct path makes the group
                               * fall back to 0 for good (RTX_STAT_GROUP_DIRECT_UPDATES counts the direct ones) */
    RTX_OPT_GROUP_WIRE = 13,  /* device groups: enum rtx_group_wire -- what travels: compact pixel words (default) or records */
    RTX_OPT_SHADOWS = 20,     /* hard shadows from the light (rtx_scene_set_light): 0 off (default), 1 on.  A pixel whose hit point faces
                               * away from the light, or whose segment to the light meets another object, is shaded with the light's two
                               * powers at 0 (ambient only; glyph and every other field unchanged).  The character modes only: RGB_NORMALS and
                               * SDL are unaffected.  With shadows off and the reference's light the frame loop launches exactly what it
                               * launches without this option; any other state traces the closest hit first and shades in a second launch,
                               * which culls occluders per 16 x 16 tile against the cone from the light through the tile's hit points.
                               * The closest hits go through a hit buffer of 8 bytes per pixel, one per render stream (at most 64 streams),
                               * allocated at the first such launch on it; a recorded graph keeps the buffer of the stream it was recorded
                               * on, so replays of it must not overlap launches on that stream or one another.
                               * No reference counterpart (RayTracing.cu:132 "#todo: INTRODUCE REAL LIGHTS!", :143-157) */
    RTX_OPT_SHADOW_CHECK = 21, /* for checks, not for the frame loop: 0 normal (default); 1 every shadow ray tests every object, no culling (the
                               * brute reference of the culled path); 2 the two-launch path with no occlusion and no self-shadow test, so that
                               * every pixel is lit.  No reference counterpart */
    RTX_OPT_REFLECT_CHECK = 22, /* for checks, not for the frame loop: 0 normal (default); 1 every secondary ray of the mirror path
                               * (rtx_scene_set_reflectivity) tests every sphere, no culling (the brute reference of the culled pass); 2 the
                               * reflection launches even where no object reflects (they then give the bytes of the launches they replace).
                               * No reference counterpart */
    RTX_OPT_QUERY_CHECK = 23, /* for checks, not for production: 0 normal (default): rtx_query_rays walks the world grid; 1 every ray tests
                               * every object (the brute kernel the grid is checked against).  The same bytes either way.
                               * No reference counterpart (RayTracingManager.cu:21,46-51) */
    RTX_OPT_QUERY_LOAD = 24,  /* spheres per cell the world grid of the ray queries aims at, in sixteenths (16 = 1 per cell); 0 = the
                               * default.  Speed only; takes effect at the next build.  No reference counterpart */
    RTX_OPT_LIGHTS_CHECK = 25, /* for checks, not for the frame loop: 0 normal (default): a set of one light (rtx_scene_set_lights) launches
                               * exactly what rtx_scene_set_light launches; 1 the several-lights kernels (rtx_lights_shade,
                               * rtx_lights_reflect_shade) are launched even for a set of one light (they then give the bytes of the
                               * launches they replace).  No reference counterpart (RayTracing.cu:132,143-157) */
    RTX_OPT_REFLECT_DEPTH = 26, /* mirrors that see mirrors: how many levels of secondary rays a reflective pixel may trace, 1 (default:
                               * today's one bounce) .. RTX_MAX_REFLECT_DEPTH; the rule is at rtx_scene_set_reflectivity.  Anything else
                               * returns RTX_ERR_INVALID_ARGUMENT and changes nothing.  Takes effect for launches queued afterwards; a
                               * recorded graph keeps the depth it was recorded with (the depth travels in the kernel arguments, as the
                               * light set does).  At depth 1 every launch is what it is without this option; deeper, the mirror path's
                               * second and third launches are rtx_reflect_chain (every level in one launch) and rtx_lights_chain_shade,
                               * and the hit buffer holds 8 (depth + 1) bytes per pixel.
                               * No reference counterpart (RayTracing.cu:635) */
    RTX_OPT_REFLECT_DEPTH_CHECK = 27, /* for checks, not for the frame loop: 0 normal (default); 1 the chain kernels (rtx_reflect_chain,
                               * rtx_lights_chain_shade) are launched even at depth 1 (they then give the bytes of the launches they
                               * replace).  No reference counterpart (RayTracing.cu:635) */
    RTX_OPT_REFLECT_SHADOWS = 28, /* shadows seen in mirrors: 0 (default: every launch, byte for byte, what it is without this option) or
                               * 1: the shadow test of RTX_OPT_SHADOWS at every reflected hit as well.  Anything else returns
                               * RTX_ERR_INVALID_ARGUMENT and changes nothing.  It has an effect only while RTX_OPT_SHADOWS is 1 and some
                               * object reflects (rtx_scene_set_reflectivity); otherwise every launch is what it is without it.  The
                               * rule, in the terms of rtx_scene_set_reflectivity: for every level j in 1 .. depth at which the chain
                               * exists and hit an object o_j, the hit point P_j = r_j.o + r_j.d * t_j with the normal n_j of o_j there
                               * gets level 0's test for every light i of the set, on its own.  Light i is dark at level j iff
                               * dot(n_j, L_i - P_j) <= 0, or the open segment from P_j to L_i crosses a plane other than o_j (inside
                               * its bounds, level 0's expressions), or comes closer than r to the centre of a sphere other than o_j.
                               * Levels j >= 1 have no far limit (level 0 keeps its distance <= cam_far condition).  local_j is then
                               * the Blinn-Phong colour with the dark lights at both powers 0; the fold, distance, glyph and normal are
                               * unchanged.  RTX_OPT_SHADOW_CHECK applies to these tests exactly as to level 0's: 1 makes every sphere a
                               * candidate, 2 applies no test, so every level is lit.  While in effect the mirror path takes the chain
                               * kernels at any depth: closest hits, rtx_reflect_chain, rtx_chain_shadow (the tests, per 16 x 16 tile
                               * and level), rtx_lights_chain_shadow_shade; the hit buffer holds 8 (depth + 1) + 4 bytes per pixel.
                               * The value travels to the launches by value: a recorded graph keeps what it was recorded with.
                               * Replicated over a device group like every option.  RTX_STAT_SHADOW_LONGEST_LIST then covers the
                               * deeper levels' lists too.  No reference counterpart (RayTracing.cu:132,635) */
    RTX_OPT_SHADOW_GRID = 29, /* shadow tests through the world grid of the ray queries: 0 (default: every launch, byte for byte and
                               * kernel for kernel, what it is without this option) or 1.  Anything else returns
                               * RTX_ERR_INVALID_ARGUMENT and changes nothing.  The rule: the test itself is unchanged -- self-shadow,
                               * the planes, and for every sphere other than the point's own the closest point of the segment to its
                               * centre, at every level RTX_OPT_SHADOWS and RTX_OPT_REFLECT_SHADOWS test -- only WHICH spheres a segment
                               * is tested against changes: those listed in the cells the segment P + k (L - P), k in [0, 1], passes
                               * through (and the grid's large spheres) instead of those a cone over the 16 x 16 tile keeps.  No sphere
                               * the test would report is left out (a proved bound), so the frames are byte for byte those of
                               * the existing path.  It has an effect only while RTX_OPT_SHADOWS is 1, RTX_OPT_SHADOW_CHECK is 0
                               * (checks 1 and 2 keep today's launches: they are the brute reference), the scene has at least one
                               * sphere, and the grid is usable (RTX_STAT_QUERY_BRUTE reads 0 after the build); otherwise every launch
                               * is what it is without it.  The launches, while in effect: closest hits (and on the mirror path
                               * rtx_reflect_hit or rtx_reflect_chain, unchanged), rtx_grid_shadow -- one pixel per thread, no list in
                               * LDS: level 0's dark lights, and in place of rtx_chain_shadow the deeper levels' -- then
                               * rtx_grid_shade / rtx_grid_reflect_shade / rtx_grid_chain_shade / rtx_grid_chain_shadow_shade, which
                               * read them, for any light set, a set of one included.  The hit buffer holds 4 more bytes per pixel
                               * (level 0's word): 12 on the shadow path, 20 for one bounce, 8 (depth + 1) + 4 (+ 4 under
                               * RTX_OPT_REFLECT_SHADOWS) on the chain.  The grid is the queries' own (one object, one
                               * RTX_STAT_QUERY_GRID_BUILDS): the first frame after rtx_scene_add_*, rtx_scene_clear or
                               * rtx_update_objects rebuilds it, which blocks as a query's build does -- a physics step per frame
                               * means a build per frame.  A segment that cannot be walked -- its point further from the spheres' box
                               * than three times the box's largest half-extent (a far floor), the light at the point itself, a length
                               * outside [2^-20, 2^20] -- tests every sphere (RTX_STAT_SHADOW_GRID_FALLBACK_POINTS).  A launch on this
                               * path is refused inside a graph capture with RTX_ERR_INVALID_ARGUMENT (the lists change with physics,
                               * and the build allocates and waits); rtx_submit_slabs queues its slabs one by one, as on the shadow
                               * path.  Replicated over a device group like every option; every member builds its own grid on its own
                               * device.  RTX_STAT_SHADOW_LONGEST_LIST reads 0 after such a set.  Off by default: where most segments
                               * fall back it is slower.  No reference counterpart (RayTracing.cu:132) */
    RTX_OPT_SUPERSAMPLE = 30, /* S x S rays per console cell, folded on the GPU: S in {1, 2, 3, 4}, default 1.  Anything else returns
                               * RTX_ERR_INVALID_ARGUMENT and changes nothing.  At S = 1 every launch is, byte for byte and kernel for
                               * kernel, what it is without the option.  The value takes effect for launches queued afterwards.
                               * Replicated over a device group like every option.  The rule, for S > 1 and a call that renders rows
                               * [row0, row0 + rows) of a W x H frame with params p in one of the five character modes:
                               * 1. The sample frame is the RTX_RENDER_VALUES output of the existing paths for p', which is p with
                               *    x = S W and y = S H (ray generation divides by x and y, so p' has exactly p's field of view), over
                               *    rows [S row0, S (row0 + rows)); scene, light set and every option unchanged; planned exactly as a
                               *    caller's frame of that size is.  Cell (c, r) with c < W - 1 owns the n = S^2 samples
                               *    (S c + i, S r + j), numbered k = j S + i; sample (0, 0) is the ray of S = 1.  Sample columns from
                               *    S (W - 1) on belong to the newline column and are ignored.
                               * 2. The fold.  vis_k means distance_k <= cam_far; m is the number of visible samples.  m = 0: the
                               *    cell's values are (99999999.f, 0, 0, 0, 0, 0, 0, 0).  m > 0: distance is the minimum of distance_k
                               *    over the visible samples, and each of the seven other floats (shadingValue, normal.xyz,
                               *    colour.xyz) is acc * (1.0f / (float)n), where acc starts at 0.0f and for k = 0 .. n - 1 in order
                               *    acc = acc + (vis_k ? v_k : 0.0f); every operation rounded to fp32, nothing reassociated or
                               *    contracted.  Samples that miss, or lie beyond cam_far, count as black: coverage against the
                               *    console's black background.
                               * 3. The output is what the record encoder makes of the folded values at (row, col) of the W x H frame:
                               *    records, pixel words or value floats by the caller's flags; the newline column as always (NUL
                               *    records, 0xffffffff, eight zeros); out_row_base, the context's own buffer with its zero-fill
                               *    semantics and RTX_RENDER_ZERO_TAIL unchanged.
                               * The launches: the existing ones into the render stream's sample buffer (32 S^2 W rows bytes, one per
                               * render stream for at most 64 streams; it grows on demand, never shrinks, is freed by rtx_destroy;
                               * RTX_ERR_OUT_OF_MEMORY when it cannot grow), then rtx_resolve<S,mode[,compact|,values]>, which
                               * rtx_last_kernel_name reports.  Everything that traces through rtx_render_rows inherits the rule:
                               * rtx_render, rtx_submit_frames / rtx_submit_slabs (queued one by one: no RTX_OPT_BATCH launch while
                               * S > 1), rtx_update, rtx_update_begin, rtx_update_delta, rtx_update_half and rtx_update_half_delta (their pixel words are the folded cells'),
                               * and device groups (rank g's cell rows are sample rows [S row0_g, S (row0_g + rows_g)) with the global
                               * row index, so a sharded frame equals the one-device frame).  RTX_SDL writes nothing and is
                               * unaffected; rtx_pick, rtx_query_*, rtx_expand, rtx_minimize* and rtx_delta_words do not trace.  A
                               * supersampled launch inside a graph capture returns RTX_ERR_INVALID_ARGUMENT (the sample buffer may
                               * grow), and so does one with S x or S y of 2^31 or more; otherwise the existing paths' limits apply
                               * to the sample frame.  No reference counterpart (RayTracing.cu:12-17 traces one ray per cell) */
    RTX_OPT_REFLECT_GRID = 31, /* mirror rays through the world grid of the ray queries: 0 (default: every launch, byte for byte and
                               * kernel for kernel, what it is without this option) or 1.  Anything else returns
                               * RTX_ERR_INVALID_ARGUMENT and changes nothing.  The rule: the test itself is unchanged -- the planes per
                               * pixel, the reference's sphere test for every sphere other than the one the ray leaves, no far limit,
                               * the winner the minimum of (t, creation index), at every level 1 .. RTX_OPT_REFLECT_DEPTH (the rule at
                               * rtx_scene_set_reflectivity) -- only WHICH spheres a secondary ray is tested against changes: the
                               * grid's large spheres and those listed in the cells the ray passes through, walked with no far limit
                               * until its best t is below the parameter at which it leaves the cell just tested, or until it leaves
                               * the grid, exactly as rtx_query_rays walks -- instead of those a bundle over the 16 x 16 tile keeps.
                               * No sphere the test would report is left out (the queries' proved bound: a mirror ray is a query ray
                               * with tmax = infinity), so the frames are byte for byte those of the existing path.  It has an effect
                               * only while the frame is on the mirror path (something reflects), RTX_OPT_REFLECT_CHECK is 0 (checks 1
                               * and 2 keep today's launches: they are the brute reference), the scene has at least one sphere, and
                               * the grid is usable (RTX_STAT_QUERY_BRUTE reads 0 after the build); otherwise every launch is what it
                               * is without it.  The launches, while in effect: closest hits; rtx_grid_reflect -- one pixel per thread,
                               * every level in one launch, no list in LDS -- in place of rtx_reflect_hit or rtx_reflect_chain; then
                               * whatever shadow pass and shade family the other options choose, unchanged (they read the hit arrays,
                               * whose layout and size are unchanged).  The grid is the queries' own, shared with RTX_OPT_SHADOW_GRID
                               * (one object, one RTX_STAT_QUERY_GRID_BUILDS: a frame with both options on builds once): the first
                               * frame after rtx_scene_add_*, an edit, a removal, rtx_scene_clear or rtx_update_objects rebuilds it,
                               * which blocks as a query's build does -- a physics step per frame means a build per frame.  A ray that
                               * cannot be walked -- its origin further from the spheres' box than three times the box's largest
                               * half-extent on some axis (a mirror floor far outside the spheres), an origin or direction that is not
                               * finite, a squared direction length outside [2^-40, 2^40] -- tests every sphere
                               * (RTX_STAT_REFLECT_GRID_FALLBACK_RAYS).  A launch on this path is refused inside a graph capture with
                               * RTX_ERR_INVALID_ARGUMENT (the lists change with physics, and the build allocates and waits).
                               * Replicated over a device group like every option; every member builds its own grid on its own
                               * device.  Everything that traces through rtx_render_rows inherits it: rtx_update*, slabs,
                               * RTX_OPT_SUPERSAMPLE, half blocks, delta frames and groups.  RTX_STAT_REFLECT_RAYS counts at any depth
                               * on this path; RTX_STAT_REFLECT_LONGEST_LIST reads 0 after such a set.  Off by default: there is no
                               * automatic policy, and where most rays fall back it is slower.  No reference counterpart
                               * (RayTracing.cu:635) */
    RTX_OPT_REFINE = 5        /* per-wave refinement of the candidate list in the binned kernel: -1 auto (dense scenes), 0 off, 1 on
                               * (needs at most 4 sub-tiles per workgroup and a macro tile of at most 64 x 64 pixels; otherwise it
                               * stays off) */
};

/* Read-only counters (rtx_get_option): how the coarse-cell lists of two-level culling were obtained so far. */
enum rtx_stat {
    RTX_STAT_CELL_BUILDS = 101,     /* binned in line because no cached list covered the camera */
    RTX_STAT_CELL_PREFETCHES = 102, /* binned ahead of time on the side stream */
    RTX_STAT_CELL_HITS = 103,       /* launches served by cached lists */
    RTX_STAT_CELL_PER_FRAME = 104,  /* launches that binned for themselves alone (reuse off, or a fast camera) */
    RTX_STAT_ORDER_PASSES = 105,    /* dispatch-order passes queued (rtx_balance_tiles / rtx_order_tiles) */
    RTX_STAT_ORDERS_FROZEN = 106,   /* dispatch orders a live recorded graph reads (kept as they are until it is destroyed) */
    RTX_STAT_VIEW_DENSE = 108,      /* 1 while launches are planned as for a dense scene because of what earlier launches saw */
    RTX_STAT_DENSITY_SWITCHES = 109,/* how often that changed */
    RTX_STAT_BATCHED_LAUNCHES = 114, /* launches that rendered several frames' slabs at once (RTX_OPT_BATCH) */
    RTX_STAT_GROUP_DIRECT_UPDATES = 116, /* Updates of a device group whose ranks minimised and copied their own rows (RTX_OPT_GROUP_UPDATE) */
    RTX_STAT_UPDATE_HOST_WRITES = 117, /* blocking Updates whose Minimize launch wrote the caller's host buffer itself (RTX_OPT_UPDATE_HOST_WRITE) */
    RTX_STAT_MINIMIZE_FALLBACKS = 115, /* fused Minimize launches redone as three launches (RTX_OPT_MINIMIZE_FUSED) */
    RTX_STAT_GROUP_SIZE = 110,      /* logical ranks of the device group this context is the root of (1: a plain context) */
    RTX_STAT_GROUP_EXCHANGE = 111,  /* the exchange the last sharded frame used: RTX_EXCHANGE_PEER_COPY or RTX_EXCHANGE_RCCL (0: none yet) */
    RTX_STAT_GROUP_GATHERS = 112,   /* sharded frames gathered so far */
    RTX_STAT_GROUP_BYTES = 113,     /* bytes the last gather moved between devices */
    RTX_STAT_SHADOW_FRAMES = 118,   /* launch pairs queued on the light / shadow path (RTX_OPT_SHADOWS, rtx_scene_set_light): one per
                                     * rtx_render_rows call, so one per slab of a sliced frame; a recorded launch counts once, when it is
                                     * recorded, not at each replay */
    RTX_STAT_SHADOW_LONGEST_LIST = 119, /* the most occluder candidates one shading workgroup kept after culling (summed over the refills of its
                                     * 1024-entry LDS list; every sphere under RTX_OPT_SHADOW_CHECK 1) in the launch pair queued last.  One
                                     * word per context: with launch pairs in flight on several streams it holds one of theirs.  Reading it
                                     * waits for the device */
    RTX_STAT_REFLECT_FRAMES = 120,  /* launch sets queued on the mirror path (rtx_scene_set_reflectivity): as RTX_STAT_SHADOW_FRAMES */
    RTX_STAT_REFLECT_LONGEST_LIST = 121, /* the most sphere candidates one workgroup kept for its secondary rays after culling (summed over
                                     * the refills of its 1024-entry LDS list; every sphere under RTX_OPT_REFLECT_CHECK 1) in the launch set
                                     * queued last; with RTX_OPT_REFLECT_DEPTH > 1 the maximum over the levels.  One word per context, as
                                     * RTX_STAT_SHADOW_LONGEST_LIST.  Reading it waits for the device */
    RTX_STAT_REFLECT_RAYS = 138,    /* 138 .. 141: the secondary rays of level 1 .. RTX_MAX_REFLECT_DEPTH that the launch set queued last on
                                     * the chain kernels (RTX_OPT_REFLECT_DEPTH > 1, or RTX_OPT_REFLECT_DEPTH_CHECK 1) or on rtx_grid_reflect
                                     * (RTX_OPT_REFLECT_GRID in effect: at any depth) traced; all 0 after a set that took rtx_reflect_hit.  One 4-word device array per context, as
                                     * RTX_STAT_REFLECT_LONGEST_LIST.  Reading it waits for the device.
                                     * No reference counterpart (RayTracing.cu:635) */
    RTX_STAT_REFLECT_SHADOW_POINTS = 142, /* 142 .. 145: the hit points of level 1 .. RTX_MAX_REFLECT_DEPTH that the launch set queued last
                                     * shadow-tested under RTX_OPT_REFLECT_SHADOWS (every point of the level that hit an object; none
                                     * under RTX_OPT_SHADOW_CHECK 2, which tests nothing); all 0 after a set the option had no effect
                                     * on.  One 4-word device array per context, as RTX_STAT_REFLECT_RAYS.  Reading it waits for the
                                     * device.  No reference counterpart (RayTracing.cu:132,635) */
    RTX_STAT_SHADOW_GRID_FRAMES = 146, /* launch sets queued with the shadow tests through the world grid (RTX_OPT_SHADOW_GRID in effect):
                                     * counted as RTX_STAT_SHADOW_FRAMES counts, on either path */
    RTX_STAT_SHADOW_GRID_FALLBACK_POINTS = 147, /* the (point, light) segments of the last such launch set that could not be walked and
                                     * tested every sphere instead, over all levels.  One word per context, as RTX_STAT_SHADOW_LONGEST_LIST.
                                     * Reading it waits for the device, as RTX_STAT_QUERY_FALLBACK_RAYS does */
    RTX_STAT_REFLECT_GRID_FRAMES = 98, /* launch sets queued with the mirror rays through the world grid (RTX_OPT_REFLECT_GRID in effect):
                                     * counted as RTX_STAT_SHADOW_FRAMES counts.  (Numbered below the other counters, as
                                     * RTX_STAT_HALF_FRAMES is) */
    RTX_STAT_REFLECT_GRID_FALLBACK_RAYS = 97, /* the secondary rays of the last such launch set that could not be walked and tested every
                                     * sphere instead, over all levels.  One word per context, as RTX_STAT_REFLECT_LONGEST_LIST.
                                     * Reading it waits for the device, as RTX_STAT_QUERY_FALLBACK_RAYS does */
    RTX_STAT_QUERY_GRID_BUILDS = 122, /* builds of the ray queries' world grid so far: one by the first query after rtx_scene_add_*,
                                     * rtx_scene_clear, rtx_update_objects or a change of RTX_OPT_QUERY_LOAD (or by the first frame after one, under
                                     * RTX_OPT_SHADOW_GRID or RTX_OPT_REFLECT_GRID: the grid is shared); none by a query or a frame on an unchanged scene */
    RTX_STAT_QUERY_FALLBACK_RAYS = 123, /* rays of the last rtx_query_rays / rtx_query_rays_host / rtx_pick call that the grid kernel answered by
                                     * testing every object because they cannot be walked (see rtx_query_rays).  0 after a call under
                                     * RTX_OPT_QUERY_CHECK 1.  Reading it waits for the device */
    RTX_STAT_QUERY_LARGE_SPHERES = 124, /* spheres the last build kept outside the cells, in the list every ray tests: those whose box covers
                                     * more than 64 cells or is not finite */
    RTX_STAT_QUERY_GRID_CELLS = 125, /* cells of the last build (0: no grid) */
    RTX_STAT_QUERY_GRID_PAIRS = 126, /* (sphere, cell) pairs the last build listed */
    RTX_STAT_QUERY_BRUTE = 127,     /* 1 while queries are answered by the brute kernel because the last build found no usable grid: more
                                     * than 256 large spheres, no finite sphere, or coordinates beyond 2^50 or below 2^-50 */
    RTX_STAT_QUERY_GRID_GEOMETRY = 128, /* 128 .. 136: the last build's grid, for checks that aim rays at cell faces and corners: the fp32 bits of
                                     * the low corner x y z, of the cell size x y z, then the cells per axis x y z.  Boundary i of an axis
                                     * is low + (float)i * size, each operation rounded to fp32 */
    RTX_STAT_LIGHTS = 137,          /* lights in the set (rtx_scene_set_lights): 1 .. RTX_MAX_LIGHTS.  No reference counterpart
                                     * (RayTracing.cu:132,143-157) */
    RTX_STAT_SCENE_EDITS = 148,     /* rtx_scene_set_spheres, rtx_scene_set_spheres_device and rtx_scene_set_plane calls that changed something
                                     * (not the refused ones, not n == 0); every member of a device group counts its own, alike.
                                     * No reference counterpart beyond Object3D.cu:34 */
    RTX_STAT_SCENE_EDIT_MOVE = 149, /* the fp32 bits of the displacement bound of the last sphere edit: no centre moved further (formed
                                     * in double on the device, rounded up); 0x7f800000 (+inf) when that edit counted as a full change of
                                     * geometry (a radius changed, or a move that is no finite float); 0 after a colour-only edit.
                                     * No reference counterpart beyond Object3D.cu:34 */
    RTX_STAT_SCENE_REMOVED = 150,   /* objects removed so far by rtx_scene_remove_objects / rtx_scene_remove_marked_device calls that succeeded
                                     * (|R| per call); every member of a device group counts its own, alike.  No reference
                                     * counterpart (Scene3D.h:15-25 creates objects, Scene3D::CleanUp frees all of them at once) */
    RTX_STAT_DELTA_FRAMES = 151,    /* frames rtx_update_delta has handed out so far, key frames included.  No reference counterpart
                                     * (PrintMachine.cpp:257-306, RayTracingManager.cu:150) */
    RTX_STAT_DELTA_KEYFRAMES = 152, /* ... of which were key frames (RTX_DELTA_KEY).  No reference counterpart
                                     * (PrintMachine.cpp:257-306, RayTracingManager.cu:150) */
    RTX_STAT_DELTA_CELLS = 153,     /* cells the last delta launch (rtx_delta_words, or an rtx_update_delta that returned RTX_DELTA_DIFF)
                                     * found changed; 0 before the first.  Two words per context, counted on the device.  Reading it
                                     * waits for the device.  A delta launch of either kind: rtx_half_delta_words and an
                                     * rtx_update_half_delta that returned RTX_DELTA_DIFF write the same two words.
                                     * No reference counterpart (PrintMachine.cpp:257-306, RayTracingManager.cu:150) */
    RTX_STAT_DELTA_RUNS = 154,      /* ... and the runs they form: the cursor escapes of that stream.  With RTX_STAT_DELTA_CELLS a caller
                                     * can tell when a key frame would have been shorter.  Reading it waits for the device.
                                     * Of the last delta launch of either kind, as RTX_STAT_DELTA_CELLS.
                                     * No reference counterpart (PrintMachine.cpp:257-306, RayTracingManager.cu:150) */
    RTX_STAT_SUPERSAMPLE_FRAMES = 100, /* supersampled launch sets queued so far (RTX_OPT_SUPERSAMPLE > 1): counted as
                                     * RTX_STAT_SHADOW_FRAMES counts, one per rtx_render_rows call; stays 0 while S = 1.  (Numbered below
                                     * the other counters: 101 .. 154 are taken.)  No reference counterpart (RayTracing.cu:12-17) */
    RTX_STAT_HALF_FRAMES = 99,      /* frames rtx_update_half has handed out so far.  (Numbered below the other counters, as
                                     * RTX_STAT_SUPERSAMPLE_FRAMES is: 100 .. 154 are taken.)  No reference counterpart
                                     * (RayTracing.cu:256,476 paint one colour per cell; PrintMachine.cpp:257-306) */
    RTX_STAT_HALF_DELTA_FRAMES = 96, /* frames rtx_update_half_delta has handed out so far, key frames included; they count neither in
                                     * RTX_STAT_HALF_FRAMES nor in RTX_STAT_DELTA_FRAMES.  (Numbered below the other counters: 97 .. 154
                                     * are taken.)  No reference counterpart (RayTracing.cu:256,476, PrintMachine.cpp:257-306,
                                     * RayTracingManager.cu:150) */
    RTX_STAT_HALF_DELTA_KEYFRAMES = 95, /* ... of which were key frames (RTX_DELTA_KEY).  No reference counterpart
                                     * (RayTracing.cu:256,476, PrintMachine.cpp:257-306, RayTracingManager.cu:150) */
    RTX_STAT_PATTERNED_OBJECTS = 94, /* objects with a pattern slot above 0 (rtx_scene_set_object_pattern).  (Numbered below the other
                                     * counters: 95 .. 154 are taken.)  No reference counterpart (RayTracing.cu:144) */
    RTX_STAT_PATTERN_FRAMES = 93,   /* launch sets queued while that count is not 0: counted as RTX_STAT_SHADOW_FRAMES counts, on whichever
                                     * of the two paths the frame takes.  No reference counterpart (RayTracing.cu:144) */
    RTX_STAT_REFRACTIVE_OBJECTS = 92, /* objects with ior > 0 (rtx_scene_set_refraction).  (Numbered below the other counters: 93 .. 154
                                     * are taken.)  No reference counterpart (RayTracing.cu:635) */
    RTX_STAT_REFRACT_FRAMES = 91,   /* launch sets queued on the mirror path while that count is not 0: counted as RTX_STAT_SHADOW_FRAMES
                                     * counts.  No reference counterpart (RayTracing.cu:635) */
    RTX_STAT_FINISHED_OBJECTS = 90, /* objects whose finish is not the default's 16 bytes (rtx_scene_set_finish).  (Numbered below the
                                     * other counters: 91 .. 154 are taken.)  No reference counterpart (RayTracing.cu:143-157) */
    RTX_STAT_FINISH_FRAMES = 89,    /* launch sets queued while that count is not 0: counted as RTX_STAT_PATTERN_FRAMES counts.  No
                                     * reference counterpart (RayTracing.cu:143-157) */
    RTX_STAT_SPOT_LIGHTS = 88,      /* lights of the set that have a cone (rtx_scene_set_spots: a dir that is not (0,0,0)).  (Numbered below
                                     * the other counters: 89 .. 154 are taken.)  No reference counterpart (RayTracing.cu:132) */
    RTX_STAT_SPOT_FRAMES = 87,      /* launch sets queued while that count is not 0: counted as RTX_STAT_PATTERN_FRAMES counts.  No
                                     * reference counterpart (RayTracing.cu:132) */
    RTX_STAT_CELL_CAPACITY_FLOOR = 107 /* entries per cell list the current grid is planned with at least (0: the default capacity has
                                     * sufficed); grown from the longest list the binning passes report */
};

/* Flags of rtx_render_rows. */
enum rtx_render_flags {
    RTX_RENDER_DEFAULT = 0,
    /* 8-bit modes use only the first 12*W*H bytes of the 20*W*H frame (RayTracing.cu:238);
     * with this flag the call also zero-fills bytes [12*W*H, 20*W*H) of a full-frame buffer,
     * as the reference's per-frame cudaMemset leaves them (RayTracingManager.cu:86,161-165). */
    RTX_RENDER_ZERO_TAIL = 1,
    /* The output is one 4-byte pixel word per pixel (W*rows words, same row addressing as the records, caller's
     * buffer only) instead of the S-byte record: byte 0..2 = the record's colour values (r, g, b; or the
     * xterm-256 index in byte 0 for the 8-bit modes), byte 3 = the glyph; 0 = pixel without a visible hit;
     * 0xffffffff = column W-1.  rtx_expand turns the words into the very records rtx_render_rows would have
     * written.  For the row-sharded multi-GPU loop: a rank ships 4 instead of 20 bytes per pixel over xGMI and
     * the GPU that assembles the frame writes the records.  No reference counterpart.  Not with RTX_SDL. */
    RTX_RENDER_COMPACT = 2,
    /* The output is the 8 floats behind each record instead of the record (32 bytes per pixel, 16-byte aligned
     * caller's buffer, same row addressing): distance (99999999.f without a hit), shadingValue, normal.xyz,
     * colour.xyz -- struct RayTraceReturnData (RayTracing.h:17-23) after RayTrace (RayTracing.cu:81-168), i.e.
     * the values the 1e-5 parity tolerance is stated on.  Normal and colour are defined for pixels with a hit
     * only; column W-1 is all zero.  For checks, not for the frame loop.  Not with RTX_SDL. */
    RTX_RENDER_VALUES = 4
};

/* One run of pixels for rtx_expand: n_pixels words starting at word src_pixel of the compact buffer become
 * the records starting at record dst_pixel of the output buffer. */
typedef struct rtx_segment {
    uint64_t src_pixel;
    uint64_t dst_pixel;
    uint64_t n_pixels;
} rtx_segment;

/* ---- context: RayTracingManager::RayTracingManager / ~RayTracingManager (RayTracingManager.cu:53-74).
 * Owns the device params block, the 20*max_w*max_h device result buffer (PrintMachine::GetMaxSize(),
 * PrintMachine.cpp:140) and the scene store.  `device` is the HIP device ordinal. */
int rtx_create(int device, size_t max_w, size_t max_h, rtx_ctx** out);
void rtx_destroy(rtx_ctx* ctx);

/* ---- device groups: the `rtx_create(ndev, ...)` of SURVEY.md 8(b) / 8(e).  One context that renders on ndev devices of this
 * process: the frame shards by pixel rows -- logical rank g (device devices[g]; NULL = devices 0 .. ndev-1) traces rows
 * [g*H/ndev, (g+1)*H/ndev) with the global row index in ray generation (RayTracing.cu:12,16) -- and the slabs are gathered
 * into the device memory of rank 0 (the root, devices[0]) by RCCL (ncclCommInitAll; grouped ncclSend / ncclRecv over xGMI,
 * ragged last slab) or hipMemcpyPeerAsync; the root then holds the byte-identical 20*W*H buffer a one-device rtx_render
 * produces (a block of rows is one contiguous byte range, RayTracing.cu:238,457).  The returned context IS the group: every
 * entry point takes it like any other context, and on it
 *   rtx_scene_* / rtx_update_objects / rtx_set_option   apply to every rank's replica of the scene (<= 6.8 MB, replicated),
 *   rtx_render, rtx_update, rtx_update_begin / _end      trace sharded and deliver on the root exactly what they deliver on one
 *                                                        device (frame buffer, minimised stream),
 *   rtx_submit_frames                                    n whole frames, sharded: every rank traces its rows of up to 16 frames with one
 *                                                        launch (RTX_OPT_BATCH) and the slabs of the chunk travel together -- the form
 *                                                        for throughput; the frames are complete in stream order on the context's own
 *                                                        stream, which the streams[i] given are made to wait for,
 *   rtx_render_rows, rtx_submit_slabs, rtx_expand, rtx_minimize, graphs   act on the root's device alone (caller's buffers there),
 *   rtx_destroy                                          releases the whole group.
 * The reference's single consumer, RayTracingManager::Update (RayTracingManager.cu:76-154, hand-off at :150), therefore
 * runs unchanged over N GPUs: include/rtx_compat.hpp takes the device list from RTX_DEVICES or Device::set_devices().
 * A device may appear more than once (several logical ranks on one GPU: how a one-GPU box walks N = 4 or 8; the gather is
 * then peer / same-device copies -- an RCCL communicator needs one rank per GPU).  ndev in [1, 64]. */
int rtx_group_create(int ndev, const int* devices, size_t max_w, size_t max_h, rtx_ctx** out);
int rtx_group_size(const rtx_ctx* ctx);                      /* logical ranks (1 for a plain context) */
rtx_ctx* rtx_group_member(rtx_ctx* ctx, int rank);           /* rank's member context, for reading (statistics, kernel names); rank 0 = ctx */
int rtx_group_rows(const rtx_ctx* ctx, size_t h, int rank, size_t* row0, size_t* rows); /* the rows rank traces of an h-row frame */
const char* rtx_group_exchange_note(const rtx_ctx* ctx);     /* one line: how the last gather moved its bytes, or why RCCL is not in use */

enum rtx_group_exchange {
    RTX_EXCHANGE_AUTO = 0,      /* RCCL where the list names ndev > 1 distinct devices and librccl loads and initialises; else peer copies */
    RTX_EXCHANGE_PEER_COPY = 1, /* hipMemcpyPeerAsync on the sender's stream, ordered by events */
    RTX_EXCHANGE_RCCL = 2,      /* grouped ncclSend / ncclRecv (distinct devices only) */
    RTX_EXCHANGE_RCCL_ALL = 3   /* ... with the root's own slab sent to itself as well: walks the RCCL path at ndev = 1 (tests) */
};
enum rtx_group_wire {
    RTX_WIRE_AUTO = 0,    /* compact */
    RTX_WIRE_RECORDS = 1, /* the 12 / 20-byte records travel and land at their place in the frame */
    RTX_WIRE_COMPACT = 2  /* 4-byte pixel words travel (RTX_RENDER_COMPACT); the root writes the records (rtx_expand) or minimises from the words */
};

/* Text of the last error on this context (or of the last failed rtx_create when ctx is NULL). */
const char* rtx_last_error(const rtx_ctx* ctx);
const char* rtx_version(void);
int rtx_set_option(rtx_ctx* ctx, int option, int64_t value);
int rtx_get_option(const rtx_ctx* ctx, int option, int64_t* value);

/* ---- scene: Scene3D::CreateSphere / CreatePlane / GetObjects (Scene3D.h:15-25, Scene3D.cpp:36-105).
 * Objects are appended (here), edited in place (rtx_scene_set_spheres / rtx_scene_set_plane) and removed one by one or in sets
 * (rtx_scene_remove_objects, which renumbers the survivors); creation order is the closest-hit tie-break order
 * (RayTracing.cu:100-136).
 * No 5 MB arena cap (Scene3D.h:6).  The add calls return the new object's index (>= 0) or -status. */
int rtx_scene_clear(rtx_ctx* ctx);
int rtx_scene_add_sphere(rtx_ctx* ctx, const float pos[3], float radius, const float rgb[3]);
int rtx_scene_add_plane(rtx_ctx* ctx, const float pos[3], const float normal[3], const float rgb[3],
                        float width, float height);
/* The point light of the Blinn-Phong shading, context state like the scene (rtx_scene_clear leaves it alone).  The reference
 * has one light, constant at its call site (RayTracing.cu:132,143-157): position (1, 50, 0), diffuse and specular colour
 * (1, 1, 1), diffuse power 2000, specular power 3000 -- the default here.  Shading keeps the reference's operation order with
 * these values in place of the constants (per component ((colour * intensity) * power) * divDistance).  44 bytes.
 * No reference counterpart. */
typedef struct rtx_light {
    float pos[3];
    float diffuse_rgb[3];
    float diffuse_power;
    float specular_rgb[3];
    float specular_power;
} rtx_light;
/* Sets the light (NULL: the reference's light again).  RTX_ERR_INVALID_ARGUMENT for a non-finite value, a negative power or a
 * negative colour component.  On a device group every rank's replica.  Takes effect for launches queued afterwards; a recorded
 * graph keeps the light (and RTX_OPT_SHADOWS) it was recorded with.  No reference counterpart (RayTracing.cu:132,143-157). */
int rtx_scene_set_light(rtx_ctx* ctx, const rtx_light* light);
/* The light in use.  No reference counterpart (RayTracing.cu:132,143-157). */
int rtx_scene_get_light(const rtx_ctx* ctx, rtx_light* out);
/* Several point lights.  rtx_scene_set_lights replaces the whole set with the n lights given, n in [1, RTX_MAX_LIGHTS], each
 * validated as rtx_scene_set_light validates its one.  All or nothing: n == 0, n > RTX_MAX_LIGHTS, lights == NULL or one bad
 * light changes nothing and returns RTX_ERR_INVALID_ARGUMENT (on a device group: validated before any rank is touched, then
 * applied to every rank).  The colour of a visible pixel (the character modes; RGB_NORMALS and SDL are unaffected) is the
 * reference's expression with the per-light terms summed in the order given: res = 0.2f * od; for each light
 * res = (res + diffuse_i * od) + specular_i * 1.0f; then res * 255.0f and minf(255.0f, .), every operation rounded to fp32 -- for
 * one light the expression of rtx_scene_set_light, operation for operation.  With RTX_OPT_SHADOWS each light gets the shadow test
 * on its own (a light the pixel is shadowed from enters with both powers 0), and one walk of the sphere array per 16 x 16 tile
 * serves all lights.  Mirrors shade their secondary hit with all lights.  Distance, glyph and normal do not depend on lights.  A set
 * of one light launches exactly what rtx_scene_set_light launches; a set of two or more takes the closest-hit launch and then
 * rtx_lights_shade (rtx_lights_reflect_shade on the mirror path), which receives the set by value in its arguments: a recorded
 * graph keeps the set it was recorded with, launches queued afterwards see a change.  rtx_scene_set_light(ctx, L) means
 * rtx_scene_set_lights(ctx, 1, L), and rtx_scene_get_light returns light 0.  Context state like the one light: rtx_scene_clear
 * leaves the set alone.  No reference counterpart (RayTracing.cu:132,143-157). */
#define RTX_MAX_LIGHTS 8
int rtx_scene_set_lights(rtx_ctx* ctx, size_t n, const rtx_light* lights);
/* The set in use: writes min(capacity, n) lights to out (which may be NULL when capacity is 0) and always *n_out = n.
 * No reference counterpart (RayTracing.cu:132,143-157). */
int rtx_scene_get_lights(const rtx_ctx* ctx, size_t capacity, rtx_light* out, size_t* n_out);
/* Spot lights: a cone and a soft edge per light of the set.  rtx_scene_set_spots(ctx, n, spots) takes n = the number of lights in
 * the set (RTX_STAT_LIGHTS; spots[i] belongs to light i) or n = 0 (spots may be NULL: every light is a point light again).  A dir
 * of (0, 0, 0) leaves that light a point light, and its cosines are ignored.  All or nothing: a refused call changes nothing, returns
 * RTX_ERR_INVALID_ARGUMENT and names the first offending light in rtx_last_error (on a device group: validated before any rank is
 * touched, then applied to every rank).  Refused: any other n; spots == NULL with n > 0; a non-zero dir with a component that is
 * not finite, or whose squared length, formed in double, lies outside [2^-40, 2^40]; a cosine that is not finite; cos_outer < -1;
 * cos_inner > 1; cos_inner - cos_outer (one fp32 subtraction) below 2^-10 -- a hard edge is a narrow band.
 * Stored, returned by rtx_scene_get_spots and read by the kernels: the axis a_q = (float)((double)dir_q / sqrt(dx^2 + dy^2 + dz^2)),
 * formed in double, the two cosines, and inv = 1.0f / (cos_inner - cos_outer), one IEEE fp32 division on the host (at most 1024).
 * A point light is stored as five zeros.
 * THE RULE (as code, once: csrc/rtx_spot.hpp).  It applies to a visible pixel in the character modes; RGB_NORMALS and SDL are
 * unaffected.  Wherever the rule of rtx_scene_set_lights enters the powers of light i at a point P -- level 0, and every level j
 * of a mirror or glass chain at P_j -- they are replaced by dpow_i * w and spow_i * w.  With ld the shading's own lightDir after its
 * normalise (normalize_gpu(L_i - P)):
 *     m = (a_x * ld_x + a_y * ld_y) + a_z * ld_z
 *     c = -m
 *     x = (c - cos_outer) * inv
 *     s = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f        (a NaN x gives 0)
 *     w = (s * s) * (3.0f - 2.0f * s)
 * every operation rounded to fp32, nothing reassociated or contracted.  A point light has w = 1, and x * 1.0f is exact: a set
 * without cones gives the bytes it gave before, operation for operation, from the kernels it launched before.  The finish weights,
 * patterns, shadow tests and the chain's fold are unchanged, and so are distance, glyph and normal.  A light that is dark at a point
 * still enters with both powers 0 -- the same float as dpow * 0.0f for a validated power.  So a light whose s at P is not above 0 is
 * treated as dark at P without a segment test: with RTX_OPT_SHADOWS such a pixel is not pending for that light, adds nothing to the
 * light's tile cone, and has no grid segment (neither walked nor counted in RTX_STAT_SHADOW_GRID_FALLBACK_POINTS).  With every cone
 * missing the frame, RTX_STAT_SHADOW_LONGEST_LIST reads 0.
 * The cones belong to the light set: rtx_scene_set_lights and rtx_scene_set_light (NULL included) replace the set, and every light
 * is a point light afterwards -- set the lights first, then the cones.  rtx_scene_clear leaves the cones alone, as it leaves the
 * lights.  The cones travel to the launches by value, as the light set does: a recorded graph keeps the cones it was recorded with,
 * nothing is uploaded, no graph goes stale.  A cone on the reference's light alone, with shadows off, makes a frame that would be
 * one launch the closest-hit launch and rtx_shadow_shade.  While a cone is set, the shade launch is the form of its family that
 * also reads the finishes (default finishes where none was set): if no launch has uploaded the finishes yet, the first frame with a
 * cone does, as the first frame with a finish would -- a graph capture cannot, so render once before capturing.  No reference
 * counterpart (RayTracing.cu:132). */
typedef struct rtx_spot {
    float dir[3];     /* where the light points, any length; (0,0,0): a point light, the cosines are then ignored */
    float cos_outer;  /* cosine of the angle from dir beyond which the light gives nothing */
    float cos_inner;  /* cosine of the angle within which it gives its full powers */
} rtx_spot;           /* 20 bytes */
int rtx_scene_set_spots(rtx_ctx* ctx, size_t n, const rtx_spot* spots);
/* The cones in use, as stored: writes min(capacity, n) entries to out (which may be NULL when capacity is 0) and always *n_out = the
 * number of lights, as rtx_scene_get_lights does.  No reference counterpart (RayTracing.cu:132). */
int rtx_scene_get_spots(const rtx_ctx* ctx, size_t capacity, rtx_spot* out, size_t* n_out);
/* The most levels of secondary rays RTX_OPT_REFLECT_DEPTH takes.  No reference counterpart (RayTracing.cu:635). */
#define RTX_MAX_REFLECT_DEPTH 4
/* Mirror reflections: the reflectivity k in [0, 1] of objects first .. first+n-1 (creation indices, spheres and planes
 * alike: what the add calls return).  Every new object has k = 0; rtx_scene_clear forgets them.  A shaded pixel (the character
 * modes; RGB_NORMALS and SDL are unaffected) whose closest object has k > 0 traces one secondary ray, the view ray mirrored
 * about its normal, from its hit point; its colour becomes minf(255, local * (1 - k) + reflected * k) per component, where
 * `reflected` is the Blinn-Phong colour of the secondary ray's closest hit (the object itself excluded; no shadow test -- deeper
 * levels: see RTX_OPT_REFLECT_SHADOWS -- and no further bounce there at the default depth; black when it hits nothing).  Distance, glyph and normal stay the primary's, so k = 0 gives today's
 * bytes.  While no object has k > 0 every launch is what it is without this call.  All or nothing: a non-finite k, k < 0,
 * k > 1 or a range past rtx_scene_count changes nothing and returns RTX_ERR_INVALID_ARGUMENT (on a device group: validated
 * before any rank is touched, then applied to every rank).  Geometry is unchanged, so sorted copies and cell lists stay valid;
 * a graph recorded before the call is refused by rtx_graph_launch (re-capture).  The device copies are uploaded by the next
 * launch that takes the mirror path, which first waits for the whole device (every stream, every logical rank on it): a change,
 * a scene edit or a new direction sort costs one such wait.  A graph capture cannot do that upload, so recording right after
 * such a change fails with RTX_ERR_INVALID_ARGUMENT ("render once before capturing").
 * The rule for any RTX_OPT_REFLECT_DEPTH (the above is depth 1, operation for operation).  Level 0 is the primary ray r_0, its hit
 * (t_0, o_0) and its local colour local_0: today's, with the shadow tests of RTX_OPT_SHADOWS and every light of the set.  A pixel
 * has a chain when it is visible and k(o_0) > 0.  For j >= 0: level j+1 exists iff j+1 <= depth, level j hit an object and
 * k(o_j) > 0; r_{j+1} = the mirror of r_j at t_j about normal_j (sphere: normalize(normalize(P - C)), plane: normalize(n), with
 * the library's normalize), tested against every object but o_j with the reference's tests for a ray of its own origin and no far
 * limit, the winner the lexicographic minimum of (t, creation index).  For j >= 1 local_j is the Blinn-Phong colour of r_j at t_j
 * with full powers for every light of the set, in order (no shadow test there unless RTX_OPT_REFLECT_SHADOWS asks for one),
 * black when level j hit nothing.  Colours are
 * folded from the deepest level inwards: C_j = local_j when level j+1 does not exist, otherwise
 * C_j = minf(255.0f, local_j * (1.0f - k_j) + C_{j+1} * k_j) per component, each operation rounded to fp32, no contraction.  The
 * pixel's colour is C_0; distance, glyph and normal stay the primary's.
 * No reference counterpart (RayTracing.cu:635 plans a recursive RayTrace). */
int rtx_scene_set_reflectivity(rtx_ctx* ctx, unsigned first, size_t n, const float* k);
/* The reflectivity of object `index`.  No reference counterpart. */
int rtx_scene_get_reflectivity(const rtx_ctx* ctx, unsigned index, float* k);
/* Glass: the index of refraction ior of objects first .. first+n-1 (creation indices, spheres and planes alike).  It belongs to an
 * object as k does: every new object has ior = 0, which means mirror -- today's behaviour; rtx_scene_clear forgets the values,
 * rtx_scene_set_spheres and rtx_scene_set_plane keep them, and after rtx_scene_remove_objects the survivors keep theirs under the
 * renumbering rule.  Accepted: 0, or a finite value in [1, 4].  All or nothing: a NaN, a value in (0, 1), a value above 4, a
 * negative value, a range past rtx_scene_count or ior == NULL with n > 0 changes nothing and returns RTX_ERR_INVALID_ARGUMENT (on a
 * device group: validated before any rank is touched, then applied to every rank).  ior only matters where k > 0: an object with
 * k = 0 has no chain.  While no object has ior > 0 every launch is what it is without this call, and the mirror path's kernels
 * load nothing more.  Geometry is unchanged, so sorted copies, cell lists and the world grid stay valid; a graph recorded before
 * a change is refused by rtx_graph_launch (re-capture).  The device copies are uploaded with the reflectivities', in the same three
 * orders, at the cost of the one device wait stated at rtx_scene_set_reflectivity; recording right after a change fails with
 * RTX_ERR_INVALID_ARGUMENT ("render once before capturing").  No new option and no new launch: RTX_OPT_REFLECT_DEPTH,
 * RTX_OPT_REFLECT_SHADOWS, RTX_OPT_REFLECT_GRID, RTX_OPT_SHADOW_GRID, light sets, patterns, supersampling, half blocks, delta
 * frames and device groups apply as they do to mirrors.
 * The rule.  In the rule of rtx_scene_set_reflectivity one sentence gains a second case: how r_{j+1} is formed from r_j, its hit
 * (t_j, o_j) and normal_j.  With ior(o_j) = 0 it is the mirror ray, bit for bit.  Otherwise take P = r_j.o + r_j.d * t_j,
 * N = normalize(normal_j) and V = normalize(-r_j.d) (the library's normalize, exactly as the mirror ray forms them), with
 * dot(a, b) = (a_x b_x + a_y b_y) + a_z b_z, every operation rounded to fp32, nothing reassociated, no contraction.
 * o_j a sphere of radius r (the stored float), q = x, y, z:
 *   ci  = dot(N, V)
 *   eta = 1.0f / ior
 *   s2  = (eta * eta) * (1.0f - ci * ci)
 *   c2  = 1.0f - s2
 *   ct  = sqrtf(c2 > 0.0f ? c2 : 0.0f)               a NaN c2 gives ct = 0
 *   g   = eta * ci - ct
 *   T_q = N_q * g - V_q * eta                        the unit direction inside
 *   L   = (2.0f * r) * ct                            the chord
 *   o_q = P_q + T_q * L                              the exit point
 *   m   = 2.0f * dot(T, V)
 *   d_q = V_q - T_q * m                              the exit direction
 * with the root and the division correctly rounded.  The exit direction comes from symmetry: reflecting the path in the plane
 * through the centre perpendicular to T maps it onto its own reverse, so there is no second Snell step and no intersection
 * test; with ior >= 1 total internal reflection cannot occur.  o_j a plane (a thin sheet): o = P, d = r_j.d.  In both cases
 * a = dot(d, d), fourA = 4a and divTwoA = 1/(2a), as the mirror ray forms them.  The ray is tested against every object but
 * o_j, exactly as the mirror ray is.  Everything else is unchanged: the existence rule k(o_j) > 0, the fold, the shadow tests at
 * P_j, distance, glyph and normal of the pixel.  As code, once: csrc/rtx_refract.hpp.
 * Out of scope: Fresnel weighting; an object that both mirrors and transmits (a ray tree); anything inside a glass sphere (the
 * interior is treated as empty); attenuated or coloured shadows (glass occludes like any object, unless it is told to cast no shadow at
 * all: rtx_scene_set_shadow_casting); a slab of finite thickness;
 * ior < 1.  No reference counterpart (RayTracing.cu:635 plans a recursive RayTrace). */
int rtx_scene_set_refraction(rtx_ctx* ctx, unsigned first, size_t n, const float* ior);
/* The index of refraction of object `index` (0: a mirror).  No reference counterpart. */
int rtx_scene_get_refraction(const rtx_ctx* ctx, unsigned index, float* ior);
/* Surface finish: how strongly an object shows its own colour under no light, every light's diffuse term and every light's
 * highlight, and how tight that highlight is.  The reference shades every object with its call-site constants (RayTracing.cu:73,
 * 143-157): the default here.  16 bytes. */
typedef struct rtx_finish {
    float ambient;           /* ka: weight of the object colour under no light      (reference: 0.2f) */
    float diffuse;           /* kd: weight of every light's diffuse term            (reference: 1)    */
    float specular;          /* ks: weight of every light's specular term           (reference: 1)    */
    uint32_t shininess_log2; /* m:  the Blinn-Phong exponent is 2^m, m in 0 .. 8    (reference: 5)    */
} rtx_finish;
/* The finish of objects first .. first+n-1 (creation indices, spheres and planes alike).  It belongs to an object as k and ior do:
 * every new object has {0.2f, 1.0f, 1.0f, 5}; rtx_scene_clear forgets the values, rtx_scene_set_spheres and rtx_scene_set_plane
 * keep them, and after rtx_scene_remove_objects the survivors keep theirs under the renumbering rule.  Accepted: ambient, diffuse
 * and specular finite and in [0, 16] (-0.0f is stored as +0.0f), shininess_log2 <= 8.  All or nothing: a NaN or infinity, a
 * negative value, a value above 16, m > 8, a range past rtx_scene_count or finishes == NULL with n > 0 changes nothing and returns
 * RTX_ERR_INVALID_ARGUMENT, and rtx_last_error names the first offending object (on a device group: validated before any rank is
 * touched, then applied to every rank).  While every object has the default finish every launch is what it is without this call,
 * and the shade kernels load nothing more.  Otherwise a frame that would be one trace launch takes the closest-hit launch and
 * rtx_shadow_shade, as a patterned frame does; every other frame keeps its launches, and the shade launch reads 16 more bytes per
 * shaded hit.  Geometry is unchanged, so sorted copies, cell lists and the world grid stay valid; a graph recorded before a change
 * is refused by rtx_graph_launch (re-capture).  The device copies are uploaded with the reflectivities', in the same three orders,
 * at the cost of the one device wait stated at rtx_scene_set_reflectivity; recording right after a change fails with
 * RTX_ERR_INVALID_ARGUMENT ("render once before capturing").  No new option and no new launch: shadows, light sets, mirrors and
 * glass at any depth, the grid options, supersampling, half blocks, delta frames and device groups apply as they do without.
 * The rule, for a visible pixel in the character modes (RGB_NORMALS and SDL are unaffected), at every level j of a mirror or glass
 * chain with the finish (ka, kd, ks, m) of o_j.  In the rule of rtx_scene_set_lights three literals and one function give way to
 * the object's values (q = r, g, b):
 *   x_i   = clampf(dot(nn, h_i), 0, 1)                      as without a finish
 *   si_i  = (float) sq^m((double) x_i)                      m squarings in double, rounded once to float (m = 5: the reference's
 *                                                           pinned pow(x, 32); m = 0: x_i)
 *   res_q = ka * od_q
 *   for each light i, in the order given:
 *   res_q = (res_q + (diffuse_iq * kd) * od_q) + specular_iq * ks
 *   res_q * 255.0f ; minf(255.0f, .)
 * diffuse_iq = ((colour_iq * diffuseIntensity_i) * dpow_i) * divDistance_i and specular_iq = ((colour_iq * si_i) * spow_i) *
 * divDistance_i are formed as without a finish, with si_i in place of the 32nd power.  Every operation is rounded to fp32, nothing
 * is reassociated or contracted; a light the pixel is shadowed from still enters with both powers 0; od is the object's colour
 * after the checker pattern.  With the default finish the expression is the one without, operation for operation (x * 1.0f is
 * exact, five squarings are the 32nd power).  Distance, glyph, normal, the shadow tests, which rays exist, the chain's fold with k
 * and the record encoders do not depend on the finish.  As code, once: csrc/rtx_finish.hpp.
 * Out of scope: a specular colour per object, emission that lights other objects, textures on the coefficients, Fresnel weighting,
 * exponents that are not powers of two.  No reference counterpart (RayTracing.cu:73,143-157). */
int rtx_scene_set_finish(rtx_ctx* ctx, unsigned first, size_t n, const rtx_finish* finishes);
/* The finish of object `index`.  No reference counterpart. */
int rtx_scene_get_finish(const rtx_ctx* ctx, unsigned index, rtx_finish* out);
/* Objects that cast no shadow: glass, light fittings, helper geometry, sky domes -- seen, lit and shadowed, but no obstacle to light.
 * The flag `cast` (0 or 1) of objects first .. first+n-1 (creation indices, spheres and planes alike).  It belongs to an object as k,
 * ior and the finish do: every new object has 1; rtx_scene_clear forgets the values, rtx_scene_set_spheres and rtx_scene_set_plane
 * keep them, and after rtx_scene_remove_objects the survivors keep theirs under the renumbering rule.  All or nothing: a value other
 * than 0 or 1, a range past rtx_scene_count or casts == NULL with n > 0 changes nothing and returns RTX_ERR_INVALID_ARGUMENT, and
 * rtx_last_error names the first offending object (on a device group: validated before any rank is touched, then applied to every
 * rank).
 * The rule.  The shadow test of RTX_OPT_SHADOWS and RTX_OPT_REFLECT_SHADOWS at a point P with normal n on object o, for light i --
 * at level 0 and at every level j of a chain, under every light set and every cone -- changes in one thing: which objects count as
 * occluders.  A plane counts only if it is not o and its cast is 1; a sphere counts only if it is not o and its cast is 1.  Light i
 * is dark at P iff
 *   dot(n, L_i - P) <= 0, or
 *   the open segment (P, L_i) crosses such a plane inside its bounds, or
 *   the segment comes closer than r to the centre of such a sphere,
 * with the expressions of rtx_scene_set_light, operation for operation.  Nothing else changes.  A non-casting object is still hit by
 * primary rays, mirror rays, glass rays and queries; it still receives shadows and still shadows itself (the dot <= 0 test stays);
 * its distance, glyph, normal, pattern and finish, the chain's fold, the cones' rule for which points are tested and rtx_query_rays
 * (RTX_QUERY_ANY included) do not read the flag.
 * What follows from it:
 *   - while every object casts, every launch is what it is without this call, byte for byte and kernel for kernel;
 *   - while some object does not cast but no shadow test runs (RTX_OPT_SHADOWS 0, or RTX_OPT_SHADOW_CHECK 2), the same: nobody
 *     reads the flags;
 *   - a flag never changes the path or the launch sequence of a frame, only which form of a kernel runs: while a shadow test runs
 *     and some object casts no shadow, the launches that make the test are the forms that also read finishes and cones;
 *   - RTX_OPT_SHADOW_CHECK 1 stays the brute reference of the culled path and honours the flags;
 *   - a non-casting sphere is never listed as a candidate: RTX_STAT_SHADOW_LONGEST_LIST counts casting spheres only (under check 1
 *     the number of casting spheres wherever a pixel is pending, 0 when no sphere casts);
 *   - geometry is unchanged, so sorted copies, cell lists and the world grid stay valid (RTX_STAT_QUERY_GRID_BUILDS does not move on
 *     a flag change, and RTX_OPT_SHADOW_GRID keeps walking the shared grid, which holds every sphere).
 * A graph recorded before a change is refused by rtx_graph_launch (re-capture).  The device copies are uploaded with the
 * reflectivities', in the same three orders and once more by creation index, at the cost of the one device wait stated at
 * rtx_scene_set_reflectivity; recording right after a change fails with RTX_ERR_INVALID_ARGUMENT ("render once before capturing").
 * Out of scope: attenuated or coloured shadows (a transmittance per object), a "receives no shadow" flag, objects invisible to
 * primary or mirror rays.  No reference counterpart (the reference casts no shadows). */
int rtx_scene_set_shadow_casting(rtx_ctx* ctx, unsigned first, size_t n, const uint8_t* casts);
/* The flag of object `index` (1: it casts shadows).  No reference counterpart. */
int rtx_scene_get_shadow_casting(const rtx_ctx* ctx, unsigned index, uint8_t* cast);
/* Checker patterns: a second colour per object, chosen by the parity of the lattice cell the hit point lies in.  The table holds
 * up to RTX_MAX_PATTERNS entries, slots 1 .. n; an object carries a slot (0: none, what every new object has).  36 bytes. */
#define RTX_MAX_PATTERNS 16
typedef struct rtx_pattern {
    float origin[3]; /* a corner of the cell lattice, world space */
    float freq[3];   /* cells per world unit along x, y, z; 0 = that axis does not count */
    float rgb[3];    /* the second colour, 0..255 as the add calls take colours */
} rtx_pattern;
/* The rule.  An object with slot s in 1 .. n is shaded (the character modes; RGB_NORMALS and SDL are unaffected) at its hit point
 * P, the point the shading already lights, P_q = r.o_q + r.d_q * t (one multiply, one add), with the colour od chosen by entry s:
 *   u_q = (P_q - origin_q) * freq_q                  q = x, y, z
 *   f   = (floorf(u_x) + floorf(u_y)) + floorf(u_z)
 *   h   = f - 2.0f * floorf(f * 0.5f)
 *   od  = (h != 0.0f) ? od2 : od_object              od2 = rgb / 255.0f, the IEEE division the add calls use
 * every operation rounded to fp32, nothing reassociated, no contraction.  A NaN h selects od2; for |f| >= 2^24 every float is even
 * and the object keeps its own colour; freq_q = 0 with a finite P gives floorf(+-0) = 0, so two zero axes make stripes and one zero
 * axis makes the checker of a floor.  The rule holds at every level of a mirror chain (rtx_scene_set_reflectivity): local_j is
 * shaded with the pattern of o_j at P_j.  Distance, glyph, normal, the shadow tests, the fold of the chain and the record encoders
 * are untouched: only the three od floats that enter Blinn-Phong change.  While no object has a slot above 0 every launch is what
 * it is without these calls, whatever the table holds; otherwise a frame takes the closest-hit launch and a shade launch (the
 * light / shadow path's, or the mirror path's), which read the slots and the table.
 * rtx_scene_set_patterns replaces the table: n in 0 .. RTX_MAX_PATTERNS, n == 0 (patterns may be NULL) clears it.  All or nothing:
 * a non-finite float among an entry's nine, n > RTX_MAX_PATTERNS, patterns == NULL with n > 0, or an n below the slot of some
 * object (rtx_last_error names the object) changes nothing and returns RTX_ERR_INVALID_ARGUMENT.  rtx_scene_set_object_pattern
 * gives objects first .. first+n-1 (creation indices, spheres and planes alike) the slot; it refuses a range past rtx_scene_count
 * and a slot above the table's count.  On a device group both are validated before any rank is touched, then applied to every
 * rank.  The table is context state like the light set: rtx_scene_clear leaves it.  The slots belong to the objects like the
 * reflectivities: rtx_scene_clear forgets them, rtx_scene_set_spheres and rtx_scene_set_plane keep them, and after
 * rtx_scene_remove_objects the survivors keep theirs under the renumbering rule.  Geometry is unchanged, so sorted copies, cell
 * lists and the world grid stay valid; a graph recorded before a change of table or slots is refused by rtx_graph_launch
 * (re-capture).  The device copies are uploaded with the reflectivities' by the next launch that needs them, at the cost stated at
 * rtx_scene_set_reflectivity; recording right after a change fails with RTX_ERR_INVALID_ARGUMENT ("render once before capturing").
 * No reference counterpart (RayTracing.cu:144 reads the one colour an object has). */
int rtx_scene_set_patterns(rtx_ctx* ctx, size_t n, const rtx_pattern* patterns);
/* The table in use: writes min(capacity, n) entries to out (which may be NULL when capacity is 0) and always *n_out = n. */
int rtx_scene_get_patterns(const rtx_ctx* ctx, size_t capacity, rtx_pattern* out, size_t* n_out);
int rtx_scene_set_object_pattern(rtx_ctx* ctx, unsigned first, size_t n, unsigned slot);
/* The slot of object `index` (0: none).  No reference counterpart. */
int rtx_scene_get_object_pattern(const rtx_ctx* ctx, unsigned index, unsigned* slot);
/* Bulk append: n records of 7 floats (cx cy cz r R G B). */
int rtx_scene_add_spheres(rtx_ctx* ctx, size_t n, const float* xyzr_rgb);
unsigned rtx_scene_count(const rtx_ctx* ctx);
/* Sphere::mover / Sphere::speed (Sphere.cu:9-12): the reference draws speed from rand(); here the caller sets it.
 * The reference only ever holds mover = -1 or +1 (Sphere.cu:9,21); any int is accepted, a step then moves the sphere by
 * speed * mover * dt (Sphere.cu:17) and the library's motion bounds (cell-list reuse, dispatch orders) count |speed * mover|. */
int rtx_scene_set_sphere_motion(rtx_ctx* ctx, unsigned index, int mover, float speed);
/* Reads object `index` back from the device store: type (1 plane, 2 sphere, Object3D.h:14) and
 * 11 floats (sphere: cx cy cz r R G B mover speed 0 0; plane: px py pz nx ny nz R G B w h). */
int rtx_scene_get_object(rtx_ctx* ctx, unsigned index, int* type, float out[11]);
/* Edits spheres in place: objects first .. first+n-1 (creation indices, as the add calls return them; every one a sphere) take the
 * centre, radius and colour of their row of 7 floats (cx cy cz r R G B, the rows of rtx_scene_add_spheres; any float is accepted,
 * as the add calls accept any).  The state afterwards is that of a context built by the same add calls in the same order with
 * these values -- od = rgb / 255.0f by the same IEEE division -- and every later launch on every path gives that context's bytes.
 * Unchanged: the creation index (the tie-break), mover and speed, the reflectivity, the light set, every option, the object
 * counts and the array addresses -- recorded graphs stay valid and replay with the new values, as after rtx_update_objects.
 * All or nothing: a range past rtx_scene_count or an index in it that is a plane changes nothing and returns
 * RTX_ERR_INVALID_ARGUMENT (rtx_last_error names the first index that is not a sphere); so does a NULL pointer with n > 0, and
 * a call inside a graph capture on the context's stream (the call waits).  n == 0: RTX_OK, nothing is launched.
 * The call uploads pending appends, makes the context's stream wait for cell-list builds in flight, runs rtx_write_spheres on
 * the context's stream and returns when the edit has been applied; it waits for the device once.  Like every scene change it
 * must not race with frames in flight on other streams.  What it costs later launches: the world grid is rebuilt (as after
 * rtx_update_objects); cell lists and dispatch orders see the largest displacement of a centre exactly as they see a physics
 * step of that size (RTX_STAT_SCENE_EDIT_MOVE; a colour-only edit costs nothing), unless a radius changed or a move is no finite
 * float: then the cell lists are rebuilt and the orders start over.  A new cy outside [-10, 10] makes the next physics step count
 * as the first after an edit (it may pull the sphere onto +-10 from anywhere).  On a device group: validated on the root before
 * any rank is touched, then applied to every rank.  No reference counterpart beyond Object3D.cu:34 (Object3D::SetMiddlePos,
 * Object3D.h:55, which the reference never calls after upload). */
int rtx_scene_set_spheres(rtx_ctx* ctx, unsigned first, size_t n, const float* xyzr_rgb);
/* The same with the rows in device memory of the caller (4-byte aligned, on the context's device; a group's root's), for
 * positions that come out of the caller's own kernels.  `stream` is a hipStream_t (NULL = the context's stream): the edit is
 * ordered after everything queued on it so far, runs on the context's stream and has been applied when the call returns; a
 * capture on either stream is refused.  The rows never come to the host, so the next direction sort (RTX_OPT_SORTED_STORE)
 * still orders by the centres the spheres were created or last edited from the host with: a speed matter only.  On a device
 * group the rows are copied to every other rank (hipMemcpyPeerAsync), behind `stream`.  No reference counterpart beyond
 * Object3D.cu:34. */
int rtx_scene_set_spheres_device(rtx_ctx* ctx, unsigned first, size_t n, const float* d_xyzr_rgb, void* stream);
/* Replaces every field of plane `index` (a creation index that is a plane; anything else: RTX_ERR_INVALID_ARGUMENT, nothing
 * changes) with what rtx_scene_add_plane would have stored for these arguments: the same safe normalise, the same od, the
 * creation index kept.  Blocking (four 16-byte uploads on the context's stream); not inside a graph capture.  Cell lists and the
 * world grid hold spheres only and stay valid; dispatch orders start over.  Reflectivity and everything else that
 * rtx_scene_set_spheres leaves alone stays.  No reference counterpart beyond Object3D.cu:34. */
int rtx_scene_set_plane(rtx_ctx* ctx, unsigned index, const float pos[3], const float normal[3],
                        const float rgb[3], float width, float height);
/* Removes objects: the n objects whose creation indices are listed (spheres and planes mixed, in any order; the set R).
 * THE RULE: afterwards the context is in the state of a context to which the surviving objects were added, in their order, with
 * their CURRENT values -- geometry and colour as rtx_scene_get_object reports them just before the call (physics steps and edits
 * included), the od words bit for bit, mover, speed and reflectivity as they are -- and a surviving object of old index i has the
 * new index  i - |{r in R : r < i}|.  Callers renumber the indices they hold by this rule.  rtx_scene_count drops by |R|, the
 * tie-break order among the survivors is unchanged, and every later launch on every path gives that fresh context's bytes.
 * Removing every object is legal and leaves what rtx_scene_clear leaves (the bound on the spheres' speed may stay as it was: an
 * upper bound).  Unchanged: the light set, every option, the hit buffers.
 * All or nothing: R is checked before anything is touched (on a device group: before any rank is).  An index >= rtx_scene_count,
 * an index listed twice, or indices == NULL with n > 0 changes nothing and returns RTX_ERR_INVALID_ARGUMENT; rtx_last_error names
 * the first offending index.  So does a call inside a graph capture on the context's stream (the call waits).  n == 0: RTX_OK,
 * nothing is launched, RTX_STAT_SCENE_REMOVED is unchanged.
 * The arrays never come to the host: the call uploads pending appends, makes the context's stream wait for cell-list builds in
 * flight, uploads R (4 bytes per removed object, twice) and runs rtx_compact_objects on the context's stream, which moves the
 * survivors into a second set of arrays that then becomes the scene; it returns when that is done, having waited for the device
 * once.  Like every scene change it must not race with frames or queries in flight on other streams.
 * What it costs later launches: object counts and array addresses change, so graphs recorded before are refused by
 * rtx_graph_launch exactly as after rtx_scene_add_*; cell lists, the world grid and the direction-sorted copy are rebuilt;
 * dispatch orders start over; the next physics step counts as the first after an edit.  On a device group: validated on the root,
 * then every member allocates what it needs, and only then does every member compact its own replica (pure moves: the replicas
 * stay identical) -- RTX_ERR_OUT_OF_MEMORY leaves every rank as it was; an RTX_ERR_HIP from a launch or a wait after that point
 * (a lost device) may leave the members with different scenes: destroy the group.
 * No reference counterpart: Scene3D.h:15-25 creates objects and Scene3D::CleanUp frees all of them at once. */
int rtx_scene_remove_objects(rtx_ctx* ctx, size_t n, const unsigned* indices);
/* The same for callers whose own kernels decide what dies (the companion of rtx_scene_set_spheres_device): d_marks is
 * rtx_scene_count bytes of device memory on the context's device (a group's root's), one byte per creation index, non-zero =
 * remove.  `stream` is a hipStream_t (NULL = the context's stream): the marks are read after everything queued on it so far; a
 * capture on either stream is refused.  The call copies the marks to pinned host memory and waits, builds the ascending list
 * of marked indices and takes exactly the path of rtx_scene_remove_objects (a device group sees a host list), so the rule
 * above holds, and it waits for the device once more.  *n_removed (may be NULL) receives |R|.  All marks zero (or an empty
 * scene): RTX_OK, nothing further is launched.  d_marks == NULL with objects in the scene: RTX_ERR_INVALID_ARGUMENT.
 * No reference counterpart: Scene3D.h:15-25 creates objects and Scene3D::CleanUp frees all of them at once. */
int rtx_scene_remove_marked_device(rtx_ctx* ctx, const uint8_t* d_marks, void* stream, size_t* n_removed);

/* ---- render: RayTracing::RayTrace (RayTracing.h:31-38, RayTracing.cu:797-867) together with the
 * zero-fill that precedes it in RayTracingManager::Update (RayTracingManager.cu:86).
 *
 * rtx_render: whole frame into the context's own device buffer, which afterwards holds exactly
 * the bytes the reference's buffer holds after memset + kernel (20*W*H of them).  Asynchronous
 * on the context's stream, like the reference's launch; rtx_synchronize waits
 * (RayTracingManager.cu:137). */
int rtx_render(rtx_ctx* ctx, const rtx_params* params, int mode);

/* Row-slab form for multi-GPU frames: traces rows [row0, row0+rows) with the GLOBAL row index in
 * ray generation (RayTracing.cu:12,16) and writes each row r at d_out + (r - out_row_base)*W*S.
 * d_out is device memory of the caller (NULL = the context's buffer, out_row_base then 0);
 * `stream` is a hipStream_t (NULL = the context's stream). */
int rtx_render_rows(rtx_ctx* ctx, const rtx_params* params, int mode, size_t row0, size_t rows,
                    void* d_out, size_t out_row_base, void* stream, unsigned flags);

/* Queues n whole frames with one call (a renderer keeping several frames in flight): frame i is traced with
 * params[i] into d_outs[i] (each a 20*W*H device buffer of the caller) on streams[i] (hipStream_t).  Frames
 * queued on different streams with different buffers may execute concurrently; on one stream they run in
 * order.  Asynchronous; the caller synchronises its streams.  Same effect as n rtx_render_rows calls.
 * Scene changes (rtx_scene_add_*, rtx_update_objects, rtx_scene_clear) must not race with frames in flight on
 * other streams: synchronise those streams first. */
int rtx_submit_frames(rtx_ctx* ctx, size_t n, const rtx_params* params, int mode, void* const* d_outs, void* const* streams);

/* The row-sharded form of rtx_submit_frames (one rank's share of n consecutive frames in the multi-GPU loop,
 * SURVEY.md 8(e)): rows [row0, row0+rows) of frame i are traced with params[i] into d_outs[i], whose first byte
 * is row out_row_base, on streams[i] (consecutive slabs given the SAME stream are traced by one launch, RTX_OPT_BATCH).  If `after` (a hipStream_t) is not NULL the n slabs are ordered after
 * everything queued on `after` so far, and `after` is made to wait for all of them (event fork/join inside the
 * call), so that the caller can queue the exchange of the slabs on `after` right away.  `flags` as for
 * rtx_render_rows (RTX_RENDER_COMPACT: d_outs[i] receives pixel words).  No reference
 * counterpart (the reference renders whole frames on one device, RayTracingManager.cu:122-135). */
int rtx_submit_slabs(rtx_ctx* ctx, size_t n, const rtx_params* params, int mode, size_t row0, size_t rows,
                     void* const* d_outs, size_t out_row_base, void* const* streams, void* after, unsigned flags);

/* Compact pixel words (RTX_RENDER_COMPACT) -> records of `mode` (12 bytes per pixel for the 8-bit modes, 20 for
 * the RGB ones; the record encoders of RayTracing.cu:206-252, 287-332, 370-472, 507-609, 645-751), for n_segments
 * runs of pixels, on `stream` (NULL = the context's).  d_compact and d_out are device memory of the caller,
 * 4-byte aligned (16-byte aligned destinations take the fast path).  Asynchronous. */
int rtx_expand(rtx_ctx* ctx, int mode, const void* d_compact, void* d_out, const rtx_segment* segments,
               size_t n_segments, void* stream);

/* ---- replayable launch sequences (HIP graphs): a frame loop that queues the same launches round after round (the
 * row-sharded loop: a round's slab launches, a round's expansions) pays one host call per replay instead of one per
 * launch.  rtx_graph_begin puts `stream` (a hipStream_t) into capture; the rtx_submit_slabs / rtx_submit_frames /
 * rtx_render_rows / rtx_expand calls that follow on it (rtx_submit_slabs may fork to its other streams and joins them
 * back) are recorded instead of executed; rtx_graph_end ends the capture and returns an executable graph;
 * rtx_graph_launch replays it on a stream.  Recorded launches keep their arguments (camera, buffers, row range) and
 * the scene arrays' addresses and object counts: a graph belongs to the scene it was recorded on, and after
 * rtx_scene_add_* / rtx_scene_clear rtx_graph_launch refuses it with RTX_ERR_INVALID_ARGUMENT ("re-capture after a scene
 * edit"; rtx_update_objects moves spheres in place and is fine).  Recorded launches need caller buffers (not the
 * context's own frame, whose zero-fill depends on what earlier launches left in it).  Dispatch order: nothing is derived
 * while recording; a recorded launch runs under the order its tile grid has converged to on that stream, if any -- that
 * order is then frozen while a graph that reads it lives (rtx_graph_destroy of the last one releases it) -- and in frame order otherwise.
 * Not recordable, and reported as RTX_ERR_INVALID_ARGUMENT: a launch that needs a scene upload (render once before
 * capturing) or the two-level pre-pass (its lists change from launch to launch).
 * No reference counterpart (one launch per frame on the default stream, RayTracingManager.cu:127-134). */
int rtx_graph_begin(rtx_ctx* ctx, void* stream);
int rtx_graph_end(rtx_ctx* ctx, void* stream, void** graph_out);
int rtx_graph_launch(rtx_ctx* ctx, void* graph, void* stream);
void rtx_graph_destroy(rtx_ctx* ctx, void* graph);

/* ---- ray queries: rays of the caller against the scene.  No reference counterpart (RayTracingManager.cu:21 "Do culling, oct-tree,
 * occlusion" and the empty Culling kernel, :46-51; the reference keeps the mouse's cell, Camera3D.cpp:189-198, and asks nothing with it).
 *
 * A ray is o + t d for t >= 0: d is not normalised and t is in units of d, as everywhere in this path (a = Dot(d, d),
 * RayTracing.cu:90-92).  It is tested with the reference's sphere and plane tests for a ray with its own origin (Sphere.cu:30-68,
 * so a ray that starts inside a sphere misses it; Plane.cu:38-72).  A hit counts iff t <= tmax: INFINITY means no limit, a NaN
 * tmax accepts nothing.  `skip` is a creation index (what the rtx_scene_add_* calls return) that is never reported, or
 * RTX_NO_OBJECT.  32 bytes. */
typedef struct rtx_ray {
    float o[3];
    float tmax;
    float d[3];
    unsigned skip;
} rtx_ray;
/* The answer.  RTX_QUERY_CLOSEST: the lexicographic minimum of (t, creation index) over the objects hit, index = the creation
 * index; nothing hit: t = 99999999.f (RayTracing.h:21), index = RTX_NO_OBJECT.  RTX_QUERY_ANY (occlusion): t = 0 and index =
 * RTX_SOME_OBJECT if any object is hit within tmax, else the no-hit pair; which object stopped the ray is not reported, so the
 * answer does not depend on any order.  8 bytes. */
typedef struct rtx_ray_hit {
    float t;
    unsigned index;
} rtx_ray_hit;
#define RTX_NO_OBJECT 0xffffffffu
#define RTX_SOME_OBJECT 0xfffffffeu
enum rtx_query_flags {
    RTX_QUERY_CLOSEST = 0,
    RTX_QUERY_ANY = 1
};
/* n rays at d_rays -> n answers at d_hits (device memory of the caller, 16- and 8-byte aligned), on `stream` (a hipStream_t; NULL =
 * the context's), ordered after earlier work on that stream; asynchronous.  Rays walk a uniform grid over the spheres' bounding box,
 * built on the GPU by the first query after a scene edit or rtx_update_objects (on the context's stream, which it waits for twice;
 * the caller's stream is made to wait for the build), and test only the spheres listed in the cells they visit, the planes and the
 * few spheres too large for the cells.  The answer is byte for byte the one of testing every object (RTX_OPT_QUERY_CHECK 1): the
 * lists are conservative by a proved bound (csrc/rtx_grid.hpp).  Rays the walk is not proved for -- origin or direction not finite,
 * Dot(d, d) outside [2^-40, 2^40], an origin further from the centre of the spheres' box than three times its largest half-extent
 * on some axis -- are not an error: they test every object (RTX_STAT_QUERY_FALLBACK_RAYS) and get whatever the tests give for them.
 * Must not race with scene edits or physics steps, like frames in flight (rtx_submit_frames).  n = 0: RTX_OK, nothing is launched.
 * NULL pointers with n > 0 or unknown flag bits: RTX_ERR_INVALID_ARGUMENT.  Inside rtx_graph_begin / rtx_graph_end (on the stream
 * given): refused with RTX_ERR_INVALID_ARGUMENT, because a build allocates and waits.  On a device group the scene is replicated:
 * the call runs on the root's device alone, not sharded.  No reference counterpart (RayTracingManager.cu:21,46-51). */
int rtx_query_rays(rtx_ctx* ctx, size_t n, const rtx_ray* d_rays, rtx_ray_hit* d_hits, unsigned flags, void* stream);
/* The same with host memory: copies the rays in, queries on the context's stream, copies the answers out.  Blocking.
 * No reference counterpart (RayTracingManager.cu:21,46-51). */
int rtx_query_rays_host(rtx_ctx* ctx, size_t n, const rtx_ray* rays, rtx_ray_hit* hits, unsigned flags);
/* Which object is under console cell (col, row) of the frame `params` describes: the primary ray of that cell, formed on the
 * device by the very expressions the trace kernels use (RayTracing.cu:12-23), queried with tmax = cam_far and RTX_QUERY_CLOSEST.
 * col >= x - 1 (the newline column) or row >= y: RTX_ERR_INVALID_ARGUMENT.  Blocking.
 * No reference counterpart (Camera3D.cpp:189-198, Engine3D.cpp:199-239 keep the mouse's cell and do nothing with it). */
int rtx_pick(rtx_ctx* ctx, const rtx_params* params, size_t col, size_t row, rtx_ray_hit* hit);

int rtx_synchronize(rtx_ctx* ctx);

/* The context's device result buffer (m_deviceResultArray, RayTracingManager.h:45) and its size. */
void* rtx_frame_device_ptr(rtx_ctx* ctx);
size_t rtx_frame_capacity(const rtx_ctx* ctx);
/* Blocking device-to-host copy of the first `bytes` of that buffer (RayTracingManager.cu:143). */
int rtx_read_frame(rtx_ctx* ctx, void* host_out, size_t bytes);

/* ---- Minimize: RayTracingManager::MinimizeResults / Minimize8bit / MinimizeRGB
 * (RayTracingManager.cu:167-319), on the GPU.  d_in is a 20*W*H frame in device memory (NULL =
 * the context's buffer), d_out device memory with room for S*W*H bytes (NULL = the context's
 * own minimise buffer).  *out_bytes receives the minimised length.  Blocking. */
int rtx_minimize(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_in, void* d_out, size_t* out_bytes);
void* rtx_minimized_device_ptr(rtx_ctx* ctx);
/* The same pass over W*H compact pixel words (RTX_RENDER_COMPACT: what a sharded frame's slabs travel as) instead of records:
 * the stream is byte for byte what rtx_minimize makes of the records rtx_expand would write from these words.  A word
 * 0xffffffff outside column W-1 is an empty slot (a slot whose record would be all NUL).  d_words: device memory, 4-byte
 * aligned; d_out as for rtx_minimize.  Blocking.  Not with RTX_SDL. */
int rtx_minimize_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_words, void* d_out, size_t* out_bytes);

/* ---- UpdateObjects: the physics kernel Update launches before tracing (RayTracingManager.cu:10-44,
 * 89-107; Sphere.cu:15-23), with a launch shape that stays valid past 1024 objects. */
int rtx_update_objects(rtx_ctx* ctx, double dt);

/* ---- RayTracingManager::Update (RayTracingManager.cu:76-154) in one call: params upload, zero
 * semantics, UpdateObjects(dt) when run_physics != 0, trace, GPU minimise, and the copy of the
 * minimised stream to host_out (room for 20*W*H bytes).  On return *out_bytes is what the
 * reference hands to PrintMachine::SetDataInBackBuffer (RayTracingManager.cu:150).  (By default the frame is traced as pixel
 * words and minimised from those, RTX_OPT_UPDATE_WORDS: the stream is the same, the context's frame buffer is left alone.) */
int rtx_update(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics,
               void* host_out, size_t* out_bytes);

/* Pipelined form of rtx_update (the copy of frame k overlapped with the trace of frame k+1).
 * rtx_update_begin queues physics, trace and minimise of a frame, waits for them, then starts the copy of the
 * minimised stream into host_out (pinned memory from rtx_host_alloc for full PCIe rate) on a separate stream and
 * returns a ticket; rtx_update_end(ticket) waits for that copy and reports its length.  At most two frames may
 * be in flight; host_out must stay valid and unread until rtx_update_end. */
int rtx_update_begin(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, void* host_out, int* ticket);
int rtx_update_end(rtx_ctx* ctx, int ticket, size_t* out_bytes);

/* ---- delta frames: only the console cells that changed since the previous frame, addressed by cursor escapes.
 * No reference counterpart: the reference's printer homes the cursor and rewrites the whole screen every frame
 * (PrintMachine.cpp:257-306) from the stream Update hands it (RayTracingManager.cu:150), minimised in space only.
 *
 * THE RULE, on pixel words (RTX_RENDER_COMPACT).  Inputs: one of the five character modes, W, H and two arrays cur and prev of W*H
 * words.  R(w) is the S-byte record rtx_expand writes for word w in that mode (S = 12 or 20), head(w) its first S-1 bytes, glyph(w)
 * its last byte.  Slot g = row*W + col; column W-1 is never a cell.
 *   changed(g)  iff  col < W-1, cur[g] != prev[g] and cur[g] != 0xffffffff
 *   start(g)    iff  changed(g) and (col == 0 or not changed(g-1))
 * A changed slot emits, in this order: if start(g), the cursor escape ESC [ <row+1> ; <col+1> H (decimal, no leading zeros: the
 * frame's cell (0,0) is screen cell (1,1), where ESC [ H puts it); then R(cur[g]) whole if start(g) or head(cur[g]) != head(cur[g-1]),
 * otherwise glyph(cur[g]) alone.  Every other slot emits nothing.  The stream is the concatenation in slot order; a frame equal to its
 * predecessor gives 0 bytes.  The head comparison is stricter than Minimize's (which compares colour digits only, so that a miss in
 * front of a black hit loses its '3' / '4' selector): replaying a delta over the previous frame's grid of records gives exactly
 * the current frame's grid of records, for any words.
 * Limits: W-1 <= 99999 and H <= 99999 (the escape is at most 14 bytes); anything larger is RTX_ERR_INVALID_ARGUMENT.  RTX_SDL and
 * anything that is no mode: RTX_ERR_INVALID_MODE.
 * Out of scope: a form whose launch writes host memory itself (RTX_OPT_UPDATE_HOST_WRITE), a pipelined begin / end form, a device
 * group's gather-free direct update (RTX_OPT_GROUP_UPDATE), bridging short unchanged gaps between runs, and choosing a key frame
 * automatically when it would be shorter -- RTX_STAT_DELTA_CELLS and RTX_STAT_DELTA_RUNS let a caller decide. */
enum rtx_delta_flags {
    RTX_DELTA_DEFAULT = 0,
    RTX_DELTA_KEYFRAME = 1 /* rtx_update_delta: a key frame whatever the context holds */
};
enum rtx_delta_kind {
    RTX_DELTA_KEY = 0, /* the whole frame, byte for byte rtx_update's stream: the consumer homes the cursor first */
    RTX_DELTA_DIFF = 1 /* the rule's stream against the frame handed out before: no cursor home */
};
/* The largest stream either kind can be for a w x h frame of `mode`: the larger of the rule's maximum (per row S c + cup r over c
 * changed cells in r runs) and the key frame's S*w*h.  0 for arguments the other two calls refuse.  Pure host arithmetic.
 * No reference counterpart (PrintMachine.cpp:257-306, RayTracingManager.cu:150; its buffers are 20*W*H, PrintMachine.cpp:140). */
size_t rtx_delta_bound(int mode, size_t w, size_t h);
/* The rule as a pass of its own over the caller's device buffers: d_cur and d_prev W*H words each (4-byte aligned), d_out the
 * stream (16-byte aligned, out_capacity bytes; less than rtx_delta_bound(mode, w, h) returns RTX_ERR_TOO_LARGE before anything is
 * launched), *out_bytes its length.  On the context's stream; blocking, like rtx_minimize_words, and with its launches:
 * RTX_OPT_MINIMIZE_FUSED 0 / 1 / 2 means here what it means there (a launch that gave up is redone as three and counted in
 * RTX_STAT_MINIMIZE_FALLBACKS).  Bytes of d_out past *out_bytes are not written.  On a device group: the root's device alone.
 * No reference counterpart (PrintMachine.cpp:257-306, RayTracingManager.cu:150). */
int rtx_delta_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_cur, const void* d_prev,
                    void* d_out, size_t out_capacity, size_t* out_bytes);
/* rtx_update with a memory of the frame before: physics as rtx_update does it, the frame traced as pixel words by the same path
 * (every shading option applies; a device group traces sharded and gathers), then
 *   a KEY frame (*kind = RTX_DELTA_KEY: byte for byte what rtx_update returns for the frame) when the context holds no valid
 *   previous frame, when the previous frame's W, H or mode differ, when `flags` has RTX_DELTA_KEYFRAME, or when rtx_update or
 *   rtx_update_begin ran on the context since the last call;
 *   otherwise the rule's stream against the frame the last successful call handed out (*kind = RTX_DELTA_DIFF).
 * The two frames live in two word buffers of the context that swap roles (allocated at the first call; the delta's output buffer
 * at first use, rtx_delta_bound bytes).  host_out: room for host_capacity bytes; a stream longer than that returns
 * RTX_ERR_TOO_LARGE, copies nothing, and the next call gives a key frame (so does a call that failed for any other reason).
 * Blocking.  Unknown flag bits: RTX_ERR_INVALID_ARGUMENT.
 * No reference counterpart (PrintMachine.cpp:257-306, RayTracingManager.cu:150). */
int rtx_update_delta(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, unsigned flags,
                     void* host_out, size_t host_capacity, size_t* out_bytes, int* kind);

/* ---- half-block frames: two pixel rows per console row.  Every cell is the glyph U+2580 (upper half block, UTF-8 E2 96 80): the
 * foreground colour paints its top half, the background colour its bottom half, so a W x H console shows W x 2H square pixels.
 * No reference counterpart: its two PIXEL modes paint one background colour under a space (RayTracing.cu:256,476), one tall
 * rectangle per cell, and its printer writes what Update hands it (PrintMachine.cpp:257-306).  Needs a UTF-8 terminal.
 *
 * THE RULE, on pixel words (RTX_RENDER_COMPACT).  Inputs: one of the five character modes, W, H and W * 2H words, row-major: row 2r is
 * the top half of console row r, row 2r+1 the bottom half, column W-1 the newline column as everywhere.
 *   Colour key K(w): a word 0xffffffff outside column W-1 counts as 0 (a miss).  8-bit family (RTX_BIT_ASCII, RTX_BIT_PIXEL):
 *   K = w & 0xff, and 16 for w == 0.  RGB family (the other three): K = w & 0xffffff, r, g, b in bytes 0, 1, 2.  The glyph byte of a
 *   word is ignored: the PIXEL modes are what the feature is for, the others are accepted and the family alone decides.
 *   Escapes SGR(sel, K), sel = '3' for the foreground and '4' for the background, dec() decimal without leading zeros:
 *   RGB ESC [ sel 8 ; 2 ; dec(r) ; dec(g) ; dec(b) m (13 .. 19 bytes), 8-bit ESC [ sel 8 ; 5 ; dec(K) m (9 .. 11 bytes).
 *   Slot g = r*W + c, r in [0, H).  For c < W-1: T = K(words[2rW + c]), B = K(words[(2r+1)W + c]).
 * In slot order: a slot with c == W-1 emits '\n'.  Every other slot is a cell; the cell before it is slot g-1, or g-2 when c == 0 (the
 * last cell of the row above); the frame's first cell has none.  A cell emits SGR('3', T) if there is no cell before it or T differs
 * from that cell's T, then SGR('4', B) likewise for B, then the three bytes E2 96 80.  W == 1: H newlines.
 * The stream is at most H ((W-1)(2E + 3) + 1) bytes, E = 19 for RGB and 11 for 8-bit.  A terminal that keeps the SGR foreground and
 * background state, fed the stream from the home position, shows (T, B) in every cell.
 * Out of scope: a pipelined begin / end form, a launch that writes host memory itself (RTX_OPT_UPDATE_HOST_WRITE), a device group's
 * gather-free direct update (RTX_OPT_GROUP_UPDATE), and a space in place of the glyph where T == B.  Not part of these three calls:
 * delta frames of half-block streams, which are a call family of their own (rtx_update_half_delta, below). */
/* The bound above for a w x h console of `mode`.  0 for anything the other two calls refuse: RTX_SDL or no mode, w == 0 or h == 0,
 * w or 2h of 2^31 or more, a product that does not fit size_t.  Pure host arithmetic.
 * No reference counterpart (RayTracing.cu:256,476; its buffers are 20*W*H, PrintMachine.cpp:140). */
size_t rtx_half_bound(int mode, size_t w, size_t h);
/* The rule as a pass of its own over the caller's device buffers: d_words w * 2h words (4-byte aligned), d_out the stream (16-byte
 * aligned, out_capacity bytes; less than rtx_half_bound(mode, w, h) returns RTX_ERR_TOO_LARGE before anything is launched),
 * *out_bytes its length.  On the context's stream; blocking, like rtx_minimize_words, and with its launches: RTX_OPT_MINIMIZE_FUSED
 * 0 / 1 / 2 means here what it means there (a launch that gave up is redone as three and counted in RTX_STAT_MINIMIZE_FALLBACKS).
 * Bytes of d_out past *out_bytes are not written.  On a device group: the root's device alone.
 * No reference counterpart (RayTracing.cu:256,476, PrintMachine.cpp:257-306). */
int rtx_half_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_words,
                   void* d_out, size_t out_capacity, size_t* out_bytes);
/* rtx_update for a console of params->x columns and params->y rows shown as half blocks: physics exactly as rtx_update runs it, then
 * the sample frame -- `params` with y doubled; ray generation divides by y, so the field of view is what it was -- traced as pixel
 * words by the path rtx_update uses (every shading option and RTX_OPT_SUPERSAMPLE apply; a device group traces sharded and
 * gathers), the rule over those words into a buffer of the context's own (rtx_half_bound bytes, grown on demand) and the stream
 * copied to host_out.  20 * W * 2H above the context's capacity: RTX_ERR_TOO_LARGE -- create the context with twice the rows.  A
 * stream longer than host_capacity: RTX_ERR_TOO_LARGE, and nothing is copied.  Blocking.  Successful or not, the call invalidates
 * rtx_update_delta's previous frame (the screen shows something else): the next delta call gives a key frame.
 * Counted in RTX_STAT_HALF_FRAMES.  No reference counterpart (RayTracing.cu:256,476, PrintMachine.cpp:257-306). */
int rtx_update_half(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics,
                    void* host_out, size_t host_capacity, size_t* out_bytes);

/* ---- delta frames of half-block streams: only the half-block cells whose two colours changed since the previous frame, addressed
 * by cursor escapes.  The delta frames' two-frame memory and runs with the half-block frames' (T, B) keys and escapes.
 * No reference counterpart: its PIXEL modes paint one colour per cell (RayTracing.cu:256,476) and its printer homes the cursor and
 * rewrites the whole screen every frame (PrintMachine.cpp:257-306) from the stream Update hands it (RayTracingManager.cu:150).
 *
 * THE RULE, on pixel words (RTX_RENDER_COMPACT).  Inputs: one of the five character modes, W, H and two arrays cur and prev of W * 2H
 * words each, laid out as rtx_half_words lays them out: row 2r is the top half of console row r, row 2r+1 the bottom half, column W-1
 * the newline column.  K(w), SGR(sel, K), the two families and the glyph E2 96 80 are those of the half-block rule: a word 0xffffffff
 * outside column W-1 counts as 0, the glyph byte of a word is ignored.
 *   Slot g = r*W + c.  For c < W-1: T = K(cur[2rW + c]), B = K(cur[(2r+1)W + c]); Tp, Bp the same of prev.
 *   changed(g)  iff  c < W-1 and (T, B) != (Tp, Bp) -- the displayed keys, not the words: a glyph-only difference is no change, 0
 *                    against 0xffffffff is no change, and in the 8-bit family 0 against a word whose byte 0 is 16 is no change
 *   start(g)    iff  changed(g) and (c == 0 or not changed(g-1))
 * A changed slot emits, in this order: if start(g), the cursor escape ESC [ <r+1> ; <c+1> H (decimal, no leading zeros, as in the
 * delta rule) and then SGR('3', T) and SGR('4', B), both unconditionally; otherwise SGR('3', T) iff T differs from the T of slot g-1
 * in cur, and SGR('4', B) likewise; then the three glyph bytes.  Every other slot emits nothing, the newline column included: a
 * delta addresses its own cells.  The stream is the concatenation in slot order; two frames with equal keys give 0 bytes.
 * A terminal that shows the (T, B) grid of prev and is fed the stream shows the (T, B) grid of cur in every cell afterwards,
 * whatever SGR state it had on entry: every run sets both colours itself.
 * With C = 2E + 3 (41 for RGB, 25 for 8-bit), c changed cells in r runs cost at most C c + cup r, cup the cursor escape's length.
 * Limits: W-1 <= 99999 and H <= 99999; anything larger is RTX_ERR_INVALID_ARGUMENT.  RTX_SDL and anything that is no mode:
 * RTX_ERR_INVALID_MODE.
 * Out of scope: tracking the terminal's SGR state across runs to elide a run's first escapes, bridging short unchanged gaps between
 * runs, choosing a key frame automatically when it would be shorter (RTX_STAT_DELTA_CELLS and RTX_STAT_DELTA_RUNS let a caller
 * decide), a pipelined begin / end form, a launch that writes host memory itself (RTX_OPT_UPDATE_HOST_WRITE), and a device group's
 * gather-free direct update (RTX_OPT_GROUP_UPDATE). */
/* The largest stream either kind can be for a w x h console of `mode`: the larger of the rule's maximum (per row C c + cup r) and
 * the key frame's rtx_half_bound(mode, w, h).  0 for arguments the other two calls refuse.  Pure host arithmetic.
 * No reference counterpart (RayTracing.cu:256,476, PrintMachine.cpp:257-306, RayTracingManager.cu:150). */
size_t rtx_half_delta_bound(int mode, size_t w, size_t h);
/* The rule as a pass of its own over the caller's device buffers: d_cur and d_prev w * 2h words each (4-byte aligned), d_out the
 * stream (16-byte aligned, out_capacity bytes; less than rtx_half_delta_bound(mode, w, h) returns RTX_ERR_TOO_LARGE before anything
 * is launched), *out_bytes its length.  On the context's stream; blocking, like rtx_delta_words, and with its launches:
 * RTX_OPT_MINIMIZE_FUSED 0 / 1 / 2 means here what it means there (a launch that gave up is redone as three and counted in
 * RTX_STAT_MINIMIZE_FALLBACKS).  Bytes of d_out past *out_bytes are not written.  RTX_STAT_DELTA_CELLS and RTX_STAT_DELTA_RUNS read
 * the launch's changed cells and runs.  On a device group: the root's device alone.
 * No reference counterpart (RayTracing.cu:256,476, PrintMachine.cpp:257-306, RayTracingManager.cu:150). */
int rtx_half_delta_words(rtx_ctx* ctx, int mode, size_t w, size_t h, const void* d_cur, const void* d_prev,
                         void* d_out, size_t out_capacity, size_t* out_bytes);
/* rtx_update_half with a memory of the frame before.  Refusals are rtx_update_half's (a character mode; 20 * W * 2H within the
 * context's capacity, else RTX_ERR_TOO_LARGE: create it with twice the rows) with rtx_update_delta's limits and its check of
 * `flags`, in rtx_update_delta's order, and physics runs where rtx_update_delta runs it.  The sample frame -- `params` with y
 * doubled -- is traced as pixel words by the path rtx_update uses (every shading option and RTX_OPT_SUPERSAMPLE apply; a device
 * group traces sharded and gathers), then
 *   a KEY frame (*kind = RTX_DELTA_KEY: byte for byte what rtx_update_half returns for the frame) when the context holds no valid
 *   previous half-block frame, when that frame's W, H or mode differ, when `flags` has RTX_DELTA_KEYFRAME, or when any other entry
 *   point of the family (rtx_update, rtx_update_begin, rtx_update_delta, rtx_update_half) ran on the context since the last call;
 *   otherwise the rule's stream against the frame the last successful call handed out (*kind = RTX_DELTA_DIFF).
 * The context remembers one frame as "what the consumer's screen shows", of one kind: a call of rtx_update_half_delta makes the next
 * rtx_update_delta a key frame as well.  The two frames live in rtx_update_delta's pair of word buffers, grown to W * 2H.  A stream
 * longer than host_capacity returns RTX_ERR_TOO_LARGE, copies nothing, and the next call gives a key frame (so does a call that
 * failed for any other reason).  Blocking.  Counted in RTX_STAT_HALF_DELTA_FRAMES and RTX_STAT_HALF_DELTA_KEYFRAMES, not in
 * RTX_STAT_HALF_FRAMES or RTX_STAT_DELTA_FRAMES.
 * No reference counterpart (RayTracing.cu:256,476, PrintMachine.cpp:257-306, RayTracingManager.cu:150). */
int rtx_update_half_delta(rtx_ctx* ctx, const rtx_params* params, int mode, double dt, int run_physics, unsigned flags,
                          void* host_out, size_t host_capacity, size_t* out_bytes, int* kind);

/* ---- ansi256_from_rgb (ANSIRGB.h:141-189) on its own: the xterm-256 index (16..255) of each packed 0xRRGGBB
 * value first_rgb, first_rgb+1, ..., first_rgb+count-1 (first_rgb + count <= 2^24), one byte per value into
 * d_out (device memory of the caller), computed by the very device function and grey lookup the two 8-bit trace
 * kernels use (RayTracing.cu:210,291).  Lets a checker cover all 2^24 inputs, which no frame does.  Asynchronous
 * on `stream` (NULL = the context's). */
int rtx_ansi256_map(rtx_ctx* ctx, uint32_t first_rgb, size_t count, void* d_out, void* stream);

/* ---- pinned host memory for the buffers Update copies into (m_minimizedResultArray / m_hostResultArray,
 * RayTracingManager.cu:62-66, which the reference allocates pageable): device-to-host copies into it run at
 * PCIe rate instead of through a staging bounce.  Optional: any host pointer is accepted by rtx_update. */
void* rtx_host_alloc(rtx_ctx* ctx, size_t bytes);
void rtx_host_free(rtx_ctx* ctx, void* p);

/* ---- measurement helpers (bench.py): HIP events on the context's stream. */
int rtx_timer_start(rtx_ctx* ctx);
int rtx_timer_stop(rtx_ctx* ctx, float* elapsed_ms); /* records, synchronises, returns start->stop */
/* Name of the kernel the last rtx_render/rtx_render_rows launched (for matching rocprofv3 rows). */
const char* rtx_last_kernel_name(const rtx_ctx* ctx);

/* ---- host-side input builders (no GPU work; pure fp32 host math).
 * rtx_camera_params: what Engine3D::Render fills (Engine3D.cpp:90-97) from Camera3D::Init/Update/
 * GetInverseVMatrix (Camera3D.cpp:8-48, 51-98, 207-376) for a camera at pos with rotation
 * (pitch, yaw, roll); NULL pos/rot = the reference's start pose (Camera3D.h:59-62). */
int rtx_camera_params(size_t w, size_t h, const float pos[3], const float rot[3], rtx_params* out);
/* SURVEY.md Appendix D synthetic scenes (the BASELINE.json configs): fills n_spheres*7 floats
 * (cx cy cz r R G B) and n_planes*11 floats (px py pz nx ny nz R G B w h), n_planes <= 6. */
int rtx_synth_scene(uint32_t seed, size_t n_spheres, size_t n_planes, float element1, float element2,
                    float* spheres_out, float* planes_out);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* RTX_H */
