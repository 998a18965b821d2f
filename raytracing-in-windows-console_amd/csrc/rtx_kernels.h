// rtx_kernels.h -- launch interface between the host API (rtx_api.cpp) and the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "rtx_finish.hpp"
#include "rtx_grid.hpp"
#include "rtx_lights.hpp"
#include "rtx_pattern.hpp"
#include "rtx_refract.hpp"
#include "rtx_plan.hpp"

// Kernel-side mode numbers = enum RenderingMode (RayTracingManager.h:21).
enum {
    RTX_K_BIT_ASCII = 0,
    RTX_K_BIT_PIXEL = 1,
    RTX_K_RGB_ASCII = 2,
    RTX_K_RGB_PIXEL = 3,
    RTX_K_RGB_NORMALS = 4,
    RTX_K_SDL = 5
};

// Kernel arguments, passed by value (they land in SGPRs through scalar loads).
struct KArgs {
    float m[12];          // first three rows of inverseVMatrix
    float ox, oy, oz;     // camPos
    float e1, e2, far;    // element1, element2, camFarDist
    float fW, fH;         // (float)W, (float)H
    uint32_t W, H;
    uint32_t row0, row_end;   // rows traced by this launch (global row indices)
    uint32_t out_row_base;    // the row stored at out[0]
    uint32_t ns, np;          // spheres, planes
    uint32_t tile_log2w;      // a sub-tile is 2^lw x 2^(8-lw) pixels (one pixel per thread)
    uint32_t nsub;            // sub-tiles per workgroup (power of two)
    uint32_t sub_log2nx;      // a workgroup's macro tile is 2^lnx sub-tiles wide, nsub >> lnx high
    // Scene, SoA in HBM (creation order within each kind; .w of the colour arrays carries the
    // creation index across kinds as uint bits; the raw colours stay in host-visible arrays of the
    // context for rtx_scene_get_object):
    // What the TRACE kernels read, by position: the direction-sorted copies when there are some (scenes from 256 spheres,
    // RTX_OPT_SORTED_STORE) -- spheres ordered by a Morton code of the direction in which they lie from where the camera stood when
    // the scene was last edited, so that a cell's ~250 spheres sit in a few dozen 128-byte lines instead of 250 (config 5: 9.3 MB
    // of lines per launch in creation order, 2.2 MB sorted) -- else the scene arrays themselves, where position = sphere index.
    // Cell lists hold positions, candidates carry positions, the winner's records are fetched by position.
    const float4* sph_geom;   // cx cy cz r
    const float4* sph_od;     // R/255 G/255 B/255 gidx  (RayTracing.cu:144: colour / 255.0f, hoisted to upload time)
    const uint32_t* sph_sorted_idx; // position -> sphere index (creation order), looked up only to break an exact tie in t; nullptr: identity
    // What rtx_bin_cells reads: the scene array in creation order (in the sorted copy a block's spheres fall into one workgroup's
    // share), and the translation it writes the lists through (nullptr: identity).
    const float4* sph_scene_geom;
    const uint32_t* sph_pos_of;
    const float4* pl_a;       // px py pz width
    const float4* pl_b;       // nx ny nz height
    const float4* pl_od;      // R/255 G/255 B/255 gidx
    const uint8_t* grey;      // 256-byte grey lookup of the xterm-256 mapper
    // Two-level culling (large scenes): per coarse cell a list of sphere indices (cell_cap entries apart, any order) and
    // its count; a count above cell_cap means the list did not fit and the cell's workgroups stage the whole scene.
    // cell_list == nullptr: every workgroup stages the whole scene.
    const uint32_t* cell_list;
    const uint32_t* cell_count;
    uint32_t* cell_list_out;  // rtx_bin_cells writes these two ...
    uint32_t* cell_count_out;
    uint32_t* cell_count_zero; // ... and zeroes this one (the other counter buffer, for the next launch on the stream)
    uint32_t cell_log2gx, cell_log2gy; // a cell is 2^gx x 2^gy macro tiles
    uint32_t cells_x, cells_y;
    uint32_t cell_cap;        // entries per cell list
    // rtx_bin_cells only: the motion budget the lists are built with (rtx_plan.hpp, "cell-list reuse"): they stay valid for
    // cameras whose ray directions differ by at most bin_theta (chord of unit vectors) and whose position -- sphere
    // motion counted in -- by at most bin_delta from this launch's.  0, 0: this camera only.
    float bin_theta, bin_delta;
    uint32_t* cell_max_out;   // rtx_bin_cells: the longest list any cell has needed so far (atomicMax; past half the capacity only), or nullptr
    // Heaviest-first dispatch (speed only; any permutation of the macro tiles renders the same frame): tile_order[b] =
    // bx | by << 16 of the macro tile that workgroup b (linear block index, x fastest) renders, built by
    // rtx_order_tiles / rtx_balance_tiles from tile_cost, the work estimate every workgroup of an earlier launch left
    // for its tile: tile_cost[tile], followed by the workgroups' start and end times (100 MHz clock) by dispatch
    // position: tile_cost[n_tiles + b], tile_cost[2 n_tiles + b].  Either may be nullptr (identity order / no estimate
    // wanted).
    const uint32_t* tile_order;
    uint32_t* tile_cost;
    // View-density feedback for the host (rtx_plan.hpp, ViewDensity), culling kernels: workgroups whose candidate list holds at
    // least longest_from entries atomicMax its length into longest_list[longest_slot] (three words in rotation, slot = epoch
    // mod 3); the first workgroup zeroes the NEXT slot, which the launches of the next epoch fill -- never the previous one,
    // whose copy to the host may still be queued on another stream (an epoch only begins once the copy of the epoch before
    // the last has landed, so the slot being zeroed is always one whose copy is done).  nullptr: no feedback.
    uint32_t* longest_list;
    uint32_t longest_from, longest_slot;
    uint8_t* out;             // records of row out_row_base start here
    uint32_t refine;          // culling kernels: per-wave refinement of the candidate list (dense scenes; nsub <= 2)
    uint32_t compact;         // 1 = RTX_RENDER_COMPACT: out holds one 4-byte pixel word per pixel instead of a record;
                              // 2 = RTX_RENDER_VALUES: out holds 8 floats per pixel (distance, shadingValue, normal, colour)
    // (experiment build only: its extra arguments; nothing in the product build)
    // the culling pyramids' planes (rtx_plan.hpp, EdgeBasis): n_up(cy) = cy up_p + up_q and n_right(cx) = cx right_p + right_q,
    // the normals of a row / column edge that point up / right in the frame; the squared lengths |P|^2, |Qr|^2, |Qc|^2 of the
    // refusal test; the camera plane's unit normal (zero: none)
    float edge_up_p[3], edge_up_q[3], edge_right_p[3], edge_right_q[3];
    float edge_pp, edge_qrqr, edge_qcqc;
    float edge_fwd[3];
    // batched launches (rtx_trace_batch, KBatch): frames in the launch (0: a plain launch), the tile grid of ONE frame
    uint32_t batch_n, batch_gx, batch_gy;
#define RTX_X_SECTION_KARGS
#include "rtx_experiment.inc"
#undef RTX_X_SECTION_KARGS
};

// A batched trace launch (rtx_trace_batch): ONE grid renders the same rows of up to kMaxBatch frames -- a rank's slab of every
// frame of a round in the row-sharded loop, where a single slab (255 workgroups for 135 rows of 1080p) is far too small to fill
// 256 CUs.  What differs from frame to frame travels beside KArgs in the kernel arguments themselves (no upload, recordable in a
// HIP graph as is): camera matrix and position, the culling pyramids' edge basis of that camera, the output buffer.  Frame size,
// projection scalars, far distance, rows, scene and plan are the launch's.  Workgroup b renders tile position b / n of frame
// b % n: the n copies of a tile are neighbours in dispatch order, so that with the tiles sorted heaviest first every CU's share
// (blocks c, c + n_cu, ...) is a stratified sample of the cost distribution.
constexpr int kMaxBatch = 16;
struct KFrame {
    float m[12];
    float ox, oy, oz;
    float edge_up_p[3], edge_up_q[3], edge_right_p[3], edge_right_q[3];
    float edge_pp, edge_qrqr, edge_qcqc;
    float edge_fwd[3];
    uint8_t* out;
};
struct KBatch {
    KFrame f[kMaxBatch];
};

// The light / shadow path's second launch (rtx_shadow_shade): the light of rtx_scene_set_light and what to test.
struct KLight {
    float px, py, pz;
    float dr, dg, db, dpow;
    float sr, sg, sb, spow;
};
struct ShadowArgs {
    const uint2* hits;  // the first launch's closest hits (kOutHit), row row0 of the launch at hits[0]
    KLight light;
    uint32_t test;      // 1: shadow rays (RTX_OPT_SHADOWS on, RTX_OPT_SHADOW_CHECK != 2); 0: every pixel lit
    uint32_t brute;     // 1: no culling, every sphere tested (RTX_OPT_SHADOW_CHECK 1)
    uint32_t* longest;  // atomicMax of the longest occluder list a workgroup held, or nullptr
};

// The shading launch for a set of several lights (rtx_lights_shade, rtx_lights_reflect_shade): the set of rtx_scene_set_lights by
// value (a recorded graph keeps it, nothing is uploaded) and what to test, as ShadowArgs.
struct LightsArgs {
    const uint2* hits;       // the first launch's closest hits (kOutHit), row row0 of the launch at hits[0]
    rtxlights::Block lights; // the count and the lights, in the order given
    uint32_t test;           // 1: shadow rays to every light; 0: every pixel lit by every light
    uint32_t brute;          // 1: no culling, every sphere a candidate for every live light (RTX_OPT_SHADOW_CHECK 1)
    uint32_t* longest;       // atomicMax of the most list entries a workgroup held, or nullptr
};

// Spot lights (rtx_scene_set_spots): the same arguments with the cones behind them, by value as the lights are.  Only the launches
// that read cones take these -- the FIN forms of the shade families (which then read finishes and cones: launched while an object
// has a finish or a light has a cone) and the SPOT forms of the two shadow passes; every other kernel's argument block is what it
// was before there were cones.
// Objects that cast no shadow (rtx_scene_set_shadow_casting): one byte per object, 0 for an object the shadow tests do not count as
// an occluder.  All nullptr while every object casts, or while the launch runs no shadow test: then nothing is loaded.  The flags
// travel with the cones, to the same launches -- the rich forms, which are then launched while an object has a finish, a light has a
// cone or an object casts no shadow under a running shadow test.  The device copies travel with the reflectivities'.
struct CastArgs {
    const uint8_t* sph;   // the spheres' flags, by the position the trace kernels index them by (KArgs::sph_geom's order): the walks
    const uint8_t* pl;    // the planes', by plane index
    const uint8_t* gidx;  // every object's, by creation index: the grid's lists know spheres by GridShadowArgs::list_gidx
};
struct SpotShadowArgs : ShadowArgs {
    rtxspot::Packed spot;    // light 0's
    CastArgs cast;
};
struct SpotLightsArgs : LightsArgs {
    rtxspot::Block spots;    // spot[i] belongs to lights.light[i]
    CastArgs cast;
};
template <bool SPOT>
using ShadowArgsOf = std::conditional_t<SPOT, SpotShadowArgs, ShadowArgs>;
template <bool SPOT>
using LightsArgsOf = std::conditional_t<SPOT, SpotLightsArgs, LightsArgs>;

// The mirror path (rtx_scene_set_reflectivity): its second launch (rtx_reflect_hit) traces one secondary ray per reflective pixel
// from the first launch's closest hits and writes its closest hit; its third (rtx_reflect_shade) shades as rtx_shadow_shade and
// blends the secondary hit's colour in.
struct ReflectArgs {
    const uint2* hits;   // the first launch's closest hits (kOutHit), row row0 of the launch at hits[0]
    uint2* hits2;        // (t, object) of each reflective pixel's secondary ray, laid out as `hits`; other pixels' entries are not written
    const float* k_sph;  // reflectivity of the spheres, by the position the trace kernels index them by (KArgs::sph_geom's order)
    const float* k_pl;   // ... of the planes, by plane index
    uint32_t brute;      // 1: no culling, every sphere tested (RTX_OPT_REFLECT_CHECK 1)
    uint32_t* longest;   // atomicMax of the longest candidate list a workgroup held, or nullptr
    // glass (rtx_scene_set_refraction): the index of refraction of the spheres and of the planes, ordered as k_sph and k_pl are;
    // both nullptr while no object is refractive -- nothing is loaded then and every secondary ray is the mirror's
    const float* ior_sph;
    const float* ior_pl;
};

// Checker patterns (rtx_scene_set_patterns) and finishes, for the shade launches alone: the slot of every object and the table.  table ==
// nullptr (no object has a slot): nothing is loaded and od is the object's.  The device copies travel with the reflectivities'.
struct PatternArgs {
    const uint8_t* slot_sph;          // slot of the spheres, by the position the trace kernels index them by (KArgs::sph_geom's order)
    const uint8_t* slot_pl;           // ... of the planes, by plane index
    const rtxpattern::Entry* table;   // entry s - 1 serves slot s
    uint32_t n;                       // entries; a slot above it (none is stored) counts as 0
    // surface finishes (rtx_scene_set_finish): 16 bytes per object, ordered as slot_sph and slot_pl are; both nullptr while every
    // object has the default finish -- then the launch is the family's kernel without finishes, which never reads them, else its FIN form
    const rtx_finish* fin_sph;
    const rtx_finish* fin_pl;
};

// Mirrors that see mirrors (RTX_OPT_REFLECT_DEPTH): rtx_reflect_chain traces every level in one launch and rtx_lights_chain_shade
// folds the chain.  The hit buffer holds depth + 1 hit arrays of px entries: level j's at ReflectArgs::hits + j * px (hits2 is
// level 1's).  By value, so a recorded graph keeps its depth.
constexpr int kMaxReflectDepth = 4; // = RTX_MAX_REFLECT_DEPTH
struct ChainArgs {
    uint32_t depth;  // levels of secondary rays, 1 .. kMaxReflectDepth
    uint32_t px;     // pixels of the launch (W * rows): the stride between the levels' hit arrays
    uint32_t* rays;  // kMaxReflectDepth words: the secondary rays traced per level (one atomicAdd per workgroup and level), or nullptr
};

// Shadows seen in mirrors (RTX_OPT_REFLECT_SHADOWS): rtx_chain_shadow, between rtx_reflect_chain and the shade launch, runs the
// shadow test at every deeper level's hit point and leaves one word per pixel, which rtx_lights_chain_shadow_shade reads.  The
// words follow the depth + 1 hit arrays in the hit buffer: 8 (depth + 1) + 4 bytes per pixel.
struct ChainShadowArgs {
    uint32_t* dark;    // px words, laid out as the hits: bit 8 (j - 1) + i: light i is dark at level j
    uint32_t* points;  // kMaxReflectDepth words: the hit points tested per level (one atomicAdd per workgroup and level), or nullptr
};

// Shadow tests through the world grid (RTX_OPT_SHADOW_GRID): rtx_grid_shadow, after the hits are known (the trace launch, and on
// the mirror path rtx_reflect_hit / rtx_reflect_chain) and before the shade launch, walks every pixel's segments through the ray
// queries' grid and leaves level 0's dark lights a word per pixel (dark0, behind everything else in the hit buffer: 4 more bytes
// per pixel), and with `deep` the deeper levels' in ChainShadowArgs::dark as rtx_chain_shadow does.  The shade launch reads both.
struct GridShadowArgs {
    rtxgrid::Grid grid;
    const uint32_t* cell_start; // the build's lists, as QueryArgs has them
    const float4* list_geom;
    const uint32_t* list_gidx;
    const float4* scene_geom;   // the scene arrays in creation order, which the large list indexes
    const float4* scene_od;
    const uint32_t* large;
    uint32_t n_large;
    uint32_t deep;              // 1: the levels 1 .. ChainArgs::depth are tested too (RTX_OPT_REFLECT_SHADOWS in effect)
    uint32_t* dark0;            // px words, laid out as the hits: bit i: light i is dark at level 0
    uint32_t* fallback;         // the (point, light) segments that tested every sphere because they cannot be walked (atomicAdd)
};

// Mirror rays through the world grid (RTX_OPT_REFLECT_GRID): rtx_grid_reflect, in place of rtx_reflect_hit / rtx_reflect_chain, walks
// every reflective pixel's secondary rays of every level through the ray queries' grid and leaves the hit arrays rtx_reflect_chain
// leaves (ReflectArgs::hits2, ChainArgs).  The grid's views are the ones GridShadowArgs carries.
struct GridReflectArgs {
    rtxgrid::Grid grid;
    const uint32_t* cell_start; // the build's lists, as QueryArgs has them
    const float4* list_geom;
    const uint32_t* list_gidx;
    const float4* scene_geom;   // the scene arrays in creation order, which the large list indexes
    const float4* scene_od;
    const uint32_t* large;
    uint32_t n_large;
    const uint32_t* pos_of_gidx; // one word per object: creation index -> the position KArgs::sph_geom knows the sphere by (planes: unused)
    uint32_t* fallback;         // the rays, over all levels, that tested every sphere because they cannot be walked (atomicAdd)
};

// Ray queries (rtx_query_rays): n rays of the caller against the scene arrays in creation order (spheres are known by sphere
// index here, not by the direction-sorted position the trace kernels use), through the world grid or against every sphere.
struct QueryArgs {
    const float4* rays;       // two float4 per ray: o.xyz tmax | d.xyz skip
    uint2* hits;              // t bits, creation index
    uint32_t n;
    uint32_t any;             // RTX_QUERY_ANY
    const float4* sph_geom;   // cx cy cz r, by sphere index
    const float4* sph_od;     // .w: creation index
    const float4* pl_a;
    const float4* pl_b;
    const float4* pl_od;
    uint32_t ns, np;
    rtxgrid::Grid grid;
    const uint32_t* cell_start; // cells + 1 offsets into the two arrays below
    const float4* list_geom;    // per (cell, sphere) pair, grouped by cell, ascending sphere index within a cell: the sphere's geometry ...
    const uint32_t* list_gidx;  // ... and its creation index
    const uint32_t* large;      // sphere indices every ray tests (ascending)
    uint32_t n_large;
    uint32_t* fallback;         // rays of the launch that tested every sphere because they could not be walked (atomicAdd)
};

// The grid's build (rtx_grid_* kernels), in launch order: bounds -> [host: rtxgrid::plan_grid] -> count -> scan -> [host: allocate the
// pair arrays] -> scatter -> sort.
struct GridBuildArgs {
    const float4* sph_geom;
    const float4* sph_od;
    uint32_t ns;
    rtxgrid::Grid grid;
    uint32_t n_cells;
    float* bounds;            // out of bounds: lo xyz, hi xyz of the finite spheres' boxes, then (as uint bits) how many are finite
    uint32_t* cell_count;     // cells + 1 words: counts, then (scan) exclusive offsets with the pair total in the last word
    uint32_t* cell_fill;      // cells words, zeroed: scatter's cursors
    uint8_t* is_large;        // ns flags (count)
    uint32_t* large;          // kLargeCap sphere indices, ascending (scan)
    uint32_t* totals;         // [0] pairs, [1] large spheres (scan)
    uint32_t* pair_tmp;       // scatter: sphere index per pair, any order within a cell
    float4* list_geom;        // sort
    uint32_t* list_gidx;
};

// Arguments of rtx_expand_words (compact pixel words -> records), by value.
constexpr int kMaxExpandSeg = 16;
constexpr int kExpandPixels = 1024;             // pixels per workgroup
struct ExpandArgs {
    const uint32_t* src;                    // compact words
    uint8_t* dst;                           // records
    uint32_t nseg;
    uint32_t aligned16;                     // every destination segment starts on a 16-byte boundary
    uint32_t first_block[kMaxExpandSeg + 1]; // workgroups [first_block[k], first_block[k+1]) expand segment k
    uint32_t npix[kMaxExpandSeg];
    uint64_t src_px[kMaxExpandSeg];         // first pixel of the segment in src / dst
    uint64_t dst_px[kMaxExpandSeg];
};

extern "C" {
int rtx_k_launch_expand(const ExpandArgs* e, int mode, unsigned blocks, void* stream);
// Launches the trace kernel for `mode`; returns the kernel's name (NULL for an invalid mode) and
// the hipGetLastError() value in *hip_error.
const char* rtx_k_launch_trace(const KArgs* a, int mode, int cull, void* stream, int* hip_error);
// The batched form (culling kernels without per-wave refinement, records or compact words): a->batch_n frames of kb in one launch.
const char* rtx_k_launch_trace_batch(const KArgs* a, const KBatch* kb, int mode, void* stream, int* hip_error);
// The launches behind the trace launch, as rtxplan::plan_shading (rtx_plan.hpp) orders them.  a->compact == 3 asks
// rtx_k_launch_trace for the closest hits alone (8 bytes per pixel into a->out, whatever the mode); the passes add to the hit
// buffer, and the shade launch of `family` writes a->out as `mode`'s records / words / values (a->compact 0 / 1 / 2).  Character
// modes only.  What a pass or a family does not take may be NULL; what it takes and finds missing or invalid (a light set of 0 or
// more than 8, a chain whose depth or stride does not fit the launch, no room for its words) refuses the launch: NULL.
struct TileArgs {
    const KArgs* a;
    const ShadowArgs* shadow;      // rtx_shadow_shade, rtx_reflect_shade
    const LightsArgs* lights;      // every other family; rtx_chain_shadow, rtx_grid_shadow
    const rtxspot::Block* spots;   // the cones of the set (rtx_scene_set_spots), or NULL while no light has one: the forms that read cones
    const CastArgs* cast;          // the shadow-casting flags (rtx_scene_set_shadow_casting), or NULL while no launch reads them: the same forms
    const ReflectArgs* reflect;    // the mirror path
    const ChainArgs* chain;        // ... through the chain kernels
    const ChainShadowArgs* deep;   // ... with the deeper levels shadow-tested
    const GridShadowArgs* grid;    // rtx_grid_shadow (which takes reflect, chain and deep by value: zero-filled where there is none)
    const uint32_t* dark0;         // the grid families: GridShadowArgs::dark0
    const GridReflectArgs* grid_reflect; // rtx_grid_reflect
    const PatternArgs* pattern;    // every shade family, by value (NULL: none, as a zero-filled one)
};
const char* rtx_k_launch_pass(rtxplan::ShadePass pass, const TileArgs* t, void* stream, int* hip_error);
const char* rtx_k_launch_shade(rtxplan::ShadeFamily family, const TileArgs* t, int mode, void* stream, int* hip_error);
// The fold of a supersampled launch (RTX_OPT_SUPERSAMPLE): S x S samples of `samples` (the values of the S a->W wide sample frame, its row
// S a->row0 first) per cell of a's rows, encoded into a->out as `mode` (the five character modes) and a->compact (0 / 1 / 2) say.
const char* rtx_k_launch_resolve(const KArgs* a, const void* samples, int S, int mode, void* stream, int* hip_error);
// kind 0: rtx_query_grid, 1: rtx_query_brute.  Returns the hipGetLastError() value.
int rtx_k_launch_query(const QueryArgs* q, int kind, void* stream);
// step 0 bounds, 1 count, 2 scan, 3 scatter, 4 sort
int rtx_k_launch_grid_build(const GridBuildArgs* b, int step, void* stream);
// the primary ray of cell (col, row) of the frame a describes, as the trace kernels form it, with tmax = a->far and no skip: one rtx_ray at d_ray
int rtx_k_launch_pick_ray(const KArgs* a, uint32_t col, uint32_t row, void* d_ray, void* stream);
int rtx_k_launch_bin_cells(const KArgs* a, unsigned splits, void* stream);
int rtx_k_launch_zero(void* p, size_t bytes, void* stream);
// tile_cost[n_tiles] (grid gx wide) -> tile_order[n_tiles], heaviest first, dealt over n_cu compute units so that the
// workgroups each unit receives in the first dispatch round (blocks c, c + n_cu, c + 2 n_cu, ...) carry equal work.
// The same for a grid whose workgroups are all resident at once (n_tiles <= 2048, n_cu <= 1024): tile_cost holds 3 n_tiles
// words (estimates by tile; start and end times by dispatch position, as the trace kernel leaves them), factor[n_tiles]
// the per-tile corrections carried from launch to launch, prev_order the order the times were taken under (NULL: frame
// order; may be tile_order itself).
int rtx_k_launch_balance_tiles(const uint32_t* tile_cost, uint32_t n_tiles, uint32_t gx, uint32_t n_cu, const uint32_t* prev_order, float* factor,
                               int have_factor, int have_times, uint32_t* tile_order, void* stream);
int rtx_k_launch_order_tiles(const uint32_t* tile_cost, uint32_t n_tiles, uint32_t gx, uint32_t n_cu, uint32_t first_round, const uint32_t* base_order,
                             uint32_t* tile_order, void* stream);
}
