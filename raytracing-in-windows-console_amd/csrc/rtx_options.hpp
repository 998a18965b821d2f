// rtx_options.hpp -- the context's options (rtx_set_option / rtx_get_option): one field each, and one table row each that says which
// values the option takes and what a refusal reads.  Pure C++, no HIP and no rtx_ctx: a host program can include it
// (tests/host/test_options.cpp).  The four options of a device group (RTX_OPT_GROUP_*) depend on the group's state and are not
// here: rtx_group.cpp.
//
// To add an option: one field, one table row, and a case in the side-effect switch of rtx_api.cpp only if setting it must do more
// than store.
#pragma once

#include "../../include/rtx.h"
#include "rtx_plan.hpp" // kMaxSupersample

#include <cstdint>

namespace rtxopt {

struct Options {
    int64_t kernel = RTX_KERNEL_AUTO;
    int64_t tile_log2w = 0;
    int64_t subtiles = 0;
    int64_t two_level = -1;         // -1 auto, 0 off, 1 on
    int64_t refine = -1;            // -1 auto, 0 off, 1 on
    int64_t cell_capacity = 0;      // entries per coarse cell list; 0 = 4 ns / cells + 1024
    int64_t tile_order = -1;        // -1 = auto (grids of one dispatch round, period 16), 0 = off, k = on: re-derive the order after
                                    // the 1st and 2nd frame of a grid, then every k-th
    int64_t cell_reuse = -1;        // -1 auto (on), 0 off: bin per frame
    int64_t xcd_order = -1;         // -1 auto (on for two-level grids), 0 off
    int64_t view_adapt = -1;        // -1 auto (on), 0 off
    int64_t sorted_store = -1;      // -1 auto (on), 0 off
    int64_t batch = -1;             // -1 auto (on), 0 off: rtx_submit_slabs renders consecutive slabs of one stream with one launch
    int64_t update_words = -1;      // -1 auto (on), 0 off: rtx_update traces pixel words and minimises from them
    int64_t min_fused = -1;         // -1 auto (on), 0 three launches, 1 on, 2 on with blocks that give up (tests)
    int64_t update_host_write = -1; // -1 auto (frames up to 2^17 slots), 0 off, 1 on
    int64_t shadows = 0;
    int64_t shadow_check = 0;
    int64_t reflect_check = 0;
    int64_t query_check = 0;
    int64_t query_load = 0;         // spheres per cell the grid aims at, in 1/16 (0: rtxgrid::kDefaultLoad)
    int64_t lights_check = 0;
    int64_t reflect_depth = 1;
    int64_t reflect_depth_check = 0;
    int64_t reflect_shadows = 0;
    int64_t shadow_grid = 0;
    int64_t supersample = 1;
    int64_t reflect_grid = 0;
};

// An option takes lo .. hi, and `extra` where its range has a hole (elsewhere extra repeats lo).
struct Row {
    int option;
    int64_t Options::*field;
    int64_t lo, hi, extra;
    const char* refusal;
};

inline constexpr Row kRows[] = {
    {RTX_OPT_KERNEL, &Options::kernel, RTX_KERNEL_AUTO, RTX_KERNEL_BINNED, RTX_KERNEL_AUTO, "RTX_OPT_KERNEL: unknown kernel"},
    {RTX_OPT_TILE_LOG2_W, &Options::tile_log2w, 2, 6, 0, "RTX_OPT_TILE_LOG2_W: 0 or 2..6"},
    {RTX_OPT_SUBTILES, &Options::subtiles, 0, 16, 0, "RTX_OPT_SUBTILES: 0..16"},
    {RTX_OPT_TWO_LEVEL, &Options::two_level, -1, 2, -1, "RTX_OPT_TWO_LEVEL: -1 (auto), 0 or 1 (2 is accepted as 1)"}, // (2 is stored and read back as 2)
    {RTX_OPT_REFINE, &Options::refine, -1, 1, -1, "RTX_OPT_REFINE: -1 (auto), 0 or 1"},
    {RTX_OPT_TILE_ORDER, &Options::tile_order, -1, 1 << 20, -1, "RTX_OPT_TILE_ORDER: -1 (auto), 0 (off) or the refresh period in frames"},
    {RTX_OPT_CELL_CAPACITY, &Options::cell_capacity, 0, 1ll << 31, 0, "RTX_OPT_CELL_CAPACITY: 0 (auto) or entries per cell list"},
    {RTX_OPT_CELL_REUSE, &Options::cell_reuse, -1, 1, -1, "RTX_OPT_CELL_REUSE: -1 (auto), 0 or 1"},
    {RTX_OPT_XCD_ORDER, &Options::xcd_order, -1, 1, -1, "RTX_OPT_XCD_ORDER: -1 (auto), 0 or 1"},
    {RTX_OPT_VIEW_ADAPT, &Options::view_adapt, -1, 1, -1, "RTX_OPT_VIEW_ADAPT: -1 (auto), 0 or 1"},
    {RTX_OPT_SORTED_STORE, &Options::sorted_store, -1, 1, -1, "RTX_OPT_SORTED_STORE: -1 (auto), 0 or 1"},
    {RTX_OPT_BATCH, &Options::batch, -1, 1, -1, "RTX_OPT_BATCH: -1 (auto), 0 or 1"},
    {RTX_OPT_UPDATE_WORDS, &Options::update_words, -1, 1, -1, "RTX_OPT_UPDATE_WORDS: -1 (auto), 0 or 1"},
    {RTX_OPT_MINIMIZE_FUSED, &Options::min_fused, -1, 2, -1, "RTX_OPT_MINIMIZE_FUSED: -1 (auto), 0, 1 or 2"},
    {RTX_OPT_UPDATE_HOST_WRITE, &Options::update_host_write, -1, 1, -1, "RTX_OPT_UPDATE_HOST_WRITE: -1 (auto), 0 or 1"},
    {RTX_OPT_SHADOWS, &Options::shadows, 0, 1, 0, "RTX_OPT_SHADOWS: 0 or 1"},
    {RTX_OPT_SHADOW_CHECK, &Options::shadow_check, 0, 2, 0, "RTX_OPT_SHADOW_CHECK: 0, 1 or 2"},
    {RTX_OPT_REFLECT_CHECK, &Options::reflect_check, 0, 2, 0, "RTX_OPT_REFLECT_CHECK: 0, 1 or 2"},
    {RTX_OPT_QUERY_CHECK, &Options::query_check, 0, 1, 0, "RTX_OPT_QUERY_CHECK: 0 or 1"},
    {RTX_OPT_QUERY_LOAD, &Options::query_load, 0, 4096, 0, "RTX_OPT_QUERY_LOAD: 0 (default) or sixteenths of a sphere per cell, up to 4096"},
    {RTX_OPT_LIGHTS_CHECK, &Options::lights_check, 0, 1, 0, "RTX_OPT_LIGHTS_CHECK: 0 or 1"},
    {RTX_OPT_REFLECT_DEPTH, &Options::reflect_depth, 1, RTX_MAX_REFLECT_DEPTH, 1, "RTX_OPT_REFLECT_DEPTH: 1 .. RTX_MAX_REFLECT_DEPTH"},
    {RTX_OPT_REFLECT_DEPTH_CHECK, &Options::reflect_depth_check, 0, 1, 0, "RTX_OPT_REFLECT_DEPTH_CHECK: 0 or 1"},
    {RTX_OPT_REFLECT_SHADOWS, &Options::reflect_shadows, 0, 1, 0, "RTX_OPT_REFLECT_SHADOWS: 0 or 1"},
    {RTX_OPT_SHADOW_GRID, &Options::shadow_grid, 0, 1, 0, "RTX_OPT_SHADOW_GRID: 0 or 1"},
    {RTX_OPT_SUPERSAMPLE, &Options::supersample, 1, rtxplan::kMaxSupersample, 1, "RTX_OPT_SUPERSAMPLE: 1, 2, 3 or 4"},
    {RTX_OPT_REFLECT_GRID, &Options::reflect_grid, 0, 1, 0, "RTX_OPT_REFLECT_GRID: 0 or 1"},
};

// The row of a context option, nullptr for any other number (a group option, a counter, nothing).
inline const Row* find(int option)
{
    for (const Row& r : kRows) {
        if (r.option == option) return &r;
    }
    return nullptr;
}

inline bool accepts(const Row& r, int64_t value) { return (value >= r.lo && value <= r.hi) || value == r.extra; }

// Stores an accepted value.  Otherwise nothing changes and *refusal is what rtx_last_error then reads.
inline bool set(Options& o, int option, int64_t value, const char** refusal)
{
    const Row* r = find(option);
    if (!r || !accepts(*r, value)) {
        *refusal = r ? r->refusal : "unknown option";
        return false;
    }
    o.*(r->field) = value;
    return true;
}

inline bool get(const Options& o, int option, int64_t* value)
{
    const Row* r = find(option);
    if (r) *value = o.*(r->field);
    return r != nullptr;
}

} // namespace rtxopt
