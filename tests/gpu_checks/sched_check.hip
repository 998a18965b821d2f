// sched_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests/test_gpu_sched_check.py).
// Runs the three passes in front of a culled trace launch on inputs of the caller's making: rtx_bin_cells (rtx_bin_cells.inc),
// rtx_order_tiles and rtx_balance_tiles (rtx_order_kernels.inc) -- the very text rtx_kernels.hip compiles, launched through the
// same inline rules (launch_bin_cells, launch_order_tiles, launch_balance_tiles) as the rtx_k_launch_* wrappers: what they refuse,
// the first_round clamp, the feedback's damping and step, the grid of the coarse-cell pass.  Nothing is rewritten here.
//
// Arrays in, arrays out.  Every output array is handed in by the caller with whatever it wants to find untouched (poison beyond
// the words a pass may write: `guard` more words are uploaded, and come back, behind each of them) and comes back as the device
// left it.  rtx_check_xcd_cell_order is the host's static base order (rtx_plan.hpp), for rtx_order_tiles.  Every entry point
// returns 0, -1 on a HIP error, -2 on arguments it or the production rule refuses: nothing is launched.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_cull.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_workgroup.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "check_args.hpp"

// BSTAMP, RTX_X_BALANCE_*: the product build's no-ops
#define RTX_X_SECTION_DEVICE
#include "../../raytracing-in-windows-console_amd/csrc/rtx_experiment.inc"
#undef RTX_X_SECTION_DEVICE
#define RTX_X_SECTION_HOST
#include "../../raytracing-in-windows-console_amd/csrc/rtx_experiment.inc"
#undef RTX_X_SECTION_HOST

#ifndef RTX_WAVES_PER_EU
#define RTX_WAVES_PER_EU 7 // rtx_kernels.hip
#endif

namespace rtx {
#include "../../raytracing-in-windows-console_amd/csrc/rtx_bin_cells.inc"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_order_kernels.inc"
} // namespace rtx

namespace {

using rtx_check::args_of;
using rtx_check::Buffers;

constexpr unsigned kMaxGuard = 1u << 20;

bool is_pow2(unsigned v) { return v != 0 && (v & (v - 1u)) == 0; }

} // namespace

#define RTX_CHECK_API extern "C" __attribute__((visibility("default")))

// rtx_order_tiles.  cost: n words; base: n packed tiles or NULL; order: n + guard words, in and out.
RTX_CHECK_API int rtx_check_order_tiles(const uint32_t* cost, unsigned n, unsigned gx, unsigned n_cu, unsigned first_round, const uint32_t* base,
                                        uint32_t* order, unsigned guard)
{
    if (!cost || !order || n > (1u << 20) || guard > kMaxGuard) return -2;
    Buffers b;
    const uint32_t* d_cost = (const uint32_t*)b.up(cost, (size_t)n * 4);
    const uint32_t* d_base = base ? (const uint32_t*)b.up(base, (size_t)n * 4) : nullptr;
    uint32_t* d_order = (uint32_t*)b.up(order, ((size_t)n + guard) * 4);
    if (!b.ok) return -1;
    const int rc = rtx::launch_order_tiles(d_cost, n, gx, n_cu, first_round, d_base, d_order, 0);
    if (rc == (int)hipErrorInvalidValue) return -2;
    return rc == 0 && b.ran() && b.down(order, d_order, ((size_t)n + guard) * 4) ? 0 : -1;
}

// rtx_balance_tiles.  cost: 3 n words (estimates by tile, start and end stamps by dispatch position); prev: n packed tiles, or NULL;
// prev_is_order: the previous order is the output buffer itself (its first n words as handed in); factor: n + guard floats and
// order: n + guard words, in and out.
RTX_CHECK_API int rtx_check_balance_tiles(const uint32_t* cost, unsigned n, unsigned gx, unsigned G, const uint32_t* prev, int prev_is_order, float* factor,
                                          int have_factor, int have_times, uint32_t* order, unsigned guard)
{
    if (!cost || !factor || !order || n > (1u << 20) || guard > kMaxGuard || (prev && prev_is_order)) return -2;
    Buffers b;
    const uint32_t* d_cost = (const uint32_t*)b.up(cost, (size_t)n * 12);
    const uint32_t* d_prev = prev ? (const uint32_t*)b.up(prev, (size_t)n * 4) : nullptr;
    float* d_factor = (float*)b.up(factor, ((size_t)n + guard) * 4);
    uint32_t* d_order = (uint32_t*)b.up(order, ((size_t)n + guard) * 4);
    if (!b.ok) return -1;
    const int rc = rtx::launch_balance_tiles(d_cost, n, gx, G, prev_is_order ? d_order : d_prev, d_factor, have_factor, have_times, d_order, 0);
    if (rc == (int)hipErrorInvalidValue) return -2;
    return rc == 0 && b.ran() && b.down(order, d_order, ((size_t)n + guard) * 4) && b.down(factor, d_factor, ((size_t)n + guard) * 4) ? 0 : -1;
}

// rtx_bin_cells.  cam: 21 floats as cull_check.hip takes them.  shape: tile_log2w, nsub, sub_log2nx, cell_log2gx, cell_log2gy, cells_x,
// cells_y, cell_cap, row0.  spheres: ns x (centre, radius); pos_of: ns words or NULL.  In and out: counts (cells + guard words, which
// the caller zeroes as the product does), lists (cells x cell_cap + guard), zeroed (cells + guard: the other counter buffer),
// cell_max (one word).
RTX_CHECK_API int rtx_check_bin_cells(const float* cam, unsigned W, unsigned H, const uint32_t* shape, float bin_theta, float bin_delta, const float* spheres,
                                      unsigned ns, const uint32_t* pos_of, unsigned splits, uint32_t* counts, uint32_t* lists, uint32_t* zeroed, uint32_t* cell_max,
                                      unsigned guard)
{
    if (!cam || !shape || !spheres || !counts || !lists || !zeroed || !cell_max || guard > kMaxGuard) return -2;
    const unsigned lw = shape[0], nsub = shape[1], lnx = shape[2], gx = shape[3], gy = shape[4], cells_x = shape[5], cells_y = shape[6], cap = shape[7], row0 = shape[8];
    if (W == 0 || H == 0 || W > (1u << 16) || H > (1u << 16) || row0 >= H || lw > 8 || !is_pow2(nsub) || nsub > 16 || (1u << lnx) > nsub || gx > 4 || gy > 4) return -2;
    if (ns == 0 || ns > (1u << 20) || splits == 0 || splits > 64 || cells_x == 0 || cells_y == 0 || cells_x > 256 || cells_y > 256 || cap == 0) return -2;
    const size_t cells = (size_t)cells_x * cells_y;
    if (cells * cap > (1u << 24)) return -2;
    // the cells tile the launch's rows and columns: no cell of the grid lies wholly beyond the frame
    const unsigned cw = ((1u << lw) << lnx) << gx, ch = ((256u >> lw) * (nsub >> lnx)) << gy;
    if ((size_t)(cells_x - 1u) * cw >= W || (size_t)row0 + (size_t)(cells_y - 1u) * ch >= H) return -2;
    Buffers b;
    KArgs a = args_of(cam, W, H);
    a.row0 = row0;
    a.ns = ns;
    a.tile_log2w = lw;
    a.nsub = nsub;
    a.sub_log2nx = lnx;
    a.cell_log2gx = gx;
    a.cell_log2gy = gy;
    a.cells_x = cells_x;
    a.cells_y = cells_y;
    a.cell_cap = cap;
    a.bin_theta = bin_theta;
    a.bin_delta = bin_delta;
    a.sph_scene_geom = (const float4*)b.up(spheres, (size_t)ns * 16);
    a.sph_pos_of = pos_of ? (const uint32_t*)b.up(pos_of, (size_t)ns * 4) : nullptr;
    a.cell_count_out = (uint32_t*)b.up(counts, (cells + guard) * 4);
    a.cell_list_out = (uint32_t*)b.up(lists, (cells * cap + guard) * 4);
    a.cell_count_zero = (uint32_t*)b.up(zeroed, (cells + guard) * 4);
    a.cell_max_out = (uint32_t*)b.up(cell_max, 4);
    if (!b.ok) return -1;
    const int rc = rtx::launch_bin_cells(&a, splits, 0);
    return rc == 0 && b.ran() && b.down(counts, a.cell_count_out, (cells + guard) * 4) && b.down(lists, a.cell_list_out, (cells * cap + guard) * 4) &&
                   b.down(zeroed, a.cell_count_zero, (cells + guard) * 4) && b.down(cell_max, a.cell_max_out, 4)
               ? 0
               : -1;
}

// rtxplan::xcd_cell_order (host): the static base order of a grid_x x grid_y tile grid with cells of 2^gx x 2^gy tiles; order_out: grid_x grid_y words.
RTX_CHECK_API int rtx_check_xcd_cell_order(unsigned grid_x, unsigned grid_y, unsigned gx, unsigned gy, uint32_t* order_out)
{
    if (!order_out || grid_x == 0 || grid_y == 0 || grid_x > 0xffffu || grid_y > 0xffffu || (uint64_t)grid_x * grid_y > (1u << 20) || gx > 8 || gy > 8) return -2;
    rtxplan::xcd_cell_order(grid_x, grid_y, gx, gy, order_out);
    return 0;
}
