// rollcall_plan.cpp -- what rtxplan::plan_tiles and rtxplan::plan_cells make of a frame and an explicit option set, printed as
// one line of numbers: tests/test_host_rollcall.py proves the tile shapes and cell grids that tests/rollcall_cases.py writes
// down as literals against it.  Host-only C++ (csrc/rtx_plan.hpp has no HIP in it), built under
// -fsanitize=address,undefined like tests/host/test_plan.cpp.
//
// usage: rollcall_plan W H rows ns e1 e2 subtiles tile_log2w refine cell_capacity m0 .. m15
// prints: lw lnx nsub mw mh grid_x grid_y refine gx gy cells_x cells_y cell_w cell_h cap
#include <cstdio>
#include <cstdlib>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

int main(int argc, char** argv)
{
    if (argc != 11 + 16) {
        std::fprintf(stderr, "rollcall_plan: expected 26 arguments, got %d\n", argc - 1);
        return 2;
    }
    const uint64_t W = std::strtoull(argv[1], nullptr, 10), H = std::strtoull(argv[2], nullptr, 10), rows = std::strtoull(argv[3], nullptr, 10);
    const uint32_t ns = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const float e1 = std::strtof(argv[5], nullptr), e2 = std::strtof(argv[6], nullptr);
    float m[16];
    for (int i = 0; i < 16; i++) m[i] = std::strtof(argv[11 + i], nullptr);
    double sx, sy;
    rtxplan::pixel_steps(m, e1, e2, W, H, &sx, &sy); // rtx_render.cpp: pixel_aspect
    rtxplan::TileRequest q;                          // rtx_render.cpp: tile_request, for the culling kernels
    q.W = W;
    q.H = H;
    q.rows = rows;
    q.ns = ns;
    q.aspect = sx / sy;
    q.n_cu = 256;
    q.cull = true;
    q.opt_subtiles = std::atoi(argv[7]);
    q.opt_tile_log2w = std::atoi(argv[8]);
    q.opt_refine = std::atoi(argv[9]);
    const rtxplan::TileShape t = rtxplan::plan_tiles(q);
    const rtxplan::CellGrid c = rtxplan::plan_cells(t, ns, q.aspect, std::atoll(argv[10]), 0);
    std::printf("%u %u %u %u %u %u %u %d %u %u %u %u %u %u %u\n", t.lw, t.lnx, t.nsub, t.mw, t.mh, t.grid_x, t.grid_y, t.refine ? 1 : 0, c.gx, c.gy, c.cells_x,
                c.cells_y, c.cell_w, c.cell_h, c.cap);
    return 0;
}
