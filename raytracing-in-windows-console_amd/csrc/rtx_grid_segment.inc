// rtx_grid_segment.inc -- the shadow test of one segment through the world grid, included into namespace rtx after rtx_tile_pass.inc
// (segment_hits_sphere) by rtx_grid_shadow_kernels.inc, whose header states what it decides, and by the direct check of the grid's
// device code (tests/gpu_checks/grid_check.hip), which compiles the same text without the shade families.

// Is the open segment from P to L (toL = L - P) within r of the centre of a sphere other than the one of creation index own_gidx
// (own_pos: its position in a.sph_geom; 0xffffffff for both: none)?  `open`: the lanes that ask.  Adds the lanes that could not
// walk their segment to n_fallback.
//
// CAST (the rich form of rtx_grid_shadow, rtx_scene_set_shadow_casting): a sphere whose flag is 0 is no occluder.  The large list and
// the cell lists know spheres by creation index (cast.gidx), the loop over the scene array by position (cast.sph); all nullptr (kernel
// arguments: the test is uniform) while every object casts.  Which cells are walked and which segments fall back does not depend on
// the flags.  Without CAST nothing of this is compiled.
template <bool CAST>
__device__ __forceinline__ bool grid_segment_dark_casting(const KArgs& a, const GridShadowArgs& gs, const CastArgs& cast, V3 P, V3 toL, uint32_t own_gidx,
                                                          uint32_t own_pos, bool open, uint32_t& n_fallback)
{
    bool flags = false; // (CAST) are there flags to read?
    if constexpr (CAST) flags = cast.gidx != nullptr;
    const float len2 = dot(toL, toL);
    const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f; // (as lights_dark_set forms it)
    const float Pf[3] = {P.x, P.y, P.z}, Df[3] = {toL.x, toL.y, toL.z};
    const bool walk = rtxgrid::segment_walkable(gs.grid, Pf, Df);
    bool hit = false;
    bool go = open && walk;
    // the large list: wave-uniform index (scalar loads)
    if (__ballot(go) != 0ull) {
        for (uint32_t j = 0; j < gs.n_large; j++) {
            const uint32_t i = gs.large[j];
            const float4 sp = gs.scene_geom[i];
            const uint32_t gidx = __float_as_uint(gs.scene_od[i].w);
            if constexpr (CAST) {
                if (flags && cast.gidx[gidx] == 0u) continue; // (uniform)
            }
            if (go && gidx != own_gidx && segment_hits_sphere(P, toL, inv_len2, sp)) {
                hit = true;
                go = false;
            }
        }
    }
    // the walk
    if (go) {
        rtxgrid::Walk w;
        go = rtxgrid::walk_start(gs.grid, Pf, Df, 1.0f, w);
        while (go) {
            const uint32_t c = rtxgrid::cell_index(gs.grid, w);
            const uint32_t b = gs.cell_start[c], e = gs.cell_start[c + 1u];
            for (uint32_t j = b; j < e; j++) {
                if (segment_hits_sphere(P, toL, inv_len2, gs.list_geom[j]) && gs.list_gidx[j] != own_gidx) {
                    if constexpr (CAST) {
                        if (flags && cast.gidx[gs.list_gidx[j]] == 0u) continue; // (met, but no occluder)
                    }
                    hit = true;
                    break;
                }
            }
            go = !hit && rtxgrid::t_out(w) <= 1.0f && rtxgrid::walk_step(gs.grid, w);
        }
    }
    // not walkable: every sphere of the scene array, by position (wave-uniform index)
    const bool fb = open && !walk;
    if (fb) n_fallback++;
    if (__ballot(fb) != 0ull) {
        bool pending = fb;
        for (uint32_t j = 0; j < a.ns && __ballot(pending) != 0ull; j++) {
            const float4 sp = a.sph_geom[j];
            if constexpr (CAST) {
                if (flags && cast.sph[j] == 0u) continue; // (uniform)
            }
            if (pending && j != own_pos && segment_hits_sphere(P, toL, inv_len2, sp)) {
                hit = true;
                pending = false;
            }
        }
    }
    return hit;
}

__device__ __forceinline__ bool grid_segment_dark(const KArgs& a, const GridShadowArgs& gs, V3 P, V3 toL, uint32_t own_gidx, uint32_t own_pos, bool open,
                                                  uint32_t& n_fallback)
{
    const CastArgs none = {nullptr, nullptr, nullptr};
    return grid_segment_dark_casting<false>(a, gs, none, P, toL, own_gidx, own_pos, open, n_fallback);
}
