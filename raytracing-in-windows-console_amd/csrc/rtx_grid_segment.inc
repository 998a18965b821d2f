// rtx_grid_segment.inc -- the shadow test of one segment through the world grid, included into namespace rtx after rtx_tile_pass.inc
// (segment_hits_sphere) by rtx_grid_shadow_kernels.inc, whose header states what it decides, and by the direct check of the grid's
// device code (tests/gpu_checks/grid_check.hip), which compiles the same text without the shade families.

// Is the open segment from P to L (toL = L - P) within r of the centre of a sphere other than the one of creation index own_gidx
// (own_pos: its position in a.sph_geom; 0xffffffff for both: none)?  `open`: the lanes that ask.  Adds the lanes that could not
// walk their segment to n_fallback.
__device__ __forceinline__ bool grid_segment_dark(const KArgs& a, const GridShadowArgs& gs, V3 P, V3 toL, uint32_t own_gidx, uint32_t own_pos, bool open,
                                                  uint32_t& n_fallback)
{
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
            if (pending && j != own_pos && segment_hits_sphere(P, toL, inv_len2, sp)) {
                hit = true;
                pending = false;
            }
        }
    }
    return hit;
}
