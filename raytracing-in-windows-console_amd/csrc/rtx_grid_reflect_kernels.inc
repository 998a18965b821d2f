// rtx_grid_reflect_kernels.inc -- the mirror path's secondary hits through the world grid (RTX_OPT_REFLECT_GRID), included into
// namespace rtx of rtx_kernels.hip after rtx_tile_pass.inc, which holds every device function of the test.
//
// rtx_grid_reflect: one instantiation, in place of rtx_reflect_hit and rtx_reflect_chain.  A 256-thread workgroup owns a 16 x 16
// tile as the other tile passes do, so that neighbouring pixels walk neighbouring cells, but there is no list in LDS and no
// barrier: every pixel is on its own.  Level 0 is set up exactly as rtx_reflect_chain does it (tile_pixel, the chain condition,
// reflectivity_of, surface_of, secondary_ray: the same operations on the same bits), then the level loop runs with the ray, the
// object left and the pending flag in registers.  A level is closest_of_planes unchanged, then secondary_sphere_hit against the
// spheres of the grid's large list, then against the lists of the cells the ray's walk visits (rtx_grid.hpp: walk_start /
// walk_step with tmax = infinity), stopping when the best t is below t_out of the cell just tested or the ray leaves the grid,
// exactly as rtx_query_grid does.  The test is the brute path's; only which spheres a ray is tested against changes, and
// rtx_grid.hpp (steps 1-3, step 5) shows that no sphere the test would report is left out: a minimum does not depend on the order
// or the number of times its candidates are met, so the winners are rtx_reflect_chain's.
//
// Indexing.  The hit buffer and the shade kernels know a sphere by its position in a.sph_geom (direction-sorted from 256 spheres
// on), the grid's lists by creation index, the large list by sphere index.  The best so far is therefore kept as (t, creation
// index) -- a plane winner's creation index beside its position form 0x80000000 | q, so that a tie between a plane and a sphere
// falls as comes_before lets it fall -- the object a ray leaves is excluded by creation_index(a, id), a candidate's creation
// index is fetched only when it can take the lead, and the winner becomes a position once per level through gr.pos_of_gidx.
//
// A ray that cannot be walked (rtxgrid::walkable: its origin beyond `reach`, an origin or direction that is not finite, a outside
// [2^-40, 2^40]) tests every sphere of a.sph_geom by position, per lane with a wave-uniform index (scalar loads), as
// grid_segment_dark does, and is counted in gr.fallback (one atomicAdd per wave).  Staging through LDS as rtx_query_grid does
// would need workgroup-uniform control flow and two barriers per 512 spheres inside the level loop, which every wave of the tile
// would have to meet whether or not it has such a ray; here a wave without one skips the loop altogether.
//
// Output: rtx_reflect_chain's contract.  A chain pixel gets an entry at every level 1 .. ca.depth (the no-hit pair where the
// chain did not reach), other pixels are never written; with depth 1 and a two-level buffer that is rtx_reflect_hit's.  ca.rays
// gets the rays per level (one atomicAdd per wave and level: the totals are rtx_reflect_chain's).

// (launch bounds alone: 91 VGPRs, no scratch, no LDS, 5 waves per SIMD -- the walk's three axes are 15 registers beside the
// loop-carried ray, the best so far and the pixel.  Asking for 6 waves brings 80 VGPRs and 32 bytes of scratch per lane, for 8 it is
// 64 and 112: the walk spills.  No scratch was chosen over a sixth wave: the kernel has no barrier, so its five waves per SIMD are
// twenty independent workgroup quarters per CU, and a spilled walk state would be reloaded at every cell.  The kernel arguments --
// KArgs, the grid by value -- do not fit the scalar registers: 133 SGPRs are parked in VGPR lanes, none in memory.
// profiles/r27_reflect_grid_resource_usage.txt.)
#ifdef RTX_GRID_REFLECT_WAVES // (an experiment build may ask for a figure: make variant DEFS=-DRTX_GRID_REFLECT_WAVES=5)
#define RTX_GRID_REFLECT_BOUNDS __launch_bounds__(kThreads, RTX_GRID_REFLECT_WAVES)
#else
#define RTX_GRID_REFLECT_BOUNDS __launch_bounds__(kThreads)
#endif
// GLASS: some object is refractive (ra.ior_sph is not null).  The kernel tests that once, outside the level loop, and runs one of two
// copies of the body: without glass the parent's instructions, with the rays formed by mirror_ray alone (measured: with the test
// inside the loop the frames without a refractive object were 4-5 % longer, profiles/r33_glass_cost.txt).
template <bool GLASS>
__device__ __forceinline__ void grid_reflect_body(const KArgs& a, const ReflectArgs& ra, const ChainArgs& ca, const GridReflectArgs& gr)
{
    constexpr uint32_t kNone = 0xffffffffu;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));

    // level 0: the primary ray, its winner's normal and the reflectivity
    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, ra.hits, tid);
    const Ray& ray = px.ray;
    const uint2 hit = px.hit;
    const size_t at = px.in_frame ? px.at(a) : 0u;
    bool pending = px.in_frame && !px.newline_col && hit.y != kNone && __uint_as_float(hit.x) <= cam.far;
    if (pending) pending = reflectivity_of(ra, hit.y) > 0.0f;
    const bool chain = pending; // the pixel has a chain: every level up to the depth gets an entry
    V3 normal = ray.d;
    if (pending) normal = surface_of(a, hit.y, add(ray.o, mulf(ray.d, __uint_as_float(hit.x)))).normal;
    Ray cur = secondary_ray<GLASS>(a, ra, ray, pending ? __uint_as_float(hit.x) : 0.0f, normal, hit.y); // the ray of the level being traced
    uint32_t id = hit.y;                                                          // the object it leaves, by position ...
    uint32_t own = kNone;                                                         // ... and by creation index
    if (pending) own = creation_index(a, id);

    uint32_t n_fallback = 0u;
    uint32_t level = 1u;
    for (; level <= ca.depth; level++) {
        uint2* const out = ra.hits2 + (size_t)(level - 1u) * ca.px;
        const unsigned long long open = __ballot(pending);
        if (open == 0ull) break; // nothing of the wave goes this deep
        if (ca.rays != nullptr && lane == 0u) atomicAdd(&ca.rays[level - 1u], (uint32_t)__popcll(open));

        // the planes: (bt, bid) with bid = 0x80000000 | q or none; bg: the winner's creation index (none: 0xffffffff, past every index)
        float bt = kNoHit;
        uint32_t bid = kNone;
        closest_of_planes(a, cur, pending, id, bt, bid);
        uint32_t bg = kNone;
        if (bid != kNone) bg = creation_index(a, bid);

        const float o[3] = {cur.o.x, cur.o.y, cur.o.z}, d[3] = {cur.d.x, cur.d.y, cur.d.z};
        const bool walk = rtxgrid::walkable(gr.grid, o, cur.a);
        // a sphere candidate takes the lead when comes_before says so: t < bt, or t == bt and the lower creation index
        // (bid: a sphere's bit 31 is clear; its position is looked up after the level)
        if (pending && walk) {
            // the large list, by sphere index (wave-uniform index: scalar loads)
            for (uint32_t j = 0; j < gr.n_large; j++) {
                const uint32_t i = gr.large[j];
                float t;
                if (secondary_sphere_hit(cur, gr.scene_geom[i], t) && t <= bt) {
                    const uint32_t g = __float_as_uint(gr.scene_od[i].w);
                    if (g != own && (t < bt || g < bg)) {
                        bt = t;
                        bg = g;
                        bid = 0u;
                    }
                }
            }
            // the walk
            rtxgrid::Walk w;
            bool go = rtxgrid::walk_start(gr.grid, o, d, INFINITY, w);
            while (go) {
                const uint32_t c = rtxgrid::cell_index(gr.grid, w);
                const uint32_t b = gr.cell_start[c], e = gr.cell_start[c + 1u];
                for (uint32_t j = b; j < e; j++) {
                    float t;
                    // (the creation index is fetched only for a candidate that can take the lead)
                    if (secondary_sphere_hit(cur, gr.list_geom[j], t) && t <= bt) {
                        const uint32_t g = gr.list_gidx[j];
                        if (g != own && (t < bt || g < bg)) {
                            bt = t;
                            bg = g;
                            bid = 0u;
                        }
                    }
                }
                go = !(bt < rtxgrid::t_out(w)) && rtxgrid::walk_step(gr.grid, w);
            }
        }
        // not walkable: every sphere of the scene, by position (wave-uniform index)
        const bool fb = pending && !walk;
        if (fb) n_fallback++;
        if (__ballot(fb) != 0ull) {
            for (uint32_t j = 0; j < a.ns; j++) {
                const float4 sp = a.sph_geom[j];
                float t;
                if (fb && j != id && secondary_sphere_hit(cur, sp, t) && t <= bt) {
                    const uint32_t g = __float_as_uint(a.sph_od[j].w);
                    if (t < bt || g < bg) {
                        bt = t;
                        bg = g;
                        bid = 0u;
                    }
                }
            }
        }
        // the winner by position: a plane has it already
        if (pending && bg != kNone && (bid & 0x80000000u) == 0u) bid = gr.pos_of_gidx[bg];

        if (pending) {
            out[at] = make_uint2(__float_as_uint(bt), bid);
        } else if (chain) {
            out[at] = make_uint2(__float_as_uint(kNoHit), kNone); // the chain ended above this level
        }

        // the next level's ray, for the lanes whose winner reflects
        bool next = pending && level < ca.depth && bid != kNone;
        if (next) next = reflectivity_of(ra, bid) > 0.0f;
        if (__ballot(next) != 0ull) {
            V3 n = cur.d;
            if (next) n = surface_of(a, bid, add(cur.o, mulf(cur.d, bt))).normal;
            cur = secondary_ray<GLASS>(a, ra, cur, next ? bt : 0.0f, n, bid);
        }
        id = bid;
        own = bg;
        pending = next;
    }

    // levels the wave did not reach
    if (chain) {
        for (; level <= ca.depth; level++) ra.hits2[(size_t)(level - 1u) * ca.px + at] = make_uint2(__float_as_uint(kNoHit), kNone);
    }

    // the rays that tested every sphere: one atomic per wave
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) n_fallback += (uint32_t)__shfl_xor((int)n_fallback, k);
    if (lane == 0u && n_fallback != 0u) atomicAdd(gr.fallback, n_fallback);
}

__global__ RTX_GRID_REFLECT_BOUNDS void rtx_grid_reflect(const KArgs a, const ReflectArgs ra, const ChainArgs ca, const GridReflectArgs gr)
{
    if (ra.ior_sph != nullptr) { // (a kernel argument: uniform)
        grid_reflect_body<true>(a, ra, ca, gr);
    } else {
        grid_reflect_body<false>(a, ra, ca, gr);
    }
}
