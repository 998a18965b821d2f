// rtx_grid_shadow_kernels.inc -- shadow tests through the world grid (RTX_OPT_SHADOW_GRID), included into namespace rtx of
// rtx_kernels.hip after rtx_tile_pass.inc, which holds every device function of the test, and after the lights' kernel files, whose
// lights_shade_body the shade family below instantiates.
//
// rtx_grid_shadow: two instantiations (SPOT, below), nothing shaded or encoded.  A 256-thread workgroup owns a 16 x 16 tile as the other tile
// passes do, so that neighbouring pixels walk neighbouring cells, but there is no list in LDS and no barrier: every pixel is on
// its own.  Each thread rebuilds its pixel exactly as lights_shade_body and rtx_chain_shadow do (tile_pixel, surface_of, the
// forward walk of the chain with reflectivity_of / secondary_ray: the same operations on the same bits, so P_j, n_j, o_j are theirs)
// and decides for level 0 -- and for the levels 1 .. depth when gs.deep is set (RTX_OPT_REFLECT_SHADOWS in effect) -- and every
// light of the set whether the point is dark: shadowed_before_spheres unchanged (the light's cone, self-shadow and planes), then segment_hits_sphere
// against the spheres of the grid's large list, then against the lists of the cells the segment's walk visits (rtx_grid.hpp:
// walk_start / walk_step with d = toL and tmax = 1), leaving at the first hit.  The test is the brute path's; only which spheres a
// segment is tested against changes, and rtx_grid.hpp (step 4) shows that no sphere the test would report is left out.  The lists
// know spheres by creation index, so the point's own sphere is excluded by creation_index(a, id).  A segment that cannot be
// walked (rtxgrid::segment_walkable: the point beyond `reach`, the light at the point itself, a length outside [2^-20, 2^20])
// tests every sphere of the scene array and is counted in gs.fallback (one atomicAdd per wave).
//
// Output: gs.dark0[pixel], bit i set iff light i is dark at level 0 (level 0 keeps its distance <= cam.far condition); cs.dark
// in rtx_chain_shadow's layout for the deeper levels (no far limit there), and cs.points counted as rtx_chain_shadow counts it.

#include "rtx_grid_segment.inc" // grid_segment_dark

// The lights (bit i) the point P -- normal `normal`, on object `id` -- is shadowed from: lights_dark_set's answer, per pixel.
// Called by every lane of the wave (shadowed_before_spheres and the loops above vote).
template <class LA>
__device__ __forceinline__ uint32_t grid_dark_set(const KArgs& a, const LA& la, const GridShadowArgs& gs, V3 P, V3 normal, uint32_t id, bool testable,
                                                  uint32_t& n_fallback)
{
    const bool on_plane = (id & 0x80000000u) != 0u;
    const uint32_t own_plane = on_plane ? (id & 0x7fffffffu) : 0xffffffffu;
    const uint32_t own_pos = on_plane ? 0xffffffffu : id;
    uint32_t own_gidx = 0xffffffffu;
    if (testable && !on_plane) own_gidx = creation_index(a, id);
    uint32_t dark = 0u;
    for (uint32_t i = 0; i < la.lights.n; i++) {
        const rtxlights::PackedLight& Lt = la.lights.light[i];
        const V3 L = v3(Lt.px, Lt.py, Lt.pz);
        const V3 toL = sub(L, P);
        bool pending = testable;
        if (shadowed_before_spheres(a, la, i, P, normal, L, toL, own_plane, pending)) dark |= 1u << i;
        if constexpr (std::is_same_v<LA, SpotLightsArgs>) { // (the rich form: the spheres that cast -- rtx_scene_set_shadow_casting)
            if (grid_segment_dark_casting<true>(a, gs, la.cast, P, toL, own_gidx, own_pos, pending, n_fallback)) dark |= 1u << i;
        } else {
            if (grid_segment_dark(a, gs, P, toL, own_gidx, own_pos, pending, n_fallback)) dark |= 1u << i;
        }
    }
    return dark;
}

// (launch bounds alone: 109 VGPRs, no scratch, 4 waves per SIMD -- the walk's three axes are 15 registers beside the loop-carried ray
// of the chain, the point, the segment and the level's word.  Asking for 5 waves brings 96 VGPRs and 48 bytes of scratch per lane,
// for 6 (rtx_chain_shadow's figure) 80 and 960: the walk spills.  No scratch was chosen over a fifth wave: the kernel has no LDS
// and no barrier, so its four waves per SIMD are sixteen independent workgroup quarters per CU, and a spilled walk state would be
// reloaded at every cell.  The kernel arguments -- KArgs, the light set by value, the grid -- do not fit the scalar registers:
// 323 SGPRs are parked in VGPR lanes, none in memory.  profiles/r12_shadow_grid_resource_usage.txt.)
#ifdef RTX_GRID_SHADOW_WAVES // (an experiment build may ask for a figure: make variant DEFS=-DRTX_GRID_SHADOW_WAVES=5)
#define RTX_GRID_SHADOW_BOUNDS __launch_bounds__(kThreads, RTX_GRID_SHADOW_WAVES)
#else
#define RTX_GRID_SHADOW_BOUNDS __launch_bounds__(kThreads)
#endif
// SPOT (rtx_scene_set_spots: the form launched while some light of the set has a cone, its arguments the set with the cones behind
// it): a point outside a light's cone is not pending for that light -- no plane test, no segment, walked or counted -- and not dark
// either: the shade launch weighs that light with 0 there.  The same launch bounds.  Without SPOT the code is what it was.
// The SPOT form also reads the shadow-casting flags (rtx_scene_set_shadow_casting: la.cast), so it is launched too while some object
// casts no shadow: a plane or a sphere whose flag is 0 is no occluder (shadowed_before_spheres, grid_segment_dark_casting).
template <bool SPOT>
__global__ RTX_GRID_SHADOW_BOUNDS void rtx_grid_shadow(const KArgs a, const LightsArgsOf<SPOT> la, const ReflectArgs ra, const ChainArgs ca, const ChainShadowArgs cs,
                                                            const GridShadowArgs gs)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));

    // level 0: the primary ray and its winner, as lights_shade_body has them
    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, la.hits, tid);
    const size_t at = px.in_frame ? px.at(a) : 0u;
    const bool any_hit = px.in_frame && !px.newline_col && px.hit.y != 0xffffffffu;
    Ray r = px.ray;
    float t = kNoHit;
    V3 n = r.d;
    uint32_t o = px.hit.y;
    if (any_hit) {
        t = __uint_as_float(px.hit.x);
        n = surface_of(a, o, add(r.o, mulf(r.d, t))).normal;
    }
    uint32_t n_fallback = 0u;
    {
        const V3 P = add(r.o, mulf(r.d, t)); // the point shade() lights
        const bool testable = la.test != 0u && any_hit && t <= cam.far;
        const uint32_t dark = grid_dark_set(a, la, gs, P, n, o, testable, n_fallback);
        if (px.in_frame) gs.dark0[at] = dark;
    }

    // the deeper levels: rtx_chain_shadow's walk of the chain
    const uint32_t levels = gs.deep != 0u ? ca.depth : 0u;
    if (levels != 0u) {
        bool alive = any_hit && t <= cam.far;
        uint32_t word = 0u;
        for (uint32_t j = 0; j < levels; j++) {
            if (alive) {
                alive = reflectivity_of(ra, o) > 0.0f;
                if (alive) {
                    r = secondary_ray(a, ra, r, t, n, o);
                    const uint2 h = ra.hits[(size_t)(j + 1u) * ca.px + at];
                    alive = h.y != 0xffffffffu;
                    if (alive) {
                        t = __uint_as_float(h.x);
                        o = h.y;
                        n = surface_of(a, o, add(r.o, mulf(r.d, t))).normal;
                    }
                }
            }
            const bool testable = la.test != 0u && alive;
            {
                const unsigned long long m = __ballot(testable);
                if (cs.points != nullptr && lane == 0u && m != 0ull) atomicAdd(&cs.points[j], (uint32_t)__popcll(m));
            }
            const V3 P = add(r.o, mulf(r.d, t));
            word |= grid_dark_set(a, la, gs, P, n, o, testable, n_fallback) << (8u * j);
        }
        if (px.in_frame) cs.dark[at] = word;
    }

    // the segments that tested every sphere: one atomic per wave
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) n_fallback += (uint32_t)__shfl_xor((int)n_fallback, k);
    if (lane == 0u && n_fallback != 0u) atomicAdd(gs.fallback, n_fallback);
}

// The shade family of the grid path: lights_shade_body with level 0's dark set read from gs.dark0 instead of computed -- no cone,
// no walk of the scene, no list in LDS -- for any set of 1 .. 8 lights.  REFLECT as there: 0 rtx_grid_shade, 1
// rtx_grid_reflect_shade (one bounce), 2 rtx_grid_chain_shade, 3 rtx_grid_chain_shadow_shade (the deeper levels' words).
template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_grid_shade(const KArgs a, const LightsArgsOf<FIN> la, const uint32_t* dark0, const PatternArgs pa)
{
    const ReflectArgs ra = {};
    const ChainArgs ca = {};
    lights_shade_body<MODE, OUT, 0, true, FIN>(a, la, ra, ca, pa, nullptr, dark0);
}

template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_grid_reflect_shade(const KArgs a, const LightsArgsOf<FIN> la, const ReflectArgs ra, const uint32_t* dark0, const PatternArgs pa)
{
    const ChainArgs ca = {};
    lights_shade_body<MODE, OUT, 1, true, FIN>(a, la, ra, ca, pa, nullptr, dark0);
}

template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_grid_chain_shade(const KArgs a, const LightsArgsOf<FIN> la, const ReflectArgs ra, const ChainArgs ca, const uint32_t* dark0,
                                                                 const PatternArgs pa)
{
    lights_shade_body<MODE, OUT, 2, true, FIN>(a, la, ra, ca, pa, nullptr, dark0);
}

template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_grid_chain_shadow_shade(const KArgs a, const LightsArgsOf<FIN> la, const ReflectArgs ra, const ChainArgs ca,
                                                                        const ChainShadowArgs cs, const uint32_t* dark0, const PatternArgs pa)
{
    lights_shade_body<MODE, OUT, 3, true, FIN>(a, la, ra, ca, pa, cs.dark, dark0);
}
