// rtx_chain_shadow_kernels.inc -- shadows seen in mirrors (RTX_OPT_REFLECT_SHADOWS): the launch between rtx_reflect_chain and the
// chain's shade launch, included into namespace rtx of rtx_kernels.hip after rtx_tile_pass.inc, which holds every device function
// it calls.  Two instantiations (SPOT, below): nothing is shaded or encoded here.
//
// Level j (1 .. depth) of a pixel's chain that hit an object o_j has the hit point P_j = r_j.o + r_j.d * t_j (as shade_lights
// forms `point`) and the normal n_j = surface_of(o_j, P_j).  Every thread walks its pixel's chain forward from the hits
// rtx_reflect_chain stored (level j at ra.hits + j * ca.px) exactly as lights_chain_blend does -- reflectivity_of, secondary_ray,
// surface_of, the same operations on the same bits, so P_j and n_j are the shade launch's -- and per level the workgroup runs
// level 0's shadow test (lights_dark_set: per light self-shadow, planes and the cone over the tile's pending level-j points, one
// walk of the scene for all lights with 8-bit light masks, segment tests at each flush) with P_j, n_j, o_j and no far limit.  The
// level loop runs ca.depth times for every thread, so all waves meet the same barriers; a level with no pending pixel in the tile
// has no live cone and no walk.  No step depends on the order of the LDS list: culled equals brute (RTX_OPT_SHADOW_CHECK 1).
//
// Output: one word per pixel of the launch at cs.dark, laid out as the hits: bit 8 (j - 1) + i set iff light i is dark at level
// j (4 levels x 8 lights).  Every pixel of the frame is written; a level that does not exist or hit nothing leaves its byte 0.
// cs.points[j - 1] += the level-j points the workgroup tested (one atomicAdd per workgroup and level; none under
// RTX_OPT_SHADOW_CHECK 2, which tests nothing).

struct ChainShadowShared {
    float4 occ[kTileList];
    uint32_t occ_pos[kTileList];
    uint32_t occ_mask[kTileList / 4]; // one byte per entry: the lights the sphere was kept for
    float red[4][6];
    rtxshadow::Cone cone[rtxlights::kMaxLights];
    uint32_t cnt;
    uint32_t points[kMaxReflectDepth]; // tested points of the workgroup, per level
};

// (6 waves per SIMD asked for, as rtx_reflect_chain does: without the hint the loop-carried ray costs 85 VGPRs and a whole wave -- 5;
// 79 VGPRs with it, no scratch, and frames 0.8-1.2 % shorter on C2 floor + quarter and the C3 room, EXPERIMENTS.md Round 11.
// 21.9 KB of LDS would allow 7.)
#ifndef RTX_CHAIN_SHADOW_WAVES
#define RTX_CHAIN_SHADOW_WAVES 6 // (an experiment build may ask for another figure: make variant DEFS=-DRTX_CHAIN_SHADOW_WAVES=1)
#endif
// SPOT (rtx_scene_set_spots: the form launched while some light of the set has a cone, its arguments the set with the cones behind
// it): a level's point outside a light's cone is not pending for that light (lights_dark_set) -- it adds nothing to the light's tile
// cone and tests no segment.  Without SPOT the code is what it was.  The SPOT form also reads the shadow-casting flags
// (rtx_scene_set_shadow_casting: la.cast, in lights_dark_set), so it is launched too while some object casts no shadow.
template <bool SPOT>
__global__ __launch_bounds__(kThreads, RTX_CHAIN_SHADOW_WAVES) void rtx_chain_shadow(const KArgs a, const LightsArgsOf<SPOT> la, const ReflectArgs ra, const ChainArgs ca,
                                                                                     const ChainShadowArgs cs)
{
    __shared__ ChainShadowShared s;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    if (tid == 0u) s.cnt = 0u;
    if (tid < (uint32_t)kMaxReflectDepth) s.points[tid] = 0u;
    lds_barrier(); // the counters are zero before any wave adds to them

    // level 0: the primary ray and its winner, as lights_shade_body has them when it calls the blend
    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, ra.hits, tid);
    const size_t at = px.in_frame ? px.at(a) : 0u;
    bool alive = px.in_frame && !px.newline_col && px.hit.y != 0xffffffffu && __uint_as_float(px.hit.x) <= cam.far; // level j hit an object
    Ray r = px.ray;
    float t = 0.0f;
    V3 n = r.d;
    uint32_t o = px.hit.y;
    if (alive) {
        t = __uint_as_float(px.hit.x);
        n = surface_of(a, o, add(r.o, mulf(r.d, t))).normal;
    }

    uint32_t word = 0u;
    for (uint32_t j = 0; j < ca.depth; j++) { // (workgroup-uniform trip count: every wave meets lights_dark_set's barriers)
        // level j + 1 of this pixel: lights_chain_blend's step
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
            if (lane == 0u && m != 0ull) atomicAdd(&s.points[j], (uint32_t)__popcll(m));
        }
        const V3 P = add(r.o, mulf(r.d, t)); // the point shade_lights lights at this level
        const uint32_t dark = lights_dark_set(a, la, s, tid, lane, wave, P, n, o, testable);
        word |= dark << (8u * j);
        // (every wave's count of this level was added before lights_dark_set's barriers, of which there is at least one)
        if (cs.points != nullptr && tid == 0u && s.points[j] != 0u) atomicAdd(&cs.points[j], s.points[j]);
    }
    if (px.in_frame) cs.dark[at] = word;
}
