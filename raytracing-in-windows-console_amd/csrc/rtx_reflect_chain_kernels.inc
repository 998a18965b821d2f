// rtx_reflect_chain_kernels.inc -- the mirror path's second launch when mirrors see mirrors (RTX_OPT_REFLECT_DEPTH > 1, or
// RTX_OPT_REFLECT_DEPTH_CHECK 1), included into namespace rtx of rtx_kernels.hip after rtx_tile_pass.inc, which holds every device
// function it calls.  rtx_reflect_hit (rtx_reflect_kernels.inc) stays the depth-1 launch.
//
// Level 0 is the primary ray and its hit.  Level j + 1 exists for a pixel iff j + 1 <= depth, level j hit an object o_j and
// k(o_j) > 0; its ray is secondary_ray(r_j, t_j, normal_j, o_j) -- the mirror's, or the glass's -- with normal_j = surface_of(o_j) at the hit (sphere:
// normalize_gpu(normalize_gpu(P - C)), plane: normalize_gpu(n)), tested against every object but o_j with the reference's tests and
// no far limit, winner the lexicographic minimum of (t, creation index).  Level j's hits go to ra.hits + j * ca.px.
//
// rtx_reflect_chain: ONE launch for all levels -- a level is the planes per pixel (closest_of_planes), the tile's bundles
// (build_bundles) and the walk with its exact test (walk_spheres, closest_of_list), wrapped in a level loop.  Every thread keeps
// its current ray, the object it left and whether it is still pending in registers; after a level's store the lanes whose winner
// reflects form the next ray.  The trip count is workgroup-uniform: at the head of a level every wave adds its pending lanes to an
// LDS counter of that level, which is read behind build_bundles' first barrier (always met), so all waves see the same count and
// meet the same barriers; a tile with no pending lane leaves the loop.  A chain pixel's levels that were not traced get the no-hit
// pair; pixels without a chain are never written (nor read past level 0).  No step depends on the order of the LDS list, so culled
// equals brute (RTX_OPT_REFLECT_CHECK 1) at every level.

// (6 waves per SIMD asked for: without the hint the loop-carried ray costs an 81st VGPR and a whole wave -- 5; 80 VGPRs with it, no
// scratch.  7, rtx_reflect_hit's and what 20.8 KB of LDS allow, spills 10 VGPRs to scratch and is not taken.)
__global__ __launch_bounds__(kThreads, 6) void rtx_reflect_chain(const KArgs a, const ReflectArgs ra, const ChainArgs ca)
{
    __shared__ float4 s_cand[kTileList];
    __shared__ uint32_t s_cand_pos[kTileList];
    __shared__ float s_red[4][8];
    __shared__ rtxreflect::Bundle s_bundle[kReflectBundles];
    __shared__ float s_lead_u[4][3];
    __shared__ uint32_t s_lead_lane[4];
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_pend[kMaxReflectDepth]; // pending rays of the workgroup, per level

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    if (tid == 0u) s_cnt = 0u;
    if (tid < (uint32_t)kMaxReflectDepth) s_pend[tid] = 0u;
    lds_barrier(); // the counters are zero before any wave adds to them

    // level 0: the primary ray, its winner's normal and the reflectivity
    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, ra.hits, tid);
    const Ray& ray = px.ray;
    const uint2 hit = px.hit;
    const size_t at = px.in_frame ? px.at(a) : 0u;
    bool pending = px.in_frame && !px.newline_col && hit.y != 0xffffffffu && __uint_as_float(hit.x) <= cam.far;
    if (pending) pending = reflectivity_of(ra, hit.y) > 0.0f;
    const bool chain = pending; // the pixel has a chain: every level up to the depth gets an entry
    V3 normal = ray.d;
    if (pending) normal = surface_of(a, hit.y, add(ray.o, mulf(ray.d, __uint_as_float(hit.x)))).normal;
    Ray cur = secondary_ray(a, ra, ray, pending ? __uint_as_float(hit.x) : 0.0f, normal, hit.y); // the ray of the level being traced
    uint32_t id = hit.y;                                                          // the object it leaves

    const uint32_t ns = a.ns;
    uint32_t level = 1u;
    for (; level <= ca.depth; level++) {
        uint2* const out = ra.hits2 + (size_t)(level - 1u) * ca.px;
        {
            const unsigned long long m = __ballot(pending);
            if (lane == 0u && m != 0ull) atomicAdd(&s_pend[level - 1u], (uint32_t)__popcll(m));
        }
        float bt = kNoHit;
        uint32_t bid = 0xffffffffu;
        closest_of_planes(a, cur, pending, id, bt, bid);

        // spheres: the tile's pending rays of this level grouped into bundles
        const uint32_t nb = build_bundles(cur, pending, ra.brute != 0u, tid, lane, wave, s_red, s_bundle, s_lead_u, s_lead_lane);

        // every wave's count of this level was added before build_bundles' first barrier: the same number for all waves
        const uint32_t n_pending = __builtin_amdgcn_readfirstlane(s_pend[level - 1u]);
        if (n_pending == 0u) break; // nothing of the tile goes this deep (uniform)
        if (ca.rays != nullptr && tid == 0u) atomicAdd(&ca.rays[level - 1u], n_pending);

        if (nb != 0u && ns != 0u) {
            const bool wave_open = __ballot(pending) != 0ull;
            // (ra.longest: the maximum over the levels of what the workgroup listed at a level)
            walk_spheres<kTileList>(a, tid, lane, s_cand, s_cand_pos, nullptr, &s_cnt, ra.longest, MayMeetBundles{s_bundle, nb}, [&](uint32_t cnt) {
                if (wave_open) closest_of_list(a, cur, pending, id, s_cand, s_cand_pos, cnt, bt, bid);
            });
        }

        if (pending) {
            out[at] = make_uint2(__float_as_uint(bt), bid);
        } else if (chain) {
            out[at] = make_uint2(__float_as_uint(kNoHit), 0xffffffffu); // the chain ended above this level
        }

        // the next level's ray, for the lanes whose winner reflects
        bool next = pending && level < ca.depth && bid != 0xffffffffu;
        if (next) next = reflectivity_of(ra, bid) > 0.0f;
        if (__ballot(next) != 0ull) {
            V3 n = cur.d;
            if (next) n = surface_of(a, bid, add(cur.o, mulf(cur.d, bt))).normal;
            cur = secondary_ray(a, ra, cur, next ? bt : 0.0f, n, bid);
        }
        id = bid;
        pending = next;
        lds_barrier(); // every read of this level's LDS (s_lead_*, s_red, s_bundle) is done before the next level writes it
    }

    // levels the tile did not reach
    if (chain) {
        for (; level <= ca.depth; level++) ra.hits2[(size_t)(level - 1u) * ca.px + at] = make_uint2(__float_as_uint(kNoHit), 0xffffffffu);
    }
}
