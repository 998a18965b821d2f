// rtx_reflect_kernels.inc -- the mirror path's second launch at depth 1 (rtx_scene_set_reflectivity), included into namespace rtx
// of rtx_kernels.hip after rtx_tile_pass.inc, which holds every device function it calls.  Three launches: the trace kernel in its
// kOutHit form (every pixel's closest hit), rtx_reflect_hit (the closest hit of each reflective pixel's secondary ray) and
// rtx_reflect_shade (rtx_shadow_kernels.inc: the shading, then the blend).
//
// A pixel reflects when it is visible (t <= cam_far, not column W-1) and its winner o has k > 0.  Its secondary ray (secondary_ray) is
// tested against every sphere and plane but o; the winner is the lexicographic minimum of (t, creation index).
//
// rtx_reflect_hit: every thread of a tile rebuilds its primary and forms its secondary ray; the planes are tested per pixel
// (closest_of_planes).  The waves reduce the tile's secondary rays to up to four bundles (build_bundles), the scene is walked and
// the spheres that may meet a bundle are listed (walk_spheres), and at every flush each wave with a pending pixel runs the exact
// closest-hit test over the list (closest_of_list).  The culled result equals the brute one.  Tiles with no reflective pixel skip
// the walk.

__global__ __launch_bounds__(kThreads) void rtx_reflect_hit(const KArgs a, const ReflectArgs ra)
{
    __shared__ float4 s_cand[kTileList];
    __shared__ uint32_t s_cand_pos[kTileList];
    __shared__ float s_red[4][8];
    __shared__ rtxreflect::Bundle s_bundle[kReflectBundles];
    __shared__ float s_lead_u[4][3];
    __shared__ uint32_t s_lead_lane[4];
    __shared__ uint32_t s_cnt;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    if (tid == 0u) s_cnt = 0u; // (visible behind build_bundles' first barrier)

    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, ra.hits, tid);
    const Ray& ray = px.ray;
    const uint32_t id = px.hit.y;
    const float distance = __uint_as_float(px.hit.x);
    bool pending = px.in_frame && !px.newline_col && id != 0xffffffffu && distance <= cam.far;
    if (pending) pending = reflectivity_of(ra, id) > 0.0f;
    V3 normal = ray.d;
    if (pending) normal = surface_of(a, id, add(ray.o, mulf(ray.d, distance))).normal;
    const Ray r2 = secondary_ray(a, ra, ray, pending ? distance : 0.0f, normal, id);
    float bt = kNoHit;
    uint32_t bid = 0xffffffffu;
    closest_of_planes(a, r2, pending, id, bt, bid);

    // spheres: the walk against the tile's bundles, unless every sphere is tested
    const uint32_t nb = build_bundles(r2, pending, ra.brute != 0u, tid, lane, wave, s_red, s_bundle, s_lead_u, s_lead_lane);
    if (nb != 0u && a.ns != 0u) {
        const bool wave_open = __ballot(pending) != 0ull;
        walk_spheres<kTileList>(a, tid, lane, s_cand, s_cand_pos, nullptr, &s_cnt, ra.longest, MayMeetBundles{s_bundle, nb}, [&](uint32_t cnt) {
            if (wave_open) closest_of_list(a, r2, pending, id, s_cand, s_cand_pos, cnt, bt, bid);
        });
    }

    if (pending) ra.hits2[px.at(a)] = make_uint2(__float_as_uint(bt), bid);
}
