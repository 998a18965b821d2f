// rtx_shadow_kernels.inc -- the shading launch for one light (RTX_OPT_SHADOWS, rtx_scene_set_light), included into namespace rtx
// of rtx_kernels.hip after rtx_tile_pass.inc, which holds the device functions the tile passes share.  The first launch is the
// trace kernel in its kOutHit form: the closest hit of every pixel, 8 bytes (t, object).  This one shades from it.
//
// Every thread of a tile rebuilds its pixel's ray, the hit point and the normal exactly as the trace body does (tile_pixel,
// surface_of), so that with no pixel in shadow the records are the one-pass kernels' bit for bit.  The shadow test of a visible
// pixel (P, N) against the light L: self-shadow when N . (L - P) <= 0; else the open segment (P, L) against every plane (crossing
// inside the plane's x/z bounds; shadowed_before_spheres) and every sphere (segment_hits_sphere), the hit object excluded.  Spheres
// are culled per workgroup first: the waves reduce their unresolved hit points to a cone from the light (light_cone), kept in
// registers, and the spheres that may touch it are listed (walk_spheres).  At every flush each wave runs its unresolved pixels
// over the list and leaves the loop as soon as none is left.  A shadowed pixel is shaded with both powers at 0; everything is
// encoded by encode_and_store.

// With REFLECT (the mirror path's third launch) each reflective pixel's secondary hit (ra.hits2) is shaded and blended into the
// colour before it is encoded (reflect_blend); without, nothing of it is compiled.
// FIN (rtx_scene_set_finish: the forms launched while some object has a finish of its own): every shade_light takes the finish of
// the object it shades; without, nothing of it is compiled and the code is what it was before there were finishes.
// The FIN forms also read the light's cone (rtx_scene_set_spots: sa is a SpotShadowArgs) and the shadow-casting flags
// (rtx_scene_set_shadow_casting: sa.cast): they are launched while some object has a finish, the light a cone, or some object casts
// no shadow while the shadow test runs.
template <bool FIN>
__device__ __forceinline__ V3 shade_light_of(const PatternArgs& pa, uint32_t id, const Ray& r, float distance, V3 normal, V3 od, const ShadowArgsOf<FIN>& sa, float dpow,
                                             float spow)
{
    if constexpr (FIN) {
        return shade_light(r, distance, normal, od, sa.light, dpow, spow, finish_of(pa, id), sa.spot);
    } else {
        return shade_light(r, distance, normal, od, sa.light, dpow, spow);
    }
}

template <int MODE, int OUT, bool REFLECT, bool FIN>
__device__ __forceinline__ void shade_body(const KArgs& a, const ShadowArgsOf<FIN>& sa, const ReflectArgs& ra, const PatternArgs& pa)
{
    __shared__ float4 s_occ[kTileList];
    __shared__ uint32_t s_occ_pos[kTileList];
    __shared__ uint32_t s_digits[256];
    __shared__ __attribute__((aligned(4))) uint8_t s_ramp[68];
    __shared__ float s_red[4][6];
    __shared__ uint32_t s_cnt;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    s_digits[tid] = digits_word(tid);
    if (tid < 17u) {
        reinterpret_cast<uint32_t*>(s_ramp)[tid] = reinterpret_cast<const uint32_t*>(kRamp)[tid];
    }
    if (tid == 0u) s_cnt = 0u; // (these three: visible behind light_cone's first barrier)

    const Camera cam = tile_camera(a);
    const TilePixel px = tile_pixel(a, cam, sa.hits, tid);
    const Ray& ray = px.ray;

    // the winner's normal and colour
    const uint32_t id = px.hit.y;
    const bool any_hit = px.in_frame && !px.newline_col && id != 0xffffffffu;
    float distance = kNoHit, shadingValue = 0.0f;
    V3 normal = ray.d, colour = ray.d, od = ray.d;
    if (any_hit) {
        distance = __uint_as_float(px.hit.x);
        const Surface s = surface_of(a, pa, id, add(ray.o, mulf(ray.d, distance)));
        normal = s.normal;
        od = s.od;
        shadingValue = normal.x * 1.0f + normal.y * 0.0f + normal.z * 0.0f; // RayTracing.cu:133
    }

    // ---- the shadow test
    const V3 L = v3(sa.light.px, sa.light.py, sa.light.pz);
    const V3 P = add(ray.o, mulf(ray.d, distance)); // the point shade() lights
    const V3 toL = sub(L, P);
    bool pending = sa.test != 0u && any_hit && distance <= cam.far;
    const uint32_t own_plane = (id & 0x80000000u) ? (id & 0x7fffffffu) : 0xffffffffu;
    bool shadowed = shadowed_before_spheres(a, sa, P, normal, L, toL, own_plane, pending);

    // spheres: the workgroup's cone from the light over its open hit points, unless every sphere is tested
    const float Lf[3] = {L.x, L.y, L.z};
    const float Pf[3] = {P.x, P.y, P.z};
    rtxshadow::Cone cone;
    if (light_cone(Lf, Pf, pending, sa.brute != 0u, a.ns, lane, wave, s_red, cone)) {
        const float len2 = dot(toL, toL);
        const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
        const uint32_t own_sphere = (id & 0x80000000u) ? 0xffffffffu : id;
        // (FIN, the rich form: the spheres that cast -- rtx_scene_set_shadow_casting; else the walk as it was)
        const uint8_t* cast_sph = nullptr;
        if constexpr (FIN) cast_sph = sa.cast.sph;
        walk_spheres_casting<kTileList, FIN>(
            a, cast_sph, tid, lane, s_occ, s_occ_pos, nullptr, &s_cnt, sa.longest,
            [&](bool in0, float4 c0, bool in1, float4 c1, uint32_t& k0, uint32_t& k1) {
                k0 = in0 && rtxshadow::may_occlude(cone, Lf, c0.x, c0.y, c0.z, c0.w) ? 1u : 0u;
                k1 = in1 && rtxshadow::may_occlude(cone, Lf, c1.x, c1.y, c1.z, c1.w) ? 1u : 0u;
            },
            [&](uint32_t cnt) {
                for (uint32_t j = 0; j < cnt && __ballot(pending) != 0ull; j++) {
                    const float4 sp = s_occ[j];
                    if (pending && s_occ_pos[j] != own_sphere && segment_hits_sphere(P, toL, inv_len2, sp)) {
                        shadowed = true;
                        pending = false;
                    }
                }
            });
    }

    // ---- shade with the light (both powers 0 in shadow) and encode
    if (any_hit) {
        colour = shade_light_of<FIN>(pa, id, ray, distance, normal, od, sa, shadowed ? 0.0f : sa.light.dpow, shadowed ? 0.0f : sa.light.spow);
        if constexpr (REFLECT) {
            if (distance <= cam.far) {
                colour = reflect_blend(a, ra, pa, ray, distance, normal, id, colour, px.at(a), [&](const Ray& r2, float t2, V3 n2, V3 od2, uint32_t id2) {
                    return shade_light_of<FIN>(pa, id2, r2, t2, n2, od2, sa, sa.light.dpow, sa.light.spow);
                });
            }
        }
    }
    encode_and_store<MODE, OUT>(a, cam, s_digits, s_ramp, px.in_frame, px.newline_col, px.row, px.col, distance, normal, colour, shadingValue);
}

template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_shadow_shade(const KArgs a, const ShadowArgsOf<FIN> sa, const PatternArgs pa)
{
    const ReflectArgs ra = {}; // (read only by the REFLECT parts, which are not compiled here)
    shade_body<MODE, OUT, false, FIN>(a, sa, ra, pa);
}

// The mirror path's third launch: rtx_shadow_shade's shading, then the blend.
template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_reflect_shade(const KArgs a, const ShadowArgsOf<FIN> sa, const ReflectArgs ra, const PatternArgs pa)
{
    shade_body<MODE, OUT, true, FIN>(a, sa, ra, pa);
}
