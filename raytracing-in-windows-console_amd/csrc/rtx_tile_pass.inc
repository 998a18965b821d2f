// rtx_tile_pass.inc -- the device code the tile passes share, included into namespace rtx of rtx_kernels.hip before the kernel
// files that use it (rtx_reflect_kernels.inc, rtx_reflect_chain_kernels.inc, rtx_shadow_kernels.inc, rtx_lights_kernels.inc,
// rtx_lights_chain_kernels.inc, rtx_chain_shadow_kernels.inc).  A tile pass is a launch that follows the trace kernel in its
// kOutHit form (every pixel's closest hit, 8 bytes: t, object): a 256-thread workgroup owns a 16 x 16 tile, every thread rebuilds its pixel's primary ray and its
// winner's surface exactly as the trace body does, the workgroup culls the scene's spheres against a bound of its pixels' rays
// (a cone of shadow segments, rtx_shadow.hpp; bundles of mirrored rays, rtx_reflect.hpp) into a list in LDS, and every thread
// runs its exact test over that list.  Each block below exists once; no floating-point operation of any of them may be added,
// removed or reordered (the passes are byte-exact against the oracle).

constexpr int kTile = 16;          // pixels per side of a workgroup's tile
constexpr int kTileList = 1024;    // sphere candidates held in LDS (20 KB with their positions)
constexpr int kReflectBundles = 4; // bundles per tile: rays grouped by direction (a tile across a room's corner spans three mirrors)

// ---------------------------------------------------------------- the pixel of a thread

struct TilePixel {
    uint32_t col, row;
    bool in_frame, newline_col;
    uint2 hit; // (t, object) of the first launch; outside the frame: no hit
    Ray ray;   // the primary ray, as the trace built it
    // the index of a pixel inside the frame in the launch's hit arrays (formed where it is used: kept, it costs two registers)
    __device__ __forceinline__ size_t at(const KArgs& a) const { return (size_t)(row - a.row0) * a.W + col; }
};

__device__ __forceinline__ Camera tile_camera(const KArgs& a)
{
    Camera cam;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        cam.m[i] = a.m[i];
    }
    cam.ox = a.ox; cam.oy = a.oy; cam.oz = a.oz;
    cam.e1 = a.e1; cam.e2 = a.e2; cam.far = a.far;
    cam.fW = a.fW; cam.fH = a.fH;
    return cam;
}

__device__ __forceinline__ TilePixel tile_pixel(const KArgs& a, const Camera& cam, const uint2* hits, uint32_t tid)
{
    TilePixel px;
    px.col = blockIdx.x * (uint32_t)kTile + (tid & (uint32_t)(kTile - 1));
    px.row = a.row0 + blockIdx.y * (uint32_t)kTile + tid / (uint32_t)kTile;
    px.in_frame = px.col < a.W && px.row < a.row_end;
    px.newline_col = px.col + 1u == a.W;
    px.hit = make_uint2(__float_as_uint(kNoHit), 0xffffffffu);
    if (px.in_frame) px.hit = hits[px.at(a)];

    // the ray, as the trace built it: RayTracing.cu:16-23 through the staged per-column / per-row terms
    const uint32_t c = px.col < a.W ? px.col : a.W - 1u;
    const uint32_t r = px.row < a.row_end ? px.row : a.row_end - 1u;
    const float vx = (((float)(2u * c) - cam.fW) / cam.fW) * cam.e1;
    const float vy = ((cam.fH - (float)(r * 2u)) / cam.fH) * cam.e2;
    px.ray = ray_from_tables(cam, make_float4(cam.m[0] * vx, cam.m[4] * vx, cam.m[8] * vx, 0.0f),
                             make_float4(cam.m[1] * vy, cam.m[5] * vy, cam.m[9] * vy, 0.0f));
    return px;
}

// ---------------------------------------------------------------- the surface of a winner

// Object `id` (sphere position, or plane index | bit 31) at point P of its surface, as the trace body derives it (RayTracing.cu:
// 123-135, Sphere.cu:67): the normal after RayTracing.cu:129 and the colour / 255.  A caller that does not read od does not load it.
struct Surface {
    V3 normal, od;
};

__device__ __forceinline__ Surface surface_of(const KArgs& a, uint32_t id, V3 P)
{
    Surface s;
    V3 n0;
    if (id & 0x80000000u) {
        const uint32_t q = id & 0x7fffffffu;
        const float4 pb = a.pl_b[q], pd = a.pl_od[q];
        n0 = v3(pb.x, pb.y, pb.z);
        s.od = v3(pd.x, pd.y, pd.z);
    } else {
        const float4 g = a.sph_geom[id], d4 = a.sph_od[id];
        n0 = normalize_gpu(sub(P, v3(g.x, g.y, g.z)));
        s.od = v3(d4.x, d4.y, d4.z);
    }
    s.normal = normalize_gpu(n0); // RayTracing.cu:129
    return s;
}

// The same for the shade launches, with the checker pattern of the object (rtx_scene_set_patterns, the rule in rtx_pattern.hpp)
// applied to od: after everything above, and feeding od alone.  One byte per shaded lane, by the index the od load used; then, for
// the lanes of a patterned object, 48 bytes of a table of at most 768 that stays in cache.  No table: no load and no arithmetic.
__device__ __forceinline__ Surface surface_of(const KArgs& a, const PatternArgs& pa, uint32_t id, V3 P)
{
    Surface s = surface_of(a, id, P);
    if (pa.table != nullptr) { // (a kernel argument: uniform)
        const uint32_t slot = (id & 0x80000000u) ? pa.slot_pl[id & 0x7fffffffu] : pa.slot_sph[id];
        if (slot != 0u && slot <= pa.n) {
            const rtxpattern::Entry e = pa.table[slot - 1u];
            const float Pf[3] = {P.x, P.y, P.z};
            if (rtxpattern::pattern_odd(Pf, e)) s.od = v3(e.od2.x, e.od2.y, e.od2.z);
        }
    }
    return s;
}

// The finish of object `id` (rtx_scene_set_finish), for the FIN forms of the shade launches (launched only while pa.fin_sph and
// pa.fin_pl are set): one 16-byte load by the index the od load used.  It is loaded where a level is shaded, not in surface_of:
// level 0's shading comes after the shadow walk, and nothing more is held across that walk.
__device__ __forceinline__ rtx_finish finish_of(const PatternArgs& pa, uint32_t id)
{
    const float4 f = (id & 0x80000000u) ? reinterpret_cast<const float4*>(pa.fin_pl)[id & 0x7fffffffu] : reinterpret_cast<const float4*>(pa.fin_sph)[id];
    return rtx_finish{f.x, f.y, f.z, __float_as_uint(f.w)};
}

// ---------------------------------------------------------------- the walk over the scene's spheres

// The scene is walked 512 spheres a step: two coalesced loads per thread, the next step's requested ahead.  keep(in0, c0, in1,
// c1, k0, k1) tests the step's two spheres of a thread together (so that a cone or a bundle is read once for both) and leaves in
// k0 / k1 what to list them with: 0 drops the sphere, anything else appends it to s_list / s_pos (ballot + mbcnt, one LDS atomic
// per wave: no test depends on the order of the list) and, where the pass has an s_payload array, its low byte beside it.  When
// the list is nearly full, and after the last step, flush(cnt) runs the threads' exact tests over its cnt entries; it must not
// contain a barrier, and nothing here may leave the loop by a condition that is not workgroup-uniform.  `longest` (or nullptr)
// gets the entries the workgroup listed over all fillings.
//
// CAST (the shadow walks of the rich forms, rtx_scene_set_shadow_casting): `cast` holds a byte per sphere in a.sph_geom's order, or
// is nullptr (a kernel argument: the test is uniform) while every sphere casts.  A sphere whose byte is 0 is dropped where it would be
// kept -- whatever keep() says of it -- so it is never listed, no flush meets it and the lists are shorter.  The byte is loaded by
// staged position (coalesced), requested with the next step's geometry and in front of it, ahead of this step's tests, and read
// behind them: the tests hide its way, the geometry's request need not have landed when it is read, and no register holds it across
// a flush (held from step to step as the geometry is, it cost the chain's families and rtx_reflect_shade an occupancy step and
// rtx_chain_shadow scratch: profiles/r39_cast_resource_usage.txt).  Without CAST nothing of this is compiled: the code is what it was.
template <int CAP, bool CAST, class Keep, class Flush>
__device__ __forceinline__ void walk_spheres_casting(const KArgs& a, const uint8_t* cast, uint32_t tid, uint32_t lane, float4* s_list, uint32_t* s_pos,
                                                     uint8_t* s_payload, uint32_t* s_cnt, uint32_t* longest, Keep keep, Flush flush)
{
    const uint32_t ns = a.ns;
    uint32_t listed = 0u; // candidates this workgroup kept after culling, over all fillings of the list
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
    if (tid < ns) g0 = a.sph_geom[tid];
    if ((uint32_t)kThreads + tid < ns) g1 = a.sph_geom[kThreads + tid];
    for (uint32_t base = 0; base < ns; base += (uint32_t)kChunk) {
        const float4 c0 = g0, c1 = g1;
        const uint32_t i0 = base + tid, i1 = base + (uint32_t)kThreads + tid;
        uint32_t f0 = 1u, f1 = 1u; // (CAST) do this step's two spheres cast a shadow?
        if constexpr (CAST) {
            if (cast != nullptr) {
                if (i0 < ns) f0 = cast[i0];
                if (i1 < ns) f1 = cast[i1];
            }
        }
        // the next step's loads go out before this step's tests
        if (i0 + (uint32_t)kChunk < ns) g0 = a.sph_geom[i0 + kChunk];
        if (i1 + (uint32_t)kChunk < ns) g1 = a.sph_geom[i1 + kChunk];
        uint32_t p0 = 0u, p1 = 0u;
        keep(i0 < ns, c0, i1 < ns, c1, p0, p1);
        if constexpr (CAST) {
            p0 = f0 != 0u ? p0 : 0u;
            p1 = f1 != 0u ? p1 : 0u;
        }
        const bool k0 = p0 != 0u, k1 = p1 != 0u;
        const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
        const uint32_t n0 = (uint32_t)__popcll(m0), n1 = (uint32_t)__popcll(m1);
        uint32_t wbase = 0u;
        if (lane == 0u && n0 + n1 != 0u) wbase = atomicAdd(s_cnt, n0 + n1);
        wbase = (uint32_t)__shfl((int)wbase, 0);
        if (k0) {
            const uint32_t p = wbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
            s_list[p] = c0;
            s_pos[p] = i0;
            if (s_payload != nullptr) s_payload[p] = (uint8_t)p0;
        }
        if (k1) {
            const uint32_t p = wbase + n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
            s_list[p] = c1;
            s_pos[p] = i1;
            if (s_payload != nullptr) s_payload[p] = (uint8_t)p1;
        }
        // The counter protocol, one step: appends (LDS atomics) | barrier | every wave reads the count | barrier | (flush: reset
        // the count, test the list | barrier).  The second barrier is what keeps it race-free: no wave appends the next step's
        // survivors, or resets the count, before every wave has read this step's count, so all waves see the same count, take
        // the same branch and meet the same barriers; and the count can only reach CAP - kChunk + kChunk before a flush.
        lds_barrier(); // this step's appends are done
        const uint32_t cnt = __builtin_amdgcn_readfirstlane(*s_cnt);
        lds_barrier(); // every wave has read the count
        if (cnt > (uint32_t)(CAP - kChunk) || base + (uint32_t)kChunk >= ns) {
            if (tid == 0u) *s_cnt = 0u; // (nothing reads or appends to it before the barrier below)
            listed += cnt;
            flush(cnt);
            lds_barrier(); // every wave is done with the list, and the reset is visible
        }
    }
    if (longest != nullptr && tid == 0u) atomicMax(longest, listed);
}

template <int CAP, class Keep, class Flush>
__device__ __forceinline__ void walk_spheres(const KArgs& a, uint32_t tid, uint32_t lane, float4* s_list, uint32_t* s_pos, uint8_t* s_payload, uint32_t* s_cnt,
                                             uint32_t* longest, Keep keep, Flush flush)
{
    walk_spheres_casting<CAP, false>(a, nullptr, tid, lane, s_list, s_pos, s_payload, s_cnt, longest, keep, flush);
}

// ---------------------------------------------------------------- the shadow test of one light

// Self-shadow and the planes, per pixel: is the visible point P (normal `normal`, on plane own_plane or 0xffffffff) cut off from
// the light L (toL = L - P)?  A pixel that is leaves `pending`; one that stays pending has its segment tested against the spheres.
// CAST (rtx_scene_set_shadow_casting): cast_pl holds a byte per plane, or is nullptr while every plane casts; a plane whose byte is 0
// is no occluder -- one wave-uniform read per plane.  Self-shadow stays: a non-casting object still shadows itself.
template <bool CAST>
__device__ __forceinline__ bool shadowed_before_spheres_casting(const KArgs& a, const uint8_t* cast_pl, V3 P, V3 normal, V3 L, V3 toL, uint32_t own_plane, bool& pending)
{
    bool shadowed = false;
    if (pending && dot(normal, toL) <= 0.0f) {
        shadowed = true; // facing away from the light
        pending = false;
    }
    // planes: few, wave-uniform index (scalar loads)
    if (__ballot(pending) != 0ull) {
        for (uint32_t q = 0; q < a.np; q++) {
            if constexpr (CAST) {
                if (cast_pl != nullptr && cast_pl[q] == 0u) continue; // (uniform)
            }
            const float4 pa = a.pl_a[q], pb = a.pl_b[q];
            const V3 pp = v3(pa.x, pa.y, pa.z), pn = v3(pb.x, pb.y, pb.z);
            const float sP = dot(sub(P, pp), pn), sL = dot(sub(L, pp), pn);
            if (pending && q != own_plane && ((sP < 0.0f && sL > 0.0f) || (sP > 0.0f && sL < 0.0f))) {
                const V3 x = add(P, mulf(toL, sP / (sP - sL)));
                const float hw = pa.w * 0.5f, hh = pb.w * 0.5f;
                if (!((x.x <= pp.x - hw || x.x >= pp.x + hw) || (x.z <= pp.z - hh || x.z >= pp.z + hh))) { // Plane.cu:66-67
                    shadowed = true;
                    pending = false;
                }
            }
        }
    }
    return shadowed;
}

__device__ __forceinline__ bool shadowed_before_spheres(const KArgs& a, V3 P, V3 normal, V3 L, V3 toL, uint32_t own_plane, bool& pending)
{
    return shadowed_before_spheres_casting<false>(a, nullptr, P, normal, L, toL, own_plane, pending);
}

// The same under a light set that may carry cones (rtx_scene_set_spots): with a SpotLightsArgs, a point outside light i's cone --
// rtx_spot.hpp's own s, from the lightDir the shading forms at P, is not above 0 -- leaves `pending` first, and is not shadowed: the
// shade launch weighs the light with 0 there, which is the float a dark light enters with.  With a LightsArgs nothing is added.
template <class LA>
__device__ __forceinline__ bool shadowed_before_spheres(const KArgs& a, const LA& la, uint32_t i, V3 P, V3 normal, V3 L, V3 toL, uint32_t own_plane, bool& pending)
{
    if constexpr (std::is_same_v<LA, SpotLightsArgs>) {
        const rtxspot::Packed& sp = la.spots.spot[i];
        if (pending && rtxspot::has_cone(sp)) {
            const V3 ld = normalize_gpu(toL);
            if (rtxspot::outside(sp, ld.x, ld.y, ld.z)) pending = false;
        }
        return shadowed_before_spheres_casting<true>(a, la.cast.pl, P, normal, L, toL, own_plane, pending); // (the planes that cast)
    }
    return shadowed_before_spheres(a, P, normal, L, toL, own_plane, pending);
}

// ... and under the one light of rtx_shadow_shade / rtx_reflect_shade (SpotShadowArgs: its cone).
template <class SA>
__device__ __forceinline__ bool shadowed_before_spheres(const KArgs& a, const SA& sa, V3 P, V3 normal, V3 L, V3 toL, uint32_t own_plane, bool& pending)
{
    if constexpr (std::is_same_v<SA, SpotShadowArgs>) {
        if (pending && rtxspot::has_cone(sa.spot)) {
            const V3 ld = normalize_gpu(toL);
            if (rtxspot::outside(sa.spot, ld.x, ld.y, ld.z)) pending = false;
        }
        return shadowed_before_spheres_casting<true>(a, sa.cast.pl, P, normal, L, toL, own_plane, pending); // (the planes that cast)
    }
    return shadowed_before_spheres(a, P, normal, L, toL, own_plane, pending);
}

// The workgroup's cone from light Lf over its pending hit points Pf (rtx_shadow.hpp).  false: no pixel of the workgroup is
// pending, or the scene has no sphere -- there is no cone and nothing to walk (workgroup-uniform, as everything derived from
// the sums); true: `cone` holds it, in every thread (brute: a cone that keeps every sphere).  Every wave meets the first
// barrier, which also makes what the caller wrote to LDS before the call visible; the caller keeps s_red untouched until its
// next barrier.
__device__ __forceinline__ bool light_cone(const float Lf[3], const float Pf[3], bool pending, bool brute, uint32_t ns, uint32_t lane, uint32_t wave,
                                           float (*s_red)[6], rtxshadow::Cone& cone)
{
    float u[3] = {0.0f, 0.0f, 0.0f}, dist = 0.0f;
    bool degenerate = false;
    if (pending) degenerate = !rtxshadow::direction_from_light(Lf, Pf, u, &dist);
    float red[6] = {u[0], u[1], u[2], pending ? 1.0f : 0.0f, pending ? dist : 0.0f, degenerate ? 1.0f : 0.0f};
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        red[0] += __shfl_xor(red[0], k);
        red[1] += __shfl_xor(red[1], k);
        red[2] += __shfl_xor(red[2], k);
        red[3] += __shfl_xor(red[3], k);
        red[4] = fmaxf(red[4], __shfl_xor(red[4], k));
        red[5] = fmaxf(red[5], __shfl_xor(red[5], k));
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 6; k++) s_red[wave][k] = red[k];
    }
    lds_barrier(); // the reduction visible
    float sum[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int w = 0; w < 4; w++) {
        sum[0] += s_red[w][0];
        sum[1] += s_red[w][1];
        sum[2] += s_red[w][2];
        sum[3] += s_red[w][3];
        sum[4] = fmaxf(sum[4], s_red[w][4]);
        sum[5] = fmaxf(sum[5], s_red[w][5]);
    }
    if (!(sum[3] > 0.0f) || ns == 0u) return false;
    float axis[3] = {0.0f, 0.0f, 0.0f};
    const bool all = brute || sum[5] > 0.0f || !rtxshadow::axis_from_sum(sum[0], sum[1], sum[2], sum[3], axis);
    float ang = 0.0f;
    if (!all) {
        ang = pending ? rtxshadow::angle_from_axis(axis, u) : 0.0f;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) ang = fmaxf(ang, __shfl_xor(ang, k));
        lds_barrier(); // everyone has read the sums
        if (lane == 0u) s_red[wave][0] = ang;
        lds_barrier();
        ang = fmaxf(fmaxf(s_red[0][0], s_red[1][0]), fmaxf(s_red[2][0], s_red[3][0]));
    }
    cone = rtxshadow::make_cone(Lf, axis, ang, sum[4], all);
    return true;
}

// The exact test of a pixel's segment (P, P + toL), inv_len2 = 1 / |toL|^2 (0 for a point): the closest point of the segment to
// the centre of sphere sp, closer than r.
__device__ __forceinline__ bool segment_hits_sphere(V3 P, V3 toL, float inv_len2, float4 sp)
{
    const V3 w = sub(v3(sp.x, sp.y, sp.z), P);
    const float s = dot(w, toL) * inv_len2;
    const float k = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
    const V3 e = sub(w, mulf(toL, k));
    return dot(e, e) < sp.w * sp.w;
}

// ---------------------------------------------------------------- the shadow test of a set of lights

// The LDS of a workgroup of the light-set kernels (rtx_lights_kernels.inc and the files after it): lights_dark_set's list, sums and
// cones, and the encoder's tables.
struct LightsShared {
    float4 occ[kTileList];
    uint32_t occ_pos[kTileList];
    uint32_t occ_mask[kTileList / 4]; // one byte per entry: the lights the sphere was kept for
    uint32_t digits[256];
    __attribute__((aligned(4))) uint8_t ramp[68];
    float red[4][6];
    rtxshadow::Cone cone[rtxlights::kMaxLights];
    uint32_t cnt;
};

// The lights (bit i: light i of la.lights) that the point P -- normal `normal`, on object `id` (sphere position, or plane index |
// bit 31) -- is shadowed from; 0 for a pixel that is not `testable`.  Per light: its cone (la a SpotLightsArgs), self-shadow and the planes per pixel
// (shadowed_before_spheres) and the workgroup's cone from that light over its open points (light_cone), kept in s.cone; a light
// with no open pixel in the workgroup has no cone.  Then ONE walk of the scene for all lights (walk_spheres): each staged sphere is
// tested against every live cone and listed once with the 8-bit mask of the lights it was kept for; at a flush every wave goes
// through the lights some lane of it is still open for, the segment (toL, 1 / len2) formed once per light.  Called by every
// thread of the workgroup (the trip counts are workgroup-uniform; every wave meets the same barriers, at least one per light).
// `s` holds occ, occ_pos, occ_mask (one byte per entry), red, cone and cnt, which is 0 on entry and 0 again on return.
template <class Shared, class LA>
__device__ __forceinline__ uint32_t lights_dark_set(const KArgs& a, const LA& la, Shared& s, uint32_t tid, uint32_t lane, uint32_t wave, V3 P, V3 normal,
                                                    uint32_t id, bool testable)
{
    const uint32_t nl = la.lights.n;
    const float Pf[3] = {P.x, P.y, P.z};
    const uint32_t own_plane = (id & 0x80000000u) ? (id & 0x7fffffffu) : 0xffffffffu;
    uint32_t open = 0u; // lights this pixel's segment is still to be tested for
    uint32_t dark = 0u; // lights this pixel is shadowed from
    uint32_t live = 0u; // lights with a cone: some pixel of the workgroup is open for them (workgroup-uniform)
    for (uint32_t i = 0; i < nl; i++) { // (every wave meets the same barriers: the trip count is the set's size)
        const rtxlights::PackedLight& Lt = la.lights.light[i];
        const V3 L = v3(Lt.px, Lt.py, Lt.pz);
        bool pending = testable;
        if (shadowed_before_spheres(a, la, i, P, normal, L, sub(L, P), own_plane, pending)) dark |= 1u << i;
        if (pending) open |= 1u << i;

        const float Lf[3] = {L.x, L.y, L.z};
        rtxshadow::Cone cone;
        if (light_cone(Lf, Pf, pending, la.brute != 0u, a.ns, lane, wave, s.red, cone)) {
            if (tid == 0u) s.cone[i] = cone;
            live |= 1u << i;
        }
        lds_barrier(); // everyone is done with this light's sums before the next light's are written; the cone is visible
    }
    live = __builtin_amdgcn_readfirstlane(live);

    // ---- spheres: one walk of the scene for all lights
    if (live != 0u) {
        const uint32_t own_sphere = (id & 0x80000000u) ? 0xffffffffu : id;
        // (the rich form: the spheres that cast -- rtx_scene_set_shadow_casting; else the walk as it was)
        constexpr bool kCast = std::is_same_v<LA, SpotLightsArgs>;
        const uint8_t* cast_sph = nullptr;
        if constexpr (kCast) cast_sph = la.cast.sph;
        walk_spheres_casting<kTileList, kCast>(
            a, cast_sph, tid, lane, s.occ, s.occ_pos, reinterpret_cast<uint8_t*>(s.occ_mask), &s.cnt, la.longest,
            [&](bool in0, float4 c0, bool in1, float4 c1, uint32_t& km0, uint32_t& km1) { // the lights each of the two spheres may occlude
                for (uint32_t m = live; m != 0u; m &= m - 1u) {
                    const uint32_t i = (uint32_t)__builtin_ctz(m);
                    const rtxshadow::Cone cone = s.cone[i];
                    const float Lf[3] = {la.lights.light[i].px, la.lights.light[i].py, la.lights.light[i].pz};
                    if (in0 && rtxshadow::may_occlude(cone, Lf, c0.x, c0.y, c0.z, c0.w)) km0 |= 1u << i;
                    if (in1 && rtxshadow::may_occlude(cone, Lf, c1.x, c1.y, c1.z, c1.w)) km1 |= 1u << i;
                }
            },
            [&](uint32_t cnt) {
                for (uint32_t m = live; m != 0u; m &= m - 1u) {
                    const uint32_t i = (uint32_t)__builtin_ctz(m), bit = 1u << i;
                    bool pending = (open & bit) != 0u;
                    if (__ballot(pending) == 0ull) continue; // no lane of this wave is open for the light
                    const V3 toL = sub(v3(la.lights.light[i].px, la.lights.light[i].py, la.lights.light[i].pz), P);
                    const float len2 = dot(toL, toL);
                    const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
                    const uint32_t sel = 0x01010101u << i;
                    for (uint32_t j4 = 0; j4 < cnt && __ballot(pending) != 0ull; j4 += 4u) {
                        // four entries' masks a word; entries at or past cnt are leftovers
                        for (uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.occ_mask[j4 >> 2]) & sel; w != 0u; w &= w - 1u) {
                            const uint32_t j = j4 + ((uint32_t)__builtin_ctz(w) >> 3);
                            if (j >= cnt) break;
                            const float4 sp = s.occ[j];
                            if (pending && s.occ_pos[j] != own_sphere) {
                                const bool hit = segment_hits_sphere(P, toL, inv_len2, sp);
                                dark |= hit ? bit : 0u;
                                pending = !hit;
                            }
                        }
                    }
                    if (!pending) open &= ~bit;
                }
            });
    }
    return dark;
}

// ---------------------------------------------------------------- the mirror's secondary rays

// The reflectivity of a winner (sphere position, or plane index | bit 31), by the order the trace kernels index spheres by.
__device__ __forceinline__ float reflectivity_of(const ReflectArgs& ra, uint32_t id)
{
    return (id & 0x80000000u) ? ra.k_pl[id & 0x7fffffffu] : ra.k_sph[id];
}

// Steps 1-2 of the mirror: the secondary ray of `ray` hit at `distance` with normal `normal` (after RayTracing.cu:129).  It starts
// at the point shade_light lights, P = O + D t, in the direction R = N c - V, c = 2 (N . V), N = normalize_gpu(normal) and V =
// normalize_gpu(-D) (shade_light's viewDir); a = R . R, fourA = 4a, divTwoA = 1 / (2a) (RayTracing.cu:90-92).
__device__ __forceinline__ Ray mirror_ray(const Ray& ray, float distance, V3 normal)
{
    const V3 N = normalize_gpu(normal);
    const V3 V = normalize_gpu(mulf(ray.d, -1.0f));
    const float c = 2.0f * dot(N, V);
    Ray r;
    r.o = add(ray.o, mulf(ray.d, distance));
    r.d = v3(N.x * c - V.x, N.y * c - V.y, N.z * c - V.z);
    r.a = dot(r.d, r.d);
    r.fourA = 4.0f * r.a;
    r.divTwoA = rcp_cr(2.0f * r.a); // = 1.0f / (2.0f * a), bit for bit
    return r;
}

// The next ray of a chain: `ray` hit object `id` (sphere position, or plane index | bit 31; 0xffffffff: none, a lane whose ray
// nobody reads) at `distance` with normal `normal`.  While no object is refractive (ra.ior_sph == nullptr, a kernel argument: the
// test is uniform) it is mirror_ray and nothing is loaded.  Otherwise ior(id) picks the case per lane (rtx_scene_set_refraction,
// the rule in include/rtx.h): 0, the mirror's ray, bit for bit; a sphere, the ray that leaves its far side (rtx_refract.hpp:
// through_sphere, with P, N and V formed as mirror_ray forms them and the stored radius); a plane, a thin sheet: the ray goes on
// from P in its direction.  a, fourA and divTwoA as mirror_ray forms them.
// (secondary_ray<GLASS>: for a caller that has made the uniform test itself, outside its level loop -- GLASS = ra.ior_sph != nullptr.)
template <bool GLASS>
__device__ __forceinline__ Ray secondary_ray(const KArgs& a, const ReflectArgs& ra, const Ray& ray, float distance, V3 normal, uint32_t id)
{
    Ray r = mirror_ray(ray, distance, normal);
    if constexpr (GLASS) {
        const bool plane = (id & 0x80000000u) != 0u;
        float ior = 0.0f;
        if (id != 0xffffffffu) ior = plane ? ra.ior_pl[id & 0x7fffffffu] : ra.ior_sph[id];
        if (ior > 0.0f) {
            if (plane) {
                r.d = ray.d; // (r.o is P already)
            } else {
                const V3 N = normalize_gpu(normal);
                const V3 V = normalize_gpu(mulf(ray.d, -1.0f));
                const float Pf[3] = {r.o.x, r.o.y, r.o.z}, Nf[3] = {N.x, N.y, N.z}, Vf[3] = {V.x, V.y, V.z};
                float of[3], df[3];
                rtxrefract::through_sphere(
                    Pf, Nf, Vf, a.sph_geom[id].w, ior, [](float x) { return sqrt_cr(x); }, [](float x) { return rcp_cr(x); }, of, df);
                r.o = v3(of[0], of[1], of[2]);
                r.d = v3(df[0], df[1], df[2]);
            }
            r.a = dot(r.d, r.d);
            r.fourA = 4.0f * r.a;
            r.divTwoA = rcp_cr(2.0f * r.a);
        }
    }
    return r;
}

__device__ __forceinline__ Ray secondary_ray(const KArgs& a, const ReflectArgs& ra, const Ray& ray, float distance, V3 normal, uint32_t id)
{
    if (ra.ior_sph != nullptr) return secondary_ray<true>(a, ra, ray, distance, normal, id);
    return mirror_ray(ray, distance, normal);
}

// Creation index of an object (sphere position, or plane index | bit 31): looked up only to break an exact tie in t.
__device__ __forceinline__ uint32_t creation_index(const KArgs& a, uint32_t id)
{
    return __float_as_uint((id & 0x80000000u) ? a.pl_od[id & 0x7fffffffu].w : a.sph_od[id].w);
}

// Does (t, id) come before the best so far (bt, bid) in (t, creation index) order?  No best yet: bid = 0xffffffff, bt = kNoHit.
__device__ __forceinline__ bool comes_before(const KArgs& a, float t, uint32_t id, float bt, uint32_t bid)
{
    return t < bt || (t == bt && (bid == 0xffffffffu || creation_index(a, id) < creation_index(a, bid)));
}

// Sphere::Trace for a ray of its own origin: otc = o - c and cc = Dot(otc, otc) - r*r per ray (Sphere.cu:34-37).
__device__ __forceinline__ bool secondary_sphere_hit(const Ray& r, float4 g, float& t)
{
    const float ox = r.o.x - g.x, oy = r.o.y - g.y, oz = r.o.z - g.z;
    const float oo = ox * ox + oy * oy + oz * oz;
    const float cc = oo - (g.w * g.w);
    float s;
    if (sphere_reject(r, ox, oy, oz, cc, s)) return false;
    return sphere_hit(r, s, cc, t);
}

// The closest hit (bt, bid) of a pending secondary ray r that leaves object `id`, with the reference's tests (Sphere.cu:30-68,
// Plane.cu:38-72) and no far limit, the winner the lexicographic minimum of (t, creation index): first over every plane, then,
// at each flush of the walk, over the cnt spheres of the list -- the minimum does not depend on the order of the list.
__device__ __forceinline__ void closest_of_planes(const KArgs& a, const Ray& r, bool pending, uint32_t id, float& bt, uint32_t& bid)
{
    // planes: few, wave-uniform index (scalar loads)
    if (__ballot(pending) != 0ull) {
        for (uint32_t q = 0; q < a.np; q++) {
            const float4 pa = a.pl_a[q], pb = a.pl_b[q];
            float t;
            const uint32_t qid = 0x80000000u | q;
            if (pending && qid != id && plane_hit(r, v3(pa.x, pa.y, pa.z), v3(pb.x, pb.y, pb.z), pa.w, pb.w, t) && comes_before(a, t, qid, bt, bid)) {
                bt = t;
                bid = qid;
            }
        }
    }
}

__device__ __forceinline__ void closest_of_list(const KArgs& a, const Ray& r, bool pending, uint32_t id, const float4* s_list, const uint32_t* s_pos,
                                                uint32_t cnt, float& bt, uint32_t& bid)
{
    for (uint32_t j = 0; j < cnt; j++) {
        const float4 sp = s_list[j];
        const uint32_t pos = s_pos[j];
        float t;
        if (pending && pos != id && secondary_sphere_hit(r, sp, t) && comes_before(a, t, pos, bt, bid)) {
            bt = t;
            bid = pos;
        }
    }
}

// The tile's pending secondary rays r grouped into up to kReflectBundles bundles, each a ball of origins and a cone of directions
// (rtx_reflect.hpp), in s_bundle; returns how many (workgroup-uniform; 0: no ray is pending).  Group g: the open ray of the lowest
// thread (its leader) and every open ray within 60 degrees of the leader's direction; the last group takes whatever is left.  A
// tile that spans two or three mirrors (a room's corner) gets a narrow bundle per mirror where one bundle over all of them would
// have a half-angle past 90 degrees and keep every sphere.  Every ray belongs to one bundle, so a list of the spheres that may
// meet any of them holds every sphere any of the tile's rays can hit.  brute: one bundle that keeps every sphere.  Every wave
// meets the first barrier, which also makes what the caller wrote to LDS before the call visible.
__device__ __forceinline__ uint32_t build_bundles(const Ray& r, bool pending, bool brute, uint32_t tid, uint32_t lane, uint32_t wave, float (*s_red)[8],
                                                  rtxreflect::Bundle* s_bundle, float (*s_lead_u)[3], uint32_t* s_lead_lane)
{
    const float Pf[3] = {r.o.x, r.o.y, r.o.z}, Rf[3] = {r.d.x, r.d.y, r.d.z};
    float u[3] = {0.0f, 0.0f, 0.0f};
    bool degenerate = false;
    if (pending) degenerate = !rtxreflect::unit_direction(Pf, Rf, u);
    uint32_t nb = 0; // bundles built (workgroup-uniform)
    bool open = pending;
    for (int g = 0; g < kReflectBundles; g++) {
        // the leader: the lowest open thread of the workgroup
        const unsigned long long m = __ballot(open);
        if (lane == 0u) s_lead_lane[wave] = m != 0ull ? (uint32_t)__builtin_ctzll(m) : 64u;
        if (open && m != 0ull && lane == (uint32_t)__builtin_ctzll(m)) {
            s_lead_u[wave][0] = u[0];
            s_lead_u[wave][1] = u[1];
            s_lead_u[wave][2] = u[2];
        }
        lds_barrier(); // (also: every read of the previous group's s_red is done)
        uint32_t lw = 0u;
        while (lw < 4u && s_lead_lane[lw] == 64u) lw++;
        if (lw == 4u) break; // no open ray left (uniform)
        const uint32_t lead_tid = lw * 64u + s_lead_lane[lw];
        const float lu[3] = {s_lead_u[lw][0], s_lead_u[lw][1], s_lead_u[lw][2]};
        const bool take_all = brute || g == kReflectBundles - 1;
        const bool member = open && (take_all || tid == lead_tid || u[0] * lu[0] + u[1] * lu[1] + u[2] * lu[2] >= 0.5f);
        open = open && !member;

        float red[8] = {member ? Pf[0] : 0.0f, member ? Pf[1] : 0.0f, member ? Pf[2] : 0.0f, member ? u[0] : 0.0f, member ? u[1] : 0.0f,
                        member ? u[2] : 0.0f, member ? 1.0f : 0.0f, member && degenerate ? 1.0f : 0.0f};
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
#pragma unroll
            for (int v = 0; v < 7; v++) red[v] += __shfl_xor(red[v], k);
            red[7] = fmaxf(red[7], __shfl_xor(red[7], k));
        }
        if (lane == 0u) {
#pragma unroll
            for (int v = 0; v < 8; v++) s_red[wave][v] = red[v];
        }
        lds_barrier(); // the group's sums visible
        float sum[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < 4; w++) {
#pragma unroll
            for (int v = 0; v < 7; v++) sum[v] += s_red[w][v];
            sum[7] = fmaxf(sum[7], s_red[w][7]);
        }
        float centre[3] = {0.0f, 0.0f, 0.0f}, axis[3] = {0.0f, 0.0f, 0.0f};
        rtxreflect::centre_from_sum(sum[0], sum[1], sum[2], sum[6], centre);
        const bool all = brute || sum[7] > 0.0f || !rtxreflect::axis_from_sum(sum[3], sum[4], sum[5], sum[6], axis);
        float dist = 0.0f, ang = 0.0f;
        if (!all) {
            dist = member ? rtxreflect::distance_from_centre(centre, Pf) : 0.0f;
            ang = member ? rtxreflect::angle_from_axis(axis, u) : 0.0f;
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                dist = fmaxf(dist, __shfl_xor(dist, k));
                ang = fmaxf(ang, __shfl_xor(ang, k));
            }
            lds_barrier(); // everyone has read the sums
            if (lane == 0u) {
                s_red[wave][0] = dist;
                s_red[wave][1] = ang;
            }
            lds_barrier();
            dist = fmaxf(fmaxf(s_red[0][0], s_red[1][0]), fmaxf(s_red[2][0], s_red[3][0]));
            ang = fmaxf(fmaxf(s_red[0][1], s_red[1][1]), fmaxf(s_red[2][1], s_red[3][1]));
        }
        if (tid == 0u) s_bundle[g] = rtxreflect::make_bundle(centre, axis, dist, ang, all);
        nb = (uint32_t)g + 1u;
        lds_barrier(); // s_bundle[g] visible; every read of s_lead_* and s_red is done before the next group writes them
    }
    return nb;
}

// keep() of walk_spheres for the mirror's passes: a sphere is listed when it may meet any of the nb bundles.
struct MayMeetBundles {
    const rtxreflect::Bundle* s_bundle;
    uint32_t nb;
    __device__ __forceinline__ void operator()(bool in0, float4 c0, bool in1, float4 c1, uint32_t& k0, uint32_t& k1) const
    {
        bool b0 = false, b1 = false;
        for (uint32_t b = 0; b < nb; b++) {
            b0 = b0 || (in0 && rtxreflect::may_hit(s_bundle[b], c0.x, c0.y, c0.z, c0.w));
            b1 = b1 || (in1 && rtxreflect::may_hit(s_bundle[b], c1.x, c1.y, c1.z, c1.w));
        }
        k0 = b0 ? 1u : 0u;
        k1 = b1 ? 1u : 0u;
    }
};

// Steps 4-6 for one pixel of the mirror path's shading launch: the secondary hit (ra.hits2[at]) shaded by shade(r2, t2, normal,
// od, object) -- the light or lights at full powers, no shadow test there (the chain's launches have one: RTX_OPT_REFLECT_SHADOWS), no
// further bounce; black without a hit -- and blended with the local colour cl.  Pixels whose winner does not reflect keep cl.
template <class Shade>
__device__ __forceinline__ V3 reflect_blend(const KArgs& a, const ReflectArgs& ra, const PatternArgs& pa, const Ray& ray, float distance, V3 normal, uint32_t id,
                                            V3 cl, size_t at, Shade shade)
{
    const float k = reflectivity_of(ra, id);
    if (!(k > 0.0f)) return cl;
    const Ray r2 = secondary_ray(a, ra, ray, distance, normal, id);
    const uint2 h = ra.hits2[at];
    V3 cr = v3(0.0f, 0.0f, 0.0f);
    if (h.y != 0xffffffffu) {
        const float t2 = __uint_as_float(h.x);
        const Surface s2 = surface_of(a, pa, h.y, add(r2.o, mulf(r2.d, t2)));
        cr = shade(r2, t2, s2.normal, s2.od, h.y);
    }
    const float w = 1.0f - k;
    return v3(minf(255.0f, cl.x * w + cr.x * k), minf(255.0f, cl.y * w + cr.y * k), minf(255.0f, cl.z * w + cr.z * k));
}
