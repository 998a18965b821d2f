// rtx_reflect_kernels.inc -- the mirror path (rtx_scene_set_reflectivity), included into namespace rtx of rtx_kernels.hip before
// rtx_shadow_kernels.inc.  Three launches: the trace kernel in its kOutHit form (every pixel's closest hit), rtx_reflect_hit (the
// closest hit of each reflective pixel's secondary ray) and rtx_reflect_shade (rtx_shadow_shade's shading, then the blend).
//
// A pixel reflects when it is visible (t <= cam_far, not column W-1) and its winner o has k > 0.  Its secondary ray starts at the
// point shade_light lights, P = O + D t, in the direction R = N c - V, c = 2 (N . V), with N = normalize_gpu(normal) of the
// primary normal after RayTracing.cu:129 and V = normalize_gpu(-D) (shade_light's viewDir); a = R . R, fourA = 4a, divTwoA =
// 1 / (2a) (RayTracing.cu:90-92).  It is tested against every sphere and plane but o with the reference's tests (Sphere.cu:30-68,
// otc = P - C and cc per ray; Plane.cu:38-72) and no far limit; the winner is the lexicographic minimum of (t, creation index).
//
// rtx_reflect_hit: a 256-thread workgroup owns a 16 x 16 tile.  Every thread rebuilds its primary exactly as rtx_shadow_shade
// does and forms its secondary ray; the planes are tested per pixel.  The waves reduce the tile's secondary rays to up to four bundles,
// each a ball of origins and a cone of directions (rtx_reflect.hpp), the scene is walked 512 spheres a step (the next step's loads in
// flight), and the spheres that may meet a bundle are appended to an LDS list by the shadow pass's counter protocol.  When
// the list is nearly full, and after the last step, every wave runs its pending pixels' exact closest-hit test over it.  The
// minimum does not depend on the order of the list, so the culled result equals the brute one.  Tiles with no reflective pixel
// skip the walk.

constexpr int kReflectTile = 16;   // pixels per side of a workgroup's tile
constexpr int kReflectList = 1024; // sphere candidates held in LDS (20 KB with their positions)
constexpr int kReflectBundles = 4; // bundles per tile: rays grouped by direction (a tile across a room's corner spans three mirrors)

// The reflectivity of a winner (sphere position, or plane index | bit 31), by the order the trace kernels index spheres by.
__device__ __forceinline__ float reflectivity_of(const ReflectArgs& ra, uint32_t id)
{
    return (id & 0x80000000u) ? ra.k_pl[id & 0x7fffffffu] : ra.k_sph[id];
}

// Steps 1-2 of the mirror: the secondary ray of primary `ray` hit at `distance` with normal `normal` (after RayTracing.cu:129).
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

// Steps 4-6 for one pixel of the third launch: the secondary hit shaded with the light's full powers (no shadow test there, no
// further bounce; black without a hit) and blended with the local colour cl.  Pixels whose winner does not reflect keep cl.
__device__ __forceinline__ V3 reflect_blend(const KArgs& a, const ShadowArgs& sa, const ReflectArgs& ra, const Ray& ray, float distance, V3 normal,
                                            uint32_t id, V3 cl, size_t at)
{
    const float k = reflectivity_of(ra, id);
    if (!(k > 0.0f)) return cl;
    const Ray r2 = mirror_ray(ray, distance, normal);
    const uint2 h = ra.hits2[at];
    V3 cr = v3(0.0f, 0.0f, 0.0f);
    if (h.y != 0xffffffffu) {
        const float t2 = __uint_as_float(h.x);
        V3 n0, od;
        if (h.y & 0x80000000u) {
            const uint32_t q = h.y & 0x7fffffffu;
            const float4 pb = a.pl_b[q], pd = a.pl_od[q];
            n0 = v3(pb.x, pb.y, pb.z);
            od = v3(pd.x, pd.y, pd.z);
        } else {
            const float4 g = a.sph_geom[h.y], d4 = a.sph_od[h.y];
            n0 = normalize_gpu(sub(add(r2.o, mulf(r2.d, t2)), v3(g.x, g.y, g.z)));
            od = v3(d4.x, d4.y, d4.z);
        }
        cr = shade_light(r2, t2, normalize_gpu(n0), od, sa.light, sa.light.dpow, sa.light.spow);
    }
    const float w = 1.0f - k;
    return v3(minf(255.0f, cl.x * w + cr.x * k), minf(255.0f, cl.y * w + cr.y * k), minf(255.0f, cl.z * w + cr.z * k));
}

__global__ __launch_bounds__(kThreads) void rtx_reflect_hit(const KArgs a, const ReflectArgs ra)
{
    __shared__ float4 s_cand[kReflectList];
    __shared__ uint32_t s_cand_pos[kReflectList];
    __shared__ float s_red[4][8];
    __shared__ rtxreflect::Bundle s_bundle[kReflectBundles];
    __shared__ float s_lead_u[4][3];
    __shared__ uint32_t s_lead_lane[4];
    __shared__ uint32_t s_cnt;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    if (tid == 0u) s_cnt = 0u;

    Camera cam;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        cam.m[i] = a.m[i];
    }
    cam.ox = a.ox; cam.oy = a.oy; cam.oz = a.oz;
    cam.e1 = a.e1; cam.e2 = a.e2; cam.far = a.far;
    cam.fW = a.fW; cam.fH = a.fH;

    const uint32_t col = blockIdx.x * (uint32_t)kReflectTile + (tid & (uint32_t)(kReflectTile - 1));
    const uint32_t row = a.row0 + blockIdx.y * (uint32_t)kReflectTile + tid / (uint32_t)kReflectTile;
    const bool in_frame = col < a.W && row < a.row_end;
    const bool newline_col = col + 1u == a.W;
    uint2 hit = make_uint2(__float_as_uint(kNoHit), 0xffffffffu);
    if (in_frame) hit = ra.hits[(size_t)(row - a.row0) * a.W + col];

    // the primary ray, its winner's normal and the reflectivity, as rtx_shadow_shade rebuilds them
    const uint32_t c = col < a.W ? col : a.W - 1u;
    const uint32_t r = row < a.row_end ? row : a.row_end - 1u;
    const float vx = (((float)(2u * c) - cam.fW) / cam.fW) * cam.e1;
    const float vy = ((cam.fH - (float)(r * 2u)) / cam.fH) * cam.e2;
    const Ray ray = ray_from_tables(cam, make_float4(cam.m[0] * vx, cam.m[4] * vx, cam.m[8] * vx, 0.0f),
                                    make_float4(cam.m[1] * vy, cam.m[5] * vy, cam.m[9] * vy, 0.0f));
    const uint32_t id = hit.y;
    const float distance = __uint_as_float(hit.x);
    bool pending = in_frame && !newline_col && id != 0xffffffffu && distance <= cam.far;
    if (pending) pending = reflectivity_of(ra, id) > 0.0f;
    V3 normal = ray.d;
    if (pending) {
        V3 n0;
        if (id & 0x80000000u) {
            const float4 pb = a.pl_b[id & 0x7fffffffu];
            n0 = v3(pb.x, pb.y, pb.z);
        } else {
            const float4 g = a.sph_geom[id];
            n0 = normalize_gpu(sub(add(ray.o, mulf(ray.d, distance)), v3(g.x, g.y, g.z)));
        }
        normal = normalize_gpu(n0); // RayTracing.cu:129
    }
    const Ray r2 = mirror_ray(ray, pending ? distance : 0.0f, normal);
    float bt = kNoHit;
    uint32_t bid = 0xffffffffu;

    // planes: few, wave-uniform index (scalar loads)
    if (__ballot(pending) != 0ull) {
        for (uint32_t q = 0; q < a.np; q++) {
            const float4 pa = a.pl_a[q], pb = a.pl_b[q];
            float t;
            const uint32_t qid = 0x80000000u | q;
            if (pending && qid != id && plane_hit(r2, v3(pa.x, pa.y, pa.z), v3(pb.x, pb.y, pb.z), pa.w, pb.w, t) && comes_before(a, t, qid, bt, bid)) {
                bt = t;
                bid = qid;
            }
        }
    }

    // spheres: the tile's pending rays grouped into up to kReflectBundles bundles (rtx_reflect.hpp), unless every sphere is tested.
    // Group g: the open ray of the lowest thread (its leader) and every open ray within 60 degrees of the leader's direction; the
    // last group takes whatever is left.  A tile that spans two or three mirrors (a room's corner) gets a narrow bundle per mirror
    // where one bundle over all of them would have a half-angle past 90 degrees and keep every sphere.  A sphere is listed when it
    // may meet any of the bundles; every ray belongs to one, so the list holds every sphere any of the tile's rays can hit.
    const float Pf[3] = {r2.o.x, r2.o.y, r2.o.z}, Rf[3] = {r2.d.x, r2.d.y, r2.d.z};
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
        lds_barrier(); // (also: s_cnt, and every read of the previous group's s_red is done)
        uint32_t lw = 0u;
        while (lw < 4u && s_lead_lane[lw] == 64u) lw++;
        if (lw == 4u) break; // no open ray left (uniform)
        const uint32_t lead_tid = lw * 64u + s_lead_lane[lw];
        const float lu[3] = {s_lead_u[lw][0], s_lead_u[lw][1], s_lead_u[lw][2]};
        const bool take_all = ra.brute != 0u || g == kReflectBundles - 1;
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
        const bool all = ra.brute != 0u || sum[7] > 0.0f || !rtxreflect::axis_from_sum(sum[3], sum[4], sum[5], sum[6], axis);
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
    const uint32_t ns = a.ns;
    if (nb != 0u && ns != 0u) {
        const bool wave_open = __ballot(pending) != 0ull;
        uint32_t listed = 0u; // candidates this workgroup kept after culling, over all fillings of the list
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
        if (tid < ns) g0 = a.sph_geom[tid];
        if ((uint32_t)kThreads + tid < ns) g1 = a.sph_geom[kThreads + tid];
        for (uint32_t base = 0; base < ns; base += (uint32_t)kChunk) {
            const float4 c0 = g0, c1 = g1;
            const uint32_t i0 = base + tid, i1 = base + (uint32_t)kThreads + tid;
            // the next step's loads go out before this step's tests
            if (i0 + (uint32_t)kChunk < ns) g0 = a.sph_geom[i0 + kChunk];
            if (i1 + (uint32_t)kChunk < ns) g1 = a.sph_geom[i1 + kChunk];
            bool k0 = false, k1 = false;
            for (uint32_t b = 0; b < nb; b++) {
                k0 = k0 || (i0 < ns && rtxreflect::may_hit(s_bundle[b], c0.x, c0.y, c0.z, c0.w));
                k1 = k1 || (i1 < ns && rtxreflect::may_hit(s_bundle[b], c1.x, c1.y, c1.z, c1.w));
            }
            const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
            const uint32_t n0 = (uint32_t)__popcll(m0), n1 = (uint32_t)__popcll(m1);
            uint32_t wbase = 0u;
            if (lane == 0u && n0 + n1 != 0u) wbase = atomicAdd(&s_cnt, n0 + n1);
            wbase = (uint32_t)__shfl((int)wbase, 0);
            if (k0) {
                const uint32_t p = wbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
                s_cand[p] = c0;
                s_cand_pos[p] = i0;
            }
            if (k1) {
                const uint32_t p = wbase + n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
                s_cand[p] = c1;
                s_cand_pos[p] = i1;
            }
            // the shadow pass's counter protocol: appends | barrier | every wave reads the count | barrier | (flush | barrier)
            lds_barrier(); // this step's appends are done
            const uint32_t cnt = __builtin_amdgcn_readfirstlane(s_cnt);
            lds_barrier(); // every wave has read the count
            if (cnt > (uint32_t)(kReflectList - kChunk) || base + (uint32_t)kChunk >= ns) {
                if (tid == 0u) s_cnt = 0u; // (nothing reads or appends to it before the barrier below)
                listed += cnt;
                if (wave_open) {
                    for (uint32_t j = 0; j < cnt; j++) {
                        const float4 sp = s_cand[j];
                        const uint32_t pos = s_cand_pos[j];
                        float t;
                        if (pending && pos != id && secondary_sphere_hit(r2, sp, t) && comes_before(a, t, pos, bt, bid)) {
                            bt = t;
                            bid = pos;
                        }
                    }
                }
                lds_barrier(); // every wave is done with the list, and the reset is visible
            }
        }
        if (ra.longest != nullptr && tid == 0u) atomicMax(ra.longest, listed);
    }

    if (pending) ra.hits2[(size_t)(row - a.row0) * a.W + col] = make_uint2(__float_as_uint(bt), bid);
}
