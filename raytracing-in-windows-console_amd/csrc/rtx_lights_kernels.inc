// rtx_lights_kernels.inc -- the shading launch for a set of several point lights (rtx_scene_set_lights), included into namespace
// rtx of rtx_kernels.hip after rtx_shadow_kernels.inc.  A set of one light keeps rtx_shadow_shade / rtx_reflect_shade; these
// kernels take a set of two or more (or any set under RTX_OPT_LIGHTS_CHECK 1).  The launches before them are the same: the trace
// kernel in its kOutHit form and, on the mirror path, rtx_reflect_hit, which does not know about lights.
//
// The colour of a visible pixel: res = 0.2f * od; for each light in the order given res = (res + diffuse_i * od) + specular_i * 1.0f;
// res * 255.0f, minf(255.0f, .) -- shade_light's expression (rtx_device.hpp) with the per-light terms summed, every operation
// rounded to fp32, and for one light shade_light's operation for operation.  What does not depend on the light (point, view
// direction, nn) is formed once.  A light the pixel is shadowed from enters with both powers 0.
//
// The shadow test is rtx_shadow_shade's, per light: self-shadow, the planes per pixel, then the spheres.  Every thread keeps a bit
// mask of the lights still open for its pixel.  Per light the workgroup reduces its open hit points to a cone from that light
// (rtx_shadow.hpp, unchanged); a light with no open pixel in the workgroup has no cone.  The sphere array is then walked ONCE for
// all lights: each staged sphere is tested against every live cone and, if kept for at least one light, appended once to the LDS
// list with the 8-bit mask of the lights it was kept for (rtx_shadow_shade's counter protocol and prefetch, unchanged).  At a
// flush every wave goes through the lights some lane of it is still open for; per light the segment (toL, 1 / len2) is formed once
// and the list entries whose mask names the light (four mask bytes a word) are tested by the lanes open for it.

struct LightsShared {
    float4 occ[kShadowList];
    uint32_t occ_pos[kShadowList];
    uint32_t occ_mask[kShadowList / 4]; // one byte per entry: the lights the sphere was kept for
    uint32_t digits[256];
    __attribute__((aligned(4))) uint8_t ramp[68];
    float red[4][6];
    rtxshadow::Cone cone[rtxlights::kMaxLights];
    uint32_t cnt;
};

// diffuse_i and specular_i of one light, as shade_light forms them; res = (res + diffuse_i * od) + specular_i * 1.0f
__device__ __forceinline__ void add_light(V3& res, V3 point, V3 nn, V3 nv, V3 od, const rtxlights::PackedLight& L, float dpow, float spow)
{
    V3 lightDir = sub(v3(L.px, L.py, L.pz), point);
    float dist = sqrt_cr(lightDir.x * lightDir.x + lightDir.y * lightDir.y + lightDir.z * lightDir.z);
    dist = dist * dist;
    const float divDistance = rcp_cr(dist);
    lightDir = normalize_gpu(lightDir);

    const float diffuseIntensity = clampf(dot(nn, lightDir), 0.0f, 1.0f);
    const V3 diffuse = v3(((L.dr * diffuseIntensity) * dpow) * divDistance, ((L.dg * diffuseIntensity) * dpow) * divDistance,
                          ((L.db * diffuseIntensity) * dpow) * divDistance);

    const V3 h = normalize_gpu(add(lightDir, nv));
    const float specularIntensity = pow32(clampf(dot(nn, h), 0.0f, 1.0f));
    const V3 specular = v3(((L.sr * specularIntensity) * spow) * divDistance, ((L.sg * specularIntensity) * spow) * divDistance,
                           ((L.sb * specularIntensity) * spow) * divDistance);

    res.x = (res.x + diffuse.x * od.x) + specular.x * 1.0f;
    res.y = (res.y + diffuse.y * od.y) + specular.y * 1.0f;
    res.z = (res.z + diffuse.z * od.z) + specular.z * 1.0f;
}

// shade_light over the set: bit i of `shadowed` puts light i in with both powers 0.
__device__ __forceinline__ V3 shade_lights(const Ray& r, float distance, V3 normal, V3 od, const rtxlights::Block& ls, uint32_t shadowed)
{
    const V3 point = add(r.o, mulf(r.d, distance));
    const V3 viewDir = normalize_gpu(mulf(r.d, -1.0f));
    const V3 nn = normalize_gpu(normal);
    const V3 nv = normalize_gpu(viewDir);
    V3 res = v3(0.2f * od.x, 0.2f * od.y, 0.2f * od.z);
    for (uint32_t i = 0; i < ls.n; i++) {
        const bool dark = ((shadowed >> i) & 1u) != 0u;
        add_light(res, point, nn, nv, od, ls.light[i], dark ? 0.0f : ls.light[i].dpow, dark ? 0.0f : ls.light[i].spow);
    }
    res = mulf(res, 255.0f);
    return v3(minf(255.0f, res.x), minf(255.0f, res.y), minf(255.0f, res.z));
}

// reflect_blend (rtx_reflect_kernels.inc) with the secondary hit shaded by every light at full powers.
__device__ __forceinline__ V3 lights_reflect_blend(const KArgs& a, const LightsArgs& la, const ReflectArgs& ra, const Ray& ray, float distance, V3 normal,
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
        cr = shade_lights(r2, t2, normalize_gpu(n0), od, la.lights, 0u);
    }
    const float w = 1.0f - k;
    return v3(minf(255.0f, cl.x * w + cr.x * k), minf(255.0f, cl.y * w + cr.y * k), minf(255.0f, cl.z * w + cr.z * k));
}

// (rtx_lights_chain_kernels.inc: the blend over a chain of up to RTX_MAX_REFLECT_DEPTH levels)
__device__ __forceinline__ V3 lights_chain_blend(const KArgs& a, const LightsArgs& la, const ReflectArgs& ra, const ChainArgs& ca, const Ray& ray,
                                                 float distance, V3 normal, uint32_t id, V3 cl, size_t at);

// REFLECT 0: no mirror; 1: one bounce (ra.hits2, lights_reflect_blend); 2: a chain (ca, lights_chain_blend).  What a value does
// not use is not compiled.
template <int MODE, int OUT, int REFLECT>
__device__ __forceinline__ void lights_shade_body(const KArgs& a, const LightsArgs& la, const ReflectArgs& ra, const ChainArgs& ca)
{
    __shared__ LightsShared s;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = tid >> 6;
    s.digits[tid] = digits_word(tid);
    if (tid < 17u) {
        reinterpret_cast<uint32_t*>(s.ramp)[tid] = reinterpret_cast<const uint32_t*>(kRamp)[tid];
    }
    if (tid == 0u) s.cnt = 0u;

    Camera cam;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        cam.m[i] = a.m[i];
    }
    cam.ox = a.ox; cam.oy = a.oy; cam.oz = a.oz;
    cam.e1 = a.e1; cam.e2 = a.e2; cam.far = a.far;
    cam.fW = a.fW; cam.fH = a.fH;

    const uint32_t col = blockIdx.x * (uint32_t)kShadowTile + (tid & (uint32_t)(kShadowTile - 1));
    const uint32_t row = a.row0 + blockIdx.y * (uint32_t)kShadowTile + tid / (uint32_t)kShadowTile;
    const bool in_frame = col < a.W && row < a.row_end;
    const bool newline_col = col + 1u == a.W;
    uint2 hit = make_uint2(__float_as_uint(kNoHit), 0xffffffffu);
    if (in_frame) hit = la.hits[(size_t)(row - a.row0) * a.W + col];

    // the ray, as the trace built it: RayTracing.cu:16-23 through the staged per-column / per-row terms
    const uint32_t c = col < a.W ? col : a.W - 1u;
    const uint32_t r = row < a.row_end ? row : a.row_end - 1u;
    const float vx = (((float)(2u * c) - cam.fW) / cam.fW) * cam.e1;
    const float vy = ((cam.fH - (float)(r * 2u)) / cam.fH) * cam.e2;
    const Ray ray = ray_from_tables(cam, make_float4(cam.m[0] * vx, cam.m[4] * vx, cam.m[8] * vx, 0.0f),
                                    make_float4(cam.m[1] * vy, cam.m[5] * vy, cam.m[9] * vy, 0.0f));

    // the winner's normal and colour, as the trace body derives them (RayTracing.cu:123-135, Sphere.cu:67)
    const uint32_t id = hit.y;
    const bool any_hit = in_frame && !newline_col && id != 0xffffffffu;
    float distance = kNoHit, shadingValue = 0.0f;
    V3 normal = ray.d, colour = ray.d, od = ray.d;
    if (any_hit) {
        distance = __uint_as_float(hit.x);
        V3 n0;
        if (id & 0x80000000u) {
            const uint32_t q = id & 0x7fffffffu;
            const float4 pb = a.pl_b[q], pd = a.pl_od[q];
            n0 = v3(pb.x, pb.y, pb.z);
            od = v3(pd.x, pd.y, pd.z);
        } else {
            const float4 g = a.sph_geom[id], d4 = a.sph_od[id];
            n0 = normalize_gpu(sub(add(ray.o, mulf(ray.d, distance)), v3(g.x, g.y, g.z)));
            od = v3(d4.x, d4.y, d4.z);
        }
        normal = normalize_gpu(n0);                                         // RayTracing.cu:129
        shadingValue = normal.x * 1.0f + normal.y * 0.0f + normal.z * 0.0f; // :133
    }

    // ---- the shadow test, per light: self-shadow and planes per pixel, and the workgroup's cone from that light
    const uint32_t nl = la.lights.n;
    const uint32_t ns = a.ns;
    const V3 P = add(ray.o, mulf(ray.d, distance)); // the point shade() lights
    const float Pf[3] = {P.x, P.y, P.z};
    const bool testable = la.test != 0u && any_hit && distance <= cam.far;
    const uint32_t own_plane = (id & 0x80000000u) ? (id & 0x7fffffffu) : 0xffffffffu;
    uint32_t open = 0u; // lights this pixel's segment is still to be tested for
    uint32_t dark = 0u; // lights this pixel is shadowed from
    uint32_t live = 0u; // lights with a cone: some pixel of the workgroup is open for them (workgroup-uniform)
    for (uint32_t i = 0; i < nl; i++) { // (every wave meets the same barriers: the trip count is the set's size)
        const rtxlights::PackedLight& Lt = la.lights.light[i];
        const V3 L = v3(Lt.px, Lt.py, Lt.pz);
        const V3 toL = sub(L, P);
        bool shadowed = false;
        bool pending = testable;
        if (pending && dot(normal, toL) <= 0.0f) {
            shadowed = true; // facing away from the light
            pending = false;
        }
        // planes: few, wave-uniform index (scalar loads)
        if (__ballot(pending) != 0ull) {
            for (uint32_t q = 0; q < a.np; q++) {
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
        if (shadowed) dark |= 1u << i;
        if (pending) open |= 1u << i;

        // the cone from this light over the workgroup's open hit points (rtx_shadow.hpp), as rtx_shadow_shade reduces it
        const float Lf[3] = {L.x, L.y, L.z};
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
            for (int k = 0; k < 6; k++) s.red[wave][k] = red[k];
        }
        lds_barrier(); // this light's reduction visible (the first time round: the tables and the count too)
        float sum[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < 4; w++) {
            sum[0] += s.red[w][0];
            sum[1] += s.red[w][1];
            sum[2] += s.red[w][2];
            sum[3] += s.red[w][3];
            sum[4] = fmaxf(sum[4], s.red[w][4]);
            sum[5] = fmaxf(sum[5], s.red[w][5]);
        }
        if (sum[3] > 0.0f && ns != 0u) { // (workgroup-uniform, as everything derived from the sums)
            float axis[3] = {0.0f, 0.0f, 0.0f};
            const bool all = la.brute != 0u || sum[5] > 0.0f || !rtxshadow::axis_from_sum(sum[0], sum[1], sum[2], sum[3], axis);
            float ang = 0.0f;
            if (!all) {
                ang = pending ? rtxshadow::angle_from_axis(axis, u) : 0.0f;
#pragma unroll
                for (int k = 32; k >= 1; k >>= 1) ang = fmaxf(ang, __shfl_xor(ang, k));
                lds_barrier(); // everyone has read the sums
                if (lane == 0u) s.red[wave][0] = ang;
                lds_barrier();
                ang = fmaxf(fmaxf(s.red[0][0], s.red[1][0]), fmaxf(s.red[2][0], s.red[3][0]));
            }
            if (tid == 0u) s.cone[i] = rtxshadow::make_cone(Lf, axis, ang, sum[4], all);
            live |= 1u << i;
        }
        lds_barrier(); // everyone is done with this light's sums before the next light's are written; the cone is visible
    }
    live = __builtin_amdgcn_readfirstlane(live);

    // ---- spheres: one walk of the scene for all lights
    if (live != 0u) {
        const uint32_t own_sphere = (id & 0x80000000u) ? 0xffffffffu : id;
        uint8_t* const occ_mask8 = reinterpret_cast<uint8_t*>(s.occ_mask);
        uint32_t listed = 0u; // list entries this workgroup kept after culling, over all fillings of the list
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
        if (tid < ns) g0 = a.sph_geom[tid];
        if ((uint32_t)kThreads + tid < ns) g1 = a.sph_geom[kThreads + tid];
        for (uint32_t base = 0; base < ns; base += (uint32_t)kChunk) {
            const float4 c0 = g0, c1 = g1;
            const uint32_t i0 = base + tid, i1 = base + (uint32_t)kThreads + tid;
            // the next step's loads go out before this step's tests
            if (i0 + (uint32_t)kChunk < ns) g0 = a.sph_geom[i0 + kChunk];
            if (i1 + (uint32_t)kChunk < ns) g1 = a.sph_geom[i1 + kChunk];
            uint32_t km0 = 0u, km1 = 0u; // the lights each of the two spheres may occlude
            for (uint32_t m = live; m != 0u; m &= m - 1u) {
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                const rtxshadow::Cone cone = s.cone[i];
                const float Lf[3] = {la.lights.light[i].px, la.lights.light[i].py, la.lights.light[i].pz};
                if (i0 < ns && rtxshadow::may_occlude(cone, Lf, c0.x, c0.y, c0.z, c0.w)) km0 |= 1u << i;
                if (i1 < ns && rtxshadow::may_occlude(cone, Lf, c1.x, c1.y, c1.z, c1.w)) km1 |= 1u << i;
            }
            const bool k0 = km0 != 0u, k1 = km1 != 0u;
            const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
            const uint32_t n0 = (uint32_t)__popcll(m0), n1 = (uint32_t)__popcll(m1);
            uint32_t wbase = 0u;
            if (lane == 0u && n0 + n1 != 0u) wbase = atomicAdd(&s.cnt, n0 + n1);
            wbase = (uint32_t)__shfl((int)wbase, 0);
            if (k0) {
                const uint32_t p = wbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
                s.occ[p] = c0;
                s.occ_pos[p] = i0;
                occ_mask8[p] = (uint8_t)km0;
            }
            if (k1) {
                const uint32_t p = wbase + n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
                s.occ[p] = c1;
                s.occ_pos[p] = i1;
                occ_mask8[p] = (uint8_t)km1;
            }
            // rtx_shadow_shade's counter protocol: appends | barrier | every wave reads the count | barrier | (flush | barrier)
            lds_barrier(); // this step's appends are done
            const uint32_t cnt = __builtin_amdgcn_readfirstlane(s.cnt);
            lds_barrier(); // every wave has read the count
            if (cnt > (uint32_t)(kShadowList - kChunk) || base + (uint32_t)kChunk >= ns) {
                if (tid == 0u) s.cnt = 0u; // (nothing reads or appends to it before the barrier below)
                listed += cnt;
                for (uint32_t m = live; m != 0u; m &= m - 1u) {
                    const uint32_t i = (uint32_t)__builtin_ctz(m), bit = 1u << i;
                    bool pending = (open & bit) != 0u;
                    if (__ballot(pending) == 0ull) continue; // no lane of this wave is open for the light
                    // exact test of this pixel's segment: the closest point of (P, L) to the centre, closer than r
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
                                const V3 wv = sub(v3(sp.x, sp.y, sp.z), P);
                                const float sc = dot(wv, toL) * inv_len2;
                                const float k = sc < 0.0f ? 0.0f : (sc > 1.0f ? 1.0f : sc);
                                const V3 e = sub(wv, mulf(toL, k));
                                if (dot(e, e) < sp.w * sp.w) {
                                    dark |= bit;
                                    pending = false;
                                }
                            }
                        }
                    }
                    if (!pending) open &= ~bit;
                }
                lds_barrier(); // every wave is done with the list, and the reset is visible
            }
        }
        if (la.longest != nullptr && tid == 0u) atomicMax(la.longest, listed);
    }

    // ---- shade with every light (both powers 0 for the lights the pixel is shadowed from) and encode
    if (any_hit) {
        colour = shade_lights(ray, distance, normal, od, la.lights, dark);
        if constexpr (REFLECT == 1) {
            if (distance <= cam.far) colour = lights_reflect_blend(a, la, ra, ray, distance, normal, id, colour, (size_t)(row - a.row0) * a.W + col);
        } else if constexpr (REFLECT == 2) {
            if (distance <= cam.far) colour = lights_chain_blend(a, la, ra, ca, ray, distance, normal, id, colour, (size_t)(row - a.row0) * a.W + col);
        }
    }
    encode_and_store<MODE, OUT>(a, cam, s.digits, s.ramp, in_frame, newline_col, row, col, distance, normal, colour, shadingValue);
}

template <int MODE, int OUT>
__global__ __launch_bounds__(kThreads) void rtx_lights_shade(const KArgs a, const LightsArgs la)
{
    const ReflectArgs ra = {}; // (read only by the REFLECT parts, which are not compiled here)
    const ChainArgs ca = {};
    lights_shade_body<MODE, OUT, 0>(a, la, ra, ca);
}

// The mirror path's third launch for a set of several lights: rtx_lights_shade's shading, then the blend.
template <int MODE, int OUT>
__global__ __launch_bounds__(kThreads) void rtx_lights_reflect_shade(const KArgs a, const LightsArgs la, const ReflectArgs ra)
{
    const ChainArgs ca = {}; // (read only by the chain's blend, which is not compiled here)
    lights_shade_body<MODE, OUT, 1>(a, la, ra, ca);
}
