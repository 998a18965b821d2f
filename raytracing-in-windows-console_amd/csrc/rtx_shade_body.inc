// rtx_shade_body.inc -- the body of rtx_shadow_shade and rtx_reflect_shade (rtx_shadow_kernels.inc), included into both.  With
// REFLECT (the mirror path's third launch) each reflective pixel's secondary hit (ra.hits2) is shaded and blended into the colour
// before it is encoded (reflect_blend, rtx_reflect_kernels.inc); without, nothing of it is compiled.
    __shared__ float4 s_occ[kShadowList];
    __shared__ uint32_t s_occ_pos[kShadowList];
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
    if (tid == 0u) s_cnt = 0u;

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
    if (in_frame) hit = sa.hits[(size_t)(row - a.row0) * a.W + col];

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

    // ---- the shadow test
    const V3 L = v3(sa.light.px, sa.light.py, sa.light.pz);
    const V3 P = add(ray.o, mulf(ray.d, distance)); // the point shade() lights
    const V3 toL = sub(L, P);
    bool shadowed = false;
    bool pending = sa.test != 0u && any_hit && distance <= cam.far;
    if (pending && dot(normal, toL) <= 0.0f) {
        shadowed = true; // facing away from the light
        pending = false;
    }
    // planes: few, wave-uniform index (scalar loads)
    const uint32_t own_plane = (id & 0x80000000u) ? (id & 0x7fffffffu) : 0xffffffffu;
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

    // spheres: the workgroup's cone from the light over its open hit points (rtx_shadow.hpp), unless every sphere is tested
    const float Lf[3] = {L.x, L.y, L.z};
    float u[3] = {0.0f, 0.0f, 0.0f}, dist = 0.0f;
    bool degenerate = false;
    const float Pf[3] = {P.x, P.y, P.z};
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
    lds_barrier(); // tables, s_cnt and the first reduction visible
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
    const bool any_open = sum[3] > 0.0f; // (workgroup-uniform, as everything derived from the sums)
    const uint32_t ns = a.ns;
    if (!any_open || ns == 0u) {
        // nothing to walk
    } else {
        rtxshadow::Cone cone;
        float axis[3] = {0.0f, 0.0f, 0.0f};
        bool all = sa.brute != 0u || sum[5] > 0.0f || !rtxshadow::axis_from_sum(sum[0], sum[1], sum[2], sum[3], axis);
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

        // exact test of this pixel's segment: the closest point of (P, L) to the centre, closer than r
        const float len2 = dot(toL, toL);
        const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
        const uint32_t own_sphere = (id & 0x80000000u) ? 0xffffffffu : id;
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
            const bool k0 = i0 < ns && rtxshadow::may_occlude(cone, Lf, c0.x, c0.y, c0.z, c0.w);
            const bool k1 = i1 < ns && rtxshadow::may_occlude(cone, Lf, c1.x, c1.y, c1.z, c1.w);
            const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
            const uint32_t n0 = (uint32_t)__popcll(m0), n1 = (uint32_t)__popcll(m1);
            uint32_t wbase = 0u;
            if (lane == 0u && n0 + n1 != 0u) wbase = atomicAdd(&s_cnt, n0 + n1);
            wbase = (uint32_t)__shfl((int)wbase, 0);
            if (k0) {
                const uint32_t p = wbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
                s_occ[p] = c0;
                s_occ_pos[p] = i0;
            }
            if (k1) {
                const uint32_t p = wbase + n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
                s_occ[p] = c1;
                s_occ_pos[p] = i1;
            }
            // The counter protocol, one step: appends (LDS atomics) | barrier | every wave reads the count | barrier | (flush: reset
            // the count, test the list | barrier).  The second barrier is what keeps it race-free: no wave appends the next step's
            // survivors, or resets the count, before every wave has read this step's count, so all waves see the same count, take
            // the same branch and meet the same barriers; and the count can only reach kShadowList - kChunk + kChunk before a flush.
            lds_barrier(); // this step's appends are done
            const uint32_t cnt = __builtin_amdgcn_readfirstlane(s_cnt);
            lds_barrier(); // every wave has read the count
            if (cnt > (uint32_t)(kShadowList - kChunk) || base + (uint32_t)kChunk >= ns) {
                if (tid == 0u) s_cnt = 0u; // (nothing reads or appends to it before the barrier below)
                listed += cnt;
                for (uint32_t j = 0; j < cnt && __ballot(pending) != 0ull; j++) {
                    const float4 sp = s_occ[j];
                    if (pending && s_occ_pos[j] != own_sphere) {
                        const V3 w = sub(v3(sp.x, sp.y, sp.z), P);
                        const float s = dot(w, toL) * inv_len2;
                        const float k = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
                        const V3 e = sub(w, mulf(toL, k));
                        if (dot(e, e) < sp.w * sp.w) {
                            shadowed = true;
                            pending = false;
                        }
                    }
                }
                lds_barrier(); // every wave is done with the list, and the reset is visible
            }
        }
        if (sa.longest != nullptr && tid == 0u) atomicMax(sa.longest, listed);
    }

    // ---- shade with the light (both powers 0 in shadow) and encode
    if (any_hit) {
        colour = shade_light(ray, distance, normal, od, sa.light, shadowed ? 0.0f : sa.light.dpow, shadowed ? 0.0f : sa.light.spow);
        if constexpr (REFLECT) {
            if (distance <= cam.far) colour = reflect_blend(a, sa, ra, ray, distance, normal, id, colour, (size_t)(row - a.row0) * a.W + col);
        }
    }
    encode_and_store<MODE, OUT>(a, cam, s_digits, s_ramp, in_frame, newline_col, row, col, distance, normal, colour, shadingValue);
