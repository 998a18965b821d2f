// rtx_reflect_chain_kernels.inc -- the mirror path's second launch when mirrors see mirrors (RTX_OPT_REFLECT_DEPTH > 1, or
// RTX_OPT_REFLECT_DEPTH_CHECK 1), included into namespace rtx of rtx_kernels.hip after rtx_reflect_kernels.inc, whose device
// functions (mirror_ray, secondary_sphere_hit, comes_before, reflectivity_of) it shares.  rtx_reflect_hit itself is untouched.
//
// Level 0 is the primary ray and its hit.  Level j + 1 exists for a pixel iff j + 1 <= depth, level j hit an object o_j and
// k(o_j) > 0; its ray is mirror_ray(r_j, t_j, normal_j) with normal_j = normalize_gpu of o_j's normal at the hit (sphere:
// normalize_gpu(normalize_gpu(P - C)), plane: normalize_gpu(n)), tested against every object but o_j with the reference's tests and
// no far limit, winner the lexicographic minimum of (t, creation index).  Level j's hits go to ra.hits + j * ca.px.
//
// rtx_reflect_chain: ONE launch for all levels -- rtx_reflect_hit's tile (16 x 16), bundles, 512-sphere walk and counter protocol,
// wrapped in a level loop.  Every thread keeps its current ray, the object it left and whether it is still pending in registers;
// after a level's store the lanes whose winner reflects form the next ray.  The trip count is workgroup-uniform: at the head of a
// level every wave adds its pending lanes to an LDS counter of that level, which is read behind the bundle loop's first barrier
// (always met), so all waves see the same count and meet the same barriers; a tile with no pending lane leaves the loop.  A chain
// pixel's levels that were not traced get the no-hit pair; pixels without a chain are never written (nor read past level 0).
// No step depends on the order of the LDS list, so culled equals brute (RTX_OPT_REFLECT_CHECK 1) at every level.

// normalize_gpu of the normal of object `id` at point P of its surface, as reflect_blend forms it for a secondary hit.
__device__ __forceinline__ V3 chain_normal(const KArgs& a, uint32_t id, V3 P)
{
    V3 n0;
    if (id & 0x80000000u) {
        const float4 pb = a.pl_b[id & 0x7fffffffu];
        n0 = v3(pb.x, pb.y, pb.z);
    } else {
        const float4 g = a.sph_geom[id];
        n0 = normalize_gpu(sub(P, v3(g.x, g.y, g.z)));
    }
    return normalize_gpu(n0); // RayTracing.cu:129
}

// (6 waves per SIMD asked for: without the hint the loop-carried ray costs an 81st VGPR and a whole wave -- 5; 80 VGPRs with it, no
// scratch.  7, rtx_reflect_hit's and what 20.8 KB of LDS allow, spills 10 VGPRs to scratch and is not taken.)
__global__ __launch_bounds__(kThreads, 6) void rtx_reflect_chain(const KArgs a, const ReflectArgs ra, const ChainArgs ca)
{
    __shared__ float4 s_cand[kReflectList];
    __shared__ uint32_t s_cand_pos[kReflectList];
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
    const size_t at = in_frame ? (size_t)(row - a.row0) * a.W + col : 0u;
    uint2 hit = make_uint2(__float_as_uint(kNoHit), 0xffffffffu);
    if (in_frame) hit = ra.hits[at];

    // level 0: the primary ray, its winner's normal and the reflectivity, as rtx_reflect_hit rebuilds them
    const uint32_t c = col < a.W ? col : a.W - 1u;
    const uint32_t r = row < a.row_end ? row : a.row_end - 1u;
    const float vx = (((float)(2u * c) - cam.fW) / cam.fW) * cam.e1;
    const float vy = ((cam.fH - (float)(r * 2u)) / cam.fH) * cam.e2;
    const Ray ray = ray_from_tables(cam, make_float4(cam.m[0] * vx, cam.m[4] * vx, cam.m[8] * vx, 0.0f),
                                    make_float4(cam.m[1] * vy, cam.m[5] * vy, cam.m[9] * vy, 0.0f));
    bool pending = in_frame && !newline_col && hit.y != 0xffffffffu && __uint_as_float(hit.x) <= cam.far;
    if (pending) pending = reflectivity_of(ra, hit.y) > 0.0f;
    const bool chain = pending; // the pixel has a chain: every level up to the depth gets an entry
    V3 normal = ray.d;
    if (pending) normal = chain_normal(a, hit.y, add(ray.o, mulf(ray.d, __uint_as_float(hit.x))));
    Ray cur = mirror_ray(ray, pending ? __uint_as_float(hit.x) : 0.0f, normal); // the ray of the level being traced
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

        // planes: few, wave-uniform index (scalar loads)
        if (__ballot(pending) != 0ull) {
            for (uint32_t q = 0; q < a.np; q++) {
                const float4 pa = a.pl_a[q], pb = a.pl_b[q];
                float t;
                const uint32_t qid = 0x80000000u | q;
                if (pending && qid != id && plane_hit(cur, v3(pa.x, pa.y, pa.z), v3(pb.x, pb.y, pb.z), pa.w, pb.w, t) && comes_before(a, t, qid, bt, bid)) {
                    bt = t;
                    bid = qid;
                }
            }
        }

        // spheres: the tile's pending rays of this level grouped into up to kReflectBundles bundles, as rtx_reflect_hit groups them
        const float Pf[3] = {cur.o.x, cur.o.y, cur.o.z}, Rf[3] = {cur.d.x, cur.d.y, cur.d.z};
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
            lds_barrier(); // (also: this level's s_pend, and every read of the previous group's s_red is done)
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

        // every wave's count of this level was added before the first barrier above: the same number for all waves
        const uint32_t n_pending = __builtin_amdgcn_readfirstlane(s_pend[level - 1u]);
        if (n_pending == 0u) break; // nothing of the tile goes this deep (uniform)
        if (ca.rays != nullptr && tid == 0u) atomicAdd(&ca.rays[level - 1u], n_pending);

        if (nb != 0u && ns != 0u) {
            const bool wave_open = __ballot(pending) != 0ull;
            uint32_t listed = 0u; // candidates this workgroup kept after culling at this level, over all fillings of the list
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
                            if (pending && pos != id && secondary_sphere_hit(cur, sp, t) && comes_before(a, t, pos, bt, bid)) {
                                bt = t;
                                bid = pos;
                            }
                        }
                    }
                    lds_barrier(); // every wave is done with the list, and the reset is visible
                }
            }
            if (ra.longest != nullptr && tid == 0u) atomicMax(ra.longest, listed); // (the maximum over the levels)
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
            if (next) n = chain_normal(a, bid, add(cur.o, mulf(cur.d, bt)));
            cur = mirror_ray(cur, next ? bt : 0.0f, n);
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
