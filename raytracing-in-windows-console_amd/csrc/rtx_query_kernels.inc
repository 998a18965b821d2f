// rtx_query_kernels.inc -- ray queries (rtx_query_rays, rtx_pick), included into namespace rtx of rtx_kernels.hip after
// rtx_tile_pass.inc, whose secondary_sphere_hit (and rtx_device.hpp's plane_hit) test every ray here: rays of the caller,
// each with its own origin, an unnormalised direction, a far limit tmax and a creation index to skip.
//
// One ray per lane, 256-thread workgroups; a ray is two 16-byte loads, a hit one 8-byte store.  Spheres are known by sphere index
// (the scene arrays in creation order), winners by creation index: the best so far is kept as (t, creation index) and a candidate
// replaces it when it comes first in that order, which is what comes_before decides from positions.
//
// rtx_query_brute: every ray against every plane and sphere, the spheres staged through LDS 512 a step.
// rtx_query_grid:  planes and the grid's large spheres per ray (wave-uniform index: scalar loads), then the cell walk of
// rtx_grid.hpp, testing each visited cell's list; a ray stops when its best t is below the parameter at which it leaves the cell
// just tested, when that parameter passes tmax, or when it leaves the grid.  Rays that cannot be walked are answered by the
// brute loop (and counted).  The lists hold every sphere a walkable ray can be reported to hit in that cell (rtx_grid.hpp), and a
// minimum does not depend on the order or the number of times its candidates are met, so both kernels give the same bytes.
//
// The build: rtx_grid_bounds (one workgroup: the spheres' box), the host's plan, rtx_grid_count (pairs per cell; large spheres
// flagged), rtx_grid_scan (one workgroup: exclusive offsets, the large list in index order), rtx_grid_scatter (sphere indices into
// the cells by atomic cursors, any order) and rtx_grid_sort (a wave per cell ranks its entries by sphere index and writes geometry
// and creation index in that order: two builds of one scene give one memory image).

constexpr uint32_t kQueryNone = 0xffffffffu; // RTX_NO_OBJECT
constexpr uint32_t kQuerySome = 0xfffffffeu; // RTX_SOME_OBJECT

__device__ __forceinline__ Ray query_ray(float4 ro, float4 rd)
{
    Ray r;
    r.o = v3(ro.x, ro.y, ro.z);
    r.d = v3(rd.x, rd.y, rd.z);
    r.a = dot(r.d, r.d);
    r.fourA = 4.0f * r.a;
    r.divTwoA = rcp_cr(2.0f * r.a); // as mirror_ray
    return r;
}

// (t, creation index) replaces the best so far when it is within tmax, not the skipped object and first in (t, creation index) order.
__device__ __forceinline__ void query_take(float t, uint32_t gidx, float tmax, uint32_t skip, float& bt, uint32_t& bid)
{
    if (t <= tmax && gidx != skip && (t < bt || (t == bt && gidx < bid))) {
        bt = t;
        bid = gidx;
    }
}

__device__ __forceinline__ void query_sphere(const Ray& r, float4 g, uint32_t gidx, float tmax, uint32_t skip, float& bt, uint32_t& bid)
{
    float t;
    if (secondary_sphere_hit(r, g, t)) query_take(t, gidx, tmax, skip, bt, bid);
}

__device__ __forceinline__ void query_planes(const QueryArgs& q, const Ray& r, bool live, float tmax, uint32_t skip, float& bt, uint32_t& bid)
{
    for (uint32_t k = 0; k < q.np; k++) {
        const float4 pa = q.pl_a[k], pb = q.pl_b[k];
        const uint32_t gidx = __float_as_uint(q.pl_od[k].w);
        float t;
        if (live && plane_hit(r, v3(pa.x, pa.y, pa.z), v3(pb.x, pb.y, pb.z), pa.w, pb.w, t)) query_take(t, gidx, tmax, skip, bt, bid);
    }
}

// Every sphere for the rays with `active`, 512 a step through LDS.  Called by all threads of the workgroup.
__device__ __forceinline__ void query_all_spheres(const QueryArgs& q, const Ray& r, bool active, float tmax, uint32_t skip, float& bt, uint32_t& bid,
                                                  float4* s_geom, uint32_t* s_gidx)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < q.ns; base += (uint32_t)kChunk) {
        const uint32_t i0 = base + tid, i1 = base + (uint32_t)kThreads + tid;
        if (i0 < q.ns) {
            s_geom[tid] = q.sph_geom[i0];
            s_gidx[tid] = __float_as_uint(q.sph_od[i0].w);
        }
        if (i1 < q.ns) {
            s_geom[kThreads + tid] = q.sph_geom[i1];
            s_gidx[kThreads + tid] = __float_as_uint(q.sph_od[i1].w);
        }
        __syncthreads();
        const uint32_t cnt = q.ns - base < (uint32_t)kChunk ? q.ns - base : (uint32_t)kChunk;
        if (q.any) active = active && bid == kQueryNone;
        if (__ballot(active) != 0ull) {
            for (uint32_t j = 0; j < cnt; j++) {
                if (active) query_sphere(r, s_geom[j], s_gidx[j], tmax, skip, bt, bid);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void query_store(const QueryArgs& q, uint32_t idx, float bt, uint32_t bid)
{
    if (q.any && bid != kQueryNone) {
        bt = 0.0f;
        bid = kQuerySome;
    }
    q.hits[idx] = make_uint2(__float_as_uint(bt), bid);
}

__global__ __launch_bounds__(kThreads) void rtx_query_brute(const QueryArgs q)
{
    __shared__ float4 s_geom[kChunk];
    __shared__ uint32_t s_gidx[kChunk];
    const uint32_t idx = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool valid = idx < q.n;
    const uint32_t at = valid ? idx : q.n - 1u;
    const float4 ro = q.rays[2u * at], rd = q.rays[2u * at + 1u];
    const Ray r = query_ray(ro, rd);
    const float tmax = ro.w;
    const uint32_t skip = __float_as_uint(rd.w);
    float bt = kNoHit;
    uint32_t bid = kQueryNone;
    query_planes(q, r, valid, tmax, skip, bt, bid);
    query_all_spheres(q, r, valid, tmax, skip, bt, bid, s_geom, s_gidx);
    if (valid) query_store(q, idx, bt, bid);
}

__global__ __launch_bounds__(kThreads) void rtx_query_grid(const QueryArgs q)
{
    __shared__ float4 s_geom[kChunk];
    __shared__ uint32_t s_gidx[kChunk];
    const uint32_t idx = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool valid = idx < q.n;
    const uint32_t at = valid ? idx : q.n - 1u;
    const float4 ro = q.rays[2u * at], rd = q.rays[2u * at + 1u];
    const Ray r = query_ray(ro, rd);
    const float tmax = ro.w;
    const uint32_t skip = __float_as_uint(rd.w);
    float bt = kNoHit;
    uint32_t bid = kQueryNone;
    const float o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
    const bool walk = rtxgrid::walkable(q.grid, o, r.a);
    const bool live = valid && tmax >= 0.0f; // a hit has 0 <= t <= tmax: nothing to find otherwise (NaN included)
    const bool fallback = valid && !walk;

    query_planes(q, r, live, tmax, skip, bt, bid);
    if (live && walk) {
        for (uint32_t j = 0; j < q.n_large; j++) {
            const uint32_t i = q.large[j];
            query_sphere(r, q.sph_geom[i], __float_as_uint(q.sph_od[i].w), tmax, skip, bt, bid);
        }
        rtxgrid::Walk w;
        bool go = !(q.any && bid != kQueryNone) && rtxgrid::walk_start(q.grid, o, d, tmax, w);
        while (go) {
            const uint32_t c = rtxgrid::cell_index(q.grid, w);
            const uint32_t b = q.cell_start[c], e = q.cell_start[c + 1u];
            for (uint32_t j = b; j < e; j++) {
                float t;
                // (the creation index is fetched only for a candidate that can take the lead)
                if (secondary_sphere_hit(r, q.list_geom[j], t) && t <= tmax && t <= bt) query_take(t, q.list_gidx[j], tmax, skip, bt, bid);
            }
            const float tout = rtxgrid::t_out(w);
            go = !(bt < tout) && tout <= tmax && !(q.any && bid != kQueryNone) && rtxgrid::walk_step(q.grid, w);
        }
    }
    // the rays the brute loop answers, counted: one that has nothing to find tests nothing, walkable or not, and is not among them
    const unsigned long long fb = __ballot(fallback && live);
    if (fb != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(q.fallback, (uint32_t)__popcll(fb));
    if (__syncthreads_or(fallback && live ? 1 : 0)) query_all_spheres(q, r, fallback && live, tmax, skip, bt, bid, s_geom, s_gidx);
    if (valid) query_store(q, idx, bt, bid);
}

// ---- the build
__global__ __launch_bounds__(kThreads) void rtx_grid_bounds(const GridBuildArgs b)
{
    __shared__ float s_red[4][7];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0u;
    for (uint32_t i = tid; i < b.ns; i += (uint32_t)kThreads) {
        const float4 g = b.sph_geom[i];
        const float r = fabsf(g.w);
        const float c[3] = {g.x, g.y, g.z};
        if (rtxgrid::finite_f(g.x) && rtxgrid::finite_f(g.y) && rtxgrid::finite_f(g.z) && rtxgrid::finite_f(r)) {
            nf++;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                lo[k] = fminf(lo[k], c[k] - r);
                hi[k] = fmaxf(hi[k], c[k] + r);
            }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], s));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], s));
        }
        nf += (uint32_t)__shfl_xor((int)nf, s);
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            s_red[wave][k] = lo[k];
            s_red[wave][3 + k] = hi[k];
        }
        s_red[wave][6] = __uint_as_float(nf);
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t total = 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            b.bounds[k] = fminf(fminf(s_red[0][k], s_red[1][k]), fminf(s_red[2][k], s_red[3][k]));
            b.bounds[3 + k] = fmaxf(fmaxf(s_red[0][3 + k], s_red[1][3 + k]), fmaxf(s_red[2][3 + k], s_red[3][3 + k]));
        }
        for (int w = 0; w < 4; w++) total += __float_as_uint(s_red[w][6]);
        b.bounds[6] = __uint_as_float(total);
    }
}

__global__ __launch_bounds__(kThreads) void rtx_grid_count(const GridBuildArgs b)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= b.ns) return;
    int i0[3], i1[3];
    const bool small = rtxgrid::sphere_cells(b.grid, b.sph_geom[i].x, b.sph_geom[i].y, b.sph_geom[i].z, b.sph_geom[i].w, i0, i1);
    b.is_large[i] = small ? 0 : 1;
    if (!small) return;
    for (int z = i0[2]; z <= i1[2]; z++) {
        for (int y = i0[1]; y <= i1[1]; y++) {
            for (int x = i0[0]; x <= i1[0]; x++) {
                atomicAdd(&b.cell_count[((uint32_t)z * b.grid.n[1] + (uint32_t)y) * b.grid.n[0] + (uint32_t)x], 1u);
            }
        }
    }
}

// Exclusive sum of `v` over the workgroup (kScanThreads threads), the total in `total`.
constexpr int kScanThreads = 1024;
__device__ __forceinline__ uint32_t grid_block_scan(uint32_t v, uint32_t* s_wave, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, s);
        if (lane >= (uint32_t)s) inc += up;
    }
    __syncthreads(); // (the previous round's reads of s_wave are done)
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t w = 0; w < (uint32_t)(kScanThreads / 64); w++) {
        const uint32_t x = s_wave[w];
        if (w < wave) before += x;
        all += x;
    }
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kScanThreads) void rtx_grid_scan(const GridBuildArgs b)
{
    __shared__ uint32_t s_wave[kScanThreads / 64];
    const uint32_t tid = threadIdx.x;
    // cell counts -> exclusive offsets: every thread owns a run of consecutive cells
    const uint32_t per = (b.n_cells + (uint32_t)kScanThreads - 1u) / (uint32_t)kScanThreads;
    const uint32_t c0 = tid * per < b.n_cells ? tid * per : b.n_cells;
    const uint32_t c1 = c0 + per < b.n_cells ? c0 + per : b.n_cells;
    uint32_t sum = 0u;
    for (uint32_t c = c0; c < c1; c++) sum += b.cell_count[c];
    uint32_t pairs;
    uint32_t run = grid_block_scan(sum, s_wave, pairs);
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t v = b.cell_count[c];
        b.cell_count[c] = run;
        run += v;
    }
    if (tid == 0u) {
        b.cell_count[b.n_cells] = pairs;
        b.totals[0] = pairs;
    }
    // large flags -> the large list, in sphere index order
    const uint32_t pers = (b.ns + (uint32_t)kScanThreads - 1u) / (uint32_t)kScanThreads;
    const uint32_t s0 = tid * pers < b.ns ? tid * pers : b.ns;
    const uint32_t s1 = s0 + pers < b.ns ? s0 + pers : b.ns;
    uint32_t nl = 0u;
    for (uint32_t i = s0; i < s1; i++) nl += b.is_large[i];
    uint32_t larges;
    uint32_t at = grid_block_scan(nl, s_wave, larges);
    for (uint32_t i = s0; i < s1; i++) {
        if (b.is_large[i]) {
            if (at < rtxgrid::kLargeCap) b.large[at] = i;
            at++;
        }
    }
    if (tid == 0u) b.totals[1] = larges;
}

__global__ __launch_bounds__(kThreads) void rtx_grid_scatter(const GridBuildArgs b)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= b.ns || b.is_large[i]) return;
    int i0[3], i1[3];
    rtxgrid::sphere_cells(b.grid, b.sph_geom[i].x, b.sph_geom[i].y, b.sph_geom[i].z, b.sph_geom[i].w, i0, i1);
    for (int z = i0[2]; z <= i1[2]; z++) {
        for (int y = i0[1]; y <= i1[1]; y++) {
            for (int x = i0[0]; x <= i1[0]; x++) {
                const uint32_t c = ((uint32_t)z * b.grid.n[1] + (uint32_t)y) * b.grid.n[0] + (uint32_t)x;
                // (the slot is below the next cell's offset: count gave this cell one slot per sphere that reaches it)
                b.pair_tmp[b.cell_count[c] + atomicAdd(&b.cell_fill[c], 1u)] = i;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void rtx_grid_sort(const GridBuildArgs b)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (uint32_t)(kThreads / 64);
    for (uint32_t c = blockIdx.x * (uint32_t)(kThreads / 64) + (threadIdx.x >> 6); c < b.n_cells; c += waves) {
        const uint32_t lo = b.cell_count[c], hi = b.cell_count[c + 1u];
        for (uint32_t e = lo + lane; e < hi; e += 64u) {
            const uint32_t i = b.pair_tmp[e];
            uint32_t rank = 0u;
            for (uint32_t j = lo; j < hi; j++) rank += b.pair_tmp[j] < i ? 1u : 0u; // (a sphere is in a cell once: indices differ)
            b.list_geom[lo + rank] = b.sph_geom[i];
            b.list_gidx[lo + rank] = __float_as_uint(b.sph_od[i].w);
        }
    }
}

// rtx_pick's ray: the primary ray of cell (col, row) exactly as the trace kernels form it, far limit the camera's.
__global__ void rtx_pick_ray(const KArgs a, uint32_t col, uint32_t row, float4* out)
{
    Camera cam;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        cam.m[i] = a.m[i];
    }
    cam.ox = a.ox; cam.oy = a.oy; cam.oz = a.oz;
    cam.e1 = a.e1; cam.e2 = a.e2; cam.far = a.far;
    cam.fW = a.fW; cam.fH = a.fH;
    const float vx = (((float)(2u * col) - cam.fW) / cam.fW) * cam.e1;
    const float vy = ((cam.fH - (float)(row * 2u)) / cam.fH) * cam.e2;
    const Ray ray = ray_from_tables(cam, make_float4(cam.m[0] * vx, cam.m[4] * vx, cam.m[8] * vx, 0.0f),
                                    make_float4(cam.m[1] * vy, cam.m[5] * vy, cam.m[9] * vy, 0.0f));
    out[0] = make_float4(ray.o.x, ray.o.y, ray.o.z, cam.far);
    out[1] = make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(kQueryNone));
}
