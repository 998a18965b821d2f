// grid_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests/test_gpu_grid_check.py).
// Runs the world grid's device code -- the five build kernels and the two query kernels of rtx_query_kernels.inc, walk_start /
// walk_step of rtx_grid.hpp, grid_segment_dark of rtx_grid_segment.inc: the very text rtx_kernels.hip compiles -- on scenes, rays and
// segments of the caller's making, with the launch shapes of rtx_k_launch_grid_build / rtx_k_launch_query and the order of
// rtx_query.cpp's fill_grid, and hands back what the device held: the bounds words, the plan, the offsets, the lists, the large
// list, every cell a walk visited with its interval.  Beside them the same header evaluated on the host side of this file (same
// flags), and the production exact tests (secondary_sphere_hit, segment_hits_sphere) for every (ray, sphere) pair.
//
// A build is kept -- the device's lists on the device, the host's in memory -- until the next one of its kind; walk, query and
// segments use the latest.  Nothing is shared with librtx_hip.so.  Every entry point returns 0, -1 on a HIP error, -2 on arguments
// it refuses (nothing is launched).
//
// head: 26 words.  [0..6] the bounds words (lo xyz, hi xyz, finite count), [7..21] the Grid (lo, cs, n, ctr, reach, margin, ok),
// [22] n_cells, [23] pairs, [24] large spheres (all of them, also past kLargeCap), [25] stage: 0 no usable grid (nothing behind
// the plan ran), 1 more than kLargeCap large spheres (count and scan ran: offsets, flags and the large list, no lists), 2 complete.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_cull.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_reflect.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_shadow.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_workgroup.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace rtx {
#include "../../raytracing-in-windows-console_amd/csrc/rtx_tile_pass.inc"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_grid_segment.inc"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_query_kernels.inc"
} // namespace rtx

namespace {

using namespace rtx;
using rtxgrid::Grid;

constexpr uint32_t kCanary = 0xC0FFEE11u, kNoT = 0xffffffffu;
constexpr uint32_t kMaxSpheres = 1u << 16, kMaxRays = 1u << 20, kMaxCap = 4096u, kMaxMatrix = 1u << 25;
constexpr uint32_t kMaxSteps = 3u * rtxgrid::kMaxAxis + 8u; // a walk moves one index by one a step and never back

// ---- the walk, for host and device: walkable, started, steps, and the first `cap` cells with their intervals
__host__ __device__ inline void walk_one(const Grid& g, const float* ray, uint32_t cap, uint32_t* flags, uint32_t* rec)
{
    const float o[3] = {ray[0], ray[1], ray[2]}, d[3] = {ray[4], ray[5], ray[6]};
    const float tmax = ray[3];
    const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]; // (as dot(): (x x + y y) + z z)
    const bool walkable = rtxgrid::walkable(g, o, a);
    bool started = false;
    uint32_t steps = 0;
    if (walkable) {
        rtxgrid::Walk w;
        bool go = started = rtxgrid::walk_start(g, o, d, tmax, w);
        while (go && steps < kMaxSteps) {
            const float tout = rtxgrid::t_out(w);
            if (steps < cap) {
                // (recorded with the sign of a zero dropped: fminf may return either of +0 and -0, host and device choose
                // differently, and no comparison of the walk or of its callers tells the two apart)
                const float tin_rec = w.t_in + 0.0f, tout_rec = tout + 0.0f;
                uint32_t tin_bits, tout_bits;
                memcpy(&tin_bits, &tin_rec, 4);
                memcpy(&tout_bits, &tout_rec, 4);
                rec[3u * steps] = rtxgrid::cell_index(g, w);
                rec[3u * steps + 1u] = tin_bits;
                rec[3u * steps + 2u] = tout_bits;
            }
            steps++;
            go = tout <= tmax && rtxgrid::walk_step(g, w);
        }
    }
    flags[0] = walkable ? 1u : 0u;
    flags[1] = started ? 1u : 0u;
    flags[2] = steps;
}

__global__ __launch_bounds__(kThreads) void k_walk(Grid g, const float* rays, uint32_t n, uint32_t cap, uint32_t* flags, uint32_t* rec)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= n) return;
    walk_one(g, rays + 8u * (size_t)i, cap, flags + 3u * (size_t)i, rec + 3u * (size_t)cap * i);
}

// secondary_sphere_hit of every (ray, sphere): t bits, kNoT where nothing is reported or the reported t is NaN (which no comparison takes)
__global__ __launch_bounds__(kThreads) void k_ray_matrix(const float4* rays, uint32_t n, const float4* geom, uint32_t ns, uint32_t* out)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)n * ns) return;
    const uint32_t p = (uint32_t)(i / ns), j = (uint32_t)(i % ns);
    const Ray r = query_ray(rays[2u * p], rays[2u * p + 1u]);
    float t = 0.0f;
    const bool hit = secondary_sphere_hit(r, geom[j], t) && t == t;
    out[i] = hit ? __float_as_uint(t) : kNoT;
}

// grid_segment_dark beside a loop over every sphere; the exact test's matrix (own sphere included)
__global__ __launch_bounds__(kThreads) void k_segments(KArgs a, GridShadowArgs gs, const float* P, const float* L, const uint32_t* own, uint32_t n, uint8_t* dark_grid,
                                                       uint8_t* dark_brute, uint8_t* matrix)
{
    const uint32_t idx = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool valid = idx < n;
    const uint32_t at = valid ? idx : n - 1u;
    const V3 p = v3(P[3u * at], P[3u * at + 1u], P[3u * at + 2u]);
    const V3 toL = sub(v3(L[3u * at], L[3u * at + 1u], L[3u * at + 2u]), p);
    const uint32_t own_gidx = own[2u * at], own_pos = own[2u * at + 1u];
    uint32_t n_fallback = 0u;
    const bool dark = grid_segment_dark(a, gs, p, toL, own_gidx, own_pos, valid, n_fallback);
    if (n_fallback != 0u) atomicAdd(gs.fallback, n_fallback);
    if (!valid) return;
    const float len2 = dot(toL, toL);
    const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
    bool brute = false;
    for (uint32_t j = 0; j < a.ns; j++) {
        const bool hit = segment_hits_sphere(p, toL, inv_len2, a.sph_geom[j]);
        if (matrix != nullptr) matrix[(size_t)idx * a.ns + j] = hit ? 1u : 0u;
        brute = brute || (hit && j != own_pos);
    }
    dark_grid[idx] = dark ? 1u : 0u;
    dark_brute[idx] = brute ? 1u : 0u;
}

// ---- a build, as the host keeps it
struct Built {
    bool have = false;
    uint32_t ns = 0, stage = 0;
    uint32_t bounds[7] = {};
    Grid g = {};
    uint32_t n_cells = 0, pairs = 0, n_large = 0;
    std::vector<uint32_t> cell_start, list_gidx;
    std::vector<float4> list_geom;
    std::vector<uint8_t> is_large;
    uint32_t large[rtxgrid::kLargeCap + 1] = {};
};

// ... and what the device build leaves on the device for query and segments
struct DeviceLists {
    std::vector<void*> held;
    float4 *sph_geom = nullptr, *sph_od = nullptr, *list_geom = nullptr;
    uint32_t *cell_count = nullptr, *list_gidx = nullptr, *large = nullptr;
    void release()
    {
        for (void* d : held) hipFree(d);
        held.clear();
        sph_geom = sph_od = list_geom = nullptr;
        cell_count = list_gidx = large = nullptr;
    }
    template <class T>
    bool get(T*& p, size_t count)
    {
        void* d = nullptr;
        if (hipMalloc(&d, (count ? count : 1) * sizeof(T)) != hipSuccess) return false;
        held.push_back(d);
        p = (T*)d;
        return true;
    }
};

Built g_host, g_dev;
DeviceLists g_lists;

// Temporary device memory of one call.
struct Scratch {
    std::vector<void*> held;
    bool ok = true;
    template <class T>
    T* get(size_t count, const void* src = nullptr, int fill = 0)
    {
        void* d = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        ok = ok && hipMalloc(&d, bytes) == hipSuccess;
        if (!ok) return nullptr;
        held.push_back(d);
        ok = (src != nullptr ? hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(d, fill, bytes)) == hipSuccess;
        return (T*)d;
    }
    bool ran() { return ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }
    bool down(void* dst, const void* d, size_t bytes) { return ok = ok && (dst == nullptr || bytes == 0 || hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess); }
    ~Scratch()
    {
        for (void* d : held) hipFree(d);
    }
};

void plan_of(Built& b, float load)
{
    float box[7];
    memcpy(box, b.bounds, sizeof box);
    b.g = rtxgrid::plan_grid(box, box + 3, b.bounds[6], load);
    b.n_cells = b.g.ok ? b.g.n[0] * b.g.n[1] * b.g.n[2] : 0u;
}

// The build on the device: rtx_query.cpp's fill_grid, launch for launch (rtx_k_launch_grid_build's shapes).
int build_device(const float4* geom, const float4* od, uint32_t ns, float load)
{
    Built& b = g_dev;
    b = Built();
    g_lists.release();
    b.ns = ns;
    b.large[rtxgrid::kLargeCap] = kCanary;
    DeviceLists& dl = g_lists;
    uint32_t* d_words = nullptr;
    uint8_t* d_is_large = nullptr;
    if (!dl.get(dl.sph_geom, ns) || !dl.get(dl.sph_od, ns) || !dl.get(dl.large, rtxgrid::kLargeCap + 1) || !dl.get(d_words, 16) || !dl.get(d_is_large, ns)) return -1;
    if (hipMemcpy(dl.sph_geom, geom, (size_t)ns * 16, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dl.sph_od, od, (size_t)ns * 16, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dl.large, b.large, sizeof b.large, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_words, 0, 64) != hipSuccess) {
        return -1;
    }
    GridBuildArgs a;
    memset(&a, 0, sizeof a);
    a.sph_geom = dl.sph_geom;
    a.sph_od = dl.sph_od;
    a.ns = ns;
    a.bounds = (float*)(d_words + 4);
    a.totals = d_words;
    a.large = dl.large;
    const dim3 per_sphere((ns + (uint32_t)kThreads - 1u) / (uint32_t)kThreads), block(kThreads);
    hipLaunchKernelGGL(rtx_grid_bounds, dim3(1), block, 0, 0, a);
    if (hipGetLastError() != hipSuccess || hipMemcpy(b.bounds, a.bounds, sizeof b.bounds, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    plan_of(b, load);
    b.have = true;
    if (!b.g.ok) return 0;
    uint32_t* d_fill = nullptr;
    if (!dl.get(dl.cell_count, (size_t)b.n_cells + 1) || !dl.get(d_fill, b.n_cells)) return -1;
    if (hipMemset(dl.cell_count, 0, ((size_t)b.n_cells + 1) * 4) != hipSuccess || hipMemset(d_fill, 0, (size_t)b.n_cells * 4) != hipSuccess) return -1;
    a.grid = b.g;
    a.n_cells = b.n_cells;
    a.cell_count = dl.cell_count;
    a.cell_fill = d_fill;
    a.is_large = d_is_large;
    hipLaunchKernelGGL(rtx_grid_count, per_sphere, block, 0, 0, a);
    hipLaunchKernelGGL(rtx_grid_scan, dim3(1), dim3(kScanThreads), 0, 0, a);
    uint32_t totals[2] = {0u, 0u};
    if (hipGetLastError() != hipSuccess || hipMemcpy(totals, d_words, sizeof totals, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    b.pairs = totals[0];
    b.n_large = totals[1];
    b.stage = 1;
    b.cell_start.resize((size_t)b.n_cells + 1);
    b.is_large.resize(ns);
    if (hipMemcpy(b.cell_start.data(), dl.cell_count, b.cell_start.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(b.is_large.data(), d_is_large, ns, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(b.large, dl.large, sizeof b.large, hipMemcpyDeviceToHost) != hipSuccess) {
        return -1;
    }
    if (b.n_large > rtxgrid::kLargeCap) return 0;
    // (the offsets' last word bounds every slot scatter and sort write: they are sized by it, as fill_grid sizes them)
    if (b.cell_start[b.n_cells] != b.pairs) return -1;
    uint32_t* d_pair_tmp = nullptr;
    if (!dl.get(d_pair_tmp, b.pairs) || !dl.get(dl.list_geom, b.pairs) || !dl.get(dl.list_gidx, b.pairs)) return -1;
    a.pair_tmp = d_pair_tmp;
    a.list_geom = dl.list_geom;
    a.list_gidx = dl.list_gidx;
    hipLaunchKernelGGL(rtx_grid_scatter, per_sphere, block, 0, 0, a);
    uint32_t blocks = (b.n_cells + 3u) / 4u;
    if (blocks > 4096u) blocks = 4096u;
    hipLaunchKernelGGL(rtx_grid_sort, dim3(blocks), block, 0, 0, a);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    b.list_geom.resize(b.pairs);
    b.list_gidx.resize(b.pairs);
    if (b.pairs != 0u && (hipMemcpy(b.list_geom.data(), dl.list_geom, (size_t)b.pairs * 16, hipMemcpyDeviceToHost) != hipSuccess ||
                          hipMemcpy(b.list_gidx.data(), dl.list_gidx, (size_t)b.pairs * 4, hipMemcpyDeviceToHost) != hipSuccess)) {
        return -1;
    }
    b.stage = 2;
    return 0;
}

// The same outputs from the header on the host: what each kernel is documented to leave, in plain loops.
int build_host(const float4* geom, const float4* od, uint32_t ns, float load)
{
    Built& b = g_host;
    b = Built();
    b.ns = ns;
    b.large[rtxgrid::kLargeCap] = kCanary;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0;
    for (uint32_t i = 0; i < ns; i++) {
        const float r = fabsf(geom[i].w);
        const float c[3] = {geom[i].x, geom[i].y, geom[i].z};
        if (!(rtxgrid::finite_f(c[0]) && rtxgrid::finite_f(c[1]) && rtxgrid::finite_f(c[2]) && rtxgrid::finite_f(r))) continue;
        nf++;
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], c[k] - r);
            hi[k] = fmaxf(hi[k], c[k] + r);
        }
    }
    for (int k = 0; k < 3; k++) {
        memcpy(&b.bounds[k], &lo[k], 4);
        memcpy(&b.bounds[3 + k], &hi[k], 4);
    }
    b.bounds[6] = nf;
    plan_of(b, load);
    b.have = true;
    if (!b.g.ok) return 0;
    const Grid& g = b.g;
    b.cell_start.assign((size_t)b.n_cells + 1, 0u);
    b.is_large.assign(ns, 0);
    std::vector<int> range((size_t)ns * 6);
    for (uint32_t i = 0; i < ns; i++) {
        int* i0 = &range[(size_t)i * 6];
        int* i1 = i0 + 3;
        const bool small = rtxgrid::sphere_cells(g, geom[i].x, geom[i].y, geom[i].z, geom[i].w, i0, i1);
        b.is_large[i] = small ? 0 : 1;
        if (!small) {
            if (b.n_large < rtxgrid::kLargeCap) b.large[b.n_large] = i;
            b.n_large++;
            continue;
        }
        for (int z = i0[2]; z <= i1[2]; z++)
            for (int y = i0[1]; y <= i1[1]; y++)
                for (int x = i0[0]; x <= i1[0]; x++) b.cell_start[((size_t)z * g.n[1] + (size_t)y) * g.n[0] + (size_t)x + 1]++;
    }
    for (size_t c = 0; c < b.n_cells; c++) b.cell_start[c + 1] += b.cell_start[c];
    b.pairs = b.cell_start[b.n_cells];
    b.stage = 1;
    if (b.n_large > rtxgrid::kLargeCap) return 0;
    b.list_geom.resize(b.pairs);
    b.list_gidx.resize(b.pairs);
    std::vector<uint32_t> cursor(b.cell_start.begin(), b.cell_start.end() - 1);
    for (uint32_t i = 0; i < ns; i++) { // (ascending sphere index: every cell's entries come out in that order)
        if (b.is_large[i]) continue;
        const int* i0 = &range[(size_t)i * 6];
        const int* i1 = i0 + 3;
        uint32_t gidx;
        memcpy(&gidx, &od[i].w, 4);
        for (int z = i0[2]; z <= i1[2]; z++)
            for (int y = i0[1]; y <= i1[1]; y++)
                for (int x = i0[0]; x <= i1[0]; x++) {
                    const uint32_t at = cursor[((size_t)z * g.n[1] + (size_t)y) * g.n[0] + (size_t)x]++;
                    b.list_geom[at] = geom[i];
                    b.list_gidx[at] = gidx;
                }
    }
    b.stage = 2;
    return 0;
}

bool rays_fit(const float* rays, unsigned n) { return rays != nullptr && n != 0 && n <= kMaxRays; }

} // namespace

#define RTX_CHECK_API extern "C" __attribute__((visibility("default")))

RTX_CHECK_API int rtx_grid_check_build(const float* sph_geom, const float* sph_od, unsigned ns, float load, int host, uint32_t* head)
{
    if (!sph_geom || !sph_od || !head || ns == 0 || ns > kMaxSpheres || !(load > 0.0f)) return -2;
    const int rc = host ? build_host((const float4*)sph_geom, (const float4*)sph_od, ns, load) : build_device((const float4*)sph_geom, (const float4*)sph_od, ns, load);
    const Built& b = host ? g_host : g_dev;
    if (rc != 0) return rc;
    static_assert(sizeof(Grid) == 15 * 4, "the Grid is 15 words");
    memcpy(head, b.bounds, 28);
    memcpy(head + 7, &b.g, 60);
    head[22] = b.n_cells;
    head[23] = b.pairs;
    head[24] = b.n_large;
    head[25] = b.stage;
    return 0;
}

// The latest build's arrays: cell_start n_cells + 1 words, list_geom 4 x pairs floats, list_gidx pairs words, large kLargeCap words
// and the canary behind them, is_large ns bytes.  A null pointer is skipped; what the build's stage did not reach is left alone.
RTX_CHECK_API int rtx_grid_check_lists(int host, uint32_t* cell_start, float* list_geom, uint32_t* list_gidx, uint32_t* large, uint8_t* is_large)
{
    const Built& b = host ? g_host : g_dev;
    if (!b.have) return -2;
    if (large) memcpy(large, b.large, sizeof b.large);
    if (b.stage >= 1) {
        if (cell_start) memcpy(cell_start, b.cell_start.data(), b.cell_start.size() * 4);
        if (is_large) memcpy(is_large, b.is_large.data(), b.is_large.size());
    }
    if (b.stage >= 2 && b.pairs != 0u) {
        if (list_geom) memcpy(list_geom, b.list_geom.data(), (size_t)b.pairs * 16);
        if (list_gidx) memcpy(list_gidx, b.list_gidx.data(), (size_t)b.pairs * 4);
    }
    return 0;
}

// rays: 8 floats each (o.xyz tmax | d.xyz skip).  flags: 3 words a ray (walkable, started, steps); rec: cap x 3 words a ray.
RTX_CHECK_API int rtx_grid_check_walk(int host, const float* rays, unsigned n, unsigned cap, uint32_t* flags, uint32_t* rec)
{
    const Built& b = host ? g_host : g_dev;
    if (!b.have || !rays_fit(rays, n) || !flags || !rec || cap == 0 || cap > kMaxCap) return -2;
    if (host) {
        for (unsigned i = 0; i < n; i++) walk_one(b.g, rays + 8u * (size_t)i, cap, flags + 3u * (size_t)i, rec + 3u * (size_t)cap * i);
        return 0;
    }
    Scratch s;
    const float* d_rays = s.get<float>((size_t)n * 8, rays);
    uint32_t* d_flags = s.get<uint32_t>((size_t)n * 3);
    uint32_t* d_rec = s.get<uint32_t>((size_t)n * cap * 3);
    if (!s.ok) return -1;
    hipLaunchKernelGGL(k_walk, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, b.g, d_rays, (uint32_t)n, (uint32_t)cap, d_flags, d_rec);
    s.ran();
    s.down(flags, d_flags, (size_t)n * 12);
    s.down(rec, d_rec, (size_t)n * cap * 12);
    return s.ok ? 0 : -1;
}

// rtx_query_grid (rtx_query_brute with grid.ok = 0 where the context would: no lists) and rtx_query_brute over the device build.
// hits: 2 words a ray; fallback: one word; matrix: n x ns words (may be null).
RTX_CHECK_API int rtx_grid_check_query(const float* rays, unsigned n, int any, uint32_t* hits_grid, uint32_t* hits_brute, uint32_t* fallback, uint32_t* matrix)
{
    const Built& b = g_dev;
    if (!b.have || !rays_fit(rays, n) || !hits_grid || !hits_brute || !fallback || (matrix && (uint64_t)n * b.ns > kMaxMatrix)) return -2;
    Scratch s;
    const float4* d_rays = (const float4*)s.get<float>((size_t)n * 8, rays);
    uint2* d_hg = s.get<uint2>(n);
    uint2* d_hb = s.get<uint2>(n);
    uint32_t* d_fb = s.get<uint32_t>(2);
    uint32_t* d_matrix = matrix ? s.get<uint32_t>((size_t)n * b.ns) : nullptr;
    if (!s.ok) return -1;
    QueryArgs q;
    memset(&q, 0, sizeof q);
    q.rays = d_rays;
    q.hits = d_hg;
    q.n = n;
    q.any = any ? 1u : 0u;
    q.sph_geom = g_lists.sph_geom;
    q.sph_od = g_lists.sph_od;
    q.ns = b.ns;
    q.grid = b.g;
    q.cell_start = g_lists.cell_count;
    q.list_geom = g_lists.list_geom;
    q.list_gidx = g_lists.list_gidx;
    q.large = g_lists.large;
    q.n_large = b.n_large;
    q.fallback = d_fb;
    const bool walk = b.stage == 2;
    if (!walk) q.grid.ok = 0;
    const dim3 grid((n + (uint32_t)kThreads - 1u) / (uint32_t)kThreads), block(kThreads);
    if (walk) {
        hipLaunchKernelGGL(rtx_query_grid, grid, block, 0, 0, q);
    } else {
        hipLaunchKernelGGL(rtx_query_brute, grid, block, 0, 0, q);
    }
    q.hits = d_hb;
    q.fallback = d_fb + 1;
    hipLaunchKernelGGL(rtx_query_brute, grid, block, 0, 0, q);
    if (d_matrix) {
        const size_t total = (size_t)n * b.ns;
        hipLaunchKernelGGL(k_ray_matrix, dim3((uint32_t)((total + kThreads - 1) / kThreads)), block, 0, 0, d_rays, (uint32_t)n, g_lists.sph_geom, b.ns, d_matrix);
    }
    s.ran();
    s.down(hits_grid, d_hg, (size_t)n * 8);
    s.down(hits_brute, d_hb, (size_t)n * 8);
    s.down(fallback, d_fb, 4);
    if (d_matrix) s.down(matrix, d_matrix, (size_t)n * b.ns * 4);
    return s.ok ? 0 : -1;
}

// Segments (P, L) with toL = L - P formed as the shadow passes form it; own: 2 words a segment (the own sphere's creation index and
// its position, 0xffffffff for both: none).  dark_grid, dark_brute: a byte a segment; matrix: n x ns bytes (may be null).
RTX_CHECK_API int rtx_grid_check_segments(const float* P, const float* L, const uint32_t* own, unsigned n, uint8_t* dark_grid, uint8_t* dark_brute, uint32_t* fallback,
                                          uint8_t* matrix)
{
    const Built& b = g_dev;
    if (!b.have || !P || !L || !own || n == 0 || n > kMaxRays || !dark_grid || !dark_brute || !fallback || (matrix && (uint64_t)n * b.ns > kMaxMatrix)) return -2;
    for (unsigned i = 0; i < n; i++) {
        if (own[2u * i + 1u] != 0xffffffffu && own[2u * i + 1u] >= b.ns) return -2;
    }
    Scratch s;
    const float* d_P = s.get<float>((size_t)n * 3, P);
    const float* d_L = s.get<float>((size_t)n * 3, L);
    const uint32_t* d_own = s.get<uint32_t>((size_t)n * 2, own);
    uint8_t* d_dg = s.get<uint8_t>(n);
    uint8_t* d_db = s.get<uint8_t>(n);
    uint32_t* d_fb = s.get<uint32_t>(1);
    uint8_t* d_matrix = matrix ? s.get<uint8_t>((size_t)n * b.ns) : nullptr;
    if (!s.ok) return -1;
    KArgs a;
    memset(&a, 0, sizeof a);
    a.ns = b.ns;
    a.sph_geom = g_lists.sph_geom;
    a.sph_od = g_lists.sph_od;
    GridShadowArgs gs;
    memset(&gs, 0, sizeof gs);
    gs.grid = b.g;
    if (b.stage != 2) gs.grid.ok = 0;
    gs.cell_start = g_lists.cell_count;
    gs.list_geom = g_lists.list_geom;
    gs.list_gidx = g_lists.list_gidx;
    gs.scene_geom = g_lists.sph_geom;
    gs.scene_od = g_lists.sph_od;
    gs.large = g_lists.large;
    gs.n_large = b.stage == 2 ? b.n_large : 0u;
    gs.fallback = d_fb;
    hipLaunchKernelGGL(k_segments, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, a, gs, d_P, d_L, d_own, (uint32_t)n, d_dg, d_db, d_matrix);
    s.ran();
    s.down(dark_grid, d_dg, n);
    s.down(dark_brute, d_db, n);
    s.down(fallback, d_fb, 4);
    if (d_matrix) s.down(matrix, d_matrix, (size_t)n * b.ns);
    return s.ok ? 0 : -1;
}
