// rtx_query.cpp -- ray queries of the C ABI (rtx_query_rays, rtx_query_rays_host, rtx_pick) and the world grid behind them.
//
// The grid (rtx_grid.hpp, rtx_query_kernels.inc) is built over the scene arrays in creation order -- the device copies, which
// rtx_update_objects moves -- on the context's stream, by the first query after a scene edit or a physics step.  A build reads
// two words back (the spheres' box for the planner, then the pair total) and allocates the lists exactly: it waits for the stream
// twice, which is why a query is refused inside a graph capture.  Lists with a capacity and a whole-scene fallback, as
// rtx_bin_cells has them, would save the second wait at the price of a cell that silently tests everything; a build is off the
// hot path, so exact it is.
#include "rtx_ctx.h"

#include <cstdio>

namespace {

// room for n elements, with a quarter to spare (the build has waited for every reader of the old lists)
template <class T>
int ensure(rtx_ctx* ctx, DeviceBuf<T>& a, size_t n)
{
    if (a.capacity() >= n && a.get()) return RTX_OK;
    if (a.reserve(n + n / 4 + 64, rtxmem::nothing()) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "ray queries: out of device memory for the world grid");
    }
    return RTX_OK;
}

// The build proper, on the context's stream, between the two halves of the write (build_grid).
int fill_grid(rtx_ctx* ctx)
{
    rtx_ctx::QueryGrid& q = ctx->qgrid;
    hipStream_t st = ctx->stream;
    q.brute = false;
    q.n_cells = q.n_large = q.pairs = 0;
    q.plan = rtxgrid::plan_grid(nullptr, nullptr, 0, 0.0f);
    ctx->stat_query_builds++;
    q.dirty = false;
    const uint32_t ns = ctx->ns;
    if (ns == 0) return RTX_OK;
    int rc;
    GridBuildArgs b;
    std::memset(&b, 0, sizeof b);
    b.sph_geom = ctx->d_sph_geom.get();
    b.sph_od = ctx->d_sph_od.get();
    b.ns = ns;
    b.bounds = (float*)(q.d_words.get() + 4);
    b.totals = q.d_words.get();
    b.large = q.d_large.get();
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_grid_build(&b, 0, st));
    float box[7];
    RTX_HIP(ctx, hipMemcpyAsync(box, b.bounds, sizeof box, hipMemcpyDeviceToHost, st));
    RTX_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t n_finite = float_to_bits(box[6]);
    const float load = ctx->opt.query_load > 0 ? (float)ctx->opt.query_load / 16.0f : rtxgrid::kDefaultLoad;
    q.plan = rtxgrid::plan_grid(box, box + 3, n_finite, load);
    if (!q.plan.ok) {
        q.brute = true; // no usable grid: nothing to walk
        return RTX_OK;
    }
    q.n_cells = q.plan.n[0] * q.plan.n[1] * q.plan.n[2];
    if ((rc = ensure(ctx, q.cell_count, (size_t)q.n_cells + 1)) != RTX_OK) return rc;
    if ((rc = ensure(ctx, q.cell_fill, q.n_cells)) != RTX_OK) return rc;
    if ((rc = ensure(ctx, q.is_large, ns)) != RTX_OK) return rc;
    RTX_HIP(ctx, hipMemsetAsync(q.cell_count.get(), 0, ((size_t)q.n_cells + 1) * sizeof(uint32_t), st));
    RTX_HIP(ctx, hipMemsetAsync(q.cell_fill.get(), 0, (size_t)q.n_cells * sizeof(uint32_t), st));
    b.grid = q.plan;
    b.n_cells = q.n_cells;
    b.cell_count = q.cell_count.get();
    b.cell_fill = q.cell_fill.get();
    b.is_large = q.is_large.get();
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_grid_build(&b, 1, st));
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_grid_build(&b, 2, st));
    uint32_t totals[2];
    RTX_HIP(ctx, hipMemcpyAsync(totals, q.d_words.get(), sizeof totals, hipMemcpyDeviceToHost, st));
    RTX_HIP(ctx, hipStreamSynchronize(st));
    q.pairs = totals[0];
    q.n_large = totals[1];
    if (q.n_large > rtxgrid::kLargeCap) {
        q.brute = true;
        return RTX_OK;
    }
    if ((rc = ensure(ctx, q.pair_tmp, q.pairs)) != RTX_OK) return rc;
    if ((rc = ensure(ctx, q.list_geom, q.pairs)) != RTX_OK) return rc;
    if ((rc = ensure(ctx, q.list_gidx, q.pairs)) != RTX_OK) return rc;
    b.pair_tmp = q.pair_tmp.get();
    b.list_geom = q.list_geom.get();
    b.list_gidx = q.list_gidx.get();
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_grid_build(&b, 3, st));
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_grid_build(&b, 4, st));
    return RTX_OK;
}

int build_grid(rtx_ctx* ctx)
{
    rtx_ctx::QueryGrid& q = ctx->qgrid;
    hipStream_t st = ctx->stream;
    if (!q.d_words.get()) {
        RTX_HIP(ctx, q.d_words.reserve(16, rtxmem::nothing()));
        RTX_HIP(ctx, hipMemsetAsync(q.d_words.get(), 0, 16 * sizeof(uint32_t), st));
    }
    RTX_HIP(ctx, q.d_large.reserve(rtxgrid::kLargeCap, rtxmem::nothing()));
    // the lists may still be read by queries and by render launches (RTX_OPT_SHADOW_GRID), on whatever streams they ran
    RTX_HIP(ctx, q.sync.begin_write(st));
    const int rc = fill_grid(ctx);
    if (rc != RTX_OK) return rc;
    RTX_HIP(ctx, q.sync.end_write(st, true));
    return RTX_OK;
}

int query_device(rtx_ctx* ctx, size_t n, const void* d_rays, void* d_hits, unsigned flags, hipStream_t stream, const char* who)
{
    if (flags & ~(unsigned)RTX_QUERY_ANY) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown flag bits");
    if (n == 0) return RTX_OK;
    if (!d_rays || !d_hits) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": rays or hits is NULL");
    if (n > 0x7fffffffu) return rtx_fail(ctx, RTX_ERR_TOO_LARGE, std::string(who) + ": at most 2^31 - 1 rays per call");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    RTX_HIP(ctx, hipStreamIsCapturing(stream, &cs));
    if (cs != hipStreamCaptureStatusNone) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": not inside a graph capture (the grid's build allocates and waits)");
    }
    int rc = rtx_sync_scene(ctx);
    if (rc != RTX_OK) return rc;
    rtx_ctx::QueryGrid& g = ctx->qgrid;
    const bool brute = ctx->opt.query_check == 1;
    if ((rc = rtx_grid_ensure(ctx, stream)) != RTX_OK) return rc;
    QueryArgs a;
    std::memset(&a, 0, sizeof a);
    a.rays = (const float4*)d_rays;
    a.hits = (uint2*)d_hits;
    a.n = (uint32_t)n;
    a.any = (flags & RTX_QUERY_ANY) ? 1u : 0u;
    a.sph_geom = ctx->d_sph_geom.get();
    a.sph_od = ctx->d_sph_od.get();
    a.pl_a = ctx->d_pl_a.get();
    a.pl_b = ctx->d_pl_b.get();
    a.pl_od = ctx->d_pl_od.get();
    a.ns = ctx->ns;
    a.np = ctx->np;
    a.grid = g.plan;
    a.cell_start = g.cell_count.get();
    a.list_geom = g.list_geom.get();
    a.list_gidx = g.list_gidx.get();
    a.large = g.d_large.get();
    a.n_large = g.n_large;
    a.fallback = g.d_words.get() + 2;
    RTX_HIP(ctx, hipMemsetAsync(g.d_words.get() + 2, 0, sizeof(uint32_t), stream));
    const bool walk = !brute && !g.brute && ctx->ns != 0;
    if (!walk) a.grid.ok = 0;
    // without spheres the grid kernel has nothing to walk; the brute kernel's loop is empty as well: either gives the planes' answer
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_query(&a, walk ? 0 : 1, stream));
    ctx->last_kernel = walk ? "rtx_query_grid" : "rtx_query_brute";
    g.sync.close(stream);
    return RTX_OK;
}

} // namespace

// The grid up to date, `stream` ordered after its build: what a query and a render launch on the grid path (RTX_OPT_SHADOW_GRID) share.
int rtx_grid_ensure(rtx_ctx* ctx, hipStream_t stream)
{
    rtx_ctx::QueryGrid& g = ctx->qgrid;
    if (g.dirty || !g.d_words.get()) {
        const int rc = build_grid(ctx);
        if (rc != RTX_OK) {
            g.dirty = true;
            return rc;
        }
    }
    // the caller's stream is ordered after the build (and after the uploads and physics steps queued on the context's stream before it)
    RTX_HIP(ctx, g.sync.read(stream));
    return RTX_OK;
}

// Launches that read the lists have been queued on `stream`: the next rebuild waits for them.
void rtx_grid_read(rtx_ctx* ctx, hipStream_t stream)
{
    ctx->qgrid.sync.close(stream);
}

bool rtx_query_stat(const rtx_ctx* ctx, int option, int64_t* value, int* status)
{
    *status = RTX_OK;
    switch (option) {
    case RTX_STAT_QUERY_GRID_BUILDS: *value = (int64_t)ctx->stat_query_builds; return true;
    case RTX_STAT_QUERY_LARGE_SPHERES: *value = (int64_t)ctx->qgrid.n_large; return true;
    case RTX_STAT_QUERY_GRID_CELLS: *value = (int64_t)ctx->qgrid.n_cells; return true;
    case RTX_STAT_QUERY_GRID_PAIRS: *value = (int64_t)ctx->qgrid.pairs; return true;
    case RTX_STAT_QUERY_BRUTE: *value = ctx->qgrid.brute ? 1 : 0; return true;
    case RTX_STAT_QUERY_FALLBACK_RAYS: {
        uint32_t w = 0;
        if (ctx->qgrid.d_words.get() && rtxmem::read_words(ctx->device, ctx->qgrid.d_words.get() + 2, 1, &w) != hipSuccess) *status = RTX_ERR_HIP;
        *value = (int64_t)w;
        return true;
    }
    default: break;
    }
    if (option >= RTX_STAT_QUERY_GRID_GEOMETRY && option < RTX_STAT_QUERY_GRID_GEOMETRY + 9) {
        const int k = option - RTX_STAT_QUERY_GRID_GEOMETRY;
        const rtxgrid::Grid& g = ctx->qgrid.plan;
        *value = k < 3 ? (int64_t)float_to_bits(g.lo[k]) : k < 6 ? (int64_t)float_to_bits(g.cs[k - 3]) : (int64_t)g.n[k - 6];
        return true;
    }
    return false;
}

extern "C" {

int rtx_query_rays(rtx_ctx* ctx, size_t n, const rtx_ray* d_rays, rtx_ray_hit* d_hits, unsigned flags, void* stream)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    return query_device(ctx, n, d_rays, d_hits, flags, stream ? (hipStream_t)stream : ctx->stream, "rtx_query_rays");
}

int rtx_query_rays_host(rtx_ctx* ctx, size_t n, const rtx_ray* rays, rtx_ray_hit* hits, unsigned flags)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    if (flags & ~(unsigned)RTX_QUERY_ANY) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_query_rays_host: unknown flag bits");
    if (n == 0) return RTX_OK;
    if (!rays || !hits) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_query_rays_host: rays or hits is NULL");
    DeviceBuf<uint8_t> buf; // (freed when the call returns: the stream has been waited for by then)
    if (buf.reserve(n * (sizeof(rtx_ray) + sizeof(rtx_ray_hit)), rtxmem::nothing()) != hipSuccess) {
        return rtx_fail(ctx, RTX_ERR_OUT_OF_MEMORY, "rtx_query_rays_host: out of device memory for the rays");
    }
    void* const d = buf.get();
    rtx_ray_hit* d_hits = (rtx_ray_hit*)((char*)d + n * sizeof(rtx_ray));
    int rc = RTX_OK;
    hipError_t e = hipMemcpyAsync(d, rays, n * sizeof(rtx_ray), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        rc = query_device(ctx, n, d, d_hits, flags, ctx->stream, "rtx_query_rays_host");
        if (rc == RTX_OK) e = hipMemcpyAsync(hits, d_hits, n * sizeof(rtx_ray_hit), hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc != RTX_OK) return rc;
    if (e != hipSuccess) return rtx_hip_fail(ctx, e, "rtx_query_rays_host: copy");
    if (es != hipSuccess) return rtx_hip_fail(ctx, es, "rtx_query_rays_host: hipStreamSynchronize");
    return RTX_OK;
}

int rtx_pick(rtx_ctx* ctx, const rtx_params* p, size_t col, size_t row, rtx_ray_hit* hit)
{
    if (!ctx) return RTX_ERR_INVALID_ARGUMENT;
    if (!p || !hit) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_pick: params or hit is NULL");
    if (p->x == 0 || p->y == 0 || p->x >= (1ull << 31) || p->y >= (1ull << 31)) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_pick: frame size out of range");
    if (col + 1 >= p->x || row >= p->y) {
        return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_pick: cell outside the frame (column x - 1 holds the row's newline)");
    }
    RTX_HIP(ctx, hipSetDevice(ctx->device));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    RTX_HIP(ctx, hipStreamIsCapturing(ctx->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return rtx_fail(ctx, RTX_ERR_INVALID_ARGUMENT, "rtx_pick: not inside a graph capture (it waits for its answer)");
    rtx_ctx::QueryGrid& g = ctx->qgrid;
    RTX_HIP(ctx, g.d_ray.reserve(sizeof(rtx_ray) + 2 * sizeof(rtx_ray_hit), rtxmem::nothing()));
    KArgs a;
    std::memset(&a, 0, sizeof a);
    std::memcpy(a.m, p->inv_v, 12 * sizeof(float));
    a.ox = p->cam_pos[0];
    a.oy = p->cam_pos[1];
    a.oz = p->cam_pos[2];
    a.e1 = p->element1;
    a.e2 = p->element2;
    a.far = p->cam_far;
    a.fW = (float)p->x;
    a.fH = (float)p->y;
    RTX_HIP(ctx, (hipError_t)rtx_k_launch_pick_ray(&a, (uint32_t)col, (uint32_t)row, g.d_ray.get(), ctx->stream));
    rtx_ray_hit* d_hit = (rtx_ray_hit*)(g.d_ray.get() + sizeof(rtx_ray));
    const int rc = query_device(ctx, 1, g.d_ray.get(), d_hit, RTX_QUERY_CLOSEST, ctx->stream, "rtx_pick");
    if (rc != RTX_OK) return rc;
    RTX_HIP(ctx, hipMemcpyAsync(hit, d_hit, sizeof *hit, hipMemcpyDeviceToHost, ctx->stream));
    RTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTX_OK;
}

} // extern "C"
