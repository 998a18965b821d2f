// cull_check.hip -- TEST INFRASTRUCTURE (built by __graft_entry__.build(), loaded only by tests/test_gpu_cull_bound.py).
// Runs the culling geometry of rtx_cull.hpp -- tile_plane, tile_culls, tile_culls_moving, plane_invisible: the very text the trace
// kernels and rtx_bin_cells compile -- on (rectangle, sphere) and (rectangle, plane) pairs of the caller's choosing and hands the
// raw verdicts and margins back, and beside them the ground truth of "can be hit": the production per-pixel tests (sphere_reject /
// sphere_hit, plane_hit) over every pixel of the rectangle, each primary ray built as the trace builds it.
//
// A camera is 21 floats: inv_v[16] (row-major), position[3], element1, element2; with it go the frame's W and H.  A rectangle is
// four uint32 (col0, row0, w, h) inside the frame, a sphere a float4 (centre, radius), a plane eight floats (px py pz width, nx ny
// nz height), a pair two uint32 (rectangle index, sphere / plane index).  Every entry point returns 0, -1 on a HIP error, -2 on
// arguments it refuses (an index or a rectangle out of range: nothing is launched).
#include "../../raytracing-in-windows-console_amd/csrc/rtx_cull.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_workgroup.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "check_args.hpp"

namespace {

using namespace rtx;
using rtx_check::args_of;
using rtx_check::Buffers;

constexpr int kBlock = 256;
// kNoHit (rtx_workgroup.hpp) is the distance a pixel starts from (RayTracing.h:21).  A test counts as a hit when the trace would
// take it: it reports one AND its t is below kNoHit -- a NaN t, which the tests let through for a NaN ray, is below nothing and
// wins no pixel.

struct Rect {
    uint32_t col0, row0, w, h;
};

// rtx_tile_pass.inc: tile_camera
__device__ __forceinline__ Camera camera_of(const KArgs& a)
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

// The primary ray of pixel (col, row): the per-column and per-row terms as rtx_tile_pass.inc (tile_pixel) and the trace body's
// s_col / s_row form them, then ray_from_tables.
__device__ __forceinline__ Ray pixel_ray(const Camera& cam, uint32_t col, uint32_t row)
{
    const float vx = (((float)(2u * col) - cam.fW) / cam.fW) * cam.e1;
    const float vy = ((cam.fH - (float)(row * 2u)) / cam.fH) * cam.e2;
    return ray_from_tables(cam, make_float4(cam.m[0] * vx, cam.m[4] * vx, cam.m[8] * vx, 0.0f), make_float4(cam.m[1] * vy, cam.m[5] * vy, cam.m[9] * vy, 0.0f));
}

// One thread per (rectangle, plane k): the normal tile_plane returns.
__global__ void tile_planes(KArgs a, const Rect* rects, uint32_t nrect, float* out)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= nrect * 5u) {
        return;
    }
    const Camera cam = camera_of(a);
    const Rect r = rects[i / 5u];
    const V3 n = tile_plane(a, cam, r.col0, r.row0, r.w, r.h, i % 5u);
    out[3u * i + 0u] = n.x;
    out[3u * i + 1u] = n.y;
    out[3u * i + 2u] = n.z;
}

// One thread per pair: the five planes, the hoisted terms as stage_chunk and rtx_bin_cells form them, both culling tests.
// flags: bit 0 tile_culls' verdict, bit 1 tile_culls_moving's, bit 2 its `inside`, bit 3 cc > 0.  margins: static, moving.
// rec: ox oy oz oo.
__global__ void cull_spheres(KArgs a, const Rect* rects, const float4* sph, const uint2* pairs, uint32_t n, float theta, float delta, uint32_t* flags,
                             float2* margins, float4* rec)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const Camera cam = camera_of(a);
    const Rect r = rects[pairs[i].x];
    const float4 g = sph[pairs[i].y];
    TileFrustum fr;
#pragma unroll
    for (uint32_t k = 0; k < 5u; k++) {
        fr.n[k] = tile_plane(a, cam, r.col0, r.row0, r.w, r.h, k);
    }
    const float ox = cam.ox - g.x, oy = cam.oy - g.y, oz = cam.oz - g.z;
    const float oo = ox * ox + oy * oy + oz * oz;
    const float cc = oo - (g.w * g.w);
    float m_static = 0.0f, m_moving = 0.0f;
    bool inside = false;
    const bool culled = tile_culls(fr, ox, oy, oz, oo, g.w, m_static);
    const bool culled_moving = tile_culls_moving(fr, ox, oy, oz, oo, g.w, theta, delta, m_moving, inside);
    flags[i] = (culled ? 1u : 0u) | (culled_moving ? 2u : 0u) | (inside ? 4u : 0u) | (cc > 0.0f ? 8u : 0u);
    margins[i] = make_float2(m_static, m_moving);
    rec[i] = make_float4(ox, oy, oz, oo);
}

// One workgroup per pair walks the rectangle's pixels: the trace's ray, its divTwoA (the non-REFINE kernels' half_recip from the
// LDS tables), the production sphere test on the hoisted terms.  hit[pair] = 1 when any pixel's test reports a hit.
__global__ __launch_bounds__(kBlock) void rect_hits(KArgs a, const Rect* rects, const float4* sph, const uint2* pairs, uint32_t* hit)
{
    __shared__ uint32_t s_half[kUnitEntries], s_unit[kUnitEntries];
    __shared__ uint32_t s_any;
    const uint32_t tid = threadIdx.x;
    half_table_fill(s_half, tid);
    unit_table_fill(s_unit, tid);
    if (tid == 0u) {
        s_any = 0u;
    }
    __syncthreads();
    const Camera cam = camera_of(a);
    const Rect r = rects[pairs[blockIdx.x].x];
    const float4 g = sph[pairs[blockIdx.x].y];
    // objectToCam = origin - spherePos; c = Dot(otc,otc) - r*r   (Sphere.cu:34-37), as stage_chunk hoists them
    const float ox = cam.ox - g.x, oy = cam.oy - g.y, oz = cam.oz - g.z;
    const float oo = ox * ox + oy * oy + oz * oz;
    const float cc = oo - (g.w * g.w);
    bool any = false;
    for (uint32_t i = tid; i < r.w * r.h; i += (uint32_t)kBlock) {
        Ray ray = pixel_ray(cam, r.col0 + i % r.w, r.row0 + i / r.w);
        float a_unit = 0.0f;
        ray.divTwoA = half_recip(ray.a, s_half, s_unit, a_unit);
        float s;
        if (!sphere_reject(ray, ox, oy, oz, cc, s)) {
            float t;
            any = (sphere_hit(ray, s, cc, t) && t < kNoHit) || any;
        }
    }
    if (any) {
        atomicOr(&s_any, 1u);
    }
    __syncthreads();
    if (tid == 0u) {
        hit[blockIdx.x] = s_any;
    }
}

// One workgroup per (rectangle, plane) pair.  out[pair]: bit 0 plane_invisible's verdict on the terms the trace body hands it,
// bit 1 some pixel's plane_hit reports a hit.
__global__ __launch_bounds__(kBlock) void cull_planes(KArgs a, const Rect* rects, const float4* planes, const uint2* pairs, uint32_t* out)
{
    __shared__ uint32_t s_any;
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) {
        s_any = 0u;
    }
    __syncthreads();
    const Camera cam = camera_of(a);
    const Rect r = rects[pairs[blockIdx.x].x];
    const float4 pla = planes[2u * pairs[blockIdx.x].y], plb = planes[2u * pairs[blockIdx.x].y + 1u];
    const V3 p = v3(pla.x, pla.y, pla.z), n = v3(plb.x, plb.y, plb.z);
    bool any = false;
    for (uint32_t i = tid; i < r.w * r.h; i += (uint32_t)kBlock) {
        const Ray ray = pixel_ray(cam, r.col0 + i % r.w, r.row0 + i / r.w);
        float t;
        any = (plane_hit(ray, p, n, pla.w, plb.w, t) && t < kNoHit) || any;
    }
    if (any) {
        atomicOr(&s_any, 2u);
    }
    __syncthreads();
    if (tid == 0u) {
        // rtx_trace_body.inc: the ray-independent parts of Plane::Trace, as the table's rows are formed
        const float num = dot(sub(p, v3(cam.ox, cam.oy, cam.oz)), n);
        const float hw = pla.w * 0.5f, hh = plb.w * 0.5f;
        const float4 bounds = make_float4(p.x - hw, p.x + hw, p.z - hh, p.z + hh);
        out[blockIdx.x] = s_any | (plane_invisible(cam, r.col0, r.row0, r.w, r.h, n, num, bounds) ? 1u : 0u);
    }
}

bool rects_fit(const uint32_t* rects, unsigned nrect, unsigned W, unsigned H)
{
    for (unsigned i = 0; i < nrect; i++) {
        const uint64_t c0 = rects[4 * i], r0 = rects[4 * i + 1], w = rects[4 * i + 2], h = rects[4 * i + 3];
        if (w == 0 || h == 0 || c0 + w > W || r0 + h > H || w * h > (1u << 20)) {
            return false;
        }
    }
    return W > 0 && H > 0 && W <= (1u << 20) && H <= (1u << 20);
}

bool pairs_fit(const uint32_t* pairs, unsigned n, unsigned nrect, unsigned nitems)
{
    for (unsigned i = 0; i < n; i++) {
        if (pairs[2 * i] >= nrect || pairs[2 * i + 1] >= nitems) {
            return false;
        }
    }
    return n > 0 && n < (1u << 30);
}

} // namespace

#define RTX_CHECK_API extern "C" __attribute__((visibility("default")))

// planes_out: nrect * 5 normals of three floats, tile_plane(k = 0..4) of every rectangle.
RTX_CHECK_API int rtx_check_tile_planes(const float* cam, unsigned W, unsigned H, const uint32_t* rects, unsigned nrect, float* planes_out)
{
    if (!cam || !rects || !planes_out || nrect == 0 || nrect > (1u << 20) || !rects_fit(rects, nrect, W, H)) return -2;
    Buffers b;
    const Rect* d_rects = (const Rect*)b.up(rects, (size_t)nrect * 16);
    float* d_out = (float*)b.up(nullptr, (size_t)nrect * 60);
    if (!b.ok) return -1;
    hipLaunchKernelGGL(tile_planes, dim3((nrect * 5u + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, args_of(cam, W, H), d_rects, nrect, d_out);
    return b.ran() && b.down(planes_out, d_out, (size_t)nrect * 60) ? 0 : -1;
}

// flags_out: n words; margins_out: n x (static, moving); rec_out: n x (ox, oy, oz, oo).
RTX_CHECK_API int rtx_check_cull_spheres(const float* cam, unsigned W, unsigned H, const uint32_t* rects, unsigned nrect, const float* spheres, unsigned ns,
                                         const uint32_t* pairs, unsigned n, float theta, float delta, uint32_t* flags_out, float* margins_out, float* rec_out)
{
    if (!cam || !rects || !spheres || !pairs || !flags_out || !margins_out || !rec_out || !rects_fit(rects, nrect, W, H) || !pairs_fit(pairs, n, nrect, ns)) return -2;
    Buffers b;
    const Rect* d_rects = (const Rect*)b.up(rects, (size_t)nrect * 16);
    const float4* d_sph = (const float4*)b.up(spheres, (size_t)ns * 16);
    const uint2* d_pairs = (const uint2*)b.up(pairs, (size_t)n * 8);
    uint32_t* d_flags = (uint32_t*)b.up(nullptr, (size_t)n * 4);
    float2* d_margins = (float2*)b.up(nullptr, (size_t)n * 8);
    float4* d_rec = (float4*)b.up(nullptr, (size_t)n * 16);
    if (!b.ok) return -1;
    hipLaunchKernelGGL(cull_spheres, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, args_of(cam, W, H), d_rects, d_sph, d_pairs, (uint32_t)n, theta, delta,
                       d_flags, d_margins, d_rec);
    return b.ran() && b.down(flags_out, d_flags, (size_t)n * 4) && b.down(margins_out, d_margins, (size_t)n * 8) && b.down(rec_out, d_rec, (size_t)n * 16) ? 0 : -1;
}

// hit_out: n words, 1 where some pixel of the pair's rectangle hits the pair's sphere from this camera.
RTX_CHECK_API int rtx_check_rect_hits(const float* cam, unsigned W, unsigned H, const uint32_t* rects, unsigned nrect, const float* spheres, unsigned ns,
                                      const uint32_t* pairs, unsigned n, uint32_t* hit_out)
{
    if (!cam || !rects || !spheres || !pairs || !hit_out || !rects_fit(rects, nrect, W, H) || !pairs_fit(pairs, n, nrect, ns)) return -2;
    Buffers b;
    const Rect* d_rects = (const Rect*)b.up(rects, (size_t)nrect * 16);
    const float4* d_sph = (const float4*)b.up(spheres, (size_t)ns * 16);
    const uint2* d_pairs = (const uint2*)b.up(pairs, (size_t)n * 8);
    uint32_t* d_hit = (uint32_t*)b.up(nullptr, (size_t)n * 4);
    if (!b.ok) return -1;
    hipLaunchKernelGGL(rect_hits, dim3(n), dim3(kBlock), 0, 0, args_of(cam, W, H), d_rects, d_sph, d_pairs, d_hit);
    return b.ran() && b.down(hit_out, d_hit, (size_t)n * 4) ? 0 : -1;
}

// out: n words, bit 0 plane_invisible, bit 1 some pixel's plane_hit hits.
RTX_CHECK_API int rtx_check_cull_planes(const float* cam, unsigned W, unsigned H, const uint32_t* rects, unsigned nrect, const float* planes, unsigned np,
                                        const uint32_t* pairs, unsigned n, uint32_t* out)
{
    if (!cam || !rects || !planes || !pairs || !out || !rects_fit(rects, nrect, W, H) || !pairs_fit(pairs, n, nrect, np)) return -2;
    Buffers b;
    const Rect* d_rects = (const Rect*)b.up(rects, (size_t)nrect * 16);
    const float4* d_planes = (const float4*)b.up(planes, (size_t)np * 32);
    const uint2* d_pairs = (const uint2*)b.up(pairs, (size_t)n * 8);
    uint32_t* d_out = (uint32_t*)b.up(nullptr, (size_t)n * 4);
    if (!b.ok) return -1;
    hipLaunchKernelGGL(cull_planes, dim3(n), dim3(kBlock), 0, 0, args_of(cam, W, H), d_rects, d_planes, d_pairs, d_out);
    return b.ran() && b.down(out, d_out, (size_t)n * 4) ? 0 : -1;
}

// rtxplan::cell_motion (host): what camera `now` has used of the budgets of lists built for camera `built`, same frame and scene,
// with drift_built / drift_now the scene's accumulated sphere motion at the two times.
RTX_CHECK_API int rtx_check_cell_motion(const float* built, const float* now, unsigned W, unsigned H, double drift_built, double drift_now, float* theta,
                                        float* delta)
{
    if (!built || !now || !theta || !delta) return -2;
    rtxplan::CellCamera cb, cn;
    cb.view = rtxplan::view_of(built, built + 16);
    cn.view = rtxplan::view_of(now, now + 16);
    cb.e1 = built[19]; cb.e2 = built[20];
    cn.e1 = now[19]; cn.e2 = now[20];
    cb.W = cn.W = W;
    cb.H = cn.H = H;
    cb.drift = drift_built;
    cn.drift = drift_now;
    const rtxplan::CellBudget m = rtxplan::cell_motion(cb, cn);
    *theta = m.theta;
    *delta = m.delta;
    return 0;
}
