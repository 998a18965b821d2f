// rtx_cull.hpp -- the culling geometry of the trace kernels and of rtx_bin_cells, and the primary ray built from the staged
// per-column / per-row terms: device functions only, so that rtx_kernels.hip and the direct check of these bounds
// (tests/gpu_checks/cull_check.hip, tests/test_gpu_cull_bound.py) compile the same text.
#pragma once

#include "rtx_device.hpp"
#include "rtx_kernels.h"

namespace rtx {

// Conservative inflation of a sphere for culling.  A ray whose fp32 test reports a hit passes, in exact
// arithmetic, within R of the centre with R^2 = r^2 (1+2u) + 15.2u |otc|^2 (u = 2^-24; derivation in
// DESIGN.md "Culling soundness"), and no further than 3u|otc| behind the apex.  kappa = 2e-6 is 2.2x
// that constant; kDelta |otc| covers the apex term and the rounding of the plane evaluation, of the
// plane normals and of the hardware sqrt used below (together < 1.5e-6 |otc|).
constexpr float kKappa = 2.0e-6f;
constexpr float kDelta = 5.0e-6f;

struct TileFrustum {
    V3 n[5]; // inward unit normals of the four side planes, then the frame's camera plane
};

__device__ __forceinline__ V3 cross(V3 a, V3 b)
{
    return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// Direction (unnormalised) through view-plane point (cx, cy): the linear part of make_ray.
__device__ __forceinline__ V3 view_dir(const Camera& c, float cx, float cy)
{
    const float vx = cx * c.e1, vy = cy * c.e2;
    return v3(c.m[0] * vx + c.m[1] * vy + c.m[2], c.m[4] * vx + c.m[5] * vy + c.m[6], c.m[8] * vx + c.m[9] * vy + c.m[10]);
}

// true when the sphere (hoisted form) provably cannot be hit by any pixel ray of the tile.
__device__ __forceinline__ bool tile_culls(const TileFrustum& f, float ox, float oy, float oz, float oo, float r, float& margin)
{
    // margin >= R + 3u|otc| + evaluation slack (see kKappa); hardware sqrt is within 1 ulp
    margin = __builtin_amdgcn_sqrtf(r * r * (1.0f + kKappa) + kKappa * oo) + kDelta * __builtin_amdgcn_sqrtf(oo);
    bool out = false;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        // n . (c - o) = -(n . otc); outside when it is below -margin.  NaN compares false: keep.
        const float d = f.n[k].x * ox + f.n[k].y * oy + f.n[k].z * oz;
        out = out || (d > margin);
    }
    return out;
}

// The same test with the margin grown for cell lists that are to outlive this frame (rtx_plan.hpp, "cell-list reuse"):
// valid for every camera whose pixel directions are within theta (chord) of this one's and whose position, sphere motion
// counted in, is within delta:   margin' = m + delta + theta (|O| + delta + m),   m = margin(r, |O| + delta),
// times 1 + 4e-6 for the rounding of these few operations (hardware sqrt included).  `inside` reports whether some
// such camera can lie inside or on the sphere (then it is never culled).  theta = delta = 0 gives tile_culls' margin
// within that factor.
__device__ __forceinline__ bool tile_culls_moving(const TileFrustum& f, float ox, float oy, float oz, float oo, float r, float theta, float delta, float& margin,
                                                  bool& inside)
{
    const float dist = __builtin_amdgcn_sqrtf(oo) * (1.0f + 1.0e-6f) + delta; // >= |O| + delta
    const float m = __builtin_amdgcn_sqrtf(r * r * (1.0f + kKappa) + kKappa * (dist * dist)) + kDelta * dist;
    margin = (m + delta + theta * (dist + m)) * (1.0f + 4.0e-6f);
    inside = !(__builtin_amdgcn_sqrtf(oo) * (1.0f - 1.0e-6f) - delta > fabsf(r) * (1.0f + 1.0e-6f));
    bool out = false;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const float d = f.n[k].x * ox + f.n[k].y * oy + f.n[k].z * oz;
        out = out || (d > margin);
    }
    return out;
}

// One plane of the pyramid spanned by the pixel centres of columns [col0, col0+w) and rows [row0, row0+h), grown by
// half a pixel on every side, selected by k: 0 the top edge (row0), 1 the right edge (col0 + w), 2 the bottom edge
// (row0 + h), 3 the left edge (col0), 4 the camera plane -- arranged so that five lanes compute the five planes side by
// side.  Pixel directions are linear in (cx, cy), so every pixel ray of the rectangle lies in the convex cone of the four
// corner directions, and the plane through the apex and an edge cy = y (cx = x) has the normal y up_p + up_q (x right_p +
// right_q), oriented up (right) in the frame, from per-frame vectors (rtx_plan.hpp, EdgeBasis: computed on the host in
// double).  NOT the cross product of the two corner directions: for a thin tile far off the view axis those are nearly
// parallel and long, and the fp32 product loses the plane (8K, first 16 columns: 4e-6 rad with the reference's own
// camera matrices -- most of the half pixel, 5.3e-6 rad there -- and up to 8e-5 rad with a rolled camera, where a culling
// kernel then drops rows of a large far sphere's cap: tools/wide_view_directed_gpu.py).
// The fifth plane is the same for every rectangle of the frame: the camera plane (it culls what lies behind the apex; all
// pixel rays of the frame point into its front half-space, which the host has checked).
// An ill-conditioned normal (degenerate or sheared matrix, NaN) becomes the zero vector, which never culls.  This is
// culling geometry, not reference arithmetic: hardware rcp/rsq (1 ulp) are used, and the slack in tile_culls covers their
// error and the normal's (4e-7 from the two roundings per component and the rounded basis; 4e-7 from the edge
// coordinate's own rounding).
__device__ __forceinline__ V3 tile_plane(const KArgs& a, const Camera& c, uint32_t col0, uint32_t row0, uint32_t w, uint32_t h, uint32_t k)
{
    if (k == 4u) {
        return v3(a.edge_fwd[0], a.edge_fwd[1], a.edge_fwd[2]);
    }
    const bool row_edge = (k & 1u) == 0u;
    // the edge's coordinate: cy of row boundary e (half a pixel above row e), cx of column boundary e
    const uint32_t e = row_edge ? row0 + (k == 2u ? h : 0u) : col0 + (k == 1u ? w : 0u);
    const float t = row_edge ? (c.fH - 2.0f * (float)e + 1.0f) * __builtin_amdgcn_rcpf(c.fH) : (2.0f * (float)e - 1.0f - c.fW) * __builtin_amdgcn_rcpf(c.fW);
    const V3 p = row_edge ? v3(a.edge_up_p[0], a.edge_up_p[1], a.edge_up_p[2]) : v3(a.edge_right_p[0], a.edge_right_p[1], a.edge_right_p[2]);
    const V3 q = row_edge ? v3(a.edge_up_q[0], a.edge_up_q[1], a.edge_up_q[2]) : v3(a.edge_right_q[0], a.edge_right_q[1], a.edge_right_q[2]);
    V3 n = v3(t * p.x + q.x, t * p.y + q.y, t * p.z + q.z);
    // refuse a sum that cancelled (the two terms are perpendicular for a camera matrix: no cancellation at all)
    const float hyp2 = (t * t) * a.edge_pp + (row_edge ? a.edge_qrqr : a.edge_qcqc);
    const float len2 = dot(n, n);
    if (!(len2 >= 0.25f * hyp2) || !(len2 > 1.0e-30f && len2 < 1.0e30f)) {
        return v3(0.0f, 0.0f, 0.0f);
    }
    // inward: down from the top edge, left from the right edge, up from the bottom edge, right from the left edge
    const float s = (k < 2u ? -1.0f : 1.0f) * __builtin_amdgcn_rsqf(len2);
    return mulf(n, s);
}

// true when no pixel ray of the rectangle (columns [col0, col0+w), rows [row0, row0+h), half a pixel out, as for the
// pyramids) can hit the bounded plane {n, num = Dot(planePos - origin, n), bounds xlo xhi zlo zhi}, so that the
// workgroup may leave the plane out of its table.  Plane::Trace (Plane.cu:38-72) reports a hit iff dn < 0 (beyond
// FLT_EPSILON), t = num / dn > 0 and the hit point lies strictly inside the bounds in x and z.
//  * num >= 0: a ray with dn < 0 gets t <= 0 -- exactly, the fp32 quotient has the sign of its operands -- and every
//    other ray is rejected on dn: no hit, whatever the rectangle.
//  * Pixel directions are convex combinations of the four corner directions w_i, and w . n is linear: if it is
//    positive at all corners (by more than 1e-5 |w||n|) every dn is positive: no hit.
//  * If it is negative at all corners, every ray hits the unbounded plane and the hit points lie in the convex
//    hull of the four corner hit points (central projection of a convex cone onto a plane that cuts all its rays).
//    The plane is invisible when their bounding interval, widened by the worst rounding error of the per-pixel
//    arithmetic, misses the bounds in x or in z.  That error: |dn| >= q = min |w_i . n| / max |w_i| over the cone,
//    dn carries an absolute error below 4e-7, so t and the hit offset d t carry a relative error below
//    4e-7 / q + 1e-6; the bound used is 2e-6 / q + 1e-5 of (|origin| + largest corner offset), and grazing
//    rectangles (q < 1e-3) are kept.
// Anything undecided (mixed signs, NaNs, degenerate matrices) keeps the plane.  Culling geometry, not reference
// arithmetic: hardware rcp/sqrt.
__device__ __forceinline__ bool plane_invisible(const Camera& c, uint32_t col0, uint32_t row0, uint32_t w, uint32_t h, V3 n, float num, float4 bd)
{
    if (num >= 0.0f) {
        return true;
    }
    const float rW = __builtin_amdgcn_rcpf(c.fW), rH = __builtin_amdgcn_rcpf(c.fH);
    const float x0 = (2.0f * (float)col0 - 1.0f - c.fW) * rW;
    const float x1 = (2.0f * (float)(col0 + w) - 1.0f - c.fW) * rW;
    const float y0 = (c.fH - 2.0f * (float)row0 + 1.0f) * rH;
    const float y1 = (c.fH - 2.0f * (float)(row0 + h) + 1.0f) * rH;
    const float nn = dot(n, n);
    bool away = true, facing = true;
    float min_abs = __builtin_inff(), max_len2 = 0.0f;
    float hx_lo = __builtin_inff(), hx_hi = -__builtin_inff(), hz_lo = __builtin_inff(), hz_hi = -__builtin_inff(), span_x = 0.0f, span_z = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const V3 wi = view_dir(c, (i == 1 || i == 2) ? x1 : x0, i >= 2 ? y1 : y0);
        const float wn = dot(wi, n), len2 = dot(wi, wi);
        const float eps = 1.0e-5f * __builtin_amdgcn_sqrtf(len2 * nn);
        away = away && (wn > eps);
        facing = facing && (wn < -eps);
        min_abs = fminf(min_abs, fabsf(wn));
        max_len2 = fmaxf(max_len2, len2);
        const float si = num * __builtin_amdgcn_rcpf(wn); // > 0 where the corner faces the plane
        const float dx = wi.x * si, dz = wi.z * si;
        hx_lo = fminf(hx_lo, c.ox + dx);
        hx_hi = fmaxf(hx_hi, c.ox + dx);
        hz_lo = fminf(hz_lo, c.oz + dz);
        hz_hi = fmaxf(hz_hi, c.oz + dz);
        span_x = fmaxf(span_x, fabsf(dx));
        span_z = fmaxf(span_z, fabsf(dz));
    }
    if (away) {
        return true;
    }
    if (!facing) {
        return false;
    }
    const float q = min_abs * __builtin_amdgcn_rsqf(max_len2 * nn);
    if (!(q > 1.0e-3f)) {
        return false;
    }
    const float rel = 2.0e-6f * __builtin_amdgcn_rcpf(q) + 1.0e-5f;
    const float ex = rel * (fabsf(c.ox) + span_x) + 1.0e-30f, ez = rel * (fabsf(c.oz) + span_z) + 1.0e-30f;
    return (hx_hi + ex <= bd.x) || (hx_lo - ex >= bd.y) || (hz_hi + ez <= bd.z) || (hz_lo - ez >= bd.w);
}

// Ray of pixel (row, col) from the staged per-column / per-row terms:
//   A = (m0, m4, m8) * (convertedX * e1),  B = (m1, m5, m9) * (convertedY * e2)
// so that d.k = ((A.k + B.k) + m[4k+2] * 1.0f) + m[4k+3] * 0.0f, the order of Matrix::Mult
// (MyMath.h:310-319) applied to (vx, vy, 1, 0) as in RayTracing.cu:19-23.
__device__ __forceinline__ Ray ray_from_tables(const Camera& c, float4 A, float4 B)
{
    V3 w;
    w.x = ((A.x + B.x) + c.m[2]) + c.m[3] * 0.0f;
    w.y = ((A.y + B.y) + c.m[6]) + c.m[7] * 0.0f;
    w.z = ((A.z + B.z) + c.m[10]) + c.m[11] * 0.0f;
    Ray r;
    r.o = v3(c.ox, c.oy, c.oz);
    r.d = normalize_gpu(w);
    r.a = dot(r.d, r.d);
    r.fourA = 4.0f * r.a;
    r.divTwoA = 0.0f; // filled by the caller that tests spheres
    return r;
}

} // namespace rtx
