// rtx_shadow.hpp -- the conservative occluder bound of the shadow pass (rtx_shadow_shade), for host and device alike.
//
// A shading workgroup owns up to 256 hit points P_i; the shadow rays are the open segments (P_i, L) to the light L.  Every one of
// them lies inside the cone with apex L that holds the directions u_i = (P_i - L) / |P_i - L|, cut off at the largest distance
// |P_i - L|.  A sphere that misses that truncated cone meets none of the segments and is culled once for the whole workgroup.
//
// The cone is an axis a (the normalised sum of the u_i), a half-angle theta (the largest angle between a and a u_i) and a
// distance dmax.  A sphere (C, r) seen from L at distance D subtends the half-angle asin(r / D); it can touch the cone only if the
// angle between a and C - L is at most theta + asin(r / D), and only if D - r < dmax.  Angles are taken with atan2(|x cross y|,
// x . y), which stays accurate near 0 where acos does not.  r is |r| throughout: the exact test squares the radius, so a sphere
// of negative radius shadows as the one of radius |r| does.
//
// Rounding: every quantity is fp32 and the exact test of the shadow pass is fp32 too, so the bound carries margins far above
// the few ulps either can be off by: the radius is inflated by a relative 1e-4 of itself and of D and by 1e-5 of the coordinate
// scale (|L| + dmax: what the hit points and the closest points of the exact test are rounded at), the angles by 1e-4 rad and
// dmax by a relative 1e-4.  Degenerate cones keep everything: a hit point at (or within 1e-6 |P| of) the light, directions that
// do not add up to a clear axis (L inside the hull of the points), and theta of 90 degrees or more.  tests/host/test_shadow_bound.cpp
// checks the bound against a float64 segment-to-ball test over millions of random cases; tests/test_gpu_tile_bound.py runs it
// on the device, with the cone as light_cone (rtx_tile_pass.inc) reduces it there.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_SHADOW_HD __host__ __device__
#else
#define RTX_SHADOW_HD
#endif

namespace rtxshadow {

constexpr float kAngleMargin = 1.0e-4f; // rad
constexpr float kRelMargin = 1.0e-4f;
constexpr float kHalfPi = 1.57079632679f;

struct Cone {
    float ax, ay, az;  // unit axis from the light
    float theta;       // half-angle, margin included
    float dmax;        // farthest hit point, margin included
    float slack;       // absolute radius inflation: the rounding of points and segments at this coordinate scale
    bool all;          // degenerate: every sphere is kept
};

RTX_SHADOW_HD inline float angle_between(float ax, float ay, float az, float bx, float by, float bz)
{
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return atan2f(sqrtf(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);
}

// Step 1, per hit point: the unit direction from the light, its distance, and whether the point is degenerate (at the light).
RTX_SHADOW_HD inline bool direction_from_light(const float L[3], const float P[3], float u[3], float* dist)
{
    const float dx = P[0] - L[0], dy = P[1] - L[1], dz = P[2] - L[2];
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    *dist = d;
    const float scale = fabsf(P[0]) + fabsf(P[1]) + fabsf(P[2]) + fabsf(L[0]) + fabsf(L[1]) + fabsf(L[2]);
    if (!(d > 1.0e-6f * scale) || !(d < 3.0e38f)) {
        u[0] = u[1] = u[2] = 0.0f;
        return false;
    }
    u[0] = dx / d;
    u[1] = dy / d;
    u[2] = dz / d;
    return true;
}

// Step 2: the axis from the sum of the directions of n points.  A sum shorter than a tenth of n has no clear axis (the light
// sits among the points, or nearly): the caller keeps everything.
RTX_SHADOW_HD inline bool axis_from_sum(float sx, float sy, float sz, float n, float a[3])
{
    const float len = sqrtf(sx * sx + sy * sy + sz * sz);
    if (!(len > 0.1f * n)) return false;
    a[0] = sx / len;
    a[1] = sy / len;
    a[2] = sz / len;
    return true;
}

// Step 3, per hit point: its angle from the axis (the workgroup keeps the largest).
RTX_SHADOW_HD inline float angle_from_axis(const float a[3], const float u[3]) { return angle_between(a[0], a[1], a[2], u[0], u[1], u[2]); }

// Step 4: the cone from the reductions (the largest angle and distance; any degenerate point).
RTX_SHADOW_HD inline Cone make_cone(const float L[3], const float a[3], float max_angle, float max_dist, bool degenerate)
{
    Cone c;
    c.ax = a[0];
    c.ay = a[1];
    c.az = a[2];
    c.theta = max_angle + kAngleMargin;
    c.dmax = max_dist * (1.0f + kRelMargin) + 1.0e-30f;
    c.slack = 1.0e-5f * (fabsf(L[0]) + fabsf(L[1]) + fabsf(L[2]) + c.dmax);
    c.all = degenerate || !(c.theta < kHalfPi) || !(c.slack < 3.0e37f);
    return c;
}

// May sphere (C, r) meet a segment of the cone?  false: it meets none of them.
RTX_SHADOW_HD inline bool may_occlude(const Cone& c, const float L[3], float cx, float cy, float cz, float r)
{
    if (c.all) return true;
    const float vx = cx - L[0], vy = cy - L[1], vz = cz - L[2];
    const float D = sqrtf(vx * vx + vy * vy + vz * vz);
    const float R = fabsf(r) * (1.0f + kRelMargin) + kRelMargin * D + c.slack; // (the exact test squares r: a negative radius is |r|)
    if (!(D > R)) return true;        // the light is inside the (inflated) ball, or NaN
    if (D - R > c.dmax) return false; // beyond the farthest hit point
    const float phi = angle_between(c.ax, c.ay, c.az, vx, vy, vz);
    const float beta = asinf(R / D);
    return phi <= c.theta + beta + kAngleMargin;
}

} // namespace rtxshadow
