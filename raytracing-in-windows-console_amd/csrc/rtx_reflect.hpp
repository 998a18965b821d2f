// rtx_reflect.hpp -- the conservative sphere bound of the mirror pass (rtx_reflect_hit), for host and device alike.
//
// A workgroup owns up to 256 secondary rays (P_i, R_i): P_i the primary hit point, R_i the mirrored view direction.  Every point
// P_i + s R_i (s >= 0) lies within rho of the cone with apex O, axis a and half-angle theta when the origins lie in the ball
// (O, rho) and the unit directions u_i = R_i / |R_i| within theta of a: O + s u_i is on the cone and |P_i - O| <= rho.  A sphere
// whose fp32 exact test reports a hit is passed, in exact arithmetic, within its error radius
//   r' = sqrt(r^2 (1 + kappa) + kappa |P - C|^2)   (R^2 = r^2 (1+2u) + 15.2u |O|^2, u = 2^-24; kappa = 2e-6 > 15.2u)
// of its centre C, so a sphere whose distance to the cone exceeds r' + rho is hit by none of the rays and is culled once for the
// whole workgroup.  |P - C| is bounded by |C - O| + rho.  The distance from C to the cone is 0 inside it and D sin(phi - theta)
// beyond it (D = |C - O|, phi the angle between a and C - O, up to phi - theta = 90 degrees, past which it is D): the sphere is kept
// when D <= r' + rho or phi <= theta + asin((r' + rho) / D).  Angles are taken with atan2(|x cross y|, x . y), accurate near 0.
//
// Rounding: the reductions and this test are fp32, so everything carries margins far above the few ulps either can be off by:
// the radius is inflated by a relative 1e-4 of itself and of D and by 1e-5 of the coordinate scale (|O| + rho), rho and theta by
// a relative 1e-4 and 1e-4 rad.  Degenerate bundles keep everything: a direction that is zero, infinite or NaN, an origin that is
// not finite, directions that do not add up to a clear axis, and theta of 90 degrees or more.  tests/host/test_reflect_bound.cpp
// checks the bound against float64 ray-to-ball distances over millions of random cases.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_REFLECT_HD __host__ __device__
#else
#define RTX_REFLECT_HD
#endif

namespace rtxreflect {

constexpr float kAngleMargin = 1.0e-4f; // rad
constexpr float kRelMargin = 1.0e-4f;
constexpr float kKappa = 2.0e-6f;
constexpr float kHalfPi = 1.57079632679f;

struct Bundle {
    float ox, oy, oz; // centre of the origins' ball
    float rho;        // its radius, margin included
    float ax, ay, az; // unit cone axis
    float theta;      // half-angle, margin included
    float slack;      // absolute radius inflation: the rounding of points at this coordinate scale
    bool all;         // degenerate: every sphere is kept
};

RTX_REFLECT_HD inline float angle_between(float ax, float ay, float az, float bx, float by, float bz)
{
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return atan2f(sqrtf(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);
}

// Step 1, per ray: the unit direction, and whether the ray is degenerate (zero, infinite or NaN direction, or origin not finite).
RTX_REFLECT_HD inline bool unit_direction(const float P[3], const float R[3], float u[3])
{
    const float len = sqrtf(R[0] * R[0] + R[1] * R[1] + R[2] * R[2]);
    const float scale = fabsf(P[0]) + fabsf(P[1]) + fabsf(P[2]);
    if (!(len > 1.0e-30f) || !(len < 3.0e38f) || !(scale < 3.0e37f)) {
        u[0] = u[1] = u[2] = 0.0f;
        return false;
    }
    u[0] = R[0] / len;
    u[1] = R[1] / len;
    u[2] = R[2] / len;
    return true;
}

// Step 2: the ball's centre from the sum of n origins, and the cone's axis from the sum of their unit directions.  A direction
// sum shorter than a tenth of n has no clear axis: the caller keeps everything.
RTX_REFLECT_HD inline void centre_from_sum(float sx, float sy, float sz, float n, float o[3])
{
    o[0] = sx / n;
    o[1] = sy / n;
    o[2] = sz / n;
}

RTX_REFLECT_HD inline bool axis_from_sum(float sx, float sy, float sz, float n, float a[3])
{
    const float len = sqrtf(sx * sx + sy * sy + sz * sz);
    if (!(len > 0.1f * n)) return false;
    a[0] = sx / len;
    a[1] = sy / len;
    a[2] = sz / len;
    return true;
}

// Step 3, per ray: its origin's distance from the centre and its direction's angle from the axis (the workgroup keeps the largest).
RTX_REFLECT_HD inline float distance_from_centre(const float o[3], const float P[3])
{
    const float dx = P[0] - o[0], dy = P[1] - o[1], dz = P[2] - o[2];
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

RTX_REFLECT_HD inline float angle_from_axis(const float a[3], const float u[3]) { return angle_between(a[0], a[1], a[2], u[0], u[1], u[2]); }

// Step 4: the bundle from the reductions (centre, axis, the largest distance and angle; any degenerate ray).
RTX_REFLECT_HD inline Bundle make_bundle(const float o[3], const float a[3], float max_dist, float max_angle, bool degenerate)
{
    Bundle b;
    b.ox = o[0];
    b.oy = o[1];
    b.oz = o[2];
    b.ax = a[0];
    b.ay = a[1];
    b.az = a[2];
    b.rho = max_dist * (1.0f + kRelMargin);
    b.theta = max_angle * (1.0f + kRelMargin) + kAngleMargin;
    b.slack = 1.0e-5f * (fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2]) + b.rho);
    b.all = degenerate || !(b.theta < kHalfPi) || !(b.slack < 3.0e37f);
    return b;
}

// May sphere (C, r) be hit by a ray of the bundle?  false: by none of them.
RTX_REFLECT_HD inline bool may_hit(const Bundle& b, float cx, float cy, float cz, float r)
{
    if (b.all) return true;
    const float vx = cx - b.ox, vy = cy - b.oy, vz = cz - b.oz;
    const float D = sqrtf(vx * vx + vy * vy + vz * vz);
    const float far = D + b.rho; // >= |P - C| for every origin P of the bundle
    const float re = sqrtf(r * r * (1.0f + kKappa) + kKappa * (far * far));
    const float R = re * (1.0f + kRelMargin) + kRelMargin * D + b.rho + b.slack;
    if (!(D > R)) return true; // the ball reaches into the (inflated) sphere, or NaN
    const float phi = angle_between(b.ax, b.ay, b.az, vx, vy, vz);
    const float beta = asinf(R / D);
    return phi <= b.theta + beta + kAngleMargin;
}

} // namespace rtxreflect
