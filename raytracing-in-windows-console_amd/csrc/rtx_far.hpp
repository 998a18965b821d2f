// rtx_far.hpp -- the far distance folded into a table plane's direction test.
// Plain C++ (no HIP builtins): included by the device code (rtx_trace_body.inc, where wave 0 builds the LDS plane table) and by
// the host proof (tests/host/test_far_threshold.cpp).
//
// Plane::Trace (Plane.cu:38-72) leaves a ray when dn = Dot(direction, n) has dn > 0 or |dn| < FLT_EPSILON, and otherwise divides:
// t1 = num / dn, num = Dot(planePos - origin, n).  Both exits together are dn > -FLT_EPSILON (kDirCut), and a NaN dn takes
// neither form.  A pixel whose closest hit has distance > far is written as the miss record (RayTracing.cu:207), so in the
// kernels whose only consumer of a pixel is that gate, a lane whose plane hit PROVABLY has t1 > far may leave the plane too:
//   * if a nearer object wins, the plane did not matter;
//   * if the plane would have won, the pixel was a miss; without it the winner is farther still (a miss) or nothing
//     (distance kNoHit = 99999999.f, a miss because the rule asks for far < kNoHit).
// The rule: for num < 0 and FLT_MIN <= far < kNoHit, with q = RN(-num / far) finite,
//     cut = min(kDirCut, -RN(q * (1 - 2^-21))),      and a lane leaves the plane when dn > cut.
// Proof that kDirCut >= dn > cut implies RN(num / dn) > far.  Write N = -num, T = -cut; the case T = FLT_EPSILON drops nothing
// new, so T > 2^-23, and then q >= T / ((1 - 2^-21)(1 + 2^-24)) is normal as T is: both roundings have relative error at most
// 2^-24 (N and far may be subnormal: a quotient's error is that of its one rounding).  So
//     |dn| < T <= (N / far) (1 + 2^-24)^2 (1 - 2^-21) < (N / far) (1 - 3 * 2^-23),
// since (1 + 2^-23 + 2^-48)(1 - 2^-21) = 1 - 2^-21 + 2^-23 - (2^-44 - 2^-48 + 2^-69).  Hence, in exact arithmetic,
//     num / dn = N / |dn| > far / (1 - 3 * 2^-23) > far (1 + 3 * 2^-23) > far + ulp(far) = nextafter(far),
// a normal far having ulp(far) <= 2^-23 far.  RN is monotonic and nextafter(far) is a float (or the overflow threshold, for
// far = FLT_MAX), so RN(num / dn) >= nextafter(far) > far; an overflowing quotient is +inf > far.  div_cr returns RN(num / dn)
// bit for bit (rtx_device.hpp).
// What the rule leaves to the parent's test (cut = kDirCut), because the argument above does not cover it:
//   * num >= 0 or NaN (no hit in front of the camera today, and none after);
//   * far NaN, <= 0, subnormal (nextafter(far) is then more than 2^-23 far away), +inf, or >= kNoHit;
//   * q = +inf (the quotient overflows: dn = -FLT_MAX can then give a t1 that rounds down to far itself);
//   * q so small that T <= FLT_EPSILON (this includes an underflowing quotient).
// tests/host/test_far_threshold.cpp checks the rule on a grid of (num, far) with windows of dn around every cut against the
// host's IEEE division; tests/gpu_checks/far_check.hip checks it beside div_cr over all 2^32 dn for chosen pairs.
#pragma once

#include <float.h>

#if defined(__HIPCC__)
#define RTX_FAR_HD __host__ __device__
#else
#define RTX_FAR_HD
#endif

namespace rtx {

// the parent's direction test as one compare: a lane leaves the plane when dn > kDirCut
constexpr float kDirCut = -1.1920928955078125e-7f; // -FLT_EPSILON
constexpr float kFarShrink = 0.999999523162841796875f; // 1 - 2^-21, exact in fp32
static_assert(kDirCut == -FLT_EPSILON && kFarShrink == 1.0f - 0x1.0p-21f, "constants of the far rule");
constexpr float kFarNoHit = 99999999.f; // RayTracing.h:21, the distance of a pixel that hit nothing (rtx_workgroup.hpp: kNoHit)

// The value a table plane's direction test compares dn with: kDirCut, or the far threshold where it is lower.  Never NaN.
RTX_FAR_HD inline float far_dir_cut(float num, float far)
{
    float cut = kDirCut;
    if (num < 0.0f && far >= FLT_MIN && far < kFarNoHit) {
        const float q = -num / far;
        if (q <= FLT_MAX) {
            const float thr = -(q * kFarShrink);
            if (thr < cut) cut = thr;
        }
    }
    return cut;
}

} // namespace rtx
