// rtx_unit.hpp -- the scale factor that re-normalising an already normalised vector multiplies by, as an integer rule.
// Plain C++ (no HIP builtins): included by the device code (rtx_device.hpp: unit_rescale) and by the host proof
// (tests/host/test_unit_rescale.cpp).
//
// Normalize_GPU (MyMath.h:139-145) scales by RN(1 / RN(sqrt(len2))).  The reference normalises several vectors twice
// (RayTracing.cu:52, 129; BlinnPhongShading's viewDir), and the squared length of a vector that fp32 has just normalised
// lies within a few ulps of 1.0f.  There the factor depends only on the bit offset k = bits(len2) - bits(1.0f), taken as
// a signed integer:
//   k >= 0:  len2 = 1 + k 2^-23.  sqrt = 1 + k 2^-24 - ..., which rounds to 1 + (k >> 1) 2^-23 (for odd k the root lies just
//            below the midpoint); its reciprocal 1 - (k >> 1) 2^-23 + ... rounds to 1 - (k & ~1) 2^-24.
//   k <  0:  len2 = 1 - j 2^-24, j = -k.  sqrt rounds to 1 - ((j + 1) >> 1) 2^-24; its reciprocal rounds to 1 + ((j + 3) >> 2) 2^-23.
// The rule is exact for k in [-8190, +2897] (second-order terms break it at -8191 and +2898); the window used is a small
// part of that.  tests/host/test_unit_rescale.cpp checks every k of the window and a margin against 1.0f / sqrtf(x);
// tests/gpu_checks/unit_check.hip checks unit_rescale() for all 2^32 inputs.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RTX_UNIT_HD __host__ __device__
#else
#define RTX_UNIT_HD
#endif

namespace rtx {

constexpr uint32_t kUnitOneBits = 0x3f800000u;  // 1.0f
// The window: what the table holds.  200 million random vectors normalised in fp32 gave k in [-7, +3] (61 % on 0 and +1).
constexpr int32_t kUnitKMin = -12, kUnitKMax = 3;
constexpr uint32_t kUnitEntries = (uint32_t)(kUnitKMax - kUnitKMin + 1);
static_assert(kUnitEntries == 16u, "the table is indexed with a 4-bit mask and takes 64 bytes of LDS");
// where the rule itself stops being true (the window must stay inside)
constexpr int32_t kUnitRuleMin = -8190, kUnitRuleMax = 2897;
static_assert(kUnitKMin >= kUnitRuleMin && kUnitKMax <= kUnitRuleMax, "window outside the rule's range");

// bits of RN(1 / RN(sqrt(x))) for bits(x) = bits(1.0f) + k, kUnitRuleMin <= k <= kUnitRuleMax
RTX_UNIT_HD constexpr uint32_t unit_rescale_bits(int32_t k)
{
    return k >= 0 ? kUnitOneBits - (uint32_t)(k & ~1) : kUnitOneBits + (uint32_t)((3 - k) >> 2);
}
static_assert(unit_rescale_bits(-8) == 0x3f800002u && unit_rescale_bits(-5) == 0x3f800002u && unit_rescale_bits(-4) == 0x3f800001u &&
              unit_rescale_bits(-1) == 0x3f800001u && unit_rescale_bits(0) == 0x3f800000u && unit_rescale_bits(1) == 0x3f800000u &&
              unit_rescale_bits(2) == 0x3f7ffffeu && unit_rescale_bits(3) == 0x3f7ffffeu, "unit rescale rule");

// The same offset k fixes another function of a ray's squared length a: divTwoA = RN(1 / RN(2 a)) of RayTracing.cu:93.
//   k >= 0:  2a = 2 + k 2^-22 exactly; 1 / (2a) = 1/2 - k 2^-24 + k^2 2^-47 - ..., and below 1/2 the spacing is 2^-25: the first
//            two terms are 2k steps down from 1/2, the third is far below half a step.
//   k <  0:  2a = 2 - j 2^-23, j = -k; 1 / (2a) = 1/2 + j 2^-25 + j^2 2^-49 + ..., and above 1/2 the spacing is 2^-24: j / 2 steps
//            up; for odd j the second-order term puts the value on the upper side of the tie: (j + 1) >> 1.
// The rule is exact for k in [-4095, +1448] (tests/host/test_half_recip.cpp finds both ends against 1.0f / (2.0f * x));
// tests/gpu_checks/half_check.hip checks half_recip() of rtx_device.hpp for all 2^32 inputs.
constexpr uint32_t kHalfBits = 0x3f000000u; // 0.5f
constexpr int32_t kHalfRuleMin = -4095, kHalfRuleMax = 1448;
static_assert(kUnitKMin >= kHalfRuleMin && kUnitKMax <= kHalfRuleMax, "window outside the half-reciprocal rule's range");

// bits of RN(1 / RN(2 x)) for bits(x) = bits(1.0f) + k, kHalfRuleMin <= k <= kHalfRuleMax
RTX_UNIT_HD constexpr uint32_t half_recip_bits(int32_t k)
{
    return k >= 0 ? kHalfBits - 2u * (uint32_t)k : kHalfBits + (uint32_t)((1 - k) >> 1);
}
static_assert(half_recip_bits(0) == 0x3f000000u && half_recip_bits(1) == 0x3efffffeu && half_recip_bits(3) == 0x3efffffau &&
              half_recip_bits(-1) == 0x3f000001u && half_recip_bits(-2) == 0x3f000001u && half_recip_bits(-3) == 0x3f000002u &&
              half_recip_bits(-12) == 0x3f000006u, "half-reciprocal rule");

// Table slot of a squared length, from its bits: below kUnitEntries inside the window; everything else -- including
// negative values, zeros, infinities and NaNs -- wraps to a large unsigned number.
RTX_UNIT_HD constexpr uint32_t unit_slot(uint32_t len2_bits) { return len2_bits - (kUnitOneBits + (uint32_t)kUnitKMin); }
static_assert(unit_slot(0x3f800000u) == 12u && unit_slot(0x3f800003u) == 15u && unit_slot(0x3f800004u) >= kUnitEntries &&
              unit_slot(0x3f7ffff4u) == 0u && unit_slot(0x3f7ffff3u) >= kUnitEntries && unit_slot(0u) >= kUnitEntries &&
              unit_slot(0xbf800000u) >= kUnitEntries && unit_slot(0x7f800000u) >= kUnitEntries && unit_slot(0x7fc00000u) >= kUnitEntries,
              "unit window");

} // namespace rtx
