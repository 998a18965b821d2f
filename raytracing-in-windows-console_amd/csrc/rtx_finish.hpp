// rtx_finish.hpp -- the surface finish of rtx_scene_set_finish, for host and device alike: which values the call accepts, how they
// are stored, and THE RULE (include/rtx.h, rtx_scene_set_finish) as code, once: power (the Blinn-Phong exponent 2^m by squaring),
// ambient and add_terms (where ka, kd and ks enter a pixel's colour).  shade_light and add_light (rtx_device.hpp,
// rtx_lights_kernels.inc) call them on the device; tests/host/test_finish.cpp runs the very same expressions on the host.  No HIP
// header is needed.  Must be compiled with -ffp-contract=off, as everything that is compared bit for bit.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rtx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define RTX_FINISH_HD __host__ __device__
#else
#define RTX_FINISH_HD
#endif

namespace rtxfinish {

constexpr float kMaxWeight = 16.0f;
constexpr uint32_t kMaxShininessLog2 = 8u;

// What every new object has: the reference's call-site constants (RayTracing.cu:143-157, pow(x, 32.0f) of RayTracing.cu:73).
RTX_FINISH_HD inline rtx_finish default_finish() { return rtx_finish{0.2f, 1.0f, 1.0f, 5u}; }

// What rtx_scene_set_finish accepts of one weight: finite, in [0, kMaxWeight] (-0 included).  A NaN fails every test.
RTX_FINISH_HD inline bool weight_ok(float v) { return v >= 0.0f && v <= kMaxWeight; }
inline bool finish_ok(const rtx_finish& f) { return weight_ok(f.ambient) && weight_ok(f.diffuse) && weight_ok(f.specular) && f.shininess_log2 <= kMaxShininessLog2; }

// A whole call: NULL for a good one, else what is wrong with it; *bad (if given) the first bad finish, or n.
inline const char* values_fault(size_t n, const rtx_finish* finishes, size_t* bad = nullptr)
{
    if (bad) *bad = n;
    if (n != 0 && finishes == nullptr) return "finishes is NULL";
    for (size_t i = 0; i < n; i++) {
        if (!finish_ok(finishes[i])) {
            if (bad) *bad = i;
            return "ambient, diffuse and specular must be finite and in [0, 16], shininess_log2 at most 8";
        }
    }
    return nullptr;
}

// As it is stored: -0 becomes +0, so that equal finishes are equal bytes.
inline rtx_finish stored(const rtx_finish& f)
{
    return rtx_finish{f.ambient > 0.0f ? f.ambient : 0.0f, f.diffuse > 0.0f ? f.diffuse : 0.0f, f.specular > 0.0f ? f.specular : 0.0f, f.shininess_log2};
}

inline bool is_default(const rtx_finish& f)
{
    const rtx_finish d = default_finish();
    return memcmp(&f, &d, sizeof d) == 0;
}

// x^(2^m): m squarings in double, rounded once to float.  m = 5 is pow32 (rtx_device.hpp) bit for bit, m = 0 is x.  x in [0, 1]
// and m <= 8: the double neither overflows nor, above 2^-1074, loses the value before the one rounding.
RTX_FINISH_HD inline float power(float x, uint32_t m)
{
    double d = (double)x;
    for (uint32_t s = 0; s < m && s < kMaxShininessLog2; s++) d = d * d;
    return (float)d;
}

// res_q = ka * od_q: a pixel's colour before the first light.
RTX_FINISH_HD inline float ambient(float ka, float od) { return ka * od; }

// res_q = (res_q + (diffuse_iq * kd) * od_q) + specular_iq * ks: one light's terms, as add_light and shade_light form them.
RTX_FINISH_HD inline float add_terms(float res, float diffuse, float kd, float od, float specular, float ks) { return (res + (diffuse * kd) * od) + specular * ks; }

} // namespace rtxfinish
