// rtx_refract.hpp -- the glass of rtx_scene_set_refraction, for host and device alike: which values the call accepts, and THE RULE
// (include/rtx.h, rtx_scene_set_refraction) as code, once: through_sphere, the ray that leaves a solid sphere a ray has entered.
// secondary_ray (rtx_tile_pass.inc) calls it on the device with sqrt_cr / rcp_cr; tests/host/test_refract.cpp runs the very same
// expressions on the host with sqrtf and 1.0f / x against a float64 statement of two Snell refractions and a chord.  The root
// and the reciprocal are passed in: both must be correctly rounded.  No HIP header is needed.  Must be compiled with
// -ffp-contract=off, as everything that is compared bit for bit.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define RTX_REFRACT_HD __host__ __device__
#else
#define RTX_REFRACT_HD
#endif

namespace rtxrefract {

constexpr float kMaxIor = 4.0f;

// What rtx_scene_set_refraction accepts of one value: 0 (a mirror), or a finite value in [1, kMaxIor].  A NaN fails every test.
RTX_REFRACT_HD inline bool ior_ok(float v) { return v == 0.0f || (v >= 1.0f && v <= kMaxIor); }

// A whole call: NULL for a good one, else what is wrong with it; *bad (if given) the first bad value, or n.
inline const char* values_fault(size_t n, const float* ior, size_t* bad = nullptr)
{
    if (bad) *bad = n;
    if (n != 0 && ior == nullptr) return "ior is NULL";
    for (size_t i = 0; i < n; i++) {
        if (!ior_ok(ior[i])) {
            if (bad) *bad = i;
            return "every value must be 0, or finite and in [1, 4]";
        }
    }
    return nullptr;
}

RTX_REFRACT_HD inline float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The ray (o, d) that leaves a solid sphere of radius r and index ior which a ray entered at P, N the unit normal there and V the
// unit vector back along the incoming ray: refract at entry (T, the unit direction inside), follow the chord of length L =
// 2 r ct, and mirror V in the plane perpendicular to T -- the path is symmetric about the plane through the centre
// perpendicular to T, so the exit direction needs no second Snell step and the exit point no intersection test.  ior >= 1: no
// total internal reflection.  A NaN c2 gives ct = 0.
template <class Sqrt, class Rcp>
RTX_REFRACT_HD inline void through_sphere(const float P[3], const float N[3], const float V[3], float r, float ior, Sqrt root, Rcp recip, float o[3], float d[3])
{
    const float ci = dot3(N, V);
    const float eta = recip(ior); // = 1.0f / ior
    const float s2 = (eta * eta) * (1.0f - ci * ci);
    const float c2 = 1.0f - s2;
    const float ct = root(c2 > 0.0f ? c2 : 0.0f);
    const float g = eta * ci - ct;
    float T[3];
    for (int q = 0; q < 3; q++) T[q] = N[q] * g - V[q] * eta;
    const float L = (2.0f * r) * ct;
    for (int q = 0; q < 3; q++) o[q] = P[q] + T[q] * L;
    const float m = 2.0f * dot3(T, V);
    for (int q = 0; q < 3; q++) d[q] = V[q] - T[q] * m;
}

} // namespace rtxrefract
