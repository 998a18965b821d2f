// rtx_spot.hpp -- the cone of a spot light (rtx_scene_set_spots), for host and device alike: how a cone is stored and THE RULE
// (include/rtx.h, rtx_scene_set_spots) as code, once: edge (the clamped position s of a direction between the outer and the inner
// cosine), weight (the smoothstep w the light's two powers are multiplied by) and outside (the pre-test of the shadow passes: s
// is not above 0, so the light gives nothing there and no segment is tested).  add_light, shade_light and shadowed_before_spheres
// (rtx_lights_kernels.inc, rtx_device.hpp, rtx_tile_pass.inc) call them on the device; tests/host/test_spot.cpp runs the very
// same expressions on the host.  What a call accepts and the packing are rtx_lights.hpp's.  No HIP header is needed.  Must be
// compiled with -ffp-contract=off, as everything that is compared bit for bit.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rtx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define RTX_SPOT_HD __host__ __device__
#else
#define RTX_SPOT_HD
#endif

namespace rtxspot {

// One cone as it is stored and as the kernels read it: the unit axis, the two cosines and inv = 1.0f / (cos_inner - cos_outer).
// A point light is all zero; a cone has inv in [0.5, 1024], never 0.  24 bytes.
struct Packed {
    float ax, ay, az;
    float cos_outer, cos_inner;
    float inv;
};

// The cones of a light set, by light: what travels by value beside rtxlights::Block in the arguments of the launches that read
// cones.  192 bytes.
struct Block {
    Packed spot[RTX_MAX_LIGHTS];
};

RTX_SPOT_HD inline bool has_cone(const Packed& p) { return p.inv != 0.0f; }

// s of the rule for the unit direction ld from the point to the light: 0 at and beyond the outer cosine, 1 at and within the inner
// one.  A NaN x fails `x > 0.0f` and gives 0.
RTX_SPOT_HD inline float edge(const Packed& p, float ldx, float ldy, float ldz)
{
    const float m = (p.ax * ldx + p.ay * ldy) + p.az * ldz;
    const float c = -m;
    const float x = (c - p.cos_outer) * p.inv;
    return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
}

// w of the rule from s.
RTX_SPOT_HD inline float smooth(float s) { return (s * s) * (3.0f - 2.0f * s); }

// w of light `p` towards ld: what its two powers are multiplied by.  A point light: exactly 1.
RTX_SPOT_HD inline float weight(const Packed& p, float ldx, float ldy, float ldz) { return has_cone(p) ? smooth(edge(p, ldx, ldy, ldz)) : 1.0f; }

// The pre-test: the light gives nothing towards ld (w = 0 because s is not above 0).  Never true where the rule's s is above 0.
RTX_SPOT_HD inline bool outside(const Packed& p, float ldx, float ldy, float ldz) { return has_cone(p) && !(edge(p, ldx, ldy, ldz) > 0.0f); }

} // namespace rtxspot
