// rtx_lights.hpp -- the light set of rtx_scene_set_lights on the host: validation of a set and its packing into the block that
// travels by value in the arguments of rtx_lights_shade / rtx_lights_reflect_shade (rtx_lights_kernels.inc).  Pure host code, no
// HIP types, so that tests/host/test_lights_pack.cpp can run it under ASan / UBSan.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtx.h"

namespace rtxlights {

constexpr size_t kMaxLights = RTX_MAX_LIGHTS;

// One light as the kernels read it (the layout of KLight, rtx_kernels.h): 44 bytes.
struct PackedLight {
    float px, py, pz;
    float dr, dg, db, dpow;
    float sr, sg, sb, spow;
};

// The kernel argument block: the count and kMaxLights lights, the unused ones all zero.
struct Block {
    uint32_t n;
    PackedLight light[kMaxLights];
};

// What rtx_scene_set_light accepts: every value finite, no negative power, no negative colour component.
// Returns NULL for a good light, else what is wrong with it.
inline const char* light_fault(const rtx_light& l)
{
    const float v[11] = {l.pos[0], l.pos[1], l.pos[2], l.diffuse_rgb[0], l.diffuse_rgb[1], l.diffuse_rgb[2], l.diffuse_power,
                         l.specular_rgb[0], l.specular_rgb[1], l.specular_rgb[2], l.specular_power};
    for (int k = 0; k < 11; k++) {
        if (!isfinite(v[k])) return "every value must be finite";
    }
    for (int k = 0; k < 3; k++) {
        if (l.diffuse_rgb[k] < 0.0f || l.specular_rgb[k] < 0.0f) return "negative colour";
    }
    if (l.diffuse_power < 0.0f || l.specular_power < 0.0f) return "negative power";
    return nullptr;
}

// A whole set: n in [1, kMaxLights], a list, every light good.  *bad (if given) receives the position of the first bad light, or
// n when the fault is the count or the list itself.
inline const char* set_fault(size_t n, const rtx_light* lights, size_t* bad = nullptr)
{
    if (bad) *bad = n;
    if (n == 0 || n > kMaxLights) return "n must be in [1, RTX_MAX_LIGHTS]";
    if (lights == nullptr) return "lights is NULL";
    for (size_t i = 0; i < n; i++) {
        const char* f = light_fault(lights[i]);
        if (f) {
            if (bad) *bad = i;
            return f;
        }
    }
    return nullptr;
}

inline PackedLight pack_light(const rtx_light& l)
{
    return PackedLight{l.pos[0], l.pos[1], l.pos[2], l.diffuse_rgb[0], l.diffuse_rgb[1], l.diffuse_rgb[2], l.diffuse_power,
                       l.specular_rgb[0], l.specular_rgb[1], l.specular_rgb[2], l.specular_power};
}

// Validates the set and packs it, in the order given.  All or nothing: a refused set leaves *dst as it was.
inline bool pack(size_t n, const rtx_light* lights, Block* dst)
{
    if (dst == nullptr || set_fault(n, lights) != nullptr) return false;
    Block b = {};
    b.n = (uint32_t)n;
    for (size_t i = 0; i < n; i++) b.light[i] = pack_light(lights[i]);
    *dst = b;
    return true;
}

} // namespace rtxlights
