// rtx_lights.hpp -- the light set of rtx_scene_set_lights on the host: validation of a set and its packing into the block that
// travels by value in the arguments of rtx_lights_shade / rtx_lights_reflect_shade (rtx_lights_kernels.inc), and the same for the
// cones of rtx_scene_set_spots (spot_fault, spots_fault, pack_spot; the rule itself is rtx_spot.hpp's).  Pure host code, no
// HIP types, so that tests/host/test_lights_pack.cpp can run it under ASan / UBSan.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtx.h"
#include "rtx_spot.hpp"

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

// ---- the cones of rtx_scene_set_spots (the rule: rtx_spot.hpp)

constexpr double kSpotMinLen2 = 0x1p-40, kSpotMaxLen2 = 0x1p40; // the squared length of a dir, formed in double
constexpr float kSpotMinBand = 0x1p-10f;                        // cos_inner - cos_outer at least: inv at most 1024

inline bool spot_is_point(const rtx_spot& s) { return s.dir[0] == 0.0f && s.dir[1] == 0.0f && s.dir[2] == 0.0f; }

inline double spot_len2(const rtx_spot& s)
{
    const double x = (double)s.dir[0], y = (double)s.dir[1], z = (double)s.dir[2];
    return x * x + y * y + z * z;
}

// What rtx_scene_set_spots accepts of one cone.  Returns NULL for a good one (a point light's cosines are not looked at), else what
// is wrong with it.
inline const char* spot_fault(const rtx_spot& s)
{
    if (spot_is_point(s)) return nullptr;
    for (int k = 0; k < 3; k++) {
        if (!isfinite(s.dir[k])) return "dir must be finite";
    }
    const double len2 = spot_len2(s);
    if (!(len2 >= kSpotMinLen2 && len2 <= kSpotMaxLen2)) return "the squared length of dir must lie in [2^-40, 2^40]";
    if (!isfinite(s.cos_outer) || !isfinite(s.cos_inner)) return "the cosines must be finite";
    if (s.cos_outer < -1.0f) return "cos_outer is below -1";
    if (s.cos_inner > 1.0f) return "cos_inner is above 1";
    const float band = s.cos_inner - s.cos_outer;
    if (band < kSpotMinBand) return "cos_inner - cos_outer must be at least 2^-10";
    return nullptr;
}

// A whole call for a set of n_lights lights: n is n_lights or 0, a list unless n is 0, every cone good.  *bad (if given) receives
// the position of the first bad cone, or n when the fault is the count or the list itself.
inline const char* spots_fault(size_t n_lights, size_t n, const rtx_spot* spots, size_t* bad = nullptr)
{
    if (bad) *bad = n;
    if (n != 0 && n != n_lights) return "n must be the number of lights in the set, or 0";
    if (n != 0 && spots == nullptr) return "spots is NULL";
    for (size_t i = 0; i < n; i++) {
        const char* f = spot_fault(spots[i]);
        if (f) {
            if (bad) *bad = i;
            return f;
        }
    }
    return nullptr;
}

// A validated cone as it is stored: the axis normalised in double, inv by one fp32 division.  A point light: all zero.
inline rtxspot::Packed pack_spot(const rtx_spot& s)
{
    if (spot_is_point(s)) return rtxspot::Packed{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const double len = sqrt(spot_len2(s));
    const float band = s.cos_inner - s.cos_outer;
    return rtxspot::Packed{(float)((double)s.dir[0] / len), (float)((double)s.dir[1] / len), (float)((double)s.dir[2] / len), s.cos_outer, s.cos_inner, 1.0f / band};
}

// ... and as rtx_scene_get_spots returns it.
inline rtx_spot stored_spot(const rtxspot::Packed& p) { return rtx_spot{{p.ax, p.ay, p.az}, p.cos_outer, p.cos_inner}; }

// Validates the call and packs it (n == 0: every light a point light).  All or nothing: a refused call leaves *dst as it was.
inline bool pack_spots(size_t n_lights, size_t n, const rtx_spot* spots, rtxspot::Block* dst)
{
    if (dst == nullptr || spots_fault(n_lights, n, spots) != nullptr) return false;
    rtxspot::Block b = {};
    for (size_t i = 0; i < n; i++) b.spot[i] = pack_spot(spots[i]);
    *dst = b;
    return true;
}

// The lights of the block that have a cone.
inline uint32_t spot_count(const rtxspot::Block& b)
{
    uint32_t c = 0;
    for (size_t i = 0; i < kMaxLights; i++) c += rtxspot::has_cone(b.spot[i]) ? 1u : 0u;
    return c;
}

} // namespace rtxlights
