// rtx_pattern.hpp -- the checker patterns of rtx_scene_set_patterns, for host and device alike: the packed form of a table entry as
// the shade kernels read it, the validation of a table, and THE RULE (include/rtx.h, rtx_scene_set_patterns) as code, once:
// pattern_odd.  surface_of (rtx_tile_pass.inc) calls it on the device; tests/host/test_pattern.cpp runs the very same expression
// on the host against a float64 statement.  No HIP header is needed: a compiler without float4 gets a plain stand-in of its layout.
// Must be compiled with -ffp-contract=off, as everything that is compared bit for bit.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define RTX_PATTERN_HD __host__ __device__
namespace rtxpattern {
using Float4 = float4;
}
#else
#define RTX_PATTERN_HD
namespace rtxpattern {
struct alignas(16) Float4 {
    float x, y, z, w;
};
} // namespace rtxpattern
#endif

namespace rtxpattern {

constexpr size_t kMaxPatterns = RTX_MAX_PATTERNS;

// One table entry on the device, 48 bytes: three 16-byte loads from a table that stays in cache.
struct Entry {
    Float4 origin; // xyz; w unused (0)
    Float4 freq;   // xyz; w unused (0)
    Float4 od2;    // rgb / 255.0f; w unused (0)
};

// Is the hit point P in a cell of odd parity of the entry's lattice?  (A NaN anywhere is odd.)
RTX_PATTERN_HD inline bool pattern_odd(const float P[3], const Entry& e)
{
    const float ux = (P[0] - e.origin.x) * e.freq.x;
    const float uy = (P[1] - e.origin.y) * e.freq.y;
    const float uz = (P[2] - e.origin.z) * e.freq.z;
    const float f = (floorf(ux) + floorf(uy)) + floorf(uz);
    const float h = f - 2.0f * floorf(f * 0.5f);
    return h != 0.0f;
}

// What rtx_scene_set_patterns accepts of one entry: nine finite floats.
inline bool entry_ok(const rtx_pattern& p)
{
    for (int q = 0; q < 3; q++) {
        if (!isfinite(p.origin[q]) || !isfinite(p.freq[q]) || !isfinite(p.rgb[q])) return false;
    }
    return true;
}

// A whole table: NULL for a good one, else what is wrong with it; *bad (if given) the first bad entry, or n.
inline const char* table_fault(size_t n, const rtx_pattern* patterns, size_t* bad = nullptr)
{
    if (bad) *bad = n;
    if (n > kMaxPatterns) return "n must be in [0, RTX_MAX_PATTERNS]";
    if (n != 0 && patterns == nullptr) return "patterns is NULL";
    for (size_t i = 0; i < n; i++) {
        if (!entry_ok(patterns[i])) {
            if (bad) *bad = i;
            return "every value must be finite";
        }
    }
    return nullptr;
}

inline Entry pack_entry(const rtx_pattern& p)
{
    Entry e;
    e.origin.x = p.origin[0]; e.origin.y = p.origin[1]; e.origin.z = p.origin[2]; e.origin.w = 0.0f;
    e.freq.x = p.freq[0]; e.freq.y = p.freq[1]; e.freq.z = p.freq[2]; e.freq.w = 0.0f;
    // the division of rtx_scene_add_sphere / rtx_scene_add_plane (RayTracing.cu:144, hoisted)
    e.od2.x = p.rgb[0] / 255.0f; e.od2.y = p.rgb[1] / 255.0f; e.od2.z = p.rgb[2] / 255.0f; e.od2.w = 0.0f;
    return e;
}

} // namespace rtxpattern
