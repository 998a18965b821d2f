// rtx_shadow_kernels.inc -- the second launch of the light / shadow path (RTX_OPT_SHADOWS, rtx_scene_set_light), included into
// namespace rtx of rtx_kernels.hip.  The first launch is the trace kernel in its kOutHit form: the closest hit of every pixel, 8
// bytes (t, object).  This one shades from it.
//
// A 256-thread workgroup owns a 16 x 16 tile.  Every thread rebuilds its pixel's ray with the trace's own arithmetic (the
// per-column and per-row terms of ray_from_tables), the hit point and the normal exactly as the trace body does, so that with no
// pixel in shadow the records are the one-pass kernels' bit for bit.  The shadow test of a visible pixel (P, N) against the light
// L: self-shadow when N . (L - P) <= 0; else the open segment (P, L) against every plane (crossing inside the plane's x/z bounds)
// and every sphere (closer than r to the centre), the hit object excluded.  Spheres are culled per workgroup first: the waves
// reduce their unresolved hit points to a cone from the light (rtx_shadow.hpp), the scene is walked 512 spheres a step (two
// coalesced loads per thread, the next step requested ahead), and the spheres that may touch the cone are appended to a list in
// LDS (ballot + mbcnt, one LDS atomic per wave: the order does not matter to an any-hit test).  When the list is nearly full,
// and after the last step, every wave runs its unresolved pixels over it and leaves the loop as soon as none is left.
// A shadowed pixel is shaded with both powers at 0; everything is encoded by encode_and_store.

constexpr int kShadowTile = 16;       // pixels per side of a workgroup's tile
constexpr int kShadowList = 1024;     // occluder candidates held in LDS (20 KB with their positions)

// The body lives in rtx_shade_body.inc, included into the two entry points below.
template <int MODE, int OUT>
__global__ __launch_bounds__(kThreads) void rtx_shadow_shade(const KArgs a, const ShadowArgs sa)
{
    constexpr bool REFLECT = false;
    const ReflectArgs ra = {}; // (read only by the REFLECT parts, which are not compiled here)
#include "rtx_shade_body.inc"
}

// The mirror path's third launch (rtx_reflect_kernels.inc): rtx_shadow_shade's shading, then the blend.
template <int MODE, int OUT>
__global__ __launch_bounds__(kThreads) void rtx_reflect_shade(const KArgs a, const ShadowArgs sa, const ReflectArgs ra)
{
    constexpr bool REFLECT = true;
#include "rtx_shade_body.inc"
}
