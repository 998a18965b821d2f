// rtx_lights_chain_kernels.inc -- the mirror path's third launch when mirrors see mirrors (RTX_OPT_REFLECT_DEPTH > 1, or
// RTX_OPT_REFLECT_DEPTH_CHECK 1), included into namespace rtx of rtx_kernels.hip after rtx_lights_kernels.inc, whose
// lights_shade_body and shade_lights it uses (the device functions the tile passes share: rtx_tile_pass.inc).  ONE shade family for
// any set of 1 .. 8 lights (the set by value, as rtx_lights_reflect_shade gets it; DESIGN.md 4.9: +6-8 % for one light, on a path
// nobody takes by default, for half the instantiations).
//
// Level 0 is lights_shade_body's work: the shadow test per light, one walk of the scene, local_0 = shade_lights with the pixel's
// dark lights at powers 0.  lights_chain_blend then walks the chain forward from the hits rtx_reflect_chain stored (level j at
// ra.hits + j * ca.px), rebuilding r_j with secondary_ray; local_j (j >= 1) = shade_lights of r_j at t_j with full powers for every
// light, in order, no shadow test (under RTX_OPT_REFLECT_SHADOWS: see below), black when level j hit nothing.  It keeps local_j and k_j for the at most 5 levels in
// registers (loops unrolled: no indexed array, no scratch), then folds from the deepest level inwards:
// C_j = local_j where level j + 1 does not exist, else minf(255.0f, local_j * (1.0f - k_j) + C_{j+1} * k_j) per component --
// reflect_blend's expression in its operation order.  With depth 1 this is reflect_blend over shade_lights operation for operation.

//
// RTX_OPT_REFLECT_SHADOWS: the blend takes a word per pixel, byte j - 1 the lights level j is shadowed from (rtx_chain_shadow's
// output), and local_j is shade_lights with those lights at powers 0.  It is written once: lights_chain_blend is the blend with the
// constant word 0 (the compiler folds the mask away: rtx_lights_chain_shade's code is what it was), rtx_lights_chain_shadow_shade
// the same body with the pixel's word.

template <bool FIN>
__device__ __forceinline__ V3 lights_chain_blend_dark(const KArgs& a, const LightsArgsOf<FIN>& la, const ReflectArgs& ra, const ChainArgs& ca, const PatternArgs& pa,
                                                      const Ray& ray, float distance, V3 normal, uint32_t id, V3 cl, size_t at, uint32_t deep_dark)
{
    V3 local[kMaxReflectDepth + 1];
    float kk[kMaxReflectDepth];
    local[0] = cl;
    Ray r = ray;
    float t = distance;
    V3 n = normal;
    uint32_t o = id;
    uint32_t deepest = 0u; // the deepest level that exists for this pixel
    bool alive = true;     // level j hit an object
#pragma unroll
    for (int j = 0; j < kMaxReflectDepth; j++) {
        kk[j] = 0.0f;
        local[j + 1] = v3(0.0f, 0.0f, 0.0f);
        if (alive && (uint32_t)j < ca.depth) {
            const float k = reflectivity_of(ra, o);
            alive = k > 0.0f;
            if (alive) {
                kk[j] = k;
                deepest = (uint32_t)j + 1u;
                r = secondary_ray(a, ra, r, t, n, o);
                const uint2 h = ra.hits[(size_t)(j + 1) * ca.px + at];
                alive = h.y != 0xffffffffu;
                if (alive) {
                    t = __uint_as_float(h.x);
                    o = h.y;
                    const Surface sf = surface_of(a, pa, h.y, add(r.o, mulf(r.d, t)));
                    n = sf.normal;
                    local[j + 1] = shade_lights_of<FIN>(pa, h.y, r, t, n, sf.od, la, (deep_dark >> (8 * j)) & 0xffu);
                }
            }
        }
    }
    V3 C = local[kMaxReflectDepth];
#pragma unroll
    for (int j = kMaxReflectDepth - 1; j >= 0; j--) {
        if ((uint32_t)j == deepest) {
            C = local[j];
        } else if ((uint32_t)j < deepest) {
            const float k = kk[j];
            const float w = 1.0f - k;
            C = v3(minf(255.0f, local[j].x * w + C.x * k), minf(255.0f, local[j].y * w + C.y * k), minf(255.0f, local[j].z * w + C.z * k));
        }
    }
    return C;
}

template <bool FIN>
__device__ __forceinline__ V3 lights_chain_blend(const KArgs& a, const LightsArgsOf<FIN>& la, const ReflectArgs& ra, const ChainArgs& ca, const PatternArgs& pa,
                                                 const Ray& ray, float distance, V3 normal, uint32_t id, V3 cl, size_t at)
{
    return lights_chain_blend_dark<FIN>(a, la, ra, ca, pa, ray, distance, normal, id, cl, at, 0u);
}

template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_lights_chain_shade(const KArgs a, const LightsArgsOf<FIN> la, const ReflectArgs ra, const ChainArgs ca, const PatternArgs pa)
{
    lights_shade_body<MODE, OUT, 2, false, FIN>(a, la, ra, ca, pa);
}

// The chain's shade launch under RTX_OPT_REFLECT_SHADOWS: rtx_lights_chain_shade with the deeper levels' dark lights (cs.dark).
template <int MODE, int OUT, bool FIN = false>
__global__ __launch_bounds__(kThreads) void rtx_lights_chain_shadow_shade(const KArgs a, const LightsArgsOf<FIN> la, const ReflectArgs ra, const ChainArgs ca,
                                                                          const ChainShadowArgs cs, const PatternArgs pa)
{
    lights_shade_body<MODE, OUT, 3, false, FIN>(a, la, ra, ca, pa, cs.dark);
}
