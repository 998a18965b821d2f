// test_plan_reflect_grid.cpp -- rtxplan::plan_shading and shading_wants_grid with RTX_OPT_REFLECT_GRID (csrc/rtx_plan.hpp), host only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/host/test_plan_reflect_grid.cpp -o test_plan_reflect_grid
// Over the full cross product of the ShadingRequest fields:
//   1. reflect_grid = false gives, field for field, the plan the planner gave before the option existed (restated below);
//   2. reflect_grid = true changes `secondary` only -- to kPassGridReflect -- and only while the option is in effect: the mirror
//      path, RTX_OPT_REFLECT_CHECK 0, a sphere in the scene, a usable grid;
//   3. shading_wants_grid is the OR of the two options' conditions, each by the options and the scene alone.
#include <cstdio>
#include <cstring>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

using namespace rtxplan;

static int g_failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (g_failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            g_failures++;                                           \
        }                                                           \
    } while (0)

// The planner before RTX_OPT_REFLECT_GRID, restated: what every frame with the option 0 must still be planned as.
struct Before {
    ShadePath path = kPathDirect;
    ShadePass secondary = kPassNone, shadow_pass = kPassNone;
    ShadeFamily family = kShadeFamilies;
    bool deep = false, dark0 = false, chain = false, wants_grid = false;
    uint32_t levels = 0, bytes_per_px = 0, deep_off = 0, dark0_off = 0;
};

static Before plan_before(const ShadingRequest& q)
{
    Before p;
    if (q.mode < kShadedModeLo || q.mode > kShadedModeHi) {
        p.path = kPathDirect;
    } else if (q.n_reflective != 0 || q.reflect_check == 2) {
        p.path = kPathMirror;
    } else if (q.shadows || q.n_lights != 1 || q.lights_check || !q.light0_is_reference) {
        p.path = kPathShaded;
    }
    p.wants_grid = p.path != kPathDirect && q.shadow_grid && q.shadows && q.shadow_check == 0 && q.ns != 0;
    if (p.path == kPathDirect) return p;
    const bool mirror = p.path == kPathMirror;
    const bool grid = p.wants_grid && q.grid_usable;
    const bool several = q.n_lights >= 2 || q.lights_check;
    p.deep = mirror && q.reflect_shadows && q.shadows && q.n_reflective != 0;
    p.chain = mirror && (q.reflect_depth > 1 || q.reflect_depth_check || p.deep);
    p.secondary = p.chain ? kPassReflectChain : (mirror ? kPassReflectHit : kPassNone);
    p.shadow_pass = grid ? kPassGridShadow : (p.deep ? kPassChainShadow : kPassNone);
    if (p.chain) {
        p.family = grid ? (p.deep ? kGridChainShadowShade : kGridChainShade) : (p.deep ? kLightsChainShadowShade : kLightsChainShade);
    } else if (mirror) {
        p.family = grid ? kGridReflectShade : (several ? kLightsReflectShade : kReflectShade);
    } else {
        p.family = grid ? kGridShade : (several ? kLightsShade : kShadowShade);
    }
    p.dark0 = grid;
    p.levels = p.chain ? q.reflect_depth + 1u : (mirror ? 2u : 1u);
    p.deep_off = 8u * p.levels;
    p.dark0_off = p.deep_off + (p.deep ? 4u : 0u);
    p.bytes_per_px = p.dark0_off + (p.dark0 ? 4u : 0u);
    return p;
}

// every field but `secondary`
static bool same_but_secondary(const ShadingPlan& p, const Before& b)
{
    return p.path == b.path && p.shadow_pass == b.shadow_pass && p.family == b.family && p.deep == b.deep && p.dark0 == b.dark0 && p.levels == b.levels &&
           p.bytes_per_px == b.bytes_per_px && p.deep_off == b.deep_off && p.dark0_off == b.dark0_off && p.chain() == b.chain;
}

int main()
{
    static_assert(kPassNone == 0 && kPassReflectHit == 1 && kPassReflectChain == 2 && kPassChainShadow == 3 && kPassGridShadow == 4 && kPassGridReflect == 5 &&
                      kShadePasses == 6,
                  "the passes keep their numbers; the new one is the last");
    size_t n = 0, n_effect = 0, n_effect_depth1 = 0, n_effect_chain = 0, n_both = 0, n_wants_mirror_only = 0;
    ShadingRequest q;
    for (q.mode = -1; q.mode < 7; q.mode++)
    for (int shadows = 0; shadows < 2; shadows++)
    for (q.shadow_check = 0; q.shadow_check < 3; q.shadow_check++)
    for (int lights_check = 0; lights_check < 2; lights_check++)
    for (int lights = 0; lights < 3; lights++) // one reference / one other / two
    for (q.n_reflective = 0; q.n_reflective < 2; q.n_reflective++)
    for (q.reflect_check = 0; q.reflect_check < 3; q.reflect_check++)
    for (q.reflect_depth = 1; q.reflect_depth <= 4; q.reflect_depth++)
    for (int bits = 0; bits < 32; bits++) {
        q.shadows = shadows != 0;
        q.lights_check = lights_check != 0;
        q.n_lights = lights == 2 ? 2 : 1;
        q.light0_is_reference = lights == 0;
        q.reflect_depth_check = (bits & 1) != 0;
        q.reflect_shadows = (bits & 2) != 0;
        q.shadow_grid = (bits & 4) != 0;
        q.grid_usable = (bits & 8) != 0;
        q.ns = (bits & 16) ? 1u : 0u;
        const Before b = plan_before(q);
        n++;

        // 1. the option off: the plan of before, field for field
        q.reflect_grid = false;
        const ShadingPlan off = plan_shading(q);
        CHECK(same_but_secondary(off, b) && off.secondary == b.secondary && !off.grid_reflect());
        CHECK(shading_wants_grid(q) == b.wants_grid);
        CHECK(shadows_want_grid(q) == b.wants_grid && !mirrors_want_grid(q));

        // 2. the option on: `secondary` alone, and only while in effect
        q.reflect_grid = true;
        const ShadingPlan on = plan_shading(q);
        const bool mirrors_want = b.path == kPathMirror && q.reflect_check == 0 && q.ns != 0;
        const bool in_effect = mirrors_want && q.grid_usable;
        CHECK(same_but_secondary(on, b));
        CHECK(on.secondary == (in_effect ? kPassGridReflect : b.secondary));
        CHECK(on.grid_reflect() == in_effect);
        CHECK(!in_effect || (b.secondary == kPassReflectHit || b.secondary == kPassReflectChain)); // it stands in for one of the two
        // (what the launch reads of the plan: the levels it writes are the buffer's, one at depth 1 without the chain's layout)
        CHECK(!in_effect || on.levels - 1u == (b.chain ? q.reflect_depth : 1u));

        // 3. the grid is asked for when either option wants it
        CHECK(mirrors_want_grid(q) == mirrors_want);
        CHECK(shadows_want_grid(q) == b.wants_grid);
        CHECK(shading_wants_grid(q) == (b.wants_grid || mirrors_want));
        ShadingRequest flipped = q; // ... by the options and the scene alone: not by whether the grid turned out usable
        flipped.grid_usable = !q.grid_usable;
        CHECK(shading_wants_grid(flipped) == shading_wants_grid(q));

        n_effect += in_effect ? 1 : 0;
        n_effect_depth1 += in_effect && !b.chain ? 1 : 0;
        n_effect_chain += in_effect && b.chain ? 1 : 0;
        n_both += in_effect && on.dark0 ? 1 : 0;
        n_wants_mirror_only += mirrors_want && !b.wants_grid ? 1 : 0;
    }
    CHECK(n == 8u * 2 * 3 * 2 * 3 * 2 * 3 * 4 * 32);
    // the product is not empty where it matters
    CHECK(n_effect > 1000 && n_effect_depth1 > 100 && n_effect_chain > 1000 && n_both > 100 && n_wants_mirror_only > 1000);
    if (g_failures != 0) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("all reflect-grid planning tests passed (%zu requests, %zu with the option in effect)\n", n, n_effect);
    return 0;
}
