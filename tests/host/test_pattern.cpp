// test_pattern.cpp -- the checker patterns of rtx_scene_set_patterns on the host (csrc/rtx_pattern.hpp, csrc/rtx_plan.hpp):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tests/host/test_pattern.cpp -o test_pattern
//   1. pattern_odd -- the very expression surface_of runs on the device -- against a float64 statement of the rule, on random
//      points at least 1e-3 of a cell away from every lattice plane (fp32 rounds u = (P - origin) * freq to within
//      |u| 2^-22 < 1e-4 here, so floor agrees there), and on the exact cases the rule names;
//   2. validation and packing of a table;
//   3. plan_shading over the cross product of the ShadingRequest fields: n_patterned = 0 gives the plan of before, field for
//      field (restated below); n_patterned = 1 in the reference's state is the light / shadow path with rtx_shadow_shade and 8
//      bytes per pixel; under any request that left the direct path already, nothing of the plan changes;
//   4. plan_removal with survivors_of: the slots move with the survivors under the renumbering rule.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_pattern.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

using namespace rtxplan;
using rtxpattern::Entry;
using rtxpattern::pattern_odd;

static int g_failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (g_failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            g_failures++;                                           \
        }                                                           \
    } while (0)

static Entry entry(float ox, float oy, float oz, float fx, float fy, float fz)
{
    const rtx_pattern p = {{ox, oy, oz}, {fx, fy, fz}, {10.0f, 20.0f, 30.0f}};
    return rtxpattern::pack_entry(p);
}

// ---------------------------------------------------------------- 1. the rule

static size_t test_against_float64()
{
    std::mt19937_64 rng(20240607u);
    std::uniform_real_distribution<double> pos(-100.0, 100.0), org(-5.0, 5.0), frq(-2.0, 2.0), coin(0.0, 1.0);
    size_t tested = 0, odd = 0, with_zero_axis = 0;
    for (int i = 0; i < 400000; i++) {
        float P[3], o[3], f[3];
        bool zero = false;
        for (int q = 0; q < 3; q++) {
            P[q] = (float)pos(rng);
            o[q] = (float)org(rng);
            f[q] = coin(rng) < 0.2 ? 0.0f : (float)frq(rng);
            zero = zero || f[q] == 0.0f;
        }
        // float64: the cell of the point, and how far it is from the cell's faces
        bool clear = true;
        double sum = 0.0;
        for (int q = 0; q < 3; q++) {
            if (f[q] == 0.0f) continue; // (the axis does not count: u = +-0)
            const double u = ((double)P[q] - (double)o[q]) * (double)f[q];
            const double fl = std::floor(u);
            if (u - fl < 1.0e-3 || fl + 1.0 - u < 1.0e-3) clear = false;
            sum += fl;
        }
        if (!clear) continue;
        const bool want = std::fmod(std::fabs(sum), 2.0) != 0.0;
        const bool got = pattern_odd(P, entry(o[0], o[1], o[2], f[0], f[1], f[2]));
        CHECK(got == want);
        tested++;
        odd += want ? 1 : 0;
        with_zero_axis += zero ? 1 : 0;
    }
    // the sample is not empty where it matters
    CHECK(tested > 300000 && odd > tested / 3 && odd < 2 * tested / 3 && with_zero_axis > 50000);
    return tested;
}

static void test_exact_cases()
{
    const Entry unit = entry(0, 0, 0, 1, 1, 1), floor_xz = entry(0, 0, 0, 1, 0, 1);
    const float a[3] = {-0.5f, 0.5f, 0.5f}; // floorf(-0.5f) = -1: odd
    CHECK(pattern_odd(a, unit));
    const float b[3] = {-0.5f, -0.5f, 0.5f};
    CHECK(!pattern_odd(b, unit));
    const float c[3] = {-1.5f, 0.5f, 0.5f}; // -2: even
    CHECK(!pattern_odd(c, unit));
    // freq = 0 with a negative P: (P - 0) * 0 = -0, floorf(-0) = -0, which adds nothing
    const float d[3] = {0.5f, -7.3f, 0.5f}, e[3] = {1.5f, -7.3f, 0.5f}, g[3] = {1.5f, -7.3f, -0.5f};
    CHECK(!pattern_odd(d, floor_xz));
    CHECK(pattern_odd(e, floor_xz));
    CHECK(!pattern_odd(g, floor_xz));
    // two zero axes: stripes
    const Entry stripes = entry(0, 0, 0, 0, 0, 1);
    const float s0[3] = {-3.0f, 9.0f, 0.25f}, s1[3] = {-3.0f, 9.0f, 1.25f};
    CHECK(!pattern_odd(s0, stripes) && pattern_odd(s1, stripes));
    // |f| = 2^24: every float from there on is even
    const float big[3] = {16777216.0f, 0.5f, 0.5f}, nbig[3] = {-16777216.0f, 0.5f, 0.5f}, huge[3] = {3.0e30f, 0.5f, 0.5f};
    CHECK(!pattern_odd(big, unit) && !pattern_odd(nbig, unit) && !pattern_odd(huge, unit));
    const float below[3] = {16777215.0f, 0.5f, 0.5f}; // the last odd float
    CHECK(pattern_odd(below, unit));
    // a NaN P is odd, on an axis that counts and on one that does not (NaN * 0 = NaN)
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float n0[3] = {nan, 0.5f, 0.5f}, n1[3] = {0.5f, nan, 0.5f};
    CHECK(pattern_odd(n0, unit) && pattern_odd(n1, floor_xz));
    // the origin shifts the lattice
    const Entry shifted = entry(0.37f, 0.0f, 0.41f, 0.25f, 0.0f, 0.25f);
    const float t0[3] = {0.38f, 5.0f, 0.42f}, t1[3] = {0.36f, 5.0f, 0.42f}, t2[3] = {4.38f, 5.0f, 0.42f};
    CHECK(!pattern_odd(t0, shifted) && pattern_odd(t1, shifted) && pattern_odd(t2, shifted));
}

// ---------------------------------------------------------------- 2. the table

static void test_table()
{
    static_assert(sizeof(rtx_pattern) == 36, "struct rtx_pattern is 36 bytes");
    static_assert(sizeof(Entry) == 48, "a packed entry is 3 x float4");
    static_assert(rtxpattern::kMaxPatterns == 16, "RTX_MAX_PATTERNS");
    rtx_pattern t[RTX_MAX_PATTERNS + 1];
    for (size_t i = 0; i <= RTX_MAX_PATTERNS; i++) t[i] = rtx_pattern{{1, 2, 3}, {0.5f, 0, -0.5f}, {255, 128, 0}};
    size_t bad = 99;
    CHECK(rtxpattern::table_fault(0, nullptr, &bad) == nullptr);
    CHECK(rtxpattern::table_fault(RTX_MAX_PATTERNS, t, &bad) == nullptr);
    CHECK(rtxpattern::table_fault(RTX_MAX_PATTERNS + 1, t, &bad) != nullptr && bad == RTX_MAX_PATTERNS + 1);
    CHECK(rtxpattern::table_fault(2, nullptr, &bad) != nullptr && bad == 2);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int field = 0; field < 9; field++) {
        for (const float v : {inf, -inf, nan}) {
            rtx_pattern u[3] = {t[0], t[0], t[0]};
            (field < 3 ? u[1].origin : (field < 6 ? u[1].freq : u[1].rgb))[field % 3] = v;
            CHECK(rtxpattern::table_fault(3, u, &bad) != nullptr && bad == 1);
            CHECK(rtxpattern::table_fault(1, u, &bad) == nullptr);
        }
    }
    const Entry e = rtxpattern::pack_entry(t[0]);
    CHECK(e.origin.x == 1 && e.origin.y == 2 && e.origin.z == 3 && e.freq.x == 0.5f && e.freq.y == 0 && e.freq.z == -0.5f);
    CHECK(e.od2.x == 255.0f / 255.0f && e.od2.y == 128.0f / 255.0f && e.od2.z == 0.0f);
}

// ---------------------------------------------------------------- 3. the planner

// The planner before patterns, restated: what every frame with no patterned object must still be planned as.
struct Before {
    ShadePath path = kPathDirect;
    ShadePass secondary = kPassNone, shadow_pass = kPassNone;
    ShadeFamily family = kShadeFamilies;
    bool deep = false, dark0 = false, wants_grid = false;
    uint32_t levels = 0, bytes_per_px = 0, deep_off = 0, dark0_off = 0;
};

static Before plan_before(const ShadingRequest& q)
{
    Before p;
    if (q.mode < 0 || q.mode > 3) {
        p.path = kPathDirect;
    } else if (q.n_reflective != 0 || q.reflect_check == 2) {
        p.path = kPathMirror;
    } else if (q.shadows || q.n_lights != 1 || q.lights_check || !q.light0_is_reference) {
        p.path = kPathShaded;
    }
    const bool shadows_grid = p.path != kPathDirect && q.shadow_grid && q.shadows && q.shadow_check == 0 && q.ns != 0;
    const bool mirrors_grid = p.path == kPathMirror && q.reflect_grid && q.reflect_check == 0 && q.ns != 0;
    p.wants_grid = shadows_grid || mirrors_grid;
    if (p.path == kPathDirect) return p;
    const bool mirror = p.path == kPathMirror;
    const bool grid = shadows_grid && q.grid_usable;
    const bool several = q.n_lights >= 2 || q.lights_check;
    p.deep = mirror && q.reflect_shadows && q.shadows && q.n_reflective != 0;
    const bool chain = mirror && (q.reflect_depth > 1 || q.reflect_depth_check || p.deep);
    p.secondary = chain ? kPassReflectChain : (mirror ? kPassReflectHit : kPassNone);
    if (mirrors_grid && q.grid_usable) p.secondary = kPassGridReflect;
    p.shadow_pass = grid ? kPassGridShadow : (p.deep ? kPassChainShadow : kPassNone);
    if (chain) {
        p.family = grid ? (p.deep ? kGridChainShadowShade : kGridChainShade) : (p.deep ? kLightsChainShadowShade : kLightsChainShade);
    } else if (mirror) {
        p.family = grid ? kGridReflectShade : (several ? kLightsReflectShade : kReflectShade);
    } else {
        p.family = grid ? kGridShade : (several ? kLightsShade : kShadowShade);
    }
    p.dark0 = grid;
    p.levels = chain ? q.reflect_depth + 1u : (mirror ? 2u : 1u);
    p.deep_off = 8u * p.levels;
    p.dark0_off = p.deep_off + (p.deep ? 4u : 0u);
    p.bytes_per_px = p.dark0_off + (p.dark0 ? 4u : 0u);
    return p;
}

static bool same(const ShadingPlan& p, const Before& b)
{
    return p.path == b.path && p.secondary == b.secondary && p.shadow_pass == b.shadow_pass && p.family == b.family && p.deep == b.deep && p.dark0 == b.dark0 &&
           p.levels == b.levels && p.bytes_per_px == b.bytes_per_px && p.deep_off == b.deep_off && p.dark0_off == b.dark0_off;
}

static size_t test_planner()
{
    {
        // the reference's state with one patterned object
        ShadingRequest r;
        CHECK(r.n_patterned == 0 && plan_shading(r).path == kPathDirect);
        for (r.mode = 0; r.mode <= 3; r.mode++) {
            r.n_patterned = 1;
            const ShadingPlan p = plan_shading(r);
            CHECK(p.path == kPathShaded && p.family == kShadowShade && p.bytes_per_px == 8u && p.levels == 1u);
            CHECK(p.secondary == kPassNone && p.shadow_pass == kPassNone && !p.deep && !p.dark0 && !p.chain() && !p.grid_reflect());
            CHECK(!shading_wants_grid(r));
        }
        r.mode = 4;
        CHECK(plan_shading(r).path == kPathDirect); // RGB_NORMALS and SDL do not shade
        r.mode = 5;
        CHECK(plan_shading(r).path == kPathDirect);
    }
    size_t n = 0, n_new_path = 0, n_unchanged = 0;
    ShadingRequest q;
    for (q.mode = -1; q.mode < 7; q.mode++)
    for (int shadows = 0; shadows < 2; shadows++)
    for (q.shadow_check = 0; q.shadow_check < 3; q.shadow_check++)
    for (int lights_check = 0; lights_check < 2; lights_check++)
    for (int lights = 0; lights < 3; lights++) // one reference / one other / two
    for (q.n_reflective = 0; q.n_reflective < 2; q.n_reflective++)
    for (q.reflect_check = 0; q.reflect_check < 3; q.reflect_check++)
    for (q.reflect_depth = 1; q.reflect_depth <= 4; q.reflect_depth++)
    for (int bits = 0; bits < 64; bits++) {
        q.shadows = shadows != 0;
        q.lights_check = lights_check != 0;
        q.n_lights = lights == 2 ? 2 : 1;
        q.light0_is_reference = lights == 0;
        q.reflect_depth_check = (bits & 1) != 0;
        q.reflect_shadows = (bits & 2) != 0;
        q.shadow_grid = (bits & 4) != 0;
        q.grid_usable = (bits & 8) != 0;
        q.ns = (bits & 16) ? 1u : 0u;
        q.reflect_grid = (bits & 32) != 0;
        const Before b = plan_before(q);
        n++;

        // no patterned object: the plan of before, field for field
        q.n_patterned = 0;
        CHECK(same(plan_shading(q), b));
        CHECK(shading_wants_grid(q) == b.wants_grid);

        // some: a frame that was direct in a mode that shades takes the light / shadow path's plainest form; nothing else changes
        for (const uint32_t np : {1u, 7u}) {
            q.n_patterned = np;
            const ShadingPlan p = plan_shading(q);
            if (b.path == kPathDirect && q.mode >= 0 && q.mode <= 3) {
                CHECK(p.path == kPathShaded && p.family == kShadowShade && p.bytes_per_px == 8u && p.levels == 1u);
                CHECK(p.secondary == kPassNone && p.shadow_pass == kPassNone && !p.deep && !p.dark0);
                CHECK(!shading_wants_grid(q));
                n_new_path++;
            } else {
                CHECK(same(p, b));
                CHECK(shading_wants_grid(q) == b.wants_grid);
                n_unchanged++;
            }
        }
    }
    CHECK(n == 8u * 2 * 3 * 2 * 3 * 2 * 3 * 4 * 64);
    CHECK(n_new_path > 1000 && n_unchanged > 100000);
    return n;
}

// ---------------------------------------------------------------- 4. removal

static void test_removal()
{
    std::mt19937 rng(5u);
    for (int round = 0; round < 200; round++) {
        const size_t n = 1 + rng() % 40;
        std::vector<uint8_t> kind_of(n), slots(n);
        for (size_t i = 0; i < n; i++) {
            kind_of[i] = (rng() % 3 == 0) ? 1 : 2;
            slots[i] = (uint8_t)(rng() % (RTX_MAX_PATTERNS + 1));
        }
        std::vector<uint32_t> removed;
        for (size_t i = 0; i < n; i++) {
            if (rng() % 4 == 0) removed.push_back((uint32_t)i);
        }
        const RemovalPlan plan = plan_removal(kind_of, removed);
        const std::vector<uint8_t> kept = survivors_of(slots, removed);
        CHECK(kept.size() == plan.kind_of.size() && kept.size() == n - removed.size());
        for (size_t i = 0; i < n; i++) {
            const uint32_t j = index_after_removal(removed, (uint32_t)i);
            if (j == kNoIndex) continue;
            CHECK(j < kept.size() && kept[j] == slots[i] && plan.kind_of[j] == kind_of[i]);
        }
    }
    // removing a sphere below a patterned one: the slot follows it down
    const std::vector<uint8_t> kinds = {2, 2, 2, 1}, slots = {0, 0, 2, 1};
    const std::vector<uint8_t> kept = survivors_of(slots, std::vector<uint32_t>{0});
    CHECK((kept == std::vector<uint8_t>{0, 2, 1}));
    CHECK(survivors_of(slots, std::vector<uint32_t>{}) == slots);
    CHECK(survivors_of(slots, std::vector<uint32_t>{0, 1, 2, 3}).empty());
    (void)kinds;
}

int main()
{
    const size_t tested = test_against_float64();
    test_exact_cases();
    test_table();
    const size_t requests = test_planner();
    test_removal();
    if (g_failures != 0) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("all pattern tests passed (%zu points against float64, %zu requests)\n", tested, requests);
    return 0;
}
