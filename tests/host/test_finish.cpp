// test_finish.cpp -- the surface finish of rtx_scene_set_finish on the host (csrc/rtx_finish.hpp, csrc/rtx_materials.hpp,
// csrc/rtx_plan.hpp):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tests/host/test_finish.cpp -o test_finish
//   1. power -- the very expression the shade kernels run -- against five squarings in double (pow32 of csrc/rtx_device.hpp) at
//      m = 5 bit for bit, against x at m = 0, and against float64 pow within 1 ulp at every other m, over a sweep of floats in
//      [0, 1]; ambient and add_terms against the literal expression without a finish under the default;
//   2. values_fault over the refusal list of include/rtx.h;
//   3. the book: counts, generations, the stale flag, all or nothing, -0 stored as +0, remove and clear, the three orders through
//      layout_of, stale_fault's order;
//   4. plan_shading over the cross product of the ShadingRequest fields: n_finished = 0 gives the plan of before, field for field
//      (restated below); n_finished = 1 in the reference's state is the light / shadow path with rtx_shadow_shade and no extra
//      bytes; under any request that left the direct path already, nothing of the plan changes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_finish.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_materials.hpp"
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

using namespace rtxplan;
using rtxmat::Book;

static int g_failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (g_failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            g_failures++;                                           \
        }                                                           \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

static bool same_bytes(const rtx_finish& a, const rtx_finish& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---------------------------------------------------------------- 1. the rule

static float pow32(float x) // csrc/rtx_device.hpp
{
    double d = (double)x;
    d = d * d;
    d = d * d;
    d = d * d;
    d = d * d;
    d = d * d;
    return (float)d;
}

static size_t test_power()
{
    std::vector<float> xs = {0.0f, 1.0f, 0.5f, 0.99999994f, 1e-30f, 1.17549435e-38f, 1e-45f, 0.70710678f, 0.9f, 0.999f};
    std::mt19937 rng(34u);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    for (int i = 0; i < 200000; i++) xs.push_back(u01(rng));
    for (int i = 0; i < 100000; i++) xs.push_back(1.0f - u01(rng) * 0.01f); // (where the high powers are not 0)
    size_t tested = 0;
    for (const float x : xs) {
        CHECK(bits(rtxfinish::power(x, 5)) == bits(pow32(x)));
        CHECK(bits(rtxfinish::power(x, 0)) == bits(x));
        for (uint32_t m = 1; m <= rtxfinish::kMaxShininessLog2; m++) {
            const float got = rtxfinish::power(x, m);
            const float want = (float)std::pow((double)x, (double)(1u << m));
            // within 1 ulp of the correctly rounded power (m squarings in double err by far less before the one rounding)
            CHECK(got == want || got == std::nextafterf(want, 2.0f) || got == std::nextafterf(want, -1.0f));
            CHECK(got >= 0.0f && got <= 1.0f);
            tested++;
        }
        CHECK(bits(rtxfinish::power(x, 9)) == bits(rtxfinish::power(x, 8))); // (never more than 8 squarings, whatever is stored)
    }
    // the default finish is the expression without a finish, operation for operation
    const rtx_finish d = rtxfinish::default_finish();
    CHECK(d.ambient == 0.2f && d.diffuse == 1.0f && d.specular == 1.0f && d.shininess_log2 == 5u && sizeof(rtx_finish) == 16);
    for (int i = 0; i < 100000; i++) {
        const float od = u01(rng), diffuse = u01(rng) * 3.0f, specular = u01(rng) * 3.0f, res = u01(rng);
        CHECK(bits(rtxfinish::ambient(d.ambient, od)) == bits(0.2f * od));
        CHECK(bits(rtxfinish::add_terms(res, diffuse, d.diffuse, od, specular, d.specular)) == bits((res + diffuse * od) + specular * 1.0f));
    }
    // where the weights enter: (diffuse * kd) * od, not diffuse * (kd * od)
    CHECK(rtxfinish::add_terms(0.25f, 3.0f, 0.5f, 2.0f, 7.0f, 3.0f) == (0.25f + (3.0f * 0.5f) * 2.0f) + 7.0f * 3.0f);
    return tested;
}

// ---------------------------------------------------------------- 2. the values a call accepts

static void test_values()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const rtx_finish good = {0.3f, 0.7f, 1.7f, 3u};
    size_t bad = 99;
    CHECK(rtxfinish::values_fault(0, nullptr, &bad) == nullptr && bad == 0);
    CHECK(rtxfinish::values_fault(2, nullptr, &bad) != nullptr && bad == 2);
    const rtx_finish edges[4] = {{0.0f, 0.0f, 0.0f, 0u}, {16.0f, 16.0f, 16.0f, 8u}, {-0.0f, -0.0f, -0.0f, 5u}, good};
    CHECK(rtxfinish::values_fault(4, edges, &bad) == nullptr && bad == 4);
    for (int field = 0; field < 3; field++) {
        for (const float v : {nan, inf, -inf, -1.0f, -1e-30f, 16.000002f, 1e30f}) {
            rtx_finish f[3] = {good, good, good};
            (field == 0 ? f[1].ambient : (field == 1 ? f[1].diffuse : f[1].specular)) = v;
            CHECK(rtxfinish::values_fault(3, f, &bad) != nullptr && bad == 1);
            CHECK(rtxfinish::values_fault(1, f, &bad) == nullptr && bad == 1);
        }
    }
    for (const uint32_t m : {9u, 32u, 0xffffffffu}) {
        rtx_finish f[2] = {good, good};
        f[0].shininess_log2 = m;
        CHECK(rtxfinish::values_fault(2, f, &bad) != nullptr && bad == 0);
    }
    const rtx_finish z = rtxfinish::stored(edges[2]);
    CHECK(bits(z.ambient) == 0u && bits(z.diffuse) == 0u && bits(z.specular) == 0u && z.shininess_log2 == 5u);
    CHECK(same_bytes(rtxfinish::stored(good), good));
    CHECK(rtxfinish::is_default(rtxfinish::default_finish()) && !rtxfinish::is_default(good));
}

// ---------------------------------------------------------------- 3. the book

static void test_book()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const rtx_finish def = rtxfinish::default_finish(), a = {0.2f, 1.0f, 0.0f, 5u}, b = {0.1f, 0.8f, 1.7f, 7u}, c = {0.8f, 0.3f, 1.0f, 0u};
    Book book;
    CHECK(book.n_finished() == 0 && book.generations().finish == 0);
    for (int i = 0; i < 5; i++) book.append();
    for (size_t i = 0; i < 5; i++) CHECK(same_bytes(book[i].finish, def)); // every new object: the default
    CHECK(book.n_finished() == 0 && book.generations().finish == 0);       // (appending moves no generation)
    book.uploaded();
    CHECK(!book.stale());

    // a good call: stored, counted, the generation moves, the copies are stale
    const rtx_finish two[2] = {a, b};
    size_t bad = 99;
    CHECK(book.set_finish(1, 2, two, &bad) == nullptr && bad == 2);
    CHECK(same_bytes(book[1].finish, a) && same_bytes(book[2].finish, b) && same_bytes(book[0].finish, def) && same_bytes(book[3].finish, def));
    CHECK(book.n_finished() == 2 && book.generations().finish == 1 && book.stale());
    CHECK(book.generations().reflectivity == 0 && book.generations().pattern == 0 && book.generations().refraction == 0);
    CHECK(book.n_reflective() == 0 && book.n_patterned() == 0 && book.n_refractive() == 0);
    book.uploaded();

    // n = 0: a good call that changes nothing (also at the end of the range, also with NULL)
    CHECK(book.set_finish(5, 0, nullptr) == nullptr && book.set_finish(0, 0, two) == nullptr);
    CHECK(book.generations().finish == 1 && !book.stale());

    // all or nothing: every refusal leaves values, count, generation and flag alone, and names the first offender
    const rtx_finish with_nan[3] = {c, {nan, 1.0f, 1.0f, 5u}, c}, with_m[2] = {c, {0.2f, 1.0f, 1.0f, 9u}}, above[1] = {{0.2f, 16.5f, 1.0f, 5u}};
    const rtx_finish negative[2] = {{0.2f, 1.0f, -0.5f, 5u}, c}, five[6] = {c, c, c, c, c, c};
    CHECK(book.set_finish(0, 3, with_nan, &bad) != nullptr && bad == 1);
    CHECK(book.set_finish(3, 2, with_m, &bad) != nullptr && bad == 1);
    CHECK(book.set_finish(4, 1, above, &bad) != nullptr && bad == 0);
    CHECK(book.set_finish(0, 2, negative, &bad) != nullptr && bad == 0);
    CHECK(book.set_finish(0, 6, five, &bad) != nullptr && bad == 6);  // a range past the count
    CHECK(book.set_finish(6, 0, five, &bad) != nullptr);
    CHECK(book.set_finish(4, 2, five, &bad) != nullptr);
    CHECK(book.set_finish(0, (size_t)-1, five, &bad) != nullptr);      // (no overflow in first + n)
    CHECK(book.set_finish(0, 2, nullptr, &bad) != nullptr && bad == 2); // finishes == NULL with n > 0
    CHECK(same_bytes(book[0].finish, def) && same_bytes(book[1].finish, a) && same_bytes(book[2].finish, b) && same_bytes(book[3].finish, def) &&
          same_bytes(book[4].finish, def));
    CHECK(book.n_finished() == 2 && book.generations().finish == 1 && !book.stale());

    // -0 is stored as +0; the default set again counts as no finish
    const rtx_finish minus[1] = {{-0.0f, -0.0f, -0.0f, 5u}};
    CHECK(book.set_finish(4, 1, minus) == nullptr);
    CHECK(bits(book[4].finish.ambient) == 0u && bits(book[4].finish.diffuse) == 0u && bits(book[4].finish.specular) == 0u);
    CHECK(book.n_finished() == 3 && book.generations().finish == 2);
    const rtx_finish back[2] = {def, def};
    CHECK(book.set_finish(1, 1, back) == nullptr && book.n_finished() == 2 && book.generations().finish == 3);
    CHECK(book.set_finish(0, 2, back) == nullptr && book.n_finished() == 2); // (default over default: still counted right)

    // the three orders: spheres by index, by sorted position, planes by index (objects 0, 2, 3 spheres, 1 and 4 planes)
    {
        const std::vector<uint8_t> kind_of = {2, 1, 2, 2, 1};
        const std::vector<uint32_t> local_of = {0, 0, 1, 2, 1}, sorted_idx = {2, 0, 1};
        const auto l = rtxmat::layout_of(book.column(&rtxmat::Surface::finish), kind_of, local_of, 3, 2, sorted_idx);
        CHECK(l.sph.size() == 3 && l.sph_sorted.size() == 3 && l.pl.size() == 2);
        CHECK(same_bytes(l.sph[0], def) && same_bytes(l.sph[1], b) && same_bytes(l.sph[2], def));
        CHECK(same_bytes(l.sph_sorted[0], def) && same_bytes(l.sph_sorted[1], def) && same_bytes(l.sph_sorted[2], b));
        CHECK(same_bytes(l.pl[0], def) && same_bytes(l.pl[1], rtxfinish::stored(minus[0])));
        CHECK(&l.spheres(true) == &l.sph_sorted && &l.spheres(false) == &l.sph);
        const auto none = rtxmat::layout_of(std::vector<rtx_finish>(), std::vector<uint8_t>(), std::vector<uint32_t>(), 0, 0, std::vector<uint32_t>());
        CHECK(none.sph.size() == 1 && none.sph_sorted.size() == 1 && none.pl.size() == 1); // (never fewer than one entry each)
    }

    // removal: the survivors keep theirs under the renumbering, every count afresh, every generation moves
    const rtxmat::Generations before = book.generations();
    book.uploaded();
    book.remove(std::vector<uint32_t>{0, 3});
    CHECK(book.size() == 3 && same_bytes(book[0].finish, def) && same_bytes(book[1].finish, b) && same_bytes(book[2].finish, rtxfinish::stored(minus[0])));
    CHECK(book.n_finished() == 2 && book.stale() && book.generations().finish == before.finish + 1 && book.generations().reflectivity == before.reflectivity + 1);
    book.remove(std::vector<uint32_t>{1});
    CHECK(book.n_finished() == 1);
    book.append();
    CHECK(same_bytes(book[2].finish, def) && book.n_finished() == 1);
    book.clear();
    CHECK(book.size() == 0 && book.n_finished() == 0);
    book.append();
    CHECK(same_bytes(book[0].finish, def));

    // stale_fault: the finish generation is asked last
    rtxmat::Generations then, now;
    CHECK(rtxmat::stale_fault(then, now) == nullptr);
    now.finish = 1;
    const char* f = rtxmat::stale_fault(then, now);
    CHECK(f != nullptr && std::strstr(f, "finishes") != nullptr && std::strstr(f, "re-capture") != nullptr);
    now.refraction = 1;
    CHECK(std::strstr(rtxmat::stale_fault(then, now), "refraction") != nullptr);
}

// ---------------------------------------------------------------- 4. the planner

// The planner before finishes, restated: what every frame with no finished object must still be planned as.
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
    } else if (q.shadows || q.n_lights != 1 || q.lights_check || !q.light0_is_reference || q.n_patterned != 0) {
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
        // the reference's state with one finished object
        ShadingRequest r;
        CHECK(r.n_finished == 0 && plan_shading(r).path == kPathDirect);
        for (r.mode = 0; r.mode <= 3; r.mode++) {
            r.n_finished = 1;
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
    for (q.n_patterned = 0; q.n_patterned < 2; q.n_patterned++)
    for (int bits_ = 0; bits_ < 64; bits_++) {
        q.shadows = shadows != 0;
        q.lights_check = lights_check != 0;
        q.n_lights = lights == 2 ? 2 : 1;
        q.light0_is_reference = lights == 0;
        q.reflect_depth_check = (bits_ & 1) != 0;
        q.reflect_shadows = (bits_ & 2) != 0;
        q.shadow_grid = (bits_ & 4) != 0;
        q.grid_usable = (bits_ & 8) != 0;
        q.ns = (bits_ & 16) ? 1u : 0u;
        q.reflect_grid = (bits_ & 32) != 0;
        const Before b = plan_before(q);
        n++;

        // no finished object: the plan of before, field for field
        q.n_finished = 0;
        CHECK(same(plan_shading(q), b));
        CHECK(shading_wants_grid(q) == b.wants_grid);

        // some: a frame that was direct in a mode that shades takes the light / shadow path's plainest form; nothing else changes
        for (const uint32_t nf : {1u, 7u}) {
            q.n_finished = nf;
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
        q.n_finished = 0;
    }
    CHECK(n == 8u * 2 * 3 * 2 * 3 * 2 * 3 * 4 * 2 * 64);
    CHECK(n_new_path > 1000 && n_unchanged > 100000);
    return n;
}

int main()
{
    const size_t powers = test_power();
    test_values();
    test_book();
    const size_t requests = test_planner();
    if (g_failures != 0) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("all finish tests passed (%zu powers against float64, %zu requests)\n", powers, requests);
    return 0;
}
