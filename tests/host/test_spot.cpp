// Host test of the cones of rtx_scene_set_spots: csrc/rtx_lights.hpp (what a call accepts, all or nothing, and the packing) and
// csrc/rtx_spot.hpp (the rule: edge, smooth, weight, outside -- the very expressions the kernels run), built with -ffp-contract=off
// under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_host_spot.py.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <limits>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_lights.hpp"

static int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);    \
            failures++;                                              \
        }                                                            \
    } while (0)

static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kInf = std::numeric_limits<float>::infinity();

static rtx_spot spot(float x, float y, float z, float co, float ci) { return rtx_spot{{x, y, z}, co, ci}; }

static rtx_spot good_no(int i) { return spot(1.0f + (float)i, -3.0f, 0.5f * (float)i, 0.5f + 0.01f * (float)i, 0.75f + 0.01f * (float)i); }

static rtxspot::Block sentinel()
{
    rtxspot::Block b;
    memset(&b, 0x5a, sizeof b);
    return b;
}

// one refused call: the fault, the offending index, and nothing stored
static long refused = 0;
static void expect_refused(size_t n_lights, size_t n, const rtx_spot* spots, size_t want_bad)
{
    size_t bad = 12345;
    CHECK(rtxlights::spots_fault(n_lights, n, spots, &bad) != nullptr);
    CHECK(bad == want_bad);
    CHECK(rtxlights::spots_fault(n_lights, n, spots) != nullptr); // (without the index)
    rtxspot::Block b = sentinel();
    const rtxspot::Block before = b;
    CHECK(!rtxlights::pack_spots(n_lights, n, spots, &b));
    CHECK(memcmp(&b, &before, sizeof b) == 0);
    refused++;
}

static float bits_next(float v, int steps) // `steps` floats above (below, if negative) a positive v
{
    uint32_t u;
    memcpy(&u, &v, 4);
    u = (uint32_t)((int32_t)u + steps);
    memcpy(&v, &u, 4);
    return v;
}

int main()
{
    static_assert(sizeof(rtx_spot) == 20, "rtx_spot is 20 bytes");
    static_assert(sizeof(rtxspot::Packed) == 24 && sizeof(rtxspot::Block) == 24 * RTX_MAX_LIGHTS, "the stored cones");

    // ---- what a call accepts
    rtx_spot set[RTX_MAX_LIGHTS];
    for (int i = 0; i < RTX_MAX_LIGHTS; i++) set[i] = good_no(i);
    for (size_t n = 1; n <= RTX_MAX_LIGHTS; n++) {
        size_t bad = 99;
        CHECK(rtxlights::spots_fault(n, n, set, &bad) == nullptr && bad == n);
        CHECK(rtxlights::spots_fault(n, 0, nullptr, &bad) == nullptr && bad == 0); // n = 0: spots may be NULL
        CHECK(rtxlights::spots_fault(n, 0, set) == nullptr);
        // any other n; NULL with n > 0
        for (size_t m = 1; m <= RTX_MAX_LIGHTS + 1; m++) {
            if (m != n) expect_refused(n, m, set, m);
        }
        expect_refused(n, n, nullptr, n);
        // every way one cone can be bad, at every position: the first offender is named, nothing is stored
        for (size_t at = 0; at < n; at++) {
            for (int k = 0; k < 3; k++) {
                for (float v : {kNaN, kInf, -kInf}) {
                    rtx_spot list[RTX_MAX_LIGHTS];
                    memcpy(list, set, sizeof list);
                    list[at].dir[k] = v;
                    expect_refused(n, n, list, at);
                }
            }
            const rtx_spot bads[] = {
                spot(0x1p-21f, 0.0f, 0.0f, 0.5f, 0.75f),              // squared length 2^-42
                spot(0.0f, 0x1p-20f * 0.99f, 0.0f, 0.5f, 0.75f),      // just below 2^-40
                spot(0x1p20f, 1.0f, 0.0f, 0.5f, 0.75f),               // just above 2^40
                spot(3.0e38f, 3.0e38f, 3.0e38f, 0.5f, 0.75f),         // finite in double, far outside
                spot(1.0e-30f, 0.0f, 0.0f, 0.5f, 0.75f),
                spot(1.0f, 2.0f, 3.0f, kNaN, 0.75f),  spot(1.0f, 2.0f, 3.0f, 0.5f, kNaN), spot(1.0f, 2.0f, 3.0f, -kInf, 0.75f),
                spot(1.0f, 2.0f, 3.0f, 0.5f, kInf),
                spot(1.0f, 2.0f, 3.0f, bits_next(1.0f, 1) * -1.0f, 0.75f), // cos_outer just below -1
                spot(1.0f, 2.0f, 3.0f, 0.5f, bits_next(1.0f, 1)),          // cos_inner just above 1
                spot(1.0f, 2.0f, 3.0f, 0.5f, 0.5f),                        // no band
                spot(1.0f, 2.0f, 3.0f, 0.75f, 0.5f),                       // inner outside outer
                spot(1.0f, 2.0f, 3.0f, 0.5f, bits_next(0.5f + 0x1p-10f, -1)), // a band one float below 2^-10
            };
            for (const rtx_spot& b : bads) {
                rtx_spot list[RTX_MAX_LIGHTS];
                memcpy(list, set, sizeof list);
                list[at] = b;
                expect_refused(n, n, list, at);
                if (at + 1 < n) { // two offenders: the first is named
                    list[at + 1] = bads[0];
                    expect_refused(n, n, list, at);
                }
            }
        }
    }
    // the ends of the ranges are accepted: squared lengths 2^-40 and 2^40, cosines -1 and 1, a band of exactly 2^-10
    {
        const rtx_spot ends[] = {spot(0x1p-20f, 0.0f, 0.0f, -1.0f, 1.0f), spot(0.0f, 0.0f, -0x1p20f, -1.0f, 1.0f), spot(1.0f, 0.0f, 0.0f, 0.5f, 0.5f + 0x1p-10f),
                                 spot(-0.0f, 0.0f, 5.0f, 1.0f - 0x1p-10f, 1.0f)};
        for (const rtx_spot& e : ends) CHECK(rtxlights::spot_fault(e) == nullptr);
        CHECK(rtxlights::pack_spot(ends[2]).inv == 1024.0f && rtxlights::pack_spot(ends[0]).inv == 0.5f);
    }
    // a point light: (0,0,0) with either sign of zero; its cosines are not looked at, and it is stored as zeros
    {
        const rtx_spot points[] = {spot(0.0f, 0.0f, 0.0f, kNaN, kInf), spot(-0.0f, 0.0f, -0.0f, 7.0f, -7.0f), spot(0.0f, -0.0f, 0.0f, 0.9f, 0.1f)};
        for (const rtx_spot& p : points) {
            CHECK(rtxlights::spot_fault(p) == nullptr && rtxlights::spot_is_point(p));
            const rtxspot::Packed k = rtxlights::pack_spot(p);
            const rtxspot::Packed zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            CHECK(memcmp(&k, &zero, sizeof k) == 0 && !rtxspot::has_cone(k));
            const rtx_spot back = rtxlights::stored_spot(k);
            const rtx_spot five_zeros = spot(0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
            CHECK(memcmp(&back, &five_zeros, sizeof back) == 0);
            // w is exactly 1 towards anything
            for (float x : {0.0f, 1.0f, -1.0f, kNaN, 0.3f}) CHECK(rtxspot::weight(k, x, 0.5f, -x) == 1.0f && !rtxspot::outside(k, x, 0.5f, -x));
        }
        // a mixed set: light 1 a point light; n = 0 clears every cone
        rtx_spot mixed[3] = {good_no(0), points[0], good_no(2)};
        rtxspot::Block b = sentinel();
        CHECK(rtxlights::pack_spots(3, 3, mixed, &b) && rtxlights::spot_count(b) == 2 && rtxspot::has_cone(b.spot[0]) && !rtxspot::has_cone(b.spot[1]));
        for (int i = 3; i < RTX_MAX_LIGHTS; i++) CHECK(!rtxspot::has_cone(b.spot[i]) && b.spot[i].ax == 0.0f);
        CHECK(rtxlights::pack_spots(3, 0, nullptr, &b) && rtxlights::spot_count(b) == 0);
        CHECK(!rtxlights::pack_spots(3, 3, mixed, nullptr));
    }

    // ---- the stored axis and inv against long double
    {
        const rtx_spot dirs[] = {spot(0.0f, -38.0f, -18.0f, 0.97029573f, 0.99026805f), spot(24.0f, -30.0f, 3.0f, 0.93969262f, 0.97814763f),
                                 spot(1.0e-5f, 3.0e-5f, -2.0e-5f, -1.0f, 1.0f),       spot(7.0e5f, -1.0f, 3.0e5f, 0.1f, 0.3f),
                                 spot(1.0f, 1.0f, 1.0f, -0.25f, 0.6f),                spot(0.0f, 0.0f, -5.0f, 0.0f, 0x1p-10f)};
        for (const rtx_spot& s : dirs) {
            CHECK(rtxlights::spot_fault(s) == nullptr);
            const rtxspot::Packed k = rtxlights::pack_spot(s);
            const long double x = s.dir[0], y = s.dir[1], z = s.dir[2], len = sqrtl(x * x + y * y + z * z);
            const long double want[3] = {x / len, y / len, z / len};
            const float got[3] = {k.ax, k.ay, k.az};
            for (int q = 0; q < 3; q++) {
                // within one rounding to float of the long double quotient (the double steps add far less than half an ulp)
                const float lo = nextafterf((float)want[q], -kInf), hi = nextafterf((float)want[q], kInf);
                CHECK(got[q] >= lo && got[q] <= hi);
                CHECK(fabsl((long double)got[q] - want[q]) <= 0x1p-24L * (fabsl(want[q]) > 0x1p-100L ? fabsl(want[q]) * 1.0001L : 0x1p-126L));
            }
            CHECK(fabs((double)k.ax * k.ax + (double)k.ay * k.ay + (double)k.az * k.az - 1.0) < 1e-6);
            const float band = s.cos_inner - s.cos_outer;
            CHECK(k.inv == 1.0f / band && k.cos_outer == s.cos_outer && k.cos_inner == s.cos_inner);
            CHECK(fabsl((long double)k.inv - 1.0L / (long double)band) <= 0x1p-24L / (long double)band);
            CHECK(k.inv >= 0.5f && k.inv <= 1024.0f && rtxspot::has_cone(k));
            const rtx_spot back = rtxlights::stored_spot(k);
            CHECK(back.dir[0] == k.ax && back.dir[1] == k.ay && back.dir[2] == k.az && back.cos_outer == s.cos_outer && back.cos_inner == s.cos_inner);
        }
    }

    // ---- the rule: the axis is (0, 0, -1), so a direction ld = (sqrt(1 - c^2), 0, c) towards the light has m = -c and the rule's c = c
    {
        // The first three are the cones of the GPU tests (14 / 8, 20 / 12 and 16 / 15 degrees): there the sweep asks for w never to
        // fall.  s is monotone in c for any cone, exactly: every operation that forms it is one rounding of a monotone function.  w is
        // not, in fp32: (s * s) rises and (3 - 2 s) falls with s, and near s = 1, where the exact 3 s^2 - 2 s^3 is flat, the product's
        // rounding decides (of the 2^30 floats s in [0, 1], 269843 have a w one ulp below their predecessor's).  What holds for any
        // cone: each of the three operations is off by at most 2^-24 of its result, so a computed w is within E = 3.0001 * 2^-24 of
        // the exact one (w <= 1), and over a rising s it falls by at most 2 E.  The wide and the narrowest bands are held to that.
        const struct {
            float co, ci;
            bool strict;
        } bands[] = {{0.97029573f, 0.99026805f, true}, {0.93969262f, 0.97814763f, true}, {0.96126169f, 0.96592583f, true}, {-1.0f, 1.0f, false},
                     {0.5f, 0.5f + 0x1p-10f, false},   {-0.3f, 0.2f, false},             {1.0f - 0x1p-10f, 1.0f, false}};
        const float two_E = 2.0f * 3.0001f * 0x1p-24f;
        for (const auto& b : bands) {
            const rtxspot::Packed k = rtxlights::pack_spot(spot(0.0f, 0.0f, -2.0f, b.co, b.ci));
            CHECK(k.ax == 0.0f && k.ay == 0.0f && k.az == -1.0f);
            const auto w_at = [&](float c) { return rtxspot::weight(k, 0.0f, 0.0f, c); };
            const auto out_at = [&](float c) { return rtxspot::outside(k, 0.0f, 0.0f, c); };
            // 0 at and beyond cos_outer, and the pre-test says so; 1 at and within cos_inner
            for (int step = 0; step <= 4; step++) {
                const float c = step == 0 ? b.co : nextafterf(b.co - (float)(step - 1) * 0.01f, -kInf);
                CHECK(w_at(c) == 0.0f && out_at(c));
                const float d = step == 0 ? b.ci : nextafterf(b.ci + (float)(step - 1) * 0.01f, kInf);
                CHECK(w_at(d) == 1.0f && !out_at(d));
            }
            CHECK(w_at(-1.5f) == 0.0f && w_at(1.5f) == 1.0f);
            // strictly inside the band: strictly between, and never called outside
            const float mid = b.co + (b.ci - b.co) * 0.5f;
            CHECK(w_at(mid) > 0.0f && w_at(mid) < 1.0f && !out_at(mid));
            // the pre-test is the rule's own s: outside exactly where edge is not above 0
            // monotone over a sweep of 2^16 values of c from below the outer cosine to above the inner one
            const float lo = b.co - 0.05f, span = (b.ci - b.co) + 0.1f;
            float prev = -1.0f, prev_s = -1.0f;
            long inside = 0;
            for (int i = 0; i < (1 << 16); i++) {
                const float c = lo + span * ((float)i / 65535.0f);
                const float s = rtxspot::edge(k, 0.0f, 0.0f, c), w = w_at(c);
                CHECK(s >= prev_s && w >= 0.0f && w <= 1.0f && s >= 0.0f && s <= 1.0f);
                CHECK(b.strict ? w >= prev : w >= prev - two_E);
                CHECK(out_at(c) == !(s > 0.0f) && w == rtxspot::smooth(s));
                if (w > 0.0f && w < 1.0f) inside++;
                prev = w;
                prev_s = s;
            }
            // (the band's share of the sweep's 2^16 values lies strictly inside it)
            CHECK(prev == 1.0f && (double)inside >= 0.9 * 65535.0 * (double)(b.ci - b.co) / (double)span);
        }
    }
    // a NaN x gives 0 (s = 0, w = 0, and the light counts as outside); an infinite one clamps
    {
        const rtxspot::Packed k = rtxlights::pack_spot(spot(0.0f, 0.0f, -1.0f, 0.5f, 0.75f));
        CHECK(rtxspot::edge(k, kNaN, 0.0f, 0.9f) == 0.0f && rtxspot::weight(k, 0.0f, kNaN, 0.9f) == 0.0f && rtxspot::outside(k, 0.0f, 0.0f, kNaN));
        CHECK(rtxspot::weight(k, 0.0f, 0.0f, kInf) == 1.0f && rtxspot::weight(k, 0.0f, 0.0f, -kInf) == 0.0f);
        rtxspot::Packed odd = k;
        odd.inv = kNaN; // (never stored: the rule itself is asked)
        CHECK(rtxspot::edge(odd, 0.0f, 0.0f, 0.9f) == 0.0f && rtxspot::smooth(0.0f) == 0.0f && rtxspot::smooth(1.0f) == 1.0f);
    }
    // the operations are the rule's, in its order: m = (ax ldx + ay ldy) + az ldz; x = (-m - cos_outer) inv; w = (s s)(3 - 2 s)
    {
        const rtxspot::Packed k = rtxlights::pack_spot(spot(24.0f, -30.0f, 3.0f, 0.93969262f, 0.97814763f));
        const float ld[3] = {-0.8039f, 0.5908f, -0.0753f}; // (about 15 degrees off the axis: inside the band)
        const float m = (k.ax * ld[0] + k.ay * ld[1]) + k.az * ld[2];
        const float x = (-m - k.cos_outer) * k.inv;
        CHECK(x > 0.0f && x < 1.0f);
        CHECK(rtxspot::edge(k, ld[0], ld[1], ld[2]) == x && rtxspot::weight(k, ld[0], ld[1], ld[2]) == (x * x) * (3.0f - 2.0f * x));
    }

    if (failures == 0) printf("all spot tests passed (%ld refused calls)\n", refused);
    return failures == 0 ? 0 : 1;
}
