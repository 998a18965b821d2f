// Host proof of csrc/rtx_far.hpp -- the far distance folded into a table plane's direction test:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/test_far_threshold.cpp -o t && ./t
// (tests/test_host_far_threshold.py builds and runs it).  No HIP, no GPU.  Host num / dn is IEEE round-to-nearest: it is what
// div_cr returns on the device, and it is the truth here.
//
// For every (num, far) of a grid and every dn of a window of +-4096 floats around the pair's cut, and at the extremes of dn:
//   * where the parent's test (dn > 0 || |dn| < FLT_EPSILON) leaves the plane, the new one (dn > cut) leaves it too;
//   * where only the new one leaves it, num / dn > far: the pixel is a miss with or without the plane;
//   * where the rule keeps the parent's cut, the two tests agree on every dn.
// The grid: every exponent of both values (subnormals included) with significands drawn from the binade's edges and middle,
// num < 0 < far; every pair of a smaller set of exponents with all 25 significand pairs and all four sign pairs; and the
// special values (zeros, infinities, NaN, FLT_MAX, the no-hit distance and its neighbours).
#include "../../raytracing-in-windows-console_amd/csrc/rtx_far.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace rtx;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            g_failed++;                                                          \
        }                                                                        \
    } while (0)

static uint32_t bits_of(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float float_of(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// Plane.cu:41-44 as the trace kernels write it
static bool parent_exit(float dn) { return dn > 0.0f || std::fabs(dn - 0.0f) < 1.1920928955078125e-7f; }

struct Tally {
    unsigned long long pairs = 0, pairs_with_cut = 0, lanes = 0, dropped = 0, bad = 0;
    unsigned long long cut_pairs_without_drop = 0;
};

// one dn of one pair; returns whether the new test dropped a lane the parent keeps
static bool check_dn(float num, float far, float cut, float dn, Tally& t)
{
    t.lanes++;
    const bool was = parent_exit(dn), now = dn > cut;
    bool ok = true;
    if (was && !now) ok = false;
    if (cut == kDirCut && was != now) ok = false; // the one-compare form of the parent's two conditions
    bool dropped = false;
    if (now && !was) {
        dropped = true;
        volatile float vn = num, vd = dn;
        volatile float t1 = vn / vd;
        if (!(t1 > far)) ok = false;
    }
    if (!ok) {
        if (t.bad++ < 8) {
            std::printf("FAIL num 0x%08x far 0x%08x cut 0x%08x dn 0x%08x: parent %d new %d t1 %a far %a\n", bits_of(num), bits_of(far), bits_of(cut), bits_of(dn),
                        (int)was, (int)now, (double)(num / dn), (double)far);
        }
    }
    return dropped;
}

static const uint32_t kExtremes[] = {
    0x00000000u, 0x80000000u,                                     // +-0
    0x34000000u, 0x33ffffffu, 0x34000001u,                        // +FLT_EPSILON and its neighbours
    0xb4000000u, 0xb3ffffffu, 0xb4000001u,                        // -FLT_EPSILON and its neighbours
    0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,           // smallest subnormals, +-FLT_MIN
    0x3f800000u, 0xbf800000u,                                     // +-1
    0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u,           // +-FLT_MAX, +-inf
    0x7fc00000u, 0xffc00000u, 0x7f800001u,                        // NaNs
};

static void check_pair(float num, float far, Tally& t)
{
    const float cut = far_dir_cut(num, far);
    t.pairs++;
    CHECK(cut == cut && cut <= kDirCut); // never NaN, never above the parent's
    const bool has_cut = cut < kDirCut;
    t.pairs_with_cut += has_cut;
    if (has_cut) {
        // only where the header says so
        if (!(num < 0.0f && far >= FLT_MIN && far < kFarNoHit)) {
            if (t.bad++ < 8) std::printf("FAIL a cut for num %a far %a\n", (double)num, (double)far);
        }
    }
    unsigned long long dropped = 0;
    const uint32_t c = bits_of(cut); // negative and finite or -inf: 0xb4000000 .. 0xff800000
    for (int32_t i = -4096; i <= 4096; i++) {
        dropped += check_dn(num, far, cut, float_of(c + (uint32_t)i), t);
    }
    for (uint32_t e : kExtremes) {
        dropped += check_dn(num, far, cut, float_of(e), t);
    }
    t.dropped += dropped;
    // a finite cut below the parent's has droppable lanes right above it (towards zero): the window must have met them
    if (has_cut && dropped == 0) t.cut_pairs_without_drop++;
}

static const uint32_t kSig[5] = {0x000000u, 0x000001u, 0x400000u, 0x7ffffeu, 0x7fffffu};

static float make(uint32_t sign, uint32_t exp, uint32_t sig)
{
    if (exp == 0u && sig == 0u) sig = 0x000002u; // (zeros are among the specials; keep this one a subnormal)
    return float_of((sign << 31) | (exp << 23) | sig);
}

int main()
{
    Tally t;

    // ---- every exponent of both, num < 0 < far, the significand pair walking through all 25 combinations
    for (uint32_t en = 0; en <= 254u; en++) {
        for (uint32_t ef = 0; ef <= 254u; ef++) {
            const uint32_t pick = (en * 7u + ef * 3u) % 25u;
            check_pair(make(1u, en, kSig[pick / 5u]), make(0u, ef, kSig[pick % 5u]), t);
        }
    }
    const unsigned long long cuts_in_sweep = t.pairs_with_cut;

    // ---- a smaller set of exponents: all significand pairs, all sign pairs.  0: subnormal; 1: FLT_MIN's binade; 103/104: the
    // quotient against far ~ 1 crosses FLT_EPSILON; 127: 1.0; 134: 250 (the bench's far); 153: kNoHit's binade; 254: FLT_MAX's
    static const uint32_t kExp[] = {0u, 1u, 2u, 24u, 64u, 103u, 104u, 126u, 127u, 128u, 134u, 152u, 153u, 154u, 200u, 253u, 254u};
    for (uint32_t en : kExp) {
        for (uint32_t ef : kExp) {
            for (uint32_t s = 0; s < 4u; s++) {
                for (uint32_t k = 0; k < 25u; k++) {
                    check_pair(make(s & 1u, en, kSig[k / 5u]), make(s >> 1, ef, kSig[k % 5u]), t);
                }
            }
        }
    }

    // ---- special values of either, against each other and against ordinary values
    const float inf = INFINITY, nan = NAN;
    const float special[] = {0.0f, -0.0f, inf, -inf, nan, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, float_of(1u), float_of(0x80000001u), float_of(0x007fffffu),
                             kFarNoHit, std::nextafter(kFarNoHit, 0.0f), std::nextafter(kFarNoHit, inf), -30.0f, 250.0f, -7500.0f, 120.0f, 1.0f, -1.0f,
                             -3e19f, 3e19f, -3e-17f, 2.5e-16f, 2.5e20f};
    for (float a : special) {
        for (float b : special) {
            check_pair(a, b, t);
        }
    }
    // quotients right at the overflow threshold and at FLT_EPSILON
    check_pair(-FLT_MAX, 1.0f, t);
    check_pair(-FLT_MAX, std::nextafter(1.0f, 0.0f), t);
    check_pair(-0x1.0p127f, 0.5f, t);
    check_pair(-0x1.000002p127f, 0x1.000002p-1f, t);
    check_pair(-FLT_EPSILON, 1.0f, t);
    check_pair(-std::nextafter(FLT_EPSILON, 1.0f), 1.0f, t);
    check_pair(-0x1.000008p-23f, 1.0f, t);

    // ---- what the rule must leave alone, stated directly
    CHECK(far_dir_cut(-30.0f, inf) == kDirCut && far_dir_cut(-30.0f, 0.0f) == kDirCut && far_dir_cut(-30.0f, -250.0f) == kDirCut);
    CHECK(far_dir_cut(-30.0f, nan) == kDirCut && far_dir_cut(-30.0f, FLT_MAX) == kDirCut && far_dir_cut(-30.0f, float_of(0x007fffffu)) == kDirCut);
    CHECK(far_dir_cut(-30.0f, kFarNoHit) == kDirCut && far_dir_cut(-3e38f, std::nextafter(kFarNoHit, 0.0f)) < kDirCut);
    CHECK(far_dir_cut(0.0f, 250.0f) == kDirCut && far_dir_cut(-0.0f, 250.0f) == kDirCut && far_dir_cut(30.0f, 250.0f) == kDirCut && far_dir_cut(nan, 250.0f) == kDirCut);
    CHECK(far_dir_cut(-inf, 250.0f) == kDirCut && far_dir_cut(-FLT_MAX, 0.5f) == kDirCut); // the quotient is not finite
    CHECK(far_dir_cut(-1e-7f, 250.0f) == kDirCut);                                        // ... or below FLT_EPSILON
    // ... and the bench's floor: y = -30 under the camera, far 250
    CHECK(far_dir_cut(-30.0f, 250.0f) == -(0.12f * kFarShrink));

    std::printf("%llu pairs (%llu with a far cut, %llu of them in the exponent sweep), %llu lanes, %llu dropped by the far cut alone\n", t.pairs, t.pairs_with_cut,
                cuts_in_sweep, t.lanes, t.dropped);
    CHECK(t.bad == 0);
    // a check that never sees a dropped lane proves nothing
    CHECK(t.dropped > 0 && t.pairs_with_cut > 10000ull && cuts_in_sweep > 10000ull);
    CHECK(t.cut_pairs_without_drop == 0);
    CHECK(t.dropped >= 4096ull * t.pairs_with_cut / 2ull);

    if (g_failed == 0) std::printf("all far-threshold host checks passed\n");
    return g_failed == 0 ? 0 : 1;
}
