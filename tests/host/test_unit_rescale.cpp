// Host proof of csrc/rtx_unit.hpp -- the factor RN(1 / RN(sqrt(x))) of nearly-unit squared lengths as an integer rule:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/test_unit_rescale.cpp -o t && ./t
// (tests/test_host_unit_rescale.py builds and runs it).  No HIP, no GPU.  Host sqrtf and 1.0f / x are IEEE: they are the truth.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_unit.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

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
// the two IEEE operations of Normalize_GPU, each rounded to fp32 (volatile: no double-precision shortcut, no folding)
static uint32_t truth(uint32_t x_bits)
{
    volatile float x = float_of(x_bits);
    volatile float root = sqrtf(x);
    volatile float r = 1.0f / root;
    return bits_of(r);
}

// what the device does with a squared length (rtx_device.hpp: unit_rescale), the table as the kernels fill it
static uint32_t g_table[kUnitEntries];
static bool window_lookup(uint32_t len2_bits, uint32_t* out)
{
    const uint32_t slot = unit_slot(len2_bits);
    if (slot >= kUnitEntries) return false; // the device takes 1.0f / sqrtf(x) itself here
    *out = g_table[slot];
    return true;
}

int main()
{
    for (uint32_t i = 0; i < kUnitEntries; i++) g_table[i] = unit_rescale_bits((int32_t)i + kUnitKMin);

    // the window covers what the issue asks for, and the observed offsets [-7, +3] with room below
    CHECK(kUnitKMin <= -12 && kUnitKMax >= 3);
    CHECK(kUnitEntries <= 16u);

    // every k of the shipped window, and 64 on each side: the rule is the truth
    for (int32_t k = kUnitKMin - 64; k <= kUnitKMax + 64; k++) {
        const uint32_t x = kUnitOneBits + (uint32_t)k;
        if (unit_rescale_bits(k) != truth(x)) {
            std::printf("FAIL rule at k = %d: 0x%08x, 1.0f / sqrtf gives 0x%08x\n", k, unit_rescale_bits(k), truth(x));
            g_failed++;
        }
    }
    // ... and on the whole range the header states, failing first just outside it
    int wrong_inside = 0;
    for (int32_t k = kUnitRuleMin; k <= kUnitRuleMax; k++) wrong_inside += unit_rescale_bits(k) != truth(kUnitOneBits + (uint32_t)k);
    CHECK(wrong_inside == 0);
    CHECK(unit_rescale_bits(kUnitRuleMin - 1) != truth(kUnitOneBits + (uint32_t)(kUnitRuleMin - 1)));
    CHECK(unit_rescale_bits(kUnitRuleMax + 1) != truth(kUnitOneBits + (uint32_t)(kUnitRuleMax + 1)));

    // the lookup: inside the window exactly the table (= the truth), outside it never answered from the rule --
    // one step beyond each end, the ends of the rule's range, and the values the unsigned compare must turn away
    for (int32_t k = kUnitKMin; k <= kUnitKMax; k++) {
        uint32_t got = 0;
        CHECK(window_lookup(kUnitOneBits + (uint32_t)k, &got) && got == truth(kUnitOneBits + (uint32_t)k));
    }
    uint32_t dummy;
    const uint32_t outside[] = {kUnitOneBits + (uint32_t)(kUnitKMin - 1), kUnitOneBits + (uint32_t)(kUnitKMax + 1),
                                kUnitOneBits + (uint32_t)kUnitRuleMin, kUnitOneBits + (uint32_t)kUnitRuleMax,
                                kUnitOneBits + (uint32_t)(kUnitKMin - 64), kUnitOneBits + (uint32_t)(kUnitKMax + 64),
                                0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x3f000000u, 0x40000000u,
                                0xbf800000u, 0xbf7ffffcu, 0x7f7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                                0x7f800001u, 0xffffffffu, kUnitOneBits + 16u, kUnitOneBits - 16u, kUnitOneBits + 0x80000000u};
    for (uint32_t x : outside) CHECK(!window_lookup(x, &dummy));
    // exactly kUnitEntries of all bit patterns are answered from the table (a sweep of the slot function's whole period would
    // take seconds; the slot is x minus a constant, so it is below kUnitEntries for exactly that many consecutive x)
    uint32_t answered = 0;
    for (uint32_t x = kUnitOneBits - 70000u; x != kUnitOneBits + 70000u; x++) answered += window_lookup(x, &dummy);
    CHECK(answered == kUnitEntries);

    if (g_failed == 0) std::printf("all unit-rescale host checks passed\n");
    return g_failed == 0 ? 0 : 1;
}
