// Host proof of csrc/rtx_unit.hpp's second rule -- divTwoA = RN(1 / RN(2 x)) of nearly-unit squared lengths as an integer rule:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/test_half_recip.cpp -o t && ./t
// (tests/test_host_half_recip.py builds and runs it).  No HIP, no GPU.  Host 2.0f * x and 1.0f / x are IEEE: they are the truth.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_unit.hpp"

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
// the two IEEE operations of RayTracing.cu:93, each rounded to fp32 (volatile: no double-precision shortcut, no folding)
static uint32_t truth(uint32_t x_bits)
{
    volatile float x = float_of(x_bits);
    volatile float twice = 2.0f * x;
    volatile float r = 1.0f / twice;
    return bits_of(r);
}
static bool rule_holds(int32_t k) { return half_recip_bits(k) == truth(kUnitOneBits + (uint32_t)k); }

int main()
{
    // every k from the rule's lower to its upper validity bound
    int wrong_inside = 0;
    for (int32_t k = kHalfRuleMin; k <= kHalfRuleMax; k++) {
        if (!rule_holds(k)) {
            if (wrong_inside++ < 8) std::printf("FAIL rule at k = %d: 0x%08x, 1.0f / (2.0f * x) gives 0x%08x\n", k, half_recip_bits(k), truth(kUnitOneBits + (uint32_t)k));
        }
    }
    CHECK(wrong_inside == 0);

    // the first k on either side where the rule fails, searched from 0 outwards: one past the header's constants
    int32_t up = 0, down = 0;
    while (up < (1 << 22) && rule_holds(up)) up++;
    while (down > -(1 << 22) && rule_holds(down)) down--;
    std::printf("rule holds for k in [%d, %d]\n", down + 1, up - 1);
    CHECK(up == kHalfRuleMax + 1);
    CHECK(down == kHalfRuleMin - 1);

    // the shipped window -- the first table's, slot for slot -- lies inside that range, and its entries are the truth
    CHECK(kUnitKMin <= -12 && kUnitKMax >= 3);
    CHECK(kUnitKMin >= kHalfRuleMin && kUnitKMax <= kHalfRuleMax);
    for (int32_t k = kUnitKMin; k <= kUnitKMax; k++) {
        const uint32_t x = kUnitOneBits + (uint32_t)k;
        CHECK(unit_slot(x) == (uint32_t)(k - kUnitKMin));
        CHECK(half_recip_bits((int32_t)unit_slot(x) + kUnitKMin) == truth(x)); // as half_table_fill fills the slot
    }
    // one step beyond each end is not answered from the table
    CHECK(unit_slot(kUnitOneBits + (uint32_t)(kUnitKMin - 1)) >= kUnitEntries);
    CHECK(unit_slot(kUnitOneBits + (uint32_t)(kUnitKMax + 1)) >= kUnitEntries);

    if (g_failed == 0) std::printf("all half-reciprocal host checks passed\n");
    return g_failed == 0 ? 0 : 1;
}
