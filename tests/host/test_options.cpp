// The option table of csrc/rtx_options.hpp against the rows of rtx_set_option's switch as it stood before there was a table, written
// out here by hand: number, lo, hi, the extra value where the range has a hole (else lo again), default, refusal text.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_options.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>

namespace {

struct Want {
    int option;
    int64_t lo, hi, extra, dflt;
    const char* refusal;
};

const Want kWant[] = {
    {1, 0, 2, 0, 0, "RTX_OPT_KERNEL: unknown kernel"},
    {2, 2, 6, 0, 0, "RTX_OPT_TILE_LOG2_W: 0 or 2..6"},
    {3, 0, 16, 0, 0, "RTX_OPT_SUBTILES: 0..16"},
    {4, -1, 2, -1, -1, "RTX_OPT_TWO_LEVEL: -1 (auto), 0 or 1 (2 is accepted as 1)"},
    {5, -1, 1, -1, -1, "RTX_OPT_REFINE: -1 (auto), 0 or 1"},
    {6, -1, 1048576, -1, -1, "RTX_OPT_TILE_ORDER: -1 (auto), 0 (off) or the refresh period in frames"},
    {7, 0, 2147483648ll, 0, 0, "RTX_OPT_CELL_CAPACITY: 0 (auto) or entries per cell list"},
    {8, -1, 1, -1, -1, "RTX_OPT_CELL_REUSE: -1 (auto), 0 or 1"},
    {9, -1, 1, -1, -1, "RTX_OPT_XCD_ORDER: -1 (auto), 0 or 1"},
    {10, -1, 1, -1, -1, "RTX_OPT_VIEW_ADAPT: -1 (auto), 0 or 1"},
    {11, -1, 1, -1, -1, "RTX_OPT_SORTED_STORE: -1 (auto), 0 or 1"},
    {14, -1, 1, -1, -1, "RTX_OPT_BATCH: -1 (auto), 0 or 1"},
    {15, -1, 1, -1, -1, "RTX_OPT_UPDATE_WORDS: -1 (auto), 0 or 1"},
    {17, -1, 2, -1, -1, "RTX_OPT_MINIMIZE_FUSED: -1 (auto), 0, 1 or 2"},
    {19, -1, 1, -1, -1, "RTX_OPT_UPDATE_HOST_WRITE: -1 (auto), 0 or 1"},
    {20, 0, 1, 0, 0, "RTX_OPT_SHADOWS: 0 or 1"},
    {21, 0, 2, 0, 0, "RTX_OPT_SHADOW_CHECK: 0, 1 or 2"},
    {22, 0, 2, 0, 0, "RTX_OPT_REFLECT_CHECK: 0, 1 or 2"},
    {23, 0, 1, 0, 0, "RTX_OPT_QUERY_CHECK: 0 or 1"},
    {24, 0, 4096, 0, 0, "RTX_OPT_QUERY_LOAD: 0 (default) or sixteenths of a sphere per cell, up to 4096"},
    {25, 0, 1, 0, 0, "RTX_OPT_LIGHTS_CHECK: 0 or 1"},
    {26, 1, 4, 1, 1, "RTX_OPT_REFLECT_DEPTH: 1 .. RTX_MAX_REFLECT_DEPTH"},
    {27, 0, 1, 0, 0, "RTX_OPT_REFLECT_DEPTH_CHECK: 0 or 1"},
    {28, 0, 1, 0, 0, "RTX_OPT_REFLECT_SHADOWS: 0 or 1"},
    {29, 0, 1, 0, 0, "RTX_OPT_SHADOW_GRID: 0 or 1"},
    {30, 1, 4, 1, 1, "RTX_OPT_SUPERSAMPLE: 1, 2, 3 or 4"},
    {31, 0, 1, 0, 0, "RTX_OPT_REFLECT_GRID: 0 or 1"},
};

int g_failed = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::printf("FAILED %s:%d: %s (option %d)\n", __FILE__, __LINE__, #cond, g_opt); \
            g_failed++;                                                                      \
        }                                                                                    \
    } while (0)
int g_opt = 0;

void accepted(const Want& w, int64_t v)
{
    rtxopt::Options o;
    const char* refusal = nullptr;
    int64_t got = INT64_MIN;
    const rtxopt::Row* r = rtxopt::find(w.option);
    CHECK(r && rtxopt::accepts(*r, v));
    CHECK(rtxopt::set(o, w.option, v, &refusal) && refusal == nullptr);
    CHECK(rtxopt::get(o, w.option, &got) && got == v);
    // nothing else moved
    for (const Want& other : kWant) {
        if (other.option == w.option) continue;
        CHECK(rtxopt::get(o, other.option, &got) && got == other.dflt);
    }
}

void refused(const Want& w, int64_t v)
{
    rtxopt::Options o;
    const char* refusal = nullptr;
    int64_t got = INT64_MIN;
    // from the default and from a stored value that is not the default
    const int64_t stored = w.hi;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) CHECK(rtxopt::set(o, w.option, stored, &refusal));
        refusal = nullptr;
        const rtxopt::Row* r = rtxopt::find(w.option);
        CHECK(r && !rtxopt::accepts(*r, v));
        CHECK(!rtxopt::set(o, w.option, v, &refusal));
        CHECK(refusal && std::strcmp(refusal, w.refusal) == 0);
        CHECK(rtxopt::get(o, w.option, &got) && got == (pass == 0 ? w.dflt : stored));
    }
}

} // namespace

int main()
{
    static_assert(sizeof kWant / sizeof kWant[0] == 27, "27 context options");
    CHECK(sizeof rtxopt::kRows / sizeof rtxopt::kRows[0] == 27);
    CHECK(sizeof(rtxopt::Options) == 27 * sizeof(int64_t)); // a field each, nothing else
    for (const Want& w : kWant) {
        g_opt = w.option;
        const rtxopt::Options fresh;
        int64_t got = INT64_MIN;
        CHECK(rtxopt::get(fresh, w.option, &got) && got == w.dflt);
        int rows = 0;
        for (const rtxopt::Row& r : rtxopt::kRows) rows += r.option == w.option ? 1 : 0;
        CHECK(rows == 1);
        accepted(w, w.lo);
        accepted(w, w.hi);
        accepted(w, w.extra);
        refused(w, w.lo - 1);
        refused(w, w.hi + 1);
        refused(w, INT64_MIN);
        refused(w, INT64_MAX);
        if (w.extra < w.lo) {
            for (int64_t v = w.extra + 1; v < w.lo; v++) refused(w, v); // the hole
        }
    }
    // RTX_OPT_TILE_LOG2_W: 0 or 2..6
    g_opt = 2;
    refused(kWant[1], 1);
    refused(kWant[1], 7);
    refused(kWant[1], -1);
    for (int64_t v = 2; v <= 6; v++) accepted(kWant[1], v);
    // the quirks: 2 stays 2; the two large upper ends are inclusive
    g_opt = 4;
    accepted(kWant[3], 2);
    g_opt = 7;
    accepted(kWant[6], 1ll << 31);
    refused(kWant[6], (1ll << 31) + 1);
    g_opt = 6;
    accepted(kWant[5], 1 << 20);
    refused(kWant[5], (1 << 20) + 1);

    // numbers that are no context option: nothing, counters, the four options of a device group
    for (const int option : {0, -1, 32, 101, 12, 13, 16, 18}) {
        g_opt = option;
        rtxopt::Options o;
        const char* refusal = nullptr;
        int64_t got = 77;
        CHECK(rtxopt::find(option) == nullptr);
        CHECK(!rtxopt::get(o, option, &got) && got == 77);
        CHECK(!rtxopt::set(o, option, 0, &refusal) && refusal && std::strcmp(refusal, "unknown option") == 0);
        for (const Want& w : kWant) CHECK(rtxopt::get(o, w.option, &got) && got == w.dflt);
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all option table tests passed\n");
    return 0;
}
