// rtxplan::cup_length, delta_run_bound, delta_bound and delta_block_bound (csrc/rtx_plan.hpp) without a GPU: the lengths the delta
// frames' buffers and the block's LDS image are sized by, against brute force over every change pattern of small rows.
// tests/test_host_delta.py compiles this as host-only C++ and runs it under AddressSanitizer + UndefinedBehaviorSanitizer.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

#include <cstdio>
#include <string>

static int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

// the escape as a terminal reads it, formatted by the C library
static size_t cup_by_printf(size_t row, size_t col)
{
    char b[64];
    return (size_t)std::snprintf(b, sizeof b, "\x1b[%zu;%zuH", row + 1, col + 1);
}

// The stream length of slots [lo, hi) of a W x H frame whose cell (row, col) changed iff bit row * (W - 1) + col of `pattern` is set,
// by the rule of rtx.h with every record whole (the longest a cell can be); `flat` != 0: every escape costs `flat` bytes instead of
// its own length.
static size_t stream_length(size_t S, size_t W, size_t H, unsigned long pattern, size_t lo, size_t hi, size_t flat)
{
    size_t n = 0;
    for (size_t g = lo; g < hi && g < W * H; g++) {
        const size_t row = g / W, col = g % W;
        if (col == W - 1) continue;
        auto changed = [&](size_t r, size_t c) { return ((pattern >> (r * (W - 1) + c)) & 1ul) != 0; };
        if (!changed(row, col)) continue;
        n += S;
        if (col == 0 || !changed(row, col - 1)) n += flat ? flat : cup_by_printf(row, col);
    }
    return n;
}

int main()
{
    using namespace rtxplan;
    // cup_length at the digit transitions: index 8 is printed as 9, index 9 as 10, ...
    for (size_t edge : {9u, 99u, 999u, 9999u}) {
        for (size_t a : {edge - 1, edge}) {
            for (size_t b : {(size_t)0, edge - 1, edge, (size_t)kDeltaMaxIndex - 1}) {
                CHECK(cup_length(a, b) == cup_by_printf(a, b));
                CHECK(cup_length(b, a) == cup_by_printf(b, a));
            }
        }
        CHECK(cup_length(edge, 0) == cup_length(edge - 1, 0) + 1);
        CHECK(cup_length(0, edge) == cup_length(0, edge - 1) + 1);
    }
    CHECK(cup_length(0, 0) == 6 && cup_length(kDeltaMaxIndex - 1, kDeltaMaxIndex - 1) == kDeltaMaxCup);

    for (size_t S : {(size_t)12, (size_t)20}) {
        // one row of up to 12 cells, every pattern: no stream is longer than delta_bound, and with every escape at the length of
        // the row's longest the bound is reached exactly
        for (size_t cells = 0; cells <= 12; cells++) {
            const size_t W = cells + 1;
            size_t worst = 0, worst_flat = 0;
            const size_t flat = cup_length(0, W >= 2 ? W - 2 : 0);
            for (unsigned long p = 0; p < (1ul << cells); p++) {
                worst = std::max(worst, stream_length(S, W, 1, p, 0, W, 0));
                worst_flat = std::max(worst_flat, stream_length(S, W, 1, p, 0, W, flat));
            }
            CHECK(worst <= delta_bound(S, W, 1));
            CHECK(worst_flat == delta_bound(S, W, 1));
            CHECK(delta_run_bound(S, flat, cells) == worst_flat);
            // every window of the row is a block: with an escape of `cup` bytes (shorter and longer than a record) the block bound is
            // the longest window, exactly
            for (size_t cup : {(size_t)6, (size_t)kDeltaMaxCup}) {
                for (size_t slots = 1; slots <= W; slots++) {
                    size_t longest = 0;
                    for (unsigned long p = 0; p < (1ul << cells); p++) {
                        for (size_t lo = 0; lo + slots <= W; lo++) longest = std::max(longest, stream_length(S, W, 1, p, lo, lo + slots, cup));
                    }
                    CHECK(longest <= delta_run_bound(S, cup, slots));
                    if (slots < W) CHECK(longest == delta_run_bound(S, cup, slots)); // (a window of cells alone reaches it)
                }
            }
        }
        // blocks that span rows: frames of up to 12 cells in rows of 1 .. 4 cells, every pattern, every window
        for (size_t W = 2; W <= 5; W++) {
            for (size_t H = 1; (W - 1) * H <= 12; H++) {
                const size_t cells = (W - 1) * H;
                size_t whole = 0;
                for (unsigned long p = 0; p < (1ul << cells); p++) {
                    whole = std::max(whole, stream_length(S, W, H, p, 0, W * H, 0));
                    for (size_t slots = 1; slots <= W * H; slots += (slots < 4 ? 1 : 3)) {
                        for (size_t lo = 0; lo + slots <= W * H; lo++) {
                            CHECK(stream_length(S, W, H, p, lo, lo + slots, kDeltaMaxCup) <= delta_block_bound(S, slots));
                        }
                    }
                }
                CHECK(whole == delta_bound(S, W, H)); // (one digit each: every escape has the row's longest length)
            }
        }
        // rows of different digit counts add up
        CHECK(delta_bound(S, 3, 12) == 9 * delta_run_bound(S, 6, 2) + 3 * delta_run_bound(S, 7, 2));
        CHECK(delta_bound(S, 1, 50) == 0 && delta_bound(S, 0, 5) == 0 && delta_bound(S, 5, 0) == 0);
        CHECK(delta_bound(S, 100000, 99999) >= S * 99999 * 99999);
    }
    // the image of a 1024-slot block: more than 1024 S for both record sizes
    CHECK(delta_block_bound(12, 1024) == 13324 && delta_block_bound(20, 1024) == 20494);
    if (g_failed) return 1;
    std::printf("all delta planning tests passed\n");
    return 0;
}
