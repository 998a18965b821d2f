// rtxplan::half_bound and half_block_bound (csrc/rtx_plan.hpp) without a GPU: the lengths the half-block frames' buffers and the
// block's LDS image are sized by, against brute force over every elision pattern of small frames and against overflow.
// tests/test_host_half.py compiles this as host-only C++ and runs it under AddressSanitizer + UndefinedBehaviorSanitizer.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

#include <algorithm>
#include <cstdio>

static int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

// the longest escape of a family, formatted by the C library
static size_t escape_by_printf(bool rgb)
{
    char b[64];
    return (size_t)(rgb ? std::snprintf(b, sizeof b, "\x1b[38;2;%d;%d;%dm", 255, 255, 255) : std::snprintf(b, sizeof b, "\x1b[48;5;%dm", 255));
}

// The stream length of slots [lo, hi) of a W x H frame by the rule of rtx.h with every escape at E bytes: cell k (in frame order)
// emits its foreground escape iff bit 2k of `pattern` is set, its background escape iff bit 2k + 1 is; the frame's first cell
// emits both whatever the pattern.
static size_t stream_length(size_t E, size_t W, size_t H, unsigned long pattern, size_t lo, size_t hi)
{
    size_t n = 0;
    for (size_t g = lo; g < hi && g < W * H; g++) {
        const size_t row = g / W, col = g % W;
        if (col == W - 1) {
            n += 1;
            continue;
        }
        const size_t k = row * (W - 1) + col;
        const bool fg = k == 0 || ((pattern >> (2 * k)) & 1ul) != 0, bg = k == 0 || ((pattern >> (2 * k + 1)) & 1ul) != 0;
        n += 3 + (fg ? E : 0) + (bg ? E : 0);
    }
    return n;
}

int main()
{
    using namespace rtxplan;
    CHECK(kHalfEscRgb == escape_by_printf(true) && kHalfEsc8 == escape_by_printf(false) && kHalfGlyph == sizeof("\xe2\x96\x80") - 1);
    for (size_t E : {(size_t)kHalfEsc8, (size_t)kHalfEscRgb}) {
        // frames of up to 10 cells, every pattern: no stream and no window of one is longer than its bound, and the pattern with
        // every escape due reaches both exactly
        for (size_t W = 1; W <= 6; W++) {
            for (size_t H = 1; (W - 1) * H <= 10 && H <= 4; H++) {
                const size_t cells = (W - 1) * H;
                size_t whole = 0;
                for (unsigned long p = 0; p < (1ul << (2 * cells)); p += (cells > 6 ? 5 : 1)) { // (a stride that keeps the all-ones pattern out: added below)
                    whole = std::max(whole, stream_length(E, W, H, p, 0, W * H));
                }
                const unsigned long all = (1ul << (2 * cells)) - 1ul;
                whole = std::max(whole, stream_length(E, W, H, all, 0, W * H));
                CHECK(whole == half_bound(E, W, H));
                CHECK(half_bound(E, W, H) == H * ((W - 1) * (2 * E + 3) + 1));
                for (size_t slots = 1; slots <= W * H; slots++) {
                    size_t longest = 0;
                    for (size_t lo = 0; lo + slots <= W * H; lo++) longest = std::max(longest, stream_length(E, W, H, all, lo, lo + slots));
                    CHECK(longest <= half_block_bound(E, slots));
                    if (slots < W) CHECK(longest == half_block_bound(E, slots)); // (a window of cells alone reaches it)
                }
            }
        }
        CHECK(half_bound(E, 1, 50) == 50 && half_bound(E, 0, 5) == 0 && half_bound(E, 5, 0) == 0);
        CHECK(half_block_bound(E, 0) == 0 && half_block_bound(E, 1) == 2 * E + 3);
        // the largest frame the entry points take, and products that do not fit: 0, never a wrapped number
        const size_t big = ((size_t)1 << 31) - 1, rows = ((size_t)1 << 30) - 1, top = ~(size_t)0;
        if (sizeof(size_t) == 8) {
            CHECK(half_bound(E, big, 1000) == 1000 * ((big - 1) * (2 * E + 3) + 1));
            CHECK(half_bound(E, big, rows) == 0); // (2^61 cells of 25 bytes and more)
            CHECK(half_bound(E, 100000, rows) == rows * (99999 * (2 * E + 3) + 1));
        }
        CHECK(half_bound(E, top, 1) == 0 && half_bound(E, top, top) == 0 && half_bound(E, 2, top) == 0 && half_bound(E, top / 2, 4) == 0);
        CHECK(half_bound(E, 2, top / (2 * E + 4)) == (top / (2 * E + 4)) * (2 * E + 4)); // (the last H that fits ...)
        CHECK(half_bound(E, 2, top / (2 * E + 4) + 1) == 0);                             // (... and the first that does not)
        CHECK(half_block_bound(E, top) == 0 && half_block_bound(E, top / (2 * E + 3)) == (top / (2 * E + 3)) * (2 * E + 3));
        CHECK(half_block_bound(E, top / (2 * E + 3) + 1) == 0);
    }
    CHECK(half_bound(65, 4, 4) == 0 && half_block_bound(65, 4) == 0); // (no escape is that long)
    // the image of a 1024-slot block
    CHECK(half_block_bound(kHalfEscRgb, 1024) == 41984 && half_block_bound(kHalfEsc8, 1024) == 25600);
    CHECK(half_bound(kHalfEscRgb, 160, 50) == 50 * (159 * 41 + 1));
    if (g_failed) return 1;
    std::printf("all half-block planning tests passed\n");
    return 0;
}
