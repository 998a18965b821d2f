// Unit tests of rtxplan::plan_supersample (csrc/rtx_plan.hpp) -- the geometry of a supersampled launch's sample frame -- on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/test_supersample_plan.cpp -o t && ./t
// (tests/test_host_supersample.py builds and runs it).  No HIP, no GPU.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

#include <cstdio>
#include <vector>

using namespace rtxplan;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            g_failed++;                                                          \
        }                                                                        \
    } while (0)

static void test_geometry()
{
    // the console sizes and 1080p, whole frames
    const uint64_t sizes[][2] = {{160, 50}, {400, 150}, {1920, 1080}, {37, 19}, {1, 1}, {2, 1}, {259, 3}};
    for (const auto& wh : sizes) {
        for (int S = 1; S <= 4; S++) {
            const uint64_t W = wh[0], H = wh[1], s = (uint64_t)S;
            const SamplePlan p = plan_supersample(W, H, 0, H, S);
            CHECK(p.ok);
            CHECK(p.W == s * W && p.H == s * H && p.row0 == 0 && p.rows == s * H);
            CHECK(p.bytes == 32u * s * s * W * H && p.cells == W * H);
        }
    }
    // S = 1 is the frame itself
    const SamplePlan one = plan_supersample(400, 150, 7, 20, 1);
    CHECK(one.ok && one.W == 400 && one.H == 150 && one.row0 == 7 && one.rows == 20 && one.bytes == 32u * 400u * 20u);
}

// Slabs of a frame give sample slabs that tile the sample frame in order, and every sample a cell owns lies in its slab's buffer.
static void test_slabs_tile()
{
    const uint64_t W = 37, H = 19;
    for (int S = 2; S <= 4; S++) {
        for (int n = 1; n <= 5; n++) {
            uint64_t next = 0, bytes = 0;
            for (int r = 0; r < n; r++) {
                const Slab sl = slab_of(H, r, n);
                const SamplePlan p = plan_supersample(W, H, sl.row0, sl.rows, S);
                CHECK(p.ok && p.row0 == next && p.rows == (uint64_t)S * sl.rows);
                next = p.row0 + p.rows;
                bytes += p.bytes;
                if (sl.rows == 0) {
                    CHECK(p.bytes == 0 && p.cells == 0);
                    continue;
                }
                // the last sample of the last cell that is folded, as the fold kernel addresses it (two 16-byte loads per sample)
                std::vector<unsigned char> buffer((size_t)p.bytes);
                const uint64_t lrow = sl.rows - 1, col = W - 2, j = (uint64_t)S - 1, i = (uint64_t)S - 1;
                const uint64_t at = (((uint64_t)S * lrow + j) * p.W + (uint64_t)S * col + i) * kSampleBytes;
                CHECK(at + kSampleBytes <= p.bytes);
                buffer[(size_t)(at + kSampleBytes - 1)] = 1; // (under ASan: inside the allocation)
                CHECK(buffer[(size_t)(at + kSampleBytes - 1)] == 1);
            }
            CHECK(next == (uint64_t)S * H && bytes == 32u * (uint64_t)(S * S) * W * H);
        }
    }
}

static void test_refusals()
{
    CHECK(!plan_supersample(37, 19, 0, 19, 0).ok);
    CHECK(!plan_supersample(37, 19, 0, 19, 5).ok);
    CHECK(!plan_supersample(37, 19, 0, 19, -1).ok);
    CHECK(!plan_supersample(0, 19, 0, 19, 2).ok);
    CHECK(!plan_supersample(37, 0, 0, 0, 2).ok);
    CHECK(!plan_supersample(37, 19, 20, 0, 2).ok);  // row0 beyond the frame
    CHECK(!plan_supersample(37, 19, 10, 10, 2).ok); // rows run past it
    CHECK(plan_supersample(37, 19, 19, 0, 2).ok);   // an empty slab at the end
    // the sample frame's sides stay below 2^31
    const uint64_t lim = 1ull << 31;
    CHECK(!plan_supersample(1ull << 30, 1, 0, 1, 4).ok);
    CHECK(!plan_supersample(1, 1ull << 30, 0, 1, 4).ok);
    CHECK(plan_supersample(1ull << 30, 1, 0, 1, 1).ok);
    CHECK(!plan_supersample(1ull << 30, 1, 0, 1, 2).ok); // 2^31 itself
    CHECK(plan_supersample((1ull << 30) - 1, 1, 0, 1, 2).ok);
    CHECK(!plan_supersample(lim, 1, 0, 1, 1).ok && !plan_supersample(1, lim, 0, 1, 1).ok);
    CHECK(!plan_supersample(~0ull, ~0ull, 0, 1, 4).ok); // nothing wraps
    // the byte count never wraps: a buffer of 2^63 bytes or more is refused, the largest below it is exact
    CHECK(!plan_supersample(lim / 4 - 1, lim / 4 - 1, 0, lim / 4 - 1, 4).ok); // 32 (2^31 - 4)^2 is about 2^67
    const SamplePlan big = plan_supersample(lim / 4 - 1, lim / 4 - 1, 0, 1u << 25, 4);
    CHECK(big.ok && big.W == lim - 4 && big.rows == 1u << 27 && big.bytes == 32u * (lim - 4) * (1ull << 27) && big.bytes / 32u / big.W == big.rows);
}

int main()
{
    test_geometry();
    test_slabs_tile();
    test_refusals();
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all supersample planning tests passed\n");
    return 0;
}
