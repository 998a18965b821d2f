// Unit tests of rtxplan::edit_effect (csrc/rtx_plan.hpp) -- what an edit of spheres in place (rtx_scene_set_spheres) means for the
// cell lists, the dispatch orders and the physics bound, from the two words rtx_write_spheres leaves -- on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/test_scene_edit.cpp -o t && ./t
// (tests/test_host_scene_edit.py builds and runs it).  No HIP, no GPU.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_plan.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

using namespace rtxplan;

static int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();

    // nothing moved, nothing flagged (a colour-only edit): costs nothing
    {
        const EditEffect e = edit_effect(0.0f, 0u);
        CHECK(e.drift_add == 0.0 && !e.invalidate_lists && !e.unsettle_physics);
    }
    // a finite move is motion: exactly that drift, the lists stay
    for (float m : {1.0e-30f, 0.05f, 0.1f, 3.0f, 123.456f, 3.0e38f}) {
        const EditEffect e = edit_effect(m, 0u);
        CHECK(e.drift_add == (double)m);
        CHECK(!e.invalidate_lists && !e.unsettle_physics);
    }
    // every combination of the flags, with and without a move
    for (float m : {0.0f, 0.25f}) {
        for (unsigned f = 0; f < 8; f++) {
            const EditEffect e = edit_effect(m, f);
            const bool full = (f & 3u) != 0u;
            CHECK(e.invalidate_lists == full);
            CHECK(e.unsettle_physics == ((f & 4u) != 0u));
            // a grown radius is not covered by the lists' position budget: never counted as motion
            CHECK(e.drift_add == (full ? 1.0e3 : (double)m));
        }
    }
    // each flag alone
    CHECK(edit_effect(0.5f, 1u).invalidate_lists && !edit_effect(0.5f, 1u).unsettle_physics);
    CHECK(edit_effect(0.5f, 2u).invalidate_lists && !edit_effect(0.5f, 2u).unsettle_physics);
    CHECK(!edit_effect(0.5f, 4u).invalidate_lists && edit_effect(0.5f, 4u).unsettle_physics && edit_effect(0.5f, 4u).drift_add == 0.5);
    // bits the kernel never sets change nothing
    CHECK(!edit_effect(0.5f, 8u).invalidate_lists && !edit_effect(0.5f, 0xfffffff8u).unsettle_physics);
    // a move without a bound always invalidates, whatever the flags say, and the drift stays a number
    for (float m : {inf, nan, -inf, -1.0f}) {
        for (unsigned f = 0; f < 8; f++) {
            const EditEffect e = edit_effect(m, f);
            CHECK(e.invalidate_lists);
            CHECK(e.drift_add == 1.0e3);
            CHECK(e.unsettle_physics == ((f & 4u) != 0u));
        }
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all scene edit planning tests passed\n");
    return 0;
}
