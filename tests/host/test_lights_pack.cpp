// Host test of csrc/rtx_lights.hpp (validation of a light set and its packing into the kernel argument block), built under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_host_lights.py.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_lights.hpp"

static int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);    \
            failures++;                                              \
        }                                                            \
    } while (0)

static rtx_light light_no(int i)
{
    rtx_light l;
    l.pos[0] = 1.0f + (float)i;
    l.pos[1] = 50.0f - (float)i;
    l.pos[2] = 2.0f * (float)i;
    l.diffuse_rgb[0] = 1.0f;
    l.diffuse_rgb[1] = 0.5f / (float)(i + 1);
    l.diffuse_rgb[2] = 0.0f;
    l.diffuse_power = 2000.0f + (float)i;
    l.specular_rgb[0] = 0.25f;
    l.specular_rgb[1] = 1.0f;
    l.specular_rgb[2] = (float)i;
    l.specular_power = (float)(i % 2) * 3000.0f; // (a power of 0 is allowed)
    return l;
}

static float* field(rtx_light& l, int k) // the 11 floats in declaration order
{
    if (k < 3) return &l.pos[k];
    if (k < 6) return &l.diffuse_rgb[k - 3];
    if (k == 6) return &l.diffuse_power;
    if (k < 10) return &l.specular_rgb[k - 7];
    return &l.specular_power;
}

static rtxlights::Block sentinel()
{
    rtxlights::Block b;
    memset(&b, 0x5a, sizeof b);
    return b;
}

int main()
{
    static_assert(rtxlights::kMaxLights == 8, "RTX_MAX_LIGHTS");
    static_assert(sizeof(rtxlights::PackedLight) == 44 && sizeof(rtx_light) == 44, "a light is 44 bytes");
    static_assert(sizeof(rtxlights::Block) == 4 + 8 * 44, "count + 8 lights");

    rtx_light set[9];
    for (int i = 0; i < 9; i++) set[i] = light_no(i);

    // n = 1 .. 8: accepted, in order, the rest of the block zero
    for (size_t n = 1; n <= 8; n++) {
        rtxlights::Block b = sentinel();
        CHECK(rtxlights::set_fault(n, set) == nullptr);
        CHECK(rtxlights::pack(n, set, &b));
        CHECK(b.n == n);
        for (size_t i = 0; i < 8; i++) {
            const rtxlights::PackedLight& q = b.light[i];
            if (i < n) {
                const rtx_light& l = set[i];
                CHECK(q.px == l.pos[0] && q.py == l.pos[1] && q.pz == l.pos[2]);
                CHECK(q.dr == l.diffuse_rgb[0] && q.dg == l.diffuse_rgb[1] && q.db == l.diffuse_rgb[2] && q.dpow == l.diffuse_power);
                CHECK(q.sr == l.specular_rgb[0] && q.sg == l.specular_rgb[1] && q.sb == l.specular_rgb[2] && q.spow == l.specular_power);
            } else {
                const rtxlights::PackedLight zero = {};
                CHECK(memcmp(&q, &zero, sizeof zero) == 0);
            }
        }
    }

    // refused: n = 0, n = 9, no list, no destination -- and the destination untouched
    const rtxlights::Block want = sentinel();
    {
        rtxlights::Block b = sentinel();
        size_t bad = 77;
        CHECK(!rtxlights::pack(0, set, &b) && memcmp(&b, &want, sizeof b) == 0);
        CHECK(!rtxlights::pack(9, set, &b) && memcmp(&b, &want, sizeof b) == 0);
        CHECK(!rtxlights::pack(3, nullptr, &b) && memcmp(&b, &want, sizeof b) == 0);
        CHECK(!rtxlights::pack(3, set, nullptr));
        CHECK(rtxlights::set_fault(0, set, &bad) != nullptr && bad == 0);
        CHECK(rtxlights::set_fault(9, set, &bad) != nullptr && bad == 9);
        CHECK(rtxlights::set_fault(3, nullptr, &bad) != nullptr && bad == 3);
    }

    // refused: NaN / inf in any field, a negative power or colour component, at any position of a list of any length
    const float poison[4] = {NAN, INFINITY, -INFINITY, -1.0f};
    long refused = 0;
    for (size_t n = 1; n <= 8; n++) {
        for (size_t at = 0; at < n; at++) {
            for (int k = 0; k < 11; k++) {
                for (int v = 0; v < 4; v++) {
                    if (v == 3 && k < 3) continue; // (a negative coordinate is a good position)
                    rtx_light list[8];
                    for (size_t i = 0; i < n; i++) list[i] = set[i];
                    *field(list[at], k) = poison[v];
                    rtxlights::Block b = sentinel();
                    size_t bad = 77;
                    CHECK(rtxlights::set_fault(n, list, &bad) != nullptr && bad == at);
                    CHECK(!rtxlights::pack(n, list, &b));
                    CHECK(memcmp(&b, &want, sizeof b) == 0);
                    refused++;
                }
            }
        }
    }
    // a negative coordinate and -0.0f anywhere are fine
    {
        rtx_light list[2] = {set[0], set[1]};
        list[1].pos[1] = -40.0f;
        list[0].diffuse_power = -0.0f;
        rtxlights::Block b = sentinel();
        CHECK(rtxlights::pack(2, list, &b) && b.n == 2 && b.light[1].py == -40.0f);
    }

    if (failures == 0) printf("all lights pack tests passed (%ld refused sets)\n", refused);
    return failures == 0 ? 0 : 1;
}
