// test_refract.cpp -- the glass of rtx_scene_set_refraction on the host (csrc/rtx_refract.hpp):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tests/host/test_refract.cpp -o test_refract
//   1. through_sphere -- the very expressions secondary_ray runs on the device, here with sqrtf and 1.0f / x -- against float64:
//      Snell's refraction at entry, the intersection of the inner ray with the sphere, Snell's refraction at exit.  The fp32
//      inputs (P, N, V, r, ior) are taken as exact; the sphere is the one through P with the normal N / |N|.  Inputs: 200 000
//      random cases (ior in [1, 4], ci in [0.05, 1], r in [0.2, 3], centres within +-5) and a directed grid of ior x ci x r.
//      MEASURED on the machine this was written on (x86-64, glibc): worst exit point 2.13e-06 of r, worst direction 1.19e-06,
//      | |d| - 1 | 6.99e-07.  THE BOUNDS are four times the first two, which leaves room for another libm: kBoundPoint =
//      8.52e-06 (of r) and kBoundDir = 4.76e-06 (also asked of | |d| - 1 |).  The closed form itself, the same expressions in
//      float64, agrees with the two refractions to 2.3e-13 (asked: 3e-12), which is the symmetry argument to rounding;
//   2. normal incidence gives d within the bound of -V; ior = 1 gives d within the bound of -V and o within the bound (of r) of
//      the far side of the sphere, P - V (2 r ci);
//   3. NaN inputs trap nowhere (the sanitizers see every operation), and a NaN c2 takes ct = 0;
//   4. which values a call accepts (the book they are stored in: csrc/rtx_materials.hpp, tests/host/test_materials.cpp).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../raytracing-in-windows-console_amd/csrc/rtx_refract.hpp"

using rtxrefract::through_sphere;

static int g_failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (g_failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            g_failures++;                                           \
        }                                                           \
    } while (0)

static constexpr double kBoundPoint = 8.52e-06; // of r: 4 x the measured worst (header)
static constexpr double kBoundDir = 4.76e-06;   // 4 x the measured worst

static float root32(float x) { return sqrtf(x); }
static float recip32(float x) { return 1.0f / x; }

static void rule32(const float P[3], const float N[3], const float V[3], float r, float ior, float o[3], float d[3])
{
    through_sphere(P, N, V, r, ior, root32, recip32, o, d);
}

struct V3d {
    double x, y, z;
};
static V3d operator+(V3d a, V3d b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3d operator-(V3d a, V3d b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3d operator*(V3d a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static double dotd(V3d a, V3d b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static double lend(V3d a) { return std::sqrt(dotd(a, a)); }
static V3d unit(V3d a) { return a * (1.0 / lend(a)); }

// Snell in float64: the unit direction I (travelling) meets a surface with unit normal n against it (n . I < 0) going from index
// n1 to n2.  false: total internal reflection.
static bool snell(V3d I, V3d n, double n1, double n2, V3d* out)
{
    const double eta = n1 / n2, c = -dotd(n, I), k = 1.0 - eta * eta * (1.0 - c * c);
    if (k < 0.0) return false;
    *out = unit(I * eta + n * (eta * c - std::sqrt(k)));
    return true;
}

// The reference: the ray that leaves the sphere through P with outward unit normal N (radius r, index ior) for a ray arriving
// along -V.  Two refractions and a real intersection.
static bool reference64(V3d P, V3d N, V3d V, double r, double ior, V3d* o, V3d* d)
{
    const V3d C = P - N * r;
    V3d T;
    if (!snell(V * -1.0, N, 1.0, ior, &T)) return false;
    // |P + T s - C|^2 = r^2, s > 0: s = -2 (P - C) . T
    const double s = -2.0 * dotd(P - C, T);
    if (!(s > 0.0)) return false;
    const V3d X = P + T * s;
    const V3d n_in = unit(C - X); // the normal against the ray inside
    if (!snell(T, n_in, ior, 1.0, d)) return false;
    *o = X;
    return true;
}

struct Worst {
    double point = 0.0, dir = 0.0, len = 0.0, closed = 0.0;
    size_t n = 0;
};

static void one_case(V3d C, V3d N, V3d tangent, double r, double ior, double ci, Worst* w)
{
    N = unit(N);
    // V at the angle acos(ci) from N, towards `tangent` (made perpendicular to N)
    V3d tp = tangent - N * dotd(tangent, N);
    if (lend(tp) < 1e-6) return;
    tp = unit(tp);
    const double si = std::sqrt(std::fmax(0.0, 1.0 - ci * ci));
    const V3d V = N * ci + tp * si, P = C + N * r;
    const float Pf[3] = {(float)P.x, (float)P.y, (float)P.z}, Nf[3] = {(float)N.x, (float)N.y, (float)N.z}, Vf[3] = {(float)V.x, (float)V.y, (float)V.z};
    const float rf = (float)r, iorf = (float)ior;
    if (!(iorf >= 1.0f && iorf <= 4.0f)) return;
    float of[3], df[3];
    rule32(Pf, Nf, Vf, rf, iorf, of, df);
    // float64 from the fp32 inputs
    const V3d P64 = {Pf[0], Pf[1], Pf[2]}, N64 = unit(V3d{Nf[0], Nf[1], Nf[2]}), V64 = unit(V3d{Vf[0], Vf[1], Vf[2]});
    if (dotd(N64, V64) < 0.05) return;
    V3d o64, d64;
    const bool ok = reference64(P64, N64, V64, rf, iorf, &o64, &d64);
    CHECK(ok);
    if (!ok) return;
    const V3d og = {of[0], of[1], of[2]}, dg = {df[0], df[1], df[2]};
    w->point = std::fmax(w->point, lend(og - o64) / rf);
    w->dir = std::fmax(w->dir, lend(dg - d64));
    w->len = std::fmax(w->len, std::fabs(lend(dg) - 1.0));
    // the closed form itself, in float64 through the same template
    const double Pd[3] = {P64.x, P64.y, P64.z}, Nd[3] = {N64.x, N64.y, N64.z}, Vd[3] = {V64.x, V64.y, V64.z};
    double od[3], dd[3];
    {
        // (the template is written for float; the same expressions in double, operation for operation)
        const double cid = (Nd[0] * Vd[0] + Nd[1] * Vd[1]) + Nd[2] * Vd[2], eta = 1.0 / (double)iorf;
        const double c2 = 1.0 - (eta * eta) * (1.0 - cid * cid), ct = std::sqrt(c2 > 0.0 ? c2 : 0.0), g = eta * cid - ct;
        double T[3];
        for (int q = 0; q < 3; q++) T[q] = Nd[q] * g - Vd[q] * eta;
        const double L = (2.0 * (double)rf) * ct;
        for (int q = 0; q < 3; q++) od[q] = Pd[q] + T[q] * L;
        const double m = 2.0 * ((T[0] * Vd[0] + T[1] * Vd[1]) + T[2] * Vd[2]);
        for (int q = 0; q < 3; q++) dd[q] = Vd[q] - T[q] * m;
    }
    w->closed = std::fmax(w->closed, std::fmax(lend(V3d{od[0], od[1], od[2]} - o64) / rf, lend(V3d{dd[0], dd[1], dd[2]} - d64)));
    w->n++;
}

static Worst test_against_float64()
{
    Worst w;
    std::mt19937_64 rng(20240911u);
    std::uniform_real_distribution<double> centre(-5.0, 5.0), rad(0.2, 3.0), index(1.0, 4.0), cosine(0.05, 1.0), comp(-1.0, 1.0);
    for (int i = 0; i < 200000; i++) {
        const V3d C = {centre(rng), centre(rng), centre(rng)}, N = {comp(rng), comp(rng), comp(rng)}, t = {comp(rng), comp(rng), comp(rng)};
        if (lend(N) < 0.1) continue;
        one_case(C, N, t, rad(rng), index(rng), cosine(rng), &w);
    }
    // directed: the ends and the middle of every range, axis normals, centres on the axes
    const double iors[] = {1.0, 1.0000001, 1.3, 1.5, 2.0, 3.999, 4.0}, cis[] = {0.05, 0.0500001, 0.3, 0.70710678, 0.999, 0.9999999, 1.0}, rs[] = {0.2, 1.0, 3.0};
    const V3d Ns[] = {{1, 0, 0}, {0, 1, 0}, {0, 0, -1}, {1, 1, 1}, {-0.3, 0.9, 0.1}}, ts[] = {{0, 1, 0}, {0, 0, 1}, {1, 0.2, 0}, {1, -1, 0.5}, {0.5, 0.5, -1}};
    const V3d Cs[] = {{0, 0, 0}, {5, 0, 0}, {-5, 5, -5}};
    for (const double ior : iors)
        for (const double ci : cis)
            for (const double r : rs)
                for (int k = 0; k < 5; k++)
                    for (const V3d& C : Cs) one_case(C, Ns[k], ts[k], r, ior, ci, &w);
    std::printf("against float64: %zu cases, worst exit point %.3g of r, worst direction %.3g, | |d| - 1 | %.3g, closed form in float64 %.3g\n",
                w.n, w.point, w.dir, w.len, w.closed);
    CHECK(w.n > 195000);
    CHECK(w.point <= kBoundPoint);
    CHECK(w.dir <= kBoundDir);
    CHECK(w.closed <= 3e-12); // (the symmetry argument, to rounding)
    CHECK(w.len <= kBoundDir);
    return w;
}

// ---------------------------------------------------------------- 2. normal incidence, ior = 1

static void test_special_cases()
{
    std::mt19937_64 rng(77u);
    std::uniform_real_distribution<double> centre(-5.0, 5.0), rad(0.2, 3.0), index(1.0, 4.0), cosine(0.05, 1.0), comp(-1.0, 1.0);
    for (int i = 0; i < 20000; i++) {
        V3d N = {comp(rng), comp(rng), comp(rng)}, t = {comp(rng), comp(rng), comp(rng)};
        if (lend(N) < 0.1) continue;
        N = unit(N);
        V3d tp = t - N * dotd(t, N);
        if (lend(tp) < 1e-6) continue;
        tp = unit(tp);
        const V3d C = {centre(rng), centre(rng), centre(rng)};
        const float r = (float)rad(rng);
        const V3d P = C + N * (double)r;
        const float Pf[3] = {(float)P.x, (float)P.y, (float)P.z}, Nf[3] = {(float)N.x, (float)N.y, (float)N.z};
        float o[3], d[3];
        // normal incidence: V = N, any index -- straight through the centre
        rule32(Pf, Nf, Nf, r, (float)index(rng), o, d);
        CHECK(lend(V3d{d[0] + Nf[0], d[1] + Nf[1], d[2] + Nf[2]}) <= kBoundDir);
        CHECK(lend(V3d{o[0] - (Pf[0] - 2.0 * r * Nf[0]), o[1] - (Pf[1] - 2.0 * r * Nf[1]), o[2] - (Pf[2] - 2.0 * r * Nf[2])}) <= kBoundPoint * r);
        // ior = 1: the ray goes on, and leaves at the far side P - V (2 r ci)
        const double ci = cosine(rng), si = std::sqrt(1.0 - ci * ci);
        const V3d V = N * ci + tp * si;
        const float Vf[3] = {(float)V.x, (float)V.y, (float)V.z};
        rule32(Pf, Nf, Vf, r, 1.0f, o, d);
        CHECK(lend(V3d{d[0] + Vf[0], d[1] + Vf[1], d[2] + Vf[2]}) <= kBoundDir);
        const V3d N64 = unit(V3d{Nf[0], Nf[1], Nf[2]}), V64 = unit(V3d{Vf[0], Vf[1], Vf[2]});
        const V3d far_side = V3d{Pf[0], Pf[1], Pf[2]} - V64 * (2.0 * r * dotd(N64, V64));
        CHECK(lend(V3d{o[0], o[1], o[2]} - far_side) <= kBoundPoint * r);
    }
}

// ---------------------------------------------------------------- 3. NaN

static void test_nan()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float good[3] = {0.0f, 1.0f, 0.0f}, bad[3] = {nan, nan, nan}, huge[3] = {inf, -inf, 3.0e38f};
    float o[3], d[3];
    const float* sets[] = {good, bad, huge};
    const float scalars[] = {1.5f, nan, inf, 0.0f, -1.0f, 3.0e38f};
    size_t calls = 0;
    for (const float* P : sets)
        for (const float* N : sets)
            for (const float* V : sets)
                for (const float r : scalars)
                    for (const float ior : scalars) {
                        rule32(P, N, V, r, ior, o, d);
                        calls++;
                    }
    CHECK(calls == 27u * 36u);
    // a NaN c2 takes ct = 0: with N = V = (0, 1, 0) and a NaN index, T = N g - V eta is all NaN, but with a NaN normal and a good
    // index the chord L = 2 r ct is 0, not NaN
    int roots = 0;
    float seen = -1.0f;
    through_sphere(
        good, bad, good, 1.0f, 1.5f,
        [&](float x) {
            roots++;
            seen = x;
            return sqrtf(x);
        },
        recip32, o, d);
    CHECK(roots == 1 && seen == 0.0f);
    CHECK(!rtxrefract::ior_ok(nan) && !rtxrefract::ior_ok(inf) && !rtxrefract::ior_ok(-inf));
}

// ---------------------------------------------------------------- 4. accepted values

static void test_values()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // values
    for (const float v : {0.0f, 1.0f, 1.5f, 4.0f, 1.0000001f}) CHECK(rtxrefract::ior_ok(v));
    for (const float v : {nan, 0.5f, 0.99999994f, 1.0e-30f, 4.0000005f, 100.0f, -1.0f, -1.5f, -1.0e-30f}) CHECK(!rtxrefract::ior_ok(v));
    // a call's values: all or nothing
    const float two[2] = {1.5f, 0.0f}, with_nan[2] = {1.5f, nan}, low[1] = {0.5f}, minus_zero[1] = {-0.0f};
    size_t bad = 99;
    CHECK(rtxrefract::values_fault(2, two, &bad) == nullptr && bad == 2);
    CHECK(rtxrefract::values_fault(0, nullptr) == nullptr);
    CHECK(rtxrefract::values_fault(2, nullptr) != nullptr);
    CHECK(rtxrefract::values_fault(2, with_nan, &bad) != nullptr && bad == 1);
    CHECK(rtxrefract::values_fault(1, low, &bad) != nullptr && bad == 0);
    CHECK(rtxrefract::values_fault(1, minus_zero) == nullptr);
}

int main()
{
    const Worst w = test_against_float64();
    test_special_cases();
    test_nan();
    test_values();
    if (g_failures != 0) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("all refract tests passed (%zu cases against float64)\n", w.n);
    return 0;
}
