// Host-only check of step 4 of raytracing-in-windows-console_amd/csrc/rtx_grid.hpp: the world grid's lists, built for the ray
// queries' test, also hold every sphere the SHADOW test reports (RTX_OPT_SHADOW_GRID).  Built with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_host_shadow_grid.py.
//
// Scenes of seeded random spheres at coordinate scales from 1e-12 to 1e12, centred on the origin and far from it, are listed in
// their cells exactly as rtx_grid_count / rtx_grid_scatter list them (as tests/host/test_grid_bound.cpp does).  Every segment
// (P, P + toL) runs the fp32 test of the kernels (segment_hits_sphere, rtx_tile_pass.inc: every operation rounded to fp32 on its
// own) against every sphere, and for every sphere that test reports for a walkable segment (rtxgrid::segment_walkable, the
// classification rtx_grid_shadow uses):
//   * the float64 point P + k toL, at the fp32 k the test formed, lies inside the box the sphere is listed with, the margin to spare;
//   * the sphere is in the large list, or in a cell that the walk as the kernel runs it (d = toL, tmax = 1, on while t_out <= 1)
//     visits, and whose interval [t_in, t_out] holds k;
// and the kernel's answer -- any hit among the large list and the visited cells' lists, leaving at the first -- is the brute one.
// Points: on spheres' surfaces (visible hit points), inside the box, on a floor under the cloud out to beyond `reach`, on the rim of
// the walkable region.  Lights: inside the cloud, far outside the grid box (to 1e4 box sizes), at the point itself and within ulps
// of it (degenerate segments), and -- a third of all segments -- placed so that the segment grazes a sphere within 1e-7 .. 1e-3 of
// its radius, ending before, inside and beyond it.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_grid.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

uint64_t g_state = 0x2545f4914f6cdd1dull;
double u01()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}
double ur(double a, double b) { return a + (b - a) * u01(); }
uint32_t ui(uint32_t n) { return (uint32_t)(u01() * n) % n; }

int g_fail = 0;
void check(bool ok, const char* what)
{
    if (!ok && g_fail++ < 20) std::printf("FAIL: %s\n", what);
}

struct Sph {
    float x, y, z, r;
};

// segment_hits_sphere (rtx_tile_pass.inc), operation for operation; k: the clamped parameter it formed
bool segment_hits(const float P[3], const float toL[3], float inv_len2, const Sph& sp, float& k)
{
    const float wx = sp.x - P[0], wy = sp.y - P[1], wz = sp.z - P[2];
    const float s = (wx * toL[0] + wy * toL[1] + wz * toL[2]) * inv_len2;
    k = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
    const float ex = wx - toL[0] * k, ey = wy - toL[1] * k, ez = wz - toL[2] * k;
    return ex * ex + ey * ey + ez * ez < sp.r * sp.r;
}

struct Scene {
    std::vector<Sph> sph;
    rtxgrid::Grid g;
    std::vector<std::vector<uint32_t>> cells;
    std::vector<uint32_t> large;
    std::vector<float> half;
};

bool sphere_cells(const rtxgrid::Grid& g, const Sph& s, int i0[3], int i1[3], float& h)
{
    h = rtxgrid::sphere_half(g, s.x, s.y, s.z, std::fabs(s.r));
    return rtxgrid::sphere_cells(g, s.x, s.y, s.z, s.r, i0, i1); // (the build kernels' own function)
}

void build(Scene& sc, float load)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0;
    for (const Sph& s : sc.sph) {
        const float c[3] = {s.x, s.y, s.z};
        const float r = std::fabs(s.r);
        nf++;
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(lo[k], c[k] - r);
            hi[k] = std::fmax(hi[k], c[k] + r);
        }
    }
    sc.g = rtxgrid::plan_grid(lo, hi, nf, load);
    sc.cells.assign(sc.g.ok ? (size_t)sc.g.n[0] * sc.g.n[1] * sc.g.n[2] : 0, {});
    sc.large.clear();
    sc.half.assign(sc.sph.size(), 0.0f);
    if (!sc.g.ok) return;
    for (uint32_t i = 0; i < sc.sph.size(); i++) {
        int i0[3], i1[3];
        if (!sphere_cells(sc.g, sc.sph[i], i0, i1, sc.half[i])) {
            sc.large.push_back(i);
            continue;
        }
        for (int z = i0[2]; z <= i1[2]; z++)
            for (int y = i0[1]; y <= i1[1]; y++)
                for (int x = i0[0]; x <= i1[0]; x++) sc.cells[((size_t)z * sc.g.n[1] + y) * sc.g.n[0] + x].push_back(i);
    }
}

uint64_t g_cases = 0, g_walked = 0, g_unwalkable = 0, g_hits = 0, g_dark = 0, g_steps = 0, g_grazing = 0, g_light_inside = 0, g_light_far = 0;

void one_segment(const Scene& sc, const float P[3], const float L[3])
{
    g_cases++;
    const rtxgrid::Grid& g = sc.g;
    const float toL[3] = {L[0] - P[0], L[1] - P[1], L[2] - P[2]}; // (sub(L, P), as the kernels form it)
    if (!rtxgrid::segment_walkable(g, P, toL)) {
        g_unwalkable++;
        return;
    }
    g_walked++;
    const float len2 = toL[0] * toL[0] + toL[1] * toL[1] + toL[2] * toL[2];
    const float inv_len2 = len2 > 0.0f ? 1.0f / len2 : 0.0f;
    bool inside = true, far = false;
    for (int k = 0; k < 3; k++) {
        inside = inside && L[k] >= g.lo[k] && L[k] <= rtxgrid::edge(g, k, (int)g.n[k]);
        far = far || std::fabs(L[k] - g.ctr[k]) > 4.0f * g.reach;
    }
    g_light_inside += inside ? 1 : 0;
    g_light_far += far ? 1 : 0;

    // brute: every sphere
    std::vector<float> ks(sc.sph.size(), -1.0f);
    bool brute_dark = false;
    for (uint32_t i = 0; i < sc.sph.size(); i++) {
        float k;
        if (segment_hits(P, toL, inv_len2, sc.sph[i], k)) {
            ks[i] = k;
            brute_dark = true;
        }
    }
    // the walk as rtx_grid_shadow runs it
    std::vector<uint8_t> seen(sc.sph.size(), 0);
    bool grid_dark = false;
    for (uint32_t i : sc.large) {
        seen[i] = 1;
        grid_dark = grid_dark || ks[i] >= 0.0f;
    }
    rtxgrid::Walk w;
    bool go = rtxgrid::walk_start(g, P, toL, 1.0f, w);
    uint32_t steps = 0;
    while (go) {
        const float tin = w.t_in, tout = rtxgrid::t_out(w);
        check(tin <= tout, "a cell's interval is reversed");
        for (uint32_t i : sc.cells[rtxgrid::cell_index(g, w)]) {
            if (ks[i] >= 0.0f) grid_dark = true;
            if (ks[i] >= tin && ks[i] <= tout) seen[i] = 1;
        }
        // (the kernel leaves at the first hit; the check goes on, to see every reported sphere's cell)
        go = tout <= 1.0f && rtxgrid::walk_step(g, w);
        if (++steps > 4000u) {
            check(false, "the walk does not end");
            break;
        }
    }
    g_steps += steps;
    check(grid_dark == brute_dark, "the grid's answer differs from the brute one");
    g_dark += brute_dark ? 1 : 0;
    for (uint32_t i = 0; i < sc.sph.size(); i++) {
        if (!(ks[i] >= 0.0f)) continue;
        g_hits++;
        check(seen[i] != 0, "a sphere the shadow test reports is in no visited cell whose interval holds its k");
        if (sc.half[i] > 0.0f) {
            const double k = (double)ks[i];
            const double c[3] = {sc.sph[i].x, sc.sph[i].y, sc.sph[i].z};
            for (int q = 0; q < 3; q++) {
                const double x = (double)P[q] + k * (double)toL[q];
                check(std::fabs(x - c[q]) <= (double)sc.half[i] - (double)g.margin, "a reported closest point lies outside the listed box less its margin");
            }
        }
    }
}

void rand_dir(double d[3])
{
    for (;;) {
        const double v[3] = {ur(-1, 1), ur(-1, 1), ur(-1, 1)};
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (l > 0.05 && l <= 1.0) {
            for (int k = 0; k < 3; k++) d[k] = v[k] / l;
            return;
        }
    }
}

void segments_for(const Scene& sc, int n)
{
    const rtxgrid::Grid& g = sc.g;
    if (!g.ok) return;
    double ext[3], ctr[3];
    for (int k = 0; k < 3; k++) {
        ext[k] = (double)rtxgrid::edge(g, k, (int)g.n[k]) - (double)g.lo[k];
        ctr[k] = g.ctr[k];
    }
    const double size = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
    for (int it = 0; it < n; it++) {
        float P[3], L[3];
        const Sph& own = sc.sph[ui((uint32_t)sc.sph.size())];
        // the point
        const int pk = (int)ui(8);
        double d[3];
        rand_dir(d);
        if (pk < 4) { // a visible hit point: on a sphere's surface
            P[0] = (float)(own.x + d[0] * std::fabs(own.r));
            P[1] = (float)(own.y + d[1] * std::fabs(own.r));
            P[2] = (float)(own.z + d[2] * std::fabs(own.r));
        } else if (pk < 6) { // anywhere in the box
            for (int k = 0; k < 3; k++) P[k] = (float)(ctr[k] + ur(-0.5, 0.5) * ext[k]);
        } else if (pk == 6) { // on a floor under the cloud, out to beyond reach
            P[0] = (float)(ctr[0] + ur(-1.2, 1.2) * g.reach);
            P[1] = (float)(g.lo[1] - ur(0, 0.2) * ext[1]);
            P[2] = (float)(ctr[2] + ur(-1.2, 1.2) * g.reach);
        } else { // the rim of the walkable region
            for (int k = 0; k < 3; k++) P[k] = (float)(ctr[k] + ur(-0.5, 0.5) * ext[k]);
            const int ax = (int)ui(3);
            P[ax] = g.ctr[ax] + (u01() < 0.5 ? 1.0f : -1.0f) * g.reach * (float)ur(0.98, 1.0);
        }
        // the light
        const int lk = (int)ui(9);
        if (lk < 3) { // grazing: the segment passes a sphere r (1 +- eps) off its centre and ends before, inside or beyond it
            g_grazing++;
            const Sph& s = sc.sph[ui((uint32_t)sc.sph.size())];
            const double v[3] = {s.x - (double)P[0], s.y - (double)P[1], s.z - (double)P[2]};
            const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], pv = d[0] * v[0] + d[1] * v[1] + d[2] * v[2];
            double q[3], ql = 0;
            for (int k = 0; k < 3; k++) {
                q[k] = d[k] - (vv > 0 ? pv / vv * v[k] : 0.0);
                ql += q[k] * q[k];
            }
            ql = std::sqrt(ql);
            const double off = std::fabs(s.r) * (1.0 + ur(-1, 1) * std::pow(10.0, ur(-7, -3)));
            const double f = u01() < 0.3 ? ur(0.9, 1.1) : (u01() < 0.5 ? ur(0.3, 1.0) : std::pow(10.0, ur(0, 4)));
            for (int k = 0; k < 3; k++) L[k] = (float)((double)P[k] + (v[k] + (ql > 0 ? q[k] / ql * off : 0.0)) * f);
        } else if (lk < 5) { // inside the cloud
            for (int k = 0; k < 3; k++) L[k] = (float)(ctr[k] + ur(-0.5, 0.5) * ext[k]);
        } else if (lk < 7) { // far outside the grid box
            double e[3];
            rand_dir(e);
            const double far = size * std::pow(10.0, ur(0.5, 4));
            for (int k = 0; k < 3; k++) L[k] = (float)(ctr[k] + e[k] * far);
        } else if (lk == 7) { // at the point, or within ulps of it
            for (int k = 0; k < 3; k++) L[k] = P[k];
            if (u01() < 0.7) {
                const int ax = (int)ui(3);
                for (int j = (int)ui(40); j >= 0; j--) L[ax] = std::nextafterf(L[ax], u01() < 0.5 ? INFINITY : -INFINITY);
            }
        } else { // through another sphere's centre, ending around it
            const Sph& s = sc.sph[ui((uint32_t)sc.sph.size())];
            const double f = ur(0.5, 2.0);
            L[0] = (float)((double)P[0] + (s.x - (double)P[0]) * f);
            L[1] = (float)((double)P[1] + (s.y - (double)P[1]) * f);
            L[2] = (float)((double)P[2] + (s.z - (double)P[2]) * f);
        }
        one_segment(sc, P, L);
    }
}

void random_scenes()
{
    for (int sci = 0; sci < 900; sci++) {
        Scene sc;
        const double scale = sci % 5 == 4 ? std::pow(10.0, ur(-12, 12)) : std::pow(10.0, ur(-2, 3));
        const double offs = sci % 7 == 6 ? scale * std::pow(10.0, ur(0, 3)) : (sci % 3 == 0 ? scale * ur(0, 2) : 0.0);
        const uint32_t n = 1u + ui(sci % 11 == 0 ? 600u : 96u);
        const double ex[3] = {scale * ur(0.05, 1), scale * ur(0.05, 1) * (sci % 13 == 5 ? 0.0 : 1.0), scale * ur(0.05, 1)};
        const double rmax = scale * std::pow(10.0, ur(-3.5, -0.5));
        for (uint32_t i = 0; i < n; i++) {
            Sph s;
            s.x = (float)(offs + ur(-1, 1) * ex[0]);
            s.y = (float)(offs * 0.5 + ur(-1, 1) * ex[1]);
            s.z = (float)(ur(-1, 1) * ex[2] - offs);
            s.r = (float)(rmax * ur(0.01, 1));
            if (u01() < 0.01) s.r = (float)(scale * ur(0.5, 3)); // one the size of the scene: the large list
            if (u01() < 0.01) s.r = 0.0f;
            if (u01() < 0.02 && i > 0) s = sc.sph[ui(i)];         // a duplicate
            sc.sph.push_back(s);
        }
        build(sc, sci % 4 == 0 ? 0.5f : (sci % 4 == 1 ? 8.0f : rtxgrid::kDefaultLoad));
        check(sc.g.ok != 0, "a plain scene got no grid");
        segments_for(sc, 2000);
    }
}

void classification_cases()
{
    const float lo[3] = {-100, -60, 30}, hi[3] = {100, 60, 200};
    const rtxgrid::Grid g = rtxgrid::plan_grid(lo, hi, 4096, 1.0f);
    const float P[3] = {0, 0, 100}, Pfar[3] = {0, 0, 1000}, Pnan[3] = {NAN, 0, 100};
    const float d1[3] = {0, 50, 0}, d0[3] = {0, 0, 0}, dtiny[3] = {1e-7f, 0, 0}, dhuge[3] = {0, 2e6f, 0}, dinf[3] = {INFINITY, 0, 0}, dnan[3] = {0, NAN, 0};
    check(rtxgrid::segment_walkable(g, P, d1), "a plain segment is walkable");
    check(!rtxgrid::segment_walkable(g, P, d0), "the light at the point: not walkable");
    check(!rtxgrid::segment_walkable(g, P, dtiny), "a segment shorter than 2^-20: not walkable");
    check(!rtxgrid::segment_walkable(g, P, dhuge), "a segment longer than 2^20: not walkable");
    check(!rtxgrid::segment_walkable(g, P, dinf) && !rtxgrid::segment_walkable(g, P, dnan), "a light that is not finite: not walkable");
    check(!rtxgrid::segment_walkable(g, Pfar, d1), "a point beyond reach: not walkable");
    check(!rtxgrid::segment_walkable(g, Pnan, d1), "a point that is not finite: not walkable");
    rtxgrid::Grid none = g;
    none.ok = 0;
    check(!rtxgrid::segment_walkable(none, P, d1), "no grid: not walkable");
}

} // namespace

int main()
{
    classification_cases();
    random_scenes();
    std::printf("segments %llu walked %llu not walkable %llu grazing %llu light inside the box %llu light far outside %llu reported spheres %llu dark %llu "
                "cells stepped %llu\n",
                (unsigned long long)g_cases, (unsigned long long)g_walked, (unsigned long long)g_unwalkable, (unsigned long long)g_grazing,
                (unsigned long long)g_light_inside, (unsigned long long)g_light_far, (unsigned long long)g_hits, (unsigned long long)g_dark,
                (unsigned long long)g_steps);
    check(g_walked >= 1000000ull, "fewer than a million walked segments");
    check(g_grazing >= 300000ull, "too few grazing segments");
    check(g_light_inside >= 100000ull && g_light_far >= 100000ull, "too few lights inside the box or far outside it");
    check(g_hits >= 200000ull && g_unwalkable >= 10000ull, "too few reported spheres or unwalkable segments for the check to mean anything");
    if (g_fail) {
        std::printf("%d failure(s)\n", g_fail);
        return 1;
    }
    std::printf("all shadow grid bound tests passed\n");
    return 0;
}
