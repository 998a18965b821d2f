// Host-only checks of the world grid of the ray queries (raytracing-in-windows-console_amd/csrc/rtx_grid.hpp): the planner's
// degenerate cases, and the conservativeness of lists and walk against float64, built with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_host_query.py.
//
// Scenes of seeded random spheres at coordinate scales from 1e-12 to 1e12, centred on the origin and far from it, are listed in
// their cells exactly as rtx_grid_count / rtx_grid_scatter list them.  Every ray runs the fp32 hit test of the kernels
// (Sphere.cu:30-68 on otc = o - c) against every sphere, and for every sphere that test reports hit at t:
//   * the float64 point o + t d lies inside the box the sphere is listed with, with the margin to spare (step 1 of the header);
//   * the sphere is in the large list or in a cell of the walk whose interval [t_in, t_out] holds t (steps 2 and 3);
// and the walk with its stopping rule returns the brute minimum of (t, index), bit for bit.  Rays: random, grazing a sphere within
// 1e-3 of its radius, axis-parallel with zero components, lying in cell faces, through cell corners, from inside and from the
// surface of spheres, from the rim of the walkable region pointing in and away, with unnormalised and nearly degenerate directions.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_grid.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
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

// secondary_sphere_hit (rtx_reflect_kernels.inc) with sqrt_cr = sqrtf and rcp_cr = 1 / x: every operation rounded to fp32 on its own
bool sphere_hit(const float o[3], const float d[3], float a, const Sph& g, float& t)
{
    const float ox = o[0] - g.x, oy = o[1] - g.y, oz = o[2] - g.z;
    const float oo = ox * ox + oy * oy + oz * oz;
    const float cc = oo - (g.r * g.r);
    const float s = d[0] * ox + d[1] * oy + d[2] * oz;
    const float q = s * s - a * cc;
    if (q < -1.0e-30f) return false;
    const float b = 2.0f * s;
    const float fourA = 4.0f * a;
    const float disc = b * b - fourA * cc;
    if (disc < 0.0f) return false;
    const float sq = std::sqrt(disc);
    const float divTwoA = 1.0f / (2.0f * a);
    const float t2 = (-b - sq) * divTwoA;
    if (t2 < 0.0f) return false;
    t = t2;
    return t2 == t2;
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
        if (!rtxgrid::finite_f(s.x) || !rtxgrid::finite_f(s.y) || !rtxgrid::finite_f(s.z) || !rtxgrid::finite_f(r)) continue;
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

uint64_t g_cases = 0, g_hits = 0, g_walked = 0, g_steps = 0, g_unwalkable = 0;

void take(float t, uint32_t i, float tmax, float& bt, uint32_t& bi)
{
    if (t <= tmax && (t < bt || (t == bt && i < bi))) {
        bt = t;
        bi = i;
    }
}

void one_ray(const Scene& sc, const float o[3], const float d[3], float tmax)
{
    g_cases++;
    const rtxgrid::Grid& g = sc.g;
    const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!rtxgrid::walkable(g, o, a)) {
        g_unwalkable++;
        return;
    }
    g_walked++;
    // brute
    float bt = 99999999.f;
    uint32_t bi = 0xffffffffu;
    std::vector<float> ts(sc.sph.size(), -1.0f);
    for (uint32_t i = 0; i < sc.sph.size(); i++) {
        float t;
        if (sphere_hit(o, d, a, sc.sph[i], t)) {
            ts[i] = t;
            take(t, i, tmax, bt, bi);
        }
    }
    // the walk with its stopping rule, as rtx_query_grid runs it
    float gt = 99999999.f;
    uint32_t gi = 0xffffffffu;
    if (tmax >= 0.0f) {
        for (uint32_t i : sc.large)
            if (ts[i] >= 0.0f) take(ts[i], i, tmax, gt, gi);
        rtxgrid::Walk w;
        bool go = rtxgrid::walk_start(g, o, d, tmax, w);
        while (go) {
            for (uint32_t i : sc.cells[rtxgrid::cell_index(g, w)])
                if (ts[i] >= 0.0f) take(ts[i], i, tmax, gt, gi);
            const float tout = rtxgrid::t_out(w);
            go = !(gt < tout) && tout <= tmax && rtxgrid::walk_step(g, w);
        }
    } else {
        bt = 99999999.f;
        bi = 0xffffffffu;
    }
    uint32_t b0, b1;
    std::memcpy(&b0, &bt, 4);
    std::memcpy(&b1, &gt, 4);
    check(b0 == b1 && bi == gi, "the walk's closest hit differs from the brute one");
    // every reported hit: where it lies, and that the full walk meets a cell that lists it while t is in the cell's interval
    std::vector<uint8_t> seen(sc.sph.size(), 0);
    for (uint32_t i : sc.large) seen[i] = 1;
    rtxgrid::Walk w;
    bool go = rtxgrid::walk_start(g, o, d, INFINITY, w);
    uint32_t steps = 0;
    while (go) {
        const float tin = w.t_in, tout = rtxgrid::t_out(w);
        check(tin <= tout, "a cell's interval is reversed");
        for (uint32_t i : sc.cells[rtxgrid::cell_index(g, w)])
            if (ts[i] >= tin && ts[i] <= tout) seen[i] = 1;
        go = rtxgrid::walk_step(g, w);
        if (++steps > 4000u) {
            check(false, "the walk does not end");
            break;
        }
    }
    g_steps += steps;
    for (uint32_t i = 0; i < sc.sph.size(); i++) {
        if (!(ts[i] >= 0.0f)) continue;
        g_hits++;
        check(seen[i] != 0, "a sphere reported hit is in no visited cell whose interval holds its t");
        if (sc.half[i] > 0.0f) {
            const double t = (double)ts[i];
            const double c[3] = {sc.sph[i].x, sc.sph[i].y, sc.sph[i].z};
            for (int k = 0; k < 3; k++) {
                const double p = (double)o[k] + t * (double)d[k];
                check(std::fabs(p - c[k]) <= (double)sc.half[i] - (double)g.margin, "a reported hit point lies outside the listed box less its margin");
            }
        }
    }
}

void rand_dir(float d[3], double len)
{
    for (;;) {
        const double v[3] = {ur(-1, 1), ur(-1, 1), ur(-1, 1)};
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (l > 0.05 && l <= 1.0) {
            for (int k = 0; k < 3; k++) d[k] = (float)(v[k] / l * len);
            return;
        }
    }
}

void rays_for(const Scene& sc, int n_rays)
{
    const rtxgrid::Grid& g = sc.g;
    if (!g.ok) return;
    float ext[3], ctr[3];
    for (int k = 0; k < 3; k++) {
        ext[k] = rtxgrid::edge(g, k, (int)g.n[k]) - g.lo[k];
        ctr[k] = g.ctr[k];
    }
    for (int it = 0; it < n_rays; it++) {
        float o[3], d[3];
        const double len = std::pow(10.0, ur(-5, 5)) * (u01() < 0.5 ? 1.0 : 0.0) + (u01() < 0.5 ? 1.0 : 0.0);
        const int kind = (int)ui(9);
        const Sph& s = sc.sph[ui((uint32_t)sc.sph.size())];
        for (int k = 0; k < 3; k++) o[k] = (float)(ctr[k] + ur(-1, 1) * ext[k]); // twice the box
        rand_dir(d, len > 0 ? len : 1.0);
        float tmax = u01() < 0.7 ? INFINITY : (float)(ur(0, 3) * g.reach / (len > 0 ? len : 1.0));
        if (kind == 1) { // grazing: aim at a point r (1 +- eps) off the centre, perpendicular to the line of sight
            float p[3];
            rand_dir(p, 1.0);
            const double v[3] = {s.x - (double)o[0], s.y - (double)o[1], s.z - (double)o[2]};
            const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], pv = p[0] * v[0] + p[1] * v[1] + p[2] * v[2];
            double q[3], ql = 0;
            for (int k = 0; k < 3; k++) {
                q[k] = p[k] - (vv > 0 ? pv / vv * v[k] : 0.0);
                ql += q[k] * q[k];
            }
            ql = std::sqrt(ql);
            const double off = std::fabs(s.r) * (1.0 + ur(-1, 1) * std::pow(10.0, ur(-7, -3)));
            for (int k = 0; k < 3; k++) d[k] = (float)((v[k] + (ql > 0 ? q[k] / ql * off : 0.0)) * ur(0.3, 3.0));
        } else if (kind == 2) { // axis-parallel, zero components
            const int ax = (int)ui(3);
            for (int k = 0; k < 3; k++) d[k] = k == ax ? (float)(u01() < 0.5 ? len : -len) : (u01() < 0.5 ? 0.0f : -0.0f);
            if (d[ax] == 0.0f) d[ax] = 1.0f;
            if (u01() < 0.5) o[(ax + 1) % 3] = rtxgrid::edge(g, (ax + 1) % 3, (int)ui(g.n[(ax + 1) % 3] + 1)); // in a cell face
        } else if (kind == 3) { // in a cell face, any direction inside it
            const int ax = (int)ui(3);
            o[ax] = rtxgrid::edge(g, ax, (int)ui(g.n[ax] + 1));
            d[ax] = 0.0f;
            if (d[(ax + 1) % 3] == 0.0f && d[(ax + 2) % 3] == 0.0f) d[(ax + 1) % 3] = 1.0f;
        } else if (kind == 4) { // through a cell corner (or from one)
            float c[3];
            for (int k = 0; k < 3; k++) c[k] = rtxgrid::edge(g, k, (int)ui(g.n[k] + 1));
            if (u01() < 0.3) {
                for (int k = 0; k < 3; k++) o[k] = c[k];
            } else {
                for (int k = 0; k < 3; k++) d[k] = c[k] - o[k];
                if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
            }
        } else if (kind == 5) { // from inside a sphere or from its surface (a secondary ray)
            float p[3];
            rand_dir(p, 1.0);
            const double rr = std::fabs(s.r) * (u01() < 0.5 ? 1.0 : ur(0, 1));
            o[0] = (float)(s.x + p[0] * rr);
            o[1] = (float)(s.y + p[1] * rr);
            o[2] = (float)(s.z + p[2] * rr);
        } else if (kind == 6) { // the rim of the walkable region, pointing in or away
            const int ax = (int)ui(3);
            o[ax] = ctr[ax] + (u01() < 0.5 ? 1.0f : -1.0f) * g.reach * (float)ur(0.98, 1.0);
            if (u01() < 0.5)
                for (int k = 0; k < 3; k++) d[k] = (float)((s.x * (k == 0) + s.y * (k == 1) + s.z * (k == 2)) - o[k]);
            if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
        } else if (kind == 7) { // nearly degenerate direction: one or two components far below the largest
            for (int k = 0; k < 3; k++)
                if (u01() < 0.5) d[k] *= (float)std::pow(10.0, ur(-14, -6));
            if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
        } else if (kind == 8) { // aimed at a sphere's centre from anywhere, tmax around the hit
            for (int k = 0; k < 3; k++) d[k] = (float)((s.x * (k == 0) + s.y * (k == 1) + s.z * (k == 2)) - o[k]);
            if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
            tmax = u01() < 0.5 ? 1.0f : (float)ur(0.0, 1.2);
        }
        one_ray(sc, o, d, tmax);
    }
}

void random_scenes()
{
    for (int sci = 0; sci < 1100; sci++) {
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
            if (u01() < 0.01) s.r = (float)(scale * ur(0.5, 3)); // one the size of the scene
            if (u01() < 0.01) s.r = 0.0f;
            if (u01() < 0.02 && i > 0) s = sc.sph[ui(i)];         // a duplicate
            sc.sph.push_back(s);
        }
        build(sc, sci % 4 == 0 ? 0.5f : (sci % 4 == 1 ? 8.0f : rtxgrid::kDefaultLoad));
        check(sc.g.ok != 0, "a plain scene got no grid");
        rays_for(sc, 2000);
    }
}

void planner_cases()
{
    using rtxgrid::Grid;
    using rtxgrid::plan_grid;
    const float z3[3] = {0, 0, 0};
    // no spheres / no finite sphere
    check(plan_grid(z3, z3, 0, 2.0f).ok == 0, "no spheres: no grid");
    const float inf_lo[3] = {INFINITY, INFINITY, INFINITY}, inf_hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    check(plan_grid(inf_lo, inf_hi, 0, 2.0f).ok == 0, "no finite sphere: no grid");
    // one sphere
    const float lo1[3] = {-1, -1, 9}, hi1[3] = {1, 1, 11};
    Grid g = plan_grid(lo1, hi1, 1, 2.0f);
    check(g.ok && g.n[0] == 1 && g.n[1] == 1 && g.n[2] == 1, "one sphere: one cell");
    check(g.lo[2] < 9 && rtxgrid::edge(g, 2, 1) > 11 && g.reach == 3.0f && g.margin > 0, "one sphere: the box holds it");
    // a point (extent 0 on every axis), at the origin and away from it
    g = plan_grid(z3, z3, 1, 2.0f);
    check(g.ok && g.n[0] * g.n[1] * g.n[2] == 1 && g.cs[0] > 0, "a point at the origin gets a cell");
    const float p5[3] = {5, 5, 5};
    g = plan_grid(p5, p5, 3, 2.0f);
    check(g.ok && g.lo[0] < 5 && rtxgrid::edge(g, 0, (int)g.n[0]) > 5, "a point away from the origin gets a cell around it");
    // coplanar centres: extent 0 on one axis
    const float lof[3] = {-50, 3, 40}, hif[3] = {50, 3, 200};
    g = plan_grid(lof, hif, 4096, 1.0f);
    check(g.ok && g.n[1] == 1 && g.n[0] > 20 && g.n[2] > 20, "a flat box: one layer of cells, resolution in the plane");
    check((uint64_t)g.n[0] * g.n[1] * g.n[2] <= 2u * 4096u, "a flat box: about a cell per sphere");
    // the synthetic scenes' shape, a cell per sphere: resolution follows the extents
    const float los[3] = {-100, -60, 30}, his[3] = {100, 60, 200};
    g = plan_grid(los, his, 65536, 1.0f);
    check(g.ok && g.n[0] > g.n[1] && g.n[0] >= 40 && g.n[0] <= 70, "65 536 spheres: tens of cells per axis");
    uint64_t tot = (uint64_t)g.n[0] * g.n[1] * g.n[2];
    check(tot > 40000 && tot < 100000, "65 536 spheres: about a cell per sphere");
    for (int k = 0; k < 3; k++) check(rtxgrid::edge(g, k, (int)g.n[k]) >= his[k] && g.lo[k] <= los[k], "the grid box holds the spheres' box");
    // the cap on cells
    g = plan_grid(los, his, 0xffffffffu, 1.0e-3f);
    tot = (uint64_t)g.n[0] * g.n[1] * g.n[2];
    check(g.ok && tot <= rtxgrid::kMaxCells && g.n[0] <= rtxgrid::kMaxAxis, "the cap on cells holds");
    const float lon[3] = {-1e6f, -1, -1}, hin[3] = {1e6f, 1, 1};
    g = plan_grid(lon, hin, 1000000, 1.0f);
    check(g.ok && g.n[0] <= rtxgrid::kMaxAxis && (uint64_t)g.n[0] * g.n[1] * g.n[2] <= rtxgrid::kMaxCells, "a needle: the cap per axis holds");
    // huge and tiny coordinates: scaled scenes
    const float lob[3] = {-1e20f, -1e20f, 3e19f}, hib[3] = {1e20f, 1e20f, 2e20f};
    check(plan_grid(lob, hib, 1024, 2.0f).ok == 0, "coordinates beyond 2^50: no grid (queries test every sphere)");
    const float lot[3] = {-1e-16f, -1e-16f, 3e-17f}, hit[3] = {1e-16f, 1e-16f, 2e-16f};
    check(plan_grid(lot, hit, 1024, 2.0f).ok == 0, "coordinates below 2^-50: no grid");
    const float lom[3] = {-1e12f, -1e12f, 3e11f}, him[3] = {1e12f, 1e12f, 2e12f};
    g = plan_grid(lom, him, 1024, 2.0f);
    check(g.ok && g.margin > 0 && rtxgrid::finite_f(g.reach), "a scene scaled by 1e10 has a grid");
    // NaN and reversed boxes, odd loads
    const float nanv[3] = {NAN, 0, 0};
    check(plan_grid(nanv, hi1, 5, 2.0f).ok == 0, "a NaN box: no grid");
    check(plan_grid(hi1, lo1, 5, 2.0f).ok == 0, "a reversed box: no grid");
    check(plan_grid(los, his, 1024, 0.0f).ok == 1 && plan_grid(los, his, 1024, NAN).ok == 1 && plan_grid(los, his, 1024, -3.0f).ok == 1,
          "a load that is not positive falls back to the default");
    // a tiny scene far from the origin: the margin follows the coordinate scale and may swallow the cells, the grid stays valid
    const float lof2[3] = {1e6f, 1e6f, 1e6f}, hif2[3] = {1e6f + 1, 1e6f + 1, 1e6f + 1};
    g = plan_grid(lof2, hif2, 100, 1.0f);
    check(g.ok && g.margin >= 15.0f && rtxgrid::edge(g, 0, (int)g.n[0]) > 1e6f + 1, "a small scene far away: margin from the coordinate scale");
    // edges are monotonic and cell_range brackets its interval
    g = plan_grid(los, his, 4096, 1.0f);
    for (int k = 0; k < 3; k++) {
        for (int i = 0; i < (int)g.n[k]; i++) check(rtxgrid::edge(g, k, i) <= rtxgrid::edge(g, k, i + 1), "edges are monotonic");
        for (int it = 0; it < 2000; it++) {
            float a = (float)ur(los[k] - 50, his[k] + 50), b = (float)ur(los[k] - 50, his[k] + 50);
            if (b < a) std::swap(a, b);
            int i0, i1;
            rtxgrid::cell_range(g, k, a, b, i0, i1);
            check(i0 >= 0 && i1 < (int)g.n[k] && i0 <= i1, "cell_range stays in the grid");
            check(i0 == 0 || rtxgrid::edge(g, k, i0) <= a, "cell_range: the first cell reaches a");
            check(i1 == (int)g.n[k] - 1 || rtxgrid::edge(g, k, i1 + 1) >= b, "cell_range: the last cell reaches b");
        }
    }
    // not walkable: non-finite, zero, out of range a, far origins
    const float o0[3] = {0, 0, 100}, on[3] = {NAN, 0, 100}, oi[3] = {INFINITY, 0, 100}, ofar[3] = {0, 0, 1000};
    check(rtxgrid::walkable(g, o0, 1.0f), "a plain ray is walkable");
    check(!rtxgrid::walkable(g, o0, 0.0f), "zero direction: not walkable");
    check(!rtxgrid::walkable(g, on, 1.0f) && !rtxgrid::walkable(g, oi, 1.0f), "origin not finite: not walkable");
    check(!rtxgrid::walkable(g, o0, NAN) && !rtxgrid::walkable(g, o0, INFINITY), "direction not finite: not walkable");
    check(!rtxgrid::walkable(g, o0, 9e12f) && !rtxgrid::walkable(g, o0, 1e-14f), "a out of range: not walkable");
    check(!rtxgrid::walkable(g, ofar, 1.0f), "an origin beyond reach: not walkable");
}

} // namespace

int main()
{
    planner_cases();
    random_scenes();
    std::printf("cases %llu walked %llu not walkable %llu reported hits %llu cells stepped %llu\n", (unsigned long long)g_cases, (unsigned long long)g_walked,
                (unsigned long long)g_unwalkable, (unsigned long long)g_hits, (unsigned long long)g_steps);
    check(g_walked >= 2000000ull, "fewer than 2 M walked cases");
    check(g_hits >= 200000ull, "too few reported hits for the check to mean anything");
    if (g_fail) {
        std::printf("%d failure(s)\n", g_fail);
        return 1;
    }
    std::printf("all grid bound tests passed\n");
    return 0;
}
