// Host-only checks of the sphere bound of the mirror pass (raytracing-in-windows-console_amd/csrc/rtx_reflect.hpp) for the bundles
// that deep reflection levels make (RTX_OPT_REFLECT_DEPTH > 1), built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_host_reflect_depth.py.  A sibling of test_reflect_bound.cpp, whose first-bounce bundles start on one mirror of a
// tile; a level-2+ bundle of rtx_reflect_chain does not:
//   (a) its origins lie on several objects spread over the scene (the ball's radius rho is comparable to the scene);
//   (b) its cone is wide, up to just under the 90 degrees beyond which everything is kept;
//   (c) its rays leave a curved mirror tangentially: origins on a sphere, directions in its tangent plane or a hair either side.
// The bundle is built exactly as the kernel builds it.  In float64 no sphere that a ray of the set (or a ray drawn from the
// bundle the reductions describe) comes within its fp32 error radius of may be culled; the bound must still cull, so that the
// check is not vacuous where a bound can cull at all.
#include "../../raytracing-in-windows-console_amd/csrc/rtx_reflect.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
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

int g_fail = 0;
void check(bool ok, const char* what)
{
    if (!ok && g_fail++ < 20) std::printf("FAIL: %s\n", what);
}

struct D3 {
    double x, y, z;
};
D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
D3 mul(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double len(D3 a) { return std::sqrt(dot(a, a)); }
D3 unit(D3 a) { return mul(a, 1.0 / len(a)); }
D3 rand_unit()
{
    for (;;) {
        const D3 v = {ur(-1, 1), ur(-1, 1), ur(-1, 1)};
        const double l = len(v);
        if (l > 0.05 && l <= 1.0) return mul(v, 1.0 / l);
    }
}
// a unit vector perpendicular to a (unit)
D3 perp(D3 a)
{
    for (;;) {
        const D3 c = cross(a, rand_unit());
        if (len(c) > 0.1) return unit(c);
    }
}
// a direction at angle `ang` from the unit axis a, at a random azimuth
D3 at_angle(D3 a, double ang)
{
    const D3 p = perp(a);
    return add(mul(a, std::cos(ang)), mul(p, std::sin(ang)));
}
// a point in the ball (c, r), or on its surface
D3 in_ball(D3 c, double r, bool surface)
{
    const double rr = surface ? r : r * std::cbrt(u01());
    return add(c, mul(rand_unit(), rr));
}

struct Ray {
    float P[3], R[3];
};

D3 pd(const Ray& r) { return {(double)r.P[0], (double)r.P[1], (double)r.P[2]}; }
D3 rd(const Ray& r) { return {(double)r.R[0], (double)r.R[1], (double)r.R[2]}; }

struct Built {
    rtxreflect::Bundle b;
    float centre[3], axis[3], max_dist, max_angle;
    bool all;
};

Built build(const std::vector<Ray>& rays)
{
    Built o;
    const size_t n = rays.size();
    float sum[6] = {0, 0, 0, 0, 0, 0};
    bool degenerate = false;
    std::vector<float> U(3 * n);
    for (size_t i = 0; i < n; i++) {
        if (!rtxreflect::unit_direction(rays[i].P, rays[i].R, &U[3 * i])) degenerate = true;
        for (int k = 0; k < 3; k++) {
            sum[k] += rays[i].P[k];
            sum[3 + k] += U[3 * i + k];
        }
    }
    o.axis[0] = o.axis[1] = o.axis[2] = 0.0f;
    rtxreflect::centre_from_sum(sum[0], sum[1], sum[2], (float)n, o.centre);
    o.all = degenerate || !rtxreflect::axis_from_sum(sum[3], sum[4], sum[5], (float)n, o.axis);
    o.max_dist = o.max_angle = 0.0f;
    if (!o.all) {
        for (size_t i = 0; i < n; i++) {
            o.max_dist = std::fmax(o.max_dist, rtxreflect::distance_from_centre(o.centre, rays[i].P));
            o.max_angle = std::fmax(o.max_angle, rtxreflect::angle_from_axis(o.axis, &U[3 * i]));
        }
    }
    o.b = rtxreflect::make_bundle(o.centre, o.axis, o.max_dist, o.max_angle, o.all);
    return o;
}

// float64: does ray (P, R), s >= 0, come within the fp32 error radius of sphere (C, r)?  R^2 = r^2 (1+2u) + 15.2u |P - C|^2.
bool within(D3 P, D3 R, D3 C, double r)
{
    const double u = 1.0 / 16777216.0;
    const D3 w = sub(C, P);
    const double s = std::fmax(0.0, dot(w, R) / dot(R, R));
    const D3 e = sub(w, mul(R, s));
    const double re2 = r * r * (1.0 + 2.0 * u) + 15.2 * u * dot(w, w);
    return dot(e, e) <= re2;
}

} // namespace


std::vector<Ray> g_rays;

void push_ray(D3 P, D3 R)
{
    Ray ry;
    ry.P[0] = (float)P.x; ry.P[1] = (float)P.y; ry.P[2] = (float)P.z;
    ry.R[0] = (float)R.x; ry.R[1] = (float)R.y; ry.R[2] = (float)R.z;
    g_rays.push_back(ry);
}

int main()
{
    long cases = 0, culled = 0, narrow_cases = 0, narrow_culled = 0, built = 0, kept_all = 0;
    const int kBundles = 60000;
    for (int bi = 0; bi < kBundles; bi++) {
        const int family = bi % 3;
        const double scale = std::pow(10.0, (double)((bi / 3 % 7) - 3)); // 1e-3 .. 1e3
        const double S = 100.0 * scale;                                  // the scene's extent
        g_rays.clear();
        const int n = 2 + (int)(u01() * 60);
        const D3 a0 = rand_unit();
        // the objects the rays start on: spheres anywhere in the scene
        const int nobj = family == 0 ? 2 + (int)(u01() * 5) : 1;
        std::vector<D3> oc((size_t)nobj);
        std::vector<double> orad((size_t)nobj);
        for (int k = 0; k < nobj; k++) {
            oc[(size_t)k] = mul(D3{ur(-1, 1), ur(-1, 1), ur(-1, 1)}, S * (family == 0 ? 1.0 : 0.3));
            orad[(size_t)k] = scale * ur(0.5, 15.0);
        }
        double th0 = 0.0;
        const D3 patch = rand_unit();           // family 2: the rays start on a patch of the sphere around this normal ...
        const D3 along0 = perp(patch);          // ... and leave it along this tangent, as a tile's rays leave a curved mirror's rim
        const double patch_ang = ur(0.01, 0.3);
        for (int i = 0; i < n; i++) {
            const size_t k = (size_t)(u01() * nobj);
            const D3 nrm = family == 2 ? at_angle(patch, patch_ang * u01()) : rand_unit();
            const D3 P = add(oc[k], mul(nrm, orad[k]));
            D3 R;
            if (family == 0) {
                th0 = 0.4;
                R = at_angle(a0, ur(0.0, th0)); // origins over several objects, a moderate cone
            } else if (family == 1) {
                th0 = ur(1.2, 1.55); // near-90 degree cones
                R = at_angle(a0, u01() < 0.4 ? th0 : th0 * u01());
            } else {
                // leaving the sphere tangentially: in the tangent plane at P, tilted by up to +-1e-3 rad (outwards or inwards)
                const D3 tg = unit(sub(along0, mul(nrm, dot(along0, nrm)))); // along0 projected into the tangent plane at P
                const double tilt = (i % 3 == 0) ? 0.0 : ur(-1e-3, 1e-3);
                R = add(mul(tg, std::cos(tilt)), mul(nrm, std::sin(tilt)));
            }
            push_ray(P, mul(R, ur(0.5, 2.0)));
        }
        const Built B = build(g_rays);
        built++;
        if (B.b.all) {
            kept_all++;
            continue;
        }
        std::vector<std::pair<D3, D3>> test;
        for (const auto& ry : g_rays) test.push_back({pd(ry), rd(ry)});
        const D3 bc = {B.centre[0], B.centre[1], B.centre[2]}, ba = {B.axis[0], B.axis[1], B.axis[2]};
        for (int j = 0; j < 16; j++) test.push_back({in_ball(bc, B.max_dist, j & 1), at_angle(unit(ba), (j & 2) ? B.max_angle : B.max_angle * u01())});
        const bool narrow = B.max_angle < 0.8f;
        for (int si = 0; si < 48; si++) {
            D3 C;
            double r;
            const int kind = si % 6;
            const auto& t = test[(size_t)(u01() * (double)test.size())];
            if (kind == 0 || kind == 1) {
                // grazing a ray: at distance r (1 +- 1e-6) from a point along it, or (kind 1) just beyond its origin
                const D3 R = unit(t.second);
                const double along = kind == 0 ? S * ur(0.0, 2.0) : -scale * ur(0.0, 1.0);
                r = scale * ur(0.001, 10.0);
                C = add(add(t.first, mul(R, along)), mul(perp(R), r * (1.0 + ur(-1e-6, 1e-6))));
            } else if (kind == 2) {
                // one of the objects the rays start on, as the kernel's walk meets it (only the own object is skipped, later)
                const size_t k = (size_t)(u01() * nobj);
                C = oc[k];
                r = orad[k];
            } else if (kind == 3) {
                // touching an origin from the other side of its tangent plane
                r = scale * ur(0.001, 10.0);
                C = add(t.first, mul(rand_unit(), r * (1.0 + ur(-1e-6, 1e-6))));
            } else if (kind == 4) {
                r = scale * ur(0.001, 5.0);
                C = in_ball(bc, (double)B.max_dist + 3.0 * r, false);
            } else {
                r = scale * ur(0.001, 10.0);
                C = mul(D3{ur(-3, 3), ur(-3, 3), ur(-3, 3)}, S);
            }
            const float cf[3] = {(float)C.x, (float)C.y, (float)C.z}, rf = (float)r;
            const D3 Cq = {cf[0], cf[1], cf[2]};
            bool hit = false;
            for (const auto& tt : test) hit = hit || within(tt.first, tt.second, Cq, (double)rf);
            const bool keep = rtxreflect::may_hit(B.b, cf[0], cf[1], cf[2], rf);
            cases++;
            if (!keep) culled++;
            if (narrow) {
                narrow_cases++;
                if (!keep) narrow_culled++;
            }
            if (hit && !keep) {
                check(false, "a sphere within reach of a ray of a deep bundle was culled");
                if (g_fail <= 5) {
                    std::printf("  family %d scale %g rho %g theta %g C (%g %g %g) r %g kind %d\n", family, scale, (double)B.max_dist, (double)B.max_angle, C.x,
                                C.y, C.z, r, kind);
                }
            }
        }
    }
    std::printf("%ld bundles (%ld keep everything), %ld cases, %ld culled; narrow bundles: %ld of %ld culled\n", built, kept_all, cases, culled, narrow_culled,
                narrow_cases);
    check(cases > 1000000, "at least a million cases");
    check(kept_all < built / 2, "most deep bundles still have a bound");
    check(culled > 0, "the bound culls for deep bundles too");
    check(narrow_cases > 100000 && narrow_culled > narrow_cases / 20, "narrow bundles over spread origins cull (not vacuous)");
    if (g_fail == 0) std::printf("all deep reflect bound tests passed\n");
    return g_fail == 0 ? 0 : 1;
}
