// rtx_grid.hpp -- the world-space grid of the ray queries (rtx_query_rays, rtx_pick): its planner (pure host code), the
// conservative sphere bound it is built with and the cell walk of a ray, for host and device alike.
//
// A uniform grid of n[0] x n[1] x n[2] cells over the spheres' bounding box; cell boundary i of axis k is the fp32 value
// edge(k, i) = lo[k] + (float)i * cs[k], non-decreasing in i because fp32 multiplication and addition are monotonic.  Build and
// walk use this one function, so a boundary is the same number for both.
//
// What must hold (exactness): a sphere whose fp32 test (secondary_sphere_hit) reports a hit at t for a walkable ray (o, d) is
// listed in a cell the walk visits before it stops.  Three steps.
//
// 1. Where the reported hit lies.  The test accepts when its rounded discriminant is not negative and reports the near root.
//    By DESIGN §4.1 (R^2 = r^2 (1+2u) + 15.2u |o - c|^2, u = 2^-24) the exact point P = o + t d then lies within
//    R = sqrt(r^2 (1 + kappa) + kappa D^2) of the centre c, kappa = 2e-6 > 2.2 x 15.2u, D >= |o - c| (the slack of kappa also
//    covers the few ulps of D by which the rounding of t moves P along the ray).  Walkable origins lie within `reach` of the
//    box centre on every axis, so D_i = |(reach + |c_k - ctr_k|)_k| bounds |o - c_i| for all of them: sphere_half().
// 2. Where a sphere is listed.  In every cell that meets the box c +- (R + margin), widened by a relative 1e-4 (cell_range();
//    the comparison is against the edge() values themselves, so only the rounding of c +- half-width enters: half an ulp of the
//    coordinate, far below margin = 2^-16 of the coordinate scale).  Spheres whose box covers more than kLargeCells cells, or is
//    not finite, are kept in a list every ray tests.
// 3. Where the walk is.  T(X) = fl(fl(X - o_k) * fl(1 / d_k)) is the parameter at which the walk crosses boundary X of axis k;
//    three roundings, so |T(X) - (X - o_k) / d_k| <= 3.01u |X - o_k| / |d_k| and the exact ray is within e = 3.01u |X - o_k| <=
//    3.01u (reach + half the box) of X at parameter T(X).  T is monotonic in X.  The walk keeps, per axis, t_near <= t_in and
//    t_out <= t_far for the T of its cell's two boundaries (walk_start() establishes it by comparing T values, never positions;
//    a step moves the axis with the smallest t_far and recomputes that T from the integer index, nothing accumulates), so for
//    every real t in [t_in, t_out] the exact point is within e of the cell on every axis.  Axes along which the direction is
//    below 2^-30 of its largest component are not walked: the coordinate moves by less than 2^-29 of the box inside the grid.
//    Both are far below margin >= 2^-16 x 4 x (half the box), so the point of step 1, at its t, is within margin of the cell
//    whose interval holds t, the sphere is listed there (step 2), and the intervals tile [t_start, leaving the grid].  t before
//    the walk's start or past its end would put P outside the grid box, which holds every listed box with margin to spare.
//    Hence the walk may stop as soon as the best t so far is below t_out of the cell just tested: no margin in t is needed,
//    because t_out and the reported t are compared as the fp32 numbers they are.
//
// 4. The shadow test (RTX_OPT_SHADOW_GRID).  Shadow segments are tested by another fp32 test, segment_hits_sphere
//    (rtx_tile_pass.inc): for the segment P + k toL, k in [0, 1], w = fl(c - P), k = the clamped fl(fl(w . toL) * inv_len2),
//    e = fl(w - fl(toL k)), hit iff fl(e . e) < fl(r r).  Claim: when it reports a hit for a walkable segment (P within `reach` of
//    the box centre on every axis, a = fl(toL . toL) in [2^-40, 2^40], everything finite), the exact point X = P + k toL, at the
//    fp32 value k the test formed and with the fp32 vectors P and toL taken as exact, lies within step 1's R of c.  Nothing is
//    assumed about how k was arrived at, only that it is an fp32 number in [0, 1] (a NaN k reports no hit).
//    Write w* = c - P and e* = w* - k toL = c - X for the exact vectors.  Per component e_i = ((w*_i (1 + d1)) - (toL_i k)(1 + d2))
//    (1 + d3) with |d| <= u, so |e - e*| <= u |w*| + u k |toL| + 1.01u |e| in norm.  A reported hit has fl(e . e) < fl(r r):
//    three non-negative products and two additions give fl(e . e) >= |e|^2 (1 - u)^3, and fl(r r) <= r^2 (1 + u), hence
//    |e| < r (1 + 3.01u).  From e* = w* - k toL, k |toL| <= |w*| + |e*|.  With E = |e*| and D >= |w*|:
//    E <= |e| (1 + 1.01u) + u (2 D + E), so E <= r (1 + 5.2u) + 2.01u D -- the point lies within r (1 + 5.2u) + eps D of the centre
//    with eps = 2.01u = 1.2e-7.  Squared, with 2 r eps D <= eps (r^2 + D^2): E^2 <= r^2 (1 + 10.5u + 1.3e-7) + 1.3e-7 D^2 <=
//    r^2 (1 + kappa) + kappa D^2 for the kappa = 2e-6 the lists are built with (10.5u + 1.3e-7 = 7.6e-7): X lies within R of c
//    and the listed boxes suffice as they are -- the grid is not rebuilt with another bound.  (Underflow is gradual on host and
//    device, denormals are not flushed: a product is off by at most 2^-149 absolutely, which moves E by less than 2^-73, against a
//    margin of at least 2^-66.)  By steps 2 and 3, read with o = P, d = toL -- the fp32 vector the test itself uses -- and t = k,
//    the sphere is listed in the cell whose walk interval holds k, or is in the large list.  k <= 1, so the walk runs with
//    tmax = 1 and may end once t_out of the cell just tested is past 1; there is no hit to report a t for, so it ends at the
//    first hit as well.  segment_walkable() is the classification, for the kernel (rtx_grid_shadow) and the host check alike;
//    tests/host/test_grid_shadow_bound.cpp checks the claim and the walk against float64.
//
// 5. Mirror rays (RTX_OPT_REFLECT_GRID).  A secondary ray of the mirror path is a query ray: mirror_ray and query_ray fill the same Ray
//    fields from (o, d) with the same operations (a = d . d, fourA = 4a, divTwoA = 1 / (2a)), both are tested with
//    secondary_sphere_hit, both take the minimum of (t, creation index) and skip the object the ray leaves, and a mirror ray has no
//    far limit: tmax = infinity.  Steps 1-3 therefore apply verbatim to rtx_grid_reflect's walk, with walkable() as the
//    classification; nothing new is bounded and no constant is added.
//
// Rays that are not walkable (origin or direction not finite, a = d . d outside [2^-40, 2^40], origin further than `reach` from
// the box centre on some axis) test every sphere instead.  tests/host/test_grid_bound.cpp checks all of this against float64;
// tests/test_gpu_grid_check.py runs the build and the walk on the device and holds them to this header evaluated on the host,
// bit for bit.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_GRID_HD __host__ __device__
#else
#define RTX_GRID_HD
#endif

namespace rtxgrid {

constexpr float kKappa = 2.0e-6f;
constexpr float kRel = 1.0e-4f;
constexpr float kMarginRel = 1.52587890625e-05f; // 2^-16 of the coordinate scale
constexpr float kReach = 3.0f;                   // walkable origins: within kReach x the largest half-extent of the box centre
constexpr float kTinyDir = 9.31322574615478515625e-10f; // 2^-30
constexpr float kMinA = 9.094947017729282e-13f;  // 2^-40
constexpr float kMaxA = 1.099511627776e12f;      // 2^40
constexpr float kMinScale = 8.881784197001252e-16f; // 2^-50
constexpr float kMaxScale = 1.125899906842624e15f;  // 2^50
constexpr uint32_t kLargeCells = 64;   // a sphere whose box covers more cells is kept out of the cells
constexpr uint32_t kLargeCap = 256;    // ... in a list of at most this many; more: the context answers with the brute kernel
constexpr uint32_t kMaxAxis = 1024;    // cells per axis
constexpr uint32_t kMaxCells = 1u << 21;
constexpr float kDefaultLoad = 1.0f;   // spheres per cell the resolution aims at (measured: EXPERIMENTS.md Round 7)

struct Grid {
    float lo[3];     // the grid box's low corner
    float cs[3];     // cell size per axis
    uint32_t n[3];   // cells per axis
    float ctr[3];    // centre of the spheres' bounding box
    float reach;     // walkable origins: |o_k - ctr_k| <= reach
    float margin;    // absolute margin of every listed box
    uint32_t ok;     // 0: no usable grid (no finite sphere, or a coordinate scale outside [2^-50, 2^50]): every ray tests every sphere
};

RTX_GRID_HD inline float edge(const Grid& g, int k, int i)
{
    const float p = (float)i * g.cs[k];
    return g.lo[k] + p;
}

RTX_GRID_HD inline bool finite_f(float x) { return fabsf(x) <= 3.0e38f; } // false for NaN

// Step 1: the half-width of the box sphere (c, r) is listed with: no walkable ray is reported to hit it further from c, margin included.
RTX_GRID_HD inline float sphere_half(const Grid& g, float cx, float cy, float cz, float r)
{
    const float ax = g.reach + fabsf(cx - g.ctr[0]), ay = g.reach + fabsf(cy - g.ctr[1]), az = g.reach + fabsf(cz - g.ctr[2]);
    const float D2 = (ax * ax + ay * ay + az * az) * (1.0f + kRel);
    const float R = sqrtf(r * r * (1.0f + kKappa) + kKappa * D2);
    return (R + g.margin) * (1.0f + kRel);
}

// Step 2: the cells [i0, i1] of axis k that meet [a, b] (a <= b, finite), by comparison with the boundaries themselves.
RTX_GRID_HD inline void cell_range(const Grid& g, int k, float a, float b, int& i0, int& i1)
{
    const int last = (int)g.n[k] - 1;
    const float fl = (float)last;
    float q0 = (a - g.lo[k]) / g.cs[k], q1 = (b - g.lo[k]) / g.cs[k];
    q0 = fminf(fmaxf(q0, 0.0f), fl);
    q1 = fminf(fmaxf(q1, 0.0f), fl);
    i0 = (int)q0;
    i1 = (int)q1;
    while (i0 > 0 && edge(g, k, i0) > a) i0--;         // the cell below reaches a
    while (i0 < last && edge(g, k, i0 + 1) < a) i0++;  // this cell ends before a
    while (i1 < last && edge(g, k, i1 + 1) < b) i1++;
    while (i1 > 0 && edge(g, k, i1) > b) i1--;
    if (i1 < i0) i1 = i0;
}

// The cells sphere (c, rw) is listed in (rw: the radius as the scene holds it, of either sign); false: a large sphere (its box is not
// finite or covers more than kLargeCells cells).  The build's kernels and the host checks share it.
RTX_GRID_HD inline bool sphere_cells(const Grid& g, float cx, float cy, float cz, float rw, int i0[3], int i1[3])
{
    const float r = fabsf(rw);
    const float h = sphere_half(g, cx, cy, cz, r);
    const float c[3] = {cx, cy, cz};
    bool fin = finite_f(h);
    uint32_t cells = 1u;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; k++) {
        const float a = c[k] - h, e = c[k] + h;
        fin = fin && finite_f(a) && finite_f(e);
        i0[k] = i1[k] = 0;
        if (fin) cell_range(g, k, a, e, i0[k], i1[k]);
        cells *= (uint32_t)(i1[k] - i0[k] + 1); // (at most 1024 per axis: no overflow)
    }
    return fin && cells <= kLargeCells;
}

// The planner: the grid of ns spheres whose boxes c +- |r| (finite ones only) span [blo, bhi]; load = spheres per cell aimed at.
inline Grid plan_grid(const float blo[3], const float bhi[3], uint32_t n_finite, float load)
{
    Grid g;
    for (int k = 0; k < 3; k++) {
        g.lo[k] = 0.0f;
        g.cs[k] = 1.0f;
        g.n[k] = 1;
        g.ctr[k] = 0.0f;
    }
    g.reach = 0.0f;
    g.margin = 0.0f;
    g.ok = 0;
    if (n_finite == 0) return g;
    float hmax = 0.0f, scale = 0.0f;
    for (int k = 0; k < 3; k++) {
        if (!finite_f(blo[k]) || !finite_f(bhi[k]) || !(blo[k] <= bhi[k])) return g;
        g.ctr[k] = 0.5f * blo[k] + 0.5f * bhi[k];
        hmax = fmaxf(hmax, 0.5f * bhi[k] - 0.5f * blo[k]);
        scale = fmaxf(scale, fmaxf(fabsf(blo[k]), fabsf(bhi[k])));
    }
    // a box without extent (one point sphere, identical centres of radius 0) still gets a cell: its size comes from the scale
    if (!(hmax > 0.0f)) hmax = scale > 0.0f ? scale * 1.0e-3f : 1.0f;
    scale = scale + 4.0f * hmax;
    if (!(scale >= kMinScale) || !(scale <= kMaxScale) || !(hmax >= kMinScale)) return g;
    g.reach = kReach * hmax;
    g.margin = kMarginRel * scale;
    // every point a walkable ray reports a hit at lies within the spheres' box grown by R - r <= r kappa / 2 + sqrt(kappa) D, D <= 4 sqrt(3) hmax;
    // the grid box holds that with more than margin to spare
    const float grow = (sqrtf(kKappa * 48.0f * (1.0f + kRel)) * hmax + g.margin) * (1.0f + 4.0f * kRel) + g.margin;
    float ext[3];
    double vol = 1.0;
    for (int k = 0; k < 3; k++) {
        g.lo[k] = blo[k] - grow;
        ext[k] = (bhi[k] + grow) - g.lo[k];
        if (!(ext[k] > 0.0f) || !finite_f(ext[k])) return g;
        // a flat axis counts as a hundredth of the largest one, so that it gets one cell and takes no resolution from the others
        vol *= (double)fmaxf(ext[k], 0.02f * hmax);
    }
    if (!(load > 0.0f)) load = kDefaultLoad;
    double cells = (double)n_finite / (double)load;
    if (cells < 1.0) cells = 1.0;
    if (cells > (double)kMaxCells) cells = (double)kMaxCells;
    const double side = cbrt(vol / cells); // cubic cells of this edge
    uint64_t total = 1;
    for (int k = 0; k < 3; k++) {
        double nk = floor((double)ext[k] / side + 0.5);
        if (!(nk >= 1.0)) nk = 1.0;
        if (nk > (double)kMaxAxis) nk = (double)kMaxAxis;
        g.n[k] = (uint32_t)nk;
        total *= g.n[k];
    }
    while (total > (uint64_t)kMaxCells) { // (rounding up on three axes can pass the cap: halve the finest axis)
        int big = 0;
        for (int k = 1; k < 3; k++) {
            if (g.n[k] > g.n[big]) big = k;
        }
        total /= g.n[big];
        g.n[big] = (g.n[big] + 1u) / 2u;
        total *= g.n[big];
    }
    for (int k = 0; k < 3; k++) {
        g.cs[k] = ext[k] / (float)g.n[k];
        // the last boundary must not fall short of the box: grow the cell by ulps until edge(n) covers it
        while (edge(g, k, (int)g.n[k]) < bhi[k] + grow) g.cs[k] = nextafterf(g.cs[k], INFINITY);
        if (!(g.cs[k] > 0.0f) || !finite_f(g.cs[k])) return g;
    }
    g.ok = 1;
    return g;
}

// ---- the walk
// May the ray be walked?  (Otherwise it tests every sphere.)
RTX_GRID_HD inline bool walkable(const Grid& g, const float o[3], float a)
{
    if (g.ok == 0u) return false;
    bool ok = a >= kMinA && a <= kMaxA; // (false for NaN; d finite follows from a finite)
    for (int k = 0; k < 3; k++) {
        ok = ok && fabsf(o[k] - g.ctr[k]) <= g.reach; // (false for NaN and infinities)
    }
    return ok;
}

// May the shadow segment (P, P + toL) be walked (d = toL, tmax = 1)?  a is formed as the shadow test forms len2.  A segment of no
// length (the light at the point itself) is not: a = 0.
RTX_GRID_HD inline bool segment_walkable(const Grid& g, const float P[3], const float toL[3])
{
    const float a = toL[0] * toL[0] + toL[1] * toL[1] + toL[2] * toL[2];
    return walkable(g, P, a);
}

struct Axis {
    float o, inv; // origin and 1 / d of the axis (inv unused when s == 0)
    int i, s;     // cell index; step +1 / -1, or 0: not walked
    float t_far;  // T of the boundary the ray leaves the cell through (+inf when s == 0)
};

RTX_GRID_HD inline float cross_t(const Axis& ax, float X) { return (X - ax.o) * ax.inv; }

// One axis of the start: the entry and exit parameters of the whole grid.  false: the ray never meets the grid on this axis.
RTX_GRID_HD inline bool axis_span(const Grid& g, int k, float o, float d, float dmax, Axis& ax, float& t_enter, float& t_exit)
{
    ax.o = o;
    ax.i = 0;
    ax.t_far = INFINITY;
    const float X0 = edge(g, k, 0), X1 = edge(g, k, (int)g.n[k]);
    if (!(fabsf(d) > kTinyDir * dmax)) {
        ax.s = 0;
        ax.inv = 0.0f;
        return o >= X0 && o <= X1;
    }
    ax.s = d > 0.0f ? 1 : -1;
    ax.inv = 1.0f / d;
    const float ta = cross_t(ax, d > 0.0f ? X0 : X1), tb = cross_t(ax, d > 0.0f ? X1 : X0);
    t_enter = fmaxf(t_enter, ta);
    t_exit = fminf(t_exit, tb);
    return true;
}

// ... and its start cell at t_start: the cell i with T(near boundary) <= t_start <= T(far boundary), found by comparing T values.
RTX_GRID_HD inline void axis_start(const Grid& g, int k, float d, float t_start, Axis& ax)
{
    const int last = (int)g.n[k] - 1;
    const float pos = ax.s == 0 ? ax.o : ax.o + t_start * d;
    float q = (pos - g.lo[k]) / g.cs[k];
    q = fminf(fmaxf(q, 0.0f), (float)last);
    int i = (int)q;
    if (ax.s == 0) {
        while (i > 0 && edge(g, k, i) > ax.o) i--;
        while (i < last && edge(g, k, i + 1) < ax.o) i++;
        ax.i = i;
        return;
    }
    if (ax.s > 0) {
        while (i < last && cross_t(ax, edge(g, k, i + 1)) < t_start) i++;
        while (i > 0 && cross_t(ax, edge(g, k, i)) > t_start) i--;
        ax.t_far = cross_t(ax, edge(g, k, i + 1));
    } else {
        while (i > 0 && cross_t(ax, edge(g, k, i)) < t_start) i--;
        while (i < last && cross_t(ax, edge(g, k, i + 1)) > t_start) i++;
        ax.t_far = cross_t(ax, edge(g, k, i));
    }
    ax.i = i;
}

struct Walk {
    Axis x, y, z;
    float t_in; // the current cell is valid for t in [t_in, t_out()]
};

RTX_GRID_HD inline float t_out(const Walk& w) { return fminf(w.x.t_far, fminf(w.y.t_far, w.z.t_far)); }

// The walk's first cell; false: the ray does not meet the grid at any t in [0, tmax].
RTX_GRID_HD inline bool walk_start(const Grid& g, const float o[3], const float d[3], float tmax, Walk& w)
{
    const float dmax = fmaxf(fabsf(d[0]), fmaxf(fabsf(d[1]), fabsf(d[2])));
    float t_enter = 0.0f, t_exit = INFINITY;
    bool meets = axis_span(g, 0, o[0], d[0], dmax, w.x, t_enter, t_exit);
    meets = axis_span(g, 1, o[1], d[1], dmax, w.y, t_enter, t_exit) && meets;
    meets = axis_span(g, 2, o[2], d[2], dmax, w.z, t_enter, t_exit) && meets;
    w.t_in = t_enter;
    if (!meets || !(t_enter <= t_exit) || !(t_enter <= tmax)) return false;
    axis_start(g, 0, d[0], t_enter, w.x);
    axis_start(g, 1, d[1], t_enter, w.y);
    axis_start(g, 2, d[2], t_enter, w.z);
    return true;
}

RTX_GRID_HD inline bool axis_step(const Grid& g, int k, Axis& ax, float& t_in)
{
    t_in = ax.t_far;
    ax.i += ax.s;
    if (ax.i < 0 || ax.i >= (int)g.n[k]) return false;
    ax.t_far = cross_t(ax, edge(g, k, ax.s > 0 ? ax.i + 1 : ax.i));
    return true;
}

// To the next cell; false: the ray has left the grid.
RTX_GRID_HD inline bool walk_step(const Grid& g, Walk& w)
{
    if (w.x.t_far <= w.y.t_far && w.x.t_far <= w.z.t_far) return axis_step(g, 0, w.x, w.t_in);
    if (w.y.t_far <= w.z.t_far) return axis_step(g, 1, w.y, w.t_in);
    return axis_step(g, 2, w.z, w.t_in);
}

RTX_GRID_HD inline uint32_t cell_index(const Grid& g, const Walk& w)
{
    return ((uint32_t)w.z.i * g.n[1] + (uint32_t)w.y.i) * g.n[0] + (uint32_t)w.x.i;
}

} // namespace rtxgrid
