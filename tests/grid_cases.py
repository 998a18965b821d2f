"""Scenes, rays and segments for the direct checks of the world grid (tests/test_gpu_grid_check.py on the device,
tests/test_host_grid_check.py without one), and the float64 side they are held to.  Everything is seeded numpy and small.

The float64 side restates csrc/rtx_grid.hpp's header, not its code:

  half64      H = (sqrt(r^2 (1 + kappa) + kappa D^2) + margin) (1 + kRel), D^2 = sum_k (reach + |c_k - ctr_k|)^2 (1 + kRel), in float64
              over the Grid's words, with the allowance A_k = 1e-6 H + 2^-23 (|c_k| + H) by which the fp32 box may differ from it:
              sphere_half is about twenty fp32 operations whose relative errors (2^-24 each, halved under the root) add up to under
              10 x 2^-24 = 6e-7 < 1e-6, and c -+ h is one more rounding, of a number no larger than |c_k| + h: 2^-24 (|c_k| + h), taken
              twice over.  Nothing here is measured.
  ranges64    per axis the cells whose [edge(i), edge(i + 1)] meets c +- (H - A) (they must list the sphere: L1) and c +- (H + A)
              (no other may: L2); a sphere is large when the first product passes 64 cells, small when the second does not (L3).
  walkable64  the header's rule on (o, d) in float64; None within 1e-6 of a threshold.
  hits64      the quadratic of Sphere::Trace in float64 (near root, t >= 0, t <= tmax, t < kNoHit).  DESIGN 4.1 bounds the fp32 test: it reports a
              hit exactly when the ray passes within sqrt(r^2 (1 + 2u) + 15.2u |o - c|^2) of the centre, u = 2^-24, give or take
              that much again; a pair is clear when |q^2 - r^2| > 4 (2u r^2 + 15.2u |o - c|^2) for the float64 distance q of the
              centre from the line, and its t is off 0 and tmax by more than 1e-4 relative.
  closest64   the winner (t, creation index) among the clear pairs; None when an unclear pair could come first or two clear ones
              of different geometry are within 1e-5 of each other.
  dark64      a segment is dark when the centre of a sphere other than its own is within r of it; step 4 of the header bounds the
              fp32 test by r (1 + 5.2u) + 2.01u D: clear when the float64 distance is off r by more than 1e-5 r + 1e-6 D.

plan32 is the planner evaluated in float32 by numpy, operation for operation; the device's Grid is compared with it bit for bit,
and the cases are built around it (a sphere whose box ends on an edge() value, origins at the rim of `reach`).

Grazing rays and segments sit on the fp32 tests' threshold by construction: at the rim of `reach` |o - c| / r is in the hundreds
and no epsilon of the 1e-3 .. 1e-6 the class uses is clear.  They are what S1 is for (every sphere the production test reports is
listed where the walk looks), and grid = brute holds for them bit for bit; the share float64 may leave undecided (2 %) is asserted
over the other classes, and a grazing ray that float64 does decide must agree like any other.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
K_KAPPA, K_REL = float(F32(2.0e-6)), float(F32(1.0e-4))
K_TINY, MIN_A, MAX_A = 2.0 ** -30, 2.0 ** -40, 2.0 ** 40
LARGE_CELLS, LARGE_CAP, MAX_AXIS, MAX_CELLS = 64, 256, 1024, 1 << 21
NONE = 0xFFFFFFFF
NO_HIT = F32(99999999.0)
EPS = (1e-3, 1e-4, 1e-5, 1e-6)


GIDX_MUL, GIDX_MOD = 400, 65537  # (a prime above every scene's size: i -> 400 i mod 65537 is one to one)


def gidx_of(i):
    """The creation index the check library's scenes give the sphere at position i: a permutation, not the position and not rising
    with it (of n257's twins at 100 and 200 the later one was created first), so that neither can stand in for the other."""
    i = np.asarray(i, np.int64)
    return np.where(i == NONE, NONE, (i * GIDX_MUL) % GIDX_MOD + 5).astype(np.uint32)


def index_of(gidx):
    """The position of the sphere of creation index gidx (gidx_of's inverse; -1 for a word no sphere has)."""
    g = np.asarray(gidx, np.int64) - 5
    i = (g * pow(GIDX_MUL, -1, GIDX_MOD)) % GIDX_MOD
    return np.where((g >= 0) & (g < GIDX_MOD), i, -1)


def creation_order(ns):
    """(order, rank): the positions in creation order, and each position's place in it."""
    order = np.argsort(gidx_of(np.arange(ns)), kind="stable")
    rank = np.empty(ns, np.int64)
    rank[order] = np.arange(ns)
    return order, rank


# ---------------------------------------------------------------------------------------------- float32: bounds and the planner

def finite32(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x) <= F32(3.0e38)


def bounds32(geom):
    """The seven bounds words: fp32 min / max of c -+ |r| over the finite spheres, and their number."""
    g = np.asarray(geom, F32)
    r = np.abs(g[:, 3])
    fin = finite32(g[:, 0]) & finite32(g[:, 1]) & finite32(g[:, 2]) & finite32(r)
    lo, hi = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
    if fin.any():
        with np.errstate(over="ignore"):
            lo, hi = (g[fin, :3] - r[fin, None]).min(0), (g[fin, :3] + r[fin, None]).max(0)
    return lo.astype(F32), hi.astype(F32), int(fin.sum()), fin


def edge32(g, k, i):
    return F32(g["lo"][k] + F32(F32(i) * g["cs"][k]))


def plan32(blo, bhi, nf, load):
    """rtxgrid::plan_grid in float32 (doubles where it uses doubles).  g["halved"]: the cap's loop ran."""
    one, kk, kr = F32(1), F32(2.0e-6), F32(1.0e-4)
    g = dict(lo=np.zeros(3, F32), cs=np.ones(3, F32), n=np.ones(3, np.uint32), ctr=np.zeros(3, F32), reach=F32(0), margin=F32(0), ok=0, halved=False)
    if nf == 0:
        return g
    with np.errstate(all="ignore"):
        hmax, scale = F32(0), F32(0)
        for k in range(3):
            if not (finite32(blo[k]) and finite32(bhi[k]) and blo[k] <= bhi[k]):
                return g
            g["ctr"][k] = F32(0.5) * blo[k] + F32(0.5) * bhi[k]
            hmax = max(hmax, F32(F32(0.5) * bhi[k] - F32(0.5) * blo[k]))
            scale = max(scale, max(abs(blo[k]), abs(bhi[k])))
        if not hmax > 0:
            hmax = F32(scale * F32(1.0e-3)) if scale > 0 else one
        scale = F32(scale + F32(4) * hmax)
        if not scale >= F32(2.0 ** -50) or not scale <= F32(2.0 ** 50) or not hmax >= F32(2.0 ** -50):
            return g
        g["reach"], g["margin"] = F32(F32(3) * hmax), F32(F32(2.0 ** -16) * scale)
        grow = F32(F32(F32(np.sqrt(F32(F32(kk * F32(48)) * F32(one + kr))) * hmax) + g["margin"]) * F32(one + F32(F32(4) * kr))) + g["margin"]
        grow = F32(grow)
        ext, vol = np.zeros(3, F32), 1.0
        for k in range(3):
            g["lo"][k] = blo[k] - grow
            ext[k] = F32(bhi[k] + grow) - g["lo"][k]
            if not ext[k] > 0 or not finite32(ext[k]):
                return g
            vol *= float(max(ext[k], F32(F32(0.02) * hmax)))
        load = F32(load) if load > 0 else one
        cells = min(max(float(nf) / float(load), 1.0), float(MAX_CELLS))
        side = float(np.cbrt(vol / cells))
        total = 1
        for k in range(3):
            nk = np.floor(float(ext[k]) / side + 0.5)
            nk = min(max(nk, 1.0), float(MAX_AXIS)) if nk >= 1.0 else 1.0
            g["n"][k] = int(nk)
            total *= int(nk)
        while total > MAX_CELLS:
            g["halved"] = True
            big = 0
            for k in (1, 2):
                if g["n"][k] > g["n"][big]:
                    big = k
            total //= int(g["n"][big])
            g["n"][big] = (int(g["n"][big]) + 1) // 2
            total *= int(g["n"][big])
        for k in range(3):
            g["cs"][k] = ext[k] / F32(g["n"][k])
            while edge32(g, k, int(g["n"][k])) < F32(bhi[k] + grow):
                g["cs"][k] = np.nextafter(g["cs"][k], F32(np.inf))
            if not g["cs"][k] > 0 or not finite32(g["cs"][k]):
                return g
    g["ok"] = 1
    return g


def plan_of(geom, load):
    lo, hi, nf, _ = bounds32(geom)
    return plan32(lo, hi, nf, load)


def grid_words(g):
    """The Grid as the 15 words the library hands back."""
    return np.concatenate([g["lo"].view(np.uint32), g["cs"].view(np.uint32), g["n"].astype(np.uint32), g["ctr"].view(np.uint32),
                           np.array([g["reach"], g["margin"]], F32).view(np.uint32), np.array([g["ok"]], np.uint32)])


def grid_from_words(w):
    w = np.ascontiguousarray(w, np.uint32)
    f = w.view(F32)
    return dict(lo=f[0:3].copy(), cs=f[3:6].copy(), n=w[6:9].copy(), ctr=f[9:12].copy(), reach=f[12], margin=f[13], ok=int(w[14]), halved=False)


def n_cells(g):
    return int(g["n"][0]) * int(g["n"][1]) * int(g["n"][2]) if g["ok"] else 0


def edges(g, k):
    """The n[k] + 1 boundaries of axis k: fp32 values, as float64."""
    i = np.arange(int(g["n"][k]) + 1, dtype=F32)
    return (g["lo"][k] + (i * g["cs"][k]).astype(F32)).astype(F32).astype(np.float64)


def sphere_half32(g, c, r):
    """rtxgrid::sphere_half in float32, for one sphere."""
    one, kk, kr = F32(1), F32(2.0e-6), F32(1.0e-4)
    with np.errstate(all="ignore"):
        a = [F32(g["reach"] + abs(F32(F32(c[k]) - g["ctr"][k]))) for k in range(3)]
        d2 = F32(F32(F32(F32(a[0] * a[0]) + F32(a[1] * a[1])) + F32(a[2] * a[2])) * F32(one + kr))
        rr = F32(np.sqrt(F32(F32(F32(F32(r) * F32(r)) * F32(one + kk)) + F32(kk * d2))))
        return F32(F32(rr + g["margin"]) * F32(one + kr))


# ---------------------------------------------------------------------------------------------- float64: the lists

def half64(g, geom):
    """(H, A): the header's half-width per sphere and the allowance per sphere and axis; NaN / inf for spheres that are not finite."""
    s = np.asarray(geom, np.float64)
    c, r = s[:, :3], np.abs(s[:, 3])
    with np.errstate(all="ignore"):
        d2 = ((float(g["reach"]) + np.abs(c - g["ctr"].astype(np.float64))) ** 2).sum(1) * (1.0 + K_REL)
        h = (np.sqrt(r * r * (1.0 + K_KAPPA) + K_KAPPA * d2) + float(g["margin"])) * (1.0 + K_REL)
        a = 1.0e-6 * h[:, None] + 2.0 ** -23 * (np.abs(c) + h[:, None])
    return h, a


def ranges64(g, geom):
    """must (ns, 3, 2), may (ns, 3, 2): first and last cell per axis for H - A and H + A; finite (ns): H and the box are finite."""
    s = np.asarray(geom, np.float64)
    h, a = half64(g, geom)
    with np.errstate(all="ignore"):
        finite = np.isfinite(h) & np.isfinite(s[:, :3]).all(1) & (h < 3.0e38) & (np.abs(s[:, :3]) + h[:, None] < 3.0e38).all(1)
    must, may = np.zeros((len(s), 3, 2), np.int64), np.zeros((len(s), 3, 2), np.int64)
    with np.errstate(all="ignore"):
        narrow, wide = h[:, None] - a, h[:, None] + a
    for k in range(3):
        e = edges(g, k)
        last = len(e) - 2
        for out, hw in ((must, narrow), (may, wide)):
            with np.errstate(all="ignore"):
                lo, hi = np.where(finite, s[:, k] - hw[:, k], 0.0), np.where(finite, s[:, k] + hw[:, k], 0.0)
            # first cell whose upper boundary reaches lo; last cell whose lower boundary does not pass hi
            out[:, k, 0] = np.clip(np.searchsorted(e[1:], lo, side="left"), 0, last)
            out[:, k, 1] = np.clip(np.searchsorted(e[:-1], hi, side="right") - 1, 0, last)
    return must, may, finite


def large64(g, geom):
    """1 large, 0 small, -1 undecided (within the allowance of a cell boundary), per sphere."""
    must, may, finite = ranges64(g, geom)
    c_lo = np.prod(np.maximum(must[:, :, 1] - must[:, :, 0] + 1, 1), axis=1)
    c_hi = np.prod(np.maximum(may[:, :, 1] - may[:, :, 0] + 1, 1), axis=1)
    out = np.where(c_lo > LARGE_CELLS, 1, np.where(c_hi <= LARGE_CELLS, 0, -1))
    return np.where(finite, out, 1)


# ---------------------------------------------------------------------------------------------- float64: rays

def split(rays):
    r = np.asarray(rays, F32).reshape(-1, 8)
    return r[:, 0:3].astype(np.float64), r[:, 4:7].astype(np.float64), r[:, 3].astype(np.float64), np.ascontiguousarray(r[:, 7]).view(np.uint32)


def walkable64(g, o, d):
    """1 / 0 per ray, -1 within 1e-6 of a threshold."""
    with np.errstate(all="ignore"):
        a = (d * d).sum(1)
        off = np.abs(o - g["ctr"].astype(np.float64))
        reach = float(g["reach"])
        ok = (a >= MIN_A) & (a <= MAX_A) & (off <= reach).all(1) & np.isfinite(o).all(1) & np.isfinite(d).all(1)
        near = (np.abs(a / MIN_A - 1.0) < 1e-6) | (np.abs(a / MAX_A - 1.0) < 1e-6) | (np.abs(off / reach - 1.0) < 1e-6).any(1)
    if not g["ok"]:
        return np.zeros(len(o), np.int64)
    return np.where(near, -1, ok.astype(np.int64))


def meets64(g, o, d, tmax):
    """Does the ray meet the grid box within [0, tmax]?  1 / 0, -1 when only the box grown or shrunk by `margin` says so."""
    res = []
    for grow in (-float(g["margin"]), float(g["margin"])):
        t0, t1 = np.zeros(len(o)), np.full(len(o), np.inf)
        ok = np.ones(len(o), bool)
        dmax = np.abs(d).max(1)
        for k in range(3):
            e = edges(g, k)
            lo, hi = e[0] - grow, e[-1] + grow
            with np.errstate(all="ignore"):
                walked = np.abs(d[:, k]) > K_TINY * dmax
                ta, tb = (lo - o[:, k]) / d[:, k], (hi - o[:, k]) / d[:, k]
                t0 = np.where(walked, np.maximum(t0, np.minimum(ta, tb)), t0)
                t1 = np.where(walked, np.minimum(t1, np.maximum(ta, tb)), t1)
                ok &= walked | ((o[:, k] >= lo) & (o[:, k] <= hi))
        with np.errstate(all="ignore"):
            res.append(ok & (t0 <= t1) & (t0 <= tmax * (1.0 - 1e-6 * np.sign(grow))))
    return np.where(res[0] == res[1], res[0].astype(np.int64), -1)


def hits64(rays, geom):
    """t (n, ns) float64, +inf where the ray misses or the near root is negative; clear (n, ns) bool."""
    o, d, tmax, _ = split(rays)
    s = np.asarray(geom, np.float64)
    with np.errstate(all="ignore"):
        oc = o[:, None, :] - s[None, :, :3]
        a = (d * d).sum(1)[:, None]
        b = 2.0 * (oc * d[:, None, :]).sum(2)
        oo = (oc * oc).sum(2)
        r2 = (s[:, 3] ** 2)[None, :]
        disc = b * b - 4.0 * a * (oo - r2)
        t = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a)
        # (a ray starts from t = kNoHit = 99999999 as its best: nothing at or beyond it is reported)
        hit = (disc >= 0.0) & (t >= 0.0) & (t <= tmax[:, None]) & (t < float(NO_HIT))
        q2 = oo - b * b / (4.0 * a)  # squared distance of the centre from the line
        clear = np.abs(q2 - r2) > 4.0 * (2.0 * U * r2 + 15.2 * U * oo)
        tref = np.sqrt(oo / a)
        at_limit = np.isfinite(tmax)[:, None] & (np.abs(t - tmax[:, None]) <= 1e-4 * np.abs(tmax[:, None]))
        at_limit |= np.abs(t - float(NO_HIT)) <= 1e-4 * float(NO_HIT)
        clear &= ~((disc >= 0.0) & ((np.abs(t) <= 1e-4 * tref) | at_limit))
        clear &= np.isfinite(a) & (a > 0.0) & np.isfinite(o).all(1)[:, None]
        # a sphere that is not finite is never reported (NaN or -inf for t: no comparison takes it): a clear miss
        clear |= ~np.isfinite(s).all(1)[None, :] & np.isfinite(a)
    return np.where(hit, t, np.inf), clear


def closest64(rays, geom):
    """(winner sphere index or NONE, decided) per ray: the lexicographic minimum of (t, creation index) among the clear pairs, the skipped
    sphere left out; undecided when an unclear pair could come first or two clear hits of different geometry are within 1e-5."""
    t, clear = hits64(rays, geom)
    o, d, tmax, skip = split(rays)
    n, ns = t.shape
    s = np.asarray(geom, F32)
    usable = np.isfinite(s).all(1)
    cols = np.arange(ns)[None, :]
    skipped = cols == np.where(skip == NONE, -1, skip.astype(np.int64))[:, None]
    tc = np.where(clear & ~skipped & usable[None, :], t, np.inf)
    order, _ = creation_order(ns)
    win = order[tc[:, order].argmin(1)]  # (of equal t the lower creation index)
    tw = tc[np.arange(n), win]
    best = np.where(np.isfinite(tw), win, NONE)
    # an unclear pair (not skipped) whose root, as far as float64 sees it, does not come clearly behind the winner
    with np.errstate(all="ignore"):
        oc = o[:, None, :] - s[None, :, :3].astype(np.float64)
        a = (d * d).sum(1)[:, None]
        tmid = -(oc * d[:, None, :]).sum(2) / a  # the parameter of closest approach bounds the root from above
        rr = np.abs(s[:, 3].astype(np.float64))[None, :] / np.sqrt(a)
        could = ~clear & ~skipped & ~((tmid - rr) * (1.0 - 1e-4) > tw[:, None]) & ~((tmid + rr) < 0.0) & ~((tmid - rr) > tmax[:, None] * (1.0 + 1e-4))
        near = np.isfinite(tc) & (tc <= tw[:, None] * (1.0 + 1e-5)) & (cols != win[:, None])
        same = (s[None, :, :] == s[win][:, None, :]).all(2)
        tie = (near & ~same).any(1)
    # nothing to report: a far limit that is negative or NaN; an origin or direction that is not finite, a direction of no length or
    # one whose square overflows fp32 -- every root is NaN then, and no comparison takes a NaN
    with np.errstate(all="ignore"):
        dead = ~(tmax >= 0.0) | ~np.isfinite(o).all(1) | ~np.isfinite(d).all(1) | ~(a[:, 0] > 0.0) | ~(a[:, 0] < 3.0e38)
    decided = (~could.any(1) & ~tie) | dead
    return np.where(dead, NONE, best).astype(np.int64), decided


def dark64(P, L, own_pos, geom):
    """1 / 0 per segment, -1 undecided; toL = fp32 L - P as the kernels form it."""
    p = np.asarray(P, F32).astype(np.float64)
    toL = (np.asarray(L, F32) - np.asarray(P, F32)).astype(np.float64)
    s = np.asarray(geom, np.float64)
    with np.errstate(all="ignore"):
        w = s[None, :, :3] - p[:, None, :]
        len2 = (toL * toL).sum(1)[:, None]
        k = np.clip(np.where(len2 > 0.0, (w * toL[:, None, :]).sum(2) / len2, 0.0), 0.0, 1.0)
        e = w - k[:, :, None] * toL[:, None, :]
        dist = np.sqrt((e * e).sum(2))
        r = np.abs(s[:, 3])[None, :]
        D = np.sqrt((w * w).sum(2))
        tol = 1e-5 * r + 1e-6 * D
        other = np.arange(len(s))[None, :] != np.where(np.asarray(own_pos) == NONE, -1, np.asarray(own_pos, np.int64))[:, None]
        fin = np.isfinite(s[:, :3]).all(1)[None, :] & np.isfinite(p).all(1)[:, None] & np.isfinite(toL).all(1)[:, None]
        # (a centre that is not finite gives NaN or inf for e . e: never a hit; an infinite radius about a finite centre: always)
        sure_hit = fin & other & np.where(np.isinf(r), True, dist < r - tol)
        maybe = fin & other & np.isfinite(r) & (np.abs(dist - r) <= tol)
    return np.where(sure_hit.any(1), 1, np.where(maybe.any(1), -1, 0))


# ---------------------------------------------------------------------------------------------- the scenes

def _cloud(rng, n, lo, hi, rlo, rhi):
    g = np.empty((n, 4), np.float64)
    g[:, :3] = rng.uniform(lo, hi, (n, 3))
    g[:, 3] = rng.uniform(rlo, rhi, n)
    return g


def _find_load(geom, target):
    for load in np.geomspace(0.25, 4.0, 4001):
        load = float(F32(load))
        if n_cells(plan_of(geom, load)) == target:
            return load
    raise AssertionError("no load gives %d cells" % target)


def _on_edge(rng):
    """200 spheres in [0, 10]^3, two of them pinning the box, and 48 whose listed box c +- h ends on an edge() value: the even ones
    exactly, the odd ones past it by 0.3 kRel h -- inside the share of h that (1 + kRel) adds and well outside the allowance."""
    base = _cloud(rng, 200, 1.0, 9.0, 0.05, 0.3)
    base[0], base[1] = (0.5, 0.5, 0.5, 0.5), (9.5, 9.5, 9.5, 0.5)
    extra = _cloud(rng, 48, 3.0, 7.0, 0.1, 0.1)
    geom = np.concatenate([base, extra]).astype(F32)
    lo, hi, nf, _ = bounds32(geom)
    g = plan32(lo, hi, nf, 1.0)  # (the 48 lie inside the box: their radii do not move it)
    found = 0
    for j in range(200, 248):
        k, sgn = (j - 200) % 3, 1.0 if (j // 3) % 2 else -1.0
        c = geom[j, :3]

        def end(rbits):
            h = sphere_half32(g, c, np.uint32(rbits).view(F32))
            return F32(c[k] + F32(sgn) * h)
        r0 = F32(0.1)
        e0 = float(end(r0.view(np.uint32)))
        ed = edges(g, k)
        X = ed[np.searchsorted(ed, e0)] if sgn > 0 else ed[np.searchsorted(ed, e0) - 1]  # the next boundary outwards
        a, b = int(r0.view(np.uint32)), int(F32(3.0).view(np.uint32))
        while b - a > 1:  # (c + sgn h is monotonic in the radius' bits)
            m = (a + b) // 2
            if (float(end(m)) - X) * sgn < 0.0:
                a = m
            else:
                b = m
        if float(end(b)) == X:
            if j % 2:  # just past: the radius at which the end is X + 0.3 kRel h (h changes by parts in 1e4 over the search)
                X = X + sgn * 0.3 * K_REL * float(sphere_half32(g, c, np.uint32(b).view(F32)))
                a, b = b, int(F32(3.0).view(np.uint32))
                while b - a > 1:
                    m = (a + b) // 2
                    if (float(end(m)) - X) * sgn < 0.0:
                        a = m
                    else:
                        b = m
            geom[j, 3] = np.uint32(b).view(F32)
            found += 1
    assert found >= 40, found
    return geom


NAMES = ("n1", "n255", "n256", "n257", "n1025", "s1e-6", "s1e6", "off1e4", "flat", "point", "bigr", "negr", "dense", "onedge", "c1025", "half", "cap", "halve", "fine",
         "large256", "large257", "nofinite", "huge")
NOGRID = ("nofinite", "huge")  # no usable grid (rtxgrid::Grid::ok == 0): every ray and segment tests every sphere
_SCENES = {}


def scene(name):
    if not _SCENES:
        _SCENES.update(scenes())
    return _SCENES[name]


def scenes():
    """name -> (geom float32 (ns, 4), load).  The first block is walked and queried too (at most 64 cells an axis)."""
    rng = np.random.default_rng(2400)
    out = {}
    out["n1"] = (np.array([[0.3, 0.2, 0.1, 0.5]]), 1.0)
    for n in (255, 256, 257):
        g = _cloud(rng, n, 0.0, 10.0, 0.05, 0.4)
        if n == 257:
            g[200] = g[100]  # twins: equal t for every ray, the one created first wins
            g[201, :3], g[201, 3] = g[101, :3], g[101, 3] * 0.5  # concentric
        out["n%d" % n] = (g, 1.0)
    out["n1025"] = (_cloud(rng, 1025, 0.0, 10.0, 0.02, 0.25), 1.0)
    out["s1e-6"] = (out["n257"][0] * 1e-6, 1.0)
    out["s1e6"] = (out["n257"][0] * 1e6, 1.0)
    g = _cloud(rng, 257, 0.0, 10.0, 0.05, 0.4)
    g[:, :3] += 1.0e4
    out["off1e4"] = (g, 1.0)
    g = _cloud(rng, 257, 0.0, 10.0, 0.0, 0.0)
    g[:, 2] = 2.5
    out["flat"] = (g, 1.0)
    out["point"] = (np.tile(np.array([[1.0, 2.0, 3.0, 0.0]]), (256, 1)), 1.0)
    out["bigr"] = (_cloud(rng, 64, 0.0, 10.0, 2.0, 6.0), 0.25)
    g = _cloud(rng, 257, 0.0, 10.0, 0.05, 0.4)
    g[10:40, 3] *= -1.0
    g[40:42, 3] = -np.inf
    g[42, 3] = np.nan
    g[43, 3] = np.inf
    g[44, 0], g[45, 1], g[46, 2], g[47, 0] = np.nan, np.inf, -np.inf, np.nan
    out["negr"] = (g, 1.0)
    g = _cloud(rng, 1026, 0.4995, 0.5005, 1e-5, 2e-5)
    g[1024], g[1025] = (-50.0, -40.0, -30.0, 1.0), (50.0, 45.0, 35.0, 1.0)
    out["dense"] = (g, 1.0)
    out["onedge"] = (_on_edge(rng), 1.0)
    # ---- build only
    g = _cloud(rng, 1025, 0.0, 1.0, 0.002, 0.01) * np.array([41.0, 25.0, 0.0, 1.0])
    g[:, 3] = 0.0
    out["c1025"] = (g, _find_load(g.astype(F32), 1025))
    out["half"] = (out["n1025"][0], 0.5)
    g = _cloud(rng, 2048, 0.0, 1.0, 0.001, 0.01)
    for shape in ((10.0, 9.0, 8.0), (10.0, 9.5, 7.0), (10.0, 8.5, 6.5), (10.0, 7.0, 5.5), (10.0, 9.0, 7.5)):
        # (a box whose three roundings together pass the cap, so that the planner's halving loop runs)
        cand = g * np.array(shape + (1.0,))
        if plan_of(cand.astype(F32), 2.0 ** -10)["halved"]:
            break
    out["halve"] = (cand, 2.0 ** -10)
    out["cap"] = (_cloud(rng, 2048, 0.0, 10.0, 0.001, 0.01), 2.0 ** -10)
    out["fine"] = (_cloud(rng, 300, 0.0, 10.0, 0.8, 1.2), 2.0 ** -10)
    for n in (256, 257):
        g = np.concatenate([_cloud(rng, 600, 5.0, 95.0, 0.05, 0.15), _cloud(rng, n, 35.0, 65.0, 28.0, 32.0)])
        g[0], g[1] = (1.0, 1.0, 1.0, 1.0), (99.0, 99.0, 99.0, 1.0)
        out["large%d" % n] = (g[rng.permutation(len(g))], 1.0)
    # ---- no usable grid: no finite sphere; a coordinate scale beyond 2^50
    g = _cloud(rng, 8, 0.0, 10.0, 0.5, 1.0)
    g[0:3, 0], g[3:5, 1], g[5:7, 3], g[7, 2] = np.nan, np.inf, -np.inf, -np.inf
    out["nofinite"] = (g, 1.0)
    g = _cloud(rng, 64, 0.0, 2.0 ** 52, 1.0e12, 1.0e12)
    out["huge"] = (g, 1.0)
    return {k: (np.ascontiguousarray(v[0], F32), float(v[1])) for k, v in out.items()}


def nogrid_rays(name, geom, n=256):
    """Rays for a scene without a grid, aimed at (and a radius or so beside) its spheres where it has finite ones: from 3 r, with a
    direction of length 2e5 so that the hit's t, 1e7, stays below kNoHit and no product of the test overflows.  A quarter cannot
    report anything (tmax negative or NaN); the skip word is a sphere's position or NONE."""
    rng = np.random.default_rng(sum(map(ord, name)) + 2403)
    s = np.asarray(geom, np.float64)
    ok = np.flatnonzero(np.isfinite(s).all(1))
    rays = np.zeros((n, 8), F32)
    for i in range(n):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if len(ok):
            j = int(rng.choice(ok))
            c, r = s[j, :3], abs(s[j, 3])
            o = c + 3.0 * r * u
            d = c + _perp(rng, u) * r * rng.uniform(0.0, 2.0) - o
            d *= 2.0e5 / np.linalg.norm(d)
        else:
            j, o, d = int(rng.integers(0, len(s))), rng.uniform(0.0, 10.0, 3), u
        rays[i, 0:3], rays[i, 4:7] = o, d
        rays[i, 3] = [np.inf, 1.0e8, -1.0, np.nan][i % 4] if i % 2 else np.inf
        rays[i, 7:8] = np.array([j if i % 8 == 0 else NONE], np.uint32).view(F32)
    return rays


WALKED = ("n1", "n255", "n256", "n257", "n1025", "s1e-6", "s1e6", "off1e4", "flat", "point", "bigr", "negr", "dense", "onedge")
# the product takes the load in sixteenths (RTX_OPT_QUERY_LOAD): these scenes' loads are such
PRODUCT = ("n1", "n257", "n1025", "s1e-6", "s1e6", "off1e4", "flat", "bigr", "negr", "dense", "onedge", "half", "large256", "large257")


# ---------------------------------------------------------------------------------------------- rays

def _perp(rng, u):
    v = np.cross(u, rng.normal(size=3))
    if not np.linalg.norm(v) > 1e-9:
        v = np.cross(u, np.array([0.0, 0.0, 1.0]) if abs(u[2]) < 0.9 else np.array([1.0, 0.0, 0.0]))
    return v / np.linalg.norm(v)


FACES = [np.array(v, np.float64) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
CORNERS = [np.array((sx, sy, sz), np.float64) / np.sqrt(3.0) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
CLASSES = ("grazing", "axis", "tiny", "faces", "outside", "tmax", "ulp", "broken", "skip", "random")


def _rim(g, p, w):
    """How far back from p along -w the origin may go before an axis passes 0.98 `reach`."""
    ctr, reach = g["ctr"].astype(np.float64), 0.98 * float(g["reach"])
    with np.errstate(all="ignore"):
        s = np.where(w > 0, (p - (ctr - reach)) / w, np.where(w < 0, (p - (ctr + reach)) / w, np.inf))
    return max(float(s.min()), 0.0)


def rays_of(name, geom, g, per_class=256, graze_spheres=None):
    """(rays float32 (n, 8) with the skip word a SPHERE INDEX or NONE, cls (n,) index into CLASSES, eps (n,) signed epsilon of grazing
    rays, far (n,) origin at the rim)."""
    rng = np.random.default_rng(sum(map(ord, name)) + 2401)
    s = np.asarray(geom, np.float64)
    ok = np.isfinite(s).all(1)
    ctr, reach = g["ctr"].astype(np.float64), float(g["reach"])
    half = np.array([(edges(g, k)[-1] - edges(g, k)[0]) / 2 for k in range(3)])
    mid = np.array([(edges(g, k)[-1] + edges(g, k)[0]) / 2 for k in range(3)])
    rows, cls, eps_, far_ = [], [], [], []

    def add(c, o, d, tmax=np.inf, skip=NONE, eps=0.0, far=False):
        row = np.zeros(8, F32)
        with np.errstate(all="ignore"):
            row[0:3], row[3], row[4:7] = np.asarray(o, np.float64), tmax, np.asarray(d, np.float64)
        row[7:8] = np.array([skip], np.uint32).view(F32)
        rows.append(row)
        cls.append(CLASSES.index(c))
        eps_.append(eps)
        far_.append(far)

    def inside(spread=1.0):
        return mid + rng.uniform(-spread, spread, 3) * half

    # grazing: past the tangent point towards each face and corner of the sphere's box, at r (1 +- eps), from the rim and from close by
    idx = np.flatnonzero(ok & (np.abs(s[:, 3]) > 0))
    if graze_spheres is None:  # every sphere while the class stays within 4096 rays, a sample of 96 beyond
        graze_spheres = len(idx) if 14 * len(idx) <= 4096 else 96
    pick = idx if len(idx) <= graze_spheres else rng.choice(idx, graze_spheres, replace=False)
    skip_rows = []
    for j in pick:
        c, r = s[j, :3], abs(s[j, 3])
        for m, u in enumerate(FACES + CORNERS):
            e = EPS[int(rng.integers(0, 4))] * (1.0 if rng.random() < 0.4 else -1.0)
            far = bool(m % 2 == (j % 2))
            w = _perp(rng, u)
            p = c + r * (1.0 + e) * u
            back = 0.98 * _rim(g, p, w) if far else 2.0 * r
            d = w * rng.uniform(0.5, 2.0)
            add("grazing", p - back * w, d, eps=e, far=far)
            if e < 0 and len(skip_rows) < per_class:
                skip_rows.append((p - back * w, d, int(j)))
    for o, d, j in skip_rows:  # the sphere aimed at is the one to skip
        add("skip", o, d, skip=j)
    for _ in range(per_class):  # axis-parallel, zeros of both signs, half of them lying in a cell face
        ax = int(rng.integers(0, 3))
        o, d = inside(1.3), np.zeros(3)
        d[ax] = rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 10.0)
        d[(ax + 1) % 3] = rng.choice([0.0, -0.0])
        if rng.random() < 0.5:
            k = (ax + 1) % 3
            o[k] = float(edge32(g, k, int(rng.integers(0, int(g["n"][k]) + 1))))
        add("axis", o, d)
    tiny = F32(2.0 ** -30)
    for i in range(per_class // 2):  # a component at kTinyDir dmax exactly (not walked), one ulp above (walked), one below, and well apart
        ax, k = int(rng.integers(0, 3)), int(rng.integers(1, 3))
        d = np.zeros(3)
        d[ax] = rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(-3, 4))
        comp = [tiny, np.nextafter(tiny, F32(1)), np.nextafter(tiny, F32(0)), F32(2.0 ** -20), F32(2.0 ** -40)][i % 5]
        d[(ax + k) % 3] = float(comp) * abs(d[ax]) * rng.choice([-1.0, 1.0])
        add("tiny", inside(0.9), d)
    for i in range(per_class):  # in a cell face; through a cell corner; from one
        cn = np.array([float(edge32(g, k, int(rng.integers(0, int(g["n"][k]) + 1)))) for k in range(3)])
        if i % 3 == 0:
            ax = int(rng.integers(0, 3))
            o, d = inside(1.2), rng.normal(size=3)
            o[ax], d[ax] = cn[ax], 0.0
            add("faces", o, d)
        elif i % 3 == 1:
            add("faces", cn, rng.normal(size=3))
        else:
            o = inside(1.5)
            add("faces", o, (cn - o) / half.max())  # (a difference of positions, brought to the size a walkable direction has)
    for i in range(per_class):  # from outside the grid (within reach), pointing in and pointing away
        ax, sgn = int(rng.integers(0, 3)), rng.choice([-1.0, 1.0])
        o = inside(1.0)
        o[ax] = mid[ax] + sgn * (half[ax] + rng.uniform(0.01, 1.0) * half.max())
        d = rng.normal(size=3)
        d[ax] = -sgn * abs(d[ax]) if i % 2 == 0 else sgn * abs(d[ax])
        add("outside", o, d)
    for i in range(per_class):  # the far limit inside a cell, and exactly at a crossing: T(X) = fl(fl(X - o) fl(1 / d))
        o, d = inside(0.9), rng.normal(size=3)
        k = int(np.abs(d).argmax())
        X = edge32(g, k, int(rng.integers(0, int(g["n"][k]) + 1)))
        with np.errstate(all="ignore"):
            T = F32(F32(X - F32(o[k])) * F32(F32(1) / F32(d[k])))
        add("tmax", o, d, tmax=float(T) if (i % 2 == 0 and T > 0) else float(rng.uniform(0.0, 2.0) * half.max()))
    for i in range(per_class // 2):  # a = d . d one ulp either side of 2^-40 and 2^40; origins one ulp either side of reach
        k = int(rng.integers(0, 3))
        o, d = inside(0.8), np.zeros(3)
        if i % 2 == 0:
            base = F32(2.0 ** -20) if i % 4 == 0 else F32(2.0 ** 20)
            d[k] = float([base, np.nextafter(base, F32(0)), np.nextafter(base, F32(np.inf))][(i // 4) % 3]) * rng.choice([-1.0, 1.0])
        else:
            d = rng.normal(size=3)
            sgn = rng.choice([-1.0, 1.0])
            at = F32(g["ctr"][k] + F32(sgn) * g["reach"])
            o[k] = float([at, np.nextafter(at, F32(np.inf)), np.nextafter(at, F32(-np.inf))][(i // 4) % 3])
        add("ulp", o, d)
    bad = [((np.nan, 0, 0), (0, 0, 1)), ((np.inf, 0, 0), (0, 0, 1)), ((0, -np.inf, 0), (0, 1, 0)), (mid, (np.nan, 0, 1)), (mid, (0, np.inf, 0)), (mid, (0, 0, 0)),
           (mid, (-0.0, 0.0, -0.0)), (mid, (1e-8, 0, 0)), (mid, (0, 3e6, 0)), (mid + np.array([0, 0, 3.5 * reach / 3.0]), (0, 0, -1)), (mid, (3e38, 3e38, 0))]
    for i in range(4):
        for o, d in bad:  # not walkable: with a far limit that lets them live, and negative / NaN ones that do not
            add("broken", o, d, tmax=[np.inf, 1.0, -1.0, np.nan][i])
    for i in range(per_class // 4):  # walkable rays that cannot report anything: negative and NaN far limits, zero
        j = int(rng.integers(0, len(s)))
        o = inside(1.0)
        add("broken", o, (np.where(np.isfinite(s[j, :3]), s[j, :3], mid) - o) / half.max() + 1e-3, tmax=[-1.0, np.nan, -0.0, 0.0, 1e-42][i % 5])
    for _ in range(per_class):  # aimed at spheres from in and about the box
        j = int(rng.choice(np.flatnonzero(ok))) if ok.any() else 0
        o = inside(1.1)
        # (a sphere too small for float64 to call at this distance is passed at a clear distance instead)
        off = abs(s[j, 3]) * 0.7 if abs(s[j, 3]) >= 0.01 * half.max() else 0.05 * half.max()
        add("random", o, (s[j, :3] + rng.normal(size=3) * off - o) / half.max() * rng.uniform(0.2, 3.0))
    perm = rng.permutation(len(rows))  # a wave holds rays of every class side by side
    return np.stack(rows)[perm], np.array(cls)[perm], np.array(eps_)[perm], np.array(far_)[perm]


def library_rays(rays):
    """The same rays with the skip word a creation index of the library's scenes (gidx_of)."""
    out = np.array(rays, F32, copy=True)
    out[:, 7] = gidx_of(np.ascontiguousarray(rays[:, 7]).view(np.uint32)).view(F32)
    return out


# ---------------------------------------------------------------------------------------------- segments

SEG_CLASSES = ("grazing", "ending", "own", "point", "short", "long", "beyond", "random")


def segments_of(name, geom, g, per_class=128, graze_spheres=48):
    """(P, L float32 (n, 3), own_pos (n,) sphere index or NONE, cls (n,))."""
    rng = np.random.default_rng(sum(map(ord, name)) + 2402)
    s = np.asarray(geom, np.float64)
    ok = np.isfinite(s).all(1)
    ctr, reach = g["ctr"].astype(np.float64), float(g["reach"])
    half = np.array([(edges(g, k)[-1] - edges(g, k)[0]) / 2 for k in range(3)])
    mid = np.array([(edges(g, k)[-1] + edges(g, k)[0]) / 2 for k in range(3)])
    P_, L_, own_, cls = [], [], [], []

    def add(c, p, l, own=NONE):
        P_.append(np.asarray(p, np.float64))
        L_.append(np.asarray(l, np.float64))
        own_.append(own)
        cls.append(SEG_CLASSES.index(c))

    idx = np.flatnonzero(ok & (np.abs(s[:, 3]) > 0))
    pick = idx if len(idx) <= graze_spheres else rng.choice(idx, graze_spheres, replace=False)
    for j in pick:
        c, r = s[j, :3], abs(s[j, 3])
        for m, u in enumerate(FACES + CORNERS):
            e = EPS[int(rng.integers(0, 4))] * (1.0 if rng.random() < 0.4 else -1.0)
            w = _perp(rng, u)
            p = c + r * (1.0 + e) * u
            back = 0.98 * _rim(g, p, w) if m % 2 == j % 2 else 2.0 * r
            if m % 3 == 0:  # past the tangent point
                add("grazing", p - back * w, p + rng.uniform(0.5, 3.0) * r * w)
            elif m % 3 == 1:  # ending inside the outermost cell of the sphere's box: just short of, at, or just past the tangent point
                add("ending", p - back * w, p + rng.uniform(-0.05, 0.05) * r * w)
            else:  # through the sphere, which is the segment's own
                q = c + r * rng.uniform(0.0, 0.9) * u
                add("own", q - back * w, q + rng.uniform(0.5, 3.0) * r * w, own=int(j))
    for i in range(per_class):
        p = mid + rng.uniform(-1.0, 1.0, 3) * half
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if i % 4 == 0:
            add("point", p, p)  # the light at the point
        elif i % 4 == 1:
            # one ulp of one coordinate: where the coordinates are below 8 a length^2 of at most 2^-42, below the limit 2^-40
            k = int(rng.integers(0, 3))
            q = p.astype(F32)
            q[k] = np.nextafter(q[k], F32(np.inf))
            add("short", p, q)
        elif i % 4 == 2:
            add("long", p, p + v * 2.0 ** 20.5)  # length^2 2^41, above 2^40
        else:
            q = ctr + rng.uniform(1.02, 1.5) * reach * np.sign(v + 1e-9)  # beyond reach on every axis
            add("beyond", q, p)
    for _ in range(per_class):
        add("random", mid + rng.uniform(-1.4, 1.4, 3) * half, mid + rng.uniform(-1.4, 1.4, 3) * half)
    perm = rng.permutation(len(P_))
    return (np.stack(P_).astype(F32)[perm], np.stack(L_).astype(F32)[perm], np.array(own_, np.uint32)[perm], np.array(cls)[perm])


def segment_rays(P, L):
    """The walk's view of the segments: o = P, d = fp32 L - P, tmax = 1."""
    rays = np.zeros((len(P), 8), F32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = P, 1.0, (np.asarray(L, F32) - np.asarray(P, F32))
    rays[:, 7] = np.array([NONE], np.uint32).view(F32)[0]
    return rays
