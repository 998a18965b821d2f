"""The culling geometry of rtx_cull.hpp -- tile_plane, tile_culls, tile_culls_moving (with `inside`), plane_invisible -- run on the
GPU on chosen (rectangle, sphere) and (rectangle, plane) pairs (tests/gpu_checks/cull_check.hip) and held to two yardsticks:

* the kernel's own test: the production sphere_reject / sphere_hit and plane_hit over every pixel of the rectangle, each primary
  ray built as the trace builds it (what a culled object must not be able to win), and
* float64: pixel half-lines, plane normals and margins worked out in numpy from the float32 inputs, with no device code.

Assertions (none has exceptions):
  S1  a sphere the caller's rule culls (cc > 0 && tile_culls) is hit by no pixel of the rectangle;
  S2  a sphere some pixel half-line passes within r (1 - 1e-5) of, in float64, at t > 0, is not culled;
  F   the margins are the documented ones: sqrt(r^2 (1 + kappa) + kappa |O|^2) + delta |O| to 1e-6 relative; the moving margin in
      [static, static (1 + 1e-5)] at theta = delta = 0 and equal to rtx_plan.hpp's formula to 1e-5 relative otherwise;
  T   a sphere whose centre lies beyond some float64 plane by more than margin (1 + 1e-4) + 2e-6 |O| is culled;
  M   lists built with a budget (theta, delta) hold for later cameras that rtxplan::cell_motion admits to that budget: a pair
      culled by tile_culls_moving (cc > 0, !inside) is hit by no pixel from any of them, and `inside` is set whenever one of them
      lies within r (1 - 1e-5) of the centre;
  D   degenerate camera matrices (singular, overflowing, flat, NaN) never cull a sphere and -- flat apart -- never hide a plane;
      the sheared matrix, a valid if thin camera, refuses its cancelled edge and is held to S1 (static and moving margins) and to
      P's first rule;
  P   plane_invisible: invisible => no pixel's plane_hit hits; a float64-clear hit => not invisible; a footprint that misses the
      bounds by more than twice the documented allowance, q > 2e-3 => invisible; one that misses them by less than 0.95 of it on
      every side => kept (the allowance is the documented one: the one assertion that holds `rel`).
Every test first asserts that its inputs are not vacuous, by the float64 rule alone.

The rules the cases follow, and their reasons:
  * Spheres are pushed beyond a plane by s margins and by r + s margins, s in 0.5 .. 10: the margin contains r, so for r > 0 only
    the first straddles the boundary, and the second gives the clearly culled bulk.  The float32 rounding of a centre can move it
    by more than the margin, so every sphere is classified from its rounded values; s only generates.
  * M: later cameras are rotated by the angle whose chord is 0.999 theta -- except at theta = 1e-3.  cell_motion adds 0.01 % +
    2 eps + 1e-6 to the chord it measures, so 0.999e-3 is over that budget by the host's own rule; there the rotations use the
    largest chord the rule admits (0.9984 theta).  At the budget (0, 0) the rotations and mixes are the built camera itself.
  * D, the sheared matrix (column 1 nearly parallel to column 2): its column edges give sound planes, so spheres ARE culled, and
    its rays are real, so a plane CAN be out of their sight.  It is held to soundness -- what is culled, with the static or the
    moving margin, is hit by no pixel; an invisible plane is hit by no pixel -- and its cancelled row edge to the zero normal.
  * D, the flat matrix (no third column): the edge basis refuses it, so no sphere is culled; its rays are real (all in one plane)
    and plane_invisible reads them from the matrix, so a plane they all face away from is invisible, rightly; for planes it is
    held to "invisible => no pixel hits".
  * A hit is one the trace would take: the test reports it and t < 99999999 (a NaN ray passes every rejection of sphere_hit
    and plane_hit with t = NaN, and wins no pixel).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

# the float64 yardsticks (shared with tests/sched_cases.py)
from cull_geometry import (DELTA, F32, KAPPA, ONE_KAPPA, Cam, Pyramid, axis_rotation, camera, later_cameras, margin64, min_ray_distance,  # noqa: F401
                           moved_spheres, moving_margin64, rotation, unit)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

FRAMES = ((64, 48), (1920, 1080), (7680, 4320))
POSES = ("default", "rolled", "general", "far")
BUDGETS = ((0.0, 0.0), (1.0e-3, 0.05), (0.02, 1.0), (0.1, 10.0))


# ---------------------------------------------------------------------------------------------- the library

class Lib:
    """ctypes face of libcull_check.so.  Arrays in, arrays out; a non-zero status is an error of the test's plumbing."""

    def __init__(self, so):
        self.so = so
        for fn in (so.rtx_check_tile_planes, so.rtx_check_cull_spheres, so.rtx_check_rect_hits, so.rtx_check_cull_planes, so.rtx_check_cell_motion):
            fn.restype = C.c_int

    @staticmethod
    def _p(a):
        return C.c_void_p(a.ctypes.data)

    def tile_planes(self, cam, rects):
        out = np.zeros((len(rects), 5, 3), F32)
        rc = self.so.rtx_check_tile_planes(self._p(cam.packed), C.c_uint(cam.W), C.c_uint(cam.H), self._p(rects), C.c_uint(len(rects)), self._p(out))
        assert rc == 0, rc
        return out

    def cull_spheres(self, cam, rects, sph, pairs, theta=0.0, delta=0.0):
        n = len(pairs)
        flags, margins, rec = np.zeros(n, np.uint32), np.zeros((n, 2), F32), np.zeros((n, 4), F32)
        rc = self.so.rtx_check_cull_spheres(self._p(cam.packed), C.c_uint(cam.W), C.c_uint(cam.H), self._p(rects), C.c_uint(len(rects)), self._p(sph),
                                            C.c_uint(len(sph)), self._p(pairs), C.c_uint(n), C.c_float(theta), C.c_float(delta), self._p(flags),
                                            self._p(margins), self._p(rec))
        assert rc == 0, rc
        return flags, margins, rec

    def rect_hits(self, cam, rects, sph, pairs):
        hit = np.zeros(len(pairs), np.uint32)
        if len(pairs) == 0:
            return hit
        rc = self.so.rtx_check_rect_hits(self._p(cam.packed), C.c_uint(cam.W), C.c_uint(cam.H), self._p(rects), C.c_uint(len(rects)), self._p(sph),
                                         C.c_uint(len(sph)), self._p(pairs), C.c_uint(len(pairs)), self._p(hit))
        assert rc == 0, rc
        return hit

    def cull_planes(self, cam, rects, planes, pairs):
        out = np.zeros(len(pairs), np.uint32)
        rc = self.so.rtx_check_cull_planes(self._p(cam.packed), C.c_uint(cam.W), C.c_uint(cam.H), self._p(rects), C.c_uint(len(rects)), self._p(planes),
                                           C.c_uint(len(planes)), self._p(pairs), C.c_uint(len(pairs)), self._p(out))
        assert rc == 0, rc
        return out

    def cell_motion(self, built, now, drift_built=0.0, drift_now=0.0):
        th, de = C.c_float(0), C.c_float(0)
        rc = self.so.rtx_check_cell_motion(self._p(built.packed), self._p(now.packed), C.c_uint(built.W), C.c_uint(built.H), C.c_double(drift_built),
                                           C.c_double(drift_now), C.byref(th), C.byref(de))
        assert rc == 0, rc
        return th.value, de.value


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    path = os.path.join(HERE, "gpu_checks", "libcull_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    return Lib(C.CDLL(path))


# ---------------------------------------------------------------------------------------------- cameras and rectangles

def rectangles(W, H):
    """(col0, row0, w, h) rows, without repeats: 16 x 16 in each corner, 64 x 64 at the centre, one 128 x 128, the whole of the
    small frame, and in the 8K frame the thin strips along its four sides."""
    r = []

    def add(c0, r0, w, h):
        w, h = min(w, W), min(h, H)
        c0, r0 = max(0, min(c0, W - w)), max(0, min(r0, H - h))
        if (c0, r0, w, h) not in r:
            r.append((c0, r0, w, h))

    for c0 in (0, W - 16):
        for r0 in (0, H - 16):
            add(c0, r0, 16, 16)
    add(W // 2 - 32, H // 2 - 32, 64, 64)
    if W >= 1920:
        add(W // 4, H // 4 * 3 - 128, 128, 128)
    if W == 64:
        add(0, 0, W, H)
    if W == 7680:
        add(0, H // 2 - 32, 4, 64)
        add(W - 4, H // 2 - 32, 4, 64)
        add(W // 2 - 32, 0, 64, 4)
        add(W // 2 - 32, H - 4, 64, 4)
    return np.array(r, np.uint32)


# ---------------------------------------------------------------------------------------------- spheres

PUSH_S = (0.5, 0.9, 0.99, 1.01, 1.1, 2.0, 10.0)
PUSH_R = (0.0, 1.0e-3, 1.0, 50.0, 1.0e4)
PUSH_D = (None, 1.0, 100.0, 1.0e4, 1.0e6)  # None: r * 1.001


def pushed(o, point_dir, D, out, r, s, literal):
    """Centre = o + D point_dir + out * push with push = s * margin (or r + s * margin, `literal`), margin taken at the centre's own
    distance (fixed point, three rounds)."""
    base = o + D * point_dir
    push = r
    for _ in range(3):
        m = margin64(r, np.linalg.norm(base + out * push - o))
        push = r + s * m if literal else s * m
    return base + out * push


def spheres_for(cam, pyr, rng):
    """The directed spheres of one rectangle: rows (x, y, z, r) in float64, and per row the plane it was aimed at (0..4 sides and
    camera plane, 5..8 the four edges of the pyramid, 9 camera cases; Case adds 10 for the non-finite spheres and 11 for the
    random bulk, which every rectangle shares)."""
    o = cam.pos
    rows, aimed = [], []
    fwd = pyr.n[4]
    for r in PUSH_R:
        for D0 in PUSH_D:
            D = r * 1.001 if D0 is None else D0
            for i, s in enumerate(PUSH_S):
                for literal in (False, True):
                    f = (0.5, 0.15, 0.85)[(i + int(literal)) % 3]
                    for k in range(4):
                        rows.append(np.append(pushed(o, pyr.edge_dir(k, f), D, -pyr.n[k], r, s, literal), r))
                        aimed.append(k)
                        # the pyramid's edge between planes k and k + 1: outward along the bisector of the two
                        out = -unit(pyr.n[k] + pyr.n[(k + 1) % 4])
                        rows.append(np.append(pushed(o, unit(pyr.corners[(k + 1) % 4]), D, out, r, s, literal), r))
                        aimed.append(5 + k)
        # behind the apex: straight back along a direction u of the pyramid (its axis, and towards each corner), as far as puts
        # the centre s margins (r + s margins) behind the camera plane -- there the side planes see it inside or barely outside.
        # (With r = 0 the margin is proportional to the distance and the ratio is fixed: the five distances then.)
        (x0, x1), (y0, y1) = pyr.cx, pyr.cy
        for j, (fx, fy) in enumerate(((0.5, 0.5), (0.1, 0.1), (0.9, 0.1), (0.9, 0.9), (0.1, 0.9))):
            u = unit(cam.dirs(x0 + fx * (x1 - x0), y0 + fy * (y1 - y0)))
            for s in PUSH_S:
                for literal in (False, True):
                    L = (0.5, 1.0, 100.0, 1.0e4, 1.0e6)[j]
                    if r > 0.0:
                        L = r
                        for _ in range(40):
                            L = min(((r if literal else 0.0) + s * margin64(r, L)) / (fwd @ u), 1.0e9 * r)
                    rows.append(np.append(o - u * L, r))
                    aimed.append(4)
    # the camera inside the sphere, on it, one ulp outside it, and a little further out (within the motion budgets of M):
    # centres in front, behind and beside the rectangle
    for r in (1.0, 50.0, 1.0e4):
        for u in (pyr.axis, -pyr.axis, unit(np.cross(pyr.axis, pyr.n[0])), -pyr.n[1]):
            for f in (0.0, 0.5, 0.999, 1.0, 1.0 + 1.2e-7, 1.0 + 1.0e-5, 1.002, 1.03):
                rows.append(np.append(o + u * (r * f), r))
                aimed.append(9)
    rows, aimed = np.array(rows), np.array(aimed)
    return rows, aimed


def nonfinite_spheres(cam):
    o, n, i = cam.pos, float("nan"), float("inf")
    return np.array([[n, 0, 0, 1], [0, n, 5, 1], [o[0], o[1], o[2] + 5, n], [i, 0, 0, 1], [0, -i, 0, 1], [o[0] + 3, o[1], o[2] + 4, i], [i, i, i, i],
                     [o[0], o[1] + 2, o[2], -i]], np.float64)


def random_spheres(cam, rng, n=300):
    """The bulk: centres uniform in a box around the camera whose size is drawn per sphere, radii log-uniform."""
    size = 10.0 ** rng.uniform(0.0, 4.0, n)
    c = cam.pos + rng.uniform(-1.0, 1.0, (n, 3)) * size[:, None]
    r = size * 10.0 ** rng.uniform(-4.0, -0.5, n)
    return np.column_stack([c, r])


class Case:
    """One camera of one frame: its rectangles, their spheres (float32), the pairs, and the float64 view of every pair."""

    def __init__(self, W, H, pose):
        self.cam = cam = camera(W, H, pose)
        self.rects = rectangles(W, H)
        self.pyr = [Pyramid(cam, r) for r in self.rects]
        rng = np.random.default_rng(1000 * W + POSES.index(pose))
        sph, pairs, aimed = [], [], []
        shared = np.vstack([random_spheres(cam, rng), nonfinite_spheres(cam)])
        n_shared = len(shared)
        sph.append(shared)
        at = n_shared
        for ri, p in enumerate(self.pyr):
            rows, aim = spheres_for(cam, p, rng)
            sph.append(rows)
            idx = np.concatenate([np.arange(n_shared), at + np.arange(len(rows))])
            pairs.append(np.column_stack([np.full(len(idx), ri), idx]))
            aimed.append(np.concatenate([np.full(n_shared, 11), aim]))
            aimed[-1][n_shared - 8:n_shared] = 10
            at += len(rows)
        with np.errstate(over="ignore", invalid="ignore"):
            self.sph = np.vstack(sph).astype(F32)
        self.pairs = np.vstack(pairs).astype(np.uint32)
        self.aimed = np.concatenate(aimed)
        self.geometry()

    def geometry(self, cam=None, sph=None):
        """float64 from the float32 inputs, per pair: otc = o - c, |O|, r, d[k] = n_k . otc (how far beyond plane k the centre
        lies), the documented margin."""
        cam = cam or self.cam
        s = (self.sph if sph is None else sph).astype(np.float64)[self.pairs[:, 1]]
        with np.errstate(over="ignore", invalid="ignore"):
            self.otc = cam.pos - s[:, :3]
            self.dist = np.sqrt((self.otc * self.otc).sum(1))
            self.r = s[:, 3]
            N = np.array([p.n for p in self.pyr])[self.pairs[:, 0]]  # (n, 5, 3)
            self.d = np.einsum("nkj,nj->nk", N, self.otc)
            self.margin = margin64(self.r, self.dist)

    def must_cull(self):
        """T's premise per pair and plane: beyond the plane by more than margin (1 + 1e-4) + 2e-6 |O|."""
        with np.errstate(invalid="ignore"):
            return self.d > (self.margin * (1.0 + 1.0e-4) + 2.0e-6 * self.dist)[:, None]

    def run(self, lib):
        if not hasattr(self, "flags"):
            self.flags, self.margins, self.rec = lib.cull_spheres(self.cam, self.rects, self.sph, self.pairs)
            self.hit = lib.rect_hits(self.cam, self.rects, self.sph, self.pairs)
        return self

    @property
    def culled(self):  # the caller's rule (stage_chunk): cc > 0 && tile_culls
        return (self.flags & 9) == 9


@functools.lru_cache(maxsize=None)
def case(W, H, pose):
    return Case(W, H, pose)


CASES = [(W, H, pose) for (W, H) in FRAMES for pose in POSES]
IDS = ["%dx%d-%s" % c for c in CASES]


def check_not_vacuous(c):
    """The counts every sphere test relies on, from the float64 rule alone: per rectangle and plane k, 20 spheres that the rule
    culls by exactly that plane; per rectangle 20 spheres beyond a plane by 0.9 .. 0.99 of the margin (and beyond no plane by
    more): kept by any sound test that is as tight as documented; and 5 with the camera inside.  Returns the mask of those
    0.9 .. 0.99 pairs."""
    must = c.must_cull()
    only = must & (must.sum(1) == 1)[:, None]
    with np.errstate(invalid="ignore"):
        frac = (c.d / c.margin[:, None]).max(1)
        just_inside = (frac >= 0.9) & (frac <= 0.99)
        cam_inside = c.dist < c.r * (1.0 - 1.0e-5)
    for ri in range(len(c.rects)):
        sel = c.pairs[:, 0] == ri
        for k in range(5):
            assert (only[sel, k]).sum() >= 20, (c.rects[ri], k, int(only[sel, k].sum()))
        assert just_inside[sel].sum() >= 20, (c.rects[ri], int(just_inside[sel].sum()))
        assert cam_inside[sel].sum() >= 5, c.rects[ri]
    return just_inside


# ---------------------------------------------------------------------------------------------- S1, S2, F, T

@pytest.mark.parametrize("W,H,pose", CASES, ids=IDS)
def test_culled_spheres_are_hit_by_no_pixel(lib, W, H, pose):
    """S1: against the kernel's own test."""
    c = case(W, H, pose).run(lib)
    check_not_vacuous(c)
    assert c.culled.sum() > 1000 and (c.hit != 0).sum() > 500 and ((c.hit != 0) & ~c.culled).sum() > 500
    bad = np.flatnonzero(c.culled & (c.hit != 0))
    print("S1 %s: %d pairs, %d culled, %d hit, %d culled and hit" % (pose, len(c.pairs), c.culled.sum(), (c.hit != 0).sum(), len(bad)))
    assert len(bad) == 0, (len(bad), [(c.rects[c.pairs[i, 0]], c.sph[c.pairs[i, 1]]) for i in bad[:5]])
    # a NaN or infinite centre or radius is never culled, by either test (every comparison with its margin is false)
    odd = c.aimed == 10
    assert odd.sum() == 8 * len(c.rects) and not np.isfinite(c.sph[c.pairs[odd, 1]]).all(1).any()
    assert not (c.flags[odd] & 3).any(), c.sph[c.pairs[odd & ((c.flags & 3) != 0), 1]]


@pytest.mark.parametrize("W,H,pose", CASES, ids=IDS)
def test_spheres_near_a_pixel_ray_in_float64_are_kept(lib, W, H, pose):
    """S2: against float64 half-lines; none of the ray-building code of the device is used."""
    c = case(W, H, pose).run(lib)
    check_not_vacuous(c)
    near = np.zeros(len(c.pairs), bool)
    s64 = c.sph.astype(np.float64)
    for ri, rect in enumerate(c.rects):
        sel = np.flatnonzero((c.pairs[:, 0] == ri) & c.culled)  # only a culled pair can fail
        near[sel] = min_ray_distance(c.cam, rect, s64[c.pairs[sel, 1], :3], s64[c.pairs[sel, 1], 3])
    bad = np.flatnonzero(near)
    print("S2 %s: %d culled pairs walked, %d of them within r (1 - 1e-5) of a pixel half-line" % (pose, c.culled.sum(), len(bad)))
    assert len(bad) == 0, (len(bad), [(c.rects[c.pairs[i, 0]], c.sph[c.pairs[i, 1]]) for i in bad[:5]])


def relative_error(got, want):
    """|got - want| / |want| where want is finite and not zero; 0 where both are the same non-finite value or both zero; inf
    otherwise."""
    got, want = got.astype(np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(got - want) / np.abs(want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(same, 0.0, np.where(np.isfinite(err), err, np.inf))


def documented_margin(c):
    """tile_culls' margin in float64 from the float32 ox, oy, oz the device formed and the float32 r."""
    o = c.rec[:, :3].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return margin64(c.r, np.sqrt((o * o).sum(1))), np.sqrt((o * o).sum(1))


@pytest.mark.parametrize("W,H,pose", CASES, ids=IDS)
def test_margins_are_the_documented_ones(lib, W, H, pose):
    """F.  1e-6 relative allows eight fp32 roundings and two 1-ulp hardware square roots."""
    c = case(W, H, pose).run(lib)
    want, dist = documented_margin(c)
    # float32 overflows where float64 does not (|O|^2 or r^2 past 3.4e38): the device's margin is then +inf, which never culls
    with np.errstate(over="ignore", invalid="ignore"):
        overflow = np.isfinite(want) & ((dist * dist > 3.0e38) | (c.r * c.r > 3.0e38))
    want = np.where(overflow, np.inf, want)
    err = relative_error(c.margins[:, 0], want)
    print("F %s: worst relative error of the static margin %.3e over %d pairs" % (pose, err.max(), len(err)))
    assert np.isfinite(want).sum() > 1000
    assert err.max() <= 1.0e-6, (int((err > 1.0e-6).sum()), err.max(), c.sph[c.pairs[err.argmax(), 1]])
    # theta = delta = 0: the moving margin within [static, static (1 + 1e-5)]
    fin = np.isfinite(c.margins[:, 0])
    st, mv = c.margins[fin, 0].astype(np.float64), c.margins[fin, 1].astype(np.float64)
    print("F %s: moving / static margin at zero budget in [%.9f, %.9f]" % (pose, (mv[st > 0] / st[st > 0]).min(), (mv[st > 0] / st[st > 0]).max()))
    assert ((mv >= st) & (mv <= st * (1.0 + 1.0e-5))).all(), int((~((mv >= st) & (mv <= st * (1.0 + 1.0e-5)))).sum())
    assert (~np.isfinite(c.margins[~fin, 1]) | np.isnan(c.margins[~fin, 0])).all()
    for theta, delta in BUDGETS[1:]:
        _, m2, _ = lib.cull_spheres(c.cam, c.rects, c.sph, c.pairs, theta, delta)
        t32, d32 = float(F32(theta)), float(F32(delta))
        with np.errstate(over="ignore", invalid="ignore"):
            want2 = np.where(overflow, np.inf, moving_margin64(c.r, dist, t32, d32))
        err2 = relative_error(m2[:, 1], want2)
        print("F %s: budget (%g, %g): worst relative error of the moving margin %.3e" % (pose, theta, delta, err2.max()))
        assert err2.max() <= 1.0e-5, (int((err2 > 1.0e-5).sum()), theta, delta, err2.max(), c.sph[c.pairs[err2.argmax(), 1]])


@pytest.mark.parametrize("W,H,pose", CASES, ids=IDS)
def test_spheres_beyond_a_float64_plane_are_culled(lib, W, H, pose):
    """T: the code culls what its own derivation allows.  The planes are cross products of the corner directions in float64."""
    c = case(W, H, pose).run(lib)
    just_inside = check_not_vacuous(c)
    must = c.must_cull().any(1)
    assert must.sum() > 1000
    # the smallest slack at which the device still culled, and the largest at which it did not (figures, before the assertion)
    with np.errstate(invalid="ignore"):
        slack = ((c.d - 2.0e-6 * c.dist[:, None]) / c.margin[:, None]).max(1)
    fin = np.isfinite(slack)
    raw = (c.flags & 1) != 0
    print("T %s: %d pairs must be culled; smallest (d - 2e-6 |O|) / margin among culled pairs %.7f, largest among kept pairs %.7f" %
          (pose, must.sum(), slack[fin & raw].min(), slack[fin & ~raw].max()))
    bad = np.flatnonzero(must & ~c.culled)
    assert len(bad) == 0, (len(bad), [(c.rects[c.pairs[i, 0]], c.sph[c.pairs[i, 1]], c.d[i], c.margin[i]) for i in bad[:5]])
    # ... and no sooner: a centre beyond its farthest plane by 0.9 .. 0.99 of the margin is kept.  The remaining 1 % of the margin
    # is at least 1.4e-5 |O| (margin >= (sqrt(kappa) + delta) |O|), seven times the 2e-6 |O| that the device's planes and its
    # evaluation may differ from float64 by, and a thousand times the margin's own error (F).
    early = np.flatnonzero(just_inside & raw)
    assert len(early) == 0, (len(early), [(c.rects[c.pairs[i, 0]], c.sph[c.pairs[i, 1]], c.d[i], c.margin[i]) for i in early[:5]])


# ---------------------------------------------------------------------------------------------- M

M_CASES = [(64, 48, "general"), (1920, 1080, "default"), (7680, 4320, "rolled")]


@pytest.mark.parametrize("W,H,pose", M_CASES, ids=["%dx%d-%s" % c for c in M_CASES])
def test_lists_built_with_a_budget_hold_for_later_cameras(lib, W, H, pose):
    """M."""
    c = case(W, H, pose).run(lib)
    rng = np.random.default_rng(7 + W)
    normals = c.pyr[len(c.pyr) // 2].n
    for theta, delta in BUDGETS:
        flags, _, _ = lib.cull_spheres(c.cam, c.rects, c.sph, c.pairs, theta, delta)
        inside = (flags & 4) != 0
        culled = ((flags & 2) != 0) & ((flags & 8) != 0) & ~inside  # rtx_bin_cells' rule
        sel = np.flatnonzero(culled)
        assert len(sel) > 500, (theta, delta, len(sel))  # every class below walks these pairs
        seen = set()
        n_close = 0
        for kind, now, drift in later_cameras(c.cam, normals, theta, delta, rng):
            used_theta, used_delta = lib.cell_motion(c.cam, now, 0.0, drift)
            assert used_theta <= float(F32(theta)) and used_delta <= float(F32(delta)), (kind, theta, delta, used_theta, used_delta)
            sph = moved_spheres(c.sph, drift, rng)
            hit = lib.rect_hits(now, c.rects, sph, c.pairs[sel])
            assert (hit != 0).sum() == 0, (int((hit != 0).sum()), kind, theta, delta, [(c.rects[c.pairs[i, 0]], c.sph[c.pairs[i, 1]]) for i in sel[hit != 0][:5]])
            # a later camera within r (1 - 1e-5) of a (moved) centre: `inside` was set
            with np.errstate(invalid="ignore", over="ignore"):
                m64 = sph.astype(np.float64)
                close = np.linalg.norm(m64[:, :3] - now.pos, axis=1) < m64[:, 3] * (1.0 - 1.0e-5)
            close_pair = close[c.pairs[:, 1]]
            n_close += int((close_pair & ~((c.dist < c.r))).sum())
            assert inside[close_pair].all(), (int((close_pair & ~inside).sum()), kind, theta, delta, c.sph[c.pairs[np.flatnonzero(close_pair & ~inside)[:5], 1]])
            seen.add(kind)
        # (at the budget (0, 0) all three classes are the built camera itself -- chord and step are zero -- so there the pairs
        # are walked 19 times from one pose: the classes differ from the second budget on)
        assert seen == {"rotation", "translation", "mix"}
        print("M %s: budget (%g, %g): %d culled pairs walked from %d later cameras; %d (pair, camera) cases with only the later camera inside" %
              (pose, theta, delta, len(sel), 19, n_close))
        if delta > 0.0:
            assert n_close > 0


# ---------------------------------------------------------------------------------------------- D

def degenerate_cameras():
    """tests/host/test_plan.cpp, test_edge_basis: singular, overflowing, flat -- and NaN in the matrix."""
    W, H = 640, 360
    z = np.zeros((3, 3))
    flat = rotation(0.1, 0.2, 0.3)
    flat[:, 2] = 0.0
    nan1 = np.zeros((3, 3))
    nan1[0, 0] = float("nan")
    nan2 = rotation(0.1, 0.2, 0.3)
    nan2[1, 2] = float("nan")
    return [("singular", Cam(W, H, z, (0, 0, 0), 1.0, 1.0)), ("overflowing", Cam(W, H, rotation(0.1, 0.2, 0.3), (0, 0, 0), 3.0e38, 3.0e38)),
            ("flat", Cam(W, H, flat, (0, 0, 0), 1.0, 1.0)), ("nan", Cam(W, H, nan1, (0, 0, 0), 1.0, 1.0)), ("nan-column", Cam(W, H, nan2, (1, 2, 3), 1.0, 1.0))]


def sheared_camera():
    sh = rotation(0.0, 0.0, 0.0)
    sh[0, 1] = sh[0, 2]
    sh[1, 1] = sh[1, 2] + 1.0e-3
    sh[2, 1] = sh[2, 2]
    return Cam(640, 360, sh, (0, 0, 0), 1.0, 1.0)


def bulk_for(cam, rng):
    rects = np.array([(0, 0, 16, 16), (624, 344, 16, 16), (288, 148, 64, 64), (0, 0, 128, 128), (0, 296, 64, 64)], np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        sph = np.vstack([random_spheres(cam, rng, 400), nonfinite_spheres(cam)]).astype(F32)
    pairs = np.array([(r, s) for r in range(len(rects)) for s in range(len(sph))], np.uint32)
    planes = []
    for y in (-1.0, -50.0, 3.0):
        for ny in (1.0, -1.0):
            for width in (1.0, 1.0e3):
                planes.append([0.0, y, 0.0, width, 0.0, ny, 0.0, width])   # num = -y ny: both signs
    planes.append([5.0, -2.0, 7.0, 10.0, 0.3, 0.8, -0.5, 4.0])
    planes = np.array(planes, F32)
    ppairs = np.array([(r, p) for r in range(len(rects)) for p in range(len(planes))], np.uint32)
    return rects, sph, pairs, planes, ppairs


def test_degenerate_cameras_never_cull(lib):
    """D.  A plane with num >= 0 is invisible whatever the camera (no ray can reach its front): those pairs are left out."""
    rng = np.random.default_rng(5)
    for name, cam in degenerate_cameras():
        rects, sph, pairs, planes, ppairs = bulk_for(cam, rng)
        n = lib.tile_planes(cam, rects)
        assert (n == 0.0).all(), (name, n)
        for theta, delta in ((0.0, 0.0), (0.02, 1.0)):
            flags, _, _ = lib.cull_spheres(cam, rects, sph, pairs, theta, delta)
            assert (flags & 3).sum() == 0, (name, int(((flags & 3) != 0).sum()))
        out = lib.cull_planes(cam, rects, planes, ppairs)
        p64 = planes.astype(np.float64)[ppairs[:, 1]]
        num = ((p64[:, :3] - cam.pos) * p64[:, 4:7]).sum(1)
        assert (num < 0.0).sum() >= 20
        assert ((out & 1) * ((out >> 1) & 1)).sum() == 0, name  # invisible => no pixel hits, whatever the matrix
        if name != "flat":
            # (the flat matrix has real rays, all in one plane, and plane_invisible reads them from the matrix, not from the
            # edge basis: a plane they all face away from IS invisible.  It is held to the line above.)
            assert ((out & 1)[num < 0.0] == 0).all(), (name, planes[ppairs[(num < 0.0) & ((out & 1) != 0), 1]][:3])


def test_sheared_camera_refuses_its_cancelled_edge_and_is_sound_elsewhere(lib):
    """D, the sheared matrix of test_edge_basis: the row edge at cy = -1 / e2, where t P + Q cancels, gets the zero normal; the
    other planes are planes of a valid if thin camera (its rays fan out in x, within 1e-3 of the plane y = 0), and what they cull,
    with the static margin or with a moving one, is hit by no pixel.  plane_invisible reads the same real rays from the matrix:
    it may hide a plane, and a plane it hides is hit by no pixel."""
    cam = sheared_camera()
    rng = np.random.default_rng(6)
    rects, sph, _, planes, _ = bulk_for(cam, rng)
    rects = np.vstack([rects, np.array([(100, 296, 64, 64)], np.uint32)])  # bottom edge: row 360, cy = -1 + 1/360
    # the random bulk mostly misses a fan this thin: 200 more spheres in its sheet, in front of the camera
    z = 10.0 ** rng.uniform(0.0, 2.0, 200)
    sheet = np.column_stack([z * rng.uniform(-0.7, 0.7, 200), z * rng.uniform(-0.02, 0.02, 200), z, z * rng.uniform(0.005, 0.05, 200)])
    sph = np.vstack([sph, sheet.astype(F32)])
    pairs =np.array([(r, i) for r in range(len(rects)) for i in range(len(sph))], np.uint32)
    n = lib.tile_planes(cam, rects)
    assert (n[-1, 2] == 0.0).all() and (n[4, 2] == 0.0).all()      # the cancelled row edge
    assert np.abs(n[:, 1]).max() > 0.5 and np.abs(n[:, 3]).max() > 0.5  # column edges are kept
    hit = lib.rect_hits(cam, rects, sph, pairs)
    print("D sheared: %d pairs, %d hit by a pixel" % (len(pairs), (hit != 0).sum()))
    assert (hit != 0).sum() > 20
    for theta, delta in ((0.0, 0.0), (0.02, 1.0)):
        flags, _, _ = lib.cull_spheres(cam, rects, sph, pairs, theta, delta)
        culled = (flags & 9) == 9                                          # stage_chunk's rule
        culled_moving = ((flags & 14) == 10)                               # rtx_bin_cells' rule: cc > 0, !inside, culled
        assert culled.sum() > 100 and culled_moving.sum() > 100, (theta, delta, int(culled.sum()), int(culled_moving.sum()))
        assert (culled & (hit != 0)).sum() == 0, (theta, delta)
        assert (culled_moving & (hit != 0)).sum() == 0, (theta, delta)
    # planes: the horizontal ones of bulk_for, which the fan grazes, and walls across it, in its way and beside it
    walls = [[x, 0.0, z, 4.0, 0.0, 0.0, nz, 4.0] for x in (0.0, 3.0, -3.0, 30.0, -30.0) for z, nz in ((5.0, -1.0), (5.0, 1.0), (-5.0, 1.0))]
    planes = np.vstack([planes, np.array(walls, F32)])
    ppairs = np.array([(r, i) for r in range(len(rects)) for i in range(len(planes))], np.uint32)
    out = lib.cull_planes(cam, rects, planes, ppairs)
    invisible, plane_hit = (out & 1) != 0, (out & 2) != 0
    p64 = planes.astype(np.float64)[ppairs[:, 1]]
    num = ((p64[:, :3] - cam.pos) * p64[:, 4:7]).sum(1)
    assert (num < 0.0).sum() >= 20 and plane_hit.sum() >= 3 and (invisible & (num < 0.0)).sum() >= 3, \
        (int((num < 0.0).sum()), int(plane_hit.sum()), int((invisible & (num < 0.0)).sum()))
    assert (invisible & plane_hit).sum() == 0, planes[ppairs[invisible & plane_hit, 1]][:3]


# ---------------------------------------------------------------------------------------------- P: plane_invisible

P_CASES = [(64, 48, "general"), (1920, 1080, "default"), (1920, 1080, "rolled"), (7680, 4320, "default"), (7680, 4320, "far")]
P_S = (0.5, 0.9, 1.1, 2.5, 5.0, 10.0)


def footprint(cam, pyr, p, n):
    """float64, from float32 plane values: corner w . n / |w||n|, q, the corner hit points' bounding interval in x and z, the
    largest corner offsets, and the documented allowance (2e-6 / q + 1e-5)(|o| + span) per axis."""
    w = pyr.corners
    wn = w @ n
    cosines = wn / (np.linalg.norm(w, axis=1) * np.linalg.norm(n))
    num = (p - cam.pos) @ n
    q = np.abs(wn).min() / (np.linalg.norm(w, axis=1).max() * np.linalg.norm(n))
    with np.errstate(divide="ignore", invalid="ignore"):
        off = w * (num / wn)[:, None]
    hp = cam.pos + off
    rel = 2.0e-6 / q + 1.0e-5
    ex = rel * (abs(cam.pos[0]) + np.abs(off[:, 0]).max())
    ez = rel * (abs(cam.pos[2]) + np.abs(off[:, 2]).max())
    return dict(cos=cosines, num=num, q=q, lo=(hp[:, 0].min(), hp[:, 2].min()), hi=(hp[:, 0].max(), hp[:, 2].max()), e=(ex, ez))


def plane_row(p0, n, xlo, xhi, zlo, zhi):
    """A plane through p0 with normal n (n.y != 0) whose bounds are [xlo, xhi] x [zlo, zhi]: px py pz width nx ny nz height."""
    px, pz = 0.5 * (xlo + xhi), 0.5 * (zlo + zhi)
    py = p0[1] - (n[0] * (px - p0[0]) + n[2] * (pz - p0[2])) / n[1]
    return [px, py, pz, xhi - xlo, n[0], n[1], n[2], zhi - zlo]


def planes_for(cam, pyr):
    """The planes of one rectangle, rows of eight, and per row (kind, side): kind 0 a bounded plane whose bounds miss the
    footprint on `side` (0 x below, 1 x above, 2 z below, 3 z above) by s allowances, 1 bounds that overlap the footprint on that
    side, 2 the camera on the plane or behind it, 3 facing away, 4 mixed signs, 5 grazing."""
    o, axis = cam.pos, pyr.axis
    rows, kinds = [], []
    up = np.array([0.0, 1.0 if axis[1] <= 0.0 else -1.0, 0.0])
    normals = [unit(-axis + 0.5 * up), unit(-0.3 * axis + up)]
    if (pyr.corners @ up < -0.05 * np.linalg.norm(pyr.corners, axis=1)).all():
        normals.append(up)  # a floor or a ceiling the whole rectangle looks at
    for n in normals:
        n = n.astype(F32).astype(np.float64)
        for h in (3.0, 400.0):
            p0 = o + axis * h
            f = footprint(cam, pyr, p0, n)
            if not ((f["cos"] < -1.0e-2).all() and f["num"] < 0.0):
                continue
            size = (max(f["hi"][0] - f["lo"][0], 1e-3 * h), max(f["hi"][1] - f["lo"][1], 1e-3 * h))
            wide = [(f["lo"][a] - 2.0 * size[a] - 1.0, f["hi"][a] + 2.0 * size[a] + 1.0) for a in (0, 1)]
            for side in range(4):
                a, above = side // 2, side % 2
                for s in P_S + (-1.0, -2.0):
                    # s > 0: the near bound s allowances away from the footprint; s < 0: inside it, at 0.3 or 0.6 of its size
                    gap = s * f["e"][a] if s > 0 else s * 0.3 * size[a]
                    if above:
                        lo = f["hi"][a] + gap
                        b = (lo, lo + size[a] + 1.0)
                    else:
                        hi = f["lo"][a] - gap
                        b = (hi - size[a] - 1.0, hi)
                    bx, bz = (b, wide[1]) if a == 0 else (wide[0], b)
                    rows.append(plane_row(p0, n, bx[0], bx[1], bz[0], bz[1]))
                    kinds.append((0 if s > 0 else 1, side))
            # the camera on the plane, and behind it (num >= 0)
            rows.append([o[0], o[1], o[2], wide[0][1] - wide[0][0], n[0], n[1], n[2], wide[1][1] - wide[1][0]])  # (exactly: num = 0)
            kinds.append((2, 0))
            rows.append(plane_row(o - axis * h, n, wide[0][0], wide[0][1], wide[1][0], wide[1][1]))
            kinds.append((2, 1))
            # facing away at all corners: the same plane seen from its back, in front of the camera
            rows.append(plane_row(p0, -n, wide[0][0], wide[0][1], wide[1][0], wide[1][1]))
            kinds.append((3, 0))
    # mixed signs: a plane that holds the rectangle's axis (the corners lie on both sides of it), num < 0
    side_dir = unit(np.cross(axis, up + 0.1 * axis))
    nm = unit(np.cross(axis, side_dir))
    if abs(nm[1]) > 0.2:
        p0 = o - nm * 2.0
        rows.append(plane_row(p0, nm, p0[0] - 500.0, p0[0] + 500.0, p0[2] - 500.0, p0[2] + 500.0))
        kinds.append((4, 0))
    # grazing: the rectangle's rays nearly in the plane, q on both sides of 1e-3; bounds far away from the footprint
    for g in (3.0e-4, 7.0e-4, 1.5e-3, 4.0e-3):
        lat = unit(up - (up @ axis) * axis)
        n = unit(lat - g * axis - max(0.0, -(pyr.corners @ lat / np.linalg.norm(pyr.corners, axis=1)).min()) * axis)
        n = n.astype(F32).astype(np.float64)
        if abs(n[1]) < 0.2:
            continue
        p0 = o + axis * 50.0
        f = footprint(cam, pyr, p0, n)
        if not ((f["cos"] < 0.0).all() and f["num"] < 0.0 and np.isfinite(f["hi"][0])):
            continue
        xhi = f["lo"][0] - 10.0 * f["e"][0] - 1.0
        rows.append(plane_row(p0, n, xhi - 10.0, xhi, f["lo"][1] - 1.0e3, f["hi"][1] + 1.0e3))
        kinds.append((5, 0))
    return rows, kinds


def pixel_plane_hits64(cam, rect, p, n, width, height):
    """Does some pixel of the rectangle hit the bounded plane CLEARLY, in float64: dn < -1e-3 |w||n|, t > 0, and the hit point
    inside the bounds by more than 1e-4 of their size."""
    w = cam.pixel_dirs(rect)
    dn = w @ n
    facing = dn < -1.0e-3 * np.linalg.norm(w, axis=1) * np.linalg.norm(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((p - cam.pos) @ n) / dn
    hp = cam.pos + w * t[:, None]
    inx = (hp[:, 0] > p[0] - 0.5 * width + 1.0e-4 * width) & (hp[:, 0] < p[0] + 0.5 * width - 1.0e-4 * width)
    inz = (hp[:, 2] > p[2] - 0.5 * height + 1.0e-4 * height) & (hp[:, 2] < p[2] + 0.5 * height - 1.0e-4 * height)
    return bool((facing & (t > 0.0) & inx & inz).any())


@pytest.mark.parametrize("W,H,pose", P_CASES, ids=["%dx%d-%s" % c for c in P_CASES])
def test_invisible_planes_are_hit_by_no_pixel_and_clear_misses_are_invisible(lib, W, H, pose):
    """P."""
    cam = camera(W, H, pose)
    rects = rectangles(W, H)
    planes, pairs, kinds = [], [], []
    for ri, rect in enumerate(rects):
        rows, k = planes_for(cam, Pyramid(cam, rect))
        pairs += [(ri, len(planes) + i) for i in range(len(rows))]
        planes += rows
        kinds += k
    planes, pairs, kinds = np.array(planes, F32), np.array(pairs, np.uint32), np.array(kinds)
    # the float64 verdicts, from the float32 values
    n_pairs = len(pairs)
    clear_hit, clear_miss, miss_side, q64 = np.zeros(n_pairs, bool), np.zeros(n_pairs, bool), np.full(n_pairs, -1), np.zeros(n_pairs)
    worst_gap = np.full(n_pairs, np.inf)
    p64 = planes.astype(np.float64)
    for i, (ri, pi) in enumerate(pairs):
        row = p64[pi]
        p, width, n, height = row[:3], row[3], row[4:7], row[7]
        pyr = Pyramid(cam, rects[ri])
        clear_hit[i] = pixel_plane_hits64(cam, rects[ri], p, n, width, height)
        f = footprint(cam, pyr, p, n)
        q64[i] = f["q"]
        if f["num"] < 0.0 and (f["cos"] < -1.0e-4).all() and f["q"] > 2.0e-3:
            bd = (p[0] - 0.5 * width, p[0] + 0.5 * width, p[2] - 0.5 * height, p[2] + 0.5 * height)
            misses = (f["hi"][0] + 2.0 * f["e"][0] < bd[0], f["lo"][0] - 2.0 * f["e"][0] > bd[1], f["hi"][1] + 2.0 * f["e"][1] < bd[2],
                      f["lo"][1] - 2.0 * f["e"][1] > bd[3])
            # side 0: the bounds lie below the footprint in x (the footprint's low end is past the bounds' high end), ...
            for side, m in zip((1, 0, 3, 2), misses):
                if m:
                    clear_miss[i], miss_side[i] = True, side
            # ... and how far the footprint misses the bounds at most, in allowances (negative: it overlaps them on every side)
            worst_gap[i] = max((bd[0] - f["hi"][0]) / f["e"][0], (f["lo"][0] - bd[1]) / f["e"][0], (bd[2] - f["hi"][1]) / f["e"][1],
                               (f["lo"][1] - bd[3]) / f["e"][1])
    for side in range(4):
        aimed = (kinds[:, 0] <= 1) & (kinds[:, 1] == side)
        assert (clear_miss & aimed & (miss_side == side)).sum() >= 10, (side, int((clear_miss & aimed).sum()))
        assert (clear_hit & aimed).sum() >= 10, (side, int((clear_hit & aimed).sum()))
    for kind in (2, 3, 4):
        assert (kinds[:, 0] == kind).sum() >= 2, kind
    out = lib.cull_planes(cam, rects, planes, pairs)
    invisible, hit = (out & 1) != 0, (out & 2) != 0
    print("P %s: %d pairs: %d invisible, %d hit by a pixel, %d clear hits and %d clear misses in float64, %d grazing" %
          (pose, n_pairs, invisible.sum(), hit.sum(), clear_hit.sum(), clear_miss.sum(), (kinds[:, 0] == 5).sum()))
    assert hit.sum() >= 40 and invisible.sum() >= 40
    assert (invisible & hit).sum() == 0, (int((invisible & hit).sum()), planes[pairs[invisible & hit, 1]][:3])
    assert (clear_hit & invisible).sum() == 0, (int((clear_hit & invisible).sum()), planes[pairs[clear_hit & invisible, 1]][:3])
    assert (clear_miss & ~invisible).sum() == 0, (int((clear_miss & ~invisible).sum()), planes[pairs[clear_miss & ~invisible, 1]][:3])
    # the allowance is the documented one and no smaller (as F for the spheres' margin: the pixel tests cannot see it, because
    # the hull is half a pixel larger than the pixels' own footprint): a facing plane that the footprint misses on no side by as
    # much as 0.95 allowances is kept
    short = (worst_gap > 0.3) & (worst_gap < 0.95)
    assert short.sum() >= 10, int(short.sum())
    assert not invisible[worst_gap < 0.95].any(), (int(invisible[worst_gap < 0.95].sum()), planes[pairs[invisible & (worst_gap < 0.95), 1]][:3])
    # what the comments promise beside it: num >= 0 and facing away are invisible, mixed signs and q < 1e-3 are kept
    assert invisible[kinds[:, 0] == 2].all() and invisible[kinds[:, 0] == 3].all()
    assert not invisible[kinds[:, 0] == 4].any()
    grazing = kinds[:, 0] == 5
    if W >= 1920:  # (the small frame's rectangles are too wide for all their corners to graze a plane)
        assert (grazing & (q64 < 0.9e-3)).sum() >= 3 and (grazing & (q64 > 2.0e-3)).sum() >= 3
    assert not invisible[grazing & (q64 < 0.9e-3)].any()
