"""The world grid of csrc/rtx_grid.hpp run directly on the GPU (tests/gpu_checks/grid_check.hip: the five build kernels and the two
query kernels of rtx_query_kernels.inc, walk_start / walk_step, grid_segment_dark of rtx_grid_segment.inc -- the production text,
with the product's launch shapes) on the scenes, rays and segments of tests/grid_cases.py, and held to the same header evaluated
on the host side of the library, to float64 (grid_cases.py states the formulas and derives every allowance) and to the production
exact tests.  tests/test_host_grid_check.py shows, without a GPU, that no class is vacuous; the counts are asserted here again
before the assertion they belong to.

  B0  every build output of the device equals the host's bit for bit: the bounds words, the Grid, n_cells, pairs, the number of
      large spheres, cell_start, list_geom, list_gidx, large[] with its canary, is_large.  The Grid also equals grid_cases.plan32,
      the planner in numpy float32.
  W0  every walk record (walkable, started, steps, and per step the cell and the bits of t_in and t_out) equals the host's.
      B0 and W0 carry tests/host/test_grid_bound.cpp and test_grid_shadow_bound.cpp over to gfx950.
  B1  the bounds words are the fp32 min / max of c -+ |r| over the finite spheres; the count is exact.
  B2  cell_start is non-decreasing from 0 to `pairs`; within a cell the sphere index ascends strictly (so a pair is listed once);
      a sphere's cells are a box, all of it; list_geom[j] and list_gidx[j] are the scene's words; large[] ascends and holds the
      flagged spheres; a sphere is in cells xor large; the canary is intact while the total reports every large sphere (257).
  L1  every cell meeting c +- (H - A) in float64 lists the sphere (H the header's half-width, A the derived allowance).
  L2  no cell outside c +- (H + A) lists it.
  L3  large iff the box is not finite or covers more than 64 cells in float64; within A of a boundary a sphere is undecided, at
      most 2 % of a case's.
  W1  (t_in and t_out are recorded with the sign of a zero dropped: fminf(+0, -0) is -0 on the device and +0 on the host, and no
      comparison tells them apart; a difference in a zero's sign alone is therefore invisible to W0)
      t_in of step k + 1 is t_out of step k bitwise; t_in <= t_out; t_out is the smallest T(X) = fl(fl(X - o) fl(1 / d)) over the far
      boundaries X of the cell, evaluated in numpy float32 from the cell's indices; consecutive cells differ by one on one axis; the float64 point
      at each interval's midpoint, and the float64 entry point, lie within `margin` of the cell on every axis; a walk whose last
      t_out is not past tmax stands in the grid's last cell on the axis walk_step would move (the first whose T is t_out).
  W2  walkable equals the header's rule in float64, started equals float64's slab test, wherever those are clear (the one-ulp
      class never is: W0 alone holds it).
  S1  a sphere that secondary_sphere_hit reports for a walkable ray at t <= tmax is in the large list or in a visited cell whose
      [t_in, t_out] holds t; one that segment_hits_sphere reports for a walkable segment is in the large list or a visited cell.
  Q   rtx_query_grid equals rtx_query_brute bit for bit, closest and any; the skipped object never wins; the fallback word is the
      number of unwalkable rays with tmax >= 0; the winner is float64's wherever that decides (twins: the lower creation index),
      and float64 decides all but 2 % of the rays outside the grazing, skip and one-ulp classes, which sit on the fp32 test's
      threshold by construction (grid_cases.py), and all but 2 % of the grazing rays from close by at |eps| >= 1e-4.  Creation
      indices are a permutation of the positions (grid_cases.gidx_of): of twins the one created first wins, not the one listed first.  grid_segment_dark equals the loop over every sphere and float64 likewise.
  P   a Context holding the same scene, created in the order of the library's creation indices, under the same RTX_OPT_QUERY_LOAD reports the library's cells, pairs, large spheres, brute
      flag and geometry words, and answers the rays byte for byte as the library's query does.  test_no_grid: the same, and Q, for
      the two scenes without a usable grid (no finite sphere; a scale beyond 2^50), where everything takes the brute routes.
"""
import ctypes as C
import os

import numpy as np
import pytest

import grid_cases as GC
import util as U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32, U32 = np.float32, np.uint32
CAP = 256
CANARY = 0xC0FFEE11
NO_T = 0xFFFFFFFF
UNDECIDED_CAP = 0.02


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


# ---------------------------------------------------------------------------------------------- the library

class Lib:
    """ctypes face of libgrid_check.so.  The library keeps the latest build of each side; `on` rebuilds when another scene is wanted."""

    def __init__(self, so):
        self.so = so
        self.current = {0: None, 1: None}
        self.kept = {}

    def ok(self, rc, what):
        if rc == -1:  # (a HIP error leaves the device in no state to go on with: nothing more is launched)
            pytest.exit("libgrid_check: HIP error in %s" % (what,), returncode=3)
        assert rc == 0, (what, rc)

    def build(self, name, host):
        geom, load = GC.scene(name)
        od = np.zeros((len(geom), 4), F32)
        od[:, 3] = GC.gidx_of(np.arange(len(geom))).view(F32)
        head = np.zeros(26, U32)
        rc = self.so.rtx_grid_check_build(_p(geom), _p(od), C.c_uint(len(geom)), C.c_float(load), C.c_int(host), _p(head))
        self.ok(rc, ("build", name, host))
        self.current[host] = name
        b = dict(head=head, bounds=head[0:7].copy(), grid=head[7:22].copy(), n_cells=int(head[22]), pairs=int(head[23]), n_large=int(head[24]), stage=int(head[25]))
        b["cell_start"] = np.zeros(b["n_cells"] + 1, U32)
        b["list_geom"] = np.zeros((b["pairs"] if b["stage"] == 2 else 0, 4), F32)
        b["list_gidx"] = np.zeros(b["pairs"] if b["stage"] == 2 else 0, U32)
        b["large"] = np.zeros(GC.LARGE_CAP + 1, U32)
        b["is_large"] = np.zeros(len(geom), np.uint8)
        rc = self.so.rtx_grid_check_lists(C.c_int(host), _p(b["cell_start"]), _p(b["list_geom"]), _p(b["list_gidx"]), _p(b["large"]), _p(b["is_large"]))
        self.ok(rc, ("lists", name, host))
        return b

    def on(self, name):
        """Both sides hold `name`; returns (device build, host build)."""
        if name not in self.kept:
            self.kept = {name: (self.build(name, 0), self.build(name, 1))}  # (one scene's arrays at a time)
        for host in (0, 1):
            if self.current[host] != name:
                self.build(name, host)
        return self.kept[name]

    def walk(self, host, rays, cap=CAP):
        rays = np.ascontiguousarray(rays, F32)
        flags, rec = np.zeros((len(rays), 3), U32), np.zeros((len(rays), cap, 3), U32)
        rc = self.so.rtx_grid_check_walk(C.c_int(host), _p(rays), C.c_uint(len(rays)), C.c_uint(cap), _p(flags), _p(rec))
        self.ok(rc, ("walk", host))
        return flags, rec

    def query(self, rays, any_, ns, matrix=False):
        rays = np.ascontiguousarray(rays, F32)
        hg, hb, fb = np.zeros((len(rays), 2), U32), np.zeros((len(rays), 2), U32), np.zeros(1, U32)
        m = np.zeros((len(rays), ns), U32) if matrix else None
        rc = self.so.rtx_grid_check_query(_p(rays), C.c_uint(len(rays)), C.c_int(any_), _p(hg), _p(hb), _p(fb), _p(m))
        self.ok(rc, "query")
        return hg, hb, int(fb[0]), m

    def segments(self, P, L, own_pos, ns):
        P, L = np.ascontiguousarray(P, F32), np.ascontiguousarray(L, F32)
        own = np.ascontiguousarray(np.stack([GC.gidx_of(own_pos), np.asarray(own_pos, U32)], axis=1))
        dg, db, fb = np.zeros(len(P), np.uint8), np.zeros(len(P), np.uint8), np.zeros(1, U32)
        m = np.zeros((len(P), ns), np.uint8)
        rc = self.so.rtx_grid_check_segments(_p(P), _p(L), _p(own), C.c_uint(len(P)), _p(dg), _p(db), _p(fb), _p(m))
        self.ok(rc, "segments")
        return dg, db, int(fb[0]), m


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    # (RTX_GRID_CHECK_LIB: another build of the library -- profiles/r24_grid_check.txt ran this file over eleven mutated ones)
    path = os.environ.get("RTX_GRID_CHECK_LIB") or os.path.join(HERE, "gpu_checks", "libgrid_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    return Lib(C.CDLL(path))


# ---------------------------------------------------------------------------------------------- the build's assertions

BUILD_KEYS = ("bounds", "grid", "n_cells", "pairs", "n_large", "stage", "cell_start", "list_geom", "list_gidx", "large", "is_large")


def check_b0(dev, host, what):
    for k in BUILD_KEYS:
        a, b = np.asarray(dev[k]), np.asarray(host[k])
        if a.ndim == 0:
            assert a == b, "%s B0: `%s` is %s on the device, %s on the host" % (what, k, a, b)
            continue
        assert a.shape == b.shape, "%s B0: `%s` has %s entries on the device, %s on the host" % (what, k, a.shape, b.shape)
        diff = np.flatnonzero(np.ascontiguousarray(a).reshape(-1).view(np.uint8) != np.ascontiguousarray(b).reshape(-1).view(np.uint8))
        assert len(diff) == 0, "%s B0: `%s` differs between device and host in %d bytes, the first at %d" % (what, k, len(diff), diff[0])


def check_b1(b, geom, what):
    lo, hi, nf, _ = GC.bounds32(geom)
    want = np.concatenate([lo.view(U32), hi.view(U32), np.array([nf], U32)])
    assert int(b["bounds"][6]) == nf, "%s B1: %d finite spheres counted, %d in the scene" % (what, int(b["bounds"][6]), nf)
    assert np.array_equal(b["bounds"].view(F32)[:6], want.view(F32)[:6]), "%s B1: bounds %s, fp32 min / max %s" % (what, b["bounds"].view(F32)[:6], want.view(F32)[:6])


def lists_of(b, ns, what):
    """B2's accounting of the offsets; returns (sphere index per entry, cell per entry)."""
    cs = b["cell_start"].astype(np.int64)
    assert cs[0] == 0 and (np.diff(cs) >= 0).all(), "%s B2: cell_start is not non-decreasing from 0" % what
    assert cs[-1] == b["pairs"], "%s B2: cell_start ends at %d, pairs %d" % (what, cs[-1], b["pairs"])
    idx = GC.index_of(b["list_gidx"])
    assert (idx >= 0).all() and (idx < ns).all(), "%s B2: a creation index that no sphere of the scene has" % what
    cell = np.repeat(np.arange(b["n_cells"]), np.diff(cs))
    return idx, cell


def check_b2(b, geom, what):
    ns = len(geom)
    flagged = np.flatnonzero(b["is_large"])
    assert b["n_large"] == len(flagged), "%s B2: %d large spheres reported, %d flagged" % (what, b["n_large"], len(flagged))
    assert b["large"][GC.LARGE_CAP] == CANARY, "%s B2: the word behind large[] was written (%#x)" % (what, b["large"][GC.LARGE_CAP])
    if not GC.grid_from_words(b["grid"])["ok"]:  # no usable grid: nothing behind the plan ran
        assert b["stage"] == 0 and b["n_cells"] == 0 and b["pairs"] == 0 and b["n_large"] == 0 and not b["is_large"].any()
        return None
    kept = min(b["n_large"], GC.LARGE_CAP)
    assert np.array_equal(b["large"][:kept], flagged[:kept]), "%s B2: large[] is not the flagged spheres in ascending order" % what
    assert b["stage"] == (1 if b["n_large"] > GC.LARGE_CAP else 2)
    if b["stage"] != 2:
        return None
    idx, cell = lists_of(b, ns, what)
    same = cell[1:] == cell[:-1]
    assert (idx[1:][same] > idx[:-1][same]).all(), "%s B2: sphere indices do not ascend strictly within a cell" % what
    assert np.array_equal(b["list_geom"].view(U32), np.asarray(geom, F32)[idx].view(U32)), "%s B2: list_geom is not the scene's geometry" % what
    assert np.array_equal(b["list_gidx"], GC.gidx_of(idx)), "%s B2: list_gidx is not the scene's creation index" % what
    listed = np.zeros(ns, bool)
    listed[idx] = True
    assert np.array_equal(listed, b["is_large"] == 0), "%s B2: spheres %s are not in cells xor large" % (what, np.flatnonzero(listed == (b["is_large"] != 0))[:8])
    return idx, cell


def ranges_of(b, g, ns, idx, cell):
    """first / last listed cell per sphere and axis (ns, 3, 2), and B2's box: the listed cells are all of that box."""
    n0, n1 = int(g["n"][0]), int(g["n"][1])
    xyz = np.stack([cell % n0, (cell // n0) % n1, cell // (n0 * n1)], axis=1)
    act = np.zeros((ns, 3, 2), np.int64)
    act[:, :, 0] = 1 << 30
    act[:, :, 1] = -1
    for k in range(3):
        np.minimum.at(act[:, k, 0], idx, xyz[:, k])
        np.maximum.at(act[:, k, 1], idx, xyz[:, k])
    count = np.bincount(idx, minlength=ns)
    box = np.prod(np.maximum(act[:, :, 1] - act[:, :, 0] + 1, 0), axis=1)
    return act, count, box


def check_lists64(b, geom, what, lists):
    """L1, L2, L3 (and B2's box) against float64 over the device's Grid."""
    g = GC.grid_from_words(b["grid"])
    ns = len(geom)
    must, may, finite = GC.ranges64(g, geom)
    verdict = GC.large64(g, geom)
    undecided = verdict == -1
    assert undecided.mean() <= UNDECIDED_CAP, "%s L3: %d of %d spheres undecided" % (what, undecided.sum(), ns)
    large = b["is_large"] != 0
    wrong = ~undecided & (large != (verdict == 1))
    assert not wrong.any(), "%s L3: spheres %s: large %s, float64 %s" % (what, np.flatnonzero(wrong)[:8], large[wrong][:8], verdict[wrong][:8])
    if lists is None:
        return
    idx, cell = lists
    act, count, box = ranges_of(b, g, ns, idx, cell)
    small = ~large
    assert (count[small] == box[small]).all(), "%s B2: the cells of spheres %s are not a whole box" % (what, np.flatnonzero(small & (count != box))[:8])
    sf = small & finite
    l1 = (act[:, :, 0] <= must[:, :, 0]) & (act[:, :, 1] >= must[:, :, 1])
    assert l1[sf].all(), "%s L1: spheres %s miss a cell their float64 box meets (listed %s, must %s)" % (
        what, np.flatnonzero(sf & ~l1.all(1))[:8], act[sf & ~l1.all(1)][:2].tolist(), must[sf & ~l1.all(1)][:2].tolist())
    l2 = (act[:, :, 0] >= may[:, :, 0]) & (act[:, :, 1] <= may[:, :, 1])
    assert l2[sf].all(), "%s L2: spheres %s are listed outside their float64 box (listed %s, may %s)" % (
        what, np.flatnonzero(sf & ~l2.all(1))[:8], act[sf & ~l2.all(1)][:2].tolist(), may[sf & ~l2.all(1)][:2].tolist())


@pytest.mark.parametrize("name", GC.NAMES)
def test_build(lib, name):
    geom, load = GC.scene(name)
    dev, host = lib.on(name)
    check_b0(dev, host, name)
    want = GC.plan_of(geom, load)
    assert np.array_equal(dev["grid"], GC.grid_words(want)), "%s B0: the Grid is not the float32 planner's: %s, %s" % (name, dev["grid"], GC.grid_words(want))
    assert dev["n_cells"] == GC.n_cells(want)
    check_b1(dev, geom, name)
    lists = check_b2(dev, geom, name)
    if name == "large257":
        assert dev["n_large"] == 257 and dev["stage"] == 1
    if name == "large256":
        assert dev["n_large"] == 256 and dev["stage"] == 2
    if name == "fine":
        assert dev["n_large"] == len(geom) > GC.LARGE_CAP
    if name == "dense":
        assert np.diff(dev["cell_start"].astype(np.int64)).max() > 256
    if name in ("cap", "halve"):
        assert dev["n_cells"] == (1 << 21 if name == "cap" else 72 * 129 * 114) and (name == "cap") != bool(want["halved"])
    if name == "c1025":
        assert dev["n_cells"] == 1025
    if name in GC.NOGRID:
        assert want["ok"] == 0 and dev["stage"] == 0
        return
    check_lists64(dev, geom, name, lists)


# ---------------------------------------------------------------------------------------------- the walk's assertions

def unpack(flags, rec):
    return dict(walkable=flags[:, 0].astype(bool), started=flags[:, 1].astype(bool), steps=flags[:, 2].astype(np.int64), cell=rec[:, :, 0].astype(np.int64),
                tin=np.ascontiguousarray(rec[:, :, 1]).view(F32), tout=np.ascontiguousarray(rec[:, :, 2]).view(F32), rec=rec)


def check_w0(dflags, drec, hflags, hrec, what):
    assert np.array_equal(dflags, hflags), "%s W0: rays %s: walkable / started / steps differ between device and host" % (what, np.flatnonzero((dflags != hflags).any(1))[:8])
    steps = dflags[:, 2].astype(np.int64)
    live = np.arange(drec.shape[1])[None, :] < steps[:, None]
    diff = (drec != hrec).any(2) & live
    assert not diff.any(), "%s W0: ray %d step %d: device %s, host %s" % ((what,) + tuple(np.argwhere(diff)[0]) + (drec[tuple(np.argwhere(diff)[0])], hrec[tuple(np.argwhere(diff)[0])]))


def check_w1(g, rays, w, what):
    o, d, tmax, _ = GC.split(rays)
    n0, n1, n2 = (int(x) for x in g["n"])
    E = [GC.edges(g, k) for k in range(3)]
    margin = float(g["margin"])
    steps = w["steps"]
    r32 = np.asarray(rays, F32).reshape(-1, 8)
    E32 = [e.astype(F32) for e in E]
    tiny, dmax32 = F32(2.0 ** -30), np.abs(r32[:, 4:7]).max(1)
    assert (steps[~w["started"]] == 0).all() and (steps[w["started"]] >= 1).all() and not (w["started"] & ~w["walkable"]).any()
    assert steps.max() <= CAP, "%s: a walk of %d steps does not fit the record" % (what, steps.max())

    def within(p, cells, rows, where):
        xyz = (cells % n0, (cells // n0) % n1, cells // (n0 * n1))
        assert (xyz[2] < n2).all(), "%s W1: a cell index past the grid" % what
        for k in range(3):
            bad = ~((p[:, k] >= E[k][xyz[k]] - margin) & (p[:, k] <= E[k][xyz[k] + 1] + margin))
            assert not bad.any(), "%s W1: ray %d, %s: the float64 point is %g outside its cell on axis %d (margin %g)" % (
                what, rows[bad][0], where, np.maximum(E[k][xyz[k]] - p[:, k], p[:, k] - E[k][xyz[k] + 1])[bad][0], k, margin)
        return xyz

    # the float64 entry point: the latest entry over the walked axes, or the origin
    st = np.flatnonzero(w["started"])
    with np.errstate(all="ignore"):
        dmax = np.abs(d).max(1)
        te = np.zeros(len(o))
        for k in range(3):
            walked = np.abs(d[:, k]) > GC.K_TINY * dmax
            near = np.where(d[:, k] > 0, E[k][0], E[k][-1])
            te = np.where(walked, np.maximum(te, (near - o[:, k]) / d[:, k]), te)
    within(o[st] + te[st, None] * d[st], w["cell"][st, 0], st, "the entry point")
    prev = None
    for k in range(int(steps.max())):
        rows = np.flatnonzero(steps > k)
        ti, to = w["tin"][rows, k].astype(np.float64), w["tout"][rows, k].astype(np.float64)
        assert (ti <= to).all(), "%s W1: ray %d step %d: t_in %r > t_out %r" % (what, rows[~(ti <= to)][0], k, ti[~(ti <= to)][0], to[~(ti <= to)][0])
        # t_out is the T of the cell's own far boundaries, T(X) = fl(fl(X - o) fl(1 / d)) from the integer index: nothing accumulates
        with np.errstate(all="ignore"):
            T = np.full(len(rows), np.inf, F32)
            for a in range(3):
                ca = (w["cell"][rows, k] // (1, n0, n0 * n1)[a]) % (n0, n1, n2)[a]
                da, oa = r32[rows, 4 + a], r32[rows, a]
                X = E32[a][np.where(da > 0, ca + 1, ca)]
                Ta = ((X - oa).astype(F32) * (F32(1) / da).astype(F32)).astype(F32)
                T = np.where(np.abs(da) > tiny * dmax32[rows], np.minimum(T, Ta), T)
        assert np.array_equal(T + F32(0), w["tout"][rows, k]), "%s W1: ray %d step %d: t_out %r is not the T of its cell's boundaries, %r" % (
            what, rows[(T + F32(0)) != w["tout"][rows, k]][0], k, w["tout"][rows, k][(T + F32(0)) != w["tout"][rows, k]][0], T[(T + F32(0)) != w["tout"][rows, k]][0])
        tm = np.where(np.isfinite(to), 0.5 * ti + 0.5 * to, ti)
        xyz = within(o[rows] + tm[:, None] * d[rows], w["cell"][rows, k], rows, "step %d's midpoint" % k)
        if k > 0:
            assert np.array_equal(w["rec"][rows, k, 1], w["rec"][rows, k - 1, 2]), "%s W1: step %d's t_in is not step %d's t_out bitwise" % (what, k, k - 1)
            assert (w["tin"][rows, k] >= w["tin"][rows, k - 1]).all(), "%s W1: t_in decreases at step %d" % (what, k)
            moved = sum(np.abs(xyz[a] - prev[a][steps[prev_rows] > k]) for a in range(3))
            assert (moved == 1).all(), "%s W1: step %d does not move one cell along one axis" % (what, k)
        prev, prev_rows = xyz, rows
    # the end: past tmax, or at the grid's boundary in the direction of travel
    last = steps[st] - 1
    to = w["tout"][st, last].astype(np.float64)
    c = w["cell"][st, last]
    xyz = (c % n0, (c // n0) % n1, c // (n0 * n1))
    nk = (n0, n1, n2)
    # ... on the axis walk_step would move: the first of x, y, z whose far boundary's T is the cell's t_out
    at_rim, taken = np.zeros(len(st), bool), np.zeros(len(st), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            dk, ok_ = r32[st, 4 + k], r32[st, k]
            X = E32[k][np.where(dk > 0, xyz[k] + 1, xyz[k])]
            Tk = ((X - ok_).astype(F32) * (F32(1) / dk).astype(F32)).astype(F32)
            mine = ~taken & (np.abs(dk) > tiny * dmax32[st]) & (Tk + F32(0) == w["tout"][st, last])
            at_rim |= mine & (((dk > 0) & (xyz[k] == nk[k] - 1)) | ((dk < 0) & (xyz[k] == 0)))
            taken |= mine
    assert taken.all(), "%s W1: ray %d: no walked axis leaves the last cell at its t_out" % (what, st[~taken][0])
    with np.errstate(invalid="ignore"):
        ended = (to > tmax[st]) | at_rim
    assert ended.all(), "%s W1: ray %d stops inside the grid before tmax" % (what, st[~ended][0])


def check_w2(g, rays, w, what, counts=None):
    o, d, tmax, _ = GC.split(rays)
    want = GC.walkable64(g, o, d)
    clear = want >= 0
    assert clear.sum() >= 0.9 * len(rays)
    bad = clear & (w["walkable"] != (want == 1))
    assert not bad.any(), "%s W2: rays %s: walkable %s, float64 %s" % (what, np.flatnonzero(bad)[:8], w["walkable"][bad][:8], want[bad][:8])
    meets = GC.meets64(g, o, d, tmax)
    sure = clear & (want == 1) & (meets >= 0)
    bad = sure & (w["started"] != (meets == 1))
    assert not bad.any(), "%s W2: rays %s: started %s, float64 %s" % (what, np.flatnonzero(bad)[:8], w["started"][bad][:8], meets[bad][:8])
    return clear, sure


def rays_for(name, dev):
    geom, _ = GC.scene(name)
    g = GC.grid_from_words(dev["grid"])
    rays, cls, eps, far = GC.rays_of(name, geom, g)
    return geom, g, rays, cls, eps, far


@pytest.mark.parametrize("name", GC.WALKED)
def test_walk(lib, name):
    dev, _ = lib.on(name)
    geom, g, rays, cls, eps, far = rays_for(name, dev)
    P, L, own, scls = GC.segments_of(name, geom, g)
    for what, rr in (("%s rays" % name, GC.library_rays(rays)), ("%s segments" % name, GC.segment_rays(P, L))):
        dflags, drec = lib.walk(0, rr)
        hflags, hrec = lib.walk(1, rr)
        check_w0(dflags, drec, hflags, hrec, what)
        w = unpack(dflags, drec)
        assert w["started"].sum() >= (0.2 if "segments" in what else 0.5) * len(rr) and (~w["walkable"]).sum() >= 30, what
        assert "segments" in what or (w["walkable"] & ~w["started"]).sum() >= 10, what
        check_w1(g, rr, w, what)
        check_w2(g, rr, w, what)


# ---------------------------------------------------------------------------------------------- S1 and Q

def covered(b, w, pairs_ray, pairs_sphere, pairs_t, ns):
    """Per (ray, sphere, t) pair: is the sphere in the large list, or in a visited cell whose [t_in, t_out] holds t (t None: any)?"""
    large = np.zeros(ns, bool)
    if b["stage"] == 2:
        large[b["large"][:b["n_large"]]] = True
    ok = large[pairs_sphere]
    if b["stage"] != 2:
        return ok
    idx, cell = lists_of(b, ns, "S1")
    member = np.unique(cell * ns + idx)
    for k in range(int(w["steps"][pairs_ray].max()) if len(pairs_ray) else 0):
        at = w["steps"][pairs_ray] > k
        if pairs_t is not None:
            at &= (w["tin"][pairs_ray, k] <= pairs_t) & (pairs_t <= w["tout"][pairs_ray, k])
        ok |= at & np.isin(w["cell"][pairs_ray, k] * ns + pairs_sphere, member)
    return ok


@pytest.mark.parametrize("name", GC.WALKED)
def test_query(lib, name):
    dev, _ = lib.on(name)
    geom, g, rays, cls, eps, far = rays_for(name, dev)
    ns = len(geom)
    lrays = GC.library_rays(rays)
    w = unpack(*lib.walk(0, lrays))
    hg, hb, fb, m = lib.query(lrays, 0, ns, matrix=True)
    ag, ab, afb, _ = lib.query(lrays, 1, ns)
    tmax32 = lrays[:, 3]
    # S1
    t = m.view(F32)
    with np.errstate(invalid="ignore"):
        reported = (m != NO_T) & (t <= tmax32[:, None]) & w["walkable"][:, None]
    pr, ps = np.nonzero(reported)
    has_graze = (cls == 0).any()
    if has_graze:
        # (inside the sphere by 1e-5 r or more, from close by, the test must report: three in eight of the rays inside; from the rim
        # it is a matter of rounding)
        graze_hits, inside = reported[cls == 0].any(1).sum(), ((cls == 0) & (eps < 0)).sum()
        assert graze_hits >= 0.3 * inside, "%s: %d of %d grazing rays inside their sphere report a hit" % (name, graze_hits, inside)
        assert reported[(cls == 0) & far].any(1).sum() >= 0.1 * ((cls == 0) & far).sum()
    ok = covered(dev, w, pr, ps, t[pr, ps], ns)
    assert ok.all(), "%s S1: %d reported hits lie in no visited cell: ray %d (class %s) sphere %d t %r" % (
        name, (~ok).sum(), pr[~ok][0], GC.CLASSES[cls[pr[~ok][0]]], ps[~ok][0], t[pr[~ok][0], ps[~ok][0]])
    # Q: grid = brute
    assert np.array_equal(hg, hb), "%s Q: closest: rays %s differ between grid and brute (grid %s, brute %s)" % (
        name, np.flatnonzero((hg != hb).any(1))[:8], hg[(hg != hb).any(1)][:2].tolist(), hb[(hg != hb).any(1)][:2].tolist())
    assert np.array_equal(ag, ab), "%s Q: any: rays %s differ between grid and brute" % (name, np.flatnonzero((ag != ab).any(1))[:8])
    hit = hg[:, 1] != GC.NONE
    assert np.array_equal(ag[:, 1] != GC.NONE, hit) and (ag[hit, 1] == 0xFFFFFFFE).all() and (ag[hit, 0] == 0).all()
    skip = np.ascontiguousarray(lrays[:, 7]).view(U32)
    assert not ((skip != GC.NONE) & (hg[:, 1] == skip)).any(), "%s Q: the skipped object wins" % name
    with np.errstate(invalid="ignore"):
        live = tmax32 >= 0
    unwalkable = int((~w["walkable"] & live).sum())
    assert (~w["walkable"] & live).sum() >= 20 and (~w["walkable"] & ~live).sum() >= 10
    assert fb == unwalkable and afb == unwalkable, "%s Q: the fallback word is %d (any: %d), %d live rays cannot be walked" % (name, fb, afb, unwalkable)
    # Q: float64's winner
    best, decided = GC.closest64(rays, geom)
    core = ~np.isin(cls, [GC.CLASSES.index(c) for c in ("grazing", "skip", "ulp")])
    assert (~decided[core]).mean() <= UNDECIDED_CAP, "%s Q: float64 leaves %d of %d rays undecided" % (name, (~decided[core]).sum(), core.sum())
    if has_graze:
        assert decided[cls == 0].sum() >= 0.25 * (cls == 0).sum()
        # from close by, at |eps| >= 1e-4, the allowance of DESIGN 4.1 is far below 2 eps r^2: these float64 must decide
        near = (cls == 0) & ~far & (np.abs(eps) >= 1e-4)
        assert near.sum() >= 0.15 * (cls == 0).sum()
        assert (~decided[near]).mean() <= UNDECIDED_CAP, "%s Q: float64 leaves %d of %d grazing rays from close by undecided" % (name, (~decided[near]).sum(), near.sum())
        sk = cls == GC.CLASSES.index("skip")
        free = np.array(rays[sk], copy=True)
        free[:, 7] = np.array([GC.NONE], U32).view(F32)[0]
        b2, d2 = GC.closest64(free, geom)
        aimed = np.ascontiguousarray(rays[sk, 7]).view(U32).astype(np.int64)
        # (those that float64 decides and no other sphere stands in front of; n1 has 14 grazing rays)
        assert (d2 & (b2 == aimed)).sum() >= (3 if name == "n1" else 8), "%s: the skipped sphere would win %d of %d rays" % (name, (d2 & (b2 == aimed)).sum(), sk.sum())
    want = GC.gidx_of(best)
    bad = decided & (hg[:, 1] != want)
    assert not bad.any(), "%s Q: rays %s (classes %s): winner %s, float64 %s" % (
        name, np.flatnonzero(bad)[:8], [GC.CLASSES[c] for c in cls[bad][:8]], hg[bad, 1][:8], want[bad][:8])
    if name == "n257":  # (the twin at position 200 has the lower creation index)
        assert GC.gidx_of(200) < GC.gidx_of(100)
        assert (best[decided] == 200).sum() >= 3 and not (hg[:, 1] == GC.gidx_of(100)).any(), "the twin created later wins"


@pytest.mark.parametrize("name", GC.WALKED)
def test_segments(lib, name):
    dev, _ = lib.on(name)
    geom, _ = GC.scene(name)
    g = GC.grid_from_words(dev["grid"])
    ns = len(geom)
    P, L, own, scls = GC.segments_of(name, geom, g)
    w = unpack(*lib.walk(0, GC.segment_rays(P, L)))
    dg, db, fb, m = lib.segments(P, L, own, ns)
    pr, ps = np.nonzero((m != 0) & w["walkable"][:, None])
    if (scls <= 2).any():  # (a third of them go through their sphere)
        assert len(np.unique(pr[scls[pr] <= 2])) >= 0.25 * ((scls <= 2) & w["walkable"]).sum(), "%s: %d grazing segments report a hit" % (name, len(np.unique(pr[scls[pr] <= 2])))
    ok = covered(dev, w, pr, ps, None, ns)
    assert ok.all(), "%s S1: segment %d (class %s) hits sphere %d, which is in no visited cell" % (name, pr[~ok][0], GC.SEG_CLASSES[scls[pr[~ok][0]]], ps[~ok][0])
    assert np.array_equal(dg, db), "%s Q: segments %s: grid %s, every sphere %s" % (name, np.flatnonzero(dg != db)[:8], dg[dg != db][:8], db[dg != db][:8])
    assert (~w["walkable"]).sum() >= 60
    assert fb == (~w["walkable"]).sum(), "%s Q: %d segments counted as fallback, %d cannot be walked" % (name, fb, (~w["walkable"]).sum())
    want = GC.dark64(P, L, own, geom)
    core = scls > 2
    assert (want[core] == -1).mean() <= UNDECIDED_CAP
    if (scls == 2).any() and name != "dense":  # (through their own sphere at 0 .. 0.9 r: without it float64 decides; dense: radii of 1e-5)
        free = GC.dark64(P[scls == 2], L[scls == 2], np.full((scls == 2).sum(), GC.NONE, U32), geom)
        assert (free == -1).mean() <= UNDECIDED_CAP
    bad = (want >= 0) & (dg != want)
    assert not bad.any(), "%s Q: segments %s (classes %s): dark %s, float64 %s" % (
        name, np.flatnonzero(bad)[:8], [GC.SEG_CLASSES[c] for c in scls[bad][:8]], dg[bad][:8], want[bad][:8])
    if (scls == 2).any():
        mine = scls == 2
        # (dense: from the rim a radius of 1e-5 is below what the fp32 test resolves)
        assert (m[mine, own[mine]] != 0).mean() >= (0.4 if name == "dense" else 0.9), "the own class goes through its own sphere"


@pytest.mark.parametrize("name", GC.NOGRID)
def test_no_grid(lib, ctx, name):
    """Q and P where rtxgrid::Grid::ok is 0: no ray is walkable, the brute kernel answers (and counts no fallback ray, as in the
    Context), every segment takes grid_segment_dark's loop over the scene and is counted."""
    R, c = ctx
    geom, load = GC.scene(name)
    dev, _ = lib.on(name)
    ns = len(geom)
    rays = GC.nogrid_rays(name, geom)
    lrays = GC.library_rays(rays)
    w = unpack(*lib.walk(0, lrays))
    assert np.array_equal(w["rec"], unpack(*lib.walk(1, lrays))["rec"]) and not w["walkable"].any() and not w["started"].any()
    best, decided = GC.closest64(rays, geom)
    assert decided.mean() >= 0.9 and (name == "nofinite" or (best[decided] != GC.NONE).sum() >= 40)
    order, rank = GC.creation_order(ns)
    for opt, v in ((R.OPT_QUERY_CHECK, 0), (R.OPT_QUERY_LOAD, 16)):
        c.set_option(opt, v)
    c.scene_clear()
    c.add_spheres(np.concatenate([geom[order], np.full((ns, 3), 200.0, F32)], axis=1))
    skip_pos = np.ascontiguousarray(rays[:, 7]).view(U32).astype(np.int64)
    pr = np.zeros(len(rays), R.RAY_DTYPE)
    pr["o"], pr["tmax"], pr["d"] = rays[:, 0:3], rays[:, 3], rays[:, 4:7]
    pr["skip"] = np.where(skip_pos == GC.NONE, GC.NONE, rank[np.minimum(skip_pos, ns - 1)]).astype(U32)
    for any_ in (0, 1):
        hg, hb, fb, _ = lib.query(lrays, any_, ns)
        assert np.array_equal(hg, hb) and fb == 0, "%s Q: the brute route differs from brute, or counts (%d)" % (name, fb)
        if not any_:
            bad = decided & (hg[:, 1] != GC.gidx_of(best))
            assert not bad.any(), "%s Q: rays %s: winner %s, float64 %s" % (name, np.flatnonzero(bad)[:8], hg[bad, 1][:8], GC.gidx_of(best)[bad][:8])
        got = c.query_rays(pr, R.QUERY_ANY if any_ else R.QUERY_CLOSEST)
        idx = got["index"].astype(np.int64)
        mapped = np.where(idx >= 0xFFFFFFFE, idx, GC.gidx_of(order[np.minimum(idx, ns - 1)])).astype(U32)
        assert np.array_equal(np.ascontiguousarray(got["t"]).view(U32), hg[:, 0]) and np.array_equal(mapped, hg[:, 1]), "%s P: the context's answers differ" % name
        assert c.get_option(R.STAT_QUERY_FALLBACK_RAYS) == 0
    assert (c.get_option(R.STAT_QUERY_BRUTE), c.get_option(R.STAT_QUERY_GRID_CELLS), c.get_option(R.STAT_QUERY_GRID_PAIRS)) == (1, 0, 0)
    # segments along the rays, from the origin to past the sphere aimed at (its near side is at t = 1e7)
    P, L = rays[:, 0:3], (rays[:, 0:3].astype(np.float64) + 1.5e7 * rays[:, 4:7].astype(np.float64)).astype(F32)
    own = np.where(np.arange(len(P)) % 8 == 0, skip_pos, GC.NONE).astype(U32)
    dg, db, sfb, m = lib.segments(P, L, own, ns)
    assert np.array_equal(dg, db) and sfb == len(P), "%s Q: segments: grid %d dark, every sphere %d; %d of %d counted" % (name, dg.sum(), db.sum(), sfb, len(P))
    want = GC.dark64(P, L, own, geom)
    bad = (want >= 0) & (dg != want)
    assert not bad.any(), "%s Q: segments %s: dark %s, float64 %s" % (name, np.flatnonzero(bad)[:8], dg[bad][:8], want[bad][:8])


# ---------------------------------------------------------------------------------------------- P: the product

@pytest.fixture(scope="module")
def ctx():
    R = U.pkg()
    c = R.Context(400, 150)
    yield R, c
    c.close()


@pytest.mark.parametrize("name", GC.PRODUCT)
def test_product(lib, ctx, name):
    R, c = ctx
    geom, load = GC.scene(name)
    dev, _ = lib.on(name)
    sixteenths = load * 16.0
    assert sixteenths == int(sixteenths) >= 1
    for opt, v in ((R.OPT_QUERY_CHECK, 0), (R.OPT_QUERY_LOAD, int(sixteenths))):
        c.set_option(opt, v)
    c.scene_clear()
    # the Context creates the spheres in the order of the library's creation indices: its index k is the library's position order[k]
    order, rank = GC.creation_order(len(geom))
    c.add_spheres(np.concatenate([geom[order], np.full((len(geom), 3), 200.0, F32)], axis=1))
    g = GC.grid_from_words(dev["grid"])
    if name in GC.WALKED:
        rays = GC.rays_of(name, geom, g)[0]
    else:
        rays = GC.rays_of(name, geom, g, per_class=64, graze_spheres=16)[0]
    pr = np.zeros(len(rays), R.RAY_DTYPE)
    skip_pos = np.ascontiguousarray(rays[:, 7]).view(U32).astype(np.int64)
    pr["o"], pr["tmax"], pr["d"] = rays[:, 0:3], rays[:, 3], rays[:, 4:7]
    pr["skip"] = np.where(skip_pos == GC.NONE, GC.NONE, rank[np.minimum(skip_pos, len(geom) - 1)]).astype(U32)
    for flags in (R.QUERY_CLOSEST, R.QUERY_ANY):
        got = c.query_rays(pr, flags)
        fb = c.get_option(R.STAT_QUERY_FALLBACK_RAYS)
        hg, _, lfb, _ = lib.query(GC.library_rays(rays), 1 if flags == R.QUERY_ANY else 0, len(geom))
        idx = got["index"].astype(np.int64)
        mapped = np.where(idx >= 0xFFFFFFFE, idx, GC.gidx_of(order[np.minimum(idx, len(geom) - 1)])).astype(U32)
        tb = np.ascontiguousarray(got["t"]).view(U32)
        differ = (tb != hg[:, 0]) | (mapped != hg[:, 1])
        assert not differ.any(), "%s P: rays %s: the context answers %s, the library %s" % (name, np.flatnonzero(differ)[:8], got[differ][:2], hg[differ][:2].tolist())
        assert fb == lfb, "%s P: fallback rays %d, the library's %d" % (name, fb, lfb)
    stats = dict(cells=c.get_option(R.STAT_QUERY_GRID_CELLS), pairs=c.get_option(R.STAT_QUERY_GRID_PAIRS), large=c.get_option(R.STAT_QUERY_LARGE_SPHERES),
                 brute=c.get_option(R.STAT_QUERY_BRUTE))
    assert stats == dict(cells=dev["n_cells"], pairs=dev["pairs"], large=dev["n_large"], brute=int(dev["stage"] != 2)), (name, stats, dev["head"][22:26])
    geo = np.array([c.get_option(R.STAT_QUERY_GRID_GEOMETRY + k) for k in range(9)], np.int64).astype(U32)
    assert np.array_equal(geo, dev["grid"][0:9]), "%s P: the context's grid %s, the library's %s" % (name, geo, dev["grid"][0:9])
