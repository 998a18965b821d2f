"""Inputs and numpy / float64 yardsticks for the passes in front of a culled trace launch -- rtx_bin_cells, rtx_order_tiles,
rtx_balance_tiles -- shared by tests/test_gpu_sched_check.py (the device, through tests/gpu_checks/sched_check.hip) and
tests/test_host_sched_check.py (the inputs and the yardsticks themselves, without a GPU).

Coarse-cell lists.  A scene is a frame, a tile shape, a pose, a motion budget and ns spheres.  Every (cell, sphere) pair is
judged in float64 from the float32 inputs (cull_geometry.py, the yardsticks of tests/test_gpu_cull_bound.py):
  near    some pixel half-line of the cell (its pixels inside the frame) passes within |r| (1 - 1e-5) of the centre at t > 0:
          the sphere must be listed (B3);
  beyond  the centre lies beyond one of the five planes of the cell's pyramid (the whole cell, as the kernel forms it, also where
          it reaches past the frame's edge) by more than margin (1 + 1e-4) + 2e-6 |O|, margin the moving margin of the scene's
          budget (assertion F of test_gpu_cull_bound.py): the sphere must not be listed (B4).
What is neither is undecided; tests/test_host_sched_check.py holds every scene to at most 5 % of such pairs.

Dispatch orders.  An order is read as tx | ty << 16, tile = ty gx + tx.  The class functions restate the kernels' integer and
float32 class arithmetic exactly (order_class, balance_classes); everything else is judged from the outputs alone.  sim_order and
sim_balance deal the same orders from a plain sort, for the host test of the judges."""
import functools
import math

import numpy as np

import cull_geometry as CG
from cull_geometry import F32

POISON = 0xA5A5A5A5
GARBAGE = 0x5EED5EED

# ---------------------------------------------------------------------------------------------- coarse-cell lists: shapes


class Shape:
    """A frame, the tile shape fields of KArgs and the cell's size in tiles, as rtx_bin_cells reads them."""

    def __init__(self, W, H, lw, nsub, lnx, gx, gy, row0=0):
        self.W, self.H, self.lw, self.nsub, self.lnx, self.gx, self.gy, self.row0 = W, H, lw, nsub, lnx, gx, gy, row0
        tw, th = 1 << lw, 256 >> lw
        self.cw, self.ch = (tw << lnx) << gx, (th * (nsub >> lnx)) << gy
        self.cells_x, self.cells_y = -(-W // self.cw), -(-(H - row0) // self.ch)
        self.n_cells = self.cells_x * self.cells_y
        self.n_blocks = ((self.cells_x + 3) >> 2) * ((self.cells_y + 3) >> 2)

    def words(self, cap):
        return np.array([self.lw, self.nsub, self.lnx, self.gx, self.gy, self.cells_x, self.cells_y, cap, self.row0], np.uint32)

    def slab(self, row0):
        return Shape(self.W, self.H, self.lw, self.nsub, self.lnx, self.gx, self.gy, row0)

    def full_rect(self, c):
        cy, cx = divmod(c, self.cells_x)
        return (cx * self.cw, self.row0 + cy * self.ch, self.cw, self.ch)

    def clipped_rect(self, c):
        c0, r0, w, h = self.full_rect(c)
        return (c0, r0, min(w, self.W - c0), min(h, self.H - r0))

    def slots_beyond_the_grid(self):
        return 16 * self.n_blocks - self.n_cells


SHAPES = {
    "16x16": Shape(80, 48, 4, 1, 0, 0, 0),      # 5 x 3 cells: two blocks, 17 of their 32 cell slots beyond the grid
    "wide": Shape(80, 48, 4, 1, 0, 1, 0),       # cells of 2 x 1 tiles: 32 x 16 pixels, 3 x 3 cells, the last column half in the frame
    "nsub4": Shape(80, 48, 4, 4, 1, 0, 0),      # macro tiles of 2 x 2 sub-tiles: 32 x 32 pixels, 3 x 2 cells, both edges cut
    "64x4": Shape(80, 48, 6, 1, 0, 0, 0),       # 64 x 4-pixel tiles: 2 x 12 cells, three blocks one above the other
}
CAPS = (1, 7, None)  # None: ns
BUDGETS = ((0.0, 0.0), (0.02, 1.0))

# name: shape, pose, budget, ns, seed, cells that get directed spheres (0 first, 1 middle, 2 last), the bulk's distances, its spread
# over the view plane (1: the frame).  A budget's margin is a strip of 0.02 rad + 1 / distance around every cell, and the directed
# spheres sit on the planes by design: the small scenes take one cell's directed set, the budget scenes a distant bulk, and the
# 513-sphere scene, whose cells fill a ninth of the frame each, a bulk spread beyond the frame, so that float64 decides 95 % of
# each scene's pairs (tests/test_host_sched_check.py).
SCENES = {
    "n5000": ("16x16", "default", BUDGETS[0], 5000, 1, (0, 1, 2), (20.0, 200.0), 1.1),
    "n1700": ("16x16", "rolled", BUDGETS[1], 1700, 2, (2,), (150.0, 600.0), 1.1),
    "n513": ("wide", "default", BUDGETS[1], 513, 3, (2,), (80.0, 400.0), 1.8),
    "n512": ("nsub4", "rolled", BUDGETS[0], 512, 4, (2,), (20.0, 200.0), 1.1),
    "n511": ("64x4", "default", BUDGETS[0], 511, 5, (1,), (20.0, 200.0), 1.1),
    "n1": ("16x16", "rolled", BUDGETS[0], 1, 6, (), (20.0, 200.0), 1.1),
}
JUDGED = tuple(n for n in SCENES if n != "n1")  # (the lone covering sphere has 15 pairs: all of them must be listed)


def planned_splits(ns, n_blocks):
    """rtx_plan.hpp, plan_cells: about 1024 binning workgroups in all, each with at least 1024 spheres."""
    return max(1, min(1024 // n_blocks, (ns + 1023) // 1024))


# ---------------------------------------------------------------------------------------------- coarse-cell lists: spheres

PUSH_S = (0.5, 0.9, 1.1, 2.0, 10.0)


def _pushed(o, point_dir, D, out, r, s, literal, margin):
    """As test_gpu_cull_bound.py's `pushed`: centre = o + D point_dir + out * push, push = s margins (or r + s margins), the margin
    taken at the centre's own distance."""
    base = o + D * point_dir
    push = r
    for _ in range(3):
        m = margin(r, np.linalg.norm(base + out * push - o))
        push = r + s * m if literal else s * m
    return base + out * push


class Scene:
    def __init__(self, name):
        shape, pose, budget, ns, seed, targets, d_range, spread = SCENES[name]
        self.name, self.shape, self.ns = name, SHAPES[shape], ns
        self.cam = cam = CG.camera(self.shape.W, self.shape.H, pose)
        self.theta, self.delta = budget
        th32, de32 = float(F32(budget[0])), float(F32(budget[1]))
        self.margin = lambda r, dist: CG.moving_margin64(r, dist, th32, de32)
        rng = np.random.default_rng(100 + seed)
        o, R = cam.pos, cam.rot
        fwd, right, up = CG.unit(R[:, 2]), CG.unit(R[:, 0]), CG.unit(R[:, 1])
        e1, e2 = cam.e
        rows, kind, aimed = [], [], []

        def add(row, k, cell=-1):
            rows.append(np.asarray(row, np.float64))
            kind.append(k)
            aimed.append(cell)

        add(np.append(o + fwd * 300.0, 290.0), "cover")   # every pixel of the frame hits it; the camera is outside
        if ns > 1:
            for v in (fwd, fwd + 0.3 * right, fwd - 0.4 * up):
                add(np.append(o - CG.unit(v) * 50.0, 5.0), "behind")
            for sx, sy, r in ((0.31, 0.22, 0.0), (-0.52, -0.4, 0.0), (0.12, -0.61, -2.0), (-0.7, 0.33, -1.0)):
                add(np.append(o + CG.unit(cam.dirs(sx, sy)) * 60.0, r), "r<=0")
            add(np.append(o + fwd * 1.0, 5.0), "inside")
            add(np.append(o + np.array([4.0, 0.0, 0.0]), 4.0), "on")    # |O| = r exactly in float32: cc = 0
            add([float("nan"), 0.0, 0.0, 1.0], "nan")
            add(np.append(o + np.array([3.0, 0.0, 4.0]), float("inf")), "inf")
            # directed: beyond each side plane of the scene's target cells by s margins / r + s margins
            sh = self.shape
            self.targets = tuple((0, sh.n_cells // 2, sh.n_cells - 1)[t] for t in targets)
            for ci, c in enumerate(self.targets):
                pyr = CG.Pyramid(cam, sh.full_rect(c))
                for k in range(4):
                    for i, s in enumerate(PUSH_S):
                        for j, r in enumerate((0.0, 0.3, 3.0)):
                            D = (30.0, 120.0)[(i + j + ci) % 2]
                            f = (0.5, 0.15, 0.85)[(i + j) % 3]
                            add(np.append(_pushed(o, pyr.edge_dir(k, f), D, -pyr.n[k], r, s, (i + j + k) % 2 == 1, self.margin), r), "directed", c)
            # the bulk: small against a cell, no smaller than the pixel spacing (a sphere between the rays is undecided)
            n_bulk = ns - len(rows)
            assert n_bulk > 0
            d = rng.uniform(d_range[0], d_range[1], n_bulk)
            w = CG.unit(cam.dirs(rng.uniform(-spread, spread, n_bulk), rng.uniform(-spread, spread, n_bulk)))
            px = 0.5 * math.hypot(2.0 * e1 / sh.W, 2.0 * e2 / sh.H)
            r = d * px * rng.uniform(1.2, 2.5, n_bulk)
            for row in np.column_stack([o + w * d[:, None], r]):
                add(row, "bulk")
        order = rng.permutation(len(rows)) if ns > 1 else np.arange(1)  # (creation order mixes the kinds)
        with np.errstate(invalid="ignore", over="ignore"):
            self.sph = np.array(rows)[order].astype(F32)
        self.kind, self.aimed = np.array(kind)[order], np.array(aimed)[order]   # (aimed: the cell a directed sphere was pushed from)
        assert len(self.sph) == ns

    def always_listed(self):
        """A camera inside or on a sphere, a NaN centre, an infinite radius: in every valid cell's list."""
        return np.flatnonzero(np.isin(self.kind, ("inside", "on", "nan", "inf")))

    def rects(self, shape=None, clipped=True):
        sh = shape or self.shape
        return np.array([sh.clipped_rect(c) if clipped else sh.full_rect(c) for c in range(sh.n_cells)], np.uint32)

    @functools.lru_cache(maxsize=None)
    def judged(self):
        """(near, beyond): n_cells x ns bools, float64 from the float32 inputs."""
        sh, cam = self.shape, self.cam
        s64 = self.sph.astype(np.float64)
        radii = np.abs(s64[:, 3])
        near, beyond = np.zeros((sh.n_cells, self.ns), bool), np.zeros((sh.n_cells, self.ns), bool)
        with np.errstate(invalid="ignore", over="ignore"):
            otc = cam.pos - s64[:, :3]
            dist = np.sqrt((otc * otc).sum(1))
            allow = self.margin(radii, dist) * (1.0 + 1.0e-4) + 2.0e-6 * dist
            for c in range(sh.n_cells):
                near[c] = CG.min_ray_distance(cam, sh.clipped_rect(c), s64[:, :3], radii)
                d = otc @ CG.Pyramid(cam, sh.full_rect(c)).n.T   # (ns, 5): how far beyond plane k the centre lies
                beyond[c] = (d > allow[:, None]).any(1)
        return near, beyond


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name)


def sets_of(counts, lists, n_cells, cap, ns):
    """The listed set of every cell from a run whose capacity held every list."""
    assert (counts[:n_cells] <= cap).all()
    assert all((lists[c * cap:c * cap + counts[c]] < ns).all() for c in range(n_cells)), "an entry is not below ns"
    return [frozenset(lists[c * cap:c * cap + counts[c]].tolist()) for c in range(n_cells)]


# ---------------------------------------------------------------------------------------------- rtx_order_tiles

ORDER_N = (1, 7, 8, 9, 1023, 1024, 1025, 40000)
GRID_OF = {1: (1, 1), 7: (7, 1), 8: (4, 2), 9: (3, 3), 1023: (33, 31), 1024: (32, 32), 1025: (41, 25), 40000: (200, 200)}
COST_KINDS = ("equal", "zero", "max", "giant", "around2p24", "ascending", "descending", "random")


def costs(kind, n, rng):
    if kind == "equal":
        c = np.full(n, 12345)
    elif kind == "zero":
        c = np.zeros(n)
    elif kind == "max":
        c = np.full(n, 0xffffffff)
    elif kind == "giant":
        c = rng.integers(100, 2000, n)
        c[n // 3] = 0xfffffff0
    elif kind == "around2p24":
        c = (1 << 24) + rng.integers(-3000, 3000, n)
    elif kind == "ascending":
        c = np.arange(n) * 37 + 5
    elif kind == "descending":
        c = (np.arange(n) * 37 + 5)[::-1]
    else:
        assert kind == "random"
        c = rng.integers(0, 1 << 20, n)
    return np.asarray(c, np.int64).astype(np.uint32)


def tiles_of(order, gx):
    order = np.asarray(order, np.int64)
    return (order >> 16) * gx + (order & 0xffff)


def permutation_errors(order, n, gx):
    """O1: a bijection from the n positions onto the n tiles."""
    t = tiles_of(order[:n], gx)
    if not ((t >= 0) & (t < n)).all():
        return "positions %s hold tiles outside [0, %d): %s" % (np.flatnonzero((t < 0) | (t >= n))[:5], n, order[:n][(t < 0) | (t >= n)][:5])
    if not ((np.asarray(order[:n], np.int64) & 0xffff) < gx).all():
        return "a tile's tx is not below gx"
    seen = np.bincount(t, minlength=n)
    if not (seen == 1).all():
        return "tiles %s are dealt %s times" % (np.flatnonzero(seen != 1)[:5], seen[seen != 1][:5])
    return None


def order_class(cost):
    """rtx_order_tiles' class of a cost, 0 the heaviest: floor((hi - c) 1024 / (hi - lo + 1)) in exact integers."""
    c = [int(v) for v in np.asarray(cost)]
    lo, hi = min(c), max(c)
    return np.array([((hi - v) * 1024) // (hi - lo + 1) for v in c], np.int64)


def rank_of_position(n, n_cu, first_round):
    """The boustrophedon of rtx_order_tiles undone: which rank each dispatch position holds.  Whole rounds only, and (the launch
    rule) none past n."""
    first_round = min(first_round, n)
    rounds = first_round // n_cu if n_cu else 0
    pos = np.arange(n)
    if not rounds:
        return pos
    k, c = pos // n_cu, pos % n_cu
    return np.where((pos < rounds * n_cu) & (k % 2 == 1), k * n_cu + (n_cu - 1 - c), pos)


def order_errors(cost, n, gx, n_cu, first_round, order):
    """O2 (after O1): classes non-decreasing along the ranks, every class holding exactly its tiles."""
    cls = order_class(cost[:n])
    by_rank = np.empty(n, np.int64)
    by_rank[rank_of_position(n, n_cu, first_round)] = tiles_of(order[:n], gx)
    along = cls[by_rank]
    if (np.diff(along) < 0).any():
        i = int(np.flatnonzero(np.diff(along) < 0)[0])
        return "rank %d holds class %d, rank %d class %d" % (i, along[i], i + 1, along[i + 1])
    if not (along == np.sort(cls)).all():
        return "the classes along the ranks are not the classes of the tiles"
    return None


def label_order_errors(cost, n, gx, base, order):
    """O3 (after O1): per label L the tiles at the positions = L (mod 8) are the base's, their 128 classes non-decreasing."""
    cls = order_class(cost[:n]) >> 3
    got, want = tiles_of(order[:n], gx), tiles_of(base[:n], gx)
    for L in range(min(8, n)):
        if sorted(got[L::8]) != sorted(want[L::8]):
            return "label %d does not keep its tiles" % L
        along = cls[got[L::8]]
        if (np.diff(along) < 0).any():
            return "label %d: classes fall along its positions: %s" % (L, along[:12])
    return None


def sim_order(cost, n, gx, n_cu, first_round, base=None):
    """The order from a plain sort (ties by tile number): for the host test of the judges above."""
    cls = order_class(cost[:n])
    pack = lambda t: (t % gx) | ((t // gx) << 16)
    out = np.zeros(n, np.int64)
    if base is None:
        by_rank = np.lexsort((np.arange(n), cls))
        out[np.arange(n)] = pack(by_rank[rank_of_position(n, n_cu, first_round)])
        return out.astype(np.uint32)
    bt = tiles_of(base[:n], gx)
    for L in range(min(8, n)):
        mine = bt[L::8]
        out[L::8] = pack(mine[np.lexsort((mine, cls[mine] >> 3))])
    return out.astype(np.uint32)


# ---------------------------------------------------------------------------------------------- rtx_balance_tiles

BALANCE_G = (1, 2, 255, 256, 1024)
BALANCE_GX = 64
STAMP_KINDS = ("plausible", "wrap", "zero", "end-before-start", "a-second")
PREV_KINDS = ("none", "permutation", "zero", "out-of-range", "output")
K_SETUP, K_BINS, DAMPING, MAX_STEP = 1800, 1024, 0.7, 0.18   # rtx_order_kernels.inc: kCostSetup, kBalanceBins; the launch rule's constants


def balance_n(G):
    return sorted({n for n in (1, 2, G - 1, G, G + 1, 2 * G, 2047, 2048) if 1 <= n <= 2048})


def group_durations(n, G, rng, slow=None):
    """Ticks each group took: 1700 .. 2300, and `slow` twice the mean of all groups (the launch's n_cu = G groups: those without a
    dispatch position have no duration)."""
    live = min(n, G)
    d = rng.integers(1700, 2300, live).astype(np.int64)
    if slow is not None and live > 2:
        # x = 2 (sum of the others + x) / G
        d[slow] = int(round(2.0 * (d.sum() - d[slow]) / (G - 2.0))) if G > 2 else d[slow]
    return d


def stamps(kind, n, G, rng, dur=None, t_ref=1_000_000):
    """(start, end) by dispatch position, uint32.  plausible / wrap: group g = p mod G runs from s_g to s_g + dur[g], its first
    position starting and its last ending it; position 0, whose start is the kernel's reference, is not the first to start."""
    p = np.arange(n)
    g = p % G
    if kind in ("plausible", "wrap"):
        dur = group_durations(n, G, rng) if dur is None else dur
        base = t_ref if kind == "plausible" else (1 << 32) - 900
        s_g = base + rng.integers(0, 30, len(dur))
        s_g[0] = base + 40
        rnd = p // G
        last = (n - 1 - g) // G
        t0 = s_g[g] + 3 * rnd
        t1 = np.where(rnd == last, s_g[g] + dur[g], s_g[g] + dur[g] - 7 - rnd)
    elif kind == "zero":
        t0 = t1 = np.zeros(n, np.int64)
    elif kind == "end-before-start":
        t0 = t_ref + rng.integers(0, 50, n)
        t1 = t0 - 5000
    else:
        assert kind == "a-second"
        t0 = t_ref + rng.integers(0, 50, n)
        t1 = t0 + 200_000_000
    return (np.asarray(t0, np.int64) % (1 << 32)).astype(np.uint32), (np.asarray(t1, np.int64) % (1 << 32)).astype(np.uint32)


def factors_in(kind, n, rng):
    if kind == "odd":      # NaN, inf, 0, 3, negative among valid ones
        f = rng.uniform(0.5, 2.0, n)
        odd = (float("nan"), float("inf"), 0.0, 3.0, -1.0, 0.49, 2.01)
        for i in range(0, n, 3):
            f[i] = odd[(i // 3) % len(odd)]
        return f.astype(F32)
    if kind == "edges":    # at and near the clamp: a slow group's step leaves [0.5, 2] without it
        return np.resize(np.array([2.0, 0.5, 1.95, 0.52, 1.0], F32), n)
    assert kind == "valid"
    return rng.uniform(0.6, 1.8, n).astype(F32)


def previous(kind, n, gx, rng):
    """(prev array or None, it is the output buffer itself)."""
    if kind == "none":
        return None, False
    if kind == "zero":
        return np.zeros(n, np.uint32), False
    if kind == "out-of-range":
        return np.full(n, 0xfffeffff, np.uint32), False
    t = rng.permutation(n)
    packed = ((t % gx) | ((t // gx) << 16)).astype(np.uint32)
    return packed, kind == "output"


def sanitised(f_in, have_factor, n):
    f = np.asarray(f_in[:n], np.float64) if have_factor else np.ones(n)
    with np.errstate(invalid="ignore"):
        return np.where((f >= 0.5) & (f <= 2.0), f, 1.0)


def expected_factors(cost3, n, gx, G, prev, f_in, have_factor, have_times):
    """O4 in float64: the factors out, for a previous order that is a permutation (or none: frame order)."""
    f = sanitised(f_in, have_factor, n)
    if not have_times:
        return f
    c = np.asarray(cost3, np.int64)
    ref = c[n]
    rel = lambda t: ((t - ref + (1 << 31)) % (1 << 32)) - (1 << 31)   # the difference as a signed 32-bit number
    t0, t1 = rel(c[n:2 * n]), rel(c[2 * n:3 * n])
    dur = np.zeros(G)
    for g in range(min(G, n)):
        d = float(t1[g::G].max() - t0[g::G].min())
        dur[g] = d if 0.0 < d < 1.0e8 else 0.0
    mean = dur.sum() / G
    if not mean > 0.0:
        return f
    ran = np.arange(n) if prev is None else tiles_of(prev[:n], gx)
    assert sorted(ran) == list(range(n))
    d = dur[np.arange(n) % G]
    r = np.clip(1.0 + DAMPING * (d / mean - 1.0), 1.0 - MAX_STEP, 1.0 + MAX_STEP)
    out = f.copy()
    out[ran] = np.where(d > 0.0, np.clip(f[ran] * r, 0.5, 2.0), f[ran])
    return out


def balance_classes(cost, n, f_out):
    """The corrected costs and their classes as rtx_balance_tiles forms them, in numpy float32: c' = (float)(c < 2^24 ? c + 1800 :
    2^24) * f (one multiply); class = (uint)((float)(hi - (uint)c') * to_bin), capped at 1023, hi / lo the largest / smallest
    (uint)c', to_bin = 1024 / ((float)(hi - lo) + 1)."""
    c = np.asarray(cost[:n], np.int64)
    corrected = np.where(c < (1 << 24), c + K_SETUP, 1 << 24).astype(F32) * np.asarray(f_out[:n], F32)
    u = corrected.astype(np.int64)     # (truncation, as the conversion to uint32)
    lo, hi = int(u.min()), int(u.max())
    to_bin = F32(K_BINS) / (F32(hi - lo) + F32(1.0))
    cls = np.minimum(((hi - u).astype(F32) * to_bin).astype(np.int64), K_BINS - 1)
    return corrected, cls


def dealing_errors(cost, n, gx, G, order, f_out):
    """O5 (after O1), from the outputs alone."""
    corrected, cls = balance_classes(cost, n, f_out)
    t = tiles_of(order[:n], gx)
    rounds = (n + G - 1) // G
    tail0 = (rounds - 1) * G
    ranked = np.sort(cls)                  # class by rank
    got = cls[t]                           # class by position
    if not (got[tail0:] == ranked[tail0:]).all():
        k = int(np.flatnonzero(got[tail0:] != ranked[tail0:])[0])
        return "the last round's position %d holds class %d, rank %d has class %d" % (tail0 + k, got[tail0 + k], tail0 + k, ranked[tail0 + k])
    c64 = corrected.astype(np.float64)
    total = float(c64.sum())
    two_classes = 2.0 * 1.25 * total / (K_BINS * G)
    top = 1.25 * total / G * (1.0 - 1.0 / K_BINS)    # sums from here on share the last sum class: their order is the atomics'
    sums = np.zeros(G)
    sums[:n - tail0] = c64[t[tail0:]]
    for r in range(rounds - 1):
        here = got[r * G:(r + 1) * G]
        if sorted(here) != list(ranked[r * G:(r + 1) * G]):
            return "round %d does not hold the ranks [%d, %d)" % (r, r * G, (r + 1) * G)
        # the group with the smaller sum holds an equal or heavier class: along rising sums, no class may exceed the smallest
        # class among the groups more than two sum classes further up
        by_sum = np.argsort(sums, kind="stable")
        s, k = sums[by_sum], here[by_sum]
        floor_after = np.minimum.accumulate(k[::-1])[::-1]          # smallest class among groups i, i + 1, ...
        first_clear = np.searchsorted(s, s + two_classes, side="right")
        judged = (first_clear < G) & (s < top)
        bad = judged & (k > floor_after[np.minimum(first_clear, G - 1)])
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            return "round %d: group %d (sum %.1f) takes class %d, a group with a larger sum a heavier one" % (r, by_sum[i], s[i], k[i])
        sums += c64[t[r * G:(r + 1) * G]]
    return None


def sim_balance(cost, n, gx, G, f_out):
    """The dealing from plain sorts (ties by number), given the factors: for the host test of dealing_errors."""
    corrected, cls = balance_classes(cost, n, f_out)
    by_rank = np.lexsort((np.arange(n), cls))
    rounds = (n + G - 1) // G
    tail0 = (rounds - 1) * G
    c64 = corrected.astype(np.float64)
    at = np.zeros(n, np.int64)
    at[tail0:] = by_rank[tail0:]
    sums = np.zeros(G)
    sums[:n - tail0] = c64[by_rank[tail0:]]
    for r in range(rounds - 1):
        k_of_group = np.empty(G, np.int64)
        k_of_group[np.argsort(sums, kind="stable")] = np.arange(G)
        at[r * G:(r + 1) * G] = by_rank[r * G + k_of_group]
        sums += c64[at[r * G:(r + 1) * G]]
    return ((at % gx) | ((at // gx) << 16)).astype(np.uint32)
