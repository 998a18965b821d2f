"""The three passes in front of every culled trace launch -- rtx_bin_cells, rtx_order_tiles, rtx_balance_tiles -- run on the GPU on
inputs made for them (tests/gpu_checks/sched_check.hip: the production text of csrc/rtx_bin_cells.inc and
csrc/rtx_order_kernels.inc, launched through the production rules) and held to float64, to the production hit test and to the
orders their comments promise.  Inputs and yardsticks: tests/sched_cases.py, proved on the CPU by tests/test_host_sched_check.py.

Coarse-cell lists (none has exceptions):
  B1  counts are the same for every capacity, split and permutation of the sphere array; the first min(count, cap) entries of a
      cell are distinct, below ns and among the set the large-capacity run lists; every other word of the buffers keeps its poison;
  B2  one listed set per cell under splits 1 / planned / 3, a reversed and a shuffled sphere array, with and without sph_pos_of,
      and for a slab (row0 > 0) against the same cells of the whole frame;
  B3  sound: a sphere some pixel of the cell hits under the production test (rtx_check_rect_hits of libcull_check.so) is listed; so
      is one a float64 pixel half-line passes within |r| (1 - 1e-5); a camera inside or on a sphere, a NaN centre and an infinite
      radius are listed in every cell; with a budget, what is not listed is hit from no later camera the budget admits (M);
  B4  tight: a centre beyond a float64 plane of the cell by more than margin (1 + 1e-4) + 2e-6 |O| is not listed;
  B5  cell_max_out ends as max(its initial value, the largest count among cells whose count exceeds cap >> 1); the other counter
      buffer is zero in every cell of the grid and untouched behind it.
Dispatch orders:
  O1  every output is a bijection from the n positions onto the n tiles, whatever the inputs hold, and nothing is written behind
      the n words; refused arguments launch nothing;
  O2  rtx_order_tiles: classes non-decreasing along the ranks, the boustrophedon of whole rounds undone;
  O3  ... with a base (rtxplan::xcd_cell_order): every label keeps its tiles, their 128 classes non-decreasing along its positions;
  O4  rtx_balance_tiles: factors out in [0.5, 2], equal to the sanitised factors in without usable times, and
      clamp(f clamp(1 + 0.7 (d / mean - 1), 1 +- 0.18), 0.5, 2) to 1e-4 relative with them (mean: a float sum of at most 1024
      terms in the kernel's order, 1024 x 2^-24 = 6e-5); the wrap of the 32-bit clock changes nothing;
  O5  ... the dealing, from the outputs alone: whole rounds of ranks, the lightest tiles last, the smaller sum the heavier tile.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sched_cases as SC
from cull_geometry import F32, Pyramid, later_cameras, moved_spheres
from test_gpu_cull_bound import Lib as CullLib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON = SC.POISON


class Lib:
    """ctypes face of libsched_check.so."""

    def __init__(self, so):
        self.so = so
        for fn in (so.rtx_check_order_tiles, so.rtx_check_balance_tiles, so.rtx_check_bin_cells, so.rtx_check_xcd_cell_order):
            fn.restype = C.c_int

    @staticmethod
    def _p(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def order(self, cost, n, gx, n_cu, first_round, base=None, guard=None):
        """-> (status, the n + guard words of the order buffer, poisoned before the launch)."""
        guard = n + n_cu + 64 if guard is None else guard
        out = np.full(n + guard, POISON, np.uint32)
        rc = self.so.rtx_check_order_tiles(self._p(cost), C.c_uint(n), C.c_uint(gx), C.c_uint(n_cu), C.c_uint(first_round), self._p(base), self._p(out), C.c_uint(guard))
        return rc, out

    def balance(self, cost3, n, gx, G, prev, prev_is_order, f_in, have_factor, have_times, guard=2048):
        """-> (status, order buffer, factor buffer), each n + guard words."""
        out = np.full(n + guard, POISON, np.uint32)
        if prev_is_order:
            out[:n] = prev
        fac = np.full(n + guard, -7.0, F32)
        fac[:n] = f_in[:n]
        rc = self.so.rtx_check_balance_tiles(self._p(cost3), C.c_uint(n), C.c_uint(gx), C.c_uint(G), None if prev_is_order else self._p(prev),
                                             C.c_int(int(prev_is_order)), self._p(fac), C.c_int(have_factor), C.c_int(have_times), self._p(out), C.c_uint(guard))
        return rc, out, fac

    def xcd_cell_order(self, grid_x, grid_y, gx, gy):
        out = np.zeros(grid_x * grid_y, np.uint32)
        assert self.so.rtx_check_xcd_cell_order(C.c_uint(grid_x), C.c_uint(grid_y), C.c_uint(gx), C.c_uint(gy), self._p(out)) == 0
        return out

    def bin(self, cam, shape, cap, theta, delta, sph, splits, pos_of=None, max_init=0):
        """-> counts, lists, zeroed, cell_max.  The counters start at zero as the product's do; lists and every guard are poisoned,
        the other counter buffer holds garbage."""
        cells = shape.n_cells
        guard = 16 * cap + 64
        counts = np.full(cells + guard, POISON, np.uint32)
        counts[:cells] = 0
        lists = np.full(cells * cap + guard, POISON, np.uint32)
        zeroed = np.full(cells + guard, SC.GARBAGE, np.uint32)
        cell_max = np.array([max_init], np.uint32)
        sph = np.ascontiguousarray(sph, F32)
        rc = self.so.rtx_check_bin_cells(self._p(cam.packed), C.c_uint(cam.W), C.c_uint(cam.H), self._p(shape.words(cap)), C.c_float(theta), C.c_float(delta),
                                         self._p(sph), C.c_uint(len(sph)), self._p(pos_of), C.c_uint(splits), self._p(counts), self._p(lists), self._p(zeroed),
                                         self._p(cell_max), C.c_uint(guard))
        assert rc == 0, rc
        assert (counts[cells:] == POISON).all() and (lists[cells * cap:] == POISON).all() and (zeroed[cells:] == SC.GARBAGE).all(), "a guard word was written"
        return counts[:cells], lists[:cells * cap], zeroed[:cells], int(cell_max[0])


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    # (RTX_SCHED_CHECK_LIB: another build of the library -- profiles/r28_sched_check.txt ran this file over mutated ones)
    path = os.environ.get("RTX_SCHED_CHECK_LIB") or os.path.join(HERE, "gpu_checks", "libsched_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    return Lib(C.CDLL(path))


@pytest.fixture(scope="module")
def cull():
    import torch  # noqa: F401
    path = os.path.join(HERE, "gpu_checks", "libcull_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    return CullLib(C.CDLL(path))


# ---------------------------------------------------------------------------------------------- coarse-cell lists

_REFERENCE = {}


def reference(lib, name):
    """The large-capacity run of a scene at its planned split, once: (counts, sets)."""
    if name not in _REFERENCE:
        sc = SC.scene(name)
        cap = sc.ns
        counts, lists, _, _ = lib.bin(sc.cam, sc.shape, cap, sc.theta, sc.delta, sc.sph, SC.planned_splits(sc.ns, sc.shape.n_blocks))
        _REFERENCE[name] = (counts.copy(), SC.sets_of(counts, lists, sc.shape.n_cells, cap, sc.ns))
    return _REFERENCE[name]


def well_formed(sc, cap, counts, lists, ref_counts, ref_sets, translate=None):
    """B1 for one run; returns the listed sets where the capacity held them (else None per cell)."""
    n_cells = sc.shape.n_cells
    assert (counts == ref_counts).all(), ("counts differ", counts, ref_counts)
    sets = []
    for c in range(n_cells):
        held = min(int(counts[c]), cap)
        mine = lists[c * cap:c * cap + held].astype(np.int64)
        assert (lists[c * cap + held:(c + 1) * cap] == POISON).all(), ("cell %d: a word at or past its entries was written" % c)
        assert (mine < sc.ns).all() and len(set(mine.tolist())) == held, ("cell %d: entries repeat or are not below ns" % c, mine[:10])
        if translate is not None:
            mine = translate[mine]
        assert set(mine.tolist()) <= ref_sets[c], ("cell %d lists %s, which the large-capacity run does not" % (c, sorted(set(mine.tolist()) - ref_sets[c])[:5]))
        sets.append(frozenset(mine.tolist()) if counts[c] <= cap else None)
    return sets


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_lists_are_well_formed_and_one_set(lib, name):
    """B1, B2, B5."""
    sc = SC.scene(name)
    sh, ns = sc.shape, sc.ns
    ref_counts, ref_sets = reference(lib, name)
    planned = SC.planned_splits(ns, sh.n_blocks)
    rng = np.random.default_rng(ns)
    print("B %s: %d cells, counts %d .. %d, planned split %d" % (name, sh.n_cells, ref_counts.min(), ref_counts.max(), planned))
    assert (ref_counts > 0).all()
    for cap in (1, 7, ns):
        for splits in (1, planned, 3):
            for max_init in (0, 1 << 20):
                if max_init and splits != planned:
                    continue
                counts, lists, zeroed, cell_max = lib.bin(sc.cam, sh, cap, sc.theta, sc.delta, sc.sph, splits, max_init=max_init)
                sets = well_formed(sc, cap, counts, lists, ref_counts, ref_sets)
                if cap == ns:
                    assert sets == ref_sets, ("splits %d lists another set" % splits)
                # B5
                over = ref_counts[ref_counts > (cap >> 1)]
                assert cell_max == max(max_init, int(over.max()) if len(over) else 0), (cap, splits, max_init, cell_max)
                assert (zeroed == 0).all(), "the other counter buffer is not zero in every cell"
    # permutations of the sphere array: the flush and split boundaries fall elsewhere
    for perm in (np.arange(ns)[::-1], rng.permutation(ns)):
        for cap in (7, ns):
            counts, lists, _, _ = lib.bin(sc.cam, sh, cap, sc.theta, sc.delta, sc.sph[perm], planned)
            sets = well_formed(sc, cap, counts, lists, ref_counts, ref_sets, translate=perm)
            assert cap != ns or sets == ref_sets, "a permuted sphere array lists another set"
    # sph_pos_of: entries are pos_of[creation index]
    pos_of = rng.permutation(ns).astype(np.uint32)
    inverse = np.argsort(pos_of)
    for cap in (7, ns):
        counts, lists, _, _ = lib.bin(sc.cam, sh, cap, sc.theta, sc.delta, sc.sph, planned, pos_of=pos_of)
        sets = well_formed(sc, cap, counts, lists, ref_counts, ref_sets, translate=inverse)
        assert cap != ns or sets == ref_sets, "sph_pos_of changes the listed set"
    # a slab: the same cells of the whole frame
    if sh.row0 == 0 and sh.cells_y > 1:
        slab = sh.slab(sh.ch)
        counts, lists, zeroed, _ = lib.bin(sc.cam, slab, ns, sc.theta, sc.delta, sc.sph, planned)
        assert (zeroed == 0).all()
        assert SC.sets_of(counts, lists, slab.n_cells, ns, ns) == ref_sets[sh.cells_x:], "a slab lists another set than the same cells of the frame"


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_lists_are_sound_and_tight(lib, cull, name):
    """B3, B4, M."""
    sc = SC.scene(name)
    sh, ns = sc.shape, sc.ns
    _, ref_sets = reference(lib, name)
    listed = np.zeros((sh.n_cells, ns), bool)
    for c, s in enumerate(ref_sets):
        listed[c, list(s)] = True
    near, beyond = sc.judged()
    rects = sc.rects()
    pairs = np.array([(c, s) for c in range(sh.n_cells) for s in range(ns)], np.uint32)
    hit = cull.rect_hits(sc.cam, rects, sc.sph, pairs).reshape(sh.n_cells, ns) != 0
    print("B %s: %d pairs: %d listed, %d hit by a pixel, %d near in float64, %d beyond a plane" % (name, listed.size, listed.sum(), hit.sum(), near.sum(), beyond.sum()))
    assert hit.sum() >= min(50, listed.size)
    assert not (hit & ~listed).any(), ("hit by a pixel and not listed", np.argwhere(hit & ~listed)[:5])
    assert not (near & ~listed).any(), ("within r of a float64 pixel half-line and not listed", np.argwhere(near & ~listed)[:5])
    assert listed[:, sc.always_listed()].all(), "a sphere that is never culled is missing from a cell"
    assert not (beyond & listed).any(), ("beyond a float64 plane and listed", np.argwhere(beyond & listed)[:5])
    if sc.theta > 0.0:
        rng = np.random.default_rng(ns + 1)
        normals = Pyramid(sc.cam, sh.full_rect(sh.n_cells // 2)).n
        out = pairs[~listed.ravel()]
        n_hit_now = 0
        for kind, now, drift in later_cameras(sc.cam, normals, sc.theta, sc.delta, rng):
            used_theta, used_delta = cull.cell_motion(sc.cam, now, 0.0, drift)
            assert used_theta <= float(F32(sc.theta)) and used_delta <= float(F32(sc.delta)), (kind, used_theta, used_delta)
            moved = moved_spheres(sc.sph, drift, rng)
            late = cull.rect_hits(now, rects, moved, out)
            assert (late != 0).sum() == 0, ("not listed, and hit from a later camera (%s)" % kind, out[late != 0][:5])
            n_hit_now += int((cull.rect_hits(now, rects, moved, pairs[listed.ravel()][::7]) != 0).sum())
        assert n_hit_now > 0  # (the later cameras do see the scene)


# ---------------------------------------------------------------------------------------------- rtx_order_tiles

def check_order(lib, cost, n, gx, n_cu, first_round, base, what):
    rc, out = lib.order(cost, n, gx, n_cu, first_round, base)
    assert rc == 0, (what, rc)
    assert (out[n:] == POISON).all(), (what, "words behind the order were written", np.flatnonzero(out[n:] != POISON)[:5] + n)
    err = SC.permutation_errors(out, n, gx)
    assert err is None, (what, err)
    err = SC.order_errors(cost, n, gx, n_cu, first_round, out) if base is None else SC.label_order_errors(cost, n, gx, base, out)
    assert err is None, (what, err)


@pytest.mark.parametrize("n", SC.ORDER_N)
def test_order_tiles_without_base(lib, n):
    """O1, O2."""
    rng = np.random.default_rng(n)
    gx = SC.GRID_OF[n][0]
    i = 0
    for n_cu in (0, 1, 256, n + 3):
        for first_round in (0, n_cu, 7 * n_cu, n + 5):
            kinds = SC.COST_KINDS if (n_cu, first_round) == (256, 7 * 256) else (SC.COST_KINDS[i % len(SC.COST_KINDS)],)
            for kind in kinds:
                check_order(lib, SC.costs(kind, n, rng), n, gx, n_cu, first_round, None, (n, n_cu, first_round, kind))
            i += 1


@pytest.mark.parametrize("n", SC.ORDER_N)
def test_order_tiles_with_base(lib, n):
    """O1, O3: the base orders are rtxplan::xcd_cell_order's, for cells of 2 x 2 and of 4 x 1 tiles."""
    rng = np.random.default_rng(n + 1)
    grid_x, grid_y = SC.GRID_OF[n]
    for cgx, cgy in ((1, 1), (2, 0)):
        base = lib.xcd_cell_order(grid_x, grid_y, cgx, cgy)
        assert SC.permutation_errors(base, n, grid_x) is None
        for kind in SC.COST_KINDS:
            check_order(lib, SC.costs(kind, n, rng), n, grid_x, 256, n, base, (n, cgx, cgy, kind))


def test_order_tiles_refuses(lib):
    """O1: n = 0, gx = 0, gx past 16 bits and more than 65 535 rows return the error; nothing is launched (the poison stays)."""
    cost = np.arange(70000, dtype=np.uint32)
    for n, gx in ((0, 4), (8, 0), (8, 0x10000), (70000, 1)):
        rc, out = lib.order(cost, n, gx, 256, 0, guard=64)
        assert rc == -2 and (out == POISON).all(), (n, gx, rc)
    rc, out = lib.order(cost, 65535, 1, 256, 0, guard=64)
    assert rc == 0 and SC.permutation_errors(out, 65535, 1) is None


# ---------------------------------------------------------------------------------------------- rtx_balance_tiles

def run_balance(lib, n, G, cost, t0, t1, prev_kind, f_in, have_factor, have_times, rng, what):
    """One launch, held to O1, the factors' range and O5; returns what went in and came out."""
    gx = SC.BALANCE_GX
    prev, is_out = SC.previous(prev_kind, n, gx, rng)
    cost3 = np.concatenate([cost, t0, t1]).astype(np.uint32)
    rc, out, fac = lib.balance(cost3, n, gx, G, prev, is_out, f_in, have_factor, have_times)
    assert rc == 0, (what, rc)
    assert (out[n:] == POISON).all() and (fac[n:] == F32(-7.0)).all(), (what, "words behind the outputs were written")
    err = SC.permutation_errors(out, n, gx)
    assert err is None, (what, err)
    f_out = fac[:n]
    assert ((f_out >= 0.5) & (f_out <= 2.0)).all(), (what, "factors outside [0.5, 2]", f_out[~((f_out >= 0.5) & (f_out <= 2.0))][:5])
    err = SC.dealing_errors(cost, n, gx, G, out, f_out)
    assert err is None, (what, err)
    return cost3, prev, f_out


@pytest.mark.parametrize("G", SC.BALANCE_G)
def test_balance_tiles_deals_a_permutation(lib, G):
    """O1, O5, the range of O4: every n, both flags both ways, costs, stamps, factors and previous orders in rotation."""
    rng = np.random.default_rng(G)
    i = 0
    for n in SC.balance_n(G):
        for have_factor in (0, 1):
            for have_times in (0, 1):
                for _ in range(2):
                    ck, sk, pk = SC.COST_KINDS[i % 8], SC.STAMP_KINDS[i % 5], SC.PREV_KINDS[(i // 2) % 5]
                    fk = ("odd", "edges", "valid")[i % 3]
                    t0, t1 = SC.stamps(sk, n, G, rng)
                    run_balance(lib, n, G, SC.costs(ck, n, rng), t0, t1, pk, SC.factors_in(fk, n, rng), have_factor, have_times, rng, (n, G, ck, sk, pk, fk))
                    i += 1


def test_balance_tiles_every_kind_of_input(lib):
    """O1, O5 at n = 2047, G = 256: every cost kind under every stamp kind and previous order."""
    rng = np.random.default_rng(77)
    n, G = 2047, 256
    for ck in SC.COST_KINDS:
        for sk in SC.STAMP_KINDS:
            for pk in SC.PREV_KINDS:
                t0, t1 = SC.stamps(sk, n, G, rng)
                run_balance(lib, n, G, SC.costs(ck, n, rng), t0, t1, pk, SC.factors_in("odd", n, rng), 1, 1, rng, (ck, sk, pk))


def test_balance_tiles_refuses(lib):
    """O1: n = 0, n > 2048, gx = 0, G = 0, G > 1024 return the error; nothing is launched."""
    cost3 = np.zeros(3 * 4096, np.uint32)
    f = np.ones(4096, F32)
    for n, gx, G in ((0, 64, 256), (2049, 64, 256), (64, 0, 256), (64, 64, 0), (64, 64, 1025)):
        rc, out, fac = lib.balance(cost3, n, gx, G, None, False, f, 1, 1, guard=64)
        assert rc == -2 and (out == POISON).all() and (fac[:n] == 1.0).all(), (n, gx, G, rc)


FACTOR_CASES = [(2047, 256), (2048, 1024), (700, 255), (9, 2), (5, 1), (100, 256), (1, 1024)]


@pytest.mark.parametrize("n,G", FACTOR_CASES, ids=["n%d-G%d" % c for c in FACTOR_CASES])
def test_balance_tiles_factors(lib, n, G):
    """O4.  (n < G: the groups without a dispatch position have no duration; the mean is over all G groups of the launch.)"""
    rng = np.random.default_rng(1000 * n + G)
    gx = SC.BALANCE_GX
    cost = SC.costs("random", n, rng)
    live = min(n, G)
    dur = SC.group_durations(n, G, rng, slow=live // 2)
    results = {}
    for fk in ("odd", "edges", "valid"):
        f_in = SC.factors_in(fk, n, rng)
        clean = SC.sanitised(f_in, 1, n)
        # without usable times: the factors in, sanitised -- no times at all, and nonsense durations
        for sk, have_times in (("plausible", 0), ("zero", 1), ("end-before-start", 1), ("a-second", 1)):
            t0, t1 = SC.stamps(sk, n, G, rng)
            _, _, f_out = run_balance(lib, n, G, cost, t0, t1, "permutation", f_in, 1, have_times, rng, (fk, sk, have_times))
            assert (f_out.astype(np.float64) == clean).all(), (fk, sk, have_times)
        _, _, f_out = run_balance(lib, n, G, cost, t0, t1, "none", f_in, 0, 0, rng, (fk, "no factors"))
        assert (f_out == 1.0).all()
        # synthetic stamps, one group at twice the mean; shifted across the wrap of the clock they give the same factors
        for sk in ("plausible", "wrap"):
            for pk in ("none", "permutation", "output"):
                t0, t1 = SC.stamps(sk, n, G, np.random.default_rng(5), dur)
                prev_rng = np.random.default_rng(6)
                cost3, prev, f_out = run_balance(lib, n, G, cost, t0, t1, pk, f_in, 1, 1, prev_rng, (fk, sk, pk))
                want = SC.expected_factors(cost3, n, gx, G, prev, f_in, 1, 1)
                err = np.abs(f_out.astype(np.float64) - want) / want
                print("O4 n %d G %d %s %s %s: worst relative error of a factor %.2e" % (n, G, fk, sk, pk, err.max()))
                assert err.max() <= 1.0e-4, (fk, sk, pk, int(err.argmax()), f_out[err.argmax()], want[err.argmax()])
                results[(fk, sk, pk)] = f_out.copy()
        for pk in ("none", "permutation", "output"):
            assert (results[(fk, "plausible", pk)] == results[(fk, "wrap", pk)]).all(), "the wrap of the clock changes the factors"
        if live > 2:
            # what the formula says of the slow group (in frame order position p ran tile p): up by the full step, or to the clamp
            slow = np.arange(n) % G == live // 2
            assert np.allclose(results[(fk, "plausible", "none")][slow], np.clip(clean[slow] * 1.18, 0.5, 2.0), rtol=1.0e-4)
        # one nonsense duration (group 0 a second long) changes nothing for its group, and the others follow the formula
        if live > 2:
            t0, t1 = SC.stamps("plausible", n, G, np.random.default_rng(5), dur)
            t1[0::G] = t0[0::G] + np.uint32(200_000_000)
            cost3, prev, f_out = run_balance(lib, n, G, cost, t0, t1, "none", f_in, 1, 1, rng, (fk, "one nonsense group"))
            want = SC.expected_factors(cost3, n, gx, G, None, f_in, 1, 1)
            assert (f_out[0::G].astype(np.float64) == clean[0::G]).all() and (np.abs(f_out - want) / want).max() <= 1.0e-4


def test_balance_tiles_equal_costs_without_times(lib):
    """O5's last line: equal costs and no times are still a permutation (every class but one is empty)."""
    rng = np.random.default_rng(8)
    for n, G in ((2048, 256), (2047, 1024), (300, 255), (2, 2), (1, 1)):
        t0 = t1 = np.zeros(n, np.uint32)
        run_balance(lib, n, G, SC.costs("equal", n, rng), t0, t1, "none", np.ones(n, F32), 0, 0, rng, (n, G))
