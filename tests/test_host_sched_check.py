"""tests/sched_cases.py without a GPU: from float64 alone, every coarse-cell scene that tests/test_gpu_sched_check.py runs on the
device decides enough of its (cell, sphere) pairs, each way, and holds the mechanisms it is there for; and the numpy class
functions and judges of the dispatch orders accept the orders a plain sort deals and refuse the identity."""
import numpy as np
import pytest

import sched_cases as SC

F32 = np.float32


# ---------------------------------------------------------------------------------------------- coarse-cell scenes

def test_shapes_are_the_smallest_with_each_mechanism():
    s = SC.SHAPES
    assert (s["16x16"].cells_x, s["16x16"].cells_y, s["16x16"].n_blocks, s["16x16"].slots_beyond_the_grid()) == (5, 3, 2, 17)
    # (two blocks of sixteen slots for fifteen cells: block 0 holds 12 cells and 4 slots below the grid, block 1 three cells)
    assert (s["wide"].cw, s["wide"].ch, s["wide"].cells_x, s["wide"].cells_y) == (32, 16, 3, 3)          # non-square, the last column cut
    assert (s["nsub4"].cw, s["nsub4"].ch, s["nsub4"].cells_x, s["nsub4"].cells_y) == (32, 32, 3, 2)
    assert (s["64x4"].cw, s["64x4"].ch, s["64x4"].cells_x, s["64x4"].cells_y, s["64x4"].n_blocks) == (64, 4, 2, 12, 3)
    assert sorted(SC.Scene(n).ns for n in SC.SCENES) == [1, 511, 512, 513, 1700, 5000]
    assert {SC.SCENES[n][1] for n in SC.SCENES} == {"default", "rolled"} and {SC.SCENES[n][2] for n in SC.SCENES} == set(SC.BUDGETS)
    assert SC.planned_splits(5000, 2) == 5 and SC.planned_splits(1700, 2) == 2 and SC.planned_splits(513, 1) == 1
    slab = s["16x16"].slab(16)
    assert (slab.cells_y, slab.full_rect(0)) == (2, s["16x16"].full_rect(5))


@pytest.mark.parametrize("name", SC.JUDGED)
def test_float64_decides_the_scene(name):
    """The condition on the inputs: at most 5 % of the pairs decided by neither rule, at least 50 decided each way, a cell whose
    list must exceed the smallest capacity."""
    sc = SC.scene(name)
    near, beyond = sc.judged()
    pairs = near.size
    undecided = ~near & ~beyond
    print("%s: %d pairs: %d must be listed, %d must not, %d undecided (%.2f %%)" % (name, pairs, near.sum(), beyond.sum(), undecided.sum(), 100.0 * undecided.sum() / pairs))
    assert not (near & beyond).any()
    assert undecided.sum() <= 0.05 * pairs, (int(undecided.sum()), pairs)
    assert near.sum() >= 50 and beyond.sum() >= 50
    assert near.sum(1).max() > min(c for c in SC.CAPS if c)
    # the kinds: the covering sphere in every cell, the spheres behind the camera in none, the never-culled ones never beyond
    kind = sc.kind
    assert near[:, kind == "cover"].all() and beyond[:, kind == "behind"].all() and (kind == "behind").sum() == 3
    assert len(sc.always_listed()) == 4 and not beyond[:, sc.always_listed()].any()
    assert (sc.sph[kind == "r<=0", 3] == 0).sum() == 2 and (sc.sph[kind == "r<=0", 3] < 0).sum() == 2
    # the directed ones straddle the planes of their cells: of a cell's 60, those pushed by less than a margin are not beyond its
    # planes (s = 0.5, 0.9 without r added: 4 planes x 2 x 1.5 on average), the others are
    assert len(sc.targets) >= 1
    for c in sc.targets:
        d = sc.aimed == c
        assert d.sum() == 60 and beyond[c, d].sum() >= 20 and (~beyond[c, d]).sum() >= 10, (c, int(beyond[c, d].sum()))


def test_a_block_passes_the_flush_threshold():
    """More than 512 spheres of the first 1536 reach block 0 (cells 0..3 of every row) in the 1700- and the 5000-sphere scene: with
    one workgroup per block the survivor buffer is flushed before the walk ends.  The float64 `near` rule is a lower bound."""
    for name in ("n1700", "n5000"):
        sc = SC.scene(name)
        near, _ = sc.judged()
        block0 = [c for c in range(sc.shape.n_cells) if c % sc.shape.cells_x < 4]
        assert near[block0][:, :1536].any(0).sum() > 512, name


def test_later_cameras_exist_for_the_budget_scenes():
    for name in SC.JUDGED:
        sc = SC.scene(name)
        if sc.theta > 0:
            pyr = SC.CG.Pyramid(sc.cam, sc.shape.full_rect(sc.shape.n_cells // 2))
            kinds = {k for k, _, _ in SC.CG.later_cameras(sc.cam, pyr.n, sc.theta, sc.delta, np.random.default_rng(1))}
            assert kinds == {"rotation", "translation", "mix"}


# ---------------------------------------------------------------------------------------------- dispatch orders

def test_order_class_is_the_plain_formula():
    rng = np.random.default_rng(3)
    for kind in SC.COST_KINDS:
        c = SC.costs(kind, 1025, rng)
        cls = SC.order_class(c)
        assert cls.min() >= 0 and cls.max() <= 1023 and cls[np.argmax(c)] == 0
        assert (np.diff(cls[np.argsort(-c.astype(np.int64), kind="stable")]) >= 0).all()   # heavier cost, lower or equal class
    assert (SC.order_class(np.array([7, 7, 7], np.uint32)) == 0).all()


@pytest.mark.parametrize("n", SC.ORDER_N)
def test_order_judges_accept_a_plain_sort_and_refuse_the_identity(n):
    rng = np.random.default_rng(n)
    gx = SC.GRID_OF[n][0]
    identity = ((np.arange(n) % gx) | ((np.arange(n) // gx) << 16)).astype(np.uint32)
    for n_cu in (0, 1, 256, n + 3):
        for first_round in (0, n_cu, 7 * n_cu, n + 5):
            r = SC.rank_of_position(n, n_cu, first_round)
            assert sorted(r) == list(range(n))
            for kind in ("ascending", "random", "giant", "equal"):
                c = SC.costs(kind, n, rng)
                o = SC.sim_order(c, n, gx, n_cu, first_round)
                assert SC.permutation_errors(o, n, gx) is None and SC.order_errors(c, n, gx, n_cu, first_round, o) is None
            if n > 8:
                assert SC.order_errors(SC.costs("ascending", n, rng), n, gx, n_cu, first_round, identity) is not None
    # rounds are undone in whole: 7 x 256 ranks of 1025 tiles become 4 rounds, of which the second and fourth run backwards
    r = SC.rank_of_position(1025, 256, 7 * 256)
    assert (r[:256] == np.arange(256)).all() and (r[256:512] == np.arange(511, 255, -1)).all() and (r[1024:] == 1024).all()
    # with a base: any permutation that keeps cells to labels will do here (the device test takes rtxplan::xcd_cell_order's)
    base = identity[rng.permutation(n)]
    c = SC.costs("random", n, rng)
    o = SC.sim_order(c, n, gx, 0, 0, base)
    assert SC.permutation_errors(o, n, gx) is None and SC.label_order_errors(c, n, gx, base, o) is None
    if n > 64:
        assert SC.label_order_errors(c, n, gx, base, base) is not None and SC.label_order_errors(c, n, gx, base, np.roll(o, 1)) is not None
    bad = o.copy()
    bad[0] = bad[n - 1]
    assert (SC.permutation_errors(bad, n, gx) is not None) == (n > 1)


@pytest.mark.parametrize("G", SC.BALANCE_G)
def test_dealing_judge_accepts_a_plain_sort_and_refuses_the_identity(G):
    rng = np.random.default_rng(G)
    gx = SC.BALANCE_GX
    for n in SC.balance_n(G):
        for kind in SC.COST_KINDS:
            c = SC.costs(kind, n, rng)
            f = rng.uniform(0.5, 2.0, n).astype(F32)
            o = SC.sim_balance(c, n, gx, G, f)
            assert SC.permutation_errors(o, n, gx) is None
            assert SC.dealing_errors(c, n, gx, G, o, f) is None, (n, kind, SC.dealing_errors(c, n, gx, G, o, f))
        if n >= 64:
            c = SC.costs("ascending", n, rng) * np.uint32(50)
            identity = ((np.arange(n) % gx) | ((np.arange(n) // gx) << 16)).astype(np.uint32)
            assert SC.dealing_errors(c, n, gx, G, identity, np.ones(n, F32)) is not None
            if G in (255, 256) and n >= 2 * G:
                # heaviest first but dealt in frame order, every round: the sums drift apart and the judge sees it
                _, cls = SC.balance_classes(c, n, np.ones(n, F32))
                by_rank = np.lexsort((np.arange(n), cls))
                o = ((by_rank % gx) | ((by_rank // gx) << 16)).astype(np.uint32)
                assert SC.dealing_errors(c, n, gx, G, o, np.ones(n, F32)) is not None


def test_expected_factors():
    rng = np.random.default_rng(9)
    n, G, gx = 2047, 256, SC.BALANCE_GX
    c = SC.costs("random", n, rng)
    f_in = SC.factors_in("odd", n, rng)
    clean = SC.sanitised(f_in, 1, n)
    assert ((clean >= 0.5) & (clean <= 2.0)).all() and (clean[np.isnan(f_in)] == 1.0).all() and (SC.sanitised(f_in, 0, n) == 1.0).all()
    for kind in ("zero", "end-before-start", "a-second"):
        t0, t1 = SC.stamps(kind, n, G, rng)
        assert (SC.expected_factors(np.concatenate([c, t0, t1]), n, gx, G, None, f_in, 1, 1) == clean).all(), kind
    dur = SC.group_durations(n, G, rng, slow=5)
    assert abs(dur[5] / (dur.sum() / G) - 2.0) < 1e-3
    out = {}
    for kind in ("plausible", "wrap"):
        t0, t1 = SC.stamps(kind, n, G, np.random.default_rng(4), dur)
        assert (kind == "wrap") == bool((t1 < t0).any())      # the wrap is straddled
        assert (t0[1:G].astype(np.int64) - int(t0[0]) < 0).any() or kind == "wrap"   # position 0 is not the first to start
        out[kind] = SC.expected_factors(np.concatenate([c, t0, t1]), n, gx, G, None, f_in, 1, 1)
    assert (out["plausible"] == out["wrap"]).all()
    slow = np.arange(n) % G == 5
    assert np.allclose(out["plausible"][slow], np.clip(clean[slow] * 1.18, 0.5, 2.0)) and (out["plausible"][~slow] != clean[~slow]).any()
    # without the clamp the edge factors would leave [0.5, 2]
    edges = SC.sanitised(SC.factors_in("edges", n, rng), 1, n)
    assert (edges[slow] * 1.18 > 2.0).any()
