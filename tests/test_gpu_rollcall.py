"""Every object count at the trace kernels' staging and list edges (rtx_trace_body.inc, stage_chunk in rtx_kernels.hip), on the device.

The inputs are the roll-call scenes of tests/rollcall_cases.py: every object owns a pixel, so a kernel that loses any one item -- item
256 of a staging step, the last entry of a full list, the 129th candidate of a wave, plane 16 -- renders another frame; the counts
are swept across every threshold of the bookkeeping, for every plan of the trace kernel.  tests/test_host_rollcall.py has judged
the scenes on the CPU (every owner the nearest hit in float64 and in the oracle's frame, every stated candidate count certain).
The expected result is always the oracle's frame, byte for byte: no tolerance is involved.

RTX_OPT_VIEW_ADAPT, _TILE_ORDER and _XCD_ORDER are 0, so that the plan is the one asked for, and every launch's kernel name is held
against the intended instantiation.  Where the index order of a scene is part of the case (sweeps 2 and 3) RTX_OPT_SORTED_STORE is
0: from 256 spheres on the kernels would otherwise stage a direction-sorted copy.

(RTX_STAT_CELL_CAPACITY_FLOOR is not held against the judged counts: it is the capacity the planner wants next -- 1.5 times the
longest list, rounded to 256 entries, and 0 while a fifth is to spare -- not the longest list itself.)"""
import functools

import numpy as np
import pytest

import oracle as O
import rollcall_cases as RC
import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(160, 160)
    for opt in (R.OPT_VIEW_ADAPT, R.OPT_TILE_ORDER, R.OPT_XCD_ORDER):
        c.set_option(opt, 0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def oracle_frame(case, mode):
    return O.render(U.oracle_params(case.params()), O.Scene.from_arrays(case.sph, case.planes), mode, threads=8)


@functools.lru_cache(maxsize=None)
def oracle_pixels(case):
    return O.render(U.oracle_params(case.params()), O.Scene.from_arrays(case.sph, case.planes), O.RGB_ASCII, want_pixels=True)[1]


def assert_same(got, want, mode, W, what):
    S = 20 if mode >= O.RGB_ASCII else 12
    assert np.array_equal(got, want), "%s: %s" % (what, U.first_diff(got, want, S, W))


def set_plan(R, ctx, plan, sorted_store=-1, reuse=-1, capacity=0):
    (kernel, tile, sub, two, refine), _ = RC.PLANS[plan]
    ctx.set_option(R.OPT_KERNEL, {"brute": R.KERNEL_BRUTE, "binned": R.KERNEL_BINNED}[kernel])
    ctx.set_option(R.OPT_TILE_LOG2_W, tile)
    ctx.set_option(R.OPT_SUBTILES, sub)
    ctx.set_option(R.OPT_TWO_LEVEL, two)
    ctx.set_option(R.OPT_REFINE, refine)
    ctx.set_option(R.OPT_SORTED_STORE, sorted_store)
    ctx.set_option(R.OPT_CELL_REUSE, reuse)
    ctx.set_option(R.OPT_CELL_CAPACITY, capacity)


def assert_kernel(ctx, plan, extra=""):
    name = ctx.last_kernel
    want = RC.PLANS[plan][1]
    assert name.startswith("rtx_trace<") and extra in name, name
    assert (",false" in name) == (want == ",false") and name.endswith(",refine>") == (want == ",refine>"), "%s launched %s" % (plan, name)


def load(ctx, case):
    ctx.set_scene(case.sph, case.planes)
    return case.params()


def frame_under(R, ctx, p, case, plan, mode=O.RGB_ASCII, what="", **opts):
    set_plan(R, ctx, plan, **opts)
    got = ctx.render_to_host(p, mode)
    assert_kernel(ctx, plan)
    assert_same(got, oracle_frame(case, mode), mode, case.W, "%s, %s %s %r" % (case.name, plan, what, opts))


# ---------------------------------------------------------------------------------------------- 1. scene size

SIZE_CASES = [(n, "permuted", "default") for n in RC.SIZES] + [(257, "identity", "default"), (1025, "identity", "default"),
                                                                (513, "permuted", "rolled"), (1281, "permuted", "rolled")]


@pytest.mark.parametrize("ns,order,pose", SIZE_CASES)
def test_scene_size_under_every_plan(R, ctx, ns, order, pose):
    """ns owners all over a 65 x 64 frame: steps of 512 items, two per thread (`second_half_empty`, the prefetch past the end), the
    brute list's 1024 and the culled lists' 704 / 640 with the overflow walk behind them, the sorted copy from 256 on."""
    case = RC.size_case(ns, order, pose)
    p = load(ctx, case)
    for plan in RC.SIZE_PLANS:
        frame_under(R, ctx, p, case, plan)
    frame_under(R, ctx, p, case, "two", reuse=0)
    frame_under(R, ctx, p, case, "two", what="again")     # (the second frame of a resting view: cached lists)
    if ns in (RC.SORTED_FROM - 1, RC.SORTED_FROM, RC.SORTED_FROM + 1):
        for store in (0, 1):
            for plan in RC.SIZE_PLANS:
                frame_under(R, ctx, p, case, plan, sorted_store=store)


@pytest.mark.parametrize("ns", RC.SIZES)
def test_scene_size_in_every_output_form(R, ctx, ns):
    """Records in RGB_ASCII (above) and BIT_PIXEL, compact words, and the value floats: the distance of every owned pixel is the
    oracle's, bit for bit."""
    import torch
    case = RC.size_case(ns)
    p = load(ctx, case)
    W, H = case.W, case.H
    px = oracle_pixels(case).reshape(-1)
    words = torch.empty(W * H, dtype=torch.int32, device="cuda")
    vals = torch.empty(W * H * 8, dtype=torch.float32, device="cuda")
    for plan in ("brute", "sub1", "sub4", "refine", "two"):
        frame_under(R, ctx, p, case, plan, O.BIT_PIXEL)
        for mode, kind in ((O.RGB_ASCII, ord("3")), (O.BIT_PIXEL, ord("4"))):
            S = 20 if mode >= O.RGB_ASCII else 12
            words.fill_(0x5A5A5A5A)
            torch.cuda.synchronize()
            ctx.render_rows(p, mode, 0, H, d_out=words.data_ptr(), out_row_base=0, flags=R.RENDER_COMPACT)
            ctx.synchronize()
            assert_kernel(ctx, plan, "compact")
            got = U.words_to_records(words.cpu().numpy().view(np.uint32), S, kind)
            assert_same(got, oracle_frame(case, mode)[:S * W * H], mode, W, "%s, %s compact words" % (case.name, plan))
        vals.fill_(-1.0)
        torch.cuda.synchronize()
        ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=vals.data_ptr(), out_row_base=0, flags=R.RENDER_VALUES)
        ctx.synchronize()
        assert_kernel(ctx, plan, "values")
        got = vals.cpu().numpy().reshape(H * W, 8)
        own = case.pix[case.owner]
        assert np.array_equal(got[own, 0].view(np.uint32), px["distance"][own].view(np.uint32)), "%s, %s: an owned pixel's distance" % (case.name, plan)
        traced = np.arange(W * H) % W != W - 1
        assert np.array_equal(got[traced, 0].view(np.uint32), px["distance"][traced].view(np.uint32)), "%s, %s: distances" % (case.name, plan)


@pytest.mark.parametrize("ns", RC.SIZES)
def test_scene_size_through_the_closest_hit_form(R, ctx, ns):
    """The same body as kOutHit: shadows on with RTX_OPT_SHADOW_CHECK 2 (no test: every pixel lit) gives the one-launch kernel's bytes
     -- the oracle's."""
    case = RC.size_case(ns)
    p = load(ctx, case)
    try:
        ctx.set_option(R.OPT_SHADOWS, 1)
        ctx.set_option(R.OPT_SHADOW_CHECK, 2)
        for plan in ("brute", "sub4", "sub16", "refine", "two"):
            set_plan(R, ctx, plan)
            before = ctx.get_option(R.STAT_SHADOW_FRAMES)
            got = ctx.render_to_host(p, O.RGB_ASCII)
            assert ctx.get_option(R.STAT_SHADOW_FRAMES) == before + 1 and "rtx_shadow_shade" in ctx.last_kernel
            assert_same(got, oracle_frame(case, O.RGB_ASCII), O.RGB_ASCII, case.W, "%s, %s, closest hits then shading" % (case.name, plan))
    finally:
        ctx.set_option(R.OPT_SHADOW_CHECK, 0)
        ctx.set_option(R.OPT_SHADOWS, 0)


@pytest.mark.parametrize("ns", RC.SIZES)
def test_scene_size_in_batched_and_ragged_slabs(R, ctx, ns):
    """rtx_trace_batch (2 and 16 slabs of one stream in one launch) and ragged row slabs placed by out_row_base."""
    import torch
    case = RC.size_case(ns)
    p = load(ctx, case)
    W, H = case.W, case.H
    want = oracle_frame(case, O.RGB_ASCII)
    st = torch.cuda.Stream()
    set_plan(R, ctx, "sub4")
    for n in (2, 16):
        bufs = [torch.full((20 * W * H,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        before = ctx.get_option(R.STAT_BATCHED_LAUNCHES)
        ctx.submit_slabs([p] * n, O.RGB_ASCII, 0, H, [b.data_ptr() for b in bufs], 0, [st.cuda_stream] * n)
        assert ctx.get_option(R.STAT_BATCHED_LAUNCHES) == before + 1 and "rtx_trace_batch" in ctx.last_kernel
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            assert_same(b.cpu().numpy(), want, O.RGB_ASCII, W, "%s, frame %d of a batch of %d" % (case.name, i, n))
    cuts = (0, 21, 22, 47, H)
    for plan in ("brute", "sub4", "refine", "two"):
        set_plan(R, ctx, plan)
        pieces = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            slab = torch.full((20 * W * (r1 - r0),), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.render_rows(p, O.RGB_ASCII, r0, r1 - r0, d_out=slab.data_ptr(), out_row_base=r0)
            ctx.synchronize()
            assert_kernel(ctx, plan)
            pieces.append(slab.cpu().numpy())
        assert_same(np.concatenate(pieces), want, O.RGB_ASCII, W, "%s, %s, ragged slabs" % (case.name, plan))


# ---------------------------------------------------------------------------------------------- 2. candidates of one macro tile

TILE_PARAMS = [(cap,) + v for cap in (RC.CAP_CULL, RC.CAP_REFINE) for v in RC.tile_variants(cap)]


@pytest.mark.parametrize("cap,k,placement,order", TILE_PARAMS)
def test_candidates_of_one_macro_tile(R, ctx, cap, k, placement, order):
    """One 32 x 32 macro tile with k candidates around the list capacity (704; 640 with REFINE) and a step of 512 either side of
    it: the list takes a step while its survivors fit, the overflow walk rescans per sub-tile and flushes past capacity - 512."""
    case = RC.tile_case(k, placement, order)
    p = load(ctx, case)
    frame_under(R, ctx, p, case, "sub4" if cap == RC.CAP_CULL else "refine", sorted_store=0)


# ---------------------------------------------------------------------------------------------- 3. a wave's list

@pytest.mark.parametrize("order", RC.ORDERS)
@pytest.mark.parametrize("n", RC.WAVE_COUNTS)
def test_candidates_of_one_wave_region(R, ctx, n, order):
    """REFINE: one 64-pixel wave region with n candidates around the wave list's 128 entries, its fifteen neighbours with 6: one
    workgroup holds refined waves and one that falls back to the whole list."""
    case = RC.wave_case(n, order)
    p = load(ctx, case)
    frame_under(R, ctx, p, case, "refine", sorted_store=0)
    frame_under(R, ctx, p, case, "two_refine", sorted_store=0, reuse=0)


@pytest.mark.parametrize("total", RC.GATE_TOTALS)
def test_refinement_gate(R, ctx, total):
    """A workgroup refines from 9 candidates on."""
    case = RC.gate_case(total)
    p = load(ctx, case)
    frame_under(R, ctx, p, case, "refine", sorted_store=0)
    frame_under(R, ctx, p, case, "refine")


# ---------------------------------------------------------------------------------------------- 4. cell lists

@pytest.mark.parametrize("listed", RC.CELL_LISTED)
def test_cell_lists(R, ctx, listed):
    """Two-level culling, one cell listing `listed` spheres: the first step requested ahead of the count, the second half from 257
    on, the capacity at listed - 1 (the whole scene instead), listed and listed + 1, an empty list."""
    case = RC.cell_case(listed)
    p = load(ctx, case)
    for plan in ("two", "two_refine"):
        for cap in (listed - 1, listed, listed + 1):
            if cap >= 1:
                frame_under(R, ctx, p, case, plan, reuse=0, capacity=cap)
                frame_under(R, ctx, p, case, plan, capacity=cap)
                frame_under(R, ctx, p, case, plan, what="again", capacity=cap)
        frame_under(R, ctx, p, case, plan, reuse=0)
        frame_under(R, ctx, p, case, plan, reuse=0, sorted_store=0)


# ---------------------------------------------------------------------------------------------- 5. planes

@pytest.mark.parametrize("with_spheres", [False, True])
@pytest.mark.parametrize("n_planes", RC.PLANE_COUNTS)
def test_planes(R, ctx, n_planes, with_spheres):
    """Every plane owns a pixel: the LDS table's 16, compacted by ballot (culled per tile from two planes on), and the direct form
    from plane 17 on -- alone in the tiles of the right half, which see no table plane."""
    case = RC.plane_case(n_planes, with_spheres)
    p = load(ctx, case)
    for plan in ("brute", "sub4", "t16", "refine"):
        frame_under(R, ctx, p, case, plan)
        frame_under(R, ctx, p, case, plan, O.BIT_PIXEL)
