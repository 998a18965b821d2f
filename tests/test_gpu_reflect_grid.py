"""Mirror rays through the world grid (RTX_OPT_REFLECT_GRID, include/rtx.h).  The option changes which spheres a secondary ray is
tested against, never the test, so every frame must be the existing path's byte for byte.

The reference of every comparison is the same context with the option 0 and RTX_OPT_REFLECT_CHECK 1: the brute pass that tests
every sphere, which is not the code under test.  Whole buffers are compared, in the three output forms (values, records, compact
words) and the four character modes, on frames of 37 x 21 and 64 x 48 cells (ragged 16 x 16 tiles, a newline column).  The scenes
a, b and c are tests/reflect_grid_cases.py's; tests/test_host_reflect_grid.py shows on the CPU that they have mirror rays at three
levels, rays that leave and hit the large-list sphere, coincident twins under the direction sort, and floor rays on both sides of
`reach` -- so no comparison here is empty."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import reflect_grid_cases as G
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
from test_gpu_shadow_grid import FLOOR, FORMS, NO_PLANES, _assert_same, _set_lights

pytestmark = pytest.mark.gpu

LIGHTS3 = [(1.0, 50.0, 0.0), (0.0, 30.0, 100.0), (-40.0, 20.0, 60.0)]


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(640, 360)
    yield c
    c.close()


def _reset(R, c):
    TC._reset(R, c)
    for opt in (R.OPT_REFLECT_SHADOWS, R.OPT_SHADOW_GRID, R.OPT_REFLECT_GRID):
        c.set_option(opt, 0)
    c.set_option(R.OPT_SUPERSAMPLE, 1)


def _load(R, c, name, W, H, depth=1):
    f = G.facts(name, W, H)
    c.set_scene(f["sph"], f["pl"])
    T._set_k(c, f["ks"])
    c.set_option(R.OPT_REFLECT_DEPTH, depth)
    return f


def _frames(R, c, p, modes=T.MODES, forms=FORMS, render=T._rows):
    out = {}
    for mode in modes:
        for form in forms:
            flags = {"values": R.RENDER_VALUES, "records": 0, "compact": R.RENDER_COMPACT}[form]
            out[(mode, form)] = render(R, c, p, mode, flags)
    return out


def _reference(R, c, p, shadow_check=None, **kw):
    """The brute pass: both grid options 0, RTX_OPT_REFLECT_CHECK 1 (and, where shadows are compared too, RTX_OPT_SHADOW_CHECK 1)."""
    grids = (c.get_option(R.OPT_REFLECT_GRID), c.get_option(R.OPT_SHADOW_GRID))
    c.set_option(R.OPT_REFLECT_GRID, 0)
    c.set_option(R.OPT_SHADOW_GRID, 0)
    c.set_option(R.OPT_REFLECT_CHECK, 1)
    if shadow_check is not None:
        c.set_option(R.OPT_SHADOW_CHECK, shadow_check)
    try:
        return _frames(R, c, p, **kw)
    finally:
        c.set_option(R.OPT_REFLECT_CHECK, 0)
        c.set_option(R.OPT_SHADOW_CHECK, 0)
        c.set_option(R.OPT_REFLECT_GRID, grids[0])
        c.set_option(R.OPT_SHADOW_GRID, grids[1])


def _on(R, c, p, **kw):
    c.set_option(R.OPT_REFLECT_GRID, 1)
    try:
        return _frames(R, c, p, **kw)
    finally:
        c.set_option(R.OPT_REFLECT_GRID, 0)


def _rays(R, c):
    return [int(c.get_option(R.STAT_REFLECT_RAYS + l)) for l in range(R.MAX_REFLECT_DEPTH)]


# ---------------------------------------------------------------- 1. the frames are the brute pass's

CASES = [(n, d) for n in G.NAMES for d in (1, 3)] + [("c", 4)]


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name,depth", CASES, ids=lambda v: str(v))
def test_frames_equal_the_brute_reference(R, ctx, name, depth, size):
    _reset(R, ctx)
    W, H = size
    f = _load(R, ctx, name, W, H, depth)
    p = f["p"]
    what = "scene %s depth %d %d x %d" % (name, depth, W, H)
    ref = _reference(R, ctx, p)
    assert ctx.get_option(R.STAT_REFLECT_LONGEST_LIST) == f["ns"]  # (the brute pass lists every sphere)
    frames0 = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
    got = _on(R, ctx, p)
    assert ctx.last_kernel.split("<")[0] == ("rtx_lights_chain_shade" if depth > 1 else "rtx_reflect_shade"), ctx.last_kernel
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0 + len(got)
    assert ctx.get_option(R.STAT_REFLECT_LONGEST_LIST) == 0
    assert ctx.get_option(R.STAT_QUERY_BRUTE) == 0 and ctx.get_option(R.STAT_QUERY_GRID_CELLS) > 1
    print(what, "rays", _rays(R, ctx), "fallback", ctx.get_option(R.STAT_REFLECT_GRID_FALLBACK_RAYS), "cells", ctx.get_option(R.STAT_QUERY_GRID_CELLS),
          "large", ctx.get_option(R.STAT_QUERY_LARGE_SPHERES))
    if name != "a":
        assert ctx.get_option(R.STAT_QUERY_LARGE_SPHERES) >= 1
    _assert_same(got, ref, what)
    # the mirrors show: without them the frame is another one
    T._clear_k(ctx, f["ns"] + len(f["pl"]))
    plain = T._rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES)
    assert not np.array_equal(plain, ref[(O.RGB_ASCII, "values")])
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. the counters

@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name,depth", CASES, ids=lambda v: str(v))
def test_rays_per_level_and_fallback_rays(R, ctx, name, depth, size):
    _reset(R, ctx)
    W, H = size
    f = _load(R, ctx, name, W, H, depth)
    p = f["p"]
    ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, 1 if depth == 1 else 0)  # (the chain kernel counts; rtx_reflect_hit does not)
    _reference(R, ctx, p, modes=[O.RGB_ASCII], forms=["values"])
    want = _rays(R, ctx)
    ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, 0)
    _on(R, ctx, p, modes=[O.RGB_ASCII], forms=["values"])
    got = _rays(R, ctx)
    fallback = int(ctx.get_option(R.STAT_REFLECT_GRID_FALLBACK_RAYS))
    said = f["rays"][:depth] + [0] * (R.MAX_REFLECT_DEPTH - depth)
    sure, unsure = sum(f["beyond"][:depth]), sum(f["unsure"][:depth])
    print(name, depth, size, "rays", got, "reference", want, "restatement", said, "fallback", fallback, "beyond reach for sure", sure, "on the boundary", unsure)
    assert got == want == said
    if name in ("a", "b"):
        assert fallback == 0
    else:
        assert sure <= fallback <= sure + unsure
        assert 0 < fallback < got[0]
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. with the shadow options and light sets

@pytest.mark.parametrize("n_lights", [1, 3])
@pytest.mark.parametrize("shadow_grid", [0, 1])
@pytest.mark.parametrize("deep", [0, 1])
def test_combinations_equal_the_all_brute_reference(R, ctx, deep, shadow_grid, n_lights):
    _reset(R, ctx)
    W, H = 64, 48
    f = _load(R, ctx, "c", W, H, depth=2)
    p = f["p"]
    _set_lights(R, ctx, LIGHTS3[:n_lights])
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, deep)
    kw = dict(modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["values"])
    ref = _reference(R, ctx, p, shadow_check=1, **kw)
    ctx.set_option(R.OPT_SHADOW_GRID, shadow_grid)
    if shadow_grid:
        # one grid, one build: the scene put again makes the next frame rebuild
        f = _load(R, ctx, "c", W, H, depth=2)
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        builds = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
        first = T._rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES)
        assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
        second = T._rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES)
        assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
        assert np.array_equal(first, second)
    frames0 = (ctx.get_option(R.STAT_REFLECT_GRID_FRAMES), ctx.get_option(R.STAT_SHADOW_GRID_FRAMES))
    got = _on(R, ctx, p, **kw)
    family = ("rtx_grid_chain_shadow_shade" if deep else "rtx_grid_chain_shade") if shadow_grid else ("rtx_lights_chain_shadow_shade" if deep else "rtx_lights_chain_shade")
    assert ctx.last_kernel.split("<")[0] == family, ctx.last_kernel
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0[0] + 2
    assert ctx.get_option(R.STAT_SHADOW_GRID_FRAMES) == frames0[1] + 2 * shadow_grid
    _assert_same(got, ref, "deep %d shadow grid %d lights %d" % (deep, shadow_grid, n_lights))
    # the shadows show: the all-lit frame is another one
    lit = _reference(R, ctx, p, shadow_check=2, modes=[O.RGB_ASCII], forms=["values"])
    assert not np.array_equal(lit[(O.RGB_ASCII, "values")], ref[(O.RGB_ASCII, "values")])
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. the map follows the scene

def test_the_position_map_follows_edits_removals_and_additions(R, ctx):
    _reset(R, ctx)
    W, H = 64, 48
    f = _load(R, ctx, "b", W, H, depth=3)
    p, sph = f["p"], f["sph"]
    kw = dict(modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["values", "records"])
    seen = []

    def check(what):
        ref = _reference(R, ctx, p, **kw)
        frames0 = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
        got = _on(R, ctx, p, **kw)
        assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0 + 4 and ctx.get_option(R.STAT_QUERY_BRUTE) == 0
        _assert_same(got, ref, what)
        for earlier in seen:
            assert not np.array_equal(earlier, ref[(O.RGB_ASCII, "values")]), what + ": the step changed nothing"
        seen.append(ref[(O.RGB_ASCII, "values")])
        return got

    check("as loaded")
    for i in range(0, len(sph), 2):
        ctx.set_sphere_motion(i, 1, 3.0)
    ctx.update_objects(0.2)
    check("after rtx_update_objects")
    # (what is moved and removed is visible: chosen by the pixels the restatement gives each sphere's primary hit)
    seen_px = np.bincount(f["trace"]["gid"][f["trace"]["vis"]], minlength=len(sph))[:len(sph)]
    first = int(np.argmax([seen_px[i:i + 20].sum() for i in range(0, 130)]))  # 20 spheres in a row, below the large sphere's index
    moved = sph[first:first + 20].copy()
    moved[:, 0] += 2.5
    moved[:, 1] -= 1.5
    ctx.set_spheres(first, moved)
    check("after rtx_scene_set_spheres")
    rest = [int(i) for i in np.argsort(-seen_px, kind="stable") if not first <= i < first + 20 and i != G.LARGE and i < 301]
    gone = sorted(rest[:8] + [min(i for i in rest[8:] if i < G.LARGE), 301])  # (301: the later twin of 142; one below the large sphere's index)
    assert len(set(gone)) == 10 and gone[0] < G.LARGE
    ctx.remove_objects(gone)
    assert ctx.object_count == len(sph) - len(gone)
    check("after rtx_scene_remove_objects")
    rng = np.random.default_rng(8)
    more = np.zeros((5, 7), dtype=np.float32)
    more[:, :3] = np.array([0, 0, 95]) + rng.uniform(-1, 1, (5, 3)) * np.array([10, 6, 8])
    more[:, 3] = 2.0
    more[:, 4:] = [200, 200, 40]
    ctx.add_spheres(more)
    n = ctx.object_count
    ctx.set_reflectivity(n - 5, np.array([0.5, 0.0, 0.5, 0.0, 0.5], dtype=np.float32))
    last = check("after adding five spheres")
    # a context built afresh from the final scene gives the same bytes
    rows = np.array([ctx.get_object(i)[1][:7] for i in range(n)], dtype=np.float32)
    ks = np.array([ctx.get_reflectivity(i) for i in range(n)], dtype=np.float32)
    with R.Context(W, H) as c2:
        c2.set_scene(rows, NO_PLANES)
        c2.set_reflectivity(0, ks)
        c2.set_option(R.OPT_REFLECT_DEPTH, 3)
        fresh = _on(R, c2, p, **kw)
        assert c2.get_option(R.STAT_REFLECT_GRID_FRAMES) == 4
    _assert_same(fresh, last, "a fresh context of the final scene")
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. where it has no effect

def _same_with_and_without(R, c, p, what):
    """The option 1 against 0 on the scene and options as they are: same bytes, same shade kernel, nothing counted."""
    frames0 = c.get_option(R.STAT_REFLECT_GRID_FRAMES)
    c.set_option(R.OPT_REFLECT_GRID, 0)
    off = _frames(R, c, p, modes=[O.RGB_ASCII, O.BIT_ASCII], forms=["values", "records"])
    k_off = c.last_kernel
    c.set_option(R.OPT_REFLECT_GRID, 1)
    on = _frames(R, c, p, modes=[O.RGB_ASCII, O.BIT_ASCII], forms=["values", "records"])
    assert c.last_kernel == k_off
    _assert_same(on, off, what)
    assert c.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0, what
    return on


def test_where_it_has_no_effect_the_launches_are_todays(R, ctx):
    _reset(R, ctx)
    W, H = 64, 48
    p = R.camera_params(W, H)
    # a reflective floor and no sphere
    ctx.set_scene(NO_PLANES[:, :7], FLOOR)
    ctx.set_reflectivity(0, 0.5)
    _same_with_and_without(R, ctx, p, "a floor and no sphere")
    assert ctx.last_kernel.startswith("rtx_reflect_shade<")
    # a scene whose only sphere has a centre that is not finite: no usable grid
    ctx.set_scene(np.array([[np.nan, 0, 100, 5, 200, 10, 10]], dtype=np.float32), FLOOR)
    ctx.set_reflectivity(0, np.array([0.4, 0.5], dtype=np.float32))
    _same_with_and_without(R, ctx, p, "one sphere that is not finite")
    assert ctx.get_option(R.STAT_QUERY_BRUTE) == 1
    # checks 1 and 2 keep today's launches
    f = _load(R, ctx, "c", W, H, depth=2)
    for check in (1, 2):
        ctx.set_option(R.OPT_REFLECT_CHECK, check)
        _same_with_and_without(R, ctx, p, "RTX_OPT_REFLECT_CHECK %d" % check)
        if check == 1:
            assert ctx.get_option(R.STAT_REFLECT_LONGEST_LIST) == f["ns"]
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)
    # nothing reflective: not the mirror path
    T._clear_k(ctx, f["ns"] + 1)
    _same_with_and_without(R, ctx, p, "nothing reflective")
    assert "reflect" not in ctx.last_kernel and "shade" not in ctx.last_kernel, ctx.last_kernel  # (the trace launch alone)
    _reset(R, ctx)


def test_option_0_after_1_is_the_state_before(R):
    W, H = 64, 48
    f = G.facts("c", W, H)
    p = f["p"]
    with R.Context(W, H) as c:  # (a context the option was never set on)
        c.set_scene(f["sph"], f["pl"])
        T._set_k(c, f["ks"])
        c.set_option(R.OPT_REFLECT_DEPTH, 2)
        kw = dict(modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["records", "values"])
        before = _frames(R, c, p, **kw)
        longest = c.get_option(R.STAT_REFLECT_LONGEST_LIST)
        assert longest > 0 and c.get_option(R.OPT_REFLECT_GRID) == 0 and c.get_option(R.STAT_REFLECT_GRID_FRAMES) == 0
        on = _on(R, c, p, **kw)
        assert c.get_option(R.STAT_REFLECT_GRID_FRAMES) == 4 and c.get_option(R.STAT_REFLECT_LONGEST_LIST) == 0
        _assert_same(on, before, "the option on")
        after = _frames(R, c, p, **kw)
        _assert_same(after, before, "the option back to 0")
        assert c.get_option(R.STAT_REFLECT_GRID_FRAMES) == 4 and c.get_option(R.STAT_REFLECT_LONGEST_LIST) == longest


def test_other_values_are_refused_and_the_option_keeps_its_value(R, ctx):
    _reset(R, ctx)
    for start in (0, 1):
        ctx.set_option(R.OPT_REFLECT_GRID, start)
        for bad in (2, -1, 1 << 40):
            with pytest.raises(R.RtxError) as e:
                ctx.set_option(R.OPT_REFLECT_GRID, bad)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            assert ctx.get_option(R.OPT_REFLECT_GRID) == start
    for stat in (R.STAT_REFLECT_GRID_FRAMES, R.STAT_REFLECT_GRID_FALLBACK_RAYS):
        with pytest.raises(R.RtxError):
            ctx.set_option(stat, 0)  # (a counter is read-only)
    _reset(R, ctx)


# ---------------------------------------------------------------- 6. what traces through rtx_render_rows inherits it

def test_a_ragged_slab(R, ctx):
    import torch
    _reset(R, ctx)
    W, H = 37, 21
    f = _load(R, ctx, "c", W, H, depth=3)
    p = f["p"]
    row0, rows = 5, 11  # rows 5 .. 15: hit indices are relative to row0, and the only tile row has 11 of its 16 rows

    def slab(R, c, p, mode, flags=0):
        S = 32 if flags & R.RENDER_VALUES else (4 if flags & R.RENDER_COMPACT else (20 if mode >= O.RGB_ASCII else 12))
        buf = torch.full((rows * W * S,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.render_rows(p, mode, row0, rows, d_out=buf.data_ptr(), out_row_base=row0, flags=flags)
        c.synchronize()
        return buf.cpu().numpy()

    kw = dict(modes=[O.RGB_ASCII, O.BIT_PIXEL], render=slab)
    ref = _reference(R, ctx, p, **kw)
    frames0 = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
    got = _on(R, ctx, p, **kw)
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0 + 6
    _assert_same(got, ref, "rows 5 .. 15 of 37 x 21")
    whole = _reference(R, ctx, p, modes=[O.RGB_ASCII], forms=["records"])[(O.RGB_ASCII, "records")]
    assert np.array_equal(ref[(O.RGB_ASCII, "records")], whole[row0 * W * 20:(row0 + rows) * W * 20])
    _reset(R, ctx)


def test_the_update_stream(R, ctx):
    _reset(R, ctx)
    f = _load(R, ctx, "c", 64, 48, depth=2)
    p = f["p"]
    for mode in (O.RGB_ASCII, O.BIT_ASCII):
        ctx.set_option(R.OPT_REFLECT_CHECK, 1)
        want = bytes(ctx.update(p, mode))
        ctx.set_option(R.OPT_REFLECT_CHECK, 0)
        frames0 = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        got = bytes(ctx.update(p, mode))
        ctx.set_option(R.OPT_REFLECT_GRID, 0)
        assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0 + 1
        assert got == want and len(got) > 500
    _reset(R, ctx)


def test_supersampled_frames(R, ctx):
    _reset(R, ctx)
    f = _load(R, ctx, "a", 37, 21, depth=3)
    p = f["p"]
    ctx.set_option(R.OPT_SUPERSAMPLE, 2)
    kw = dict(modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["values", "records"])
    ref = _reference(R, ctx, p, **kw)
    frames0 = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
    got = _on(R, ctx, p, **kw)
    assert ctx.last_kernel.startswith("rtx_resolve<"), ctx.last_kernel
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0 + 4
    _assert_same(got, ref, "S = 2")
    ctx.set_option(R.OPT_SUPERSAMPLE, 1)
    one = _reference(R, ctx, p, modes=[O.RGB_ASCII], forms=["values"])
    assert not np.array_equal(one[(O.RGB_ASCII, "values")], ref[(O.RGB_ASCII, "values")])
    _reset(R, ctx)


def test_three_logical_ranks_equal_the_one_device_reference(R, ctx):
    _reset(R, ctx)
    f = _load(R, ctx, "c", 64, 48, depth=3)
    p = f["p"]
    ctx.set_option(R.OPT_REFLECT_CHECK, 1)
    want = [ctx.render_to_host(p, m).copy() for m in (O.BIT_ASCII, O.RGB_ASCII)]
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)
    with R.Context(64, 48, devices=[0, 0, 0]) as g:
        g.set_scene(f["sph"], f["pl"])
        T._set_k(g, f["ks"])
        g.set_option(R.OPT_REFLECT_DEPTH, 3)
        g.set_option(R.OPT_REFLECT_GRID, 1)
        assert g.get_option(R.OPT_REFLECT_GRID) == 1
        with pytest.raises(R.RtxError):
            g.set_option(R.OPT_REFLECT_GRID, 2)
        assert [g.member_option(r, R.OPT_REFLECT_GRID) for r in range(3)] == [1, 1, 1]
        got = [g.render_to_host(p, m).copy() for m in (O.BIT_ASCII, O.RGB_ASCII)]
        assert [g.member_option(r, R.STAT_REFLECT_GRID_FRAMES) for r in range(3)] == [2, 2, 2]
        assert [g.member_option(r, R.STAT_QUERY_GRID_BUILDS) for r in range(3)] == [1, 1, 1]  # every member builds its own grid
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    _reset(R, ctx)


def test_a_capture_refuses_the_grid_path_and_the_context_goes_on(R, ctx):
    import torch
    _reset(R, ctx)
    W, H = 64, 48
    f = _load(R, ctx, "c", W, H, depth=2)
    p = f["p"]
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    want = T._rows(R, ctx, p, O.RGB_ASCII)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(s.cuda_stream)
    with pytest.raises(R.RtxError) as e:
        ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
    # the capture goes on: with the option off the same call is recorded
    ctx.set_option(R.OPT_REFLECT_GRID, 0)
    ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want)
    finally:
        ctx.graph_destroy(g)
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    frames0 = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
    assert np.array_equal(T._rows(R, ctx, p, O.RGB_ASCII), want)
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == frames0 + 1
    _reset(R, ctx)


# ---------------------------------------------------------------- 7. the facade

def test_the_facade_sets_the_option(tmp_path):
    """tests/host/compat_reflect_grid.cpp: Scene3D::SetReflectGrid(true) gives the frame of the option set through the ABI, which is
    the frame without the option; the launch sets are counted for both and for neither of the frames with the option off."""
    R = U.pkg()
    exe = str(tmp_path / "compat_reflect_grid")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(U.ROOT, "include"),
                           os.path.join(U.ROOT, "tests", "host", "compat_reflect_grid.cpp"), "-o", exe, "-L", R.PKG_DIR, "-lrtx_hip", "-pthread",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "facade reflect grid ok" in p.stdout, p.stdout[-4000:]
    assert "frames off 0 facade 1 abi 2 off again 2" in p.stdout, p.stdout[-4000:]
