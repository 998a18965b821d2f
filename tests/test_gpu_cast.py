"""Objects that cast no shadow (rtx_scene_set_shadow_casting, include/rtx.h) on the GPU, bit for bit.  The inputs are judged on the
CPU by tests/test_host_restate_cast.py.
  1. float64 decides: on restate_shadows' three scenes with U = the even-numbered spheres non-casting, a frame's values are
     restate_shadows.shade_chain_dark's under the dark sets restate_cast decides per level, on every pixel float64 decides (the
     ambiguous ones are skipped and nothing else); one and three lights, depth 1 and 3, RTX_OPT_REFLECT_SHADOWS on; the frame differs
     from the all-casting frame at no fewer pixels than level 0 lights again.
  2. an independent exact oracle: scene A with U non-casting against scene B = A after rtx_scene_remove_objects(U): wherever distance
     and normal are bit-equal in both frames all eight floats are; no mirrors; U holds a plane above the scene, under the light.
  3. culled = brute = grid: RTX_OPT_SHADOW_CHECK 0 / 1, RTX_OPT_SHADOW_GRID 0 / 1 and RTX_OPT_LIGHTS_CHECK 0 / 1 give the same bytes
     on the shaded, mirror and chain paths.
  4. the walk's and the lists' edges: 1 .. 1537 spheres with the non-casters at the ends of the loads and steps, and with only those
     casting; RTX_OPT_SORTED_STORE 0 and 1; a 48 x 27 frame; oracle 2 throughout; RTX_STAT_SHADOW_LONGEST_LIST under check 1 is the
     number of casting spheres; RTX_STAT_SHADOW_GRID_FALLBACK_POINTS does not depend on the flags.
  6. no flags, no change: with every object casting -- never set, set to 1, or set and cleared -- kernel names and bytes are those
     of a context that never made the call; and with flags but no shadow test likewise.
  5. lives, on the small scene of tests/test_gpu_materials.py (a mirror, a glass sphere, two patterned objects, one light, shadows
     on): the flags survive rtx_scene_set_spheres and physics, follow the renumbering after a removal, are forgotten by
     rtx_scene_clear; a recorded graph is refused after a change and replays after re-capture; a device group of three ranks gives
     the one-device frame and a refused call changes nothing on it; rtx_update and rtx_update_half show the result."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_cast as RC
import restate_shadows as RH
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_half as TH
import test_gpu_materials as TM
import restate_half as RHALF


def _shadowless(c, n):
    """How many of the objects 0 .. n-1 cast no shadow, by rtx_scene_get_shadow_casting."""
    return sum(1 - c.get_shadow_casting(i) for i in range(n))

pytestmark = pytest.mark.gpu

EDGES = (0, 31, 32, 255, 256, 511, 512)


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
    c.set_option(R.OPT_REFLECT_SHADOWS, 0)
    c.set_option(R.OPT_SHADOW_GRID, 0)


def _u32(v):
    return np.ascontiguousarray(v).view(np.uint32)


# ---------------------------------------------------------------- 1. float64 decides

@pytest.mark.parametrize("nl,depth", [(1, 1), (1, 3), (3, 1), (3, 3)])
@pytest.mark.parametrize("name", RH.SCENES)
def test_float64_decides_under_the_mask(R, ctx, name, nl, depth):
    _reset(R, ctx)
    p, sph, pl, ks, pix, trace = RH.traced(name)
    _, lights, casts, full, masked = RC.sets(name, nl, depth)
    ctx.set_scene(sph, pl)
    T._set_k(ctx, ks)
    pp = TC._params(p)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    all_cast = TC._values(R, ctx, pp)
    plain_kernel = ctx.last_kernel
    ctx.set_shadow_casting(0, casts)
    assert _shadowless(ctx, len(casts)) == int((casts == 0).sum())
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shadow_shade<") and ctx.last_kernel == plain_kernel, (ctx.last_kernel, plain_kernel)
    what = "%s, %d lights, depth %d" % (name, nl, depth)
    # distance, glyph value and normal are the trace's, whatever the flags
    TC._assert_values(got, trace, [got[:, 5], got[:, 6], got[:, 7]], what, fields=range(5))
    want = RH.shade_chain_dark(trace, lights, [m["dset"] for m in masked] + [0] * (4 - depth))[depth]
    decided = np.logical_and.reduce([m["decided"] for m in masked]) & trace["vis"]
    same = np.logical_and.reduce([RS.same_floats(got[:, 5 + q], want[q]) for q in range(3)])
    bad = np.nonzero(decided & ~same)[0]
    print("%s: %d visible, %d decided, %d differ from the restatement" % (what, int(trace["vis"].sum()), int(decided.sum()), bad.size))
    assert bad.size == 0, "%s: %d of %d decided pixels are not shaded with the masked sets, e.g. pixel %d: got %r want %r" % (
        what, bad.size, int(decided.sum()), int(trace["pix"][bad[0]]), got[bad[0], 5:8], [w[bad[0]] for w in want])
    assert int(decided.sum()) >= 0.99 * int(trace["vis"].sum())
    # the flags show: at least the pixels whose level 0 is lit again differ from the all-casting frame
    lit0 = RC.lit_again(name, nl, 0)[3]
    changed = (_u32(got) != _u32(all_cast)).any(axis=1)
    print("%s: %d pixels differ from the all-casting frame, %d are lit again at level 0" % (what, int(changed.sum()), int(lit0.sum())))
    assert int(changed.sum()) >= int(lit0.sum()) >= 1000
    _reset(R, ctx)
    ctx.set_shadow_casting(0, np.ones(len(casts), dtype=np.uint8))


# ---------------------------------------------------------------- 2. the independent oracle: non-casting = removed, where both are seen alike

ORACLE_W, ORACLE_H = RC.ORACLE_W, RC.ORACLE_H


def _same_view(a, b):
    """Pixels whose distance and normal are bit-equal in two values frames."""
    return (_u32(a[:, 0]) == _u32(b[:, 0])) & (_u32(a[:, 2:5]) == _u32(b[:, 2:5])).all(axis=1)


def _assert_non_casting_equals_removed(R, a, b, pp, what, share=None):
    """Oracle 2 on two contexts that hold scene A (U non-casting) and scene B (U removed): returns A's frame."""
    va, vb = TC._values(R, a, pp), TC._values(R, b, pp)
    alike = _same_view(va, vb)
    visible = va[:, 0] != RS.NO_HIT
    bad = np.nonzero(alike & (_u32(va) != _u32(vb)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d pixels seen alike differ, e.g. pixel %d: %r against %r" % (what, bad.size, int(alike.sum()), int(bad[0]), va[bad[0]], vb[bad[0]])
    if share is not None:
        assert int((alike & visible).sum()) >= share * int(visible.sum()), "%s: %d of %d visible pixels are seen alike" % (what, int((alike & visible).sum()), int(visible.sum()))
    return va


@pytest.mark.parametrize("nl", [1, 3])
def test_non_casting_is_removed_where_both_are_seen_alike(R, nl):
    p, sph, pl, u = RC.oracle_scene()
    pp = TC._params(p)
    lights = RH.lights("wall", nl)
    casts = np.ones(len(sph) + len(pl), dtype=np.uint8)
    casts[u] = 0
    with R.Context(ORACLE_W, ORACLE_H) as a, R.Context(ORACLE_W, ORACLE_H) as b:
        for c in (a, b):
            c.set_scene(sph, pl)
            TC._set_lights(R, c, lights)
            c.set_option(R.OPT_SHADOWS, 1)
        all_cast = TC._values(R, a, pp)
        a.set_shadow_casting(0, casts)
        b.remove_objects(u)
        va = _assert_non_casting_equals_removed(R, a, b, pp, "%d lights" % nl, share=0.8)
        assert a.last_kernel.startswith("rtx_shadow_shade<" if nl == 1 else "rtx_lights_shade<")
        # the lid and the spheres threw shadows that are gone now
        assert int((_u32(va) != _u32(all_cast)).any(axis=1).sum()) >= 500
        for opt in (R.OPT_SHADOW_CHECK, R.OPT_SHADOW_GRID, R.OPT_LIGHTS_CHECK):  # ... under the brute test, the grid and the lights' kernels
            a.set_option(opt, 1)
            b.set_option(opt, 1)
            assert np.array_equal(_assert_non_casting_equals_removed(R, a, b, pp, "%d lights, option %d" % (nl, opt)), va)
            a.set_option(opt, 0)
            b.set_option(opt, 0)


# ---------------------------------------------------------------- 3. culled = brute = grid

@pytest.mark.parametrize("path", ["shaded", "mirror", "chain"])
@pytest.mark.parametrize("nl", [1, 3])
def test_culled_equals_brute_equals_grid(R, ctx, path, nl):
    _reset(R, ctx)
    p, sph, pl, ks, pix, trace = RH.traced("wall")
    casts = RC.even_spheres(len(sph), len(pl))
    ctx.set_scene(sph, pl)
    if path != "shaded":
        T._set_k(ctx, ks)
    pp = TC._params(p)
    TC._set_lights(R, ctx, RH.lights("wall", nl))
    ctx.set_option(R.OPT_SHADOWS, 1)
    if path == "chain":
        ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
        ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    all_cast = TC._values(R, ctx, pp)
    ctx.set_shadow_casting(0, casts)
    builds = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    culled = TC._values(R, ctx, pp)
    assert (_u32(culled) != _u32(all_cast)).any()
    kernels = {"culled": ctx.last_kernel}
    for name, opt in (("brute", R.OPT_SHADOW_CHECK), ("grid", R.OPT_SHADOW_GRID), ("lights", R.OPT_LIGHTS_CHECK)):
        ctx.set_option(opt, 1)
        got = TC._values(R, ctx, pp)
        kernels[name] = ctx.last_kernel
        ctx.set_option(opt, 0)
        assert np.array_equal(_u32(got), _u32(culled)), "%s differs from culled at %d pixels" % (name, int((_u32(got) != _u32(culled)).any(axis=1).sum()))
    assert "grid" in kernels["grid"], kernels
    if nl == 1 and path != "chain":
        assert kernels["lights"] != kernels["culled"], kernels
    # a flag change does not rebuild the grid: one build for the grid frame, none for the flags
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) <= builds + 1
    b1 = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    TC._values(R, ctx, pp)
    b2 = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    ctx.set_shadow_casting(0, np.ones(len(casts), dtype=np.uint8))
    back = TC._values(R, ctx, pp)
    ctx.set_shadow_casting(1, [0])
    TC._values(R, ctx, pp)
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == b2 and b2 <= b1 + 1
    assert np.array_equal(_u32(back), _u32(all_cast))
    ctx.set_shadow_casting(0, np.ones(len(casts), dtype=np.uint8))
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. the walk's and the lists' edges

EDGE_W, EDGE_H = 48, 27


def edge_scene(ns):
    """ns spheres over a floor under one light, a dense cluster of small spheres in the light's way (a cone from the light over a tile
    of the floor meets most of them: the list fills and refills), seen from above."""
    rng = np.random.default_rng(1000 + ns)
    c = np.stack([rng.uniform(-9, 9, ns), rng.uniform(3, 9, ns), rng.uniform(22, 38, ns)], axis=1)
    r = rng.uniform(0.3, 0.9, ns) if ns > 1 else np.array([4.0])
    col = rng.integers(20, 255, size=(ns, 3))
    sph = np.concatenate([c, r[:, None], col], axis=1).astype(np.float32)
    pl = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 60, 60]], dtype=np.float32)
    p = O.camera_params(EDGE_W, EDGE_H, pos=(0.0, 12.0, 0.0), rot=(0.3, RS.PI32, 0.0))
    return p, sph, pl


@pytest.mark.parametrize("ns", [1, 33, 256, 257, 512, 513, 1537])
def test_the_walks_and_lists_edges(R, ns):
    p, sph, pl = edge_scene(ns)
    pp = TC._params(p)
    at = sorted({i for i in EDGES + (ns - 1,) if i < ns})
    light = R.make_light(pos=(1.0, 60.0, 28.0), diffuse_power=2500.0, specular_power=3000.0)
    seen = set()
    for only_those_cast in (False, True):
        casts = np.full(ns + 1, 1 if not only_those_cast else 0, dtype=np.uint8)
        casts[at] = 0 if not only_those_cast else 1
        casts[ns] = 1  # the floor
        u = [int(i) for i in np.flatnonzero(casts == 0)]
        casters = int(casts[:ns].sum())
        frames = []
        for store in ((0, 1) if ns >= 256 else (-1,)):
            with R.Context(EDGE_W, EDGE_H) as a, R.Context(EDGE_W, EDGE_H) as b:
                for c in (a, b):
                    c.set_option(R.OPT_SORTED_STORE, store)
                    c.set_scene(sph, pl)
                    c.set_light(light)
                    c.set_option(R.OPT_SHADOWS, 1)
                a.set_option(R.OPT_SHADOW_GRID, 1)
                TC._values(R, a, pp)
                fallback = a.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS)
                a.set_option(R.OPT_SHADOW_GRID, 0)
                a.set_shadow_casting(0, casts)
                assert [i for i in range(ns + 1) if a.get_shadow_casting(i) == 0] == u
                b.remove_objects(u)
                what = "%d spheres, %s, store %d" % (ns, "only the edges cast" if only_those_cast else "the edges cast none", store)
                va = _assert_non_casting_equals_removed(R, a, b, pp, what)
                assert a.last_kernel.startswith("rtx_shadow_shade<"), a.last_kernel
                frames.append(va.tobytes())
                for opt in (R.OPT_SHADOW_CHECK, R.OPT_SHADOW_GRID, R.OPT_LIGHTS_CHECK):
                    a.set_option(opt, 1)
                    got = TC._values(R, a, pp)
                    assert got.tobytes() == frames[-1], "%s: option %d changes %d pixels" % (what, opt, int((_u32(got) != _u32(va)).any(axis=1).sum()))
                    if opt == R.OPT_SHADOW_CHECK:  # every caster is a candidate wherever a pixel is pending, and nothing else is
                        assert a.get_option(R.STAT_SHADOW_LONGEST_LIST) == casters, (what, a.get_option(R.STAT_SHADOW_LONGEST_LIST), casters)
                    if opt == R.OPT_SHADOW_GRID:
                        assert "grid" in a.last_kernel
                        assert a.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS) == fallback
                    a.set_option(opt, 0)
        assert len(set(frames)) == 1, "RTX_OPT_SORTED_STORE changes the frame"
        seen.add(frames[0])
    if len(at) < ns:
        assert len(seen) == 2  # (the two masks are two pictures)


# ---------------------------------------------------------------- 6. no flags, no change

@pytest.mark.parametrize("path", ["direct", "shaded", "chain"])
def test_no_flags_no_change(R, path):
    p, sph, pl, ks, pix, trace = RH.traced("mirror_floor_shadows")
    pp = TC._params(p)
    n = len(sph) + len(pl)
    W, H = int(p.x), int(p.y)

    def make(c):
        c.set_scene(sph, pl)
        if path != "direct":
            TC._set_lights(R, c, RH.lights("mirror_floor_shadows", 3))
            c.set_option(R.OPT_SHADOWS, 1)
        if path == "chain":
            T._set_k(c, ks)
            c.set_option(R.OPT_REFLECT_DEPTH, 2)
            c.set_option(R.OPT_REFLECT_SHADOWS, 1)

    def frames(c):
        out = []
        for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_PIXEL, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES)):
            out.append((T._rows(R, c, pp, mode, flags).tobytes(), c.last_kernel))
        return out

    with R.Context(W, H) as never, R.Context(W, H) as c:
        make(never)
        make(c)
        want = frames(never)
        c.set_shadow_casting(0, np.ones(n, dtype=np.uint8))  # set to what they are
        assert frames(c) == want
        c.set_shadow_casting(0, RC.even_spheres(len(sph), len(pl)))
        with_flags = frames(c)
        if path == "direct":  # no shadow test: nobody reads the flags
            assert with_flags == want
        else:
            assert [f[0] for f in with_flags] != [f[0] for f in want]
            c.set_option(R.OPT_SHADOW_CHECK, 2)  # the test that tests nothing: the same
            never.set_option(R.OPT_SHADOW_CHECK, 2)
            assert frames(c) == frames(never)
            c.set_option(R.OPT_SHADOW_CHECK, 0)
            never.set_option(R.OPT_SHADOW_CHECK, 0)
            c.set_option(R.OPT_SHADOWS, 0)
            never.set_option(R.OPT_SHADOWS, 0)
            assert frames(c) == frames(never)
            c.set_option(R.OPT_SHADOWS, 1)
            never.set_option(R.OPT_SHADOWS, 1)
        assert _shadowless(c, n) == (len(sph) + 1) // 2
        c.set_shadow_casting(0, np.ones(n, dtype=np.uint8))  # cleared again
        assert _shadowless(c, n) == 0
        assert frames(c) == want


# ---------------------------------------------------------------- 5. lives

LW, LH, LMODE = TM.W, TM.H, TM.MODE
CASTS = {2: 0, 5: 0}  # (by creation index; 5: the plane)
LIVE_LIGHT = (-6.0, 40.0, 24.0)  # (above the left column: sphere 2's shadow falls on sphere 0 and the floor, sphere 3's on sphere 1)


def _live_context(R, spheres, planes, casts, devices=None, shadows=1):
    c = R.Context(LW, LH) if devices is None else R.Context(LW, LH, devices=devices)
    c.set_scene(spheres, planes)
    c.set_option(R.OPT_SHADOWS, shadows)
    c.set_light(R.make_light(pos=LIVE_LIGHT))
    c.set_patterns([R.make_pattern(*t) for t in TM.TABLE])
    TM._apply(c, TM.STATE)
    for i, v in casts.items():
        c.set_shadow_casting(i, [v])
    return c


def _live_frame(R, c, pose=TM.POSES[0]):
    return T._rows(R, c, R.camera_params(LW, LH, *pose), LMODE).tobytes()


def test_the_flags_show_in_this_view(R):
    with _live_context(R, TM.SPHERES, TM.PLANE, CASTS) as c, _live_context(R, TM.SPHERES, TM.PLANE, {}) as plain:
        assert _live_frame(R, c) != _live_frame(R, plain)
        assert _shadowless(c, TM.N) == len(CASTS) and _shadowless(plain, TM.N) == 0
        assert c.get_option(R.STAT_REFLECT_FRAMES) == plain.get_option(R.STAT_REFLECT_FRAMES) == 1  # (counted as the path's frames are)
    # shadows off: the flags are kept, nobody reads them, and the bytes are those without flags
    with _live_context(R, TM.SPHERES, TM.PLANE, CASTS, shadows=0) as c, _live_context(R, TM.SPHERES, TM.PLANE, {}, shadows=0) as plain:
        assert _live_frame(R, c) == _live_frame(R, plain)
        assert _shadowless(c, TM.N) == len(CASTS)


def test_edits_physics_removal_and_clear(R):
    n = TM.N
    moved = TM.SPHERES.copy()
    moved[2, 1] += 1.0
    flags = lambda c, k: [c.get_shadow_casting(i) for i in range(k)]
    want = [CASTS.get(i, 1) for i in range(n)]
    with _live_context(R, TM.SPHERES, TM.PLANE, CASTS) as c:
        before = _live_frame(R, c)
        c.set_spheres(2, moved[2])  # an edit keeps the flag
        got = _live_frame(R, c)
        assert flags(c, n) == want
        with _live_context(R, moved, TM.PLANE, CASTS) as fresh:
            assert got == _live_frame(R, fresh) and got != before
        c.update_objects(0.016)  # physics moves spheres, not flags
        assert flags(c, n) == want
        c.set_spheres(0, moved)  # (every sphere back where it was)
        assert _live_frame(R, c) == got
        c.remove_objects([0])  # the survivors keep theirs under the renumbering
        after = _live_frame(R, c)
        assert flags(c, n - 1) == want[1:]
        survivors = {name: {i - 1: v for i, v in TM.STATE[name].items() if i != 0} for name in TM.STATE}
        with R.Context(LW, LH) as fresh:
            fresh.set_scene(moved[1:], TM.PLANE)
            fresh.set_option(R.OPT_SHADOWS, 1)
            fresh.set_light(R.make_light(pos=LIVE_LIGHT))
            fresh.set_patterns([R.make_pattern(*t) for t in TM.TABLE])
            TM._apply(fresh, survivors)
            for i, v in CASTS.items():
                if i != 0:
                    fresh.set_shadow_casting(i - 1, [v])
            assert after == _live_frame(R, fresh) and after != got
        c.scene_clear()  # forgotten
        assert c.object_count == 0
        c.set_scene(TM.SPHERES, TM.PLANE)
        assert flags(c, n) == [1] * n


def test_a_graph_recorded_before_a_change_is_refused(R):
    import torch
    pp = R.camera_params(LW, LH)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * LW * LH, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with _live_context(R, TM.SPHERES, TM.PLANE, CASTS) as c:
        last = _live_frame(R, c)  # (render once before capturing: the device copies are uploaded here)
        before = TM._record(R, c, pp, s, buf)
        try:
            assert TM._replay(c, before, s, buf) == last
            c.set_shadow_casting(3, [0])
            with pytest.raises(R.RtxError) as e:
                c.graph_launch(before, s.cuda_stream)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and "shadow-casting flags changed" in str(e.value) and "re-capture" in str(e.value)
        finally:
            c.graph_destroy(before)
        got = _live_frame(R, c)
        assert got != last
        with _live_context(R, TM.SPHERES, TM.PLANE, {**CASTS, 3: 0}) as fresh:
            assert got == _live_frame(R, fresh)
        recorded = TM._record(R, c, pp, s, buf)
        try:
            assert TM._replay(c, recorded, s, buf) == got
        finally:
            c.graph_destroy(recorded)


def test_a_group_of_three_ranks_gives_the_one_device_frame(R):
    pp = R.camera_params(LW, LH)
    with _live_context(R, TM.SPHERES, TM.PLANE, CASTS) as c, _live_context(R, TM.SPHERES, TM.PLANE, CASTS, devices=[0, 0, 0]) as g:
        want = c.render_to_host(pp, LMODE)
        assert np.array_equal(g.render_to_host(pp, LMODE), want)
        with pytest.raises(R.RtxError) as e:  # validated on the root before any rank is touched: a refusal changes nothing
            g.set_shadow_casting(0, [1, 1, 2, 0])
        assert "object 2:" in str(e.value)
        assert [g.get_shadow_casting(i) for i in range(TM.N)] == [CASTS.get(i, 1) for i in range(TM.N)]
        assert np.array_equal(g.render_to_host(pp, LMODE), want)
        g.set_shadow_casting(3, [0])
        c.set_shadow_casting(3, [0])
        other = c.render_to_host(pp, LMODE)
        assert not np.array_equal(other, want) and np.array_equal(g.render_to_host(pp, LMODE), other)


def test_update_and_update_half_show_the_result(R):
    mode = O.RGB_PIXEL
    console = R.camera_params(LW, LH)
    console.y = LH // 2
    pp = TH.sample_params(R, console)
    assert (int(pp.x), int(pp.y)) == (LW, LH)
    streams, texts = {}, {}
    for name, casts in (("flags", CASTS), ("plain", {})):
        with _live_context(R, TM.SPHERES, TM.PLANE, casts) as c:
            words = T._rows(R, c, pp, mode, R.RENDER_COMPACT).view(np.uint32)
            stream = bytes(c.update_half(console, mode))
            assert stream == TH.run_half(R, c, mode, LW, LH // 2, words)
            assert RHALF.replay(mode, stream, LW, LH // 2) == RHALF.keys(mode, LW, LH // 2, words)
            streams[name] = stream
            texts[name] = bytes(c.update(R.camera_params(LW, LH), mode))
    assert streams["flags"] != streams["plain"] and texts["flags"] != texts["plain"]
