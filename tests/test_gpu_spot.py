"""Spot lights on the GPU (rtx_scene_set_spots, include/rtx.h) against tests/restate_spot.py, whose inputs
tests/test_host_restate_spot.py judges on the CPU.  The scene is restate.chain_scene("mirror_floor_shadows") under
restate.shadow_lights(name, 3) with the cones of restate_spot.CONES, at 320 x 180 through RTX_RENDER_VALUES: all eight floats of
every pixel bit for bit (restate.same_floats), shadowed frames included -- restate_spot.dark_sets_spot restates the kernels' exact
shadow tests in fp32 and adds the lights a point lies outside the cone of.
  1. one custom light with a cone (rtx_shadow_shade), shadows off and on; the three-light set (rtx_lights_shade);
  2. mirrors at depth 1 and depth 3 (rtx_reflect_shade / rtx_lights_reflect_shade, rtx_lights_chain_shade), RTX_OPT_REFLECT_SHADOWS at
     depth 3; RTX_OPT_SHADOW_GRID and RTX_OPT_REFLECT_GRID on give the bytes they give off (the four grid families and both shadow
     passes in their SPOT form);
  3. a mixed set (light 1 a point light); beside a finish and a pattern on the floor, and sphere 1 as glass;
  4. records and compact words of one case are the encoders' of the restated values;
  5. a cone on the default light alone makes a direct frame a shaded one, n = 0 makes it direct again with the bytes of a context
     that never had a cone; rtx_scene_set_lights clears the cones; every refusal changes nothing; both counters;
  6. a cone aimed away from the whole frame gives the bytes of the same lights with both powers 0 and, with shadows on, leaves
     RTX_STAT_SHADOW_LONGEST_LIST at 0;
  7. a recorded graph replays the cones it was recorded with; three logical ranks, RTX_OPT_SUPERSAMPLE 2 and rtx_update_half."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_finish as RF
import restate_glass as RG
import restate_half as RH
import restate_pattern as RP
import restate_spot as SP
import restate_supersample as SS
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_half as TH

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 320, 180
FLOOR = 4
AWAY = ((0.0, 1.0, 0.0), 0.9, 0.95)  # straight up, 26 degrees wide: every light is above the whole scene


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(W, H)
    yield c
    c.close()


def _reset(R, c):
    TC._reset(R, c)  # (rtx_scene_set_light(NULL) among it: the cones are gone)
    for opt, v in ((R.OPT_REFLECT_SHADOWS, 0), (R.OPT_SHADOW_GRID, 0), (R.OPT_REFLECT_GRID, 0), (R.OPT_SORTED_STORE, -1), (R.OPT_SUPERSAMPLE, 1)):
        c.set_option(opt, v)
    c.scene_clear()
    c.set_patterns([])
    assert c.get_option(R.STAT_SPOT_LIGHTS) == 0


def _lights(n=3):
    return RS.shadow_lights(SP.SCENE, n)


def _load(R, c, n=3, mirrors=True, spots="scene"):
    """The scene on the context under its first n lights and their cones; returns (product params, lights, cones)."""
    p, sph, pl, ks, pix = SP.scene()[:5]
    assert (int(p.x), int(p.y)) == (W, H)
    c.set_scene(sph, pl)
    if mirrors:
        T._set_k(c, ks)
    lights = _lights(n)
    TC._set_lights(R, c, lights)
    spots = SP.scene_cones(lights) if spots == "scene" else spots
    c.set_spots(spots)
    assert c.get_option(R.STAT_SPOT_LIGHTS) == sum(0 if SP.is_point(s) else 1 for s in spots)
    return TC._params(p), lights, spots


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _differ(a, b, mask):
    return int((np.logical_or.reduce([a[q] != b[q] for q in range(3)]) & mask).sum())


# ---------------------------------------------------------------- 1. without mirrors: one light, three lights, shadows off and on

@pytest.mark.parametrize("shadows", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
def test_the_kernels_without_mirrors(R, ctx, n, shadows):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, n, mirrors=False)
    trace = SP.scene()[6]
    ctx.set_option(R.OPT_SHADOWS, shadows)
    frames0 = ctx.get_option(R.STAT_SPOT_FRAMES)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_shadow_shade<" if n == 1 else "rtx_lights_shade<"), ctx.last_kernel
    dark0 = SP.dark_sets_spot(trace, lights, spots, False)[0] if shadows else 0
    want = SP.shade_plain_spot(trace, lights, spots, None, dark0)
    TC._assert_values(got, trace, want, "%d lights, shadows %d" % (n, shadows))
    assert _differ(want, RF.shade_plain_finish(trace, lights, None, RG.dark_sets(trace, lights, False)[0] if shadows else 0), trace["vis"]) >= 10000  # (the cones are in the picture)
    if shadows:
        assert _differ(want, SP.shade_plain_spot(trace, lights, spots), trace["vis"]) >= 100  # (and so are shadows inside them)
        ctx.set_option(R.OPT_SHADOW_GRID, 1)
        grid = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith("rtx_grid_shade<"), ctx.last_kernel
        assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    assert ctx.get_option(R.STAT_SPOT_FRAMES) == frames0 + 1 + shadows
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. mirrors, shadows at every level, the grids

@pytest.mark.parametrize("n", [1, 3])
def test_mirror_kernels_at_depths_1_and_3(R, ctx, n):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, n)
    trace = SP.scene()[5]
    want = SP.shade_chain_spot(trace, lights, spots, depths=[1, 3])
    plain = RS.shade_chain(trace, lights)
    one_bounce = "rtx_reflect_shade<" if n == 1 else "rtx_lights_reflect_shade<"
    for depth, check, kernel in ((1, 0, one_bounce), (1, 1, "rtx_lights_chain_shade<"), (3, 0, "rtx_lights_chain_shade<")):
        ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
        ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, check)
        got = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
        TC._assert_values(got, trace, want[depth], "%d lights, depth %d on %s" % (n, depth, kernel))
        assert _differ(want[depth], plain[depth], trace["vis"]) >= 10000  # (the cones are in the picture)
    _reset(R, ctx)


@pytest.mark.parametrize("n", [1, 3])
def test_level_0_shadows_under_mirrors_and_through_the_grids(R, ctx, n):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, n)
    trace = SP.scene()[5]
    ctx.set_option(R.OPT_SHADOWS, 1)
    dark = SP.dark_sets_spot(trace, lights, spots, False)
    one_bounce = "rtx_reflect_shade<" if n == 1 else "rtx_lights_reflect_shade<"
    for depth, kernel, grid_kernel in ((1, one_bounce, "rtx_grid_reflect_shade<"), (2, "rtx_lights_chain_shade<", "rtx_grid_chain_shade<")):
        ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
        got = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
        want = SP.shade_chain_spot(trace, lights, spots, None, dark0=dark[0], depths=[depth])[depth]
        TC._assert_values(got, trace, want, "%d lights, shadows, depth %d" % (n, depth))
        assert _differ(want, SP.shade_chain_spot(trace, lights, spots, depths=[depth])[depth], trace["vis"]) >= 100  # (shadows are in the picture)
        ctx.set_option(R.OPT_SHADOW_GRID, 1)
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        grid = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(grid_kernel), ctx.last_kernel
        assert np.array_equal(_bits(grid), _bits(got)), "the grid options change bytes at depth %d" % depth
        ctx.set_option(R.OPT_SHADOW_GRID, 0)
        ctx.set_option(R.OPT_REFLECT_GRID, 0)
    _reset(R, ctx)


@pytest.mark.parametrize("n", [1, 3])
def test_shadows_seen_in_mirrors(R, ctx, n):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, n)
    trace = SP.scene()[5]
    depth = 3
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shadow_shade<"), ctx.last_kernel
    dark = SP.dark_sets_spot(trace, lights, spots, True)
    want = SP.shade_chain_spot(trace, lights, spots, None, dark0=dark[0], deep_dark=dark[1:], depths=[depth])[depth]
    TC._assert_values(got, trace, want, "%d lights, shadows at every level" % n)
    level0_only = SP.shade_chain_spot(trace, lights, spots, None, dark0=dark[0], depths=[depth])[depth]
    assert _differ(want, level0_only, trace["vis"]) >= 50  # (deeper shadows are in the picture)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<"), ctx.last_kernel
    assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    both = TC._values(R, ctx, pp)
    assert np.array_equal(_bits(both), _bits(got)), "both grids change bytes"
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. a mixed set; beside finishes, patterns and glass

def test_a_point_light_among_cones(R, ctx):
    _reset(R, ctx)
    lights = _lights(3)
    cones = SP.scene_cones(lights)
    mixed = [cones[0], ((0.0, 0.0, 0.0), 0.3, 0.9), cones[2]]
    pp, lights, spots = _load(R, ctx, 3, spots=mixed)
    got_spots = ctx.get_spots()
    assert (tuple(got_spots[1].dir), got_spots[1].cos_outer, got_spots[1].cos_inner) == ((0.0, 0.0, 0.0), 0.0, 0.0)  # five zeros
    trace = SP.scene()[5]
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    dark = SP.dark_sets_spot(trace, lights, mixed, True)
    want = SP.shade_chain_spot(trace, lights, mixed, None, dark0=dark[0], deep_dark=dark[1:], depths=[3])[3]
    TC._assert_values(TC._values(R, ctx, pp), trace, want, "light 1 a point light")
    all_cones = SP.dark_sets_spot(trace, lights, cones, True)
    assert _differ(want, SP.shade_chain_spot(trace, lights, cones, None, dark0=all_cones[0], deep_dark=all_cones[1:], depths=[3])[3], trace["vis"]) >= 1000
    _reset(R, ctx)


def test_beside_a_finish_a_pattern_and_glass(R, ctx):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, 3)
    p, sph, pl, ks, pix = SP.scene()[:5]
    fin = {FLOOR: (0.3, 0.8, 1.6, 3), 1: (0.1, 0.8, 1.7, 7)}
    for i, f in fin.items():
        ctx.set_finish(i, [f])
    table = RP.SCENE_A_TABLE[:1]
    ctx.set_patterns([R.make_pattern(*t) for t in table])
    ctx.set_object_pattern(FLOOR, 1)
    ctx.set_refraction(1, 1.5)
    trace = RP.patterned(RG.trace_chain_glass(p, sph, pl, ks, {1: 1.5}, pix, max_depth=2), table, {FLOOR: 1})
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    want = SP.shade_chain_spot(trace, lights, spots, fin, depths=[2])[2]
    TC._assert_values(TC._values(R, ctx, pp), trace, want, "finish, pattern, glass")
    assert ctx.get_option(R.STAT_FINISHED_OBJECTS) == 2
    # each of the three is in the picture
    assert _differ(want, SP.shade_chain_spot(trace, lights, spots, None, depths=[2])[2], trace["vis"]) >= 100
    assert _differ(want, SP.shade_chain_spot(SP.scene()[5], lights, spots, fin, depths=[2])[2], trace["vis"]) >= 100
    assert _differ(want, RF.shade_chain_finish(trace, lights, fin)[2], trace["vis"]) >= 10000
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. records and words

@pytest.mark.parametrize("mode", [O.BIT_ASCII, O.RGB_PIXEL])
def test_records_and_words_encode_the_values(R, ctx, mode):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, 3)
    trace = SP.scene()[5]
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    far = float(pp.cam_far)
    colour = SP.shade_chain_spot(trace, lights, spots, depths=[2])[2]
    want = RS.values8(trace, colour)
    TC._assert_values(TC._values(R, ctx, pp, mode), trace, colour, O.MODE_NAMES[mode])
    S = 12 if mode < O.RGB_ASCII else 20
    rec = T._rows(R, ctx, pp, mode).reshape(-1, S)
    assert np.array_equal(rec, RS.encode_records(want, mode, far))
    words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT).view(np.uint32)
    assert np.array_equal(words, RS.encode_words(want, mode, far))
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. the launches, the state, the refusals, the counters

def _frames(R, c, pp):
    out = []
    for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES), (O.BIT_PIXEL, 0)):
        out.append((T._rows(R, c, pp, mode, flags).tobytes(), c.last_kernel))
    return out


def test_a_cone_on_the_default_light_takes_the_shade_launch_and_n_0_gives_it_back(R):
    p, sph, pl = SP.scene()[:3]
    pp = TC._params(p)
    trace = SP.scene()[6]
    ref = RS.reference_light()
    cone = SP.cone(ref, (0.0, 2.0, 32.0), 14.0, 8.0)
    with R.Context(W, H) as c:  # (a context that never saw the call)
        c.set_scene(sph, pl)
        fresh = _frames(R, c, pp)
        normals = T._rows(R, c, pp, O.RGB_NORMALS).tobytes()
        direct = c.last_kernel
        assert all("shade" not in k for _, k in fresh) and c.get_option(R.STAT_SPOT_FRAMES) == 0
        # a point light, set explicitly, and n = 0: nothing changes
        c.set_spots([((0.0, 0.0, 0.0), 0.5, 0.7)])
        assert c.get_option(R.STAT_SPOT_LIGHTS) == 0 and _frames(R, c, pp) == fresh
        c.set_spots([])
        assert _frames(R, c, pp) == fresh and c.get_option(R.STAT_SPOT_FRAMES) == 0
        # the cone: the closest-hit launch and rtx_shadow_shade, with the restated values
        c.set_spots([cone])
        assert c.get_option(R.STAT_SPOT_LIGHTS) == 1 and c.get_option(R.STAT_LIGHTS) == 1
        got = TC._values(R, c, pp)
        assert c.last_kernel.startswith("rtx_shadow_shade<"), c.last_kernel
        TC._assert_values(got, trace, SP.shade_plain_spot(trace, [ref], [cone]), "a cone on the reference's light")
        shaded = _frames(R, c, pp)
        assert all(k.startswith("rtx_shadow_shade<") for _, k in shaded) and all(a[0] != b[0] for a, b in zip(shaded, fresh))
        assert c.get_option(R.STAT_SPOT_FRAMES) == 5 and c.get_option(R.STAT_FINISH_FRAMES) == 0
        # RGB_NORMALS does not shade: its launch and its bytes stay
        assert T._rows(R, c, pp, O.RGB_NORMALS).tobytes() == normals and c.last_kernel == direct
        assert c.get_option(R.STAT_SPOT_FRAMES) == 5
        # rtx_scene_clear leaves the cones alone, as it leaves the lights
        c.scene_clear()
        assert c.get_option(R.STAT_SPOT_LIGHTS) == 1
        c.set_scene(sph, pl)
        assert _frames(R, c, pp) == shaded
        # n = 0: the direct launch again, the first bytes again
        c.set_spots([])
        assert c.get_option(R.STAT_SPOT_LIGHTS) == 0
        assert _frames(R, c, pp) == fresh
        assert c.get_option(R.STAT_SPOT_FRAMES) == 9
        # and rtx_scene_set_light(NULL) clears a cone as well
        c.set_spots([cone])
        c.set_light(None)
        assert c.get_option(R.STAT_SPOT_LIGHTS) == 0 and _frames(R, c, pp) == fresh


def _spot_tuple(s):
    return (tuple(s.dir), s.cos_outer, s.cos_inner)


def test_set_lights_clears_the_cones_and_refusals_change_nothing(R, ctx):
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, 3, mirrors=False)
    L = R.lib()
    stored = [_spot_tuple(s) for s in ctx.get_spots()]
    assert len(stored) == 3
    for got, sp in zip(stored, spots):  # what is stored: the axis normalised in double, the cosines as given
        st = SP.stored(sp)
        assert got == ((st[0], st[1], st[2]), st[3], st[4])
    nan, inf = float("nan"), float("inf")
    ok = spots[0]
    for bad_set, offender in (([ok, ((nan, 0.0, 1.0), 0.5, 0.7), ok], 1), ([((1.0, inf, 0.0), 0.5, 0.7), ok, ok], 0), ([ok, ok, ((1e-25, 0.0, 0.0), 0.5, 0.7)], 2),
                              ([ok, ok, ((1e25, 0.0, 0.0), 0.5, 0.7)], 2), ([ok, ((0.0, -1.0, 0.0), nan, 0.7), ok], 1), ([ok, ((0.0, -1.0, 0.0), 0.5, inf), ok], 1),
                              ([((0.0, -1.0, 0.0), -1.5, 0.7), ok, ok], 0), ([ok, ok, ((0.0, -1.0, 0.0), 0.5, 1.5)], 2), ([ok, ((0.0, -1.0, 0.0), 0.7, 0.7), ((0.0, -1.0, 0.0), 0.9, 0.7)], 1),
                              ([ok, ok, ((0.0, -1.0, 0.0), 0.5, 0.5 + 2.0 ** -11)], 2), ([ok], None), ([ok, ok], None), ([ok] * 4, None), ([ok] * 8, None)):
        with pytest.raises(R.RtxError) as e:
            ctx.set_spots(bad_set)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
        if offender is not None:  # rtx_last_error names the first offending light
            assert "light %d:" % offender in str(e.value), str(e.value)
        else:
            assert "number of lights" in str(e.value), str(e.value)
        assert [_spot_tuple(s) for s in ctx.get_spots()] == stored and ctx.get_option(R.STAT_SPOT_LIGHTS) == 3
    assert L.rtx_scene_set_spots(ctx._h, 3, None) == R.ERR_INVALID_ARGUMENT  # spots == NULL with n > 0
    # rtx_scene_get_spots: min(capacity, n) entries, *n_out always the number of lights
    out = (R.Spot * 8)()
    out[2].cos_outer = 7.0
    n = C.c_size_t(99)
    assert L.rtx_scene_get_spots(ctx._h, 2, out, C.byref(n)) == R.OK and n.value == 3 and out[2].cos_outer == 7.0 and _spot_tuple(out[1]) == stored[1]
    assert L.rtx_scene_get_spots(ctx._h, 0, None, C.byref(n)) == R.OK and n.value == 3
    assert L.rtx_scene_get_spots(ctx._h, 2, None, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert [_spot_tuple(s) for s in ctx.get_spots()] == stored
    # the frame under the cones, then the same lights set again: point lights, the bytes of a set that never had cones
    trace = SP.scene()[6]
    TC._assert_values(TC._values(R, ctx, pp), trace, SP.shade_plain_spot(trace, lights, spots), "before")
    TC._set_lights(R, ctx, lights)
    assert ctx.get_option(R.STAT_SPOT_LIGHTS) == 0
    assert [_spot_tuple(s) for s in ctx.get_spots()] == [((0.0, 0.0, 0.0), 0.0, 0.0)] * 3
    frames = ctx.get_option(R.STAT_SPOT_FRAMES)
    TC._assert_values(TC._values(R, ctx, pp), trace, RF.shade_plain_finish(trace, lights, None), "after rtx_scene_set_lights")
    assert ctx.last_kernel.startswith("rtx_lights_shade<") and ctx.get_option(R.STAT_SPOT_FRAMES) == frames
    _reset(R, ctx)


# ---------------------------------------------------------------- 6. cones that miss the frame

@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
def test_cones_aimed_away_are_lights_without_power_and_test_no_segment(R, ctx, n, grid):
    _reset(R, ctx)
    pp, lights, _ = _load(R, ctx, n, spots=[AWAY] * n)
    trace = SP.scene()[5]
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    ctx.set_option(R.OPT_SHADOW_GRID, grid)
    away = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<" if grid else "rtx_lights_chain_shadow_shade<"), ctx.last_kernel
    assert ctx.get_option(R.STAT_SHADOW_LONGEST_LIST) == 0
    if grid:
        assert ctx.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS) == 0
    # no pixel is inside a cone, at any level
    for j in range(4):
        assert all(c[1] == 0 and c[2] == 0 for c in SP.classes(trace, lights, [AWAY] * n, j))
    # the same lights with both powers 0, no cones: the same bytes -- and without cones the set does test segments
    TC._set_lights(R, ctx, [RS.dark(l) for l in lights])
    assert ctx.get_option(R.STAT_SPOT_LIGHTS) == 0
    powerless = TC._values(R, ctx, pp)
    assert np.array_equal(_bits(away), _bits(powerless))
    TC._assert_values(away, trace, RS.shade_chain(trace, [RS.dark(l) for l in lights])[3], "cones aimed away")
    if not grid:
        assert ctx.get_option(R.STAT_SHADOW_LONGEST_LIST) > 0
    _reset(R, ctx)


# ---------------------------------------------------------------- 7. graphs, groups, supersampling, half blocks

def test_a_recorded_graph_keeps_its_cones(R, ctx):
    import torch
    _reset(R, ctx)
    pp, lights, spots = _load(R, ctx, 3)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    mode = O.RGB_ASCII
    other = SP.scene_cones(lights, [((4.0, 0.0, 30.0), 18.0, 10.0), ((0.0, 2.0, 32.0), 15.0, 9.0), ((-5.0, 0.0, 26.0), 22.0, 12.0)])
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = T._rows(R, ctx, pp, mode).tobytes()  # (render once before capturing: the device copies are uploaded here)
    ctx.graph_begin(s.cuda_stream)
    ctx.render_rows(pp, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)

    def replay():
        buf.fill_(0xEE)
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        return buf.cpu().numpy().tobytes()

    try:
        assert replay() == first
        ctx.set_spots(other)  # no upload, no stale graph: the recorded launches carry their cones by value
        second = T._rows(R, ctx, pp, mode).tobytes()
        assert second != first
        assert replay() == first
        ctx.set_spots([])
        assert replay() == first
    finally:
        ctx.graph_destroy(g)
    _reset(R, ctx)


def _context(R, devices=None, w=W, h=H, spots="scene"):
    c = R.Context(w, h) if devices is None else R.Context(w, h, devices=devices)
    p, sph, pl, ks, pix = SP.scene()[:5]
    c.set_scene(sph, pl)
    T._set_k(c, ks)
    lights = _lights(3)
    TC._set_lights(R, c, lights)
    c.set_spots(SP.scene_cones(lights) if spots == "scene" else spots)
    c.set_option(R.OPT_REFLECT_DEPTH, 2)
    c.set_option(R.OPT_SHADOWS, 1)
    return c


def test_a_group_of_three_ranks_gives_the_one_device_frame(R):
    p = SP.scene()[0]
    pp = TC._params(p)
    trace = SP.scene()[5]
    lights = _lights(3)
    spots = SP.scene_cones(lights)
    mode = O.RGB_ASCII
    dark = SP.dark_sets_spot(trace, lights, spots, False)
    want = RS.encode_records(RS.values8(trace, SP.shade_chain_spot(trace, lights, spots, None, dark0=dark[0], depths=[2])[2]), mode, float(pp.cam_far))
    with _context(R, devices=[0, 0, 0]) as g:
        assert np.array_equal(g.render_to_host(pp, mode).reshape(-1, 20), want)
        assert g.get_option(R.STAT_SPOT_LIGHTS) == 3
        with pytest.raises(R.RtxError) as e:  # validated on the root before any rank is touched
            g.set_spots([spots[0], ((0.0, -1.0, 0.0), 0.9, 0.5), spots[2]])
        assert "light 1:" in str(e.value)
        assert np.array_equal(g.render_to_host(pp, mode).reshape(-1, 20), want)
        g.set_spots([])  # every rank's replica: point lights again
        d = RG.dark_sets(trace, lights, False)
        plain = RS.encode_records(RS.values8(trace, SP.shade_chain_spot(trace, lights, None, None, dark0=d[0], depths=[2])[2]), mode, float(pp.cam_far))
        assert np.array_equal(g.render_to_host(pp, mode).reshape(-1, 20), plain)


def _restated_frame():
    """(product params, trace, colour) of the frame _context() renders: depth 2, level 0 shadow-tested."""
    trace = SP.scene()[5]
    lights = _lights(3)
    spots = SP.scene_cones(lights)
    dark = SP.dark_sets_spot(trace, lights, spots, False)
    return TC._params(SP.scene()[0]), trace, SP.shade_chain_spot(trace, lights, spots, None, dark0=dark[0], depths=[2])[2]


def test_supersampling_folds_the_sample_frame_under_cones(R):
    S = 2
    w, h = W // S, H // S
    ps, trace, colour = _restated_frame()  # the sample frame is the restated one: p' = p with x = S W, y = S H
    p = R.Params.from_buffer_copy(bytes(ps))
    p.x, p.y = w, h
    assert bytes(SS.sample_params(p, S)) == bytes(ps)
    mode = O.RGB_ASCII
    with _context(R) as c:
        samples = T._rows(R, c, ps, mode, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
        TC._assert_values(samples, trace, colour, "the sample frame")
        want = SS.fold(RS.values8(trace, colour), w, h, S, float(p.cam_far))
        c.set_option(R.OPT_SUPERSAMPLE, S)
        got = T._rows(R, c, p, mode, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
        assert c.last_kernel.startswith("rtx_resolve<%d," % S), c.last_kernel
        same = RS.same_floats(got, want)
        assert same.all(), "%d cells differ" % int((~same.all(axis=1)).sum())
        assert c.get_option(R.STAT_SPOT_FRAMES) >= 2
    with _context(R, spots=[]) as c:  # (and the fold is of samples under cones)
        c.set_option(R.OPT_SUPERSAMPLE, S)
        assert T._rows(R, c, p, mode, R.RENDER_VALUES).tobytes() != got.tobytes()


def test_update_half_shows_the_cones(R):
    mode = O.RGB_PIXEL
    scene_pp, trace, colour = _restated_frame()  # the W x H pixel frame under the console's W x H/2 cells is the restated one
    console = R.Params.from_buffer_copy(bytes(scene_pp))
    console.y = H // 2
    pp = TH.sample_params(R, console)
    assert bytes(pp) == bytes(scene_pp)
    streams = {}
    for name, spots in (("cones", "scene"), ("plain", [])):
        with _context(R, spots=spots) as c:
            words = T._rows(R, c, pp, mode, R.RENDER_COMPACT).view(np.uint32)
            if name == "cones":
                assert np.array_equal(words, RS.encode_words(RS.values8(trace, colour), mode, float(pp.cam_far)))
            stream = bytes(c.update_half(console, mode))
            assert stream == TH.run_half(R, c, mode, W, H // 2, words)
            assert RH.replay(mode, stream, W, H // 2) == RH.keys(mode, W, H // 2, words)
            streams[name] = stream
    assert streams["cones"] != streams["plain"]
