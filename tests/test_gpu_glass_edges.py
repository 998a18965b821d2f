"""Glass on the GPU where objects do not stand clear of each other (rtx_scene_set_refraction, include/rtx.h): the ray through a
sphere starts on its far side, up to 2 r from the hit point, and in the scenes of tests/test_gpu_glass.py that point never lies in
another object.  Here it does.  Scene C (restate_glass.scene_c): glass spheres that overlap a glass sphere and two mirrors, one sunk
into the floor, so that rays start inside another sphere's cells and bounds and on the wrong side of a plane.  Scene D
(restate_glass.scene_d): 300 spheres (the direction-sorted copies exist) and a glass sphere that holds dozens of them and lies in
the world grid's large list.  Both again after rtx_update_objects has moved their spheres, against the restatement traced on the
positions rtx_scene_get_object reads back -- not against another frame of the same context.

Frames of 41 x 23 on one context; all eight value floats of every pixel bit for bit against tests/restate_glass.py
(test_gpu_chain_lights._assert_values), shadowed frames included.  tests/test_host_restate_glass.py judges the inputs on the CPU;
the counts it asserts are asserted here again before the comparisons they belong to.
  1. scene C through every secondary kernel: the default walk, RTX_OPT_REFLECT_CHECK, RTX_OPT_REFLECT_GRID, the rays per level;
  2. scene C's shadows at every level: culled, RTX_OPT_SHADOW_CHECK, RTX_OPT_SHADOW_GRID, both grids;
  3. scene D: the sorted store on and off, with and without the grid, the large list, shadows through the grid;
  4. both scenes after each of three rtx_update_objects steps;
  5. scene C after its steps on a device group of two ranks, and through rtx_update."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_glass as RG
import restate_pattern as RP
import restate_shadows as RH
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_glass as TG
import test_gpu_half as TH
from test_host_restate_glass import class_counts

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = RG.GW, RG.GH
C_SLOTS = {RG.C_FLOOR: 1}
STEPS, DT = 3, 0.2


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(2 * W, 2 * H)
    yield c
    c.close()


_bits = TG._bits
_reset = TG._reset
_lights = TG._lights


def _put(R, c, sph, pl, ks, iors):
    """The objects on the context; scene C (two planes) with its floor patterned as scene A's."""
    c.set_scene(sph, pl)
    TG._set_ks(c, ks)
    TG._set_glass(c, iors)
    if len(pl) == 2:
        c.set_patterns([R.make_pattern(*t) for t in TG.FLOOR_TABLE])
        c.set_object_pattern(RG.C_FLOOR, 1)


def _trace(scene, sph=None, max_depth=4):
    """The restatement of a scene (its spheres replaced by `sph`), scene C's floor patterned."""
    p, sph0, pl, ks, iors, pix, trace = scene
    if sph is not None:
        trace = RG.trace_chain_glass(p, sph, pl, ks, iors, pix, max_depth=max_depth)
    return RP.patterned(trace, TG.FLOOR_TABLE, C_SLOTS) if len(pl) == 2 else trace


_cache = {}


def _scene(name):
    """(scene tuple, product params, trace as rendered), once per module."""
    if name not in _cache:
        scene = getattr(RG, "scene_" + name)()
        _cache[name] = (scene, TC._params(scene[0]), _trace(scene))
    return _cache[name]


def _assert_c_classes(trace, what="scene C"):
    c = class_counts(trace, RG.C_FLOOR)
    print(what, "rays", trace["rays"], c)
    assert c["inside"] >= 75 and c["inside_hit"] >= 35, c
    assert c["beyond"] >= 85, c
    return c


def _assert_d_classes(trace, what="scene D"):
    c = class_counts(trace, RG.D_FLOOR)
    big = sum(int((lev["glass"] & (lev["left"] == RG.D_BIG)).sum()) for lev in trace["levels"][1:])
    print(what, "rays", trace["rays"], "leave the big sphere", big, c)
    assert c["inside"] >= 45 and big >= 75 and c["glass"] >= 150, (big, c)
    return c


def _rays_are_finite(trace, depth):
    return all(np.isfinite(np.stack(lev["O"] + lev["D"])).all() for lev in trace["levels"][1:depth + 1])


# ---------------------------------------------------------------- 1. scene C, every secondary kernel

@pytest.mark.parametrize("depth,nl", [(1, 0), (2, 0), (4, 0), (3, 3)])
def test_scene_c_through_every_secondary_kernel(R, ctx, depth, nl):
    _reset(R, ctx)
    scene, pp, trace = _scene("c")
    c = _assert_c_classes(trace)
    assert c["beyond_hit"] >= 5 and set(c["levels"]) >= {1, 2, 3} and c["left"] == set(RG.C_GLASS)
    _put(R, ctx, *scene[1:5])
    lights = _lights(nl)
    if nl:
        TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    assert ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == len(RG.C_GLASS)
    got = TC._values(R, ctx, pp)
    want = RS.shade_chain(trace, lights)[depth]
    TC._assert_values(got, trace, want, "scene C, depth %d, %d lights" % (depth, nl))
    if depth > 1:
        assert TC._ray_stats(R, ctx)[:depth] == trace["rays"][:depth]
    ctx.set_option(R.OPT_REFLECT_CHECK, 1)
    brute = TC._values(R, ctx, pp)
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)
    assert np.array_equal(_bits(brute), _bits(got)), "RTX_OPT_REFLECT_CHECK 1 changes bytes"
    grid_frames = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == grid_frames + 1
    assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_REFLECT_GRID 1 changes bytes"
    assert TC._ray_stats(R, ctx)[:depth] == trace["rays"][:depth]
    fallback = int(ctx.get_option(R.STAT_REFLECT_GRID_FALLBACK_RAYS))
    print("depth %d: %d rays fell back from the grid" % (depth, fallback))
    if _rays_are_finite(trace, depth):
        assert fallback == 0
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. scene C, shadows at every level

@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("nl", [1, 3])
def test_scene_c_shadows_at_every_level(R, ctx, nl, deep):
    _reset(R, ctx)
    scene, pp, trace = _scene("c")
    _assert_c_classes(trace)
    _put(R, ctx, *scene[1:5])
    lights = _lights(nl)
    TC._set_lights(R, ctx, lights)
    depth = 3
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, deep)
    dark = RG.dark_sets(trace, lights, bool(deep))
    for j in (0, 1, 2) if deep else (0,):
        lev = trace["levels"][j]
        tested = np.zeros(trace["n"], dtype=bool)
        tested[lev["idx"][lev["gid"] >= 0]] = True
        if j == 0:
            tested &= trace["vis"] & (trace["t"] <= f32(pp.cam_far))
        assert (dark[j][tested] != 0).sum() >= 10 and (dark[j][tested] == 0).sum() >= 10, j
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shadow_shade<" if deep else "rtx_lights_chain_shade<"), ctx.last_kernel
    want = RH.shade_chain_dark(trace, lights, dark)[depth]
    TC._assert_values(got, trace, want, "scene C, %d lights, deep %d" % (nl, deep))
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = TC._values(R, ctx, pp)
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    assert np.array_equal(_bits(brute), _bits(got)), "RTX_OPT_SHADOW_CHECK 1 changes bytes"
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<" if deep else "rtx_grid_chain_shade<"), ctx.last_kernel
    assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    both = TC._values(R, ctx, pp)
    assert np.array_equal(_bits(both), _bits(got)), "both grids change bytes"
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. scene D: the sorted store, the large list

def test_scene_d_under_both_stores_and_the_grid(R, ctx):
    _reset(R, ctx)
    scene, pp, trace = _scene("d")
    _assert_d_classes(trace)
    depth = 3
    want = RS.shade_chain(trace, _lights(0))[depth]
    frames = {}
    for store in (-1, 0):
        ctx.set_option(R.OPT_SORTED_STORE, store)
        _put(R, ctx, *scene[1:5])
        ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
        assert ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == RG.D_NS // 4
        frames[store] = TC._values(R, ctx, pp)
        TC._assert_values(frames[store], trace, want, "scene D, sorted store %d" % store)
        assert TC._ray_stats(R, ctx)[:depth] == trace["rays"][:depth]
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        grid = TC._values(R, ctx, pp)
        assert ctx.get_option(R.STAT_QUERY_LARGE_SPHERES) >= 1
        TC._assert_values(grid, trace, want, "scene D, sorted store %d, through the grid" % store)
        assert TC._ray_stats(R, ctx)[:depth] == trace["rays"][:depth]
        ctx.set_option(R.OPT_REFLECT_GRID, 0)
    assert np.array_equal(_bits(frames[-1]), _bits(frames[0]))
    _reset(R, ctx)


def test_scene_d_shadows_through_the_grid(R, ctx):
    _reset(R, ctx)
    scene, pp, trace = _scene("d")
    _assert_d_classes(trace)
    _put(R, ctx, *scene[1:5])
    lights = _lights(1)
    TC._set_lights(R, ctx, lights)
    depth = 3
    for opt, v in ((R.OPT_REFLECT_DEPTH, depth), (R.OPT_SHADOWS, 1), (R.OPT_REFLECT_SHADOWS, 1), (R.OPT_SHADOW_GRID, 1)):
        ctx.set_option(opt, v)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<"), ctx.last_kernel
    want = RH.shade_chain_dark(trace, lights, RG.dark_sets(trace, lights, True))[depth]
    TC._assert_values(got, trace, want, "scene D, shadows through the grid")
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. physics

C_MOTION = {0: (-1, 3.0), 4: (-1, 3.0), 5: (-1, 3.0), 7: (1, 2.0)}
D_MOTION = {i: (1 if (i // 3) % 2 else -1, 3.0) for i in range(0, RG.D_NS, 3)}


def _set_motion(c, motion):
    for i, (mover, speed) in motion.items():
        c.set_sphere_motion(i, mover, speed)


def _spheres(c, ns):
    """Every sphere as rtx_scene_get_object reads it back."""
    return np.array([c.get_object(i)[1][:7] for i in range(ns)], dtype=np.float32)


def _check_after_each_step(R, c, name, motion, assert_classes):
    """Three rtx_update_objects steps; after each, the restatement traced on the positions read back against the default walk,
    the reflect grid, and shadows at every level through the shadow grid.  Returns the spheres after the last step."""
    scene, pp, trace = _scene(name)
    ns = len(scene[1])
    depth = 3
    lights = _lights(1)
    _put(R, c, *scene[1:5])
    _set_motion(c, motion)
    TC._set_lights(R, c, lights)
    c.set_option(R.OPT_REFLECT_DEPTH, depth)
    assert np.array_equal(_spheres(c, ns), scene[1])
    before = TC._values(R, c, pp)
    TC._assert_values(before, trace, RS.shade_chain(trace, lights)[depth], "scene %s before the first step" % name.upper())
    sph = None
    for step in range(1, STEPS + 1):
        what = "scene %s after step %d" % (name.upper(), step)
        c.update_objects(DT)
        sph = _spheres(c, ns)
        moved = _trace(scene, sph, max_depth=depth)
        assert_classes(moved, what)
        got = TC._values(R, c, pp)
        TC._assert_values(got, moved, RS.shade_chain(moved, lights)[depth], what)
        assert TC._ray_stats(R, c)[:depth] == moved["rays"][:depth]
        assert not np.array_equal(_bits(got), _bits(before)), what + ": the step changed nothing"
        before = got
        c.set_option(R.OPT_REFLECT_GRID, 1)
        grid = TC._values(R, c, pp)
        c.set_option(R.OPT_REFLECT_GRID, 0)
        assert np.array_equal(_bits(grid), _bits(got)), what + ": RTX_OPT_REFLECT_GRID 1 changes bytes"
        for opt in (R.OPT_SHADOWS, R.OPT_REFLECT_SHADOWS, R.OPT_SHADOW_GRID):
            c.set_option(opt, 1)
        shadowed = TC._values(R, c, pp)
        for opt in (R.OPT_SHADOWS, R.OPT_REFLECT_SHADOWS, R.OPT_SHADOW_GRID):
            c.set_option(opt, 0)
        want = RH.shade_chain_dark(moved, lights, RG.dark_sets(moved, lights, True))[depth]
        TC._assert_values(shadowed, moved, want, what + ", shadows through the grid")
    return sph


def _steps_of_c(R, c):
    return _check_after_each_step(R, c, "c", C_MOTION, _assert_c_classes)


def test_scene_c_after_each_physics_step(R, ctx):
    _reset(R, ctx)
    sph0 = RG.C_SPH
    floor_y = float(RG.C_PL[0, 1])
    sph = _steps_of_c(R, ctx)
    # (a sphere nobody gave a motion falls at speed 1, as rtx_scene_add_spheres leaves it: every y has changed, and nothing else)
    assert (sph[:, 1] != sph0[:, 1]).all() and np.array_equal(np.delete(sph, 1, axis=1), np.delete(sph0, 1, axis=1))
    sunk_before, sunk_after = floor_y - float(sph0[RG.C_SUNK, 1] - sph0[RG.C_SUNK, 3]), floor_y - float(sph[RG.C_SUNK, 1] - sph[RG.C_SUNK, 3])
    print("sphere %d's lowest point below the floor: %.3f before, %.3f after" % (RG.C_SUNK, sunk_before, sunk_after))
    assert sunk_after > sunk_before > 0.0
    _reset(R, ctx)


@pytest.mark.parametrize("store", [-1, 0])
def test_scene_d_after_each_physics_step(R, ctx, store):
    _reset(R, ctx)
    ctx.set_option(R.OPT_SORTED_STORE, store)
    sph = _check_after_each_step(R, ctx, "d", D_MOTION, _assert_d_classes)
    sph0 = _scene("d")[0][1]
    assert (sph[:, 1] != sph0[:, 1]).all() and np.array_equal(np.delete(sph, 1, axis=1), np.delete(sph0, 1, axis=1))
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. inheritance at the edges

def test_a_device_group_and_update_after_the_steps(R, ctx):
    import torch
    _reset(R, ctx)
    scene, pp, _ = _scene("c")
    mode = O.RGB_ASCII
    sph = _steps_of_c(R, ctx)
    want = ctx.render_to_host(pp, mode)
    with R.Context(W, H, devices=[0, 0]) as g:
        _put(R, g, *scene[1:5])
        _set_motion(g, C_MOTION)
        TC._set_lights(R, g, _lights(1))
        g.set_option(R.OPT_REFLECT_DEPTH, 3)
        for _ in range(STEPS):
            g.update_objects(DT)
        assert np.array_equal(_spheres(g, len(sph)), sph)
        assert np.array_equal(g.render_to_host(pp, mode), want)
    # rtx_update: the Minimize of the rendered words
    vals = TC._values(R, ctx, pp, mode)
    words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT).view(np.uint32)
    assert np.array_equal(words, RS.encode_words(vals, mode, float(pp.cam_far)))
    tw = TH.to_device(words)
    out = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = ctx.minimize_words(mode, W, H, tw.data_ptr(), out.data_ptr())
    ctx.synchronize()
    before = ctx.get_option(R.STAT_REFRACT_FRAMES)
    assert bytes(ctx.update(pp, mode)) == bytes(out.cpu().numpy()[:n]) and n > 0
    assert ctx.get_option(R.STAT_REFRACT_FRAMES) > before
    _reset(R, ctx)
