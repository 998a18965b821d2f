"""Which object's finish a lane reads (rtx_scene_set_finish, include/rtx.h), on the GPU against tests/restate_finish.py.
tests/test_gpu_finish.py holds the rule to the restatement on scene F: spheres created first, one plane, fewer than 256 spheres,
every object clear of every other.  Here the finish is looked up where the `id` a level carries is most at risk:
  1. scene C (restate_glass.scene_c: overlapping glass, a sphere sunk into the floor, rays that start inside other objects; two
     planes with different finishes, the floor patterned) through every family that shades a chain, each of them again under
     RTX_OPT_REFLECT_CHECK, RTX_OPT_SHADOW_CHECK, RTX_OPT_SHADOW_GRID, RTX_OPT_REFLECT_GRID and both grids;
  2. scene C created with spheres and planes interleaved (restate_finish.creation_orders), its attributes set by creation index
     with ranges that run across a plane, read back, and again after the removal of a sphere;
  3. scene D (300 spheres: the kernels read the copies by sorted position) under both sorted stores, through the walk, the reflect
     grid and shadows through the shadow grid; again after an rtx_update_objects step has moved the copies, after the finished
     spheres have traded places (rtx_scene_set_spheres), and after a change of store has sorted them anew from another camera;
  4. scene E: the weights 0 and 16, m = 1, 2, 4, 6 and 8, a weight given as -0.0;
  5. a device group of two logical ranks on the interleaved scene.
Frames of 41 x 23 (scenes C and D) and 320 x 180 (scene E) on one context; all eight value floats of every pixel bit for bit
(test_gpu_chain_lights._assert_values), shadowed frames included.  tests/test_host_restate_finish.py judges the inputs on the CPU."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_finish as RF
import restate_glass as RG
import restate_pattern as RP
import restate_shadows as RH
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_finish as TF
import test_gpu_glass as TG
import test_gpu_glass_edges as TE

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = RG.GW, RG.GH
EW, EH = 320, 180
DEPTH = 3

_put, _scene, _trace, _lights, _reset = TE._put, TE._scene, TE._trace, TE._lights, TE._reset
_set_finishes = TF._set_finishes
_bits = TG._bits


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(EW, EH)
    yield c
    c.close()


def _kernel(depth, nl, shadows=0, deep=0, shadow_grid=0):
    """The shade launch rtxplan::plan_shading chooses (depth 0: no mirrors)."""
    grid = shadows and shadow_grid
    if deep:
        return "rtx_grid_chain_shadow_shade<" if grid else "rtx_lights_chain_shadow_shade<"
    if depth >= 2:
        return "rtx_grid_chain_shade<" if grid else "rtx_lights_chain_shade<"
    if grid:
        return ("rtx_grid_shade<", "rtx_grid_reflect_shade<")[depth]
    return (("rtx_shadow_shade<", "rtx_reflect_shade<") if nl == 1 else ("rtx_lights_shade<", "rtx_lights_reflect_shade<"))[depth]


def _render(R, c, pp, kernel, finished):
    """One values frame: the finished-object count before it, the launch's name and the finished-frame counter after it."""
    assert c.get_option(R.STAT_FINISHED_OBJECTS) == finished
    frames = c.get_option(R.STAT_FINISH_FRAMES)
    got = TC._values(R, c, pp)
    assert c.last_kernel.startswith(kernel), (c.last_kernel, kernel)
    assert c.get_option(R.STAT_FINISH_FRAMES) == frames + 1
    return got


def _want(trace, lights, finishes, depth, shadows=0, deep=0):
    """The restated colours: depth 0 without mirrors; shadows at level 0, `deep`: at every level (restate_glass.dark_sets)."""
    dark = RG.dark_sets(trace, lights, bool(deep)) if shadows else None
    if depth == 0:
        return RF.shade_plain_finish(trace, lights, finishes, dark[0] if shadows else 0)
    if not shadows:
        return RF.shade_chain_finish(trace, lights, finishes)[depth]
    return RF.shade_chain_finish(trace, lights, finishes, dark0=dark[0], deep_dark=dark[1:] if deep else None)[depth]


def _options(R, c, depth, shadows, deep):
    c.set_option(R.OPT_REFLECT_DEPTH, max(depth, 1))
    c.set_option(R.OPT_SHADOWS, shadows)
    c.set_option(R.OPT_REFLECT_SHADOWS, deep)


def _finish_tuple(f):
    return (f.ambient, f.diffuse, f.specular, f.shininess_log2)


def _stored(f):
    return tuple(f32(v) for v in f[:3]) + (f[3],)


# ---------------------------------------------------------------- 1. scene C, every family that shades a chain

C_CASES = [(1, 0, 0), (2, 0, 0), (4, 0, 0), (1, 1, 0), (DEPTH, 1, 0), (DEPTH, 1, 1)]  # (depth, RTX_OPT_SHADOWS, RTX_OPT_REFLECT_SHADOWS)


@pytest.mark.parametrize("nl", [1, 3])
@pytest.mark.parametrize("depth,shadows,deep", C_CASES)
def test_scene_c_through_every_family_and_every_option(R, ctx, depth, shadows, deep, nl):
    _reset(R, ctx)
    scene, pp, trace = _scene("c")
    fin = RF.C_FINISHES
    _put(R, ctx, *scene[1:5])
    _set_finishes(ctx, fin)
    lights = _lights(nl)
    TC._set_lights(R, ctx, lights)
    _options(R, ctx, depth, shadows, deep)
    what = "scene C, depth %d, %d lights, shadows %d, deep %d" % (depth, nl, shadows, deep)
    want = _want(trace, lights, fin, depth, shadows, deep)
    got = _render(R, ctx, pp, _kernel(depth, nl, shadows, deep), len(fin))
    TC._assert_values(got, trace, want, what)
    plain = (RS.shade_chain(trace, lights) if not shadows else RH.shade_chain_dark(trace, lights, RG.dark_sets(trace, lights, bool(deep))))[depth]
    assert TF._differ(want, plain, trace["vis"]) >= 100  # (the finishes are in the picture)
    grid_frames = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
    for options in ({R.OPT_REFLECT_CHECK: 1}, {R.OPT_SHADOW_CHECK: 1}, {R.OPT_SHADOW_GRID: 1}, {R.OPT_REFLECT_GRID: 1},
                    {R.OPT_SHADOW_GRID: 1, R.OPT_REFLECT_GRID: 1}):
        for opt, v in options.items():
            ctx.set_option(opt, v)
        other = _render(R, ctx, pp, _kernel(depth, nl, shadows, deep, options.get(R.OPT_SHADOW_GRID, 0)), len(fin))
        for opt in options:
            ctx.set_option(opt, 0)
        assert np.array_equal(_bits(other), _bits(got)), "%s: options %r change bytes" % (what, options)
    assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == grid_frames + 2
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. scene C, spheres and planes created interleaved

ORDERS = RF.creation_orders(len(RG.C_SPH), len(RG.C_PL))


def _create(c, order, sph, pl):
    """The objects through rtx_scene_add_sphere (a lone sphere), _add_spheres (a run of them) and _add_plane, in `order`."""
    c.scene_clear()
    at = 0
    while at < len(order):
        kind, i = order[at]
        if kind == "p":
            row = pl[i]
            assert c.add_plane(row[0:3], row[3:6], row[6:9], float(row[9]), float(row[10])) == at
            at += 1
            continue
        run = 1
        while at + run < len(order) and order[at + run][0] == "s":
            run += 1
        if run == 1:
            assert c.add_sphere(float(sph[i, 3]), sph[i, 0:3], sph[i, 4:7]) == at
        else:
            c.add_spheres(sph[i:i + run])
        at += run
    assert c.object_count == len(order)


def _dress_c(R, c, index):
    """Scene C's k, ior, pattern slot and finish on objects created in another order: index[restatement's index] = creation index.
    The slot and the finishes go in by ranges that run across a plane."""
    n = len(index)
    for i, k in RG.C_KS.items():
        c.set_reflectivity(int(index[i]), k)
    for i, ior in RG.C_IORS.items():
        c.set_refraction(int(index[i]), ior)
    c.set_patterns([R.make_pattern(*t) for t in TG.FLOOR_TABLE])
    floor = int(index[RG.C_FLOOR])
    first = max(floor - 1, 0)
    c.set_object_pattern(first, 1, n=floor - first + 2)  # (the object before the floor if there is one, the floor, the one after)
    for i in range(first, floor + 2):
        if i != floor:
            c.set_object_pattern(i, 0)
    fin = RF.by_creation(RF.C_FINISHES, index)
    c.set_finish(0, [fin.get(i, RF.DEFAULT) for i in range(n)])  # (one call for every object: sphere, plane, sphere, ...)
    assert c.get_option(R.STAT_FINISHED_OBJECTS) == len(fin)


def _read_back(c, index, ks, iors, slots, fin):
    for i, ci in enumerate(int(v) for v in index):
        assert c.get_reflectivity(ci) == float(f32(ks.get(i, 0.0))) and c.get_refraction(ci) == float(f32(iors.get(i, 0.0))), (i, ci)
        assert c.get_object_pattern(ci) == slots.get(i, 0), (i, ci)
        assert _finish_tuple(c.get_finish(ci)) == _stored(fin.get(i, RF.DEFAULT)), (i, ci)


def _without(values, gone):
    """{index: value} after object `gone` has left: the later ones move down by one."""
    return {i - (i > gone): v for i, v in values.items() if i != gone}


def _shadowed_three_lights(R, c):
    lights = _lights(3)
    TC._set_lights(R, c, lights)
    _options(R, c, DEPTH, 1, 1)
    return lights


@pytest.mark.parametrize("which", range(len(ORDERS)))
def test_scene_c_created_in_another_order(R, ctx, which):
    _reset(R, ctx)
    order, index = ORDERS[which]
    scene, pp, trace = _scene("c")
    p, sph, pl, ks, iors, pix = scene[:6]
    _create(ctx, order, sph, pl)
    types = [ctx.get_object(i)[0] for i in range(len(order))]
    assert len(set(types)) == 2 and [t == types[int(index[0])] for t in types] == [k == "s" for k, _ in order]
    _dress_c(R, ctx, index)
    _read_back(ctx, index, ks, iors, TE.C_SLOTS, RF.C_FINISHES)
    lights = _shadowed_three_lights(R, ctx)
    got = _render(R, ctx, pp, _kernel(DEPTH, 3, 1, 1), len(RF.C_FINISHES))
    TC._assert_values(got, trace, _want(trace, lights, RF.C_FINISHES, DEPTH, 1, 1), "scene C in creation order %d" % which)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    grid = _render(R, ctx, pp, _kernel(DEPTH, 3, 1, 1, 1), len(RF.C_FINISHES))
    assert np.array_equal(_bits(grid), _bits(got)), "both grids change bytes"
    ctx.set_option(R.OPT_SHADOW_GRID, 0)
    ctx.set_option(R.OPT_REFLECT_GRID, 0)
    # the sphere created right after the first plane leaves: the survivors' attributes move with them
    after_plane = order.index(("p", 0)) + 1
    kind, gone = order[after_plane]
    assert kind == "s"
    ctx.remove_objects([after_plane])
    ks2, iors2, fin2, slots2 = (_without(v, gone) for v in (ks, iors, RF.C_FINISHES, TE.C_SLOTS))
    index2 = np.array([ci - (ci > after_plane) for i, ci in enumerate(index) if i != gone])
    _read_back(ctx, index2, ks2, iors2, slots2, fin2)
    less = RP.patterned(RG.trace_chain_glass(p, np.delete(sph, gone, axis=0), pl, ks2, iors2, pix, max_depth=DEPTH), TG.FLOOR_TABLE, slots2)
    got2 = _render(R, ctx, pp, _kernel(DEPTH, 3, 1, 1), len(fin2))
    TC._assert_values(got2, less, _want(less, lights, fin2, DEPTH, 1, 1), "scene C in creation order %d without sphere %d" % (which, gone))
    assert not np.array_equal(_bits(got2), _bits(got))
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. scene D: the copies by sorted position, re-sorted

SIDE_POS, SIDE_ROT = (30.0, 12.0, 32.0), (0.3, RS.PI32 * 0.5, 0.0)  # (scene D from its right-hand side)


@pytest.mark.parametrize("store", [-1, 0])
def test_scene_d_under_a_sorted_store_before_and_after_a_step(R, ctx, store):
    _reset(R, ctx)
    scene, pp, trace = _scene("d")
    fin = RF.d_finishes()
    ctx.set_option(R.OPT_SORTED_STORE, store)
    _put(R, ctx, *scene[1:5])
    _set_finishes(ctx, fin)
    TE._set_motion(ctx, TE.D_MOTION)
    three, one = _lights(3), _lights(1)

    def check(trace, what, pp=pp):
        TC._set_lights(R, ctx, three)
        _options(R, ctx, DEPTH, 0, 0)
        want = _want(trace, three, fin, DEPTH)
        TC._assert_values(_render(R, ctx, pp, _kernel(DEPTH, 3), len(fin)), trace, want, what + ", the walk")
        assert TC._ray_stats(R, ctx)[:DEPTH] == trace["rays"][:DEPTH]
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        grid_frames = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
        TC._assert_values(_render(R, ctx, pp, _kernel(DEPTH, 3), len(fin)), trace, want, what + ", the reflect grid")
        assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == grid_frames + 1 and ctx.get_option(R.STAT_QUERY_LARGE_SPHERES) >= 1
        ctx.set_option(R.OPT_REFLECT_GRID, 0)
        return want

    before = check(trace, "scene D, sorted store %d" % store)
    assert TF._differ(before, RS.shade_chain(trace, three)[DEPTH], trace["vis"]) >= 100  # (the finishes are in the picture)
    TC._set_lights(R, ctx, one)
    _options(R, ctx, DEPTH, 1, 1)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    got = _render(R, ctx, pp, _kernel(DEPTH, 1, 1, 1, 1), len(fin))
    TC._assert_values(got, trace, _want(trace, one, fin, DEPTH, 1, 1), "scene D, sorted store %d, shadows through the grid" % store)
    ctx.set_option(R.OPT_SHADOW_GRID, 0)
    # one step: every third sphere moves, the copies are sorted again
    ctx.update_objects(TE.DT)
    sph = TE._spheres(ctx, RG.D_NS)
    assert (sph[:, 1] != scene[1][:, 1]).all()
    moved = _trace(scene, sph, max_depth=DEPTH)
    after = check(moved, "scene D, sorted store %d, after the step" % store)
    assert TF._differ(after, before, trace["vis"] & moved["vis"]) >= 100
    # a scene edit: the finished spheres trade places, the next frame sorts anew and the finishes have to follow their spheres
    third = np.arange(0, RG.D_NS, 3)
    edited = sph.copy()
    edited[third, :4] = sph[third[::-1], :4]
    ctx.set_spheres(0, edited)
    assert np.array_equal(TE._spheres(ctx, RG.D_NS), edited)
    traded = _trace(scene, edited, max_depth=DEPTH)
    last = check(traded, "scene D, sorted store %d, after the spheres traded places" % store)
    assert TF._differ(last, after, moved["vis"] & traded["vis"]) >= 100
    # the other store and back, the first frame after each change seen from the side: a sort from another origin, with no attribute touched
    side_p = O.camera_params(W, H, pos=SIDE_POS, rot=SIDE_ROT)
    side = RG.trace_chain_glass(side_p, edited, *scene[2:6], max_depth=DEPTH)
    assert side["vis"].sum() >= W * H // 2 and side["rays"][1] >= 200  # (the scene fills the side view, with chains to look up finishes in)
    for s in (-1 - store, store):
        ctx.set_option(R.OPT_SORTED_STORE, s)
        check(side, "scene D from the side, sorted store %d" % s, TC._params(side_p))
        check(traded, "scene D from the front again, sorted store %d" % s)
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. scene E: the ends of the ranges

def _put_e(c, mirrors, finishes=RF.E_FINISHES):
    p, sph, pl, ks = RF.scene_e()[:4]
    c.set_scene(sph, pl)
    if mirrors:
        T._set_k(c, ks)
    _set_finishes(c, finishes)
    return TC._params(p)


@pytest.mark.parametrize("which", ["1custom", "8"])
def test_scene_e_the_ends_of_the_weights_and_of_m(R, ctx, which):
    _reset(R, ctx)
    E = RF.E_FINISHES
    chain, plain = RF.scene_e()[5:7]
    lights = RS.chain_lights("mirror_floor", which)
    nl = len(lights)
    pp = _put_e(ctx, False)
    TC._set_lights(R, ctx, lights)
    for shadows in (0, 1):
        _options(R, ctx, 0, shadows, 0)
        got = _render(R, ctx, pp, _kernel(0, nl, shadows), len(E))
        TC._assert_values(got, plain, _want(plain, lights, E, 0, shadows), "scene E, %s, shadows %d" % (which, shadows))
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = _render(R, ctx, pp, _kernel(0, nl, 1, 0, 1), len(E))
    assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    assert TF._differ(_want(plain, lights, E, 0), _want(plain, lights, None, 0), plain["vis"]) >= 10000  # (the finishes are in the picture)
    _reset(R, ctx)
    pp = _put_e(ctx, True)
    TC._set_lights(R, ctx, lights)
    _options(R, ctx, 2, 0, 0)
    got = _render(R, ctx, pp, _kernel(2, nl), len(E))
    TC._assert_values(got, chain, _want(chain, lights, E, 2), "scene E, %s, depth 2" % which)
    _reset(R, ctx)


def test_scene_e_a_weight_given_as_minus_zero_is_plus_zero(R, ctx):
    _reset(R, ctx)
    E = RF.E_FINISHES
    obj = RF.E_MINUS_ZERO
    given = E[obj]
    assert given[2] == 0.0 and np.signbit(given[2])
    plus = {**E, obj: given[:2] + (0.0,) + given[3:]}
    lights = RS.chain_lights("mirror_floor", "1custom")
    frames = []
    with R.Context(EW, EH) as other:
        for c, finishes in ((ctx, E), (other, plus)):
            pp = _put_e(c, True, finishes)
            read = c.get_finish(obj)
            assert read.specular == 0.0 and not np.signbit(read.specular) and _finish_tuple(read) == _stored(plus[obj])
            TC._set_lights(R, c, lights)
            _options(R, c, 2, 0, 0)
            frames.append(_render(R, c, pp, _kernel(2, 1), len(E)))
    assert np.array_equal(_bits(frames[0]), _bits(frames[1]))
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. a device group

def test_a_device_group_of_two_ranks_on_the_interleaved_scene(R, ctx):
    _reset(R, ctx)
    order, index = ORDERS[1]
    scene, pp, trace = _scene("c")
    sph, pl = scene[1:3]
    _create(ctx, order, sph, pl)
    _dress_c(R, ctx, index)
    lights = _shadowed_three_lights(R, ctx)
    got = _render(R, ctx, pp, _kernel(DEPTH, 3, 1, 1), len(RF.C_FINISHES))
    TC._assert_values(got, trace, _want(trace, lights, RF.C_FINISHES, DEPTH, 1, 1), "scene C in creation order 1")
    want = ctx.render_to_host(pp, O.RGB_ASCII)
    with R.Context(W, H, devices=[0, 0]) as g:
        _create(g, order, sph, pl)
        _dress_c(R, g, index)
        _shadowed_three_lights(R, g)
        assert np.array_equal(g.render_to_host(pp, O.RGB_ASCII), want)
        plain = dict.fromkeys(range(len(order)), RF.DEFAULT)
        _set_finishes(g, plain)
        assert g.get_option(R.STAT_FINISHED_OBJECTS) == 0 and not np.array_equal(g.render_to_host(pp, O.RGB_ASCII), want)
    _reset(R, ctx)
