"""Per-object surface finishes on the GPU (rtx_scene_set_finish, include/rtx.h) against tests/restate_finish.py, whose inputs
tests/test_host_restate_finish.py judges on the CPU.  Scene F (restate.chain_scene("mirror_floor") with restate_finish.F_FINISHES) at
320 x 180 through RTX_RENDER_VALUES: all eight floats of every pixel bit for bit (restate.same_floats), shadowed frames included --
restate_glass.dark_sets restates the kernels' exact shadow tests in fp32.
  1. depths 1 and 4 x the light sets `1custom` and `8`: the one-bounce kernels (rtx_reflect_shade, rtx_lights_reflect_shade) and the
     chain kernel at both depths; without mirrors rtx_shadow_shade and rtx_lights_shade, shadows off and on;
  2. one light and RTX_OPT_SHADOWS on the shadow twin of the scene, then RTX_OPT_REFLECT_SHADOWS at depth 3; RTX_OPT_SHADOW_GRID and
     RTX_OPT_REFLECT_GRID on give the bytes they give off (the four grid families);
  3. scene A's first pattern on the floor; sphere 1 as glass, ior 1.5;
  4. records and compact words of one case are the encoders' of the restated values;
  5. a finished object alone makes a direct frame a shaded one, the default set back makes it direct again with the bytes of a
     context that never had a finish; RGB_NORMALS bytes do not depend on finishes; both counters."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_finish as RF
import restate_glass as RG
import restate_pattern as RP
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 320, 180
F = RF.F_FINISHES
FLOOR = 4


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(W, H)
    yield c
    c.close()


def _reset(R, c):
    TC._reset(R, c)
    for opt, v in ((R.OPT_REFLECT_SHADOWS, 0), (R.OPT_SHADOW_GRID, 0), (R.OPT_REFLECT_GRID, 0), (R.OPT_SORTED_STORE, -1), (R.OPT_SUPERSAMPLE, 1)):
        c.set_option(opt, v)
    c.scene_clear()
    c.set_patterns([])


def _set_finishes(c, finishes):
    for i, f in finishes.items():
        c.set_finish(int(i), [f])


def _load(R, c, name="mirror_floor", mirrors=True):
    """Scene F (or its shadow twin) on the context; returns (product params, spheres, planes, ks, pixels)."""
    p, sph, pl, ks, pix = RF.scene_f(name)[:5]
    c.set_scene(sph, pl)
    if mirrors:
        T._set_k(c, ks)
    _set_finishes(c, F)
    assert c.get_option(R.STAT_FINISHED_OBJECTS) == len(F)
    return TC._params(p), sph, pl, ks, pix


_plain = {}


def _trace_without_mirrors():
    if "t" not in _plain:
        p, sph, pl, _, pix = RF.scene_f()[:5]
        _plain["t"] = RS.trace_chain(p, sph, pl, {}, pix, max_depth=1)
    return _plain["t"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _differ(a, b, mask):
    return int((np.logical_or.reduce([a[q] != b[q] for q in range(3)]) & mask).sum())


# ---------------------------------------------------------------- 1. every tile family, shadows off (and on without mirrors)

@pytest.mark.parametrize("which", ["1custom", "8"])
def test_mirror_kernels_at_depths_1_and_4(R, ctx, which):
    _reset(R, ctx)
    pp = _load(R, ctx)[0]
    trace = RF.scene_f()[5]
    lights = RS.chain_lights("mirror_floor", which)
    TC._set_lights(R, ctx, lights)
    want = RF.shade_chain_finish(trace, lights, F)
    plain = RS.shade_chain(trace, lights)
    one_bounce = "rtx_reflect_shade<" if len(lights) == 1 else "rtx_lights_reflect_shade<"
    frames0 = ctx.get_option(R.STAT_FINISH_FRAMES)
    for depth, check, kernel in ((1, 0, one_bounce), (1, 1, "rtx_lights_chain_shade<"), (4, 0, "rtx_lights_chain_shade<")):
        ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
        ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, check)
        got = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
        TC._assert_values(got, trace, want[depth], "%s, depth %d on %s" % (which, depth, kernel))
        assert _differ(want[depth], plain[depth], trace["vis"]) >= 1000  # (the finishes are in the picture)
    assert ctx.get_option(R.STAT_FINISH_FRAMES) == frames0 + 3
    _reset(R, ctx)


@pytest.mark.parametrize("shadows", [0, 1])
@pytest.mark.parametrize("which", ["1custom", "8"])
def test_the_kernels_without_mirrors(R, ctx, which, shadows):
    _reset(R, ctx)
    pp = _load(R, ctx, mirrors=False)[0]
    trace = _trace_without_mirrors()
    lights = RS.chain_lights("mirror_floor", which)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_SHADOWS, shadows)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_shadow_shade<" if len(lights) == 1 else "rtx_lights_shade<"), ctx.last_kernel
    dark0 = RG.dark_sets(trace, lights, False)[0] if shadows else 0
    want = RF.shade_plain_finish(trace, lights, F, dark0)
    TC._assert_values(got, trace, want, "%s, shadows %d" % (which, shadows))
    if shadows:
        assert _differ(want, RF.shade_plain_finish(trace, lights, F), trace["vis"]) >= 100  # (shadows are in the picture)
        ctx.set_option(R.OPT_SHADOW_GRID, 1)
        grid = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith("rtx_grid_shade<"), ctx.last_kernel
        assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. shadows at level 0, at every level, and through the grids

def test_one_light_and_shadows_on_the_shadow_twin(R, ctx):
    _reset(R, ctx)
    pp = _load(R, ctx, "mirror_floor_shadows")[0]
    trace = RF.scene_f("mirror_floor_shadows")[5]
    lights = RS.shadow_lights("mirror_floor_shadows", 1)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_SHADOWS, 1)
    dark = RG.dark_sets(trace, lights, False)
    for depth, kernel, grid_kernel in ((1, "rtx_reflect_shade<", "rtx_grid_reflect_shade<"), (2, "rtx_lights_chain_shade<", "rtx_grid_chain_shade<")):
        ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
        got = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
        want = RF.shade_chain_finish(trace, lights, F, dark0=dark[0])[depth]
        TC._assert_values(got, trace, want, "one light, shadows, depth %d" % depth)
        assert _differ(want, RF.shade_chain_finish(trace, lights, F)[depth], trace["vis"]) >= 100  # (shadows are in the picture)
        ctx.set_option(R.OPT_SHADOW_GRID, 1)
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        grid = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(grid_kernel), ctx.last_kernel
        assert np.array_equal(_bits(grid), _bits(got)), "the grid options change bytes at depth %d" % depth
        ctx.set_option(R.OPT_SHADOW_GRID, 0)
        ctx.set_option(R.OPT_REFLECT_GRID, 0)
    _reset(R, ctx)


@pytest.mark.parametrize("nl", [1, 3])
def test_shadows_seen_in_mirrors(R, ctx, nl):
    _reset(R, ctx)
    pp = _load(R, ctx, "mirror_floor_shadows")[0]
    trace = RF.scene_f("mirror_floor_shadows")[5]
    lights = RS.shadow_lights("mirror_floor_shadows", nl)
    TC._set_lights(R, ctx, lights)
    depth = 3
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shadow_shade<"), ctx.last_kernel
    dark = RG.dark_sets(trace, lights, True)
    want = RF.shade_chain_finish(trace, lights, F, dark0=dark[0], deep_dark=dark[1:])[depth]
    TC._assert_values(got, trace, want, "%d lights, shadows at every level" % nl)
    level0_only = RF.shade_chain_finish(trace, lights, F, dark0=dark[0])[depth]
    assert _differ(want, level0_only, trace["vis"]) >= 50  # (deeper shadows are in the picture)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<"), ctx.last_kernel
    assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    ctx.set_option(R.OPT_REFLECT_GRID, 1)
    both = TC._values(R, ctx, pp)
    assert np.array_equal(_bits(both), _bits(got)), "both grids change bytes"
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. beside patterns and glass

def test_a_patterned_floor_keeps_its_finish(R, ctx):
    _reset(R, ctx)
    pp = _load(R, ctx)[0]
    table = RP.SCENE_A_TABLE[:1]
    ctx.set_patterns([R.make_pattern(*t) for t in table])
    ctx.set_object_pattern(FLOOR, 1)
    trace = RP.patterned(RF.scene_f()[5], table, {FLOOR: 1})
    lights = RS.chain_lights("mirror_floor", "8")
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    want = RF.shade_chain_finish(trace, lights, F)[2]
    TC._assert_values(TC._values(R, ctx, pp), trace, want, "patterned floor")
    # (the pattern is in the picture: the same bound as the conditions of tests/test_host_restate_finish.py, on the restatement alone)
    assert _differ(want, RF.shade_chain_finish(RF.scene_f()[5], lights, F)[2], trace["vis"]) >= 100
    _reset(R, ctx)


def test_a_glass_sphere_among_the_finishes(R, ctx):
    _reset(R, ctx)
    pp, sph, pl, ks, pix = _load(R, ctx)
    ctx.set_refraction(1, 1.5)
    trace = RG.trace_chain_glass(RF.scene_f()[0], sph, pl, ks, {1: 1.5}, pix, max_depth=2)
    lights = RS.chain_lights("mirror_floor", "1custom")
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    want = RF.shade_chain_finish(trace, lights, F)[2]
    TC._assert_values(TC._values(R, ctx, pp), trace, want, "glass")
    assert _differ(want, RF.shade_chain_finish(RF.scene_f()[5], lights, F)[2], trace["vis"]) >= 100  # (the glass is in the picture)
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. records and words

@pytest.mark.parametrize("mode", [O.BIT_ASCII, O.RGB_PIXEL])
def test_records_and_words_encode_the_values(R, ctx, mode):
    _reset(R, ctx)
    pp = _load(R, ctx)[0]
    trace = RF.scene_f()[5]
    lights = RS.chain_lights("mirror_floor", "1custom")
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    far = float(pp.cam_far)
    want = RS.values8(trace, RF.shade_chain_finish(trace, lights, F)[2])
    TC._assert_values(TC._values(R, ctx, pp, mode), trace, RF.shade_chain_finish(trace, lights, F)[2], O.MODE_NAMES[mode])
    S = 12 if mode < O.RGB_ASCII else 20
    rec = T._rows(R, ctx, pp, mode).reshape(-1, S)
    assert np.array_equal(rec, RS.encode_records(want, mode, far))
    words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT).view(np.uint32)
    assert np.array_equal(words, RS.encode_words(want, mode, far))
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. the launches, the modes that do not shade, the counters

def _frames(R, c, pp):
    out = []
    for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES), (O.BIT_PIXEL, 0)):
        out.append((T._rows(R, c, pp, mode, flags).tobytes(), c.last_kernel))
    return out


def test_a_finish_alone_takes_the_shade_launch_and_the_default_gives_it_back(R):
    p, sph, pl = RF.scene_f()[:3]
    pp = TC._params(p)
    trace = _trace_without_mirrors()
    with R.Context(W, H) as c:  # (a context that never saw the call)
        c.set_scene(sph, pl)
        fresh = _frames(R, c, pp)
        normals = T._rows(R, c, pp, O.RGB_NORMALS).tobytes()
        direct = c.last_kernel
        assert all("shade" not in k for _, k in fresh) and c.get_option(R.STAT_FINISH_FRAMES) == 0
        # the default finish, set explicitly: nothing changes
        c.set_finish(0, [RF.DEFAULT] * 5)
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 0 and _frames(R, c, pp) == fresh
        # one finished object: the closest-hit launch and rtx_shadow_shade, with the restated values
        c.set_finish(3, [F[3]])
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 1
        got = TC._values(R, c, pp)
        assert c.last_kernel.startswith("rtx_shadow_shade<"), c.last_kernel
        TC._assert_values(got, trace, RF.shade_plain_finish(trace, [RS.reference_light()], {3: F[3]}), "one finished object")
        shaded = _frames(R, c, pp)
        assert all(k.startswith("rtx_shadow_shade<") for _, k in shaded) and all(a[0] != b[0] for a, b in zip(shaded, fresh))
        assert c.get_option(R.STAT_FINISH_FRAMES) == 5
        # RGB_NORMALS does not shade: its launch and its bytes stay
        assert T._rows(R, c, pp, O.RGB_NORMALS).tobytes() == normals and c.last_kernel == direct
        assert c.get_option(R.STAT_FINISH_FRAMES) == 5
        # the default set back: the direct launch again, the first bytes again
        c.set_finish(3, [RF.DEFAULT])
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 0
        assert _frames(R, c, pp) == fresh
        assert c.get_option(R.STAT_FINISH_FRAMES) == 5


def test_the_counters_follow_sets_removal_and_clear(R, ctx):
    _reset(R, ctx)
    pp, sph, pl, ks, pix = _load(R, ctx)
    n = len(sph) + len(pl)
    assert ctx.get_option(R.STAT_FINISHED_OBJECTS) == 4
    ctx.set_finish(2, [(0.2, 1.0, 1.0, 6)])
    assert ctx.get_option(R.STAT_FINISHED_OBJECTS) == 5
    ctx.set_finish(2, [RF.DEFAULT])
    ctx.set_finish(0, [RF.DEFAULT])
    assert ctx.get_option(R.STAT_FINISHED_OBJECTS) == 3
    ctx.set_spheres(1, sph[1] + np.array([0, 1, 0, 0, 0, 0, 0], dtype=np.float32))  # (rtx_scene_set_spheres keeps the finish)
    got = ctx.get_finish(1)
    assert (got.ambient, got.diffuse, got.specular, got.shininess_log2) == tuple(f32(v) for v in F[1][:3]) + (7,)
    ctx.remove_objects([1])  # the survivors keep theirs under the renumbering: 3 -> 2, the floor 4 -> 3
    assert ctx.get_option(R.STAT_FINISHED_OBJECTS) == 2
    kept = [ctx.get_finish(i) for i in range(n - 1)]
    assert [(k.ambient, k.diffuse, k.specular, k.shininess_log2) for k in kept] == [
        tuple(f32(v) for v in f[:3]) + (f[3],) for f in (RF.DEFAULT, RF.DEFAULT, F[3], F[4])]
    frames = ctx.get_option(R.STAT_FINISH_FRAMES)
    TC._values(R, ctx, pp)
    assert ctx.get_option(R.STAT_FINISH_FRAMES) == frames + 1
    ctx.scene_clear()
    assert ctx.get_option(R.STAT_FINISHED_OBJECTS) == 0
    ctx.set_scene(sph, pl)
    d = ctx.get_finish(4)
    assert (d.ambient, d.diffuse, d.specular, d.shininess_log2) == (f32(0.2), 1.0, 1.0, 5)
    TC._values(R, ctx, pp)
    assert ctx.get_option(R.STAT_FINISH_FRAMES) == frames + 1
    _reset(R, ctx)
