"""Glass on the GPU (rtx_scene_set_refraction, include/rtx.h) against tests/restate_glass.py, whose inputs
tests/test_host_restate_glass.py judges on the CPU.  Frames of 41 x 23 (the 16 x 16 tiles ragged in both directions); all eight
value floats of every pixel bit for bit (restate.same_floats), shadowed frames included: restate_glass.dark_sets restates the
kernels' exact shadow tests in fp32.
  1. every secondary kernel on scene A (restate_glass.scene_a, its floor patterned): rtx_reflect_hit at depth 1, rtx_reflect_chain
     at depths 2 and 4, rtx_grid_reflect at depths 1 and 4, the brute form -- culled, grid and brute give equal bytes; records and
     compact words of one BIT and one RGB mode are the encoders' of the values;
  2. every forward walk: one light and three, RTX_OPT_SHADOWS with RTX_OPT_REFLECT_SHADOWS (rtx_chain_shadow rebuilds the glass
     rays), the same under RTX_OPT_SHADOW_GRID (rtx_grid_shadow's walk), the patterned floor seen through glass;
  3. scene B (300 spheres, a quarter glass): the direction-sorted store on and off;
  4. neutrality: mirrors with every ior 0 give the bytes they give before any call, and again after the values are set back;
  5. inheritance: RTX_OPT_SUPERSAMPLE 2, rtx_update, a device group of two logical ranks;
  6. lifecycle: an edited radius, removal, clear, a recorded graph, both counters.
Here every object stands clear of every other; tests/test_gpu_glass_edges.py: glass that overlaps, sinks, nests and moves."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_glass as RG
import restate_pattern as RP
import restate_shadows as RH
import restate_supersample as SS
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_half as TH

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = RG.GW, RG.GH
FLOOR_TABLE = RP.SCENE_A_TABLE[:1]
FLOOR_SLOTS = {RG.A_FLOOR: 1}


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(2 * W, 2 * H)
    yield c
    c.close()


def _reset(R, c):
    TC._reset(R, c)
    for opt, v in ((R.OPT_REFLECT_SHADOWS, 0), (R.OPT_SHADOW_GRID, 0), (R.OPT_REFLECT_GRID, 0), (R.OPT_SORTED_STORE, -1), (R.OPT_SUPERSAMPLE, 1)):
        c.set_option(opt, v)
    c.scene_clear()
    c.set_patterns([])


def _set_glass(c, iors):
    items = iors.items() if isinstance(iors, dict) else [(i, float(v)) for i, v in enumerate(iors) if v]
    for i, v in items:
        c.set_refraction(int(i), float(v))


def _set_ks(c, ks):
    if isinstance(ks, dict):
        T._set_k(c, ks)
    else:
        c.set_reflectivity(0, np.asarray(ks, dtype=np.float32))


def _load(R, c, scene, glass=True):
    """A scene on the context (scene A with its floor patterned); returns (product params, trace with the pattern applied)."""
    p, sph, pl, ks, iors, pix, trace = scene
    c.set_scene(sph, pl)
    _set_ks(c, ks)
    if glass:
        _set_glass(c, iors)
    if len(sph) == len(RG.A_SPH):
        c.set_patterns([R.make_pattern(*t) for t in FLOOR_TABLE])
        c.set_object_pattern(RG.A_FLOOR, 1)
        trace = _patterned_a()
    return TC._params(p), trace


_cache = {}


def _patterned_a():
    if "a" not in _cache:
        _cache["a"] = RP.patterned(RG.scene_a()[6], FLOOR_TABLE, FLOOR_SLOTS)
    return _cache["a"]


def _lights(nl):
    return [RS.reference_light()] if nl == 0 else RG.lights_a(nl)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- 1. every secondary kernel

@pytest.mark.parametrize("depth,nl", [(1, 0), (2, 3), (4, 0)])
def test_every_secondary_kernel_equals_the_restatement(R, ctx, depth, nl):
    _reset(R, ctx)
    pp, trace = _load(R, ctx, RG.scene_a())
    lights = _lights(nl)
    if nl:
        TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    assert ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == 4
    before = ctx.get_option(R.STAT_REFRACT_FRAMES)
    got = TC._values(R, ctx, pp)
    assert ctx.get_option(R.STAT_REFRACT_FRAMES) == before + 1
    want = RS.shade_chain(trace, lights)[depth]
    TC._assert_values(got, trace, want, "depth %d" % depth)
    if depth > 1:
        assert TC._ray_stats(R, ctx)[:depth] == trace["rays"][:depth]
    # the mirrors-only frame is another one: glass is in the picture
    plain = RS.shade_chain(RP.patterned(RS.trace_chain(*RG.scene_a()[:4], RG.scene_a()[5]), FLOOR_TABLE, FLOOR_SLOTS), lights)[depth]
    assert (np.logical_or.reduce([plain[q] != want[q] for q in range(3)]) & trace["vis"]).sum() >= 100
    # brute: every sphere tested
    ctx.set_option(R.OPT_REFLECT_CHECK, 1)
    brute = TC._values(R, ctx, pp)
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)
    assert np.array_equal(_bits(brute), _bits(got)), "RTX_OPT_REFLECT_CHECK 1 changes bytes"
    # through the world grid
    if depth in (1, 4):
        grid_frames = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        grid = TC._values(R, ctx, pp)
        assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == grid_frames + 1
        assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_REFLECT_GRID 1 changes bytes"
        assert TC._ray_stats(R, ctx)[:depth] == trace["rays"][:depth]
    _reset(R, ctx)


@pytest.mark.parametrize("mode", [O.BIT_ASCII, O.RGB_PIXEL])
def test_records_and_words_encode_the_values(R, ctx, mode):
    _reset(R, ctx)
    pp, trace = _load(R, ctx, RG.scene_a())
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    far = float(pp.cam_far)
    vals = TC._values(R, ctx, pp, mode)
    TC._assert_values(vals, trace, RS.shade_chain(trace, _lights(0))[2], O.MODE_NAMES[mode])
    S = 12 if mode < O.RGB_ASCII else 20
    rec = T._rows(R, ctx, pp, mode).reshape(-1, S)
    assert np.array_equal(rec, RS.encode_records(vals, mode, far))
    words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT).view(np.uint32)
    assert np.array_equal(words, RS.encode_words(vals, mode, far))
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. every forward walk

@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("nl", [1, 3])
def test_shadows_at_every_level_on_every_pixel(R, ctx, nl, deep):
    _reset(R, ctx)
    pp, trace = _load(R, ctx, RG.scene_a())
    lights = _lights(nl)
    TC._set_lights(R, ctx, lights)
    depth = 3
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, deep)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shadow_shade<" if deep else "rtx_lights_chain_shade<"), ctx.last_kernel
    dark = RG.dark_sets(trace, lights, bool(deep))
    want = RH.shade_chain_dark(trace, lights, dark)[depth]
    TC._assert_values(got, trace, want, "%d lights, deep %d" % (nl, deep))
    lit = RS.shade_chain(trace, lights)[depth]
    assert (np.logical_or.reduce([lit[q] != want[q] for q in range(3)]) & trace["vis"]).sum() >= 50  # (shadows are in the picture)
    # the brute shadow test and the world grid's walk: the default's bytes
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = TC._values(R, ctx, pp)
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    assert np.array_equal(_bits(brute), _bits(got)), "RTX_OPT_SHADOW_CHECK 1 changes bytes"
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<" if deep else "rtx_grid_chain_shade<"), ctx.last_kernel
    assert np.array_equal(_bits(grid), _bits(got)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    if deep:  # both grids: rtx_grid_reflect's rays, rtx_grid_shadow's walk
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        both = TC._values(R, ctx, pp)
        assert np.array_equal(_bits(both), _bits(got)), "both grids change bytes"
    _reset(R, ctx)


def test_one_bounce_under_a_light_set_and_shadows(R, ctx):
    """reflect_blend's call sites: rtx_reflect_shade (one light) and rtx_lights_reflect_shade (three), level 0 shadowed."""
    for nl in (1, 3):
        _reset(R, ctx)
        pp, trace = _load(R, ctx, RG.scene_a())
        lights = _lights(nl)
        TC._set_lights(R, ctx, lights)
        ctx.set_option(R.OPT_SHADOWS, 1)
        got = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith("rtx_reflect_shade<" if nl == 1 else "rtx_lights_reflect_shade<"), ctx.last_kernel
        want = RH.shade_chain_dark(trace, lights, RG.dark_sets(trace, lights, False))[1]
        TC._assert_values(got, trace, want, "one bounce, %d lights" % nl)
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. the sorted store

def test_sorted_store_carries_the_values(R, ctx):
    _reset(R, ctx)
    scene = RG.scene_b()
    p, sph, pl, ks, iors, pix, trace = scene
    want = RS.shade_chain(trace, _lights(0))[2]
    frames = {}
    for store in (-1, 0):
        ctx.set_option(R.OPT_SORTED_STORE, store)
        pp, _ = _load(R, ctx, scene)
        ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
        assert ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == RG.B_NS // 4
        frames[store] = TC._values(R, ctx, pp)
        TC._assert_values(frames[store], trace, want, "sorted store %d" % store)
        assert TC._ray_stats(R, ctx)[:2] == trace["rays"][:2]
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        assert np.array_equal(_bits(TC._values(R, ctx, pp)), _bits(frames[store])), "RTX_OPT_REFLECT_GRID 1 changes bytes"
        ctx.set_option(R.OPT_REFLECT_GRID, 0)
    assert np.array_equal(_bits(frames[-1]), _bits(frames[0]))
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. neutrality

def _frames(R, c, pp):
    out = []
    for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES), (O.BIT_PIXEL, 0)):
        out.append((T._rows(R, c, pp, mode, flags).tobytes(), c.last_kernel))
    return out


@pytest.mark.parametrize("depth", [1, 3])
def test_every_ior_zero_is_the_frame_before_any_call(R, depth):
    p, sph, pl, ks, iors = RG.scene_a()[:5]
    pp = TC._params(p)
    with R.Context(W, H) as c:  # (a context that never saw the call)
        c.set_scene(sph, pl)
        T._set_k(c, ks)
        c.set_option(R.OPT_REFLECT_DEPTH, depth)
        fresh = _frames(R, c, pp)
        c.set_refraction(0, np.zeros(len(sph) + len(pl), dtype=np.float32))
        assert _frames(R, c, pp) == fresh
        assert c.get_option(R.STAT_REFRACT_FRAMES) == 0 and c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 0
        _set_glass(c, iors)
        assert c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 4
        glass = _frames(R, c, pp)
        assert [k for _, k in glass] == [k for _, k in fresh] and all(a[0] != b[0] for a, b in zip(glass, fresh))
        assert c.get_option(R.STAT_REFRACT_FRAMES) == 4
        # ior only matters where k > 0: the opaque sphere may carry one
        c.set_refraction(4, 2.0)
        assert c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 5
        assert [a for a, _ in _frames(R, c, pp)] == [a for a, _ in glass]
        # every value back to 0: the first frames again
        c.set_refraction(0, np.zeros(len(sph) + len(pl), dtype=np.float32))
        assert c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 0
        assert _frames(R, c, pp) == fresh
        assert c.get_option(R.STAT_REFRACT_FRAMES) == 8


# ---------------------------------------------------------------- 5. inheritance

def test_supersampling_folds_the_glass_sample_frame(R, ctx):
    _reset(R, ctx)
    S, mode = 2, O.RGB_ASCII
    p0 = RG.scene_a_params()
    p, ps = SS.case_params(O, W, H, S, tuple(p0.cam_pos[:3]), float(p0.cam_far), rot=(0.3, RS.PI32, 0.0))
    sph, pl, ks, iors = RG.scene_a()[1:5]
    ctx.set_scene(sph, pl)
    T._set_k(ctx, ks)
    _set_glass(ctx, iors)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    sample = RG.trace_chain_glass(ps, sph, pl, ks, iors, np.arange(S * W * S * H), max_depth=2)
    samples = RS.values8(sample, RS.shade_chain(sample, _lights(0))[2])
    TC._assert_values(TC._values(R, ctx, TC._params(ps), mode), sample, RS.shade_chain(sample, _lights(0))[2], "the sample frame")
    want = SS.fold(samples, W, H, S, float(p.cam_far))
    ctx.set_option(R.OPT_SUPERSAMPLE, S)
    got = T._rows(R, ctx, TC._params(p), mode, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
    assert ctx.last_kernel.startswith("rtx_resolve<%d," % S), ctx.last_kernel
    same = RS.same_floats(got, want)
    assert same.all(), "%d cells differ" % int((~same.all(axis=1)).sum())
    _reset(R, ctx)


def test_update_is_minimize_of_the_rendered_words(R, ctx):
    import torch
    _reset(R, ctx)
    mode = O.RGB_ASCII
    pp, trace = _load(R, ctx, RG.scene_a())
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
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


def test_a_device_group_gives_the_one_device_frame(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks, iors = RG.scene_a()[:5]
    pp, _ = _load(R, ctx, RG.scene_a())
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    want = ctx.render_to_host(pp, O.RGB_ASCII)
    with R.Context(W, H, devices=[0, 0]) as g:
        _load(R, g, RG.scene_a())
        g.set_option(R.OPT_REFLECT_DEPTH, 2)
        assert np.array_equal(g.render_to_host(pp, O.RGB_ASCII), want)
        with pytest.raises(R.RtxError):  # validated on the root before any rank is touched
            g.set_refraction(0, [1.5, 0.5])
        assert g.get_refraction(0) == 1.5
        assert np.array_equal(g.render_to_host(pp, O.RGB_ASCII), want)
        g.set_refraction(0, 0.0)
        ctx.set_refraction(0, 0.0)
        other = ctx.render_to_host(pp, O.RGB_ASCII)
        assert not np.array_equal(other, want) and np.array_equal(g.render_to_host(pp, O.RGB_ASCII), other)
    _reset(R, ctx)


# ---------------------------------------------------------------- 6. lifecycle

def test_an_edited_radius_changes_the_chord(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks, iors, pix, _ = RG.scene_a()
    pp, _ = _load(R, ctx, RG.scene_a())
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    edited = sph.copy()
    edited[0, 3] = 3.25
    ctx.set_spheres(0, edited[0])
    assert ctx.get_refraction(0) == 1.5 and ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == 4  # (rtx_scene_set_spheres keeps the value)
    trace = RP.patterned(RG.trace_chain_glass(p, edited, pl, ks, iors, pix, max_depth=2), FLOOR_TABLE, FLOOR_SLOTS)
    TC._assert_values(TC._values(R, ctx, pp), trace, RS.shade_chain(trace, _lights(0))[2], "the edited radius")
    _reset(R, ctx)


def test_removal_renumbers_and_clear_forgets(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks, iors, pix, _ = RG.scene_a()
    pp, _ = _load(R, ctx, RG.scene_a())
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    n = len(sph) + len(pl)
    assert [ctx.get_refraction(i) for i in range(n)] == [float(f32(iors.get(i, 0.0))) for i in range(n)]
    ctx.remove_objects([1, 4])  # a glass sphere and the opaque one: the floor becomes object 3, the sheet object 4
    keep = [0, 2, 3, 5, 6]
    assert [ctx.get_refraction(i) for i in range(5)] == [float(f32(iors.get(g, 0.0))) for g in keep]
    assert ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == 3
    ks2 = {j: ks[g] for j, g in enumerate(keep) if g in ks}
    iors2 = {j: iors[g] for j, g in enumerate(keep) if g in iors}
    trace = RP.patterned(RG.trace_chain_glass(p, sph[[0, 2, 3]], pl, ks2, iors2, pix, max_depth=2), FLOOR_TABLE, {3: 1})
    TC._assert_values(TC._values(R, ctx, pp), trace, RS.shade_chain(trace, _lights(0))[2], "after the removal")
    ctx.scene_clear()
    assert ctx.get_option(R.STAT_REFRACTIVE_OBJECTS) == 0
    ctx.set_scene(sph, pl)
    assert [ctx.get_refraction(i) for i in range(n)] == [0.0] * n
    _reset(R, ctx)


def test_a_graph_recorded_before_a_change_is_refused(R, ctx):
    import torch
    _reset(R, ctx)
    pp, _ = _load(R, ctx, RG.scene_a())
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    want = T._rows(R, ctx, pp, O.RGB_ASCII)  # (render once before capturing: the device copies are uploaded here)
    ctx.graph_begin(s.cuda_stream)
    ctx.render_rows(pp, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want)
        ctx.set_refraction(0, 2.0)
        with pytest.raises(R.RtxError) as e:
            ctx.graph_launch(g, s.cuda_stream)
        assert e.value.status == R.ERR_INVALID_ARGUMENT and "refraction" in str(e.value)
    finally:
        ctx.graph_destroy(g)
    _reset(R, ctx)
