"""Checker patterns on the GPU (rtx_scene_set_patterns, include/rtx.h) against tests/restate_pattern.py, whose inputs
tests/test_host_restate_pattern.py judges on the CPU.  Frames of 320 x 180; all eight value floats bit for bit (restate.same_floats).
  2. no mirrors, the reference's light, shadows off: rtx_shadow_shade, counted by RTX_STAT_PATTERN_FRAMES; records and words of the
     four character modes are the encoding of the values;
  3. every family: one bounce, light sets of 2 and 8 with and without mirrors, the chain at depths 2 and 4; RTX_OPT_REFLECT_GRID 1
     gives the same bytes;
  4. shadows: the pixels float64 decides under 1 and 3 lights, RTX_OPT_SHADOWS alone and with RTX_OPT_REFLECT_SHADOWS at depth 2;
     RTX_OPT_SHADOW_CHECK 1 and RTX_OPT_SHADOW_GRID 1 give the default's bytes;
  5. the direction-sorted store: 300 spheres, every third patterned, RTX_OPT_SORTED_STORE -1 and 0;
  6. neutrality: a table without a slot is a fresh context, byte for byte and kernel for kernel; a pattern of the object's own
     colour is the unpatterned frame;
  7. lifecycle: removal, edits in place, a shrinking table, a recorded graph, a device group, rtx_update and rtx_update_half.
(Scene A, case 1 of the list, is restate_pattern.scene_a.)"""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_pattern as RP
import restate_shadows as RH
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_half as TH

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 320, 180


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
    for opt, v in ((R.OPT_REFLECT_SHADOWS, 0), (R.OPT_SHADOW_GRID, 0), (R.OPT_REFLECT_GRID, 0), (R.OPT_SORTED_STORE, -1)):
        c.set_option(opt, v)
    c.scene_clear()      # (forgets the slots, so that the table may go)
    c.set_patterns([])


def _set_patterns(R, c, table, slots):
    c.set_patterns([R.make_pattern(*t) for t in table])
    items = slots.items() if isinstance(slots, dict) else [(i, int(s)) for i, s in enumerate(slots) if s]
    for i, s in items:
        c.set_object_pattern(int(i), int(s))


def _load_a(R, c, mirrors=True, ks=None):
    """Scene A on the context; returns (product params, ks)."""
    p, sph, pl, ks_a, pix, trace, pat = RP.scene_a()
    c.set_scene(sph, pl)
    ks = ks_a if ks is None else ks
    if mirrors:
        T._set_k(c, ks)
    _set_patterns(R, c, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS)
    return TC._params(p)


_traces = {}


def _flat():
    """Scene A without mirrors: (trace, patterned trace)."""
    if "flat" not in _traces:
        p, sph, pl, ks, pix = RP.scene_a()[:5]
        t = RS.trace_chain(p, sph, pl, {}, pix, max_depth=1)
        _traces["flat"] = (t, RP.patterned(t, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS))
    return _traces["flat"]


def _shadow_traces():
    """mirror_floor_shadows (scene A's geometry, the floor at k = 0.6): (trace, patterned trace)."""
    if "shadows" not in _traces:
        t = RH.traced("mirror_floor_shadows")[5]
        _traces["shadows"] = (t, RP.patterned(t, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS))
    return _traces["shadows"]


_level_sets = {}


def _sets(nl):
    if nl not in _level_sets:
        lights = RH.lights("mirror_floor_shadows", nl)
        _level_sets[nl] = (lights, RH.level_sets(_shadow_traces()[0], lights, 2))
    return _level_sets[nl]


def _assert_decided(got, pat, want, decided, what):
    """The eight floats of the visible pixels float64 decides."""
    full = RS.values8(pat, want)
    same = RS.same_floats(got, full)
    sel = pat["vis"] & decided
    for j in range(8):
        bad = np.nonzero(~same[:, j] & sel)[0]
        assert bad.size == 0, "%s: %s differs at %d of %d decided pixels, e.g. pixel %d got %r want %r" % (
            what, TC.FIELDS[j], bad.size, int(sel.sum()), int(pat["pix"][bad[0]]), got[bad[0], j], full[bad[0], j])


# ---------------------------------------------------------------- 2. no mirrors

def test_no_mirrors_values_records_and_words(R, ctx):
    _reset(R, ctx)
    pp = _load_a(R, ctx, mirrors=False)
    trace, pat = _flat()
    assert ctx.get_option(R.STAT_PATTERNED_OBJECTS) == 3
    before = ctx.get_option(R.STAT_PATTERN_FRAMES)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_shadow_shade<"), ctx.last_kernel
    assert ctx.get_option(R.STAT_PATTERN_FRAMES) == before + 1
    want = RS.shade_chain(pat, [RS.reference_light()])[1]
    TC._assert_values(got, pat, want, "no mirrors")
    plain = RS.shade_chain(trace, [RS.reference_light()])[1]
    assert (np.logical_or.reduce([plain[q] != want[q] for q in range(3)]) & trace["vis"]).sum() > 10000  # (the pattern shows)
    far = float(pp.cam_far)
    for mode in T.MODES:
        S = 12 if mode < O.RGB_ASCII else 20
        vals = TC._values(R, ctx, pp, mode)
        TC._assert_values(vals, pat, want, O.MODE_NAMES[mode])
        rec = T._rows(R, ctx, pp, mode).reshape(-1, S)
        assert ctx.last_kernel.startswith("rtx_shadow_shade<"), ctx.last_kernel
        assert np.array_equal(rec, RS.encode_records(vals, mode, far)), O.MODE_NAMES[mode]
        words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT).view(np.uint32)
        assert np.array_equal(words, RS.encode_words(vals, mode, far)), O.MODE_NAMES[mode]
    assert ctx.get_option(R.STAT_PATTERN_FRAMES) == before + 1 + 3 * len(T.MODES)
    # RGB_NORMALS is unaffected: the bytes and the launch of the scene without slots
    normals = T._rows(R, ctx, pp, O.RGB_NORMALS)
    kernel = ctx.last_kernel
    frames = ctx.get_option(R.STAT_PATTERN_FRAMES)
    ctx.set_object_pattern(0, 0, n=5)
    assert ctx.get_option(R.STAT_PATTERNED_OBJECTS) == 0
    assert np.array_equal(T._rows(R, ctx, pp, O.RGB_NORMALS), normals) and ctx.last_kernel == kernel
    assert ctx.get_option(R.STAT_PATTERN_FRAMES) == frames
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. every family

FAMILIES = {  # name -> (mirrors, light set or None for the reference's light, depth, kernel)
    "reflect": (True, None, 1, "rtx_reflect_shade<"),
    "lights2_flat": (False, "2", 1, "rtx_lights_shade<"),
    "lights8_flat": (False, "8", 1, "rtx_lights_shade<"),
    "lights2_reflect": (True, "2", 1, "rtx_lights_reflect_shade<"),
    "lights8_reflect": (True, "8", 1, "rtx_lights_reflect_shade<"),
    "chain2": (True, "2", 2, "rtx_lights_chain_shade<"),
    "chain4": (True, None, 4, "rtx_lights_chain_shade<"),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_every_family_equals_the_restatement(R, ctx, name):
    mirrors, which, depth, kernel = FAMILIES[name]
    _reset(R, ctx)
    pp = _load_a(R, ctx, mirrors=mirrors)
    lights = [RS.reference_light()] if which is None else RS.chain_lights("mirror_floor", which)
    if which is not None:
        TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    pat = RP.scene_a()[6] if mirrors else _flat()[1]
    before = ctx.get_option(R.STAT_PATTERN_FRAMES)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
    assert ctx.get_option(R.STAT_PATTERN_FRAMES) == before + 1
    want = RS.shade_chain(pat, lights)[depth if mirrors else 1]
    TC._assert_values(got, pat, want, name)
    if mirrors:
        assert TC._ray_stats(R, ctx)[:depth] == pat["rays"][:depth] if depth > 1 else True
        grid_frames = ctx.get_option(R.STAT_REFLECT_GRID_FRAMES)
        ctx.set_option(R.OPT_REFLECT_GRID, 1)
        on = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
        assert ctx.get_option(R.STAT_REFLECT_GRID_FRAMES) == grid_frames + 1
        assert np.array_equal(on.view(np.uint32), got.view(np.uint32)), "RTX_OPT_REFLECT_GRID changes bytes"
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. shadows

@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("nl", [1, 3])
def test_shadows_on_the_pixels_float64_decides(R, ctx, nl, deep):
    _reset(R, ctx)
    trace, pat = _shadow_traces()
    ks = RH.traced("mirror_floor_shadows")[3]
    pp = _load_a(R, ctx, ks=ks)
    lights, lev = _sets(nl)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, deep)
    kernel = "rtx_lights_chain_shadow_shade<" if deep else "rtx_lights_chain_shade<"
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
    levels = lev[:3] if deep else lev[:1]
    decided = np.logical_and.reduce([l["decided"] for l in levels])
    undecided = int((pat["vis"] & ~decided).sum())
    print("%d lights, deep %d: %d visible, %d undecided" % (nl, deep, int(pat["vis"].sum()), undecided))
    assert undecided <= 0.001 * nl * pat["n"]
    dark = [l["dset"] for l in levels] + [0] * (5 - len(levels))
    want = RH.shade_chain_dark(pat, lights, dark)[2]
    _assert_decided(got, pat, want, decided, "%d lights, deep %d" % (nl, deep))
    some_dark = np.logical_or.reduce([l["dset"] != 0 for l in levels])
    assert (pat["vis"] & decided & some_dark).sum() > 500  # (shadows are in the picture)
    # the brute reference and the world grid: the default's bytes
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith(kernel), ctx.last_kernel
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    assert np.array_equal(brute.view(np.uint32), got.view(np.uint32)), "RTX_OPT_SHADOW_CHECK 1 changes bytes"
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<" if deep else "rtx_grid_chain_shade<"), ctx.last_kernel
    assert np.array_equal(grid.view(np.uint32), got.view(np.uint32)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    _reset(R, ctx)


@pytest.mark.parametrize("mirrors", [False, True])
def test_shadows_at_depth_1_and_the_grid_families(R, ctx, mirrors):
    """rtx_lights_shade / rtx_lights_reflect_shade with shadows, and rtx_grid_shade / rtx_grid_reflect_shade beside them."""
    _reset(R, ctx)
    ks = RH.traced("mirror_floor_shadows")[3]
    pp = _load_a(R, ctx, mirrors=mirrors, ks=ks)
    pat = _shadow_traces()[1] if mirrors else _flat()[1]
    lights, lev = _sets(3)  # (level 0's points and sets do not depend on k)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_SHADOWS, 1)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_reflect_shade<" if mirrors else "rtx_lights_shade<"), ctx.last_kernel
    want = RH.shade_chain_dark(pat, lights, [lev[0]["dset"], 0, 0, 0, 0])[1]
    _assert_decided(got, pat, want, lev[0]["decided"], "depth 1, mirrors %d" % mirrors)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    grid = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_grid_reflect_shade<" if mirrors else "rtx_grid_shade<"), ctx.last_kernel
    assert np.array_equal(grid.view(np.uint32), got.view(np.uint32)), "RTX_OPT_SHADOW_GRID 1 changes bytes"
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. the sorted store

def test_sorted_store_carries_the_slots(R, ctx):
    _reset(R, ctx)
    p, sph, pl, slots, trace, pat = RP.sorted_scene()
    pp = TC._params(p)
    want = RS.shade_chain(pat, [RS.reference_light()])[1]
    plain = RS.shade_chain(trace, [RS.reference_light()])[1]
    assert (np.logical_or.reduce([plain[q] != want[q] for q in range(3)]) & trace["vis"]).sum() > 1000
    frames = {}
    for store in (-1, 0):
        ctx.set_option(R.OPT_SORTED_STORE, store)
        ctx.set_scene(sph, pl)
        _set_patterns(R, ctx, RP.SCENE_A_TABLE, slots)
        assert ctx.get_option(R.STAT_PATTERNED_OBJECTS) == 100
        frames[store] = TC._values(R, ctx, pp)
        assert ctx.last_kernel.startswith("rtx_shadow_shade<"), ctx.last_kernel
        TC._assert_values(frames[store], pat, want, "sorted store %d" % store)
    assert np.array_equal(frames[-1].view(np.uint32), frames[0].view(np.uint32))
    _reset(R, ctx)


# ---------------------------------------------------------------- 6. neutrality

def _frames(R, c, pp):
    out = []
    for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES), (O.BIT_PIXEL, 0)):
        out.append((T._rows(R, c, pp, mode, flags).tobytes(), c.last_kernel))
    return out


@pytest.mark.parametrize("mirrors", [False, True])
def test_a_table_without_a_slot_is_a_fresh_context(R, mirrors):
    p, sph, pl, ks = RP.scene_a()[:4]
    pp = TC._params(p)
    with R.Context(W, H) as c:  # (a context that never saw a pattern)
        c.set_scene(sph, pl)
        if mirrors:
            T._set_k(c, ks)
        fresh = _frames(R, c, pp)
        assert not any("_shade<" in k for _, k in fresh) or mirrors  # (no mirrors: the direct path, one trace launch)
        c.set_patterns([R.make_pattern(*t) for t in RP.SCENE_A_TABLE])
        assert len(c.get_patterns()) == 2
        assert _frames(R, c, pp) == fresh
        assert c.get_option(R.STAT_PATTERN_FRAMES) == 0 and c.get_option(R.STAT_PATTERNED_OBJECTS) == 0
        # a slot given and taken back: the same again
        c.set_object_pattern(4, 1)
        assert _frames(R, c, pp) != fresh
        assert c.get_option(R.STAT_PATTERN_FRAMES) == 4
        c.set_object_pattern(4, 0)
        assert _frames(R, c, pp) == fresh
        assert c.get_option(R.STAT_PATTERN_FRAMES) == 4


def test_a_pattern_of_the_objects_own_colour_changes_nothing(R, ctx):
    _reset(R, ctx)
    p, sph, pl = RP.scene_a()[:3]
    pp = TC._params(p)
    ctx.set_scene(sph, pl)
    ctx.set_option(R.OPT_LIGHTS_CHECK, 1)
    plain = _frames(R, ctx, pp)
    assert all(k.startswith("rtx_lights_shade<") for _, k in plain), [k for _, k in plain]
    floor, ball = RP.SCENE_A_TABLE[0], RP.SCENE_A_TABLE[1]
    ctx.set_patterns([R.make_pattern(floor.origin, floor.freq, tuple(pl[0, 6:9])), R.make_pattern(ball.origin, ball.freq, tuple(sph[1, 4:7]))])
    ctx.set_object_pattern(4, 1)
    ctx.set_object_pattern(1, 2)
    before = ctx.get_option(R.STAT_PATTERN_FRAMES)
    assert _frames(R, ctx, pp) == plain
    assert ctx.get_option(R.STAT_PATTERN_FRAMES) == before + 4
    _reset(R, ctx)


# ---------------------------------------------------------------- 7. lifecycle

def _built(R, sph, pl, ks, table, slots):
    c = R.Context(W, H)
    c.set_scene(sph, pl)
    T._set_k(c, ks)
    _set_patterns(R, c, table, slots)
    return c


def test_removal_keeps_the_survivors_slots(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks = RP.scene_a()[:4]
    pp = _load_a(R, ctx)
    ctx.remove_objects([0])  # a sphere below the patterned ones
    assert [ctx.get_object_pattern(i) for i in range(4)] == [2, 0, 2, 1]
    assert ctx.get_option(R.STAT_PATTERNED_OBJECTS) == 3
    got = _frames(R, ctx, pp)
    with _built(R, sph[1:], pl, {i - 1: k for i, k in ks.items() if i > 0}, RP.SCENE_A_TABLE, {0: 2, 2: 2, 3: 1}) as fresh:
        want = _frames(R, fresh, pp)
    assert got == want
    assert all(k.startswith("rtx_reflect_shade<") for _, k in got)
    _reset(R, ctx)


def test_edits_in_place_keep_the_slot_and_a_shrinking_table_is_refused(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks = RP.scene_a()[:4]
    pp = _load_a(R, ctx)
    moved = sph.copy()
    moved[1, :4] = (1.0, 6.0, 34.0, 4.5)
    ctx.set_spheres(1, moved[1])
    ctx.set_plane(4, tuple(pl[0, 0:3]), tuple(pl[0, 3:6]), (90.0, 120.0, 150.0), float(pl[0, 9]), float(pl[0, 10]))
    assert ctx.get_object_pattern(1) == 2 and ctx.get_object_pattern(4) == 1
    got = _frames(R, ctx, pp)
    pl2 = pl.copy()
    pl2[0, 6:9] = (90.0, 120.0, 150.0)
    with _built(R, moved, pl2, ks, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS) as fresh:
        assert got == _frames(R, fresh, pp)
    # the table may not shrink under an assigned slot: nothing changes
    for bad in ([R.make_pattern(*RP.SCENE_A_TABLE[0])], []):
        with pytest.raises(R.RtxError) as e:
            ctx.set_patterns(bad)
        assert e.value.status == R.ERR_INVALID_ARGUMENT and "object 1" in str(e.value), str(e.value)
    nan = R.make_pattern((0.0, float("nan"), 0.0), (1.0, 1.0, 1.0), (1.0, 2.0, 3.0))
    for bad in ([R.make_pattern(), nan], [R.make_pattern()] * (R.MAX_PATTERNS + 1)):
        with pytest.raises(R.RtxError) as e:
            ctx.set_patterns(bad)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
    for first, n, slot in ((0, 1, 3), (4, 2, 1), (6, 0, 0)):
        with pytest.raises(R.RtxError) as e:
            ctx.set_object_pattern(first, slot, n=n)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
    tab = ctx.get_patterns()
    assert len(tab) == 2 and tuple(tab[0].freq) == (0.25, 0.0, 0.25) and tuple(tab[1].rgb) == (250.0, 250.0, 250.0)
    assert [ctx.get_object_pattern(i) for i in range(5)] == [0, 2, 0, 2, 1]
    assert _frames(R, ctx, pp) == got
    # rtx_scene_clear forgets the slots and leaves the table
    ctx.scene_clear()
    assert ctx.get_option(R.STAT_PATTERNED_OBJECTS) == 0 and len(ctx.get_patterns()) == 2
    ctx.set_scene(sph, pl)
    assert [ctx.get_object_pattern(i) for i in range(5)] == [0] * 5
    _reset(R, ctx)


def test_a_graph_recorded_before_a_slot_change_is_refused(R, ctx):
    import torch
    _reset(R, ctx)
    pp = _load_a(R, ctx)
    want = T._rows(R, ctx, pp, O.RGB_ASCII)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(s.cuda_stream)
    ctx.render_rows(pp, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want)
        ctx.set_object_pattern(3, 0)
        with pytest.raises(R.RtxError) as e:
            ctx.graph_launch(g, s.cuda_stream)
        assert e.value.status == R.ERR_INVALID_ARGUMENT and "pattern" in str(e.value)
    finally:
        ctx.graph_destroy(g)
    _reset(R, ctx)


def test_a_device_group_gives_the_one_device_frame(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks = RP.scene_a()[:4]
    pp = _load_a(R, ctx)
    want = ctx.render_to_host(pp, O.RGB_ASCII)
    assert ctx.last_kernel.startswith("rtx_reflect_shade<")
    with R.Context(W, H, devices=[0, 0, 0]) as g:
        g.set_scene(sph, pl)
        T._set_k(g, ks)
        _set_patterns(R, g, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS)
        assert np.array_equal(g.render_to_host(pp, O.RGB_ASCII), want)
        with pytest.raises(R.RtxError):  # validated on the root before any rank is touched
            g.set_patterns([])
        assert np.array_equal(g.render_to_host(pp, O.RGB_ASCII), want)
        g.set_object_pattern(4, 0)
        ctx.set_object_pattern(4, 0)
        assert np.array_equal(g.render_to_host(pp, O.RGB_ASCII), ctx.render_to_host(pp, O.RGB_ASCII))
    _reset(R, ctx)


@pytest.mark.parametrize("mode", [O.RGB_ASCII, O.BIT_PIXEL])
def test_update_and_update_half_are_the_passes_over_the_words(R, mode):
    import torch
    p, sph, pl, ks = RP.scene_a()[:4]
    pp = TC._params(p)
    with R.Context(W, H) as c:
        c.set_scene(sph, pl)
        _set_patterns(R, c, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS)
        # the words are the encoding of the values test 2 compares with the restatement
        vals = TC._values(R, c, pp, mode)
        words = T._rows(R, c, pp, mode, R.RENDER_COMPACT).view(np.uint32)
        assert np.array_equal(words, RS.encode_words(vals, mode, float(pp.cam_far)))
        # rtx_update: Minimize over those words
        tw = TH.to_device(words)
        out = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = c.minimize_words(mode, W, H, tw.data_ptr(), out.data_ptr())
        c.synchronize()
        before = c.get_option(R.STAT_PATTERN_FRAMES)
        assert bytes(c.update(pp, mode)) == bytes(out.cpu().numpy()[:n]) and n > 0
        assert c.get_option(R.STAT_PATTERN_FRAMES) > before
        # rtx_update_half: the console of half the rows, whose sample frame is this frame
        console = R.Params.from_buffer_copy(bytes(pp))
        console.y = H // 2
        assert bytes(TH.sample_params(R, console)) == bytes(pp)
        assert bytes(c.update_half(console, mode)) == TH.run_half(R, c, mode, W, H // 2, words)
