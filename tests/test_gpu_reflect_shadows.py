"""Shadows seen in mirrors (RTX_OPT_REFLECT_SHADOWS, include/rtx.h) against tests/restate_shadows.py, whose inputs
tests/test_host_reflect_shadows.py judges on the CPU:
  1. float64 decides: every visible pixel's colour is shade_chain_dark's for some assignment of dark sets to the levels, and the
     assignment float64 decides wherever it decides every level; distance, shadingValue and normal are the trace's; the new shade
     family is launched; RTX_STAT_REFLECT_SHADOW_POINTS counts the trace's hits per level; culled equals brute;
  2. culled = brute where the occluder list fills up (C2's 1024 spheres) and refills with a partial last step (1700 spheres);
  3. under RTX_OPT_SHADOW_CHECK 2 nothing is dark: option 1 gives option 0's bytes in values, records and words;
  4. option 0 is the context's state before the option was ever set, byte for byte and launch for launch; option 1 changes some
     colour; without shadows, or without a reflective object, it changes nothing;
  5. the new family's records and words are the encoding of its values in the four character modes, rtx_expand included;
  6. a 37 x 21 frame, ragged slabs, three logical ranks, a recorded graph;
  7. the option's arguments."""

import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_shadows as RH
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC

pytestmark = pytest.mark.gpu

f32 = np.float32
FAMILY = "rtx_lights_chain_shadow_shade<"


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


def _load(R, c, name):
    p, sph, pl, ks, pix, trace = RH.traced(name)
    c.set_scene(sph, pl)
    T._set_k(c, ks)
    return TC._params(p), trace


def _points_stats(R, c):
    return [int(c.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(R.MAX_REFLECT_DEPTH)]


def _trace_points(trace, depth):
    return [int((trace["levels"][j]["gid"] >= 0).sum()) if j <= min(depth, trace["max_depth"]) else 0 for j in range(1, 5)]


def _check_against_float64(got, trace, lights, lev, depth, what):
    """Test 1's comparison of a frame's values with the restatement and float64's per-level sets."""
    nl = len(lights)
    TC._assert_values(got, trace, [got[:, 5], got[:, 6], got[:, 7]], what, fields=range(5))
    vis = trace["vis"]
    some = np.zeros(trace["n"], dtype=bool)
    right = np.zeros(trace["n"], dtype=bool)
    for combo in RH.combinations(nl, depth):
        want = RH.shade_chain_dark(trace, lights, list(combo) + [0] * (4 - depth))[depth]
        m = np.logical_and.reduce([RS.same_floats(got[:, 5 + q], want[q]) for q in range(3)])
        some |= m
        right |= m & np.logical_and.reduce([lev[j]["dset"] == combo[j] for j in range(depth + 1)])
    bad = np.nonzero(vis & ~some)[0]
    assert bad.size == 0, "%s: %d visible pixels show no assignment of dark sets to the levels, e.g. pixel %d: %r" % (
        what, bad.size, int(trace["pix"][bad[0]]), got[bad[0], 5:8])
    decided = np.logical_and.reduce([l["decided"] for l in lev])
    wrong = np.nonzero(vis & decided & ~right)[0]
    assert wrong.size == 0, "%s: %d of %d decided pixels are not shaded with the sets float64 decides, e.g. pixel %d (sets %r): %r" % (
        what, wrong.size, int((vis & decided).sum()), int(trace["pix"][wrong[0]]), [int(l["dset"][wrong[0]]) for l in lev], got[wrong[0], 5:8])
    deep_dark = np.logical_or.reduce([l["dset"] != 0 for l in lev[1:]])
    print("%s: %d visible, %d decided at every level, %d of those dark at some deeper level" % (
        what, int(vis.sum()), int((vis & decided).sum()), int((vis & decided & deep_dark).sum())))


# ---------------------------------------------------------------- 1. float64 decides (and culled = brute on the same frames)

@pytest.mark.parametrize("nl,depth", RH.CASES)
@pytest.mark.parametrize("name", RH.SCENES)
def test_float64_decides_every_level(R, ctx, name, nl, depth):
    _reset(R, ctx)
    pp, trace = _load(R, ctx, name)
    _, lights, lev = RH.sets(name, nl, depth)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    got = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith(FAMILY), ctx.last_kernel
    assert _points_stats(R, ctx) == _trace_points(trace, depth), (_points_stats(R, ctx), _trace_points(trace, depth))
    assert TC._ray_stats(R, ctx) == trace["rays"][:depth] + [0] * (4 - depth)
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = TC._values(R, ctx, pp)
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    assert np.array_equal(got.view(np.uint32), brute.view(np.uint32)), "culled differs from brute"
    _check_against_float64(got, trace, lights, lev, depth, "%s, %d lights, depth %d" % (name, nl, depth))
    # the option shows: the frame without it is another one
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 0)
    off = TC._values(R, ctx, pp)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shade<" if depth > 1 else ("rtx_reflect_shade<" if nl == 1 else "rtx_lights_reflect_shade<"))
    assert _points_stats(R, ctx) == [0, 0, 0, 0]
    assert (off.view(np.uint32) != got.view(np.uint32)).any()
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. culled = brute on long lists

@pytest.mark.parametrize("case", ["C2", "1700"])
def test_culled_equals_brute_when_the_list_fills(R, ctx, case):
    """C2's scene, floor + quarter reflective, 160 x 90, depth 2: under RTX_OPT_SHADOW_CHECK 1 every workgroup lists all 1024
    spheres, the whole LDS list, in one filling (512, then 1024 at the last step).  1700 spheres over a floor -- three full
    steps and a partial one of 164 -- make it refill: cnt = 1024 > CAP - kChunk after the second step flushes, the last step
    flushes the other 676, and a longest list of 1700 > CAP entries can only be the sum over more than one filling."""
    _reset(R, ctx)
    p = R.camera_params(160, 90)
    if case == "C2":
        _, sph, pl = R.config_inputs("C2")
        ks = RS._scene_k("C2", sph, pl, "floor+quarter")
    else:
        sph, pl = U.numpy_synth_scene(77, 1700, 1, p.element1, p.element2)
        ks = RS._scene_k("x", sph, pl, "floor+quarter")
    trace = RS.trace_chain(p, sph, pl, ks, np.arange(160 * 90), max_depth=2)
    want_pts = _trace_points(trace, 2)
    assert want_pts[0] > 1000 and want_pts[1] > 100, want_pts
    # float64: spheres do occlude level-1 points that face the first light, so some tile's list cannot be empty
    idx, P1, N1, owner1 = RH.level_points(trace, 1)
    k1 = RH.classify64_points(P1, N1, owner1, trace["sph"], trace["pl"], RS.record_lights(3)[0].pos)
    faces = np.einsum("nk,nk->n", N1.astype(np.float64), np.array(RS.record_lights(3)[0].pos) - P1.astype(np.float64)) > 0
    assert ((k1 == 1) & faces).sum() >= 100 and (k1 == 0).sum() >= 100, (int(((k1 == 1) & faces).sum()), int((k1 == 0).sum()))
    ctx.set_scene(sph, pl)
    T._set_k(ctx, ks)
    TC._set_lights(R, ctx, RS.record_lights(3))
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    frames = {}
    for check in (0, 1):
        ctx.set_option(R.OPT_SHADOW_CHECK, check)
        frames[check] = [TC._values(R, ctx, p), T._rows(R, ctx, p, O.BIT_ASCII)]
        assert ctx.last_kernel.startswith(FAMILY)
        longest = ctx.get_option(R.STAT_SHADOW_LONGEST_LIST)
        pts = _points_stats(R, ctx)
        print(case, "check", check, "longest list", longest, "points", pts)
        assert (longest == len(sph)) if check else (0 < longest <= len(sph))
        assert case == "C2" or len(sph) > 1024 + 512  # (more than one filling of the 1024-entry list, and a partial last step)
        assert pts == want_pts, (pts, want_pts)
    for a, b in zip(frames[0], frames[1]):
        assert np.array_equal(a, b), "culled differs from brute"
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 0)
    assert (TC._values(R, ctx, p).view(np.uint32) != frames[0][0].view(np.uint32)).any(), "the option changes no colour"
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. nothing dark = option off

def test_no_test_gives_the_bytes_of_option_off(R, ctx):
    _reset(R, ctx)
    pp, trace = _load(R, ctx, "mirror_floor_shadows")
    TC._set_lights(R, ctx, RH.lights("mirror_floor_shadows", 2))
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_SHADOW_CHECK, 2)
    out = {}
    for opt in (0, 1):
        ctx.set_option(R.OPT_REFLECT_SHADOWS, opt)
        frames = []
        for mode in (O.RGB_ASCII, O.BIT_PIXEL):
            for flags in (R.RENDER_VALUES, 0, R.RENDER_COMPACT):
                frames.append(T._rows(R, ctx, pp, mode, flags))
                assert ctx.last_kernel.startswith(FAMILY if opt else "rtx_lights_chain_shade<"), ctx.last_kernel
        out[opt] = frames
        if opt:
            assert _points_stats(R, ctx) == [0, 0, 0, 0]  # (no point is tested)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    # and every pixel is lit: the colour of no dark set at any level
    want = RH.shade_chain_dark(trace, RH.lights("mirror_floor_shadows", 2), [0, 0, 0, 0, 0])[2]
    TC._assert_values(out[1][0].view(np.float32).reshape(-1, 8), trace, want, "no test")
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. option 0 is today

@pytest.mark.parametrize("nl", [1, 3])
@pytest.mark.parametrize("depth", [1, 2])
def test_option_0_is_the_state_before_the_option_existed(R, depth, nl):
    p, sph, pl, ks, pix, trace = RH.traced("mirror_floor_shadows")
    pp = TC._params(p)
    with R.Context(320, 180) as c:  # (a context the option was never set on)
        c.set_scene(sph, pl)
        T._set_k(c, ks)
        TC._set_lights(R, c, RH.lights("mirror_floor_shadows", nl))
        c.set_option(R.OPT_REFLECT_DEPTH, depth)

        def frames():
            out = []
            for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES)):
                out.append((T._rows(R, c, pp, mode, flags).tobytes(), c.last_kernel))
            return out

        c.set_option(R.OPT_SHADOWS, 1)
        before = frames()
        assert not any(k.startswith(FAMILY) for _, k in before)
        assert c.get_option(R.OPT_REFLECT_SHADOWS) == 0
        c.set_option(R.OPT_REFLECT_SHADOWS, 0)
        assert frames() == before
        c.set_option(R.OPT_REFLECT_SHADOWS, 1)
        on = frames()
        assert all(k.startswith(FAMILY) for _, k in on), [k for _, k in on]
        assert all(a[0] != b[0] for a, b in zip(on, before)), "option 1 changes no colour"
        c.set_option(R.OPT_REFLECT_SHADOWS, 0)
        assert frames() == before
        # shadows off: the option has no effect
        c.set_option(R.OPT_SHADOWS, 0)
        off = frames()
        c.set_option(R.OPT_REFLECT_SHADOWS, 1)
        assert frames() == off
        assert [int(c.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(4)] == [0, 0, 0, 0]
        # no reflective object: no effect either
        c.set_option(R.OPT_SHADOWS, 1)
        T._clear_k(c, len(sph) + len(pl))
        with_opt = frames()
        assert [int(c.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(4)] == [0, 0, 0, 0]  # (not the counts of the frames before)
        c.set_option(R.OPT_REFLECT_SHADOWS, 0)
        assert frames() == with_opt
        assert not any("chain" in k or "reflect" in k for _, k in with_opt), [k for _, k in with_opt]


# ---------------------------------------------------------------- 5. records and words are the encoding of the values

def test_records_and_words_encode_the_values(R, ctx):
    import torch
    _reset(R, ctx)
    pp, sph, pl = R.config_inputs("C1")
    W, H = int(pp.x), int(pp.y)
    ctx.set_scene(sph, pl)
    T._set_k(ctx, RS._scene_k("C1", sph, pl, "quarter"))
    TC._set_lights(R, ctx, RS.record_lights(3))
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    ctx.set_option(R.OPT_SHADOWS, 1)
    frames = {}
    for opt in (1, 0):
        ctx.set_option(R.OPT_REFLECT_SHADOWS, opt)
        frames[opt] = T._rows(R, ctx, pp, O.RGB_ASCII)
    assert not np.array_equal(frames[0], frames[1]), "the option changes no record"
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    for mode in T.MODES:
        S = 12 if mode < O.RGB_ASCII else 20
        what = "C1 %s" % O.MODE_NAMES[mode]
        vals = TC._values(R, ctx, pp, mode)
        assert ctx.last_kernel.startswith(FAMILY) and ctx.last_kernel.endswith(",values>"), ctx.last_kernel
        rec = T._rows(R, ctx, pp, mode)
        assert ctx.last_kernel.startswith(FAMILY), ctx.last_kernel
        words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT)
        assert ctx.last_kernel.startswith(FAMILY) and ctx.last_kernel.endswith(",compact>"), ctx.last_kernel
        want = RS.encode_records(vals, mode, pp.cam_far).reshape(-1)
        assert np.array_equal(rec, want), "%s: the records are not the encoding of the values: %s" % (what, U.first_diff(rec, want, S, W))
        want_words = RS.encode_words(vals, mode, pp.cam_far)
        bad = np.nonzero(words.view(np.uint32) != want_words)[0]
        assert bad.size == 0, "%s: %d words are not the encoding of the values, e.g. pixel %d" % (what, bad.size, int(bad[0]))
        d_words = torch.from_numpy(words).cuda()
        d_rec = torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.expand(mode, d_words.data_ptr(), d_rec.data_ptr(), [(0, 0, W * H)])
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(d_rec.cpu().numpy(), rec), "%s: rtx_expand of the words gives other records" % what
    _reset(R, ctx)


# ---------------------------------------------------------------- 6. shapes

def test_a_frame_that_is_no_multiple_of_the_tile(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks, pix = RH.scene("wall", 37, 21)
    trace = RS.trace_chain(p, sph, pl, ks, pix)
    lights = RH.lights("wall", 2)
    lev = RH.level_sets(trace, lights, 2)
    assert lev[1]["tested"].sum() >= 20 and (lev[1]["dset"] != 0).sum() >= 5
    ctx.set_scene(sph, pl)
    T._set_k(ctx, ks)
    TC._set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    got = TC._values(R, ctx, TC._params(p))
    assert ctx.last_kernel.startswith(FAMILY)
    assert _points_stats(R, ctx) == _trace_points(trace, 2)
    _check_against_float64(got, trace, lights, lev, 2, "wall 37 x 21")
    _reset(R, ctx)


@pytest.fixture()
def floor_on(R, ctx):
    _reset(R, ctx)
    pp, trace = _load(R, ctx, "mirror_floor_shadows")
    TC._set_lights(R, ctx, RH.lights("mirror_floor_shadows", 3))
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    ctx.set_option(R.OPT_SHADOWS, 1)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    yield pp, trace
    _reset(R, ctx)


def test_two_ragged_slabs_equal_the_frame(R, ctx, floor_on):
    import torch
    pp, trace = floor_on
    W, H = int(pp.x), int(pp.y)
    for mode, flags, S in ((O.RGB_ASCII, 0, 20), (O.BIT_PIXEL, R.RENDER_COMPACT, 4)):
        whole = T._rows(R, ctx, pp, mode, flags)
        parts = []
        for r0, r1 in ((0, 70), (70, 180)):
            buf = torch.full(((r1 - r0) * W * S,), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.render_rows(pp, mode, r0, r1 - r0, d_out=buf.data_ptr(), out_row_base=r0, flags=flags)
            ctx.synchronize()
            assert ctx.last_kernel.startswith(FAMILY)
            parts.append(buf.cpu().numpy())
        assert np.array_equal(np.concatenate(parts), whole)
    # (the counters are the last launch set's: the second slab's points)
    pts = _points_stats(R, ctx)
    assert 0 < pts[0] < _trace_points(trace, 3)[0], pts


def test_three_logical_ranks_equal_one_device(R):
    p, sph, pl, ks, pix, trace = RH.traced("mirror_floor_shadows")
    pp = TC._params(p)
    outs = []
    for devices in (None, [0, 0, 0]):
        c = R.Context(int(p.x), int(p.y), devices=devices)
        try:
            c.set_scene(sph, pl)
            T._set_k(c, ks)
            TC._set_lights(R, c, RH.lights("mirror_floor_shadows", 2))
            c.set_option(R.OPT_REFLECT_DEPTH, 2)
            c.set_option(R.OPT_SHADOWS, 1)
            off = c.render_to_host(pp, O.RGB_ASCII).copy()
            c.set_option(R.OPT_REFLECT_SHADOWS, 1)
            assert c.get_option(R.OPT_REFLECT_SHADOWS) == 1
            with pytest.raises(R.RtxError):
                c.set_option(R.OPT_REFLECT_SHADOWS, 2)
            assert c.get_option(R.OPT_REFLECT_SHADOWS) == 1
            on = [c.render_to_host(pp, m).copy() for m in (O.BIT_ASCII, O.RGB_ASCII)]
            assert not np.array_equal(on[1], off), "the option changes no byte"
            outs.append(on)
        finally:
            c.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_a_recorded_graph_keeps_the_option(R, ctx, floor_on):
    import torch
    pp, trace = floor_on
    W, H = int(pp.x), int(pp.y)
    want_on = T._rows(R, ctx, pp, O.RGB_ASCII)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(s.cuda_stream)
    ctx.render_rows(pp, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want_on)
        ctx.set_option(R.OPT_REFLECT_SHADOWS, 0)
        want_off = T._rows(R, ctx, pp, O.RGB_ASCII)
        assert not np.array_equal(want_off, want_on)
        buf.zero_()
        torch.cuda.synchronize()
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want_on), "the replay follows the context's option"
    finally:
        ctx.graph_destroy(g)


# ---------------------------------------------------------------- 7. arguments

def test_option_arguments(R, ctx):
    _reset(R, ctx)
    assert ctx.get_option(R.OPT_REFLECT_SHADOWS) == 0
    for start in (0, 1):
        ctx.set_option(R.OPT_REFLECT_SHADOWS, start)
        for bad in (2, -1):
            with pytest.raises(R.RtxError) as e:
                ctx.set_option(R.OPT_REFLECT_SHADOWS, bad)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            assert ctx.get_option(R.OPT_REFLECT_SHADOWS) == start
    with pytest.raises(R.RtxError):
        ctx.set_option(R.STAT_REFLECT_SHADOW_POINTS, 0)  # (a counter is read-only)
    _reset(R, ctx)
