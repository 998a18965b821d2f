"""Where several lights, shadows, mirrors and mirrors that see mirrors meet, against tests/restate.py (tied to the CPU oracle and
to float64 by tests/test_host_restate.py, which also states the conditions the inputs below meet):
  a. depths 1-4 x light sets, shadows off: all eight RTX_RENDER_VALUES floats (t, shadingValue, normal, colour) bit for bit on
     the default scene and the mirror floor (every pixel, and RTX_STAT_REFLECT_RAYS) and on samples of C2 floor+quarter and C3
     room; the reversed set matches its own restatement and is another frame;
  b. shadows on, depths 2 and 4, 1 custom, 2 and 3 lights: every pixel's colour is shade_chain's for one set of lights dark AT
     LEVEL 0 ONLY -- the deeper levels at full power whatever float64 says about their points -- and the set is the one float64
     decides where it decides every light; culled equals brute;
  c. per shade kernel, shadows off and on, the four character modes: the records and the compact words are the encoding of the
     values of the same state (restate.encode_records / encode_words), and rtx_expand of the words gives the records;
  d. twelve fuzzed scenes (tests/fuzz_cases.py::chain_case) at depth 4 against the restatement, all eight values."""

import numpy as np
import pytest

import fuzz_cases as F
import oracle as O
import restate as RS
import util as U
import test_gpu_reflect as T
from test_host_restate import shadow_sets

pytestmark = pytest.mark.gpu

MODES = T.MODES
f32 = np.float32
FIELDS = ["t", "shadingValue", "normal.x", "normal.y", "normal.z", "colour.r", "colour.g", "colour.b"]


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(3840, 2160)
    yield c
    c.close()


def _reset(R, c):
    T._reset(R, c)
    c.set_option(R.OPT_REFLECT_DEPTH, 1)
    c.set_option(R.OPT_REFLECT_DEPTH_CHECK, 0)
    c.set_option(R.OPT_LIGHTS_CHECK, 0)


def _params(p):
    return U.product_params(np.array(p.inv_v, dtype=np.float32), p.cam_pos[:], p.x, p.y, p.element1, p.element2, p.cam_far)


def _set_lights(R, c, lights):
    """One light through rtx_scene_set_light, several through rtx_scene_set_lights."""
    made = [R.make_light(*RS.light_tuple(l)) for l in lights]
    if len(made) == 1:
        c.set_light(made[0])
    else:
        c.set_lights(made)


_traces = {}


def _load(R, c, name):
    """The scene `name` of restate.chain_scene on the context, its mirrors set; the geometry traced once per module."""
    if name not in _traces:
        p, sph, pl, ks, pix = RS.chain_scene(name)
        _traces[name] = (p, sph, pl, ks, pix, RS.trace_chain(p, sph, pl, ks, pix))
    p, sph, pl, ks, pix, trace = _traces[name]
    if name in ("C2", "C3"):
        rp, rsph, rpl = R.config_inputs(name)  # (the numpy scene generator gives the library's scene, the oracle's camera the library's)
        assert np.array_equal(rsph, sph) and np.array_equal(rpl, pl) and bytes(rp) == bytes(_params(p))
    c.set_scene(sph, pl)
    T._set_k(c, ks)
    return _params(p), p, pix, trace


def _values(R, c, pp, mode=O.RGB_ASCII):
    return T._rows(R, c, pp, mode, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)


def _assert_values(got, trace, colour, what, fields=range(8)):
    """Every pixel of the trace: a hit's eight floats bit for bit, a miss's distance, column W-1 all zero."""
    want = RS.values8(trace, colour)
    same = RS.same_floats(got, want)
    vis = trace["vis"]
    for j in fields:
        bad = np.nonzero(~same[:, j] & vis)[0]
        assert bad.size == 0, "%s: %s differs at %d of %d visible pixels, e.g. pixel %d got %r want %r" % (
            what, FIELDS[j], bad.size, int(vis.sum()), int(trace["pix"][bad[0]]), got[bad[0], j], want[bad[0], j])
    last = trace["pix"] % trace["W"] == trace["W"] - 1
    assert (got[last].view(np.uint32) == 0).all(), "%s: column W-1 holds values" % what
    assert (got[~trace["hit"] & ~last, 0] == RS.NO_HIT).all(), "%s: a pixel without a hit has a distance" % what


def _ray_stats(R, c):
    return [int(c.get_option(R.STAT_REFLECT_RAYS + l)) for l in range(R.MAX_REFLECT_DEPTH)]


# ---------------------------------------------------------------- a. depths x light sets, shadows off

@pytest.mark.parametrize("which", list(RS.LIGHT_SETS))
@pytest.mark.parametrize("name", ["default", "mirror_floor", "C2", "C3"])
def test_depths_1_to_4_under_light_sets_bit_for_bit(R, ctx, name, which):
    _reset(R, ctx)
    pp, p, pix, trace = _load(R, ctx, name)
    whole = len(pix) == int(p.x) * int(p.y)
    lights = RS.chain_lights(name, which)
    frames = {}
    for order, ls in (("given", lights), ("reversed", lights[::-1])):
        if order == "reversed" and len(lights) == 1:
            continue
        _set_lights(R, ctx, ls)
        colour = RS.shade_chain(trace, ls)
        for depth in ((1, 2, 3, 4) if order == "given" else (2, 4)):
            ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
            got = _values(R, ctx, pp)[pix]
            want_kernel = "rtx_lights_chain_shade<" if depth >= 2 else ("rtx_reflect_shade<" if len(ls) == 1 else "rtx_lights_reflect_shade<")
            assert ctx.last_kernel.startswith(want_kernel), (depth, ctx.last_kernel)
            _assert_values(got, trace, colour[depth], "%s, lights %s %s, depth %d" % (name, which, order, depth))
            if whole:
                stats = _ray_stats(R, ctx)
                assert stats == ([0, 0, 0, 0] if depth == 1 else trace["rays"][:depth] + [0] * (4 - depth)), (depth, stats, trace["rays"])
            frames[(order, depth)] = got[:, 5:8].copy().view(np.uint32)
    assert (frames[("given", 2)] != frames[("given", 1)]).any() and (frames[("given", 4)] != frames[("given", 2)]).any()
    if len(lights) > 1:
        assert (frames[("reversed", 4)] != frames[("given", 4)]).any(), "the reversed set renders the same frame"
    _reset(R, ctx)


# ---------------------------------------------------------------- b. shadows: level 0 only

@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("name", ["mirror_floor_shadows", "directed"])
def test_shadows_darken_level_0_only(R, ctx, name, nl, depth):
    _reset(R, ctx)
    pp, p, pix, trace = _load(R, ctx, name)
    _, lights, dset, decided, amb = shadow_sets(name, nl)
    _set_lights(R, ctx, lights)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_SHADOWS, 1)
    got = _values(R, ctx, pp)[pix]
    assert ctx.last_kernel.startswith("rtx_lights_chain_shade<")
    assert _ray_stats(R, ctx) == trace["rays"][:depth] + [0] * (4 - depth)
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = _values(R, ctx, pp)[pix]
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    assert np.array_equal(got.view(np.uint32), brute.view(np.uint32)), "culled differs from brute"
    # distance, glyph value and normal do not depend on lights or shadows (and are what float64 judged)
    _assert_values(got, trace, [got[:, 5], got[:, 6], got[:, 7]], "%s, %d lights, depth %d" % (name, nl, depth), fields=range(5))
    vis = trace["vis"]
    match = {}
    for S in range(1 << nl):
        want = RS.shade_chain(trace, lights, dark0=S)[depth]
        match[S] = np.logical_and.reduce([RS.same_floats(got[:, 5 + q], want[q]) for q in range(3)])
    some = np.logical_or.reduce(list(match.values()))
    bad = np.nonzero(vis & ~some)[0]
    assert bad.size == 0, "%d visible pixels show no set of lights dark at level 0 only, e.g. pixel %d: %r" % (bad.size, int(pix[bad[0]]), got[bad[0], 5:8])
    right = np.zeros(len(pix), dtype=bool)
    for S, m in match.items():
        right |= m & (dset == S)
    wrong = np.nonzero(vis & decided & ~right)[0]
    assert wrong.size == 0, "%d of %d decided pixels are not shaded with the set float64 decides, e.g. pixel %d (set %d): %r" % (
        wrong.size, int((vis & decided).sum()), int(pix[wrong[0]]), int(dset[wrong[0]]), got[wrong[0], 5:8])
    l2 = trace["levels"][2]["exists"]
    print("%s, %d lights, depth %d: %d visible, %d decided, %d with a dark light, %d of those with a level-2 ray" % (
        name, nl, depth, int(vis.sum()), int((vis & decided).sum()), int((vis & decided & (dset != 0)).sum()), int((vis & decided & (dset != 0) & l2).sum())))
    _reset(R, ctx)


# ---------------------------------------------------------------- c. records and words are the encoding of the values

KERNEL_STATES = {"rtx_shadow_shade": (False, 1, 1), "rtx_lights_shade": (False, 3, 1), "rtx_reflect_shade": (True, 1, 1),
                 "rtx_lights_reflect_shade": (True, 3, 1), "rtx_lights_chain_shade": (True, 3, 3)}  # (mirrors, lights, depth)


@pytest.mark.parametrize("kernel", list(KERNEL_STATES))
@pytest.mark.parametrize("name", ["C1", "C2"])
def test_records_and_words_encode_the_values(R, ctx, name, kernel):
    import torch
    _reset(R, ctx)
    mirrors, nl, depth = KERNEL_STATES[kernel]
    pp, sph, pl = R.config_inputs(name)
    W, H = int(pp.x), int(pp.y)
    ctx.set_scene(sph, pl)
    if mirrors:
        T._set_k(ctx, RS._scene_k(name, sph, pl, "quarter" if name == "C1" else "floor+quarter"))
    _set_lights(R, ctx, RS.record_lights(nl))
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    frames = []
    for shadows in (0, 1):
        ctx.set_option(R.OPT_SHADOWS, shadows)
        for mode in MODES:
            S = 12 if mode < O.RGB_ASCII else 20
            what = "%s %s shadows %d %s" % (name, kernel, shadows, O.MODE_NAMES[mode])
            vals = _values(R, ctx, pp, mode)
            assert ctx.last_kernel.startswith(kernel + "<"), ctx.last_kernel
            rec = T._rows(R, ctx, pp, mode)
            assert ctx.last_kernel.startswith(kernel + "<"), ctx.last_kernel
            words = T._rows(R, ctx, pp, mode, R.RENDER_COMPACT)
            assert ctx.last_kernel.startswith(kernel + "<"), ctx.last_kernel
            want = RS.encode_records(vals, mode, pp.cam_far).reshape(-1)
            assert np.array_equal(rec, want), "%s: the records are not the encoding of the values: %s" % (what, U.first_diff(rec, want, S, W))
            want_words = RS.encode_words(vals, mode, pp.cam_far)
            got_words = words.view(np.uint32)
            bad = np.nonzero(got_words != want_words)[0]
            assert bad.size == 0, "%s: %d words are not the encoding of the values, e.g. pixel %d: %08x, want %08x" % (
                what, bad.size, int(bad[0]), int(got_words[bad[0]]), int(want_words[bad[0]]))
            d_words = torch.from_numpy(words).cuda()
            d_rec = torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.expand(mode, d_words.data_ptr(), d_rec.data_ptr(), [(0, 0, W * H)])
            ctx.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(d_rec.cpu().numpy(), rec), "%s: rtx_expand of the words gives other records" % what
            if mode == O.RGB_ASCII:
                frames.append(rec)
                visible = int((vals[:, 0] <= f32(pp.cam_far)).sum() - (vals.view(np.uint32) == 0).all(axis=1).sum())
                assert visible > 0.15 * W * H, visible
    assert not np.array_equal(frames[0], frames[1]), "shadows change no record"
    _reset(R, ctx)


# ---------------------------------------------------------------- d. fuzzed scenes against the restatement

@pytest.mark.parametrize("seed", RS.FUZZ_SEEDS)
def test_fuzzed_chains_equal_the_restatement(R, ctx, seed):
    import torch
    _reset(R, ctx)
    stats = {}
    found = F.chain_case(R, torch, ctx, seed, stats=stats)
    print("seed %d: %r" % (seed, stats))
    assert found == [], "\n".join(found)
    _reset(R, ctx)
