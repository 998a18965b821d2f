"""RTX_OPT_SUPERSAMPLE on the GPU (include/rtx.h): a supersampled frame is the fold of the S W x S H frame the existing launches give
in values form.  That frame is rendered with S = 1, folded in numpy exactly as the rule words it (tests/restate_supersample.py) and
encoded (restate.encode_records / encode_words); the supersampled launch must give those values bit for bit, those records and
those words, and write nothing else.  The input condition of the 37 x 19 case (every kind of cell is there) is
tests/test_host_supersample.py's."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_delta as RD
import restate_supersample as SS
import util as U

pytestmark = pytest.mark.gpu

W, H, CAM, FAR = 37, 19, (0.0, 5.0, -10.0), 33.0
MODES = [O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS]
GUARD = 256  # bytes in front of and behind every output buffer that must stay as they were filled


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    with R.Context(4 * W, 4 * H) as c:
        c.set_reference_default_scene()
        yield c


def _prm(p):
    return U.product_params(np.array(p.inv_v, dtype=np.float32), p.cam_pos[:], p.x, p.y, p.element1, p.element2, p.cam_far)


def _cell_bytes(R, mode, flags):
    if flags & R.RENDER_VALUES:
        return 32
    if flags & R.RENDER_COMPACT:
        return 4
    return 20 if mode >= O.RGB_ASCII else 12


def _rows(R, c, p, mode, flags=0, row0=0, rows=None, stream=None):
    """Rows [row0, row0 + rows) of frame `p` into a caller buffer with out_row_base = row0; the bytes, after checking that the guard
    bytes around them are untouched."""
    import torch
    w = int(p.x)
    rows = int(p.y) - row0 if rows is None else rows
    n = rows * w * _cell_bytes(R, mode, flags)
    buf = torch.full((n + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.render_rows(p, mode, row0, rows, d_out=buf.data_ptr() + GUARD, out_row_base=row0, stream=stream, flags=flags)
    c.synchronize()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == 0xEE).all() and (out[GUARD + n:] == 0xEE).all(), "bytes outside the frame were written"
    return out[GUARD:GUARD + n].copy()


_expected = {}


def _expect(R, c, key, p, S, mode):
    """(values, records, words) the supersampled frame `p` must be: the S = 1 values of p' folded and encoded.  Once per key."""
    if key not in _expected:
        assert c.get_option(R.OPT_SUPERSAMPLE) == 1
        ps = SS.sample_params(p, S)
        samples = _rows(R, c, ps, mode, R.RENDER_VALUES).view(np.float32)
        assert not c.last_kernel.startswith("rtx_resolve")
        exp = SS.expected(samples, int(p.x), int(p.y), S, mode, float(p.cam_far))
        for a in exp:
            a.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def _check_frame(R, c, p, S, mode, want, row0=0, rows=None):
    """The three output forms of rows [row0, row0 + rows) of the supersampled frame against `want` (the whole frame's)."""
    w = int(p.x)
    rows = int(p.y) - row0 if rows is None else rows
    lo, hi = row0 * w, (row0 + rows) * w
    v, rec, words = want
    got = _rows(R, c, p, mode, R.RENDER_VALUES, row0, rows).view(np.float32).reshape(-1, 8)
    assert c.last_kernel.startswith("rtx_resolve<%d," % S) and c.last_kernel.endswith(",values>"), c.last_kernel
    same = RS.same_floats(got, v[lo:hi])
    assert same.all(), "values: %d cells differ, first %d: got %r want %r" % (
        (~same.all(axis=1)).sum(), np.flatnonzero(~same.all(axis=1))[0], got[~same.all(axis=1)][0], v[lo:hi][~same.all(axis=1)][0])
    got = _rows(R, c, p, mode, 0, row0, rows)
    assert np.array_equal(got, rec[lo:hi].reshape(-1)), U.first_diff(got, rec[lo:hi].reshape(-1), rec.shape[1], w)
    got = _rows(R, c, p, mode, R.RENDER_COMPACT, row0, rows).view(np.uint32)
    assert c.last_kernel.endswith(",compact>") and np.array_equal(got, words[lo:hi])


# ---- 1. the fold

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [2, 3, 4])
def test_fold(R, ctx, S, mode):
    p = _prm(SS.case_params(O, W, H, S, CAM, FAR)[0])
    ctx.set_option(R.OPT_SUPERSAMPLE, 1)
    want = _expect(R, ctx, ("fold", S, mode), p, S, mode)
    v = want[0].reshape(H, W, 8)
    assert (v[:, :W - 1, 0] <= np.float32(FAR)).any() and (v[:, :W - 1, 0] == SS.NO_HIT).any()
    before = ctx.get_option(R.STAT_SUPERSAMPLE_FRAMES)
    ctx.set_option(R.OPT_SUPERSAMPLE, S)
    try:
        _check_frame(R, ctx, p, S, mode, want)
        assert ctx.get_option(R.STAT_SUPERSAMPLE_FRAMES) == before + 3
    finally:
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)


# ---- 2. off means off

def test_default_path_is_untouched(R):
    """A context whose option was never set: the oracle's bytes from today's kernel."""
    with R.Context(W, H) as c:
        c.set_reference_default_scene()
        p = _prm(SS.case_params(O, W, H, 2, CAM, FAR)[0])
        for mode in (O.RGB_ASCII, O.BIT_ASCII):
            got = c.render_to_host(p, mode)
            assert np.array_equal(got, O.render(U.oracle_params(p), O.Scene.reference_default(), mode))
            assert c.last_kernel.startswith("rtx_trace<"), c.last_kernel


def test_one_is_off_and_other_values_are_refused(R):
    with R.Context(W, H) as c:
        c.set_reference_default_scene()
        p = _prm(SS.case_params(O, W, H, 2, CAM, FAR)[0])
        assert c.get_option(R.OPT_SUPERSAMPLE) == 1
        never = [(_rows(R, c, p, m, f).tobytes(), c.last_kernel) for m in MODES for f in (0, R.RENDER_COMPACT, R.RENDER_VALUES)]
        own = c.render_to_host(p, O.BIT_ASCII).tobytes()
        c.set_option(R.OPT_SUPERSAMPLE, 1)
        assert never == [(_rows(R, c, p, m, f).tobytes(), c.last_kernel) for m in MODES for f in (0, R.RENDER_COMPACT, R.RENDER_VALUES)]
        assert own == c.render_to_host(p, O.BIT_ASCII).tobytes()
        assert c.get_option(R.STAT_SUPERSAMPLE_FRAMES) == 0
        c.set_option(R.OPT_SUPERSAMPLE, 3)
        for bad in (0, 5, -1):
            with pytest.raises(R.RtxError) as e:
                c.set_option(R.OPT_SUPERSAMPLE, bad)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and c.get_option(R.OPT_SUPERSAMPLE) == 3
        # RTX_SDL writes nothing, supersampled or not
        c.render(p, R.SDL)
        c.synchronize()
        assert c.get_option(R.STAT_SUPERSAMPLE_FRAMES) == 0 and not c.last_kernel.startswith("rtx_resolve")
        c.set_option(R.OPT_SUPERSAMPLE, 1)
        assert never[0] == (_rows(R, c, p, MODES[0], 0).tobytes(), c.last_kernel)


# ---- 3. shapes

@pytest.mark.parametrize("w,h,S", [(1, 2, 2), (1, 1, 4), (2, 1, 2), (2, 1, 3), (259, 3, 2), (259, 3, 3)])
def test_shapes(R, ctx, w, h, S):
    """The newline column alone, one cell, a row longer than a workgroup."""
    p = _prm(SS.case_params(O, w, h, S, CAM, FAR)[0])
    mode = O.RGB_ASCII
    ctx.set_option(R.OPT_SUPERSAMPLE, 1)
    want = _expect(R, ctx, ("shape", w, h, S), p, S, mode)
    if w > 2:
        d = want[0].reshape(h, w, 8)[:, :w - 1, 0]
        assert (d <= np.float32(FAR)).any() and (d == SS.NO_HIT).any()
    ctx.set_option(R.OPT_SUPERSAMPLE, S)
    try:
        _check_frame(R, ctx, p, S, mode, want)
    finally:
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)


@pytest.mark.parametrize("S", [2, 3])
def test_ragged_slabs_and_the_contexts_buffer(R, ctx, S):
    mode = O.RGB_ASCII
    p = _prm(SS.case_params(O, W, H, S, CAM, FAR)[0])
    ctx.set_option(R.OPT_SUPERSAMPLE, 1)
    want = _expect(R, ctx, ("fold", S, mode), p, S, mode)
    ctx.set_option(R.OPT_SUPERSAMPLE, S)
    try:
        for row0, rows in ((0, 7), (7, 1), (8, 11)):
            _check_frame(R, ctx, p, S, mode, want, row0, rows)
        # rtx_render into the context's own buffer: the caller-buffer form's records, in both record sizes (the 8-bit frame's tail zero)
        for m in (O.RGB_ASCII, O.BIT_ASCII):
            ctx.set_option(R.OPT_SUPERSAMPLE, 1)
            rec = _expect(R, ctx, ("fold", S, m), p, S, m)[1]
            ctx.set_option(R.OPT_SUPERSAMPLE, S)
            got = ctx.render_to_host(p, m)
            assert ctx.last_kernel.startswith("rtx_resolve<%d," % S)
            assert np.array_equal(got[:rec.size], rec.reshape(-1)) and not got[rec.size:].any()
    finally:
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)


# ---- 4. through the shading paths

PATHS = {  # name -> (scene of restate.chain_scene, lights, mirrors, options, the family that shades the sample frame)
    "shadows": ("directed", 1, False, {"OPT_SHADOWS": 1}, "rtx_shadow_shade<"),
    "two_lights_shadows": ("directed", 2, False, {"OPT_SHADOWS": 1}, "rtx_lights_shade<"),
    "one_bounce": ("mirror_floor_shadows", 1, True, {}, "rtx_reflect_shade<"),
    "depth3_reflect_shadows": ("mirror_floor_shadows", 2, True, {"OPT_SHADOWS": 1, "OPT_REFLECT_DEPTH": 3, "OPT_REFLECT_SHADOWS": 1},
                               "rtx_lights_chain_shadow_shade<"),
    "shadow_grid": ("directed", 1, False, {"OPT_SHADOWS": 1, "OPT_SHADOW_GRID": 1}, "rtx_grid_shade<"),
}


@pytest.mark.parametrize("name", sorted(PATHS))
def test_through_the_shading_paths(R, name):
    scene, nl, mirrors, options, family = PATHS[name]
    S, w, h, mode = 2, 24, 10, O.RGB_ASCII
    p0, sph, pl, ks, _ = RS.chain_scene(scene)
    ps = U.product_params(np.array(p0.inv_v, dtype=np.float32), p0.cam_pos[:], S * w, S * h, p0.element1, p0.element2, p0.cam_far)
    p = U.product_params(np.array(p0.inv_v, dtype=np.float32), p0.cam_pos[:], w, h, p0.element1, p0.element2, p0.cam_far)
    with R.Context(S * w, S * h) as c:
        c.set_scene(sph, pl)
        if mirrors:
            for g, k in ks.items():
                c.set_reflectivity(g, k)
        made = [R.make_light(*RS.light_tuple(l)) for l in RS.shadow_lights(scene, nl)]
        if nl == 1:
            c.set_light(made[0])
        else:
            c.set_lights(made)
        for opt, val in options.items():
            c.set_option(getattr(R, opt), val)
        samples = _rows(R, c, ps, mode, R.RENDER_VALUES).view(np.float32)
        assert c.last_kernel.startswith(family), c.last_kernel
        want = SS.expected(samples, w, h, S, mode, float(p.cam_far))
        d = want[0].reshape(h, w, 8)[:, :w - 1]
        assert (d[..., 0] <= np.float32(p.cam_far)).sum() >= 20 and len(np.unique(d[..., 5:].reshape(-1, 3), axis=0)) >= 20
        frames = c.get_option(R.STAT_SHADOW_FRAMES) + c.get_option(R.STAT_REFLECT_FRAMES)
        c.set_option(R.OPT_SUPERSAMPLE, S)
        _check_frame(R, c, p, S, mode, want)
        assert c.get_option(R.STAT_SHADOW_FRAMES) + c.get_option(R.STAT_REFLECT_FRAMES) == frames + 3
        assert c.get_option(R.STAT_SUPERSAMPLE_FRAMES) == 3


# ---- 5. update

def _frame20(rec, w, h):
    frame = np.zeros(20 * w * h, dtype=np.uint8)
    frame[:rec.size] = rec.reshape(-1)
    return frame


@pytest.mark.parametrize("mode", [O.RGB_ASCII, O.BIT_ASCII])
def test_update_hands_over_the_folded_frame(R, ctx, mode):
    S = 2
    p = _prm(SS.case_params(O, W, H, S, CAM, FAR)[0])
    ctx.set_option(R.OPT_SUPERSAMPLE, 1)
    rec = _expect(R, ctx, ("fold", S, mode), p, S, mode)[1]
    ctx.set_option(R.OPT_SUPERSAMPLE, S)
    try:
        got = ctx.update(p, mode).copy()
        assert np.array_equal(got, O.minimize(mode, _frame20(rec, W, H), W, H))
    finally:
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)


def _grid(rec, w, h):
    return [[bytes(rec[r * w + c]) for c in range(w - 1)] for r in range(h)]


def test_update_delta_diffs_folded_cells(R):
    """A key frame, a physics step, a diff: replayed over the first frame's records it gives the second frame's."""
    S, mode, dt = 2, O.RGB_ASCII, 0.125
    p = _prm(SS.case_params(O, W, H, S, CAM, FAR)[0])
    with R.Context(S * W, S * H) as c, R.Context(S * W, S * H) as twin:
        for x in (c, twin):
            x.set_reference_default_scene()
            for i in range(5):
                x.set_sphere_motion(i, 1 if i % 2 else -1, 3.0)
        first = SS.expected(_rows(R, twin, SS.sample_params(p, S), mode, R.RENDER_VALUES).view(np.float32), W, H, S, mode, FAR)[1]
        twin.update_objects(dt)
        second = SS.expected(_rows(R, twin, SS.sample_params(p, S), mode, R.RENDER_VALUES).view(np.float32), W, H, S, mode, FAR)[1]
        assert not np.array_equal(first, second)
        c.set_option(R.OPT_SUPERSAMPLE, S)
        s, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_KEY and np.array_equal(s, O.minimize(mode, _frame20(first, W, H), W, H))
        s, kind = c.update_delta(p, mode, dt=dt, run_physics=True)
        assert kind == R.DELTA_DIFF and len(s) > 0
        assert RD.apply_delta(_grid(first, W, H), bytes(s)) == _grid(second, W, H)


# ---- 6. group

def test_group_of_three_gives_the_one_context_bytes(R):
    S, w, h = 2, 37, 7
    p = _prm(SS.case_params(O, w, h, S, CAM, FAR)[0])
    with R.Context(w, h, devices=[0, 0, 0]) as g, R.Context(w, h) as one:
        for x in (g, one):
            x.set_reference_default_scene()
            x.set_option(R.OPT_SUPERSAMPLE, S)
        assert [g.member_option(r, R.OPT_SUPERSAMPLE) for r in range(3)] == [S, S, S]
        for mode in (O.RGB_ASCII, O.BIT_ASCII):
            want = one.render_to_host(p, mode)
            assert one.last_kernel.startswith("rtx_resolve<2,")
            assert np.array_equal(g.render_to_host(p, mode), want)
            assert all(g.member_kernel(r).startswith("rtx_resolve<2,") for r in range(3)), [g.member_kernel(r) for r in range(3)]
            assert np.array_equal(g.update(p, mode).copy(), one.update(p, mode).copy())
        # ... which are the fold's
        samples = None
        one.set_option(R.OPT_SUPERSAMPLE, 1)
        samples = _rows(R, one, SS.sample_params(p, S), O.RGB_ASCII, R.RENDER_VALUES).view(np.float32)
        rec = SS.expected(samples, w, h, S, O.RGB_ASCII, FAR)[1]
        assert np.array_equal(g.render_to_host(p, O.RGB_ASCII)[:rec.size], rec.reshape(-1))


# ---- 7. refusals

def test_refused_inside_a_capture(R, ctx):
    import torch
    S, mode = 2, O.RGB_ASCII
    p = _prm(SS.case_params(O, W, H, S, CAM, FAR)[0])
    ctx.set_option(R.OPT_SUPERSAMPLE, 1)
    want = _rows(R, ctx, p, mode)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frames = ctx.get_option(R.STAT_SUPERSAMPLE_FRAMES)
    ctx.set_option(R.OPT_SUPERSAMPLE, S)
    ctx.graph_begin(s.cuda_stream)
    try:
        with pytest.raises(R.RtxError) as e:
            ctx.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
        assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
        assert ctx.get_option(R.STAT_SUPERSAMPLE_FRAMES) == frames
        # the capture goes on: with one sample per cell the same call is recorded
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)
        ctx.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    finally:
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)
        g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want)
    finally:
        ctx.graph_destroy(g)


def test_a_sample_frame_of_2_to_the_31_is_refused(R, ctx):
    import torch
    buf = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = _prm(SS.case_params(O, W, H, 2, CAM, FAR)[0])
    ctx.set_option(R.OPT_SUPERSAMPLE, 4)
    try:
        frames, kernel = ctx.get_option(R.STAT_SUPERSAMPLE_FRAMES), ctx.last_kernel
        for x, y in ((1 << 30, 1), (1, 1 << 30)):
            p.x, p.y = x, y
            with pytest.raises(R.RtxError) as e:
                ctx.render_rows(p, O.RGB_ASCII, 0, 1, d_out=buf.data_ptr(), out_row_base=0, flags=R.RENDER_COMPACT)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and "2^31" in str(e.value)
        ctx.synchronize()
        assert ctx.get_option(R.STAT_SUPERSAMPLE_FRAMES) == frames and ctx.last_kernel == kernel
        assert (buf.cpu().numpy() == 0xEE).all()
    finally:
        ctx.set_option(R.OPT_SUPERSAMPLE, 1)
