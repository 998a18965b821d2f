"""Half-block frames on the GPU (rtx_half_words, rtx_update_half; include/rtx.h) against tests/restate_half.py: rtx_half_words is
byte for byte half_stream at the smallest shapes at which each piece of the slot source can go wrong, in its three launch forms, and
rtx_update_half hands out the restatement's stream of the words rtx_render_rows gives for the sample frame on the same context."""
import numpy as np
import pytest

import restate_half as RH
import util as U

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
FILL = 0xA5

# (W, H) of the console: what each shape exercises is said in the issue's table and beside the case it fails at
SHAPES = [(1, 3),       # no cells
          (2, 1),       # one cell
          (2, 5),       # the previous cell is always a row up
          (3, 1),       # a single short row
          (33, 31),     # 1023 slots
          (32, 32),     # exactly one block
          (41, 25),     # 1025 slots
          (1025, 1),    # a block boundary inside a row
          (1024, 3),    # rows begin at block boundaries: the g-2 cell comes from the halo
          (257, 260)]   # 66 blocks: the look-back's second level


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(64, 64)
    yield c
    c.close()


def to_device(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).cuda()


def run_half(R, ctx, mode, W, H, words):
    """rtx_half_words on the frame: the stream.  The output buffer is pre-filled: nothing past the stream is written."""
    import torch
    tw = to_device(words)
    cap = R.half_bound(mode, W, H)
    out = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the context works on its own non-blocking stream
    n = ctx.half_words(mode, W, H, tw.data_ptr(), out.data_ptr(), cap)
    got = out.cpu().numpy()
    assert n <= cap and (got[n:] == FILL).all(), "bytes written past the stream"
    return bytes(got[:n])


def check(R, ctx, mode, W, H, words, what=""):
    want = RH.half_stream(mode, W, H, words)
    got = run_half(R, ctx, mode, W, H, words)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        k = min(a.size, b.size)
        d = np.flatnonzero(a[:k] != b[:k])
        at = int(d[0]) if d.size else k
        raise AssertionError("mode %d %dx%d %s: %d bytes against %d, first difference at %d: got %r want %r" %
                             (mode, W, H, what, a.size, b.size, at, got[max(0, at - 24):at + 24], want[max(0, at - 24):at + 24]))
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL])
def test_half_words_is_the_restatement(R, ctx, mode, shape):
    W, H = shape
    rng = np.random.default_rng(1000 + 100 * mode + W + H)
    for name, words in RH.populations(rng, W, H):
        s = check(R, ctx, mode, W, H, words, name)
        if name == "zeros":
            first = RH.sgr(mode, "3", RH.key(mode, 0)) + RH.sgr(mode, "4", RH.key(mode, 0))
            assert s == ((first + RH.GLYPH + RH.GLYPH * (W - 2) + b"\n" + (RH.GLYPH * (W - 1) + b"\n") * (H - 1)) if W > 1 else b"\n" * H)
    if (W, H) == (33, 31):
        assert RH.replay(mode, s, W, H) == RH.keys(mode, W, H, words)


def test_the_glyph_byte_is_ignored_in_an_ascii_mode(R, ctx):
    W, H = 41, 25
    rng = np.random.default_rng(1100)
    for name, words in RH.populations(rng, W, H):
        s = check(R, ctx, RH.RGB_ASCII, W, H, words, name)
        assert s == RH.half_stream(RH.RGB_PIXEL, W, H, words & np.uint32(0x00FFFFFF) | np.where(words == NO, np.uint32(0xFF000000), np.uint32(0)))


def test_the_bound_is_met_by_a_frame_whose_cells_all_differ(R, ctx):
    # a block of cells alone (one long row), every escape due at its full length: the block's image is full
    W, H = 1200, 2
    v = 100 + (np.arange(W * 2 * H, dtype=np.uint32) * 7 + (np.arange(W * 2 * H, dtype=np.uint32) // W) * 3) % 150
    words = (v | ((v + 1) << np.uint32(8)) | ((v + 2) << np.uint32(16))).astype(np.uint32)
    words.reshape(2 * H, W)[:, W - 1] = NO
    for mode in (RH.BIT_PIXEL, RH.RGB_PIXEL):
        assert len(check(R, ctx, mode, W, H, words)) == R.half_bound(mode, W, H)


def test_the_three_forms_give_the_same_bytes(R):
    rng = np.random.default_rng(1200)
    with R.Context(64, 64) as c:
        before = c.get_option(R.STAT_MINIMIZE_FALLBACKS)
        launches = 0
        for mode in (RH.BIT_PIXEL, RH.RGB_PIXEL):
            for (W, H) in ((41, 25), (257, 260)):
                words = dict(RH.populations(rng, W, H))["random" if W == 41 else "palette"]
                for form in (1, 0, 2):
                    c.set_option(R.OPT_MINIMIZE_FUSED, form)
                    check(R, c, mode, W, H, words, "form %d" % form)
                launches += 1
        assert c.get_option(R.STAT_MINIMIZE_FALLBACKS) - before == launches  # one per launch of form 2


def test_refusals_leave_the_output_alone(R, ctx):
    import torch
    W, H = 33, 31
    words = to_device(dict(RH.populations(np.random.default_rng(1300), W, H))["random"])
    out = torch.full((R.half_bound(RH.RGB_PIXEL, W, H) + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, o = words.data_ptr(), out.data_ptr()
    for args, status in (((R.RGB_PIXEL, W, H, w, o, R.half_bound(R.RGB_PIXEL, W, H) - 1), R.ERR_TOO_LARGE),  # one below the bound
                         ((R.SDL, W, H, w, o, 1 << 30), R.ERR_INVALID_MODE),
                         ((6, W, H, w, o, 1 << 30), R.ERR_INVALID_MODE),
                         ((R.RGB_PIXEL, 0, H, w, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, 0, w, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, 1 << 31, 1, w, o, 1 << 62), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, 1, 1 << 30, w, o, 1 << 62), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, H, w + 2, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, H, w, o + 8, 1 << 30), R.ERR_INVALID_ARGUMENT)):
        with pytest.raises(R.RtxError) as e:
            ctx.half_words(*args)
        assert e.value.status == status, args
    ctx.synchronize()
    assert (out.cpu().numpy() == FILL).all()


# ---- rtx_update_half on a small scene

SIZES = [(81, 25), (160, 50)]


def small_scene(R, c, W, H):
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(91, 64, 1, p.element1, p.element2)
    c.set_scene(sph, pl)
    return p


def sample_params(R, p):
    """p': the console's params with twice the rows."""
    q = R.Params.from_buffer_copy(bytes(p))
    q.y = 2 * int(p.y)
    return q


def sample_words(R, c, p, mode):
    """The sample frame's pixel words as rtx_render_rows stores them on this context."""
    import torch
    q = sample_params(R, p)
    W, H2 = int(q.x), int(q.y)
    t = torch.zeros(W * H2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.render_rows(q, mode, 0, H2, d_out=t.data_ptr(), flags=R.RENDER_COMPACT)
    c.synchronize()
    return t.cpu().numpy().view(np.uint32)


def check_update(R, c, p, mode):
    W, H = int(p.x), int(p.y)
    s = bytes(c.update_half(p, mode))
    words = sample_words(R, c, p, mode)
    assert s == RH.half_stream(mode, W, H, words)
    grid = RH.keys(mode, W, H, words)
    assert RH.replay(mode, s, W, H) == grid
    assert len({cell for row in grid for cell in row}) > 8  # (a picture, not one colour)
    return s


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL])
def test_update_half_is_the_restatement_of_the_sample_frame(R, mode, size):
    W, H = size
    with R.Context(W, 2 * H) as c:
        p = small_scene(R, c, W, H)
        before = c.get_option(R.STAT_HALF_FRAMES)
        check_update(R, c, p, mode)
        moved = R.camera_params(W, H, (0.0, 1.0, 0.0), (0.05, 3.14159274 + 0.2, 0.0))
        check_update(R, c, moved, mode)
        assert c.get_option(R.STAT_HALF_FRAMES) - before == 2


def test_update_half_supersampled(R):
    W, H = SIZES[0]
    with R.Context(W, 2 * H) as c:
        p = small_scene(R, c, W, H)
        plain = check_update(R, c, p, RH.RGB_PIXEL)
        c.set_option(R.OPT_SUPERSAMPLE, 2)
        assert check_update(R, c, p, RH.RGB_PIXEL) != plain  # (partial coverage shows at the silhouettes)


def test_update_half_with_shadows_two_lights_and_mirrors(R):
    W, H = SIZES[0]
    with R.Context(W, 2 * H) as c:
        p = small_scene(R, c, W, H)
        plain = check_update(R, c, p, RH.RGB_PIXEL)
        c.set_option(R.OPT_SHADOWS, 1)
        c.set_lights([R.make_light(), R.make_light(pos=(-20.0, 30.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=900.0)])
        c.set_option(R.OPT_REFLECT_DEPTH, 2)
        c.set_reflectivity(0, [0.5] * 65)
        assert check_update(R, c, p, RH.RGB_PIXEL) != plain


def test_update_half_on_a_group_of_three_ranks(R):
    W, H = SIZES[0]
    with R.Context(W, 2 * H) as c, R.Context(W, 2 * H, devices=[0, 0, 0]) as g:
        p = small_scene(R, c, W, H)
        small_scene(R, g, W, H)
        assert g.group_size == 3  # (50 sample rows over three ranks: ragged slabs)
        assert check_update(R, g, p, RH.RGB_PIXEL) == check_update(R, c, p, RH.RGB_PIXEL)


def test_update_half_behaviour(R):
    W, H = SIZES[0]
    mode = RH.RGB_PIXEL
    with R.Context(W, H) as small:
        p = small_scene(R, small, W, H)
        with pytest.raises(R.RtxError) as e:
            small.update_half(p, mode)  # a context created for H rows
        assert e.value.status == R.ERR_TOO_LARGE
        assert small.get_option(R.STAT_HALF_FRAMES) == 0
    with R.Context(W, 2 * H) as c:
        p = small_scene(R, c, W, H)
        # rtx_update's bytes for the same camera are the same before and after a half frame
        before = bytes(c.update(p, mode))
        s = check_update(R, c, p, mode)
        assert bytes(c.update(p, mode)) == before and len(before) > 0
        # a host_capacity one short: RTX_ERR_TOO_LARGE, and host_out is left as it was
        ptr, size, arr = c._pinned_buffer(R.half_bound(mode, W, H))
        arr[:] = FILL
        with pytest.raises(R.RtxError) as e:
            c.update_half(p, mode, capacity=len(s) - 1)
        assert e.value.status == R.ERR_TOO_LARGE and (arr == FILL).all()
        assert bytes(c.update_half(p, mode, capacity=len(s))) == s
        # a delta frame after a half frame is a key frame -- after a failed one too
        _, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_KEY
        _, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_DIFF
        c.update_half(p, mode)
        _, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_KEY
        c.update_delta(p, mode)
        with pytest.raises(R.RtxError):
            c.update_half(p, mode, capacity=8)
        _, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_KEY
        assert c.get_option(R.STAT_HALF_FRAMES) == 3
        for bad in (R.SDL, 6, -1):
            with pytest.raises(R.RtxError) as e:
                c.update_half(p, bad)
            assert e.value.status == R.ERR_INVALID_MODE
