"""Delta frames of half-block streams on the GPU (rtx_half_delta_words, rtx_update_half_delta; include/rtx.h) against
tests/restate_half_delta.py: rtx_half_delta_words is byte for byte half_delta_stream at the smallest shapes at which each piece of
the slot source can go wrong, in its three launch forms, with its two counters; and rtx_update_half_delta, as one sequence on a small
scene, hands out rtx_update_half's bytes as key frames and the restatement's stream of the words rtx_render_rows gives for the two
sample frames as deltas."""
import numpy as np
import pytest

import restate_half as RH
import restate_half_delta as RD
import util as U

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
FILL = 0xA5

# (W, H) of the console
SHAPES = [(1, 3),       # no cells, 0 bytes
          (2, 1),       # one cell
          (2, 5),       # every cell is column 0: every changed cell is a start
          (3, 1),       # a single short row
          (33, 31),     # 1023 slots
          (32, 32),     # exactly one block
          (41, 25),     # 1025 slots
          (1025, 1),    # a block boundary inside a row: the left neighbour comes from the halo
          (1024, 3),    # rows begin at block boundaries: the halo must not be consulted
          (257, 260),   # 66 blocks: the look-back's second level
          (120, 101)]   # row and column numbers cross 9 -> 10 and 99 -> 100
DENSITIES = (0.0, 0.02, 0.5, 1.0)


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


def run_delta(R, ctx, mode, W, H, cur, prev):
    """rtx_half_delta_words on the pair: (stream, changed cells, runs).  The output buffer is pre-filled: nothing past the stream is
    written, and the stream is no longer than the bound."""
    import torch
    tc, tp = to_device(cur), to_device(prev)
    cap = R.half_delta_bound(mode, W, H)
    out = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the context works on its own non-blocking stream
    n = ctx.half_delta_words(mode, W, H, tc.data_ptr(), tp.data_ptr(), out.data_ptr(), cap)
    got = out.cpu().numpy()
    assert n <= cap and (got[n:] == FILL).all(), "bytes written past the stream"
    return bytes(got[:n]), ctx.get_option(R.STAT_DELTA_CELLS), ctx.get_option(R.STAT_DELTA_RUNS)


def check(R, ctx, mode, W, H, cur, prev, what=""):
    want = RD.half_delta_stream(mode, W, H, cur, prev)
    got = run_delta(R, ctx, mode, W, H, cur, prev)
    if got[0] != want[0]:
        a, b = np.frombuffer(got[0], np.uint8), np.frombuffer(want[0], np.uint8)
        k = min(a.size, b.size)
        d = np.flatnonzero(a[:k] != b[:k])
        at = int(d[0]) if d.size else k
        raise AssertionError("mode %d %dx%d %s: %d bytes against %d, first difference at %d: got %r want %r" %
                             (mode, W, H, what, a.size, b.size, at, got[0][max(0, at - 24):at + 24], want[0][max(0, at - 24):at + 24]))
    assert got[1:] == want[1:], (mode, W, H, what, got[1:], want[1:])
    assert len(got[0]) <= RD.half_delta_bound(mode, W, H) == R.half_delta_bound(mode, W, H)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL])
def test_half_delta_words_is_the_restatement(R, ctx, mode, shape):
    W, H = shape
    rng = np.random.default_rng(3000 + 100 * mode + W + H)
    replayed = False
    for density in DENSITIES:
        for name, cur, prev in RD.frame_pairs(rng, W, H, density):
            s, cells, runs = check(R, ctx, mode, W, H, cur, prev, "%s at density %g" % (name, density))
            if density == 0.0 or W == 1:
                assert (s, cells, runs) == (b"", 0, 0)
            if W == 2:
                assert runs == cells  # column 0 alone: every changed cell starts a run
            if (W, H) in ((33, 31), (120, 101)) and density == 0.5 and name == "digits":
                assert RD.apply_half_delta(mode, RH.keys(mode, W, H, prev), s) == RH.keys(mode, W, H, cur)
                replayed = True
    assert replayed == ((W, H) in ((33, 31), (120, 101)))


def test_equal_frames_leave_the_output_untouched(R, ctx):
    rng = np.random.default_rng(3100)
    for name, words in RH.populations(rng, 37, 61):
        for mode in (RH.BIT_PIXEL, RH.RGB_PIXEL):
            # (run_delta checks the fill behind the stream: all of it; and reads both counters)
            assert run_delta(R, ctx, mode, 37, 61, words, words.copy()) == (b"", 0, 0), name


def test_what_is_no_change_emits_nothing(R, ctx):
    W, H = 41, 25
    rng = np.random.default_rng(3200)
    words = dict(RH.populations(rng, W, H))["palette"].copy()
    miss = rng.random(words.size) < 0.2
    words[miss] = 0
    words.reshape(2 * H, W)[:, W - 1] = NO
    # other glyphs over the same colours, and 0 against 0xffffffff outside the last column, in both families
    other = (words & np.uint32(0x00FFFFFF)) | (rng.integers(32, 127, size=words.size, dtype=np.uint32) << np.uint32(24))
    other = np.where(miss, np.where(rng.random(words.size) < 0.5, np.uint32(NO), np.uint32(0)), other).astype(np.uint32)
    other.reshape(2 * H, W)[:, W - 1] = NO
    assert (other != words).sum() > 1000
    for mode in (RH.BIT_PIXEL, RH.RGB_PIXEL, RH.BIT_ASCII):
        assert check(R, ctx, mode, W, H, other, words) == (b"", 0, 0)
        assert check(R, ctx, mode, W, H, words, other) == (b"", 0, 0)
    # the 8-bit family: 0 against any word whose byte 0 is 16; the RGB family sees those cells change
    sixteen = np.where(words == 0, np.uint32(0x41332210), words).astype(np.uint32)
    assert (sixteen != words).sum() > 50
    assert check(R, ctx, RH.BIT_PIXEL, W, H, sixteen, words) == (b"", 0, 0)
    assert check(R, ctx, RH.RGB_PIXEL, W, H, sixteen, words)[1] > 25


@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL])
def test_cells_of_which_one_half_changed(R, ctx, mode):
    W, H = 6, 2
    G = RH.GLYPH
    prev = np.full((2 * H, W), 0x20010203, dtype=np.uint32)
    prev[:, W - 1] = NO
    cur = prev.copy()
    cur[0, 1] = 0x20040506      # row 0: cell 1, the top alone: a start, both escapes
    cur[1, 3] = 0x20040506      #        cell 3, the bottom alone: a start
    cur[1, 4] = 0x20070809      #        cell 4, the bottom alone, inside the run: the background escape alone
    cur[2, 0:3] = 0x20040506    # row 1: cells 0 .. 2, the top alone: one run, one foreground escape
    cur[3, 2] = 0x20070809      #        and cell 2's bottom as well: its background escape alone
    s, cells, runs = check(R, ctx, mode, W, H, cur.reshape(-1), prev.reshape(-1))
    k = lambda w: RH.key(mode, w)
    fg, bg = (lambda w: RH.sgr(mode, "3", k(w))), (lambda w: RH.sgr(mode, "4", k(w)))
    old, a, b = 0x20010203, 0x20040506, 0x20070809
    assert s == (RD.cup(0, 1) + fg(a) + bg(old) + G +
                 RD.cup(0, 3) + fg(old) + bg(a) + G + bg(b) + G +
                 RD.cup(1, 0) + fg(a) + bg(old) + G + G + bg(b) + G)
    assert (cells, runs) == (6, 3)


def test_an_ascii_mode_gives_the_pixel_modes_bytes(R, ctx):
    W, H = 41, 25
    rng = np.random.default_rng(3300)
    for name, cur, prev in RD.frame_pairs(rng, W, H, 0.5):
        assert check(R, ctx, RH.RGB_ASCII, W, H, cur, prev, name) == check(R, ctx, RH.RGB_PIXEL, W, H, cur, prev, name)


def full_length_row(W):
    """Two rows of W words (a one-row console): neighbouring cells differ in both halves, every component has three digits."""
    i = np.arange(2 * W, dtype=np.uint32)
    v = 100 + (i * 7 + (i // W) * 3) % 150
    words = (v | ((v + 1) << np.uint32(8)) | ((v + 2) << np.uint32(16))).astype(np.uint32)
    words.reshape(2, W)[:, W - 1] = NO
    return words


@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL])
def test_a_row_longer_than_a_block(R, ctx, mode):
    W, H = 2100, 1
    C = 41 if mode == RH.RGB_PIXEL else 25
    cur = full_length_row(W)
    other = np.where(cur == NO, np.uint32(NO), np.uint32(0x00FEFDFC))  # differs from every cell of cur in both halves

    def pair(changed):
        prev = cur.copy().reshape(2, W)
        prev[:, changed] = other.reshape(2, W)[:, changed]
        return prev.reshape(-1)

    # 1. cells 1023 and 1024 changed: the run crosses the block edge -- no cursor escape at block 1's first slot, and its elision is
    #    made against the halo
    s, cells, runs = check(R, ctx, mode, W, H, cur, pair([1023, 1024]), "a run across the block edge")
    assert (cells, runs) == (2, 1) and len(s) == 9 + 2 * C and s.startswith(RD.cup(0, 1023))
    same_top = cur.copy().reshape(2, W)
    same_top[0, 1024] = same_top[0, 1023]  # the halo's T: the foreground escape of cell 1024 is elided
    prev = same_top.copy()
    prev[:, [1023, 1024]] = 0x00FEFDFC
    s, cells, runs = check(R, ctx, mode, W, H, same_top.reshape(-1), prev.reshape(-1), "elision against the halo")
    assert (cells, runs) == (2, 1) and len(s) == 9 + 2 * C - (C - 3) // 2
    # 2. cell 1023 unchanged, cells 1024 .. 2047 all changed, every escape at full length: block 1 emits 9 + 1024 C bytes, more than
    #    a half-block frame's block can
    s, cells, runs = check(R, ctx, mode, W, H, cur, pair(np.arange(1024, 2048)), "a block's longest stream")
    assert (cells, runs) == (1024, 1) and len(s) == 9 + 1024 * C > 1024 * C and s.startswith(RD.cup(0, 1024))
    # 3. every cell changed
    s, cells, runs = check(R, ctx, mode, W, H, cur, pair(np.arange(0, W - 1)), "every cell")
    assert (cells, runs) == (W - 1, 1) and len(s) == 6 + (W - 1) * C
    # 4. alternating cells: as many runs as cells
    s, cells, runs = check(R, ctx, mode, W, H, cur, pair(np.arange(0, W - 1, 2)), "alternating cells")
    assert cells == runs == W // 2
    s, cells, runs = check(R, ctx, mode, W, H, cur, pair(np.arange(1, W - 1, 2)), "the other alternating cells")
    assert cells == runs == (W - 1) // 2


def test_the_three_forms_give_the_same_bytes(R):
    rng = np.random.default_rng(3400)
    with R.Context(64, 64) as c:
        before = c.get_option(R.STAT_MINIMIZE_FALLBACKS)
        launches = 0
        for mode in (RH.BIT_PIXEL, RH.RGB_PIXEL):
            for (W, H) in ((41, 25), (257, 260)):
                pairs = {name: (cur, prev) for name, cur, prev in RD.frame_pairs(rng, W, H, 0.5 if W == 41 else 0.02)}
                cur, prev = pairs["random" if W == 41 else "palette"]
                want = RD.half_delta_stream(mode, W, H, cur, prev)
                assert want[1] > 0
                for form in (1, 0, 2):
                    c.set_option(R.OPT_MINIMIZE_FUSED, form)
                    assert run_delta(R, c, mode, W, H, cur, prev) == want, (mode, W, H, form)
                launches += 1
        assert c.get_option(R.STAT_MINIMIZE_FALLBACKS) - before == launches  # one per launch of form 2


def test_refusals_leave_the_output_alone(R, ctx):
    import torch
    W, H = 33, 31
    _, cur, prev = RD.frame_pairs(np.random.default_rng(3500), W, H, 0.5)[1]
    tc, tp = to_device(cur), to_device(prev)
    bound = R.half_delta_bound(RH.RGB_PIXEL, W, H)
    out = torch.full((bound + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a, b, o = tc.data_ptr(), tp.data_ptr(), out.data_ptr()
    for args, status in (((R.RGB_PIXEL, W, H, a, b, o, bound - 1), R.ERR_TOO_LARGE),  # one below the bound
                         ((R.SDL, W, H, a, b, o, 1 << 30), R.ERR_INVALID_MODE),
                         ((6, W, H, a, b, o, 1 << 30), R.ERR_INVALID_MODE),
                         ((R.RGB_PIXEL, 0, H, a, b, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, 0, a, b, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, 100001, 1, a, b, o, 1 << 62), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, 1, 100000, a, b, o, 1 << 62), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, H, a + 2, b, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, H, a, b + 2, o, 1 << 30), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_PIXEL, W, H, a, b, o + 8, 1 << 30), R.ERR_INVALID_ARGUMENT)):
        with pytest.raises(R.RtxError) as e:
            ctx.half_delta_words(*args)
        assert e.value.status == status, args
    ctx.synchronize()
    assert (out.cpu().numpy() == FILL).all()


# ---- rtx_update_half_delta on a small scene, as one sequence

SIZES = [(81, 25), (160, 50)]
YAW = 3.14159274


def small_scene(R, c, W, H):
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(91, 64, 1, p.element1, p.element2)
    c.set_scene(sph, pl)
    for i in range(0, 64, 3):
        c.set_sphere_motion(i, 1 if i % 2 else -1, 3.0)
    return p


def sample_words(R, c, p, mode):
    """The sample frame's pixel words -- p with twice the rows -- as rtx_render_rows stores them on this context."""
    import torch
    q = R.Params.from_buffer_copy(bytes(p))
    q.y = 2 * int(p.y)
    W, H2 = int(q.x), int(q.y)
    t = torch.zeros(W * H2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.render_rows(q, mode, 0, H2, d_out=t.data_ptr(), flags=R.RENDER_COMPACT)
    c.synchronize()
    return t.cpu().numpy().view(np.uint32)


def call(c, p, mode, **kw):
    s, kind = c.update_half_delta(p, mode, **kw)
    return bytes(s), kind


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_update_half_delta_as_one_sequence(R, size):
    W, H = size
    mode = RH.RGB_PIXEL
    with R.Context(W, 2 * H) as c, R.Context(W, 2 * H) as twin:
        p = small_scene(R, c, W, H)
        small_scene(R, twin, W, H)
        state = {}

        def expect_key(p, mode, **kw):
            s, kind = call(c, p, mode, **kw)
            words = sample_words(R, c, p, mode)
            assert kind == R.DELTA_KEY and s == RH.half_stream(mode, int(p.x), int(p.y), words) and len(s) > 0
            state["words"], state["grid"] = words, RH.keys(mode, int(p.x), int(p.y), words)
            # and the frame after it is a delta against it: at rest, nothing
            assert call(c, p, mode) == (b"", R.DELTA_DIFF)
            assert c.get_option(R.STAT_DELTA_CELLS) == 0 and c.get_option(R.STAT_DELTA_RUNS) == 0
            return s

        def step(p, mode, **kw):
            s, kind = call(c, p, mode, **kw)
            assert kind == R.DELTA_DIFF
            now = sample_words(R, c, p, mode)
            want, cells, runs = RD.half_delta_stream(mode, int(p.x), int(p.y), now, state["words"])
            assert s == want
            assert (c.get_option(R.STAT_DELTA_CELLS), c.get_option(R.STAT_DELTA_RUNS)) == (cells, runs)
            grid = RD.apply_half_delta(mode, state["grid"], s)
            assert grid == RH.keys(mode, int(p.x), int(p.y), now)
            state["words"], state["grid"] = now, grid
            return cells

        # the first call: a key frame, rtx_update_half's bytes; then rest
        assert expect_key(p, mode) == bytes(twin.update_half(p, mode))
        assert len({cell for row in state["grid"] for cell in row}) > 8  # (a picture, not one colour)
        assert step(p, mode, dt=0.25, run_physics=True) > 0              # a physics step
        moved = R.camera_params(W, H, (0.0, 0.0, 0.0), (0.0, YAW + 0.02, 0.0))
        assert step(moved, mode) > 0                                     # a camera step
        assert (c.get_option(R.STAT_HALF_DELTA_FRAMES), c.get_option(R.STAT_HALF_DELTA_KEYFRAMES)) == (4, 1)
        expect_key(moved, mode, flags=R.DELTA_KEYFRAME)                  # the flag
        expect_key(moved, RH.BIT_PIXEL)                                  # another mode
        if size == SIZES[0]:
            small = R.camera_params(48, 20, (0.0, 0.0, 0.0), (0.0, YAW + 0.02, 0.0))
            expect_key(small, RH.BIT_PIXEL)                              # another size
            expect_key(moved, mode)
            keys = 5
            # every other entry point of the family in between makes the next call a key frame
            assert len(c.update(moved, mode)) > 0
            expect_key(moved, mode)
            ptr, _, _ = c._pinned_buffer(20 * W * H)
            assert c.update_end(c.update_begin(moved, mode, ptr)) > 0
            expect_key(moved, mode)
            _, kind = c.update_delta(moved, mode)
            assert kind == R.DELTA_KEY
            expect_key(moved, mode)
            assert len(c.update_half(moved, mode)) > 0
            expect_key(moved, mode)
            keys += 4
            # and rtx_update_delta after a half-block delta gives a key frame, twice in a row only once
            _, kind = c.update_delta(moved, mode)
            assert kind == R.DELTA_KEY
            _, kind = c.update_delta(moved, mode)
            assert kind == R.DELTA_DIFF
            expect_key(moved, mode)
            keys += 1
            # a host buffer too small for the stream: RTX_ERR_TOO_LARGE, nothing copied, and a key frame next
            turned = R.camera_params(W, H, (0.0, 0.0, 0.0), (0.0, YAW - 0.3, 0.0))
            ptr, _, arr = c._pinned_buffer(R.half_delta_bound(mode, W, H))
            arr[:] = FILL
            with pytest.raises(R.RtxError) as e:
                c.update_half_delta(turned, mode, capacity=8)
            assert e.value.status == R.ERR_TOO_LARGE and (arr == FILL).all()
            expect_key(turned, mode)
            keys += 1
            assert step(moved, mode) > 0                                 # and deltas go on from there
            assert c.get_option(R.STAT_HALF_DELTA_KEYFRAMES) == keys
            frames = c.get_option(R.STAT_HALF_DELTA_FRAMES)
            # refusals: they count nothing, and a call refused by a check leaves the next one a delta
            for bad in (R.SDL, 6, -1):
                with pytest.raises(R.RtxError) as e:
                    c.update_half_delta(moved, bad)
                assert e.value.status == R.ERR_INVALID_MODE
            with pytest.raises(R.RtxError) as e:
                c.update_half_delta(moved, mode, flags=2)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            assert call(c, moved, mode) == (b"", R.DELTA_DIFF)
            assert c.get_option(R.STAT_HALF_DELTA_FRAMES) == frames + 1
            # the older counters: the one half-block frame and the three delta frames asked for by name above, no more
            assert c.get_option(R.STAT_HALF_FRAMES) == 1 and c.get_option(R.STAT_DELTA_FRAMES) == 3
    with R.Context(W, H) as small_ctx:
        p = small_scene(R, small_ctx, W, H)
        with pytest.raises(R.RtxError) as e:
            small_ctx.update_half_delta(p, mode)  # a context created for H rows
        assert e.value.status == R.ERR_TOO_LARGE
        assert small_ctx.get_option(R.STAT_HALF_DELTA_FRAMES) == 0


def frames_of(R, c, W, H, mode):
    """Key frame, rest, a physics step, a camera step: the four streams with their kinds."""
    p = R.camera_params(W, H)
    moved = R.camera_params(W, H, (0.0, 0.0, 0.0), (0.05, YAW + 0.03, 0.0))
    return [call(c, p, mode), call(c, p, mode), call(c, p, mode, dt=0.125, run_physics=True), call(c, moved, mode)]


def test_update_half_delta_supersampled(R):
    W, H = SIZES[0]
    mode = RH.RGB_PIXEL
    with R.Context(W, 2 * H) as c:
        p = small_scene(R, c, W, H)
        c.set_option(R.OPT_SUPERSAMPLE, 2)
        s, kind = call(c, p, mode)
        assert kind == R.DELTA_KEY and s == bytes(c.update_half(p, mode))
        assert call(c, p, mode)[1] == R.DELTA_KEY  # (rtx_update_half ran in between)
        before = sample_words(R, c, p, mode)
        s, kind = call(c, p, mode, dt=0.25, run_physics=True)
        now = sample_words(R, c, p, mode)
        assert kind == R.DELTA_DIFF and s == RD.half_delta_stream(mode, W, H, now, before)[0] and len(s) > 0
        assert RD.apply_half_delta(mode, RH.keys(mode, W, H, before), s) == RH.keys(mode, W, H, now)


def test_update_half_delta_with_shadows_two_lights_and_mirrors(R):
    W, H = SIZES[0]
    mode = RH.RGB_PIXEL
    with R.Context(W, 2 * H) as c:
        p = small_scene(R, c, W, H)
        plain, _ = call(c, p, mode)
        c.set_option(R.OPT_SHADOWS, 1)
        c.set_lights([R.make_light(), R.make_light(pos=(-20.0, 30.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=900.0)])
        c.set_option(R.OPT_REFLECT_DEPTH, 2)
        c.set_reflectivity(0, [0.5] * 65)
        before = sample_words(R, c, p, mode)
        s, kind = call(c, p, mode, flags=R.DELTA_KEYFRAME)
        assert kind == R.DELTA_KEY and s == RH.half_stream(mode, W, H, before) and s != plain
        s, kind = call(c, p, mode, dt=0.25, run_physics=True)
        now = sample_words(R, c, p, mode)
        assert kind == R.DELTA_DIFF and s == RD.half_delta_stream(mode, W, H, now, before)[0] and len(s) > 0
        assert RD.apply_half_delta(mode, RH.keys(mode, W, H, before), s) == RH.keys(mode, W, H, now)


def test_a_group_of_three_ranks_gives_the_plain_bytes(R):
    W, H = SIZES[0]
    mode = RH.RGB_PIXEL
    with R.Context(W, 2 * H) as c, R.Context(W, 2 * H, devices=[0, 0, 0]) as g:
        small_scene(R, c, W, H)
        small_scene(R, g, W, H)
        assert g.group_size == 3  # (50 sample rows over three ranks: ragged slabs)
        plain, group = frames_of(R, c, W, H, mode), frames_of(R, g, W, H, mode)
        assert plain == group
        assert [k for _, k in plain] == [R.DELTA_KEY, R.DELTA_DIFF, R.DELTA_DIFF, R.DELTA_DIFF]
        assert plain[1][0] == b"" and len(plain[2][0]) > 0 and len(plain[3][0]) > 0
