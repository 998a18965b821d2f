"""Delta frames on the GPU (rtx_delta_words, rtx_update_delta; include/rtx.h) against tests/restate_delta.py: the restatement's
records are rtx_expand's, rtx_delta_words is byte for byte delta_stream at the smallest shapes at which it can go wrong, and the
streams rtx_update_delta hands out, replayed over a grid of records, give every frame's records."""
import numpy as np
import pytest

import restate_delta as RD
import util as U

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
FILL = 0xA5


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(1040, 128)
    yield c
    c.close()


def to_device(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).cuda()


def run_delta(R, ctx, mode, W, H, cur, prev):
    """rtx_delta_words on the two frames: (stream, cells, runs).  The output buffer is pre-filled: nothing past the stream is written."""
    import torch
    tc, tp = to_device(cur), to_device(prev)
    cap = R.delta_bound(mode, W, H)
    out = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the context works on its own non-blocking stream
    n = ctx.delta_words(mode, W, H, tc.data_ptr(), tp.data_ptr(), out.data_ptr(), cap)
    got = out.cpu().numpy()
    assert n <= cap and (got[n:] == FILL).all(), "bytes written past the stream"
    return bytes(got[:n]), ctx.get_option(R.STAT_DELTA_CELLS), ctx.get_option(R.STAT_DELTA_RUNS)


def check(R, ctx, mode, W, H, cur, prev):
    want = RD.delta_stream(mode, W, H, cur, prev)
    got = run_delta(R, ctx, mode, W, H, cur, prev)
    assert got[1:] == want[1:], (mode, W, H, got[1:], want[1:])
    if got[0] != want[0]:
        a, b = np.frombuffer(got[0], np.uint8), np.frombuffer(want[0], np.uint8)
        k = min(a.size, b.size)
        d = np.flatnonzero(a[:k] != b[:k])
        at = int(d[0]) if d.size else k
        raise AssertionError("mode %d %dx%d: %d bytes against %d, first difference at %d: got %r want %r" %
                             (mode, W, H, a.size, b.size, at, got[0][max(0, at - 24):at + 24], want[0][max(0, at - 24):at + 24]))
    return got


@pytest.mark.parametrize("mode", range(5))
def test_the_restated_records_are_the_ones_rtx_expand_writes(R, ctx, mode):
    import torch
    rng = np.random.default_rng(100 + mode)
    n = 3000
    words = (rng.integers(33, 127, size=n, dtype=np.uint32) << np.uint32(24)) | rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
    words[:256] = (np.uint32(65) << np.uint32(24)) | np.arange(256, dtype=np.uint32)          # every value of the first colour byte
    words[256:512] = (np.uint32(66) << np.uint32(24)) | (np.arange(256, dtype=np.uint32) << np.uint32(16))
    words[512:520] = [0, NO, 0x41000000, 0x20000000, 0x7E000010, 0x21FFFFFF, 0x30000a00, 0x39640000]
    S = RD.record_size(mode)
    src = to_device(words)
    dst = torch.full((S * n,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.expand(mode, src.data_ptr(), dst.data_ptr(), [(0, 0, n)])
    ctx.synchronize()
    got = dst.cpu().numpy().reshape(n, S)
    for i in range(n):
        assert bytes(got[i]) == RD.record_of_word(mode, words[i]), (i, hex(int(words[i])))


def test_a_frame_of_newline_columns_alone_is_empty(R, ctx):
    cur = np.array([1, 2, 3, 4, 5], dtype=np.uint32)
    prev = np.array([9, 9, 9, 9, 9], dtype=np.uint32)
    assert check(R, ctx, R.RGB_ASCII, 1, 5, cur, prev) == (b"", 0, 0)


@pytest.mark.parametrize("mode", range(5))
def test_two_columns_by_seven_rows(R, ctx, mode):
    rng = np.random.default_rng(200 + mode)
    cur, prev = RD.random_frame_pair(rng, 2, 7, 0.7)
    s, cells, runs = check(R, ctx, mode, 2, 7, cur, prev)
    assert cells == runs > 0  # one cell per row: every changed cell starts a run


@pytest.mark.parametrize("density", [0.0, 0.02, 0.5, 1.0])
@pytest.mark.parametrize("mode", range(5))
def test_three_blocks_at_every_density(R, ctx, mode, density):
    rng = np.random.default_rng(300 + 10 * mode + int(density * 100))
    cur, prev = RD.random_frame_pair(rng, 37, 61, density, holes=0.03 if density == 0.5 else 0.0)
    s, cells, runs = check(R, ctx, mode, 37, 61, cur, prev)
    if density == 0.0:
        assert (s, cells, runs) == (b"", 0, 0)
    if density == 1.0:
        assert RD.apply_delta(RD.records(mode, 37, 61, prev), s) == RD.records(mode, 37, 61, cur)


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("case", ["edge_pair", "first_slot_of_a_block", "every_cell"])
def test_a_row_longer_than_a_block(R, ctx, mode, case):
    W, H = 1030, 3
    rng = np.random.default_rng(400 + mode)
    cur, prev = RD.random_frame_pair(rng, W, H, 1.0)
    if case != "every_cell":
        cur = prev.copy()
        for g in ((1023, 1024) if case == "edge_pair" else (1024,)):
            cur[g] = prev[g] ^ np.uint32(0x01010101) if prev[g] != 0 else np.uint32(0x41020304)
    else:
        # alternating cells as well: the longest stream a block can emit
        cur2 = cur.copy()
        cur2.reshape(H, W)[1, 0:W - 1:2] = prev.reshape(H, W)[1, 0:W - 1:2]
        check(R, ctx, mode, W, H, cur2, prev)
    s, cells, runs = check(R, ctx, mode, W, H, cur, prev)
    if case == "edge_pair":
        assert (cells, runs) == (2, 1) and s.startswith(b"\x1b[1;1024H")
    if case == "first_slot_of_a_block":
        assert (cells, runs) == (1, 1) and s.startswith(b"\x1b[1;1025H")


@pytest.mark.parametrize("mode", [1, 2])
def test_ninety_nine_blocks_and_the_digit_transitions(R, ctx, mode):
    W, H = 1001, 101
    rng = np.random.default_rng(500 + mode)
    cur, prev = RD.random_frame_pair(rng, W, H, 0.3)
    check(R, ctx, mode, W, H, cur, prev)
    # single cells on both sides of 9 / 10, 99 / 100 and 999 / 1000, as columns and (the first two) as rows
    cur = prev.copy()
    c2, p2 = cur.reshape(H, W), prev.reshape(H, W)
    want = []
    for row, cols in ((8, (8, 98, 998)), (9, (9, 99, 999)), (98, (9, 99, 999)), (99, (8, 98, 998)), (100, (8, 99, 998))):
        for col in cols:
            c2[row, col] = p2[row, col] ^ np.uint32(0x01010101) if p2[row, col] != 0 else np.uint32(0x41020304)
            want.append(b"\x1b[%d;%dH" % (row + 1, col + 1))
    s, cells, runs = check(R, ctx, mode, W, H, cur, prev)
    assert cells == runs == 15
    at = 0
    for esc in want:
        at = s.index(esc, at) + len(esc)


@pytest.mark.parametrize("mode", range(5))
def test_equal_colours_misses_black_hits_and_empty_slots(R, ctx, mode):
    W, H = 10, 2
    A, B, black = 0x41102030, 0x42102030, 0x43000000  # one colour under two glyphs; a black hit
    cur = np.array([A, B, A, 0, black, 0, NO, B, B, NO,
                    black, 0, 0, black, A, NO, NO, A, B, NO], dtype=np.uint32)
    prev = np.full(W * H, 0x44554433, dtype=np.uint32)
    prev[[6, 15, 16]] = 7
    prev.reshape(H, W)[:, W - 1] = NO
    s, cells, runs = check(R, ctx, mode, W, H, cur, prev)
    assert (cells, runs) == (15, 4)  # the empty slots are skipped and split their rows
    rec = lambda w: RD.record_of_word(mode, w)
    head = rec(A)
    assert s.startswith(RD.cup(0, 0) + head + b"B" + b"A")  # neighbours of one colour: glyphs alone
    ascii_mode = mode in (R.BIT_ASCII, R.RGB_ASCII)
    if ascii_mode:
        # a miss beside a black hit: the same colour digits under another selector -- whole records both ways
        assert rec(0) + rec(black) + rec(0) in s and RD.cup(1, 0) + rec(black) + rec(0) + b" " + rec(black) in s
    elif mode in (R.RGB_PIXEL, R.RGB_NORMALS):
        assert rec(0) + b"C" + b" " in s and RD.cup(1, 0) + rec(black) + b" " + b" " + b"C" in s
    # the cells left of an empty slot keep what they showed; replaying gives the current records everywhere else
    grid = RD.apply_delta(RD.records(mode, W, H, prev), s)
    now = RD.records(mode, W, H, cur)
    for r in range(H):
        for c in range(W - 1):
            if cur[r * W + c] != NO:
                assert grid[r][c] == now[r][c], (r, c)
            else:
                assert grid[r][c] == RD.record_of_word(mode, 7)


def test_equal_frames_leave_the_output_untouched(R, ctx):
    rng = np.random.default_rng(600)
    cur, _ = RD.random_frame_pair(rng, 37, 61, 1.0)
    assert run_delta(R, ctx, R.RGB_ASCII, 37, 61, cur, cur.copy()) == (b"", 0, 0)  # (run_delta checks the fill behind the stream: all of it)


def test_the_three_forms_give_the_same_bytes(R):
    rng = np.random.default_rng(700)
    with R.Context(64, 64) as c:
        before = c.get_option(R.STAT_MINIMIZE_FALLBACKS)
        for mode in (R.BIT_ASCII, R.RGB_PIXEL):
            cur, prev = RD.random_frame_pair(rng, 37, 61, 0.4)
            want = RD.delta_stream(mode, 37, 61, cur, prev)
            for form in (0, 1, 2):
                c.set_option(R.OPT_MINIMIZE_FUSED, form)
                assert run_delta(R, c, mode, 37, 61, cur, prev) == want, (mode, form)
        assert c.get_option(R.STAT_MINIMIZE_FALLBACKS) - before == 2  # one per launch of form 2


def test_refusals(R, ctx):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    for args, status in (((R.SDL, 4, 4, p, p, p, 4096), R.ERR_INVALID_MODE),
                         ((R.RGB_ASCII, 4, 4, p, p, p, R.delta_bound(R.RGB_ASCII, 4, 4) - 1), R.ERR_TOO_LARGE),
                         ((R.RGB_ASCII, 100001, 1, p, p, p, 1 << 40), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_ASCII, 1, 100000, p, p, p, 1 << 40), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_ASCII, 4, 4, p + 2, p, p, 4096), R.ERR_INVALID_ARGUMENT),
                         ((R.RGB_ASCII, 4, 4, p, p, p + 8, 4096), R.ERR_INVALID_ARGUMENT)):
        with pytest.raises(R.RtxError) as e:
            ctx.delta_words(*args)
        assert e.value.status == status, args


# ---- rtx_update_delta on a small scene, as one sequence

W0, H0 = 64, 40


def small_scene(R, c):
    p = R.camera_params(W0, H0)
    sph, pl = R.synth_scene(77, 40, 1, p.element1, p.element2)
    c.set_scene(sph, pl)
    for i in range(0, 40, 3):
        c.set_sphere_motion(i, 1 if i % 2 else -1, 3.0)


def frame_words(R, c, p, mode):
    """The frame's pixel words as rtx_render_rows stores them."""
    import torch
    W, H = int(p.x), int(p.y)
    t = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.render_rows(p, mode, 0, H, d_out=t.data_ptr(), flags=R.RENDER_COMPACT)
    c.synchronize()
    return t.cpu().numpy().view(np.uint32)


def key_stream(R, c, p, mode, words):
    """What rtx_update makes of these words: rtx_minimize_words."""
    import torch
    W, H = int(p.x), int(p.y)
    src = to_device(words)
    dst = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = c.minimize_words(mode, W, H, src.data_ptr(), dst.data_ptr())
    return bytes(dst.cpu().numpy()[:n])


def test_update_delta_as_one_sequence(R):
    mode = R.RGB_ASCII
    with R.Context(W0, H0) as c, R.Context(W0, H0) as twin:
        small_scene(R, c)
        small_scene(R, twin)
        p = R.camera_params(W0, H0)
        # the first call: a key frame, rtx_update's bytes
        s, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_KEY and bytes(s) == bytes(twin.update(p, mode)) and len(s) > 0
        words = frame_words(R, c, p, mode)
        grid = RD.records(mode, W0, H0, words)
        # rest: nothing
        s, kind = c.update_delta(p, mode)
        assert kind == R.DELTA_DIFF and len(s) == 0
        assert c.get_option(R.STAT_DELTA_CELLS) == 0 and c.get_option(R.STAT_DELTA_RUNS) == 0

        def step(p, mode, **kw):
            nonlocal grid, words
            s, kind = c.update_delta(p, mode, **kw)
            assert kind == R.DELTA_DIFF
            now = frame_words(R, c, p, mode)
            want, cells, runs = RD.delta_stream(mode, int(p.x), int(p.y), now, words)
            assert bytes(s) == want
            assert (c.get_option(R.STAT_DELTA_CELLS), c.get_option(R.STAT_DELTA_RUNS)) == (cells, runs)
            grid = RD.apply_delta(grid, bytes(s))
            assert grid == RD.records(mode, int(p.x), int(p.y), now)
            words = now
            return cells

        assert step(R.camera_params(W0, H0, (0.0, 0.0, 0.0), (0.0, 3.14159274 + 0.02, 0.0)), mode) > 0      # a camera step
        p = R.camera_params(W0, H0, (0.0, 0.0, 0.0), (0.0, 3.14159274 + 0.02, 0.0))
        assert step(p, mode, dt=0.25, run_physics=True) > 0                                                 # a physics step
        c.set_option(R.OPT_SHADOWS, 1)
        c.set_reflectivity(40, 0.6)                                                                         # the plane: a mirror
        assert step(p, mode) > 0
        frames, keys = c.get_option(R.STAT_DELTA_FRAMES), c.get_option(R.STAT_DELTA_KEYFRAMES)
        assert (frames, keys) == (5, 1)

        def expect_key(p, mode, **kw):
            nonlocal grid, words
            s, kind = c.update_delta(p, mode, **kw)
            assert kind == R.DELTA_KEY
            words = frame_words(R, c, p, mode)
            assert bytes(s) == key_stream(R, c, p, mode, words)
            grid = RD.records(mode, int(p.x), int(p.y), words)
            # and the frame after it is a delta against it: at rest, nothing
            s, kind = c.update_delta(p, mode)
            assert kind == R.DELTA_DIFF and len(s) == 0

        expect_key(p, mode, flags=R.DELTA_KEYFRAME)                 # the flag
        mode = R.BIT_PIXEL
        expect_key(p, mode)                                         # another mode
        p = R.camera_params(48, 30, (0.0, 0.0, 0.0), (0.0, 3.14159274 + 0.02, 0.0))
        expect_key(p, mode)                                         # another size
        assert len(c.update(p, mode)) > 0
        expect_key(p, mode)                                         # an rtx_update in between
        q = R.camera_params(48, 30, (0.0, 0.0, 0.0), (0.0, 3.14159274 - 0.3, 0.0))
        with pytest.raises(R.RtxError) as e:
            c.update_delta(q, mode, capacity=8)                     # a delta that does not fit the host buffer
        assert e.value.status == R.ERR_TOO_LARGE
        expect_key(q, mode)
        step(p, mode)                                               # and deltas go on from there
        assert c.get_option(R.STAT_DELTA_KEYFRAMES) == keys + 5
        for bad in (R.SDL, 6, -1):
            with pytest.raises(R.RtxError) as e:
                c.update_delta(p, bad)
            assert e.value.status == R.ERR_INVALID_MODE
        with pytest.raises(R.RtxError) as e:
            c.update_delta(p, mode, flags=2)
        assert e.value.status == R.ERR_INVALID_ARGUMENT


def test_a_group_of_three_ranks_gives_the_plain_bytes(R):
    mode = R.RGB_ASCII
    with R.Context(W0, H0) as c, R.Context(W0, H0, devices=[0, 0, 0]) as g:
        small_scene(R, c)
        small_scene(R, g)
        assert g.group_size == 3
        poses = [(0.0, 3.14159274), (0.0, 3.14159274), (0.0, 3.14159274 + 0.03), (0.05, 3.14159274 + 0.03)]
        for i, (pitch, yaw) in enumerate(poses):
            p = R.camera_params(W0, H0, (0.0, 0.0, 0.0), (pitch, yaw, 0.0))
            a, ka = c.update_delta(p, mode, dt=0.125, run_physics=i == 3)
            a = bytes(a)
            b, kb = g.update_delta(p, mode, dt=0.125, run_physics=i == 3)
            assert ka == kb == (R.DELTA_KEY if i == 0 else R.DELTA_DIFF) and a == bytes(b), i
            assert (len(a) == 0) == (i == 1)
