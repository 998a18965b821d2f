"""Delta frames of half-block streams (rtx_half_delta_words, rtx_update_half_delta; include/rtx.h) restated in plain Python over the
key / sgr / keys of tests/restate_half.py: the stream of two W x 2H frames of pixel words, its bound, and a terminal that replays a
stream over a grid of (T, B) -- one that FORGETS both colours at every cursor escape, so that a run which relies on SGR state from
before it fails.  No GPU, no library: self_test() (run by tests/test_host_half_delta.py) checks the restatement against itself, and
tests/test_gpu_half_delta.py checks the kernels against it byte for byte."""
import re

import restate_half as RH

MAX_INDEX = 99999
MAX_CUP = 14


def cup(row, col):
    return b"\x1b[%d;%dH" % (row + 1, col + 1)


def half_delta_stream(mode, W, H, cur, prev):
    """(stream, changed cells, runs) of the header's rule."""
    assert W >= 1 and H >= 1 and len(cur) == W * 2 * H and len(prev) == W * 2 * H
    now, before = RH.keys(mode, W, H, cur), RH.keys(mode, W, H, prev)
    out = bytearray()
    cells = runs = 0
    for r in range(H):
        for c in range(W - 1):
            if now[r][c] == before[r][c]:
                continue
            t, b = now[r][c]
            cells += 1
            if c == 0 or now[r][c - 1] == before[r][c - 1]:  # a run starts
                runs += 1
                out += cup(r, c) + RH.sgr(mode, "3", t) + RH.sgr(mode, "4", b)
            else:
                if t != now[r][c - 1][0]:
                    out += RH.sgr(mode, "3", t)
                if b != now[r][c - 1][1]:
                    out += RH.sgr(mode, "4", b)
            out += RH.GLYPH
    return bytes(out), cells, runs


# ---- the bound

def _digits(v):
    return len(str(v))


def cup_length(row, col):
    return 4 + _digits(row + 1) + _digits(col + 1)


def run_bound(C, cup_len, n):
    """The most bytes n consecutive cells can emit at C bytes a cell and cup_len a run: c cells in r runs with r <= c and
    c + r - 1 <= n, tried for every c."""
    return max([C * c + cup_len * min(c, n + 1 - c) for c in range(n + 1)])


def run_bound_closed(C, cup_len, n):
    """... as the library forms it: at the bend (n + 1) // 2, one behind it, or at c = n."""
    value = lambda c: 0 if c > n else C * c + cup_len * min(c, n + 1 - c)
    return max(value((n + 1) // 2), value((n + 1) // 2 + 1), value(n))


def half_delta_bound(mode, W, H):
    """rtx_half_delta_bound: the rows' sums -- a row's W-1 cells under the longest cursor escape the row can need -- or the key
    frame's half_bound, whichever is larger; 0 for what the calls refuse."""
    if mode not in (RH.BIT_ASCII, RH.BIT_PIXEL, RH.RGB_ASCII, RH.RGB_PIXEL, RH.RGB_NORMALS):
        return 0
    if W < 1 or H < 1 or W - 1 > MAX_INDEX or H > MAX_INDEX:
        return 0
    C = 2 * (19 if RH.is_rgb(mode) else 11) + 3
    total = 0
    if W >= 2:
        lo, hi = 0, 9
        while lo < H:  # rows lo .. hi - 1 share the digits of lo + 1
            total += (min(hi, H) - lo) * run_bound_closed(C, cup_length(lo, W - 2), W - 1)
            lo, hi = hi, hi * 10 + 9
    return max(total, RH.half_bound(mode, W, H))


def block_bound(mode, slots=1024):
    C = 2 * (19 if RH.is_rgb(mode) else 11) + 3
    return run_bound_closed(C, MAX_CUP, slots)


# ---- the replaying terminal

_CUP = re.compile(rb"\x1b\[([1-9]\d*);([1-9]\d*)H")
_SGR_RGB = re.compile(rb"\x1b\[([34])8;2;(0|[1-9]\d{0,2});(0|[1-9]\d{0,2});(0|[1-9]\d{0,2})m")
_SGR_8 = re.compile(rb"\x1b\[([34])8;5;(0|[1-9]\d{0,2})m")


def apply_half_delta(mode, grid, stream):
    """Replays `stream` over `grid` (H rows of W-1 pairs (T, B), changed in place and returned).  A cursor escape moves the cursor
    AND forgets both colours; a glyph under a forgotten colour, before any cursor escape or outside the grid raises ValueError, and
    so does anything that is neither a cursor escape, an escape of the mode's family nor the glyph."""
    rgb = RH.is_rgb(mode)
    row = col = fg = bg = None
    at = 0
    while at < len(stream):
        m = _CUP.match(stream, at)
        if m:
            row, col, fg, bg = int(m.group(1)) - 1, int(m.group(2)) - 1, None, None
            at = m.end()
            continue
        m = (_SGR_RGB if rgb else _SGR_8).match(stream, at)
        if m:
            comps = [int(v) for v in m.groups()[1:]]
            if max(comps) > 255:
                raise ValueError("byte %d: component above 255" % at)
            k = comps[0] | (comps[1] << 8) | (comps[2] << 16) if rgb else comps[0]
            if m.group(1) == b"3":
                fg = k
            else:
                bg = k
            at = m.end()
            continue
        if stream.startswith(RH.GLYPH, at):
            if row is None:
                raise ValueError("byte %d: a glyph before any cursor escape" % at)
            if fg is None or bg is None:
                raise ValueError("byte %d: a glyph under a colour the run did not set" % at)
            if not (0 <= row < len(grid) and 0 <= col < len(grid[row])):
                raise ValueError("byte %d: a glyph at (%d, %d), outside the grid" % (at, row, col))
            grid[row][col] = (fg, bg)
            col += 1
            at += 3
            continue
        raise ValueError("byte %d: %r is neither an escape nor the glyph" % (at, stream[at:at + 4]))
    return grid


# ---- frame pairs (numpy is needed from here on)

def frame_pairs(rng, W, H, density):
    """(name, cur, prev) for each word population of restate_half.populations: prev is one draw of the population, cur takes another
    draw's words in the cells picked with probability `density` (top and bottom picked apart) and prev's elsewhere."""
    import numpy as np
    out = []
    for (name, prev), (_, other) in zip(RH.populations(rng, W, H), RH.populations(rng, W, H)):
        cur = np.where(rng.random(prev.size) < density, other, prev).astype(np.uint32)
        cur.reshape(2 * H, W)[:, W - 1] = RH.NO
        out.append((name, cur, prev))
    return out


def self_test(seed=20240917):
    import numpy as np
    rng = np.random.default_rng(seed)
    for mode in (RH.BIT_ASCII, RH.BIT_PIXEL, RH.RGB_PIXEL, RH.RGB_NORMALS):
        for (W, H) in ((1, 3), (2, 4), (7, 2), (23, 9), (120, 11), (12, 101)):
            for density in (0.0, 0.02, 0.5, 1.0):
                for name, cur, prev in frame_pairs(rng, W, H, density):
                    what = (mode, W, H, density, name)
                    stream, cells, runs = half_delta_stream(mode, W, H, cur, prev)
                    assert apply_half_delta(mode, RH.keys(mode, W, H, prev), stream) == RH.keys(mode, W, H, cur), what
                    assert runs <= cells and len(_CUP.findall(stream)) == runs and stream.count(RH.GLYPH) == cells, what
                    assert len(stream) <= half_delta_bound(mode, W, H), what
                    assert density != 0.0 or (stream == b"" and cells == 0), what
    # the closed form of a row's bound is the maximum over every count of changed cells
    for C in (25, 41):
        for cup_len in range(6, 15):
            for n in range(0, 60):
                assert run_bound(C, cup_len, n) == run_bound_closed(C, cup_len, n), (C, cup_len, n)
    assert block_bound(RH.RGB_PIXEL) == 41998 and block_bound(RH.BIT_PIXEL) == 25614
    assert half_delta_bound(RH.RGB_PIXEL, 160, 50) == 326391 and half_delta_bound(RH.BIT_PIXEL, 160, 50) == 199191
    # what is no change: a glyph, 0 against 0xffffffff, the 8-bit family's 0 against byte 0 = 16
    a = np.array([0x41102030, 0, 0, RH.NO, 0x42000010, 0x41000011, 0, RH.NO], dtype=np.uint32)
    b = np.array([0x5A102030, RH.NO, 0x43000010, RH.NO, 0, 0x41000011, 0x44000010, RH.NO], dtype=np.uint32)
    assert half_delta_stream(RH.BIT_PIXEL, 4, 1, a, b) == (b"", 0, 0)
    assert half_delta_stream(RH.RGB_PIXEL, 4, 1, a, b)[1:] == (2, 2)  # (the RGB family sees 0 against 0x000010 in cells 0 and 2)
    # a terminal that forgets its colours refuses a run that sets only one of them
    try:
        apply_half_delta(RH.RGB_PIXEL, [[(0, 0)]], cup(0, 0) + RH.sgr(RH.RGB_PIXEL, "3", 5) + RH.GLYPH)
    except ValueError:
        pass
    else:
        raise AssertionError("a run without its background escape was accepted")
    return True
