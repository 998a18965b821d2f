"""Delta frames (rtx_delta_words, rtx_update_delta; include/rtx.h) restated in plain Python, from the header's rule and the record
layouts of SURVEY.md App. B alone: the record of a pixel word, the delta stream of two frames of words, and a decoder that replays
a stream over a grid of records as a terminal would.  tests/test_gpu_delta.py ties record_of_word to rtx_expand and checks the
product against delta_stream byte for byte; self_test() (run by tests/test_host_delta.py) checks the restatement against itself:
replaying a delta over the previous frame's records gives the current frame's."""
import re

import numpy as np

BIT_ASCII, BIT_PIXEL, RGB_ASCII, RGB_PIXEL, RGB_NORMALS = range(5)
NO_WORD = 0xFFFFFFFF
MAX_INDEX = 99999


def record_size(mode):
    return 20 if mode >= RGB_ASCII else 12


def _digits(v):
    """Three decimal digits, absent leading ones NUL (RayTracing.cu:212-229)."""
    return bytes([48 + v // 100 if v >= 100 else 0, 48 + (v // 10) % 10 if v >= 10 else 0, 48 + v % 10])


def record_of_word(mode, w):
    """The S bytes rtx_expand writes for pixel word w: 0xffffffff is an empty slot (all NUL), 0 a pixel without a hit."""
    w = int(w)
    S = record_size(mode)
    if w == NO_WORD:
        return bytes(S)
    hit = w != 0
    kind = b"3" if hit and mode in (BIT_ASCII, RGB_ASCII) else b"4"
    glyph = bytes([w >> 24]) if hit else b" "
    if S == 20:
        r, g, b = (w & 255, (w >> 8) & 255, (w >> 16) & 255) if hit else (0, 0, 0)
        return b"\x1b[" + kind + b"8;2;" + _digits(r) + b";" + _digits(g) + b";" + _digits(b) + b"m" + glyph
    return b"\x1b[" + kind + b"8;5;" + _digits((w & 255) if hit else 16) + b"m" + glyph


def records(mode, W, H, words):
    """The H x (W-1) grid of records of a frame of words (column W-1 is no cell)."""
    words = np.asarray(words, dtype=np.uint32).reshape(H, W)
    return [[record_of_word(mode, words[r, c]) for c in range(W - 1)] for r in range(H)]


def cup(row, col):
    return b"\x1b[%d;%dH" % (row + 1, col + 1)


def delta_stream(mode, W, H, cur, prev):
    """(stream, changed cells, runs) of the header's rule."""
    cur = np.asarray(cur, dtype=np.uint32).reshape(H, W)
    prev = np.asarray(prev, dtype=np.uint32).reshape(H, W)
    out = bytearray()
    cells = runs = 0
    for row in range(H):
        left_changed = False
        left = None
        for col in range(W - 1):
            w = int(cur[row, col])
            changed = w != int(prev[row, col]) and w != NO_WORD
            if changed:
                rec = record_of_word(mode, w)
                cells += 1
                if not left_changed:
                    runs += 1
                    out += cup(row, col) + rec
                elif rec[:-1] != left[:-1]:
                    out += rec
                else:
                    out += rec[-1:]
                left = rec
            left_changed = changed
    return bytes(out), cells, runs


_CUP = re.compile(rb"\x1b\[(\d+);(\d+)H")


def apply_delta(grid, stream):
    """Replays `stream` over `grid` (H rows of W-1 records, changed in place and returned): a cursor escape moves the cursor (a
    record's NUL digits and third ';' never match it), a byte ESC starts a whole record, any other byte is a glyph under the head
    of the record to its left; every cell written moves the cursor one column on."""
    S = len(grid[0][0]) if grid and grid[0] else 0
    row = col = None
    at = 0
    while at < len(stream):
        m = _CUP.match(stream, at)
        if m:
            row, col = int(m.group(1)) - 1, int(m.group(2)) - 1
            at = m.end()
            continue
        assert row is not None, "a cell before any cursor escape"
        if stream[at] == 0x1B:
            rec = stream[at:at + S]
            assert len(rec) == S, "a record cut short"
            at += S
        else:
            assert col > 0, "a glyph alone in column 0"
            rec = grid[row][col - 1][:-1] + stream[at:at + 1]
            at += 1
        grid[row][col] = rec
        col += 1
    return grid


def random_frame_pair(rng, W, H, density, holes=0.0, colours=6):
    """Two frames of words with printable glyphs from a small palette (so that heads repeat), misses included; a cell differs with
    probability about `density`; column W-1 is 0xffffffff as the trace kernels leave it."""
    n = W * H
    palette = rng.integers(0, 1 << 24, size=colours, dtype=np.uint32)

    def frame():
        w = (rng.integers(33, 127, size=n, dtype=np.uint32) << np.uint32(24)) | palette[rng.integers(0, colours, size=n)]
        w[rng.random(n) < 0.2] = 0
        return w

    prev = frame()
    cur = np.where(rng.random(n) < density, frame(), prev).astype(np.uint32)
    if holes:
        cur[rng.random(n) < holes] = NO_WORD
        prev[rng.random(n) < holes] = NO_WORD
    for a in (prev, cur):
        a.reshape(H, W)[:, W - 1] = NO_WORD
    return cur, prev


def self_test(seed=20240611):
    rng = np.random.default_rng(seed)
    for mode in range(5):
        for (W, H) in ((1, 3), (2, 4), (7, 2), (23, 9), (120, 11)):
            for density in (0.0, 0.05, 0.5, 1.0):
                cur, prev = random_frame_pair(rng, W, H, density)
                stream, cells, runs = delta_stream(mode, W, H, cur, prev)
                assert apply_delta(records(mode, W, H, prev), stream) == records(mode, W, H, cur), (mode, W, H, density)
                assert runs <= cells and (density != 0.0 or (stream == b"" and cells == 0))
                assert len(_CUP.findall(stream)) == runs
    return True
