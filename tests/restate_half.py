"""Half-block frames (rtx_half_words, rtx_update_half; include/rtx.h) restated in plain Python: the colour key of a pixel word, the
SGR escapes, the stream of a W x H console over W x 2H pixel words, its bound, and a small terminal that turns a stream back into
the grid of (T, B) it shows.  No GPU, no library: what tests/test_host_half.py checks against itself and tests/test_gpu_half.py
checks the kernels against."""
BIT_ASCII, BIT_PIXEL, RGB_ASCII, RGB_PIXEL, RGB_NORMALS, SDL = range(6)
NO = 0xFFFFFFFF
GLYPH = b"\xe2\x96\x80"  # U+2580, the upper half block


def is_rgb(mode):
    if mode not in (BIT_ASCII, BIT_PIXEL, RGB_ASCII, RGB_PIXEL, RGB_NORMALS):
        raise ValueError("no half-block frames in mode %r" % (mode,))
    return mode >= RGB_ASCII


def key(mode, w):
    """K(w) of a cell's word: 0xffffffff counts as 0; the 8-bit family takes byte 0 (16 for a miss), the RGB family bytes 0..2."""
    w = int(w)
    if w == NO:
        w = 0
    if is_rgb(mode):
        return w & 0xFFFFFF
    return (w & 0xFF) if w != 0 else 16


def sgr(mode, sel, k):
    """SGR(sel, K): sel is '3' (foreground) or '4' (background)."""
    assert sel in ("3", "4")
    if is_rgb(mode):
        return ("\x1b[%s8;2;%d;%d;%dm" % (sel, k & 255, (k >> 8) & 255, (k >> 16) & 255)).encode()
    return ("\x1b[%s8;5;%dm" % (sel, k)).encode()


def keys(mode, W, H, words):
    """The grid the stream must show: H rows of W-1 pairs (T, B)."""
    assert len(words) == W * 2 * H
    return [[(key(mode, words[2 * r * W + c]), key(mode, words[(2 * r + 1) * W + c])) for c in range(W - 1)] for r in range(H)]


def half_stream(mode, W, H, words):
    assert W >= 1 and H >= 1 and len(words) == W * 2 * H
    out = bytearray()
    prev = None
    for r in range(H):
        for c in range(W - 1):
            t, b = key(mode, words[2 * r * W + c]), key(mode, words[(2 * r + 1) * W + c])
            if prev is None or prev[0] != t:
                out += sgr(mode, "3", t)
            if prev is None or prev[1] != b:
                out += sgr(mode, "4", b)
            out += GLYPH
            prev = (t, b)
        out += b"\n"
    return bytes(out)


def half_bound(mode, W, H):
    E = 19 if is_rgb(mode) else 11
    return H * ((W - 1) * (2 * E + 3) + 1)


def _number(stream, at, what):
    """A decimal without leading zeros at stream[at:]: (value, the position behind it)."""
    end = at
    while end < len(stream) and 0x30 <= stream[end] <= 0x39:
        end += 1
    if end == at or (end - at > 1 and stream[at] == 0x30) or end - at > 3:
        raise ValueError("byte %d: %s is no decimal without leading zeros" % (at, what))
    return int(stream[at:end]), end


def _expect(stream, at, byte):
    if at >= len(stream) or stream[at] != byte:
        raise ValueError("byte %d: expected %r" % (at, bytes([byte])))
    return at + 1


def replay(mode, stream, W, H):
    """A terminal that keeps the SGR foreground and background state, fed `stream` from the home position: the H x (W-1) grid of
    (T, B) it shows.  Anything that is not a well-formed escape of the mode's family, the glyph or a newline raises ValueError, and
    so does a glyph under an unset colour, a row of another length and a stream of another number of rows."""
    rgb = is_rgb(mode)
    fg = bg = None
    grid, row = [], []
    at = 0
    while at < len(stream):
        if stream[at] == 0x0A:
            if len(row) != W - 1:
                raise ValueError("byte %d: a row of %d cells" % (at, len(row)))
            grid.append(row)
            row = []
            at += 1
        elif stream.startswith(GLYPH, at):
            if fg is None or bg is None:
                raise ValueError("byte %d: a glyph under an unset colour" % at)
            row.append((fg, bg))
            at += 3
        elif stream[at] == 0x1B:
            start = at
            at = _expect(stream, at + 1, 0x5B)
            if at >= len(stream) or stream[at] not in (0x33, 0x34):
                raise ValueError("byte %d: the selector is neither 3 nor 4" % at)
            sel = stream[at]
            at = _expect(stream, at + 1, 0x38)
            at = _expect(stream, at, 0x3B)
            at = _expect(stream, at, 0x32 if rgb else 0x35)
            comps = []
            for _ in range(3 if rgb else 1):
                at = _expect(stream, at, 0x3B)
                v, at = _number(stream, at, "a colour component")
                if v > 255:
                    raise ValueError("byte %d: component %d" % (at, v))
                comps.append(v)
            at = _expect(stream, at, 0x6D)
            k = comps[0] | (comps[1] << 8) | (comps[2] << 16) if rgb else comps[0]
            assert stream[start:at] == sgr(mode, chr(sel), k)
            if sel == 0x33:
                fg = k
            else:
                bg = k
        else:
            raise ValueError("byte %d: %r is neither an escape, the glyph nor a newline" % (at, stream[at:at + 4]))
    if row or len(grid) != H:
        raise ValueError("%d rows and %d cells behind the last newline" % (len(grid), len(row)))
    return grid


# ---- word populations (numpy is needed from here on)

def populations(rng, W, H):
    """The word populations of the issue for a W x 2H frame, as (name, uint32 array) pairs: the last column is 0xffffffff."""
    import numpy as np
    n = W * 2 * H

    def finish(a):
        a = np.asarray(a, dtype=np.uint32).copy()
        a.reshape(2 * H, W)[:, W - 1] = NO
        return a

    glyphs = rng.integers(32, 127, size=n, dtype=np.uint32) << np.uint32(24)
    palette = np.array([0x00102030, 0x000A64FF, 0x00000000], dtype=np.uint32)
    runs = np.repeat(palette[rng.integers(0, 3, size=n // 5 + 1)], rng.integers(1, 12, size=n // 5 + 1))
    runs = np.resize(runs, n)
    # (the rows of a pair drawn apart, so that a cell's top and bottom run out at different columns)
    rand = rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
    sprinkled = np.where(rng.random(n) < 0.1, np.uint32(NO), np.where(rng.random(n) < 0.5, rand, np.uint32(0x00102030)))
    digit_choices = np.array([0, 5, 9, 10, 42, 99, 100, 177, 255], dtype=np.uint32)
    pick = lambda: digit_choices[rng.integers(0, digit_choices.size, size=n)]
    digits = pick() | (pick() << np.uint32(8)) | (pick() << np.uint32(16))
    return [("palette", finish(runs | glyphs)), ("random", finish(rand | glyphs)), ("zeros", finish(np.zeros(n, dtype=np.uint32))),
            ("sprinkled", finish(sprinkled)), ("digits", finish(digits | glyphs))]
