"""Half-block frames without a GPU: the Python restatement of the rule (tests/restate_half.py) against known answers, against its own
replay and against its bound; and rtxplan::half_bound / half_block_bound (csrc/rtx_plan.hpp) against brute force and overflow --
tests/host/test_half.cpp, compiled as host-only C++ and run under AddressSanitizer + UndefinedBehaviorSanitizer with the g++ line of
tests/test_host_delta.py."""
import os
import subprocess

import numpy as np
import pytest

import restate_half as RH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = RH.NO


def test_half_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_half")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_half.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all half-block planning tests passed" in p.stdout, p.stdout[-4000:]


def test_known_answers():
    words = [0x200A64FF, 0x200A64FF, NO, 0, 0, NO]
    assert RH.half_stream(RH.RGB_PIXEL, 3, 1, words) == b"\x1b[38;2;255;100;10m\x1b[48;2;0;0;0m\xe2\x96\x80\xe2\x96\x80\n"
    # an 8-bit miss is colour 16; a hit carries its index in byte 0
    assert RH.key(RH.BIT_PIXEL, 0) == 16 and RH.key(RH.BIT_PIXEL, 0x200A64FF) == 255 and RH.key(RH.BIT_ASCII, 0x41000000) == 0
    assert RH.half_stream(RH.BIT_PIXEL, 2, 1, [0, NO, 0x200000C4, NO]) == b"\x1b[38;5;16m\x1b[48;5;196m\xe2\x96\x80\n"
    # 0xffffffff outside the last column behaves as 0, in both families
    for mode in (RH.BIT_PIXEL, RH.RGB_PIXEL, RH.RGB_ASCII):
        assert RH.key(mode, NO) == RH.key(mode, 0)
        assert RH.half_stream(mode, 3, 2, [NO, 7, NO, 9, NO, NO] * 2) == RH.half_stream(mode, 3, 2, [0, 7, NO, 9, 0, NO] * 2)
    # the glyph byte is ignored; the family alone decides
    a = [0x41112233, 0x42112233, NO, 0x43445566, 0x20445566, NO]
    assert RH.half_stream(RH.RGB_ASCII, 3, 1, a) == RH.half_stream(RH.RGB_PIXEL, 3, 1, a) == RH.half_stream(RH.RGB_NORMALS, 3, 1, a)
    assert RH.half_stream(RH.RGB_ASCII, 3, 1, a) == b"\x1b[38;2;51;34;17m\x1b[48;2;102;85;68m" + RH.GLYPH * 2 + b"\n"
    assert RH.half_stream(RH.BIT_ASCII, 3, 1, a) == RH.half_stream(RH.BIT_PIXEL, 3, 1, a) == b"\x1b[38;5;51m\x1b[48;5;102m" + RH.GLYPH * 2 + b"\n"
    # the previous cell of column 0 is the last cell of the row above: one escape alone where one half changes
    b = [5, NO, 6, NO, 5, NO, 7, NO]
    assert RH.half_stream(RH.BIT_PIXEL, 2, 2, b) == b"\x1b[38;5;5m\x1b[48;5;6m" + RH.GLYPH + b"\n\x1b[48;5;7m" + RH.GLYPH + b"\n"
    assert RH.half_stream(RH.RGB_PIXEL, 1, 3, [1, 2, 3, 4, 5, 6]) == b"\n\n\n"
    for bad in (RH.SDL, 6, -1):
        with pytest.raises(ValueError):
            RH.half_stream(bad, 2, 1, [0, NO, 0, NO])


@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL, RH.BIT_ASCII, RH.RGB_NORMALS])
def test_replaying_the_stream_shows_the_keys(mode):
    rng = np.random.default_rng(900 + mode)
    for (W, H) in ((1, 3), (2, 1), (2, 5), (3, 1), (7, 4), (33, 9)):
        for name, words in RH.populations(rng, W, H):
            s = RH.half_stream(mode, W, H, words)
            assert RH.replay(mode, s, W, H) == RH.keys(mode, W, H, words), (W, H, name)
            assert len(s) <= RH.half_bound(mode, W, H), (W, H, name)


def test_the_replay_rejects_what_is_not_a_stream():
    mode = RH.RGB_PIXEL
    good = RH.half_stream(mode, 3, 1, [0x200A64FF, 0x200A64FF, NO, 0, 1, NO])
    assert RH.replay(mode, good, 3, 1) == [[(0x0A64FF, 0), (0x0A64FF, 1)]]
    for bad in (good[:-1],                                   # no newline
                good + b"\n",                                # a row too many
                good.replace(b"255", b"256"),                # a component out of range
                good.replace(b";100;", b";0100;"),           # leading zeros
                good.replace(b"[38", b"[58"),                # another selector
                good.replace(b"m\xe2", b"M\xe2"),            # another final byte
                good.replace(b"\xe2\x96\x80", b" ", 1),      # another glyph
                good.replace(b"48;2;0;0;0", b"48;5;0"),      # the other family's escape
                good[18:],                                 # a glyph before the foreground is set
                good.replace(b"\n", b"\x1b[H\n")):           # another escape
        with pytest.raises(ValueError):
            RH.replay(mode, bad, 3, 1)
    with pytest.raises(ValueError):
        RH.replay(RH.BIT_PIXEL, good, 3, 1)


@pytest.mark.parametrize("mode", [RH.BIT_PIXEL, RH.RGB_PIXEL])
def test_the_bound_is_met_exactly(mode):
    # neighbouring cells differ in both halves, every component has three digits
    W, H = 6, 3
    words = np.zeros((2 * H, W), dtype=np.uint32)
    for r in range(2 * H):
        for c in range(W - 1):
            v = 100 + ((r * 7 + c * 3) % 150)  # (differs from the cell before it in the row, and from the row above's last)
            words[r, c] = v | ((v + 1) << 8) | ((v + 2) << 16)
        words[r, W - 1] = NO
    grid = RH.keys(mode, W, H, words.reshape(-1))
    cells = [cell for row in grid for cell in row]
    assert all(a[0] != b[0] and a[1] != b[1] for a, b in zip(cells, cells[1:]))
    s = RH.half_stream(mode, W, H, words.reshape(-1))
    assert len(s) == RH.half_bound(mode, W, H) == H * ((W - 1) * (41 if mode == RH.RGB_PIXEL else 25) + 1)
    assert RH.replay(mode, s, W, H) == grid
