"""RayTracingManager::SetHalfDeltaFrames (include/rtx_compat.hpp) on the GPU: tests/host/compat_half_delta.cpp, host C++ over the C
ABI with the printer thread on a pipe, built once and run once per scenario.  Three frames through the facade: the first stands
behind a cursor home, the later ones carry none, and replaying every byte the printer wrote as a terminal would gives the (T, B)
grid of the last frame.  SetHalfBlocks(true) with SetDeltaFrames(true) alone still sends whole frames."""
import os
import re
import subprocess

import pytest

import restate_half as RH
import restate_half_delta as RD
import util as U

pytestmark = pytest.mark.gpu

W, H = 48, 20
MODE = RH.RGB_PIXEL
HOME, RESET = b"\x1b[H", b"\x1b[m"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    R = U.pkg()
    out = str(tmp_path_factory.mktemp("compat_half_delta") / "compat_half_delta")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(U.ROOT, "include"),
                           os.path.join(U.ROOT, "tests", "host", "compat_half_delta.cpp"), "-o", out, "-L", R.PKG_DIR, "-lrtx_hip", "-pthread",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def run(exe, tmp_path, scenario):
    p = subprocess.run([exe, str(tmp_path), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "facade half-block delta ok" in p.stdout, p.stdout[-4000:]
    read = lambda name: open(os.path.join(str(tmp_path), name), "rb").read()
    params = U.pkg().Params.from_buffer_copy(read("params.bin"))
    assert (int(params.x), int(params.y)) == (W, H)
    return p.stdout, read("stream.bin"), (read("last.bin") if scenario != "unprepared" else b""), params


_CUP = re.compile(rb"\x1b\[([1-9]\d*);([1-9]\d*)H")
_SGR = re.compile(rb"\x1b\[([34])8;2;(\d{1,3});(\d{1,3});(\d{1,3})m")


def terminal(stream):
    """What a terminal of W-1 x H cells shows after `stream`: the printer's cursor homes and attribute resets, whole half-block frames
    with their newlines, and deltas with their cursor escapes.  Colours are forgotten at every cursor movement by escape and at
    every reset, so a glyph shows only what its own run or frame has set."""
    grid = [[None] * (W - 1) for _ in range(H)]
    row = col = 0
    fg = bg = None
    at = 0
    while at < len(stream):
        if stream.startswith(HOME, at):
            row, col, fg, bg, at = 0, 0, None, None, at + 3
        elif stream.startswith(RESET, at):
            fg, bg, at = None, None, at + 3
        elif stream[at] == 0x0A:
            row, col, at = row + 1, 0, at + 1
        elif stream.startswith(RH.GLYPH, at):
            assert fg is not None and bg is not None and row < H and col < W - 1, at
            grid[row][col] = (fg, bg)
            col, at = col + 1, at + 3
        else:
            m = _CUP.match(stream, at)
            if m:
                row, col, fg, bg, at = int(m.group(1)) - 1, int(m.group(2)) - 1, None, None, m.end()
                continue
            m = _SGR.match(stream, at)
            assert m, (at, stream[at:at + 8])
            k = int(m.group(2)) | (int(m.group(3)) << 8) | (int(m.group(4)) << 16)
            if m.group(1) == b"3":
                fg = k
            else:
                bg = k
            at = m.end()
    return grid


def test_half_block_deltas_reach_the_printer(exe, tmp_path):
    R = U.pkg()
    out, stream, last, p = run(exe, tmp_path, "on")
    assert "half 0 half-delta 3 keys 1 delta 0" in out
    # one frame per hand-off, each closed by the printer's reset: the first behind a cursor home, the later ones without
    pieces = stream.split(RESET)
    assert len(pieces) == 4 and pieces[3] == b""
    assert pieces[0].startswith(HOME) and stream.count(HOME) == 1
    key = pieces[0][3:]
    assert key.count(b"\n") == H and RH.replay(MODE, key, W, H)  # a whole half-block frame
    for piece in pieces[1:3]:
        assert 0 < len(piece) < len(key) and b"\n" not in piece and _CUP.match(piece)  # runs behind cursor escapes: the camera turned
        assert len(piece) <= R.half_delta_bound(MODE, W, H)
    # replayed, the whole stream shows the last frame
    want = RH.replay(MODE, last, W, H)
    assert terminal(stream) == want
    # ... and each delta is the rule's: over the grid before it, it gives the grid after it
    grid = RH.replay(MODE, key, W, H)
    for piece in pieces[1:3]:
        grid = RD.apply_half_delta(MODE, grid, piece)
    assert grid == want
    hits = sum(1 for row in want for (t_, b_) in row if t_ or b_)
    assert hits >= 20 and (W - 1) * H - hits >= 20
    assert len(last) <= R.half_bound(MODE, W, H)


def test_half_blocks_with_delta_frames_alone_still_send_whole_frames(exe, tmp_path):
    out, stream, last, p = run(exe, tmp_path, "whole")
    assert "half 3 half-delta 0 keys 0 delta 0" in out
    pieces = stream.split(RESET)
    assert len(pieces) == 4 and pieces[3] == b"" and stream.count(HOME) == 3
    for piece in pieces[:3]:
        assert piece.startswith(HOME) and piece.count(b"\n") == H and not _CUP.search(piece)
        RH.replay(MODE, piece[3:], W, H)
    assert pieces[2][3:] == last and terminal(stream) == RH.replay(MODE, last, W, H)


def test_switching_on_without_the_printer_prepared_throws(exe, tmp_path):
    out, stream, last, p = run(exe, tmp_path, "unprepared")
    assert "half 0 half-delta 0 keys 0 delta 0" in out and stream == b""
