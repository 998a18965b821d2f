"""RayTracingManager::SetDeltaFrames and PrintMachine's delta hand-off (include/rtx_compat.hpp) on the GPU: tests/host/compat_delta.cpp,
host C++ over the C ABI with the printer thread on a pipe, built once and run once per scenario.  What the printer wrote is decoded
here as a terminal would read it and must give the records of the last frame; with delta frames off the byte stream is the one the
facade wrote before it knew about them."""
import os
import re
import subprocess

import numpy as np
import pytest

import restate_delta as RD
import util as U

pytestmark = pytest.mark.gpu

W, H, S = 48, 20, 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    R = U.pkg()
    out = str(tmp_path_factory.mktemp("compat_delta") / "compat_delta")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(U.ROOT, "include"),
                           os.path.join(U.ROOT, "tests", "host", "compat_delta.cpp"), "-o", out, "-L", R.PKG_DIR, "-lrtx_hip", "-pthread",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def run(exe, tmp_path, scenario):
    p = subprocess.run([exe, str(tmp_path), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "facade delta ok" in p.stdout, p.stdout[-4000:]
    return p.stdout, open(os.path.join(str(tmp_path), "stream.bin"), "rb").read()


def screen_after(stream, status_rows=0):
    """The H x (W-1) grid of records a terminal shows after `stream`: ESC [ H homes, ESC [ r ; c H moves, a byte ESC starts a record
    (never `ESC [ m`, the colour reset, which is skipped), a newline goes to the next row, any other byte is a glyph under the
    colour of the last whole record.  Returns (grid, homes, cursor escapes).  Rows from H on (the status lines) are dropped."""
    grid = [[None] * (W - 1) for _ in range(H + status_rows)]
    row = col = homes = moves = at = 0
    head = None
    while at < len(stream):
        if stream.startswith(b"\x1b[H", at):
            row = col = 0
            homes += 1
            at += 3
        elif stream.startswith(b"\x1b[m", at):
            head = None
            at += 3
        elif RD._CUP.match(stream, at):
            m = RD._CUP.match(stream, at)
            row, col = int(m.group(1)) - 1, int(m.group(2)) - 1
            moves += 1
            at = m.end()
        elif stream[at] == 0x0A:
            row, col = row + 1, 0
            at += 1
        elif stream[at] == 0x1B:
            rec = stream[at:at + S]
            head = rec[:-1]
            grid[row][col] = rec
            col += 1
            at += S
        else:
            if row < H:
                assert head is not None, "a glyph without a colour at byte %d" % at
                grid[row][col] = head + stream[at:at + 1]
            col += 1
            at += 1
    return grid[:H], homes, moves


def last_frame(tmp_path):
    rec = np.fromfile(os.path.join(str(tmp_path), "frame.bin"), dtype=np.uint8).reshape(H, W, S)
    return [[bytes(rec[r, c]) for c in range(W - 1)] for r in range(H)]


def test_lock_step_deltas_give_the_last_frame(exe, tmp_path):
    out, stream = run(exe, tmp_path, "lockstep")
    assert "frames 4 keys 1" in out
    grid, homes, moves = screen_after(stream)
    assert homes == 1 and moves > 0  # the cursor is homed in front of the key frame alone
    assert grid == last_frame(tmp_path)


def test_deltas_appended_before_the_printer_takes_them(exe, tmp_path):
    out, stream = run(exe, tmp_path, "appended")
    assert "frames 4 keys 1" in out
    grid, homes, moves = screen_after(stream)
    assert homes == 1 and moves > 0 and stream.count(b"\x1b[m") == 1  # one write: the key frame and the deltas behind it
    assert grid == last_frame(tmp_path)


def test_status_lines_are_addressed_in_delta_mode(exe, tmp_path):
    out, stream = run(exe, tmp_path, "status")
    line = b"\x1b[%d;1H\x1b[mRendering FPS: " % (H + 1)
    assert stream.count(line) == 4 and stream.count(b"\x1b[H") == 1
    grid, _, _ = screen_after(re.sub(rb"Rendering FPS: \d+    \nPrinting FPS: \d+    \n", b"", stream))
    assert grid == last_frame(tmp_path)


def test_without_delta_frames_the_stream_is_what_it_was(exe, tmp_path):
    _, stream = run(exe, tmp_path, "off")
    want = open(os.path.join(str(tmp_path), "expected.bin"), "rb").read()
    assert len(want) > 4 * 1000 and stream == want
    assert RD._CUP.search(stream) is None and stream.count(b"\x1b[H") == 4
