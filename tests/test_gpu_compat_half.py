"""RayTracingManager::SetHalfBlocks (include/rtx_compat.hpp) on the GPU: tests/host/compat_half.cpp, host C++ over the C ABI with the
printer thread on a pipe, built once and run once per scenario.  With PrintMachine::Start(W, H, true) and SetHalfBlocks(true) what the
printer wrote is rtx_update_half's stream for that frame -- replayed as a terminal would read it, the keys of the sample frame's
pixel words (tests/restate_half.py); with the call never made the stream is rtx_update's, as it is today."""
import os
import subprocess

import numpy as np
import pytest

import restate_half as RH
import util as U

pytestmark = pytest.mark.gpu

W, H = 48, 20
MODE = RH.RGB_PIXEL


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    R = U.pkg()
    out = str(tmp_path_factory.mktemp("compat_half") / "compat_half")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(U.ROOT, "include"),
                           os.path.join(U.ROOT, "tests", "host", "compat_half.cpp"), "-o", out, "-L", R.PKG_DIR, "-lrtx_hip", "-pthread",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def run(exe, tmp_path, scenario):
    p = subprocess.run([exe, str(tmp_path), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "facade half blocks ok" in p.stdout, p.stdout[-4000:]
    read = lambda name: open(os.path.join(str(tmp_path), name), "rb").read()
    params = U.pkg().Params.from_buffer_copy(read("params.bin"))
    assert (int(params.x), int(params.y)) == (W, H)
    return p.stdout, read("stream.bin"), read("expected.bin"), params


def test_half_block_frames_reach_the_printer(exe, tmp_path):
    import torch
    R = U.pkg()
    out, stream, expected, p = run(exe, tmp_path, "on")
    bound = R.half_bound(MODE, W, H)
    assert "frames 2 max %d bound %d capacity %d" % (bound, bound, 20 * W * 2 * H) in out  # (rtx_update_half there and the facade's Update)
    assert stream == expected and stream.startswith(b"\x1b[H") and stream.endswith(b"\x1b[m") and stream.count(b"\x1b[H") == 1
    # the sample frame's words on a context of this test's own
    with R.Context(W, 2 * H) as c:
        c.set_reference_default_scene()
        q = R.Params.from_buffer_copy(bytes(p))
        q.y = 2 * H
        t = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.render_rows(q, MODE, 0, 2 * H, d_out=t.data_ptr(), flags=R.RENDER_COMPACT)
        c.synchronize()
        words = t.cpu().numpy().view(np.uint32)
        assert bytes(c.update_half(p, MODE)) == stream[3:-3]
    assert stream[3:-3] == RH.half_stream(MODE, W, H, words)
    grid = RH.keys(MODE, W, H, words)
    assert RH.replay(MODE, stream[3:-3], W, H) == grid
    hits = sum(1 for row in grid for (t_, b_) in row if t_ or b_)
    assert hits >= 20 and (W - 1) * H - hits >= 20


def test_unset_the_stream_is_what_it_was(exe, tmp_path):
    R = U.pkg()
    out, stream, expected, p = run(exe, tmp_path, "off")
    assert "frames 0 max %d " % (20 * W * H) in out and "capacity %d" % (20 * W * H) in out
    assert stream == expected and len(stream) > 1000 and stream.count(b"\x1b[H") == 1
    with R.Context(W, H) as c:
        c.set_reference_default_scene()
        assert b"\x1b[H" + bytes(c.update(p, MODE)) + b"\x1b[m" == stream


def test_switching_on_without_the_printer_prepared_throws(exe, tmp_path):
    out, stream, expected, p = run(exe, tmp_path, "unprepared")
    assert "frames 0 " in out and stream == expected
