"""RayTracingManager::SetSupersampling (include/rtx_compat.hpp) on the GPU: tests/host/compat_supersample.cpp, host C++ over the C ABI
with the printer thread on a pipe, built once and run once per scenario.  With SetSupersampling(2) what the printer wrote, decoded as
a terminal would read it, must give the records of the folded frame (tests/restate_supersample.py over the S = 1 values of the
sample frame); with the call never made the stream is the one the facade writes today, the oracle's frame."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import restate_supersample as SS
import util as U

pytestmark = pytest.mark.gpu

W, H, S = 48, 20, 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    R = U.pkg()
    out = str(tmp_path_factory.mktemp("compat_supersample") / "compat_supersample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(U.ROOT, "include"),
                           os.path.join(U.ROOT, "tests", "host", "compat_supersample.cpp"), "-o", out, "-L", R.PKG_DIR, "-lrtx_hip", "-pthread",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def run(exe, tmp_path, scenario):
    p = subprocess.run([exe, str(tmp_path), scenario], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "facade supersampling ok" in p.stdout, p.stdout[-4000:]
    read = lambda name: open(os.path.join(str(tmp_path), name), "rb").read()
    params = U.pkg().Params.from_buffer_copy(read("params.bin"))
    assert (int(params.x), int(params.y)) == (W, H)
    return p.stdout, read("stream.bin"), read("expected.bin"), params


def screen_after(stream):
    """The H x (W-1) grid of records a terminal shows after one whole frame: ESC [ H homes, ESC [ m (the colour reset) is skipped, a
    byte ESC starts a record, a newline goes to the next row, any other byte is a glyph under the colour of the last whole record."""
    grid = [[None] * (W - 1) for _ in range(H)]
    row = col = at = 0
    head = None
    while at < len(stream):
        if stream.startswith(b"\x1b[H", at):
            row = col = 0
            at += 3
        elif stream.startswith(b"\x1b[m", at):
            head = None
            at += 3
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
            assert head is not None, "a glyph without a colour at byte %d" % at
            grid[row][col] = head + stream[at:at + 1]
            col += 1
            at += 1
    return grid


def grid_of(rec):
    rec = np.asarray(rec, dtype=np.uint8).reshape(-1)[:S * W * H].reshape(H * W, S)
    return [[bytes(rec[r * W + c]) for c in range(W - 1)] for r in range(H)]


def test_supersampled_frames_reach_the_printer(exe, tmp_path):
    import torch
    R = U.pkg()
    out, stream, expected, p = run(exe, tmp_path, "on")
    assert "samples 2 frames 2" in out  # (rtx_update here and the facade's Update)
    assert stream == expected and stream.count(b"\x1b[H") == 1
    # the records of the folded frame, from the S = 1 values of the sample frame on a context of this test's own
    with R.Context(2 * W, 2 * H) as c:
        c.set_reference_default_scene()
        ps = SS.sample_params(p, 2)
        buf = torch.zeros(32 * 4 * W * H, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.render_rows(ps, O.RGB_ASCII, 0, 2 * H, d_out=buf.data_ptr(), out_row_base=0, flags=R.RENDER_VALUES)
        c.synchronize()
        assert c.last_kernel.startswith("rtx_trace<")
        values, rec, _ = SS.expected(buf.cpu().numpy().view(np.float32), W, H, 2, O.RGB_ASCII, float(p.cam_far))
    cells = values.reshape(H, W, 8)[:, :W - 1]
    m = cells[..., 0] <= np.float32(p.cam_far)
    assert m.sum() >= 20 and (~m).sum() >= 20
    assert screen_after(stream) == grid_of(rec)
    plain = grid_of(O.render(U.oracle_params(p), O.Scene.reference_default(), O.RGB_ASCII))
    assert screen_after(stream) != plain  # (partial coverage shows: the frame is not the one-ray frame)


def test_unset_the_stream_is_what_it_was(exe, tmp_path):
    out, stream, expected, p = run(exe, tmp_path, "off")
    assert "samples 1 frames 0" in out
    assert stream == expected and len(stream) > 1000 and stream.count(b"\x1b[H") == 1
    assert screen_after(stream) == grid_of(O.render(U.oracle_params(p), O.Scene.reference_default(), O.RGB_ASCII))
