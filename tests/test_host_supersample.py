"""RTX_OPT_SUPERSAMPLE on the CPU: rtxplan::plan_supersample under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/test_supersample_plan.cpp), the self-checks of the fold's numpy restatement (tests/restate_supersample.py), and the input
condition of the GPU cases (tests/test_gpu_supersample.py), judged with the oracle alone.  No HIP, no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_supersample as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the case of the GPU tests: the reference's default scene from (0, 5, -10), far plane at 33, 37 x 19 cells
W, H, CAM, FAR = 37, 19, (0.0, 5.0, -10.0), 33.0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_supersample_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_supersample_plan.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all supersample planning tests passed" in p.stdout, p.stdout[-4000:]


def _random_values(rng, rows, w):
    v = rng.normal(size=(rows, w, 8)).astype(np.float32)
    v[..., 0] = rng.uniform(1.0, 60.0, size=(rows, w)).astype(np.float32)
    v[rng.random((rows, w)) < 0.3, 0] = SS.NO_HIT
    return v


def test_one_sample_is_the_identity():
    """S = 1: a visible cell keeps its eight floats bit for bit, any other becomes the miss values, column W-1 zeros."""
    rng = np.random.default_rng(5)
    v = _random_values(rng, 6, 9)
    got = SS.fold(v, 9, 6, 1, FAR).reshape(6, 9, 8)
    vis = v[..., 0] <= np.float32(FAR)
    assert vis[:, :8].any() and (~vis[:, :8]).any()
    assert RS.same_floats(got[:, :8][vis[:, :8]], v[:, :8][vis[:, :8]]).all()
    miss = got[:, :8][~vis[:, :8]]
    assert (miss[:, 0] == SS.NO_HIT).all() and (miss[:, 1:].view(np.uint32) == 0).all()
    assert (got[:, 8].view(np.uint32) == 0).all()


def test_sums_run_in_the_stated_order():
    """1 + 2^-24 + 2^-24 + 0 from the left is 1 (each add rounds to even); from the right it is 1 + 2^-23: the last bit tells."""
    tiny = np.float32(2.0 ** -24)
    s = np.zeros((2, 4, 8), dtype=np.float32)  # one cell of 2 x 2 samples and the newline column's
    s[:, :, 0] = 1.0
    for k, val in enumerate((np.float32(1.0), tiny, tiny, np.float32(0.0))):
        s[k // 2, k % 2, 1:] = val
    stated = SS.fold(s, 2, 1, 2, FAR)[0]
    other = SS.fold(s, 2, 1, 2, FAR, order=[3, 2, 1, 0])[0]
    assert (stated[1:] == np.float32(0.25)).all()
    assert (other[1:] == np.float32(0.25) * (np.float32(1.0) + np.float32(2.0 ** -23))).all()
    assert (stated[1:].view(np.uint32) + 1 == other[1:].view(np.uint32)).all()
    # one multiply by 1.0f / 9.0f, not a division: the two differ for 3 x 3 samples of 1.0
    n = np.zeros((3, 6, 8), dtype=np.float32)
    n[:, :3, :] = 1.0
    v = SS.fold(n, 2, 1, 3, FAR)[0]
    assert v[1] == np.float32(9.0) * (np.float32(1.0) / np.float32(9.0)) and v[0] == np.float32(1.0)


def test_samples_beyond_far_count_as_black():
    s = np.zeros((2, 4, 8), dtype=np.float32)
    s[0, 0] = [10.0, 0.5, 0.0, 1.0, 0.0, 200.0, 100.0, 50.0]
    s[0, 1] = [40.0, 0.9, 1.0, 0.0, 0.0, 255.0, 255.0, 255.0]   # hit, beyond far
    s[1, 0] = [SS.NO_HIT, 0, 0, 0, 0, 0, 0, 0]
    s[1, 1] = [20.0, 0.25, 0.0, 0.0, 1.0, 40.0, 20.0, 10.0]
    v = SS.fold(s, 2, 1, 2, FAR)[0]
    assert v.tolist() == [10.0, 0.1875, 0.0, 0.25, 0.25, 60.0, 30.0, 15.0]
    none = SS.fold(s, 2, 1, 2, 5.0)[0]
    assert none[0] == SS.NO_HIT and (none[1:].view(np.uint32) == 0).all()


@pytest.mark.parametrize("S", [2, 3, 4])
def test_gpu_case_holds_every_kind_of_cell(S):
    """At least 10 cells of each kind in the sample frame the GPU tests fold (the smallest class: 11 cells at S = 2)."""
    _, ps = SS.case_params(O, W, H, S, CAM, FAR)
    _, px = O.render(ps, O.Scene.reference_default(), O.RGB_ASCII, want_pixels=True)
    kinds = SS.cell_classes(px["distance"], px["hit"], W, H, S, FAR)
    counts = {k: int(v.sum()) for k, v in kinds.items()}
    print("S = %d: %r" % (S, counts))
    assert all(n >= 10 for n in counts.values()), counts


DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    enum rtx_option o = RTX_OPT_SUPERSAMPLE;
    enum rtx_stat s = RTX_STAT_SUPERSAMPLE_FRAMES;
    printf("%d %d %d\n", (int)o, (int)s, (int)RTX_STAT_DELTA_RUNS);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_option_and_counter_numbers_across_the_boundary(tmp_path):
    """The header as a C99 compiler reads it, and the Python binding: option 30, counter 100, numbers no other option or counter has."""
    import re
    import util as U
    R = U.pkg()
    src = tmp_path / "decl.c"
    src.write_text(DECL_C)
    exe = str(tmp_path / "decl")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["30", "100", "154"]
    assert (R.OPT_SUPERSAMPLE, R.STAT_SUPERSAMPLE_FRAMES) == (30, 100)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx.h")).read(), flags=re.S)
    numbered = {n: int(v) for n, v in re.findall(r"\b(RTX_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*[,}\n]", text)}
    assert (numbered["RTX_OPT_SUPERSAMPLE"], numbered["RTX_STAT_SUPERSAMPLE_FRAMES"]) == (30, 100)
    others = [v for n, v in numbered.items() if n.startswith(("RTX_OPT_", "RTX_STAT_")) and n not in ("RTX_OPT_SUPERSAMPLE", "RTX_STAT_SUPERSAMPLE_FRAMES")]
    assert 30 not in others and 100 not in others  # (rtx_get_option reads options and counters by one number)
    # no new exported symbol: the option and the counter go through rtx_set_option / rtx_get_option
    assert not [n for n in R.EXPORTED_SYMBOLS if "supersample" in n or "resolve" in n]
    v = C.c_int64(7)
    assert R.lib().rtx_get_option(None, R.STAT_SUPERSAMPLE_FRAMES, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7
    assert R.lib().rtx_set_option(None, R.OPT_SUPERSAMPLE, 2) == R.ERR_INVALID_ARGUMENT
