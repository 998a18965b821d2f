"""RTX_OPT_REFLECT_GRID, RTX_STAT_REFLECT_GRID_FRAMES and RTX_STAT_REFLECT_GRID_FALLBACK_RAYS across the boundary, on the CPU:
include/rtx.h (parsed as tests/test_abi.py parses it), the Python constants and a C99 translation unit agree on 31, 98 and 97, no
number is used twice, and the option added no entry point."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    enum rtx_option o = RTX_OPT_REFLECT_GRID;
    enum rtx_stat s = RTX_STAT_REFLECT_GRID_FRAMES;
    printf("%d %d %d %d %d\n", (int)o, (int)s, (int)RTX_STAT_REFLECT_GRID_FALLBACK_RAYS, (int)RTX_OPT_SHADOW_GRID, (int)RTX_STAT_REFLECT_RAYS);
    return 0;
}
"""


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    assert e["RTX_OPT_REFLECT_GRID"] == 31 == R.OPT_REFLECT_GRID
    assert e["RTX_STAT_REFLECT_GRID_FRAMES"] == 98 == R.STAT_REFLECT_GRID_FRAMES
    assert e["RTX_STAT_REFLECT_GRID_FALLBACK_RAYS"] == 97 == R.STAT_REFLECT_GRID_FALLBACK_RAYS
    # no number taken twice among the options or among the counters, the ranges of the per-level counters and of the grid's
    # geometry included
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = []
    for k, v in e.items():
        if k.startswith("RTX_STAT_"):
            span = {"RTX_STAT_REFLECT_RAYS": R.MAX_REFLECT_DEPTH, "RTX_STAT_REFLECT_SHADOW_POINTS": R.MAX_REFLECT_DEPTH, "RTX_STAT_QUERY_GRID_GEOMETRY": 9}.get(k, 1)
            stats += list(range(v, v + span))
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    assert not set(opts) & set(stats)  # (one rtx_get_option serves both)
    for name in dir(R):
        if name.startswith(("OPT_", "STAT_")) and isinstance(getattr(R, name), int):
            assert e.get("RTX_" + name) == getattr(R, name), name


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(DECL_C)
    exe = str(tmp_path / "decl")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(U.ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["31", "98", "97", "29", "138"]


def test_no_new_entry_point():
    R = U.pkg()
    names = header_functions()
    assert sorted(R.EXPORTED_SYMBOLS) == names
    assert not [n for n in names if "reflect_grid" in n or "grid_reflect" in n]
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    if os.path.exists(so) and shutil.which("nm"):  # nm -D still equals the header
        out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
        exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("rtx_"))
        assert exported == names


def test_option_calls_without_a_context_are_refused():
    R = U.pkg()
    v = C.c_int64(7)
    for opt in (R.OPT_REFLECT_GRID, R.STAT_REFLECT_GRID_FRAMES, R.STAT_REFLECT_GRID_FALLBACK_RAYS):
        assert R.lib().rtx_get_option(None, opt, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7
    assert R.lib().rtx_set_option(None, R.OPT_REFLECT_GRID, 1) == R.ERR_INVALID_ARGUMENT
