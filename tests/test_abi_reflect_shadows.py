"""RTX_OPT_REFLECT_SHADOWS and RTX_STAT_REFLECT_SHADOW_POINTS across the boundary, on the CPU: include/rtx.h (parsed as
tests/test_abi.py parses it), the Python constants and the library's own idea of the numbers agree on 28 and 142 .. 145, and the
option added no entry point."""
import ctypes as C
import os
import re

import util as U
from test_abi import header_functions


def header_enums():
    src = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: int(value) for name, value in re.findall(r"\b(RTX_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*[,}\n]", src)}


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    assert e["RTX_OPT_REFLECT_SHADOWS"] == 28 == R.OPT_REFLECT_SHADOWS
    assert e["RTX_STAT_REFLECT_SHADOW_POINTS"] == 142 == R.STAT_REFLECT_SHADOW_POINTS
    assert R.MAX_REFLECT_DEPTH == 4  # 142 .. 145
    # the neighbours it sits beside, and no number taken twice among the options or among the counters
    assert e["RTX_OPT_REFLECT_DEPTH"] == R.OPT_REFLECT_DEPTH == 26 and e["RTX_OPT_REFLECT_DEPTH_CHECK"] == R.OPT_REFLECT_DEPTH_CHECK == 27
    assert e["RTX_STAT_REFLECT_RAYS"] == R.STAT_REFLECT_RAYS == 138
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    # 142 .. 145 are the four levels' counters: no other name sits on them
    assert not [k for k, v in e.items() if 143 <= v <= 145 and k.startswith(("RTX_OPT_", "RTX_STAT_"))]


def test_every_python_option_constant_is_the_headers():
    R = U.pkg()
    e = header_enums()
    for name in dir(R):
        if name.startswith(("OPT_", "STAT_")) and isinstance(getattr(R, name), int):
            assert e.get("RTX_" + name) == getattr(R, name), name


def test_no_new_entry_point():
    R = U.pkg()
    names = header_functions()
    assert sorted(R.EXPORTED_SYMBOLS) == names
    assert not [n for n in names if "reflect_shadow" in n or "chain_shadow" in n]


def test_get_option_without_a_context_is_refused():
    R = U.pkg()
    v = C.c_int64(7)
    assert R.lib().rtx_get_option(None, R.OPT_REFLECT_SHADOWS, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7
    assert R.lib().rtx_set_option(None, R.OPT_REFLECT_SHADOWS, 1) == R.ERR_INVALID_ARGUMENT
