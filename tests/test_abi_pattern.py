"""Checker patterns across the boundary, on the CPU: struct rtx_pattern is 36 bytes on both sides, include/rtx.h (parsed as
tests/test_abi.py parses it) and the Python constants agree on RTX_MAX_PATTERNS and on the counters 94 and 93, which no other name
holds, the header still compiles as C99 with -pedantic -Werror, the ctypes table is the header, the library exports the four new
entry points, and each of them refuses a call without a context."""
import ctypes as C
import os
import re
import subprocess

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_get_object_pattern", "rtx_scene_get_patterns", "rtx_scene_set_object_pattern", "rtx_scene_set_patterns"]


def test_struct_is_36_bytes_on_both_sides(tmp_path):
    R = U.pkg()
    assert C.sizeof(R.Pattern) == 36
    assert (R.Pattern.origin.offset, R.Pattern.freq.offset, R.Pattern.rgb.offset) == (0, 12, 24)
    src = tmp_path / "size.c"
    src.write_text('#include "rtx.h"\n#include <stddef.h>\n'
                   "typedef char size_is_36[sizeof(rtx_pattern) == 36 ? 1 : -1];\n"
                   "typedef char freq_at_12[offsetof(rtx_pattern, freq) == 12 ? 1 : -1];\n"
                   "typedef char rgb_at_24[offsetof(rtx_pattern, rgb) == 24 ? 1 : -1];\n"
                   "typedef char sixteen[RTX_MAX_PATTERNS == 16 ? 1 : -1];\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(U.ROOT, "include"), str(src)])


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    assert e["RTX_STAT_PATTERNED_OBJECTS"] == 94 == R.STAT_PATTERNED_OBJECTS
    assert e["RTX_STAT_PATTERN_FRAMES"] == 93 == R.STAT_PATTERN_FRAMES
    src = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    assert int(re.search(r"#define\s+RTX_MAX_PATTERNS\s+(\d+)", src).group(1)) == 16 == R.MAX_PATTERNS
    # 93 and 94 are taken once, and no number is taken twice among the options or among the counters
    assert [k for k, v in e.items() if v in (93, 94) and k.startswith(("RTX_OPT_", "RTX_STAT_"))] == ["RTX_STAT_PATTERNED_OBJECTS", "RTX_STAT_PATTERN_FRAMES"]
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    # no new option
    assert not [k for k in e if k.startswith("RTX_OPT_") and "PATTERN" in k]
    for name in dir(R):
        if name.startswith(("OPT_", "STAT_")) and isinstance(getattr(R, name), int):
            assert e.get("RTX_" + name) == getattr(R, name), name


def test_header_compiles_as_c99_pedantic():
    inc = os.path.join(U.ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, os.path.join(U.ROOT, "examples", "c_abi_demo.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, os.path.join(U.ROOT, "examples", "console_engine.cpp")])


def test_exported_symbols_equal_the_header():
    R = U.pkg()
    names = header_functions()
    assert sorted(R.EXPORTED_SYMBOLS) == names
    assert [n for n in names if "pattern" in n] == NEW
    syms = subprocess.check_output(["nm", "-D", "--defined-only", R.LIB_PATH]).decode()
    exported = sorted(ln.split()[-1] for ln in syms.splitlines() if ln.split()[-1].startswith("rtx_") and " T " in ln)
    assert exported == names


def test_every_new_call_without_a_context_is_refused():
    R = U.pkg()
    L = R.lib()
    one = (R.Pattern * 1)(R.make_pattern())
    n = C.c_size_t(7)
    slot = C.c_uint(7)
    assert L.rtx_scene_set_patterns(None, 1, one) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_set_patterns(None, 0, None) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_get_patterns(None, 1, one, C.byref(n)) == R.ERR_INVALID_ARGUMENT and n.value == 7
    assert L.rtx_scene_set_object_pattern(None, 0, 0, 0) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_get_object_pattern(None, 0, C.byref(slot)) == R.ERR_INVALID_ARGUMENT and slot.value == 7
    v = C.c_int64(7)
    for stat in (R.STAT_PATTERNED_OBJECTS, R.STAT_PATTERN_FRAMES):
        assert L.rtx_get_option(None, stat, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7
