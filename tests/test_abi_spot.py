"""Spot lights across the boundary, on the CPU: include/rtx.h (parsed as tests/test_abi.py parses it) and the Python constants agree
on the counters 88 and 87, which no other name holds, struct rtx_spot is 20 bytes on both sides, there is no new option, the ctypes
table is the header, the library exports the two new entry points, and each of them refuses a call without a context and writes
nothing."""
import ctypes as C
import os
import subprocess

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_get_spots", "rtx_scene_set_spots"]


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    assert e["RTX_STAT_SPOT_LIGHTS"] == 88 == R.STAT_SPOT_LIGHTS
    assert e["RTX_STAT_SPOT_FRAMES"] == 87 == R.STAT_SPOT_FRAMES
    # 87 and 88 are taken once, and no number is taken twice among the options or among the counters
    assert sorted(k for k, v in e.items() if v in (87, 88) and k.startswith(("RTX_OPT_", "RTX_STAT_"))) == ["RTX_STAT_SPOT_FRAMES", "RTX_STAT_SPOT_LIGHTS"]
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    assert max(stats) == 154 and min(stats) == 87
    # no new option
    assert not [k for k in e if k.startswith("RTX_OPT_") and ("SPOT" in k or "CONE" in k)]
    assert not [n for n in dir(R) if n.startswith("OPT_") and ("SPOT" in n or "CONE" in n)]
    for name in dir(R):
        if name.startswith(("OPT_", "STAT_")) and isinstance(getattr(R, name), int):
            assert e.get("RTX_" + name) == getattr(R, name), name


def test_struct_is_20_bytes_on_both_sides(tmp_path):
    R = U.pkg()
    assert C.sizeof(R.Spot) == 20
    assert [(n, getattr(R.Spot, n).offset) for n, _ in R.Spot._fields_] == [("dir", 0), ("cos_outer", 12), ("cos_inner", 16)]
    s = R.make_spot()
    assert (tuple(s.dir), s.cos_outer, s.cos_inner) == ((0.0, 0.0, 0.0), 0.0, 0.0)  # the default: a point light
    s = R.make_spot((1.0, -2.0, 3.0), 0.5, 0.75)
    assert (tuple(s.dir), s.cos_outer, s.cos_inner) == ((1.0, -2.0, 3.0), 0.5, 0.75)
    # the header's own struct, field by field, through the C compiler
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rtx.h"\n'
                   "typedef char size_is_20[sizeof(rtx_spot) == 20 ? 1 : -1];\n"
                   "typedef char offsets[offsetof(rtx_spot, dir) == 0 && offsetof(rtx_spot, cos_outer) == 12 && offsetof(rtx_spot, cos_inner) == 16 ? 1 : -1];\n"
                   "int main(void)\n{\n"
                   "    int (*set)(rtx_ctx*, size_t, const rtx_spot*);\n"
                   "    int (*get)(const rtx_ctx*, size_t, rtx_spot*, size_t*);\n"
                   "    (void)sizeof(set = rtx_scene_set_spots); /* the declarations' types, checked without linking the library */\n"
                   "    (void)sizeof(get = rtx_scene_get_spots);\n"
                   "    return (int)RTX_STAT_SPOT_LIGHTS - 88 + (int)RTX_STAT_SPOT_FRAMES - 87;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(U.ROOT, "include"), str(src)])


def test_header_and_examples_compile():
    inc = os.path.join(U.ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, os.path.join(U.ROOT, "examples", "c_abi_demo.c")])
    engine = os.path.join(U.ROOT, "examples", "console_engine.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, engine])
    text = open(engine).read()
    assert "--spot" in text and "SetSpots" in text and "[--spot]" in text  # (the switch, its call and the usage line)
    assert "SetSpots(const rtx_spot* spots, const size_t n)" in open(os.path.join(inc, "rtx_compat.hpp")).read()


def test_exported_symbols_equal_the_header():
    R = U.pkg()
    names = header_functions()
    assert sorted(R.EXPORTED_SYMBOLS) == names
    assert [n for n in names if "spot" in n] == NEW
    syms = subprocess.check_output(["nm", "-D", "--defined-only", R.LIB_PATH]).decode()
    exported = sorted(ln.split()[-1] for ln in syms.splitlines() if ln.split()[-1].startswith("rtx_") and " T " in ln)
    assert exported == names
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_scene_set_spots"][1:] == (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(R.Spot)])
    assert sig["rtx_scene_get_spots"][1:] == (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(R.Spot), C.POINTER(C.c_size_t)])
    assert callable(R.Context.set_spots) and callable(R.Context.get_spots)


def test_every_new_call_without_a_context_is_refused():
    R = U.pkg()
    L = R.lib()
    one = (R.Spot * 1)(R.make_spot((0.0, -1.0, 0.0), 0.5, 0.75))
    assert L.rtx_scene_set_spots(None, 1, one) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_set_spots(None, 0, None) == R.ERR_INVALID_ARGUMENT
    out = (R.Spot * 8)()
    for i in range(8):
        out[i].cos_outer = 7.0
    n = C.c_size_t(99)
    assert L.rtx_scene_get_spots(None, 8, out, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_get_spots(None, 0, None, None) == R.ERR_INVALID_ARGUMENT
    assert n.value == 99 and all(out[i].cos_outer == 7.0 for i in range(8))
    v = C.c_int64(7)
    for stat in (R.STAT_SPOT_LIGHTS, R.STAT_SPOT_FRAMES):
        assert L.rtx_get_option(None, stat, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7
