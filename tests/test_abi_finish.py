"""Surface finishes across the boundary, on the CPU: include/rtx.h (parsed as tests/test_abi.py parses it) and the Python constants
agree on the counters 90 and 89, which no other name holds, struct rtx_finish is 16 bytes on both sides, there is no new option,
the header still compiles as C99 with -pedantic -Werror, the ctypes table is the header, the library exports the two new entry
points, each of them refuses a call without a context and writes nothing, and (on a GPU) every refusal the header lists changes
nothing on a live context."""
import ctypes as C
import os
import re
import subprocess

import pytest

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_get_finish", "rtx_scene_set_finish"]


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    assert e["RTX_STAT_FINISHED_OBJECTS"] == 90 == R.STAT_FINISHED_OBJECTS
    assert e["RTX_STAT_FINISH_FRAMES"] == 89 == R.STAT_FINISH_FRAMES
    # 89 and 90 are taken once, and no number is taken twice among the options or among the counters
    assert sorted(k for k, v in e.items() if v in (89, 90) and k.startswith(("RTX_OPT_", "RTX_STAT_"))) == ["RTX_STAT_FINISHED_OBJECTS", "RTX_STAT_FINISH_FRAMES"]
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    assert max(stats) == 154
    # no new option
    assert not [k for k in e if k.startswith("RTX_OPT_") and ("FINISH" in k or "SHININESS" in k or "AMBIENT" in k or "SPECULAR" in k)]
    assert not [n for n in dir(R) if n.startswith("OPT_") and ("FINISH" in n or "SHININESS" in n)]
    for name in dir(R):
        if name.startswith(("OPT_", "STAT_")) and isinstance(getattr(R, name), int):
            assert e.get("RTX_" + name) == getattr(R, name), name


def test_struct_is_16_bytes_on_both_sides(tmp_path):
    R = U.pkg()
    assert C.sizeof(R.Finish) == 16
    assert [(n, getattr(R.Finish, n).offset) for n, _ in R.Finish._fields_] == [("ambient", 0), ("diffuse", 4), ("specular", 8), ("shininess_log2", 12)]
    f = R.make_finish()
    assert (f.ambient, f.diffuse, f.specular, f.shininess_log2) == (C.c_float(0.2).value, 1.0, 1.0, 5)
    # the header's own struct, field by field, through the C compiler
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rtx.h"\n'
                   "typedef char size_is_16[sizeof(rtx_finish) == 16 ? 1 : -1];\n"
                   "typedef char offsets[offsetof(rtx_finish, ambient) == 0 && offsetof(rtx_finish, diffuse) == 4 && offsetof(rtx_finish, specular) == 8 &&\n"
                   "                     offsetof(rtx_finish, shininess_log2) == 12 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(U.ROOT, "include"), str(src)])
    # and the names carry none of the substrings the older ABI tests filter the header by
    for name in NEW + ["RTX_STAT_FINISHED_OBJECTS", "RTX_STAT_FINISH_FRAMES", "rtx_finish"]:
        assert not re.search("light|pattern|refraction|reflect|half|delta", name, re.I), name


def test_header_compiles_as_c99_pedantic():
    inc = os.path.join(U.ROOT, "include")
    demo = os.path.join(U.ROOT, "examples", "c_abi_demo.c")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, demo])
    assert "rtx_scene_set_finish" in open(demo).read()  # (so that the C99 check covers the struct in use)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, os.path.join(U.ROOT, "examples", "console_engine.cpp")])


def test_exported_symbols_equal_the_header():
    R = U.pkg()
    names = header_functions()
    assert sorted(R.EXPORTED_SYMBOLS) == names
    assert [n for n in names if "finish" in n] == NEW
    syms = subprocess.check_output(["nm", "-D", "--defined-only", R.LIB_PATH]).decode()
    exported = sorted(ln.split()[-1] for ln in syms.splitlines() if ln.split()[-1].startswith("rtx_") and " T " in ln)
    assert exported == names


def test_every_new_call_without_a_context_is_refused():
    R = U.pkg()
    L = R.lib()
    one = (R.Finish * 1)(R.make_finish(0.5, 0.5, 0.5, 3))
    out = R.make_finish(7.0, 7.0, 7.0, 7)
    assert L.rtx_scene_set_finish(None, 0, 1, one) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_set_finish(None, 0, 0, None) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_get_finish(None, 0, C.byref(out)) == R.ERR_INVALID_ARGUMENT
    assert (out.ambient, out.diffuse, out.specular, out.shininess_log2) == (7.0, 7.0, 7.0, 7)
    v = C.c_int64(7)
    for stat in (R.STAT_FINISHED_OBJECTS, R.STAT_FINISH_FRAMES):
        assert L.rtx_get_option(None, stat, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7


def _tuple(f):
    return (f.ambient, f.diffuse, f.specular, f.shininess_log2)


@pytest.mark.gpu
def test_refusals_change_nothing():
    """The header's list on a live context (creating one needs a device; nothing is rendered)."""
    R = U.pkg()
    L = R.lib()
    f32 = lambda v: C.c_float(v).value
    default = (f32(0.2), 1.0, 1.0, 5)
    with R.Context(41, 23) as c:
        for i in range(3):
            c.add_sphere(1.0, (float(i), 0.0, 20.0), (200.0, 100.0, 50.0))
        c.add_plane((0.0, -3.0, 30.0), (0.0, 1.0, 0.0), (100.0, 100.0, 100.0), 10.0, 20.0)
        assert [_tuple(c.get_finish(i)) for i in range(4)] == [default] * 4  # every new object: the reference's constants
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 0
        c.set_finish(0, [(0.5, 0.25, 1.7, 7), default, (16.0, 0.0, 16.0, 0), (-0.0, 1.0, 1.0, 8)])
        want = [(0.5, 0.25, f32(1.7), 7), default, (16.0, 0.0, 16.0, 0), (0.0, 1.0, 1.0, 8)]
        assert [_tuple(c.get_finish(i)) for i in range(4)] == want
        assert C.c_uint32.from_buffer_copy(C.c_float(c.get_finish(3).ambient)).value == 0  # -0.0f is stored as +0.0f
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 3
        nan, inf, ok = float("nan"), float("inf"), (0.5, 0.5, 0.5, 5)
        for first, vals, offender in ((0, [(nan, 1, 1, 5)], 0), (0, [ok, (1, inf, 1, 5)], 1), (1, [(1, 1, -inf, 5)], 1), (2, [(-1.0, 1, 1, 5)], 2),
                                      (0, [ok, ok, (1, 1, -1e-30, 5)], 2), (1, [(16.000002, 1, 1, 5)], 1), (0, [(1, 17.0, 1, 5)], 0), (3, [(1, 1, 1, 9)], 3),
                                      (0, [ok, (1, 1, 1, 0xffffffff)], 1), (3, [ok, ok], None), (5, [], None), (4, [ok], None), (0, [ok] * 5, None)):
            with pytest.raises(R.RtxError) as e:
                c.set_finish(first, vals)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            if offender is not None:  # rtx_last_error names the first offending object
                assert "object %d:" % offender in str(e.value), str(e.value)
            else:
                assert "rtx_scene_count" in str(e.value), str(e.value)
            assert [_tuple(c.get_finish(i)) for i in range(4)] == want
        # finishes == NULL with n > 0
        assert L.rtx_scene_set_finish(c._h, 0, 2, None) == R.ERR_INVALID_ARGUMENT
        out = R.make_finish(7.0, 7.0, 7.0, 7)
        assert L.rtx_scene_get_finish(c._h, 4, C.byref(out)) == R.ERR_INVALID_ARGUMENT and _tuple(out) == (7.0, 7.0, 7.0, 7)
        assert L.rtx_scene_get_finish(c._h, 0, None) == R.ERR_INVALID_ARGUMENT
        assert [_tuple(c.get_finish(i)) for i in range(4)] == want and c.get_option(R.STAT_FINISHED_OBJECTS) == 3
        c.set_finish(4, [])  # an empty range at the end is fine
        c.scene_clear()
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 0
