"""Objects that cast no shadow across the boundary, on the CPU: include/rtx.h (parsed as tests/test_abi.py parses it) and the Python
constants agree, the call adds no option and no counter, the header and the examples still
compile (C99 with -pedantic -Werror; the compat layer's SetCastsShadow), the ctypes table is the header, the library exports the two
new entry points, each of them refuses a call without a context and writes nothing, and (on a GPU) every refusal the header lists
changes nothing on a live context."""
import ctypes as C
import os
import subprocess

import pytest

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_get_shadow_casting", "rtx_scene_set_shadow_casting"]


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    # no number is taken twice among the options or among the counters
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    # no new option and no new counter
    assert not [k for k in e if k.startswith("RTX_STAT_") and ("CAST" in k or "SHADOWLESS" in k)]
    assert not [k for k in e if k.startswith("RTX_OPT_") and ("CAST" in k or "SHADOWLESS" in k)]
    assert not [n for n in dir(R) if n.startswith("OPT_") and ("CAST" in n or "SHADOWLESS" in n)]
    for name in dir(R):
        if name.startswith(("OPT_", "STAT_")) and isinstance(getattr(R, name), int):
            assert e.get("RTX_" + name) == getattr(R, name), name


def test_header_and_examples_compile(tmp_path):
    inc = os.path.join(U.ROOT, "include")
    src = tmp_path / "types.c"
    src.write_text('#include "rtx.h"\n'
                   "int main(void)\n{\n"
                   "    int (*set)(rtx_ctx*, unsigned, size_t, const uint8_t*);\n"
                   "    int (*get)(const rtx_ctx*, unsigned, uint8_t*);\n"
                   "    (void)sizeof(set = rtx_scene_set_shadow_casting); /* the declarations' types, checked without linking the library */\n"
                   "    (void)sizeof(get = rtx_scene_get_shadow_casting);\n"
                   "    return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    demo = os.path.join(U.ROOT, "examples", "c_abi_demo.c")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, demo])
    assert "rtx_scene_set_shadow_casting" in open(demo).read()
    engine = os.path.join(U.ROOT, "examples", "console_engine.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, engine])
    text = open(engine).read()
    assert "--clear-glass" in text and "SetCastsShadow" in text
    assert "SetCastsShadow" in open(os.path.join(inc, "rtx_compat.hpp")).read()


def test_exported_symbols_equal_the_header():
    R = U.pkg()
    names = header_functions()
    assert sorted(R.EXPORTED_SYMBOLS) == names
    assert [n for n in names if "shadow_casting" in n] == NEW
    syms = subprocess.check_output(["nm", "-D", "--defined-only", R.LIB_PATH]).decode()
    exported = sorted(ln.split()[-1] for ln in syms.splitlines() if ln.split()[-1].startswith("rtx_") and " T " in ln)
    assert exported == names


def test_every_new_call_without_a_context_is_refused():
    R = U.pkg()
    L = R.lib()
    one = (C.c_uint8 * 1)(0)
    out = C.c_uint8(7)
    assert L.rtx_scene_set_shadow_casting(None, 0, 1, one) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_set_shadow_casting(None, 0, 0, None) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_get_shadow_casting(None, 0, C.byref(out)) == R.ERR_INVALID_ARGUMENT and out.value == 7


@pytest.mark.gpu
def test_refusals_change_nothing():
    """The header's list on a live context (creating one needs a device; nothing is rendered)."""
    R = U.pkg()
    L = R.lib()
    with R.Context(41, 23) as c:
        for i in range(3):
            c.add_sphere(1.0, (float(i), 0.0, 20.0), (200.0, 100.0, 50.0))
        c.add_plane((0.0, -3.0, 30.0), (0.0, 1.0, 0.0), (100.0, 100.0, 100.0), 10.0, 20.0)
        flags = lambda: [c.get_shadow_casting(i) for i in range(4)]
        assert flags() == [1, 1, 1, 1]  # every new object casts
        c.set_shadow_casting(0, [0, 1, 1, 0])
        want = [0, 1, 1, 0]
        assert flags() == want
        for first, vals, offender in ((0, [2], 0), (0, [1, 255], 1), (1, [0, 0, 3], 3), (3, [128], 3), (3, [1, 1], None), (5, [], None), (4, [0], None), (0, [0] * 5, None)):
            with pytest.raises(R.RtxError) as e:
                c.set_shadow_casting(first, vals)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            if offender is not None:  # rtx_last_error names the first offending object
                assert "object %d:" % offender in str(e.value), str(e.value)
            else:
                assert "rtx_scene_count" in str(e.value), str(e.value)
            assert flags() == want
        # casts == NULL with n > 0
        assert L.rtx_scene_set_shadow_casting(c._h, 0, 2, None) == R.ERR_INVALID_ARGUMENT
        out = C.c_uint8(7)
        assert L.rtx_scene_get_shadow_casting(c._h, 4, C.byref(out)) == R.ERR_INVALID_ARGUMENT and out.value == 7
        assert L.rtx_scene_get_shadow_casting(c._h, 0, None) == R.ERR_INVALID_ARGUMENT
        assert flags() == want
        c.set_shadow_casting(4, [])  # an empty range at the end is fine
        c.add_sphere(1.0, (5.0, 0.0, 20.0), (200.0, 100.0, 50.0))
        assert c.get_shadow_casting(4) == 1 and flags() == want  # a new object casts, the others keep theirs
        c.scene_clear()  # the flags are forgotten: a new scene's objects cast
        c.add_sphere(1.0, (0.0, 0.0, 20.0), (200.0, 100.0, 50.0))
        assert c.get_shadow_casting(0) == 1
