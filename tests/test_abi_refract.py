"""Glass across the boundary, on the CPU: include/rtx.h (parsed as tests/test_abi.py parses it) and the Python constants agree on
the counters 92 and 91, which no other name holds, there is no new option, the header still compiles as C99 with -pedantic
-Werror, the ctypes table is the header, the library exports the two new entry points, each of them refuses a call without a
context, and every refusal the header lists changes nothing (on a context without a device behind it: nothing is launched)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_get_refraction", "rtx_scene_set_refraction"]


def test_header_and_python_constants_agree():
    R = U.pkg()
    e = header_enums()
    assert e["RTX_STAT_REFRACTIVE_OBJECTS"] == 92 == R.STAT_REFRACTIVE_OBJECTS
    assert e["RTX_STAT_REFRACT_FRAMES"] == 91 == R.STAT_REFRACT_FRAMES
    # 91 and 92 are taken once, and no number is taken twice among the options or among the counters
    assert [k for k, v in e.items() if v in (91, 92) and k.startswith(("RTX_OPT_", "RTX_STAT_"))] == ["RTX_STAT_REFRACTIVE_OBJECTS", "RTX_STAT_REFRACT_FRAMES"]
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(opts) == len(set(opts)) and len(stats) == len(set(stats))
    assert max(stats) == 154
    # no new option
    assert not [k for k in e if k.startswith("RTX_OPT_") and ("REFRACT" in k or "GLASS" in k or "IOR" in k)]
    assert not [n for n in dir(R) if n.startswith("OPT_") and ("REFRACT" in n or "GLASS" in n)]
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
    assert [n for n in names if "refraction" in n] == NEW
    syms = subprocess.check_output(["nm", "-D", "--defined-only", R.LIB_PATH]).decode()
    exported = sorted(ln.split()[-1] for ln in syms.splitlines() if ln.split()[-1].startswith("rtx_") and " T " in ln)
    assert exported == names


def test_every_new_call_without_a_context_is_refused():
    R = U.pkg()
    L = R.lib()
    one = (C.c_float * 1)(1.5)
    out = C.c_float(7.0)
    assert L.rtx_scene_set_refraction(None, 0, 1, one) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_set_refraction(None, 0, 0, None) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_scene_get_refraction(None, 0, C.byref(out)) == R.ERR_INVALID_ARGUMENT and out.value == 7.0
    v = C.c_int64(7)
    for stat in (R.STAT_REFRACTIVE_OBJECTS, R.STAT_REFRACT_FRAMES):
        assert L.rtx_get_option(None, stat, C.byref(v)) == R.ERR_INVALID_ARGUMENT and v.value == 7


@pytest.mark.gpu
def test_refusals_change_nothing():
    """The header's list on a live context (creating one needs a device; nothing is rendered)."""
    R = U.pkg()
    L = R.lib()
    with R.Context(41, 23) as c:
        for i in range(3):
            c.add_sphere(1.0, (float(i), 0.0, 20.0), (200.0, 100.0, 50.0))
        c.add_plane((0.0, -3.0, 30.0), (0.0, 1.0, 0.0), (100.0, 100.0, 100.0), 10.0, 20.0)
        assert [c.get_refraction(i) for i in range(4)] == [0.0] * 4  # every new object: a mirror
        c.set_refraction(0, [1.5, 0.0, 4.0, 1.0])
        want = [1.5, 0.0, 4.0, 1.0]
        assert c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 3
        for first, vals in ((0, [float("nan")]), (0, [1.25, 0.5]), (1, [4.5]), (2, [-1.0]), (0, [1.5, float("inf")]), (3, [1.5, 1.5]),
                            (5, []), (4, [1.5]), (0, [1.5, 1.5, 1.5, 1.5, 1.5]), (0, [0.99999994]), (0, [4.0000005])):
            with pytest.raises(R.RtxError) as e:
                c.set_refraction(first, np.array(vals, dtype=np.float32))
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            assert [c.get_refraction(i) for i in range(4)] == want
        # ior == NULL with n > 0
        assert L.rtx_scene_set_refraction(c._h, 0, 2, None) == R.ERR_INVALID_ARGUMENT
        out = C.c_float(7.0)
        assert L.rtx_scene_get_refraction(c._h, 4, C.byref(out)) == R.ERR_INVALID_ARGUMENT and out.value == 7.0
        assert L.rtx_scene_get_refraction(c._h, 0, None) == R.ERR_INVALID_ARGUMENT
        assert [c.get_refraction(i) for i in range(4)] == want and c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 3
        c.set_refraction(4, [])  # an empty range at the end is fine
        c.scene_clear()
        assert c.get_option(R.STAT_REFRACTIVE_OBJECTS) == 0
