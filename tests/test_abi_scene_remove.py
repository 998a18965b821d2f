"""rtx_scene_remove_objects, rtx_scene_remove_marked_device and RTX_STAT_SCENE_REMOVED across the boundary, on the CPU: include/rtx.h
(parsed as tests/test_abi.py parses it), the Python binding and a C99 translation unit agree on the two entry points and on 150."""
import ctypes as C
import os
import subprocess

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_remove_marked_device", "rtx_scene_remove_objects"]

DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    int (*a)(rtx_ctx*, size_t, const unsigned*) = rtx_scene_remove_objects;
    int (*b)(rtx_ctx*, const uint8_t*, void*, size_t*) = rtx_scene_remove_marked_device;
    enum rtx_stat s = RTX_STAT_SCENE_REMOVED;
    printf("%d %d\n", (int)s, a != 0 && b != 0);
    return 0;
}
"""


def test_header_declares_what_python_binds():
    R = U.pkg()
    names = header_functions()
    for n in NEW:
        assert n in names and n in R.EXPORTED_SYMBOLS, n
    assert sorted(R.EXPORTED_SYMBOLS) == names
    e = header_enums()
    assert e["RTX_STAT_SCENE_REMOVED"] == 150 == R.STAT_SCENE_REMOVED
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(stats) == len(set(stats)) and stats.count(150) == 1
    assert e["RTX_STAT_SCENE_EDIT_MOVE"] < 150
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_scene_remove_objects"][1] is C.c_int and sig["rtx_scene_remove_marked_device"][1] is C.c_int
    assert sig["rtx_scene_remove_objects"][2] == [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint)]
    assert sig["rtx_scene_remove_marked_device"][2] == [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    for m in ("remove_objects", "remove_marked_device"):
        assert callable(getattr(R.Context, m))


def test_every_declaration_states_its_reference_counterpart():
    text = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    for n in NEW + ["RTX_STAT_SCENE_REMOVED"]:
        at = text.index(n + ("(" if n.startswith("rtx_") else " ="))
        around = text[max(0, at - 3600):at + 700]
        assert "No reference counterpart" in around and "Scene3D.h:15-25" in around, n
    assert "never removed one by one" not in text


def test_the_header_still_compiles_as_c99_with_the_demo(tmp_path):
    R = U.pkg()
    inc = os.path.join(U.ROOT, "include")
    src = tmp_path / "decl.c"
    src.write_text(DECL_C)
    exe = str(tmp_path / "decl")
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    assert os.path.exists(so), "run build() first"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L", R.PKG_DIR, "-lrtx_hip",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.check_output([exe], text=True).split() == ["150", "1"]
    # the C demo of the ABI as well: the header alone, no C++
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(U.ROOT, "examples", "c_abi_demo.c"),
                           "-o", str(tmp_path / "demo.o")])


def test_the_library_exports_the_two_calls():
    R = U.pkg()
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("rtx_"))
    assert exported == header_functions()
    for n in NEW:
        assert n in exported, n


def test_calls_without_a_context_are_refused():
    R = U.pkg()
    idx = (C.c_uint * 1)(0)
    n = C.c_size_t(7)
    assert R.lib().rtx_scene_remove_objects(None, 1, idx) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_scene_remove_objects(None, 0, None) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_scene_remove_marked_device(None, None, None, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert n.value == 7
