"""rtx_scene_set_spheres, rtx_scene_set_spheres_device, rtx_scene_set_plane, RTX_STAT_SCENE_EDITS and RTX_STAT_SCENE_EDIT_MOVE across
the boundary, on the CPU: include/rtx.h (parsed as tests/test_abi.py parses it), the Python binding and a C99 translation unit agree
on the three entry points and on 148 and 149."""
import ctypes as C
import os
import subprocess

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_scene_set_plane", "rtx_scene_set_spheres", "rtx_scene_set_spheres_device"]

DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    int (*a)(rtx_ctx*, unsigned, size_t, const float*) = rtx_scene_set_spheres;
    int (*b)(rtx_ctx*, unsigned, size_t, const float*, void*) = rtx_scene_set_spheres_device;
    int (*c)(rtx_ctx*, unsigned, const float*, const float*, const float*, float, float) = rtx_scene_set_plane;
    enum rtx_stat s = RTX_STAT_SCENE_EDITS;
    printf("%d %d %d\n", (int)s, (int)RTX_STAT_SCENE_EDIT_MOVE, a != 0 && b != 0 && c != 0);
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
    assert e["RTX_STAT_SCENE_EDITS"] == 148 == R.STAT_SCENE_EDITS
    assert e["RTX_STAT_SCENE_EDIT_MOVE"] == 149 == R.STAT_SCENE_EDIT_MOVE
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(stats) == len(set(stats))
    assert e["RTX_STAT_SHADOW_GRID_FALLBACK_POINTS"] < 148
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_scene_set_spheres"][1] is C.c_int and len(sig["rtx_scene_set_spheres"][2]) == 4
    assert len(sig["rtx_scene_set_spheres_device"][2]) == 5 and len(sig["rtx_scene_set_plane"][2]) == 7
    for m in ("set_spheres", "set_spheres_device", "set_plane"):
        assert callable(getattr(R.Context, m))


def test_every_declaration_states_its_reference_counterpart():
    text = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    for n in NEW + ["RTX_STAT_SCENE_EDITS", "RTX_STAT_SCENE_EDIT_MOVE"]:
        at = text.index(n + ("(" if n.startswith("rtx_") else " ="))
        around = text[max(0, at - 2600):at + 700]
        assert "No reference counterpart beyond Object3D.cu:34" in around, n


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
    assert subprocess.check_output([exe], text=True).split() == ["148", "149", "1"]
    # the C demo of the ABI as well: the header alone, no C++
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(U.ROOT, "examples", "c_abi_demo.c"),
                           "-o", str(tmp_path / "demo.o")])


def test_the_library_exports_the_three_calls():
    R = U.pkg()
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("rtx_"))
    assert exported == header_functions()


def test_calls_without_a_context_are_refused():
    R = U.pkg()
    rows = (C.c_float * 7)()
    v3 = (C.c_float * 3)()
    assert R.lib().rtx_scene_set_spheres(None, 0, 1, rows) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_scene_set_spheres_device(None, 0, 1, rows, None) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_scene_set_plane(None, 0, v3, v3, v3, 1.0, 1.0) == R.ERR_INVALID_ARGUMENT
