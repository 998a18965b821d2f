"""The several-lights ABI (rtx_scene_set_lights / rtx_scene_get_lights) and the host side of the light set, without a GPU:
  * include/rtx.h as plain C99: RTX_MAX_LIGHTS, the two function types, the option and counter numbers, against the binding;
  * the two entry points refuse a NULL context through ctypes (no device is touched);
  * csrc/rtx_lights.hpp (validation and packing into the kernel argument block) under AddressSanitizer +
    UndefinedBehaviorSanitizer (tests/host/test_lights_pack.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    int (*set)(rtx_ctx*, size_t, const rtx_light*);
    int (*get)(const rtx_ctx*, size_t, rtx_light*, size_t*);
    rtx_light all[RTX_MAX_LIGHTS];
    (void)sizeof(set = rtx_scene_set_lights); /* the declarations' types, checked without linking the library */
    (void)sizeof(get = rtx_scene_get_lights);
    printf("%d %u %d %d\n", (int)RTX_MAX_LIGHTS, (unsigned)sizeof all, (int)RTX_OPT_LIGHTS_CHECK, (int)RTX_STAT_LIGHTS);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_lights_header_in_c99_and_in_the_binding(tmp_path):
    src = tmp_path / "lights.c"
    src.write_text(HEADER_C)
    exe = str(tmp_path / "lights")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).split()
    R = U.pkg()
    assert out == ["8", str(8 * 44), str(R.OPT_LIGHTS_CHECK), str(R.STAT_LIGHTS)]
    assert (R.MAX_LIGHTS, R.OPT_LIGHTS_CHECK, R.STAT_LIGHTS) == (8, 25, 137)
    for name in ("rtx_scene_set_lights", "rtx_scene_get_lights"):
        assert name in R.EXPORTED_SYMBOLS
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_scene_set_lights"][1:] == (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(R.Light)])
    assert sig["rtx_scene_get_lights"][1:] == (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(R.Light), C.POINTER(C.c_size_t)])
    assert callable(R.Context.set_lights) and callable(R.Context.get_lights)


def test_null_context_is_refused_without_a_gpu():
    R = U.pkg()
    lib = R.lib()
    l = R.make_light()
    assert lib.rtx_scene_set_lights(None, 1, C.byref(l)) == R.ERR_INVALID_ARGUMENT
    out = (R.Light * 8)()
    n = C.c_size_t(99)
    assert lib.rtx_scene_get_lights(None, 8, out, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert lib.rtx_scene_get_lights(None, 0, None, None) == R.ERR_INVALID_ARGUMENT
    assert n.value == 99


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lights_pack_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_lights_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_lights_pack.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all lights pack tests passed" in p.stdout, p.stdout[-4000:]
