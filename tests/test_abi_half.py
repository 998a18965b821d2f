"""rtx_half_bound, rtx_half_words, rtx_update_half and RTX_STAT_HALF_FRAMES across the boundary, on the CPU: include/rtx.h (parsed
as tests/test_abi.py parses it), the Python binding, the library's exports and a C99 translation unit agree on them; rtx_half_bound
against the restatement of tests/restate_half.py, and its zeros."""
import ctypes as C
import os
import subprocess

import restate_half as RH
import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_half_bound", "rtx_half_words", "rtx_update_half"]

DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    size_t (*a)(int, size_t, size_t) = rtx_half_bound;
    int (*b)(rtx_ctx*, int, size_t, size_t, const void*, void*, size_t, size_t*) = rtx_half_words;
    int (*c)(rtx_ctx*, const rtx_params*, int, double, int, void*, size_t, size_t*) = rtx_update_half;
    printf("%d %d\n", (int)RTX_STAT_HALF_FRAMES, a != 0 && b != 0 && c != 0);
    printf("%lu %lu %lu\n", (unsigned long)rtx_half_bound(RTX_RGB_PIXEL, 160, 50), (unsigned long)rtx_half_bound(RTX_BIT_PIXEL, 160, 50),
           (unsigned long)rtx_half_bound(RTX_SDL, 160, 50));
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
    assert e["RTX_STAT_HALF_FRAMES"] == R.STAT_HALF_FRAMES
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    assert len(stats) == len(set(stats)) and not set(stats) & set(opts)
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_half_bound"][1] is C.c_size_t and sig["rtx_half_bound"][2] == [C.c_int, C.c_size_t, C.c_size_t]
    assert sig["rtx_half_words"][1] is C.c_int
    assert sig["rtx_half_words"][2] == [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert sig["rtx_update_half"][1] is C.c_int
    assert sig["rtx_update_half"][2] == [C.c_void_p, C.POINTER(R.Params), C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
    for m in ("half_words", "update_half"):
        assert callable(getattr(R.Context, m))
    assert callable(R.half_bound)


def test_every_declaration_states_its_reference_counterpart_and_what_is_out_of_scope():
    text = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    for n in NEW + ["RTX_STAT_HALF_FRAMES"]:
        at = text.index(n + ("(" if n.startswith("rtx_") else " ="))
        around = text[max(0, at - 1500):at + 700]
        assert "No reference counterpart" in around and "RayTracing.cu:256,476" in around, n
    at = text.index("size_t rtx_half_bound(")
    before = text[at - 4500:at]
    for phrase in ("THE RULE", "E2 96 80", "Out of scope", "pipelined", "RTX_OPT_UPDATE_HOST_WRITE", "RTX_OPT_GROUP_UPDATE", "delta frames of half-block",
                   "a space in place of the glyph"):
        assert phrase in before, phrase


def test_the_header_still_compiles_as_c99(tmp_path):
    R = U.pkg()
    inc = os.path.join(U.ROOT, "include")
    src = tmp_path / "decl.c"
    src.write_text(DECL_C)
    exe = str(tmp_path / "decl")
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    assert os.path.exists(so), "run build() first"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L", R.PKG_DIR, "-lrtx_hip",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.check_output([exe], text=True).split()
    assert out[:2] == [str(R.STAT_HALF_FRAMES), "1"]
    assert [int(v) for v in out[2:]] == [50 * (159 * 41 + 1), 50 * (159 * 25 + 1), 0]


def test_the_library_exports_the_three_symbols():
    R = U.pkg()
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("rtx_"))
    assert exported == header_functions()
    for n in NEW:
        assert n in exported, n


def test_half_bound_against_the_restatement_and_its_zeros():
    R = U.pkg()
    for mode in (R.BIT_ASCII, R.BIT_PIXEL, R.RGB_ASCII, R.RGB_PIXEL, R.RGB_NORMALS):
        for (w, h) in ((1, 3), (2, 1), (2, 5), (3, 1), (33, 31), (32, 32), (41, 25), (1025, 1), (1024, 3), (257, 260), (160, 50), (1920, 540),
                       ((1 << 31) - 1, 1000), (100000, (1 << 30) - 1)):
            assert R.half_bound(mode, w, h) == RH.half_bound(mode, w, h) > 0, (mode, w, h)
    big = (1 << 31) - 1
    for bad in ((R.SDL, 10, 10), (-1, 10, 10), (6, 10, 10), (R.RGB_PIXEL, 0, 10), (R.RGB_PIXEL, 10, 0),
                (R.RGB_PIXEL, 1 << 31, 10),        # w of 2^31
                (R.RGB_PIXEL, 10, 1 << 30),        # 2h of 2^31
                (R.RGB_PIXEL, big, (1 << 30) - 1), # a product that does not fit size_t
                (R.BIT_PIXEL, big, (1 << 30) - 1)):
        assert R.half_bound(*bad) == 0, bad


def test_calls_without_a_context_are_refused():
    R = U.pkg()
    n = C.c_size_t(7)
    p = R.Params()
    assert R.lib().rtx_half_words(None, R.RGB_PIXEL, 4, 4, None, None, 0, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_update_half(None, C.byref(p), R.RGB_PIXEL, 0.0, 0, None, 0, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert n.value == 7
