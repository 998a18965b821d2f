"""rtx_half_delta_bound, rtx_half_delta_words, rtx_update_half_delta and their two counters across the boundary, on the CPU:
include/rtx.h (parsed as tests/test_abi.py parses it), the Python binding, the library's exports and a C99 translation unit agree on
them; rtx_half_delta_bound against the restatement of tests/restate_half_delta.py, and its zeros."""
import ctypes as C
import os
import subprocess

import restate_half_delta as RD
import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_half_delta_bound", "rtx_half_delta_words", "rtx_update_half_delta"]
NEW_STATS = ["RTX_STAT_HALF_DELTA_FRAMES", "RTX_STAT_HALF_DELTA_KEYFRAMES"]

DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    size_t (*a)(int, size_t, size_t) = rtx_half_delta_bound;
    int (*b)(rtx_ctx*, int, size_t, size_t, const void*, const void*, void*, size_t, size_t*) = rtx_half_delta_words;
    int (*c)(rtx_ctx*, const rtx_params*, int, double, int, unsigned, void*, size_t, size_t*, int*) = rtx_update_half_delta;
    printf("%d %d %d\n", (int)RTX_STAT_HALF_DELTA_FRAMES, (int)RTX_STAT_HALF_DELTA_KEYFRAMES, a != 0 && b != 0 && c != 0);
    printf("%lu %lu %lu\n", (unsigned long)rtx_half_delta_bound(RTX_RGB_PIXEL, 160, 50), (unsigned long)rtx_half_delta_bound(RTX_BIT_PIXEL, 160, 50),
           (unsigned long)rtx_half_delta_bound(RTX_SDL, 160, 50));
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
    assert e["RTX_STAT_HALF_DELTA_FRAMES"] == R.STAT_HALF_DELTA_FRAMES == 96
    assert e["RTX_STAT_HALF_DELTA_KEYFRAMES"] == R.STAT_HALF_DELTA_KEYFRAMES == 95
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    opts = [v for k, v in e.items() if k.startswith("RTX_OPT_")]
    assert len(stats) == len(set(stats)) and not set(stats) & set(opts)
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_half_delta_bound"][1] is C.c_size_t and sig["rtx_half_delta_bound"][2] == [C.c_int, C.c_size_t, C.c_size_t]
    assert sig["rtx_half_delta_words"][1] is C.c_int
    assert sig["rtx_half_delta_words"][2] == [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.POINTER(C.c_size_t)]
    assert sig["rtx_update_half_delta"][1] is C.c_int
    assert sig["rtx_update_half_delta"][2] == [C.c_void_p, C.POINTER(R.Params), C.c_int, C.c_double, C.c_int, C.c_uint, C.c_void_p, C.c_size_t,
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    for m in ("half_delta_words", "update_half_delta"):
        assert callable(getattr(R.Context, m))
    assert callable(R.half_delta_bound)


def test_every_declaration_states_its_reference_counterpart_and_what_is_out_of_scope():
    text = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    for n in NEW + NEW_STATS:
        at = text.index(n + ("(" if n.startswith("rtx_") else " ="))
        around = text[max(0, at - 1800):at + 700]
        for cite in ("No reference counterpart", "RayTracing.cu:256,476", "PrintMachine.cpp:257-306", "RayTracingManager.cu:150"):
            assert cite in around, (n, cite)
    # the declarations stand behind rtx_update_half and in front of rtx_ansi256_map
    assert text.index("int rtx_update_half(") < text.index("size_t rtx_half_delta_bound(") < text.index("int rtx_half_delta_words(") \
        < text.index("int rtx_update_half_delta(") < text.index("int rtx_ansi256_map(")
    at = text.index("size_t rtx_half_delta_bound(")
    before = text[at - 4200:at]
    for phrase in ("THE RULE", "E2 96 80", "Out of scope", "tracking the terminal's SGR state", "bridging short unchanged gaps", "choosing a key frame",
                   "pipelined", "RTX_OPT_UPDATE_HOST_WRITE", "RTX_OPT_GROUP_UPDATE", "whatever SGR state"):
        assert phrase in before, phrase
    # the half-block rule still names them, as a family of their own
    at = text.index("size_t rtx_half_bound(")
    assert "delta frames of half-block" in text[at - 4500:at] and "a call family of their own" in text[at - 4500:at]
    # the two launch counters say that they serve both kinds
    for n in ("RTX_STAT_DELTA_CELLS", "RTX_STAT_DELTA_RUNS"):
        at = text.index(n + " =")
        assert "either kind" in text[at:at + 900], n


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
    assert out[:3] == ["96", "95", "1"]
    assert [int(v) for v in out[3:]] == [326391, 199191, 0]


def test_the_library_exports_the_three_symbols():
    R = U.pkg()
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("rtx_"))
    assert exported == header_functions()
    for n in NEW:
        assert n in exported, n


def test_half_delta_bound_against_the_restatement_and_its_zeros():
    R = U.pkg()
    for mode in (R.BIT_ASCII, R.BIT_PIXEL, R.RGB_ASCII, R.RGB_PIXEL, R.RGB_NORMALS):
        for (w, h) in ((1, 3), (2, 1), (2, 5), (3, 1), (33, 31), (32, 32), (41, 25), (1025, 1), (1024, 3), (257, 260), (120, 101), (160, 50),
                       (1920, 540), (2100, 1), (100000, 99999)):
            assert R.half_delta_bound(mode, w, h) == RD.half_delta_bound(mode, w, h) >= R.half_bound(mode, w, h) > 0, (mode, w, h)
    assert R.half_delta_bound(R.RGB_PIXEL, 160, 50) == 326391 and R.half_delta_bound(R.BIT_PIXEL, 160, 50) == 199191
    for bad in ((R.SDL, 10, 10), (-1, 10, 10), (6, 10, 10), (R.RGB_PIXEL, 0, 10), (R.RGB_PIXEL, 10, 0),
                (R.RGB_PIXEL, 100001, 10),            # w - 1 above 99999
                (R.RGB_PIXEL, 10, 100000),            # h above 99999
                (R.RGB_PIXEL, 1 << 31, 10), (R.BIT_PIXEL, 10, 1 << 30), (R.RGB_PIXEL, (1 << 64) - 1, (1 << 64) - 1)):
        assert R.half_delta_bound(*bad) == 0, bad


def test_calls_without_a_context_are_refused():
    R = U.pkg()
    n, kind = C.c_size_t(7), C.c_int(9)
    p = R.Params()
    assert R.lib().rtx_half_delta_words(None, R.RGB_PIXEL, 4, 4, None, None, None, 0, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_update_half_delta(None, C.byref(p), R.RGB_PIXEL, 0.0, 0, 0, None, 0, C.byref(n), C.byref(kind)) == R.ERR_INVALID_ARGUMENT
    assert n.value == 7 and kind.value == 9
