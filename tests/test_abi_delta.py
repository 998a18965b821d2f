"""rtx_delta_bound, rtx_delta_words, rtx_update_delta, the two delta enums and RTX_STAT_DELTA_* across the boundary, on the CPU:
include/rtx.h (parsed as tests/test_abi.py parses it), the Python binding and a C99 translation unit agree on them; rtx_delta_bound
against the formula of the issue, worked out here in Python."""
import ctypes as C
import os
import subprocess

import util as U
from test_abi import header_functions
from test_abi_reflect_shadows import header_enums

NEW = ["rtx_delta_bound", "rtx_delta_words", "rtx_update_delta"]
STATS = {"RTX_STAT_DELTA_FRAMES": 151, "RTX_STAT_DELTA_KEYFRAMES": 152, "RTX_STAT_DELTA_CELLS": 153, "RTX_STAT_DELTA_RUNS": 154}

DECL_C = r"""
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    size_t (*a)(int, size_t, size_t) = rtx_delta_bound;
    int (*b)(rtx_ctx*, int, size_t, size_t, const void*, const void*, void*, size_t, size_t*) = rtx_delta_words;
    int (*c)(rtx_ctx*, const rtx_params*, int, double, int, unsigned, void*, size_t, size_t*, int*) = rtx_update_delta;
    enum rtx_delta_flags f = RTX_DELTA_KEYFRAME;
    enum rtx_delta_kind k = RTX_DELTA_DIFF;
    printf("%d %d %d %d %d %d %d %d %d\n", (int)RTX_DELTA_DEFAULT, (int)f, (int)RTX_DELTA_KEY, (int)k, (int)RTX_STAT_DELTA_FRAMES,
           (int)RTX_STAT_DELTA_KEYFRAMES, (int)RTX_STAT_DELTA_CELLS, (int)RTX_STAT_DELTA_RUNS, a != 0 && b != 0 && c != 0);
    printf("%lu %lu\n", (unsigned long)rtx_delta_bound(RTX_RGB_ASCII, 400, 150), (unsigned long)rtx_delta_bound(RTX_SDL, 400, 150));
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
    for k, v in STATS.items():
        assert e[k] == v == getattr(R, k[4:]), k
    stats = [v for k, v in e.items() if k.startswith("RTX_STAT_")]
    assert len(stats) == len(set(stats)) and max(stats) == 154 and e["RTX_STAT_SCENE_REMOVED"] == 150
    assert (e["RTX_DELTA_DEFAULT"], e["RTX_DELTA_KEYFRAME"]) == (0, 1) == (R.DELTA_DEFAULT, R.DELTA_KEYFRAME)
    assert (e["RTX_DELTA_KEY"], e["RTX_DELTA_DIFF"]) == (0, 1) == (R.DELTA_KEY, R.DELTA_DIFF)
    sig = {s[0]: s for s in R._SIGNATURES}
    assert sig["rtx_delta_bound"][1] is C.c_size_t and sig["rtx_delta_bound"][2] == [C.c_int, C.c_size_t, C.c_size_t]
    assert sig["rtx_delta_words"][1] is C.c_int
    assert sig["rtx_delta_words"][2] == [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
    assert sig["rtx_update_delta"][1] is C.c_int
    assert sig["rtx_update_delta"][2] == [C.c_void_p, C.POINTER(R.Params), C.c_int, C.c_double, C.c_int, C.c_uint, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    for m in ("delta_words", "update_delta"):
        assert callable(getattr(R.Context, m))
    assert callable(R.delta_bound)


def test_every_declaration_states_its_reference_counterpart():
    text = open(os.path.join(U.ROOT, "include", "rtx.h")).read()
    for n in NEW + list(STATS):
        at = text.index(n + ("(" if n.startswith("rtx_") else " ="))
        around = text[max(0, at - 2500):at + 700]
        assert "No reference counterpart" in around and "PrintMachine.cpp:257-306" in around and "RayTracingManager.cu:150" in around, n
    # what is out of scope is said where the calls are declared
    at = text.index("enum rtx_delta_flags")
    before = text[at - 3500:at]
    for phrase in ("Out of scope", "RTX_OPT_UPDATE_HOST_WRITE", "pipelined", "RTX_OPT_GROUP_UPDATE", "gaps", "automatically"):
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
    assert out[:9] == ["0", "1", "0", "1", "151", "152", "153", "154", "1"]
    assert [int(v) for v in out[9:]] == [formula_bound(20, 400, 150), 0]


def test_the_library_exports_exactly_the_header():
    R = U.pkg()
    so = os.path.join(R.PKG_DIR, "librtx_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("rtx_"))
    assert exported == header_functions()
    for n in NEW:
        assert n in exported, n


def cup_length(row, col):
    return len("\x1b[%d;%dH" % (row + 1, col + 1))


def formula_bound(S, w, h):
    """Per row the largest S c + cup r over c changed cells in r runs, r <= c and r <= (w - 1) - c + 1, the escape at the row's
    longest; summed over the rows; and no less than the key frame's S w h.  Every c is tried."""
    total = 0
    per_cup = {}  # (rows with escapes of one length share their maximum)
    for row in range(h):
        cup = cup_length(row, w - 2) if w >= 2 else 0
        if cup not in per_cup:
            per_cup[cup] = max(S * c + cup * min(c, (w - 1) - c + 1) for c in range(0, w))
        total += per_cup[cup]
    return max(total, S * w * h)


def test_delta_bound_against_the_formula():
    R = U.pkg()
    for mode, S in ((R.BIT_ASCII, 12), (R.BIT_PIXEL, 12), (R.RGB_ASCII, 20), (R.RGB_PIXEL, 20), (R.RGB_NORMALS, 20)):
        for (w, h) in ((1, 5), (2, 7), (3, 1), (37, 61), (1030, 3), (1001, 101), (400, 150), (12, 1000), (1920, 1080)):
            assert R.delta_bound(mode, w, h) == formula_bound(S, w, h), (mode, w, h)
    # at the limits an escape (14 bytes) is longer than a 12-byte record: alternating cells are then longer than a key frame;
    # 20-byte records never are
    assert R.delta_bound(R.BIT_ASCII, 100000, 99999) == formula_bound(12, 100000, 99999) > 12 * 100000 * 99999
    assert R.delta_bound(R.RGB_ASCII, 100000, 99999) == 20 * 100000 * 99999 == formula_bound(20, 100000, 99999)
    assert R.delta_bound(R.RGB_ASCII, 1001, 101) == 20 * 1001 * 101
    for bad in ((R.SDL, 10, 10), (-1, 10, 10), (6, 10, 10), (R.RGB_ASCII, 0, 10), (R.RGB_ASCII, 10, 0), (R.RGB_ASCII, 100001, 10),
                (R.RGB_ASCII, 10, 100000)):
        assert R.delta_bound(*bad) == 0, bad


def test_calls_without_a_context_are_refused():
    R = U.pkg()
    n = C.c_size_t(7)
    k = C.c_int(7)
    p = R.Params()
    assert R.lib().rtx_delta_words(None, R.RGB_ASCII, 4, 4, None, None, None, 0, C.byref(n)) == R.ERR_INVALID_ARGUMENT
    assert R.lib().rtx_update_delta(None, C.byref(p), R.RGB_ASCII, 0.0, 0, 0, None, 0, C.byref(n), C.byref(k)) == R.ERR_INVALID_ARGUMENT
    assert (n.value, k.value) == (7, 7)
