"""The far cut of csrc/rtx_far.hpp on the device (tests/gpu_checks/far_check.hip): for each (num, far) below, one launch over all
2^32 fp32 bit patterns of dn = Dot(direction, n) compares the new direction test followed by div_cr with the parent's expressions
(dn > 0 || |dn| < FLT_EPSILON, then div_cr): 0 mismatches in whether the pixel shows the plane and, where it does, in t1; every
lane the far cut alone drops has num / dn > far by the compiler's IEEE division; and the number of such lanes is the CPU's -- the
floats dn with cut < dn <= -FLT_EPSILON, from the cut the host evaluation of the same header gives and from a numpy float32
restatement of the rule.

The pairs are drawn from the grid of tests/host/test_far_threshold.cpp: the bench's floor (num -30, far 250) and the directed
scene's far 120; the same scaled by 1e5 and 1e-18; a subnormal num under a far in FLT_MIN's binade; a far one float below the
no-hit distance with a huge num; and a cut only a few floats below -FLT_EPSILON.  The pairs of the second list are ones the
rule must leave to the parent's test (the floor scaled by 1e18, whose far lies past the no-hit distance; far +inf, 0, negative, NaN, FLT_MAX, subnormal, at the no-hit distance; num >= 0; an
overflowing and an underflowing quotient): the launch must count no dropped lane at all."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32

EPS_BITS = 0xB4000000          # -FLT_EPSILON
NO_HIT = f32(99999999.0)
SUBNORMAL = float(np.uint32(0x007FFFFF).view(f32))

CUT_PAIRS = [(-30.0, 250.0), (-30.0, 120.0), (-3e6, 2.5e7), (-3e-17, 2.5e-16), (-1e-39, 2e-38),
             (-3e38, float(np.nextafter(NO_HIT, f32(0)))), (-1.1920943e-07, 1.0)]
PARENT_PAIRS = [(-3e19, 2.5e20), (-30.0, float("inf")), (-30.0, 0.0), (-30.0, -250.0), (-30.0, float("nan")), (-30.0, 3.4028234663852886e38),
                (-30.0, SUBNORMAL), (-30.0, float(NO_HIT)), (30.0, 250.0), (0.0, 250.0), (-3.4028234663852886e38, 0.5), (-1e-30, 250.0)]


def _bits(x):
    return int(np.array(x, dtype=f32).view(np.uint32))


def restated_cut(num, far):
    """rtx_far.hpp's far_dir_cut in numpy float32 (each operation rounded to fp32)."""
    num, far = f32(num), f32(far)
    cut = f32(-1.1920928955078125e-7)
    with np.errstate(all="ignore"):
        if num < 0 and far >= f32(1.17549435e-38) and far < NO_HIT:
            q = f32(-num / far)
            if q <= f32(3.4028234663852886e38):
                thr = f32(-f32(q * f32(1.0 - 2.0 ** -21)))
                if thr < cut:
                    cut = thr
    return cut


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    path = os.path.join(HERE, "gpu_checks", "libfar_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    so = C.CDLL(path)
    so.rtx_check_far_cut_exhaustive.restype = C.c_longlong
    so.rtx_check_far_cut_exhaustive.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]
    so.rtx_far_cut_host.restype = C.c_float
    so.rtx_far_cut_host.argtypes = [C.c_float, C.c_float]
    return so


def _run(lib, num, far):
    first, dropped, cut = C.c_uint(0), C.c_ulonglong(0), C.c_uint(0)
    bad = lib.rtx_check_far_cut_exhaustive(num, far, C.byref(first), C.byref(dropped), C.byref(cut))
    host_cut = _bits(lib.rtx_far_cut_host(num, far))
    print("num %r far %r: device cut 0x%08x host cut 0x%08x restated 0x%08x, dropped %d, mismatches %d" % (
        num, far, cut.value, host_cut, _bits(restated_cut(num, far)), dropped.value, bad))
    assert bad == 0, "num %r far %r: %d of 2^32 dn differ, first bit pattern 0x%08x" % (num, far, bad, first.value)
    assert cut.value == host_cut == _bits(restated_cut(num, far))
    # the CPU's count: negative floats are ordered by their bit patterns, and the lanes dropped by the far cut alone are
    # the dn with cut < dn <= -FLT_EPSILON
    assert dropped.value == host_cut - EPS_BITS
    return dropped.value


@pytest.mark.parametrize("num,far", CUT_PAIRS)
def test_far_cut_changes_nothing_visible_and_drops_what_the_cpu_counts(lib, num, far):
    assert _run(lib, num, far) > 0


@pytest.mark.parametrize("num,far", PARENT_PAIRS)
def test_pairs_outside_the_rule_keep_the_parents_test(lib, num, far):
    assert _run(lib, num, far) == 0
