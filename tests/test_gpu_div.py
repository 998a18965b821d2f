"""GPU proof that the short correctly rounded division of the plane test (rtx_device.hpp: div_cr) returns exactly the bits of
the compiler's IEEE expansion of num / den: every pair of significands (which, inside the safe range, fixes the result for all
exponents and signs), a grid of edge values including the range guard's boundaries, and 2^32 random pairs of bit patterns."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    path = os.path.join(HERE, "gpu_checks", "libdiv_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    lib = C.CDLL(path)
    lib.rtx_check_div.restype = C.c_longlong
    lib.rtx_check_div.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return lib


@pytest.mark.parametrize("which,name", [(0, "all 2^46 significand pairs"), (1, "edge-value grid"), (2, "2^32 random bit patterns")])
def test_div_cr_is_bit_identical_to_ieee_division(checker, which, name):
    first = C.c_ulonglong(0)
    bad = checker.rtx_check_div(which, C.byref(first))
    assert bad == 0, "div_cr(num, den) != num / den on %d pairs of the %s; first num 0x%08x den 0x%08x" % (
        bad, name, first.value >> 32, first.value & 0xffffffff)
