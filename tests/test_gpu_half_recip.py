"""The two exhaustive proofs of tests/gpu_checks/half_check.hip, each one launch over all 2^32 fp32 bit patterns:

1. half_recip(a) (rtx_device.hpp: divTwoA from the table of rtx_unit.hpp inside its window, the generic expansion outside) returns
   the bits of 1.0f / (2.0f * a), and the rescale factor it reads beside it those of 1.0f / sqrtf(a), for every a.
2. u8_clamped(x), a colour channel's byte without the float clamp, equals u8_sat(minf(255.0f, x)), the expression it replaced,
   for every x -- NaNs, negatives, infinities and values past the u32 range included."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# rtx_unit.hpp: the window of bit offsets from 1.0f that the tables answer
K_MIN, K_MAX = -12, 3


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    path = os.path.join(HERE, "gpu_checks", "libhalf_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    so = C.CDLL(path)
    for fn in (so.rtx_check_half_recip_exhaustive, so.rtx_check_half_recip_poisoned, so.rtx_check_channel_byte_exhaustive):
        fn.restype = C.c_longlong
        fn.argtypes = [C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)]
    return so


def test_half_recip_is_bit_identical_on_all_inputs(lib):
    first, tabled = C.c_uint(0), C.c_ulonglong(0)
    bad = lib.rtx_check_half_recip_exhaustive(C.byref(first), C.byref(tabled))
    assert bad == 0, "half_recip(a) != 1.0f/(2.0f*a) on %d inputs, first bit pattern 0x%08x" % (bad, first.value)
    assert tabled.value == K_MAX - K_MIN + 1 == 16   # the table answered exactly its window: the walk did go through it


def test_half_recip_answers_exactly_its_window_from_the_table(lib):
    """The same walk with one bit of every table entry flipped: the inputs that come out wrong are those the helper took from
    the table -- counted from the path it took, where the test above counts slots."""
    first, tabled = C.c_uint(0), C.c_ulonglong(0)
    bad = lib.rtx_check_half_recip_poisoned(C.byref(first), C.byref(tabled))
    assert bad == K_MAX - K_MIN + 1 == 16
    assert first.value == 0x3F800000 + K_MIN      # the lowest of them is the window's lower end


def test_channel_byte_without_the_float_clamp_is_the_clamped_byte_on_all_inputs(lib):
    first, saturated = C.c_uint(0), C.c_ulonglong(0)
    bad = lib.rtx_check_channel_byte_exhaustive(C.byref(first), C.byref(saturated))
    assert bad == 0, "u8_clamped(x) != u8_sat(minf(255, x)) on %d inputs, first bit pattern 0x%08x" % (bad, first.value)
    # the byte 255 comes from exactly the positive floats from 255.0f (0x437f0000) up to +inf (0x7f800000): the walk saw them
    assert saturated.value == 0x7F800000 - 0x437F0000 + 1

