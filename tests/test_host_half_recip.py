"""csrc/rtx_unit.hpp -- divTwoA = 1 / (2 a) of nearly-unit squared lengths as an integer rule -- against host 2.0f * x and 1.0f / x
(IEEE), compiled as host-only C++ without FMA contraction and run under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/test_half_recip.cpp): every offset of the range the header claims, the first failing offset on either side equal to
the header's constants, and the shipped window inside that range.  No HIP, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_half_recip_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_half_recip")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_half_recip.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0 and "all half-reciprocal host checks passed" in p.stdout, p.stdout[-4000:]
