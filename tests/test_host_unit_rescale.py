"""csrc/rtx_unit.hpp -- the rescale factor of nearly-unit squared lengths as an integer rule -- against host sqrtf and 1.0f / x
(IEEE), compiled as host-only C++ without FMA contraction and run under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/test_unit_rescale.cpp): every offset of the shipped window, a margin of 64 on each side, the whole range the header
claims, and that nothing outside the window is answered from the table.  No HIP, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_unit_rescale_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_unit_rescale")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_unit_rescale.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0 and "all unit-rescale host checks passed" in p.stdout, p.stdout[-4000:]
