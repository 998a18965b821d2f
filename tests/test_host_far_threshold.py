"""csrc/rtx_far.hpp -- the far distance folded into a table plane's direction test -- against the host's IEEE division, compiled as
host-only C++ without FMA contraction and run under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/test_far_threshold.cpp): on a grid of (num, far) over every exponent, both signs, binade-edge significands and the
special values, every dn the new test drops either was dropped by the parent's test or has num / dn > far, every dn the
parent's test drops is still dropped, and the windows do contain dropped lanes.  No HIP, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_far_threshold_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_far_threshold")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_far_threshold.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "all far-threshold host checks passed" in p.stdout, p.stdout[-4000:]
