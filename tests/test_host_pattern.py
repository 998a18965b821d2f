"""Checker patterns on the host (tests/host/test_pattern.cpp under ASan + UBSan): csrc/rtx_pattern.hpp's pattern_odd -- the expression
the shade kernels run -- against float64 and on the rule's exact cases, the table's validation and packing, rtxplan::plan_shading
with n_patterned over the cross product of its request, and the slots under rtxplan::plan_removal's renumbering."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pattern_rule_planner_and_removal_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_pattern")
    # -ffp-contract=off: the rule is stated without contraction, and the library is built that way
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_pattern.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all pattern tests passed" in p.stdout, p.stdout[-4000:]
