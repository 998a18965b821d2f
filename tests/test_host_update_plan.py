"""rtxplan::plan_update (csrc/rtx_plan.hpp) -- the form of a call of the Update family: its refusal, whether the physics step precedes
it, what is traced and encoded, which ways of delivering are tried -- compiled as host-only C++ and run under AddressSanitizer +
UndefinedBehaviorSanitizer over the whole request space, against the entry points' conditions written out one by one
(tests/host/test_update_plan.cpp).  No HIP, no GPU: the decision is pure."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_update_plans_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_update_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_update_plan.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "update plans passed" in p.stdout, p.stdout[-4000:]
