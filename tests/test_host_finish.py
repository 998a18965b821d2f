"""Surface finishes on the host (tests/host/test_finish.cpp under ASan + UBSan): csrc/rtx_finish.hpp's power -- the expression the
shade kernels run -- against pow32 at m = 5, x at m = 0 and float64 pow within 1 ulp elsewhere, the values a call accepts, the book
they are stored in (counts, generations, all or nothing, -0, removal, the three orders) and plan_shading with n_finished over the
cross product of its request."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_finish_rule_book_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_finish")
    # -ffp-contract=off: the rule is stated without contraction, and the library is built that way
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_finish.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "all finish tests passed" in p.stdout, p.stdout[-4000:]
