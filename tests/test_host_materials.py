"""The book of per-object surface attributes on the host (tests/host/test_materials.cpp under ASan + UBSan): csrc/rtx_materials.hpp's
operations in random sequences against a naive model, refused calls that change nothing, removal under rtxplan's renumbering
rule, the layout of the device copies with and without a sorted index, and which generation a recorded graph is stale against."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_materials_book_and_layouts_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_materials")
    # -ffp-contract=off: as the library is built (rtx_refract.hpp is among the headers)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_materials.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "all materials tests passed" in p.stdout, p.stdout[-4000:]
