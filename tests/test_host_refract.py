"""Glass on the host (tests/host/test_refract.cpp under ASan + UBSan): csrc/rtx_refract.hpp's through_sphere -- the expressions
secondary_ray runs on the device -- against two float64 Snell refractions with a real chord intersection, normal incidence and
ior = 1, NaN inputs, and the values a call accepts (the book they are stored in: tests/host/test_materials.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_refraction_rule_and_books_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_refract")
    # -ffp-contract=off: the rule is stated without contraction, and the library is built that way
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_refract.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "all refract tests passed" in p.stdout, p.stdout[-4000:]
