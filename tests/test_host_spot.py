"""The host side of the spot lights (rtx_scene_set_spots) without a GPU: csrc/rtx_lights.hpp (what a call accepts, all or nothing,
with the offending index, and the packing: the axis normalised in double, inv by one fp32 division) and csrc/rtx_spot.hpp (the rule
the kernels run: w exactly 1 for a point light, 0 at and beyond cos_outer, 1 at and within cos_inner, 0 for a NaN, monotone over
2^16 values of c) under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_spot.cpp, a program of its own)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_spot_rule_and_packing_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_spot")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_spot.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all spot tests passed" in p.stdout, p.stdout[-4000:]
