"""Step 4 of csrc/rtx_grid.hpp without a GPU: the world grid's lists, built with the ray queries' bound, hold every sphere the
shadow test (segment_hits_sphere) reports for a walkable segment, in a cell the walk with d = toL and tmax = 1 visits before it ends.
tests/host/test_grid_shadow_bound.cpp, compiled as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer with the g++ line
of tests/test_host_query.py::test_grid_bound_and_planner, checks over a million seeded segments against float64."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shadow_test_is_covered_by_the_grid(tmp_path):
    exe = str(tmp_path / "test_grid_shadow_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall",
                           "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_grid_shadow_bound.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all shadow grid bound tests passed" in p.stdout, p.stdout[-4000:]
    walked = int(p.stdout.split("walked")[1].split()[0])
    assert walked >= 1000000, p.stdout[-400:]
    print(p.stdout[-600:])
