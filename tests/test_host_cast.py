"""Objects that cast no shadow on the host (tests/host/test_cast.cpp under ASan + UBSan): the values rtx_scene_set_shadow_casting
accepts and refuses, the book's fifth column (counts, the fifth generation, all or nothing, removal, clear, the three orders under a
sorted order that is no identity, stale_fault's order) and plan_shading with n_shadowless 0 and not 0 over the cross product of its
request: identical plans."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cast_column_book_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_cast")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_cast.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "all cast tests passed" in p.stdout, p.stdout[-4000:]
