"""rtxplan::edit_effect (csrc/rtx_plan.hpp) without a GPU: what the two result words of an edit in place (rtx_scene_set_spheres) do to
the cell lists, the dispatch orders and the physics bound.  tests/host/test_scene_edit.cpp, compiled as host-only C++ and run under
AddressSanitizer + UndefinedBehaviorSanitizer with the g++ line of tests/test_host_plan.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edit_effect_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_scene_edit")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_scene_edit.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all scene edit planning tests passed" in p.stdout, p.stdout[-4000:]
