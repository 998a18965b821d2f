"""rtxplan::removal_fault, index_after_removal and plan_removal (csrc/rtx_plan.hpp) without a GPU: the host part of
rtx_scene_remove_objects -- the checked ascending set, the new kind_of / local_of, the per-kind lists of removed local indices and the
rule that renumbers the survivors -- against a model that erases the objects one by one.  tests/host/test_scene_remove.cpp, compiled
as host-only C++ and run under AddressSanitizer + UndefinedBehaviorSanitizer with the g++ line of tests/test_host_scene_edit.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_removal_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_scene_remove")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_scene_remove.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all scene removal planning tests passed" in p.stdout, p.stdout[-4000:]
