"""Scene3D::RemoveObject / RemoveObjects of include/rtx_compat.hpp on the GPU: tests/host/compat_remove.cpp, host C++ over the C ABI,
built against the library and run once -- the facade's own plane indices follow the renumbering rule of rtx_scene_remove_objects."""
import os
import subprocess

import pytest

import util as U

pytestmark = pytest.mark.gpu


def test_the_facade_renumbers_its_planes(tmp_path):
    R = U.pkg()
    exe = str(tmp_path / "compat_remove")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(U.ROOT, "include"),
                           os.path.join(U.ROOT, "tests", "host", "compat_remove.cpp"), "-o", exe, "-L", R.PKG_DIR, "-lrtx_hip", "-pthread",
                           "-Wl,-rpath," + R.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "facade removal ok" in p.stdout, p.stdout[-4000:]
