"""Mirrors that see mirrors (RTX_OPT_REFLECT_DEPTH), the parts that need no GPU:
  * csrc/rtx_reflect.hpp compiled as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer against float64 for the bundles
    deep levels make (tests/host/test_reflect_bound_deep.cpp): origins spread over several objects, near-90-degree cones, rays
    that leave a sphere tangentially; no reachable sphere is ever culled;
  * the new constants in the header as plain C99 and as C++, and in the Python binding;
  * the console example's `b` key (reflection depth 1 -> 2 -> 3 -> 4 -> 1)."""
import os
import shutil
import subprocess

import pytest

import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reflect_bound_never_culls_a_reachable_sphere_for_deep_bundles(tmp_path):
    exe = str(tmp_path / "test_reflect_bound_deep")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_reflect_bound_deep.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all deep reflect bound tests passed" in p.stdout, p.stdout[-4000:]


DECL_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    int depth[RTX_MAX_REFLECT_DEPTH]; /* a constant expression */
    printf("%d %d %d %d\n", (int)RTX_OPT_REFLECT_DEPTH, (int)RTX_OPT_REFLECT_DEPTH_CHECK, (int)RTX_STAT_REFLECT_RAYS,
           (int)(sizeof depth / sizeof depth[0]));
    return 0;
}
"""


@pytest.mark.parametrize("lang", ["c99", "c++"])
def test_reflect_depth_constants_compile_as_c99_and_cxx(tmp_path, lang):
    cc = "gcc" if lang == "c99" else "g++"
    if shutil.which(cc) is None:
        pytest.skip("needs " + cc)
    src = tmp_path / ("decl.c" if lang == "c99" else "decl.cpp")
    src.write_text(DECL_C)
    exe = str(tmp_path / "decl")
    std = ["-std=c99", "-pedantic"] if lang == "c99" else ["-std=c++11"]
    subprocess.check_call([cc] + std + ["-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).split()
    R = U.pkg()
    assert out == ["26", "27", "138", "4"]
    assert (R.OPT_REFLECT_DEPTH, R.OPT_REFLECT_DEPTH_CHECK, R.STAT_REFLECT_RAYS, R.MAX_REFLECT_DEPTH) == (26, 27, 138, 4)
    # the earlier constants of the path keep their values
    assert (R.OPT_REFLECT_CHECK, R.STAT_REFLECT_FRAMES, R.STAT_REFLECT_LONGEST_LIST) == (22, 120, 121)


def test_console_b_key_cycles_bounces_on_a_pty():
    """examples/console_engine.cpp --keys-only: `b` (and `B`) decode to the bounce cycle; `k` stays "other"."""
    import pty
    import select
    import time
    R = U.pkg()
    exe = os.path.join(R.PKG_DIR, "console_engine")
    if not os.path.exists(exe):
        R.build()
    try:
        master, slave = pty.openpty()
    except OSError:
        pytest.skip("no pty devices here")
    proc = subprocess.Popen([exe, "--keys-only"], stdin=slave, stdout=slave, stderr=subprocess.PIPE, close_fds=True)
    out = bytearray()
    try:
        for raw, name in ((b"", "raw 1"), (b"b", "key bounces"), (b"B", "key bounces"), (b"k", "key other"), (b"m", "key mirrors"), (b"x", "key quit")):
            n = out.count(b"\n")
            if raw:
                os.write(master, raw)
            end = time.time() + 20
            while (out.count(b"\n") == n or name.encode() not in bytes(out).replace(b"\r\n", b"\n").rstrip().split(b"\n")[-1]) and time.time() < end:
                r, _, _ = select.select([master], [], [], 0.2)
                if r:
                    out.extend(os.read(master, 4096))
            assert bytes(out).replace(b"\r\n", b"\n").rstrip().split(b"\n")[-1] == name.encode(), (raw, bytes(out)[-80:])
        assert proc.wait(timeout=10) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        os.close(master)
        os.close(slave)
