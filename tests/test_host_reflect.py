"""The mirror ABI and the sphere bound of the mirror pass, without a GPU:
  * csrc/rtx_reflect.hpp compiled as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_reflect_bound.cpp):
    millions of seeded random cases, no sphere within reach of a ray of the bundle ever culled;
  * the new declarations and constants in the header as plain C99 and as C++, and in the Python binding;
  * the console example's `m` key (every plane a half mirror or not)."""
import os
import shutil
import subprocess

import pytest

import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reflect_bound_never_culls_a_reachable_sphere(tmp_path):
    exe = str(tmp_path / "test_reflect_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_reflect_bound.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all reflect bound tests passed" in p.stdout, p.stdout[-4000:]


DECL_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    int (*set)(rtx_ctx*, unsigned, size_t, const float*);
    int (*get)(const rtx_ctx*, unsigned, float*);
    (void)sizeof(set = rtx_scene_set_reflectivity); /* the declarations' types, checked without linking the library */
    (void)sizeof(get = rtx_scene_get_reflectivity);
    printf("%d %d %d\n", (int)RTX_OPT_REFLECT_CHECK, (int)RTX_STAT_REFLECT_FRAMES, (int)RTX_STAT_REFLECT_LONGEST_LIST);
    return 0;
}
"""


@pytest.mark.parametrize("lang", ["c99", "c++"])
def test_reflect_declarations_compile_as_c99_and_cxx(tmp_path, lang):
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
    assert out == ["22", "120", "121"]
    assert (R.OPT_REFLECT_CHECK, R.STAT_REFLECT_FRAMES, R.STAT_REFLECT_LONGEST_LIST) == (22, 120, 121)
    for name in ("rtx_scene_set_reflectivity", "rtx_scene_get_reflectivity"):
        assert name in R.EXPORTED_SYMBOLS


def test_console_m_key_toggles_mirrors_on_a_pty():
    """examples/console_engine.cpp --keys-only: `m` (and `M`) decode to the mirror toggle; `k` stays "other"."""
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
        for raw, name in ((b"", "raw 1"), (b"m", "key mirrors"), (b"M", "key mirrors"), (b"k", "key other"), (b"h", "key shadows"), (b"x", "key quit")):
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
