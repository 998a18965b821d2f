"""The light / shadow ABI and the occluder bound of the shadow pass, without a GPU:
  * csrc/rtx_shadow.hpp compiled as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_shadow_bound.cpp):
    millions of seeded random cases, no true occluder ever culled;
  * struct rtx_light's layout (44 bytes, field offsets) in the header as plain C99 and in the Python binding;
  * the console example's `h` key (shadows on / off)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shadow_bound_never_culls_an_occluder(tmp_path):
    exe = str(tmp_path / "test_shadow_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_shadow_bound.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all shadow bound tests passed" in p.stdout, p.stdout[-4000:]


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    rtx_light l;
    int (*set)(rtx_ctx*, const rtx_light*);
    int (*get)(const rtx_ctx*, rtx_light*);
    (void)sizeof(set = rtx_scene_set_light); /* the declarations' types, checked without linking the library */
    (void)sizeof(get = rtx_scene_get_light);
    (void)l;
    printf("%u %u %u %u %u %u %d %d %d %d\n", (unsigned)sizeof(rtx_light), (unsigned)offsetof(rtx_light, pos), (unsigned)offsetof(rtx_light, diffuse_rgb),
           (unsigned)offsetof(rtx_light, diffuse_power), (unsigned)offsetof(rtx_light, specular_rgb), (unsigned)offsetof(rtx_light, specular_power),
           (int)RTX_OPT_SHADOWS, (int)RTX_OPT_SHADOW_CHECK, (int)RTX_STAT_SHADOW_FRAMES, (int)RTX_STAT_SHADOW_LONGEST_LIST);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_light_layout_in_c99_and_in_the_binding(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).split()
    R = U.pkg()
    assert out == ["44", "0", "12", "24", "28", "40", str(R.OPT_SHADOWS), str(R.OPT_SHADOW_CHECK), str(R.STAT_SHADOW_FRAMES),
                   str(R.STAT_SHADOW_LONGEST_LIST)]
    assert C.sizeof(R.Light) == 44
    assert [getattr(R.Light, f).offset for f in ("pos", "diffuse_rgb", "diffuse_power", "specular_rgb", "specular_power")] == [0, 12, 24, 28, 40]
    assert (R.OPT_SHADOWS, R.OPT_SHADOW_CHECK) == (20, 21)
    for name in ("rtx_scene_set_light", "rtx_scene_get_light"):
        assert name in R.EXPORTED_SYMBOLS
    l = R.make_light()
    assert list(l.pos) == [1.0, 50.0, 0.0] and list(l.diffuse_rgb) == [1.0, 1.0, 1.0] and l.diffuse_power == 2000.0
    assert list(l.specular_rgb) == [1.0, 1.0, 1.0] and l.specular_power == 3000.0


def test_console_h_key_toggles_shadows_on_a_pty():
    """examples/console_engine.cpp --keys-only: `h` (and `H`) decode to the shadow toggle; no key the reference uses changes."""
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
        for raw, name in ((b"", "raw 1"), (b"h", "key shadows"), (b"H", "key shadows"), (b"w", "key w"), (b"x", "key quit")):
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
