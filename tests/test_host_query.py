"""The ray-query ABI and the world grid behind it, without a GPU:
  * csrc/rtx_grid.hpp compiled as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_grid_bound.cpp): the
    planner's degenerate boxes, and over two million seeded rays no sphere the fp32 test reports hit is ever missing from the cells
    the walk visits before it stops;
  * the new declarations and constants in the header as plain C99 and as C++, and in the Python binding;
  * the console example's `p` key (rtx_pick on the centre cell)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_grid_bound_and_planner(tmp_path):
    exe = str(tmp_path / "test_grid_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall",
                           "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "test_grid_bound.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all grid bound tests passed" in p.stdout, p.stdout[-4000:]
    walked = int(p.stdout.split("walked")[1].split()[0])
    assert walked >= 2000000, p.stdout[-400:]


DECL_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rtx.h"
int main(void)
{
    int (*q)(rtx_ctx*, size_t, const rtx_ray*, rtx_ray_hit*, unsigned, void*);
    int (*h)(rtx_ctx*, size_t, const rtx_ray*, rtx_ray_hit*, unsigned);
    int (*p)(rtx_ctx*, const rtx_params*, size_t, size_t, rtx_ray_hit*);
    rtx_ray r;
    rtx_ray_hit a;
    (void)sizeof(q = rtx_query_rays); /* the declarations' types, checked without linking the library */
    (void)sizeof(h = rtx_query_rays_host);
    (void)sizeof(p = rtx_pick);
    r.o[2] = r.d[2] = r.tmax = 0.0f;
    r.skip = RTX_NO_OBJECT;
    a.t = r.tmax;
    a.index = RTX_SOME_OBJECT;
    printf("%d %d %d %d %d %d %d ", (int)sizeof(rtx_ray), (int)sizeof(rtx_ray_hit), (int)RTX_OPT_QUERY_CHECK, (int)RTX_STAT_QUERY_GRID_BUILDS,
           (int)RTX_STAT_QUERY_FALLBACK_RAYS, (int)RTX_STAT_QUERY_LARGE_SPHERES, (int)RTX_OPT_QUERY_LOAD);
    printf("%d %d %x %x %d %d %d %d\n", (int)RTX_QUERY_CLOSEST, (int)RTX_QUERY_ANY, r.skip, a.index, (int)RTX_STAT_QUERY_GRID_CELLS,
           (int)RTX_STAT_QUERY_GRID_PAIRS, (int)RTX_STAT_QUERY_BRUTE, (int)RTX_STAT_QUERY_GRID_GEOMETRY);
    return 0;
}
"""


@pytest.mark.parametrize("lang", ["c99", "c++"])
def test_query_declarations_compile_as_c99_and_cxx(tmp_path, lang):
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
    assert out == ["32", "8", "23", "122", "123", "124", "24", "0", "1", "ffffffff", "fffffffe", "125", "126", "127", "128"]
    assert (R.OPT_QUERY_CHECK, R.STAT_QUERY_GRID_BUILDS, R.STAT_QUERY_FALLBACK_RAYS, R.STAT_QUERY_LARGE_SPHERES) == (23, 122, 123, 124)
    assert (R.OPT_QUERY_LOAD, R.STAT_QUERY_GRID_CELLS, R.STAT_QUERY_GRID_PAIRS, R.STAT_QUERY_BRUTE, R.STAT_QUERY_GRID_GEOMETRY) == (24, 125, 126, 127, 128)
    assert (R.QUERY_CLOSEST, R.QUERY_ANY, R.NO_OBJECT, R.SOME_OBJECT) == (0, 1, 0xFFFFFFFF, 0xFFFFFFFE)
    assert R.RAY_DTYPE.itemsize == 32 and R.RAY_HIT_DTYPE.itemsize == 8
    assert [R.RAY_DTYPE.fields[k][1] for k in ("o", "tmax", "d", "skip")] == [0, 12, 16, 28]
    assert [R.RAY_HIT_DTYPE.fields[k][1] for k in ("t", "index")] == [0, 4]
    for name in ("rtx_query_rays", "rtx_query_rays_host", "rtx_pick"):
        assert name in R.EXPORTED_SYMBOLS


def test_make_rays_layout():
    R = U.pkg()
    rays = R.make_rays([(1, 2, 3), (4, 5, 6)], [(0, 0, 1), (0, 1, 0)], tmax=[7.0, np.inf], skip=5)
    raw = rays.view(np.uint8).reshape(2, 32)
    assert np.array_equal(raw[0, :16].view(np.float32), np.array([1, 2, 3, 7], np.float32))
    assert np.array_equal(raw[1, 16:28].view(np.float32), np.array([0, 1, 0], np.float32))
    assert raw[1, 28:32].view(np.uint32)[0] == 5 and np.isinf(rays["tmax"][1])
    assert R.make_rays(np.zeros((3, 3)), np.ones((3, 3)))["skip"].tolist() == [R.NO_OBJECT] * 3


def test_console_p_key_picks_on_a_pty():
    """examples/console_engine.cpp --keys-only: `p` (and `P`) decode to the pick key; `k` stays "other", `m` the mirror toggle."""
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
        for raw, name in ((b"", "raw 1"), (b"p", "key pick"), (b"P", "key pick"), (b"k", "key other"), (b"m", "key mirrors"), (b"x", "key quit")):
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
