"""The inputs of the RTX_OPT_REFLECT_GRID tests, judged on the CPU with tests/restate.py::trace_chain alone, so that the comparisons of
tests/test_gpu_reflect_grid.py cannot be empty: every scene has mirror rays at three levels that hit spheres, scene b's rays leave and
hit the large-list sphere and meet the coincident twins, and scene c's floor starts rays on both sides of the grid's `reach`.

The floors asserted are far below what was measured when the scenes were chosen (without the twins, at 37 x 21 / 64 x 48: rays per
level 1 .. 4 of a 214 18 2 1 / 817 62 7 1, of b 96 27 9 5 / 183 56 26 13, of c 381 135 68 26 / 1405 298 133 62; level-1 hits on spheres
of a 24 / 106, of b 55 / 99).  Also here: the host-only planner test (tests/host/test_plan_reflect_grid.cpp under ASan + UBSan)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import reflect_grid_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", G.NAMES)
def test_every_scene_has_mirror_rays_at_three_levels(name, size):
    f = G.facts(name, *size)
    print(name, size, "rays per level", f["rays"], "level-1 hits on spheres", f["sphere_hits1"], "inside / beyond / unsure per level",
          f["inside"], f["beyond"], f["unsure"])
    assert f["rays"][0] >= 30
    assert f["sphere_hits1"] >= 20
    assert f["rays"][1] >= 5
    assert f["rays"][2] >= 1
    if name in ("a", "b"):  # origins on spheres lie inside the spheres' box: every ray can be walked
        assert sum(f["beyond"]) == 0 and sum(f["unsure"]) == 0


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: "%dx%d" % s)
def test_scene_b_meets_the_large_sphere_and_the_twins(size):
    f = G.facts("b", *size)
    win, left = f["winners1"], f["left1"]
    n_leave, n_won = int((left == G.LARGE).sum()), int((win == G.LARGE).sum())
    earlier = int(np.isin(win, list(G.TWINS.values())).sum())
    later = int(np.isin(win, list(G.TWINS.keys())).sum())
    print(size, "leave the large sphere", n_leave, "won by it", n_won, "earlier twin wins", earlier, "later twin wins", later)
    assert n_leave >= 1
    assert n_won >= 1
    assert earlier >= 5
    assert later == 0
    # the twins are coincident: same centre and radius, another colour
    sph = f["sph"]
    for late, early in G.TWINS.items():
        assert np.array_equal(sph[late, :4], sph[early, :4]) and not np.array_equal(sph[late, 4:], sph[early, 4:])
    assert len(sph) >= 256  # the direction-sorted store is engaged


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: "%dx%d" % s)
def test_scene_c_starts_rays_on_both_sides_of_reach(size):
    f = G.facts("c", *size)
    print(size, "level-1 origins within reach", f["inside"][0], "beyond", f["beyond"][0], "on the boundary", f["unsure"][0])
    assert f["inside"][0] >= 100
    assert f["beyond"][0] >= 100
    assert f["inside"][0] + f["beyond"][0] + f["unsure"][0] == f["rays"][0]
    assert max(f["ks"]) == f["ns"] and len(f["pl"]) == 1  # the floor is the last object


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_plan_reflect_grid")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_plan_reflect_grid.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all reflect-grid planning tests passed" in p.stdout, p.stdout[-4000:]
