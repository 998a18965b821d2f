"""tests/restate_shadows.py on the CPU: no GPU, no torch.
  1. shade_chain_dark with only level 0 dark is restate.shade_chain bit for bit; a dark set at a deeper level changes the colour
     of the pixels that have that level, and of no other.
  2. classify64_points with the trace's owner agrees with tests/test_gpu_lights.py::classify64 on level 0 wherever both decide.
  3. The inputs of tests/test_gpu_reflect_shadows.py, judged on the restatement alone so that the GPU tests cannot hide a failure
     behind them, per scene x (lights, depth): few ambiguous points, level-1 points in shadow, level-1 points in shadow from a
     light they face (occlusion, not self-shadow), and per-level sets that show in the colour's bits."""
import numpy as np
import pytest

import restate as RS
import restate_shadows as RH

f32 = np.float32


def _differs(a, b):
    return np.logical_or.reduce([a[q].view(np.uint32) != b[q].view(np.uint32) for q in range(3)])


# ---------------------------------------------------------------- 1. the colour

@pytest.mark.parametrize("name", ["mirror_floor_shadows", "wall"])
def test_level_0_dark_only_is_shade_chain(name):
    trace = RH.traced(name)[5]
    lights = RH.lights(name, 3)
    for S in (0, 1, 5, 7):
        want = RS.shade_chain(trace, lights, dark0=S)
        got = RH.shade_chain_dark(trace, lights, [S, 0, 0, 0, 0])
        arr = RH.shade_chain_dark(trace, lights, [np.full(trace["n"], S), np.zeros(trace["n"], dtype=np.int64), 0, 0, 0])
        for depth in (1, 2, 3, 4):
            for q in range(3):
                assert np.array_equal(got[depth][q].view(np.uint32), want[depth][q].view(np.uint32)), (S, depth, q)
                assert np.array_equal(arr[depth][q].view(np.uint32), want[depth][q].view(np.uint32)), (S, depth, q)


def test_a_deep_dark_set_changes_the_pixels_of_that_level_only():
    trace = RH.traced("mirror_floor_shadows")[5]
    lights = RH.lights("mirror_floor_shadows", 2)
    lit = RH.shade_chain_dark(trace, lights, [0, 0, 0, 0, 0])
    for j in (1, 2, 3):
        d = [0, 0, 0, 0, 0]
        d[j] = 3
        c = RH.shade_chain_dark(trace, lights, d)
        hit_j = np.zeros(trace["n"], dtype=bool)
        lev = trace["levels"][j]
        hit_j[lev["idx"]] = lev["gid"] >= 0
        for depth in (1, 2, 3, 4):
            ch = _differs(c[depth], lit[depth])
            assert not (ch & ~hit_j).any(), (j, depth)
            if depth >= j:
                assert ch.sum() >= 0.5 * (hit_j & trace["vis"]).sum(), (j, depth, int(ch.sum()), int(hit_j.sum()))
            else:
                assert not ch.any(), (j, depth)
    # a per-pixel array selects per pixel: even pixels dark at level 1, odd pixels lit
    sel = np.where(np.arange(trace["n"]) % 2 == 0, 3, 0)
    mixed = RH.shade_chain_dark(trace, lights, [0, sel, 0, 0, 0])[2]
    dark1 = RH.shade_chain_dark(trace, lights, [0, 3, 0, 0, 0])[2]
    for q in range(3):
        assert np.array_equal(mixed[q][::2].view(np.uint32), dark1[q][::2].view(np.uint32))
        assert np.array_equal(mixed[q][1::2].view(np.uint32), lit[2][q][1::2].view(np.uint32))


# ---------------------------------------------------------------- 2. float64 at given points

@pytest.mark.parametrize("name", ["mirror_floor_shadows", "directed"])
def test_classify64_points_agrees_with_classify64_on_level_0(name):
    import test_gpu_lights as TL
    p, sph, pl, ks, pix, trace = RH.traced(name)
    lights = RH.lights(name, 3)
    vals = RS.values8(trace, RS.shade_chain(trace, lights)[1])
    idx, P, N, owner = RH.level_points(trace, 0)
    assert len(idx) > 0.15 * trace["n"]
    for l in lights:
        old = TL.classify64(p, trace["sph"], trace["pl"], vals, l.pos, pix)
        new = RH.classify64_points(P, N, owner, trace["sph"], trace["pl"], l.pos)
        assert (old[idx] != -2).all() and (np.delete(old, idx) == -2).all(), "the two judge other pixels"
        both = (old[idx] >= 0) & (new >= 0)
        print(name, "level 0: both decide %d of %d points, shadowed %d" % (int(both.sum()), len(idx), int((new[both] == 1).sum())))
        assert both.sum() >= 0.99 * len(idx)
        assert np.array_equal(old[idx][both], new[both]), "%d points decided differently" % int((old[idx][both] != new[both]).sum())
        assert (new[both] == 1).sum() >= 0.01 * len(idx) and (new[both] == 0).sum() >= 0.01 * len(idx)


# ---------------------------------------------------------------- 3. the inputs of the GPU test

@pytest.mark.parametrize("nl,depth", RH.CASES)
@pytest.mark.parametrize("name", RH.SCENES)
def test_reflect_shadow_inputs(name, nl, depth):
    """Measured (320 x 180, every pixel; level-1 points = pixels whose level 1 hit an object):
      scene                 lights depth  ambiguous  level-1 points  dark at level 1  ... for a light they face  sets show
      mirror_floor_shadows    1      4        6          5932            4660               834               2802
      mirror_floor_shadows    2      2        7          5932            4978              1194               3427
      mirror_floor_shadows    3      1        9          5932            5272              1423               2897
      directed                1      4        4          5764            4210               761               2402
      directed                2      2        4          5764            4331               860               2800
      directed                3      1        2          5764            4452               959               2047
      wall                    1      4       10          2425             397               396                393
      wall                    2      2       24          2425             665               664                661
      wall                    3      1       36          2425             992               991                987
    Floors: ambiguous (pixel, light, level) triples at most 0.001 x lights x levels x pixels; at least 1 % of the level-1 points
    dark for some light at level 1; on at least one scene at least 1 % of them dark for a light they face; on at least 1 % of the
    level-1 pixels the decided per-level sets give a colour whose bits differ from the level-0-only colour."""
    trace, lights, lev = RH.sets(name, nl, depth)
    n = trace["n"]
    amb = sum(l["ambiguous"] for l in lev)
    l1 = lev[1]["tested"]
    dark1 = l1 & lev[1]["decided"] & (lev[1]["dset"] != 0)
    facing1 = l1 & lev[1]["decided"] & lev[1]["facing_dark"]
    decided = np.logical_and.reduce([l["decided"] for l in lev])
    full = RH.shade_chain_dark(trace, lights, [l["dset"] for l in lev] + [0] * (4 - depth))[depth]
    only0 = RH.shade_chain_dark(trace, lights, [lev[0]["dset"], 0, 0, 0, 0])[depth]
    shows = _differs(full, only0) & decided & l1 & trace["vis"]
    print("%s, %d lights, depth %d: ambiguous %d, level-1 points %d, dark at level 1 %d, for a light they face %d, sets show on %d" % (
        name, nl, depth, amb, int(l1.sum()), int(dark1.sum()), int(facing1.sum()), int(shows.sum())))
    assert amb <= 0.001 * nl * (depth + 1) * n
    assert l1.sum() >= 1000
    assert dark1.sum() >= 0.01 * l1.sum()
    assert shows.sum() >= 0.01 * l1.sum()


def test_some_scene_has_level_1_points_occluded_from_a_light_they_face():
    best = {}
    for name in RH.SCENES:
        trace, lights, lev = RH.sets(name, 1, 4)
        l1 = lev[1]["tested"]
        best[name] = (int((l1 & lev[1]["decided"] & lev[1]["facing_dark"]).sum()), int(l1.sum()))
    print("level-1 points dark for a light they face, of the level-1 points:", best)
    assert any(f >= 0.01 * t for f, t in best.values())
    assert best["wall"][0] >= 0.01 * best["wall"][1], "the wall's level-1 points do not lie in the spheres' shadows"


def test_the_cases_stay_within_64_combinations():
    for nl, depth in RH.CASES:
        assert len(RH.combinations(nl, depth)) == (1 << nl) ** (depth + 1) <= 64
