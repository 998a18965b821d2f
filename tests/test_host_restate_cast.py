"""tests/restate_cast.py on the CPU, and the input conditions tests/test_gpu_cast.py relies on.
  * With every object casting, restate_cast.classify64_points returns restate_shadows.classify64_points' array exactly, and
    level_sets the same dicts.
  * A mask changes a decision in one direction only: a pair that is lit stays lit; a non-casting owner still shadows itself.
  * restate_shadows' three scenes at 320 x 180 with U = the even-numbered spheres, level 0, one and three lights: at least 1000
    (point, light) pairs are lit again per scene, and at most 0.1 % of the tested pairs are ambiguous.  Found here:
        mirror_floor_shadows   1854 of 33643 lit again; 3 lights: 4913;  ambiguous 4 of 33643 / 9 of 100929
        directed               2241 of 42167;           3 lights: 6729;  ambiguous 2 of 42167 / 2 of 126501
        wall                   2700 of 41079;           3 lights: 11773; ambiguous 10 of 41079 / 36 of 123237
    (a pair counts as lit again where float64 decides it under both masks).
  * The second oracle's scene (restate_cast.oracle_scene): by the CPU trace at least 80 % of scene A's visible pixels have the same
    distance and normal in scene B, A without U."""
import numpy as np
import pytest

import restate_cast as RC
import restate_shadows as RH


@pytest.mark.parametrize("name", RH.SCENES)
def test_all_ones_is_the_unmasked_decision(name):
    trace = RH.traced(name)[5]
    ones = np.ones(len(trace["sph"]) + len(trace["pl"]), dtype=np.uint8)
    for j in (0, 1):
        idx, P, N, owner = RH.level_points(trace, j)
        for l in RH.lights(name, 3):
            want = RH.classify64_points(P, N, owner, trace["sph"], trace["pl"], l.pos)
            got = RC.classify64_points(P, N, owner, trace["sph"], trace["pl"], l.pos, ones)
            assert got.dtype == want.dtype and np.array_equal(got, want)
    _, ls, full = RH.sets(name, 1, 1)
    for a, b in zip(full, RC.level_sets(trace, ls, 1, ones)):
        assert a["ambiguous"] == b["ambiguous"]
        for key in ("tested", "dset", "decided", "facing_dark"):
            assert np.array_equal(a[key], b[key]), key


def test_a_mask_only_lights_and_the_owner_still_shadows_itself():
    # one sphere over a floor, the light above: the floor below the sphere is dark, the sphere's underside is dark by itself
    sph = np.array([[0, 5, 20, 2, 255, 0, 0], [40, 5, 20, 2, 0, 255, 0]], dtype=np.float32)
    pl = np.array([[0, 0, 20, 0, 1, 0, 100, 100, 100, 200, 200], [0, 20, 20, 0, -1, 0, 100, 100, 100, 10, 10]], dtype=np.float32)
    light = (0.0, 50.0, 20.0)
    P = np.array([[0, 0, 20], [30, 0, 20], [0, 3, 20], [0, 7, 20]], dtype=np.float64)  # floor under the sphere, floor aside, underside, top
    N = np.array([[0, 1, 0], [0, 1, 0], [0, -1, 0], [0, 1, 0]], dtype=np.float64)
    owner = np.array([2, 2, 0, 0])
    k = lambda casts: RC.classify64_points(P, N, owner, sph, pl, light, np.array(casts, dtype=np.uint8)).tolist()
    assert k([1, 1, 1, 1]) == [1, 0, 1, 1]  # (the small plane above the scene shadows the floor under it and the sphere's top)
    assert k([1, 1, 1, 0]) == [1, 0, 1, 0]  # the plane above casts no shadow: the sphere's top is lit, the floor is dark by the sphere
    assert k([0, 1, 1, 0]) == [0, 0, 1, 0]  # nor does the sphere: the floor is lit; its underside still faces away from the light
    assert k([0, 0, 0, 0]) == [0, 0, 1, 0]
    assert k([0, 1, 1, 1]) == [1, 0, 1, 1]


@pytest.mark.parametrize("name", RH.SCENES)
def test_the_scenes_light_enough_pairs_again_and_few_are_ambiguous(name):
    for nl in (1, 3):
        tested, lit, amb, differ = RC.lit_again(name, nl, 0)
        trace, ls, casts, full, masked = RC.sets(name, nl, 0)
        print("%s, %d light(s): %d of %d tested pairs lit again on %d pixels, %d ambiguous" % (name, nl, lit, tested, int(differ.sum()), amb))
        assert int(casts.sum()) == len(casts) - (len(trace["sph"]) + 1) // 2
        assert lit >= 1000
        assert amb <= 0.001 * tested
        # one direction only: no decided pair goes dark under the mask
        both = full[0]["decided"] & masked[0]["decided"]
        assert not (masked[0]["dset"] & ~full[0]["dset"])[both].any()


def test_the_second_oracles_scenes_are_seen_alike_on_most_pixels():
    visible, alike = RC.seen_alike()
    print("%d visible pixels, %d seen alike without U" % (visible, alike))
    assert visible >= 0.5 * RC.ORACLE_W * RC.ORACLE_H and alike >= 0.8 * visible
