"""The inputs of tests/test_gpu_pattern.py, judged on the CPU with tests/restate_pattern.py alone, so that its comparisons cannot be
empty: in scene A both colours of every patterned object are seen directly and in mirrors of two levels, in the sorted-store scene
every visible patterned sphere shows both, and `patterned` changes od where the rule says and nowhere else.

Measured when the scenes were chosen (320 x 180): the smaller parity's share of an object's pixels is at least 0.44 at level 0, 0.42
at level 1 (object 1) and 0.45 at level 2; the thinnest case is object 3 at level 2 with 136 pixels, 61 of them of its rarer parity;
78 patterned spheres of the sorted-store scene are visible."""
import numpy as np
import pytest

import restate as RS
import restate_pattern as RP

f32 = np.float32


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("obj", RP.SCENE_A_OBJECTS)
def test_scene_a_shows_both_parities_at_three_levels(obj, level):
    trace = RP.scene_a()[5]
    even, odd = RP.parity_counts(trace, RP.SCENE_A_TABLE, RP.SCENE_A_SLOTS, obj, level)
    print("object %d level %d: %d even, %d odd, smaller share %.3f" % (obj, level, even, odd, min(even, odd) / max(even + odd, 1)))
    assert min(even, odd) >= 50
    assert min(even, odd) >= 0.25 * (even + odd)


def test_patterned_changes_od_by_the_rule_and_nothing_else():
    p, sph, pl, ks, pix, trace, pat = RP.scene_a()
    slots = RP.slot_array(RP.SCENE_A_SLOTS, len(sph) + len(pl))
    for key in ("t", "gid", "sv", "normal", "hit", "vis", "rays"):
        assert pat[key] is trace[key]
    changed_somewhere = 0
    for a, b in zip(trace["levels"], pat["levels"]):
        for key in a:
            if key != "od":
                assert b[key] is a[key], key
        slot, is_odd = RP.level_parity(a, RP.SCENE_A_TABLE, slots)
        differs = np.logical_or.reduce([a["od"][q].view(np.uint32) != b["od"][q].view(np.uint32) for q in range(3)])
        assert not (differs & ~((slot > 0) & is_odd)).any()
        for s, t in enumerate(RP.SCENE_A_TABLE, start=1):
            m = (slot == s) & is_odd
            for q in range(3):
                assert (b["od"][q][m] == f32(t.rgb[q]) / f32(255.0)).all()
        changed_somewhere += int(differs.sum())
    assert changed_somewhere > 10000
    # the input is left as it was, and shading the copy gives another picture
    lights = [RS.reference_light()]
    c0, c1 = RS.shade_chain(trace, lights)[2], RS.shade_chain(pat, lights)[2]
    # (the floor has k = 1: its own colour carries no weight, so the picture changes on the spheres and in what mirrors show of them)
    assert (np.logical_or.reduce([c0[q] != c1[q] for q in range(3)]) & trace["vis"]).sum() > 1000


def test_the_rules_exact_cases():
    one = lambda x, y, z: tuple(np.array([v], dtype=np.float32) for v in (x, y, z))
    unit = RP.Pattern((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert RP.odd(one(-0.5, 0.5, 0.5), unit)[0]            # floorf(-0.5f) = -1
    assert not RP.odd(one(-0.5, -0.5, 0.5), unit)[0]
    floor = RP.Pattern((0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (0.0, 0.0, 0.0))
    assert not RP.odd(one(0.5, -7.3, 0.5), floor)[0]       # freq 0, negative P: floorf(-0) = 0
    assert RP.odd(one(1.5, -7.3, 0.5), floor)[0]
    assert not RP.odd(one(16777216.0, 0.5, 0.5), unit)[0]  # |f| = 2^24: even
    assert not RP.odd(one(-16777216.0, 0.5, 0.5), unit)[0]
    assert RP.odd(one(np.nan, 0.5, 0.5), unit)[0]          # a NaN is odd


def test_sorted_store_scene_shows_both_parities_on_every_visible_patterned_sphere():
    p, sph, pl, slots, trace, pat = RP.sorted_scene()
    assert len(sph) >= 256  # the direction-sorted store is engaged
    lev = trace["levels"][0]
    _, is_odd = RP.level_parity(lev, RP.SCENE_A_TABLE, slots)
    seen = trace["vis"] & (lev["t"] <= f32(p.cam_far))
    visible = [i for i in range(0, len(sph), 3) if (seen & (lev["gid"] == i)).any()]
    both = [i for i in visible if (seen & (lev["gid"] == i) & is_odd).any() and (seen & (lev["gid"] == i) & ~is_odd).any()]
    print("%d patterned spheres visible, %d show both parities" % (len(visible), len(both)))
    assert len(visible) == 78
    assert both == visible
