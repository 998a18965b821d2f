"""The input conditions of tests/test_gpu_spot.py, judged on the restatement alone (tests/restate_spot.py; CPU, no GPU): the scene
is restate.chain_scene("mirror_floor_shadows") under restate.shadow_lights(name, 3), each light a cone aimed from the light at one
point (restate_spot.CONES: (0, 2, 32) 14 / 8 degrees, (-6, 0, 28) 20 / 12, (8, 0, 34) 16 / 15).
  (a) for every level 0 .. 2 and every light the hit pixels fall into the three classes w = 0, 0 < w < 1 and w = 1.  Each count was
      measured once and stands in CLASSES below; half of it is the floor asserted.  The smallest class has 196 pixels (level 2,
      light 2, the band);
  (b) with no cone the restatement is restate._shade_lights bit for bit, and a set of point lights is the same as no cones;
  (c) every wrong= variant of the restatement (a bug a kernel could have) changes at least 100 visible pixels of the depth-3 frame;
  (d) the out-of-cone lights added to the dark sets change no float: a dark light and a weight of 0 give the same colour.
The bounds are conditions on the inputs, not tolerances: the GPU tests compare bit for bit."""
import numpy as np
import pytest

import restate as RS
import restate_finish as RF
import restate_spot as SP

f32 = np.float32

# hit pixels per class, {level: per light (w = 0, 0 < w < 1, w = 1)}
CLASSES = {0: [(25571, 5935, 2220), (16785, 12443, 4498), (29749, 477, 3500)],
           1: [(1022, 3025, 1885), (317, 2940, 2675), (3154, 253, 2525)],
           2: [(487, 1120, 1083), (229, 983, 1478), (1276, 196, 1218)]}


def _scene():
    trace = SP.scene()[5]
    lights = RS.shadow_lights(SP.SCENE, 3)
    return trace, lights, SP.scene_cones(lights)


def _differs(a, b):
    return np.logical_or.reduce([a[q].view(np.uint32) != b[q].view(np.uint32) for q in range(3)])


def test_the_cones_are_the_issues():
    trace, lights, spots = _scene()
    assert [tuple(l.pos) for l in lights] == [(0.0, 40.0, 50.0), (-30.0, 30.0, 25.0), (30.0, 30.0, 25.0)]
    assert [s[0] for s in spots] == [(0.0, -38.0, -18.0), (24.0, -30.0, 3.0), (-22.0, -30.0, 9.0)]
    for s, (_, outer, inner) in zip(spots, SP.CONES):
        assert s[1] == f32(np.cos(np.radians(outer))) and s[2] == f32(np.cos(np.radians(inner))) and f32(s[2]) - f32(s[1]) >= f32(2.0 ** -10)
        st = SP.stored(s)
        assert abs(float(st[0]) ** 2 + float(st[1]) ** 2 + float(st[2]) ** 2 - 1.0) < 1e-6 and st[5] == f32(1.0) / (f32(s[2]) - f32(s[1]))


@pytest.mark.parametrize("j", [0, 1, 2])
def test_every_class_is_in_the_picture_at_every_level(j):
    trace, lights, spots = _scene()
    got = SP.classes(trace, lights, spots, j)
    print(j, got)
    hit = int((trace["levels"][j]["gid"] >= 0).sum())
    for i, (g, want) in enumerate(zip(got, CLASSES[j])):
        assert sum(g) == hit
        assert all(a >= b // 2 for a, b in zip(g, want)), (j, i, g, want)
    assert min(min(c) for c in CLASSES[j]) // 2 >= 98


def test_no_cone_is_the_rule_of_the_light_set_bit_for_bit():
    trace, lights, spots = _scene()
    points = [((0.0, 0.0, 0.0), 0.3, 0.9)] * 3  # (point lights: the cosines are ignored)
    for j in range(3):
        lev = trace["levels"][j]
        hit = lev["gid"] >= 0
        with np.errstate(all="ignore"):
            want = RS._shade_lights(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights)
            fin = RF.finish_arrays(None, lev["gid"])
            for sp in (None, [None] * 3, points):
                got = SP.shade_lights_spot(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights, sp, fin)
                for q in range(3):
                    assert np.array_equal(got[q][hit].view(np.uint32), want[q][hit].view(np.uint32)), (j, q)
    a, b = SP.shade_chain_spot(trace, lights, None), RS.shade_chain(trace, lights)
    for depth in (1, 3):
        for q in range(3):
            assert RS.same_floats(a[depth][q], b[depth][q])[trace["hit"]].all()
    # and the cones are in the picture: they change most visible pixels of the depth-3 frame
    c = SP.shade_chain_spot(trace, lights, spots, depths=[3])[3]
    assert int((_differs(c, b[3]) & trace["vis"]).sum()) >= 10000


@pytest.mark.parametrize("wrong", SP.WRONG)
def test_every_wrong_variant_would_be_seen(wrong):
    trace, lights, spots = _scene()
    right = SP.shade_chain_spot(trace, lights, spots, depths=[3])[3]
    bad = SP.shade_chain_spot(trace, lights, spots, wrong=wrong, depths=[3])[3]
    n = int((_differs(right, bad) & trace["vis"]).sum())
    print(wrong, n)
    assert n >= 100, (wrong, n)


def test_out_of_cone_lights_in_the_dark_sets_change_no_float():
    trace, lights, spots = _scene()
    plain = SP.scene()[6]
    import restate_glass as RG
    for tr, depth in ((plain, 0), (trace, 3)):
        d_spot = SP.dark_sets_spot(tr, lights, spots, True)
        d_seg = RG.dark_sets(tr, lights, True)
        assert any(int((a != b).sum()) >= 1000 for a, b in zip(d_spot, d_seg))  # (the sets do differ)
        if depth == 0:
            a = SP.shade_plain_spot(tr, lights, spots, None, d_spot[0])
            b = SP.shade_plain_spot(tr, lights, spots, None, d_seg[0])
        else:
            a = SP.shade_chain_spot(tr, lights, spots, None, d_spot[0], d_spot[1:], depths=[depth])[depth]
            b = SP.shade_chain_spot(tr, lights, spots, None, d_seg[0], d_seg[1:], depths=[depth])[depth]
        for q in range(3):
            assert RS.same_floats(a[q], b[q])[tr["vis"]].all()
