"""The input conditions of tests/test_gpu_finish.py, judged on the restatement alone (tests/restate_finish.py; CPU, no GPU): scene F
is restate.chain_scene("mirror_floor") with restate_finish.F_FINISHES, under the light sets `1custom` and `8`.
  (a) with the default finish the restated rule is restate._shade_lights bit for bit on every hit pixel of levels 0 .. 2;
  (b) every finished object shows at each of levels 0, 1 and 2: at least 100 pixels whose level hit it, whose colour there differs
      from the default finish's and has a component below the 255 clamp;
  (c) every wrong= variant of the restatement (a bug a kernel could have) differs from the rule in some colour bit on at least 100
      hit pixels at level 0 and on at least 10 at level 2.
And those of tests/test_gpu_finish_edges.py, where the question is which object's finish a level reads: scene C and scene D of
tests/restate_glass.py with restate_finish.C_FINISHES and d_finishes() under restate_glass.lights_a(1) and lights_a(3) (what
test_gpu_glass._lights(1) and (3) give), scene E under `1custom` and `8`.  Each count was measured once and stands in a table
below (SHOWS_C, SHOWS_D, CHANGED, ENDS_E, M8_E); half of it is the floor asserted.
  (d) scene C: per finished object the pixels at which it shows (as in (b)) at levels 0, 1, 2 -- the floor 101, 172, 101 (97 under
      three lights), the sheet 696, 30, 0; both planes show at levels 0 and 1, and at every level at least three objects do;
  (e) scene D: 9 finished spheres show at level 0 and 14 at level 1 (at least 8 asked), on 407 .. 417, 248 .. 250 and 65 pixels of
      levels 0, 1 and 2;
  (f) each of restate_finish.WRONG_LOOKUP and of WRONG changes visible pixels of the depth-3 frame of the scene it is aimed at,
      shadowed as the GPU test renders it: plane0 726 of scene C's 878; level0 540 (C) and 445 of scene D's 720; unsorted 583 (D);
      m_cap7 404 .. 1368 of scene E's frames; the six rule variants 20 .. 484 (C).  Floors: half, never below 5;
  (g) scene E: each end (0 and 16) of each weight shows at level 0 on at least 861 pixels of its object (at least 20 asked), m = 8
      differs from m = 7 on 404 (`1custom`) and 754 (`8`) pixels of its sphere; 16 od < 1 for every object;
  (h) every m in 0 .. 8 occurs across C, D and E; creation_orders interleaves and keeps each kind in its own order.
The bounds are conditions on the inputs, not tolerances: the GPU tests compare bit for bit."""
import numpy as np
import pytest

import restate as RS
import restate_finish as RF
import restate_glass as RG
import restate_pattern as RP

f32 = np.float32
SETS = ["1custom", "8"]


def _lights(which):
    return RS.chain_lights("mirror_floor", which)


def _level_colours(trace, lights, finishes, j, wrong=None):
    """The colour of level j's hit under `finishes`, for the pixels level j exists for: [r, g, b] over lev["idx"]."""
    lev = trace["levels"][j]
    with np.errstate(all="ignore"):
        return RF.shade_lights_finish(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights, RF.finish_arrays(finishes, lev["gid"]), 0, wrong)


def _differs(a, b):
    return np.logical_or.reduce([a[q].view(np.uint32) != b[q].view(np.uint32) for q in range(3)])


@pytest.mark.parametrize("which", SETS)
def test_default_finish_is_the_rule_without_finishes(which):
    trace = RF.scene_f()[5]
    lights = _lights(which)
    for j in range(3):
        lev = trace["levels"][j]
        hit = lev["gid"] >= 0
        assert hit.sum() >= 1000
        with np.errstate(all="ignore"):
            want = RS._shade_lights(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights)
        got = _level_colours(trace, lights, None, j)
        explicit = _level_colours(trace, lights, {i: RF.DEFAULT for i in range(5)}, j)
        for q in range(3):
            assert np.array_equal(got[q][hit].view(np.uint32), want[q][hit].view(np.uint32)), (which, j, q)
            assert np.array_equal(explicit[q][hit].view(np.uint32), want[q][hit].view(np.uint32)), (which, j, q)
    # and the folds: shade_chain_finish without finishes is restate.shade_chain
    a, b = RF.shade_chain_finish(trace, lights, None), RS.shade_chain(trace, lights)
    for depth in (1, 4):
        for q in range(3):
            assert RS.same_floats(a[depth][q], b[depth][q])[trace["hit"]].all()


@pytest.mark.parametrize("which", SETS)
def test_every_finished_object_shows_at_levels_0_to_2(which):
    trace = RF.scene_f()[5]
    lights = _lights(which)
    counts = {}
    for j in range(3):
        lev = trace["levels"][j]
        plain = _level_colours(trace, lights, None, j)
        fin = _level_colours(trace, lights, RF.F_FINISHES, j)
        below = np.logical_or.reduce([fin[q] < f32(255.0) for q in range(3)])
        seen = _differs(plain, fin) & below
        for obj in RF.F_FINISHES:
            counts[(obj, j)] = int((seen & (lev["gid"] == obj)).sum())
        assert not (seen & (lev["gid"] == 2)).any()  # (sphere 2 keeps the default finish)
    print(which, counts)
    assert min(counts.values()) >= 100, counts


@pytest.mark.parametrize("wrong", RF.WRONG)
@pytest.mark.parametrize("which", SETS)
def test_every_wrong_variant_would_be_seen(which, wrong):
    trace = RF.scene_f()[5]
    lights = _lights(which)
    n = {}
    for j, least in ((0, 100), (2, 10)):
        hit = trace["levels"][j]["gid"] >= 0
        n[j] = int((_differs(_level_colours(trace, lights, RF.F_FINISHES, j), _level_colours(trace, lights, RF.F_FINISHES, j, wrong)) & hit).sum())
        assert n[j] >= least, (which, wrong, n)
    print(which, wrong, n)


# ---------------------------------------------------------------- the inputs of tests/test_gpu_finish_edges.py

FLOOR_TABLE = RP.SCENE_A_TABLE[:1]  # (test_gpu_glass.FLOOR_TABLE: scene C's floor is patterned as scene A's)
_edge = {}


def edge_scene(name):
    """(trace as the GPU tests render it, finishes, {config: (lights, shadows at every level)}) of scene C or D."""
    if name not in _edge:
        if name == "c":
            trace = RP.patterned(RG.scene_c()[6], FLOOR_TABLE, {RG.C_FLOOR: 1})
            _edge[name] = (trace, RF.C_FINISHES, {"1 light, shadows": (RG.lights_a(1), True), "3 lights, shadows": (RG.lights_a(3), True)})
        else:
            _edge[name] = (RG.scene_d()[6], RF.d_finishes(), {"3 lights": (RG.lights_a(3), False), "1 light, shadows": (RG.lights_a(1), True)})
    return _edge[name]


def shows(trace, lights, finishes, j):
    """{finished object: pixels whose level j hit it, whose colour there differs in some bit from the default finish's and has a
    component below the 255 clamp}."""
    lev = trace["levels"][j]
    plain = _level_colours(trace, lights, None, j)
    fin = _level_colours(trace, lights, finishes, j)
    seen = _differs(plain, fin) & np.logical_or.reduce([fin[q] < f32(255.0) for q in range(3)])
    return {obj: int((seen & (lev["gid"] == obj)).sum()) for obj in finishes}


def frame(trace, lights, finishes, depth, shadows, wrong=None):
    """The colour floats of the depth-`depth` frame (0: no mirrors, level 0 alone), under shadows at every level or none."""
    dark = RG.dark_sets(trace, lights, True) if shadows else None
    if depth == 0:
        return RF.shade_plain_finish(trace, lights, finishes, dark[0] if shadows else 0, wrong)
    if shadows:
        return RF.shade_chain_finish(trace, lights, finishes, dark0=dark[0], deep_dark=dark[1:], wrong=wrong)[depth]
    return RF.shade_chain_finish(trace, lights, finishes, wrong=wrong)[depth]


def changed(trace, lights, finishes, depth, shadows, wrong):
    """Visible pixels of the frame on which `wrong` changes some colour bit."""
    a, b = frame(trace, lights, finishes, depth, shadows), frame(trace, lights, finishes, depth, shadows, wrong)
    return int((_differs(a, b) & trace["vis"]).sum())


def e_frames():
    """{name: (trace, lights, depth)}: the frames tests/test_gpu_finish_edges.py renders of scene E, and the depth-3 frame."""
    e = RF.scene_e()
    out = {}
    for which in SETS:
        for name, trace, depth in (("no mirrors", e[6], 0), ("depth 2", e[5], 2), ("depth 3", e[5], 3)):
            out["%s, %s" % (which, name)] = (trace, _lights(which), depth)
    return out


# What the inputs give (pixels; the frames are 41 x 23 for scenes C and D, 320 x 180 for scene E).  Every assertion below is half
# of its entry, the variants never below 5.
#   scene C, per light set: {finished object: pixels at which it shows at levels 0, 1, 2}
SHOWS_C = {"1 light, shadows": {0: (47, 51, 6), 1: (9, 37, 13), 2: (0, 33, 13), 3: (0, 0, 4), 4: (24, 162, 56), 5: (18, 12, 2), 7: (0, 70, 0),
                                RG.C_FLOOR: (101, 172, 101), RG.C_SHEET: (696, 30, 0)},
           "3 lights, shadows": {0: (47, 51, 6), 1: (9, 37, 13), 2: (0, 33, 13), 3: (0, 0, 4), 4: (24, 162, 56), 5: (18, 12, 2), 7: (0, 70, 0),
                                 RG.C_FLOOR: (101, 172, 97), RG.C_SHEET: (696, 30, 0)}}
#   scene D, per light set: (finished spheres that show at level 0, at level 1; pixels at which one shows at levels 0, 1, 2)
SHOWS_D = {"3 lights": (9, 14, 407, 248, 65), "1 light, shadows": (9, 14, 417, 250, 65)}
#   (variant, scene) -> {frame: visible pixels of the depth-3 frame that change (scene E: of each frame rendered)}
AIMS = [("plane0", "c"), ("level0", "c"), ("level0", "d"), ("unsorted", "d"), ("m_cap7", "e")] + [(w, "c") for w in RF.WRONG]
CHANGED = {("plane0", "c"): {"1 light, shadows": 726, "3 lights, shadows": 726},  # (of 878 visible pixels)
           ("level0", "c"): {"1 light, shadows": 540, "3 lights, shadows": 540},
           ("level0", "d"): {"3 lights": 445, "1 light, shadows": 445},  # (of 720)
           ("unsorted", "d"): {"3 lights": 583, "1 light, shadows": 583},
           ("m_cap7", "e"): {"1custom, no mirrors": 404, "1custom, depth 2": 706, "1custom, depth 3": 737,
                             "8, no mirrors": 754, "8, depth 2": 1305, "8, depth 3": 1368},
           ("kd_on_od", "c"): {"1 light, shadows": 20, "3 lights, shadows": 34},
           ("kd_in_power", "c"): {"1 light, shadows": 24, "3 lights, shadows": 32},
           ("ks_in_power", "c"): {"1 light, shadows": 93, "3 lights, shadows": 150},
           ("m+1", "c"): {"1 light, shadows": 298, "3 lights, shadows": 484},
           ("powf32", "c"): {"1 light, shadows": 111, "3 lights, shadows": 195},
           ("sum_order", "c"): {"1 light, shadows": 79, "3 lights, shadows": 242}}
#   scene E, per light set: {(weight, end): level-0 pixels of its object that differ from the default and lie below the clamp}, and
#   the level-0 pixels of object E_M8 that m = 7 would change
ENDS_E = {"1custom": {("ka", 0): 1309, ("ka", 16): 1289, ("kd", 0): 1289, ("kd", 16): 1309, ("ks", 0): 861, ("ks", 16): 28836},
          "8": {("ka", 0): 1309, ("ka", 16): 1289, ("kd", 0): 1289, ("kd", 16): 1309, ("ks", 0): 861, ("ks", 16): 28932}}
M8_E = {"1custom": 404, "8": 754}


def test_scene_c_both_planes_and_three_objects_per_level_show():
    trace, fin, configs = edge_scene("c")
    assert set(fin) == set(range(10)) - {6} and fin[RG.C_FLOOR] != fin[RG.C_SHEET]
    for name, (lights, _) in configs.items():
        got = {obj: tuple(shows(trace, lights, fin, j)[obj] for j in range(3)) for obj in fin}
        print(name, got)
        for obj, counts in SHOWS_C[name].items():
            assert all(g >= m // 2 for g, m in zip(got[obj], counts)), (name, obj, got[obj], counts)
        floors = {obj: tuple(m // 2 for m in counts) for obj, counts in SHOWS_C[name].items()}
        for plane in (RG.C_FLOOR, RG.C_SHEET):
            assert floors[plane][0] >= 1 and floors[plane][1] >= 1, (name, plane)
        for j in range(3):
            assert sum(f[j] >= 1 for f in floors.values()) >= 3, (name, j)


def test_scene_d_eight_finished_spheres_show_at_levels_0_and_1():
    trace, fin, configs = edge_scene("d")
    assert set(fin) == set(range(0, RG.D_NS, 3)) | {RG.D_FLOOR}
    for f in fin.values():
        assert 0.0 <= f[0] <= 1.0 and 0.2 <= f[1] <= 1.5 and 0.0 <= f[2] <= 2.0 and 0 <= f[3] <= 8
        assert not any(RF.power_of_two(v) for v in f[:3])
    for name, (lights, _) in configs.items():
        per = [shows(trace, lights, fin, j) for j in range(3)]
        got = tuple(sum(1 for o, n in per[j].items() if n and o < RG.D_NS) for j in (0, 1)) + tuple(sum(per[j].values()) for j in range(3))
        print(name, got)
        want = SHOWS_D[name]
        assert all(g >= m // 2 for g, m in zip(got, want)), (name, got, want)
        assert got[0] >= 8 and got[1] >= 8, (name, got)


def test_every_m_and_both_ends_of_the_weights_reach_a_kernel():
    ms = {f[3] for fin in (RF.C_FINISHES, RF.d_finishes(), RF.E_FINISHES) for f in fin.values()}
    assert ms == set(range(9))
    E = RF.E_FINISHES
    assert {f[3] for f in E.values()} >= {1, 2, 4, 6, 8} and E[RF.E_M8][3] == 8
    for (w, end), obj in RF.E_ENDS.items():
        assert E[obj]["ka kd ks".split().index(w)] == end
    assert any(v == 0.0 and np.signbit(v) for v in E[RF.E_MINUS_ZERO][:3])
    p, sph, pl = RF.scene_e()[:3]
    assert 16.0 * max(sph[:, 4:7].max(), pl[:, 6:9].max()) / 255.0 < 1.0


def test_creation_orders_interleave_and_keep_each_kind_in_order():
    ns, npl = len(RG.C_SPH), len(RG.C_PL)
    orders = RF.creation_orders(ns, npl)
    assert len(orders) >= 2
    for order, index in orders:
        assert [i for k, i in order if k == "s"] == list(range(ns)) and [i for k, i in order if k == "p"] == list(range(npl))
        assert sorted(index) == list(range(ns + npl))
        assert all(order[index[i]] == (("s", i) if i < ns else ("p", i - ns)) for i in range(ns + npl))
        kinds = "".join(k for k, _ in order)
        assert "sps" in kinds and kinds != "s" * ns + "p" * npl
    assert [k for k, _ in orders[0][0]][:2] == ["p", "s"] and [k for k, _ in orders[1][0]][:3] == ["s", "p", "s"]


@pytest.mark.parametrize("wrong,scene", AIMS)
def test_every_wrong_lookup_and_rule_would_be_seen_at_the_edges(wrong, scene):
    if scene == "e":
        frames = {name: (trace, lights, depth, False) for name, (trace, lights, depth) in e_frames().items()}
        fin = RF.E_FINISHES
    else:
        trace, fin, configs = edge_scene(scene)
        frames = {name: (trace, lights, 3, shadows) for name, (lights, shadows) in configs.items()}
    got = {name: changed(trace, lights, fin, depth, shadows, wrong) for name, (trace, lights, depth, shadows) in frames.items()}
    print(wrong, scene, got)
    want = CHANGED[(wrong, scene)]
    assert set(want) == set(got)
    for name in got:
        assert got[name] >= max(5, want[name] // 2), (wrong, scene, name, got[name], want[name])


@pytest.mark.parametrize("which", SETS)
def test_scene_e_both_ends_of_every_weight_and_m_8_show(which):
    trace = RF.scene_e()[6]
    lights = _lights(which)
    E = RF.E_FINISHES
    per = shows(trace, lights, E, 0)
    got = {pair: per[obj] for pair, obj in RF.E_ENDS.items()}
    fin = _level_colours(trace, lights, E, 0)
    capped = _level_colours(trace, lights, {**E, RF.E_M8: E[RF.E_M8][:3] + (7,)}, 0)
    m8 = int((_differs(fin, capped) & (trace["levels"][0]["gid"] == RF.E_M8)).sum())
    print(which, got, m8)
    for pair, n in got.items():
        assert n >= max(20, ENDS_E[which][pair] // 2), (which, pair, n)
    assert m8 >= max(20, M8_E[which] // 2), (which, m8)
