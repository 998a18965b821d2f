"""The input conditions of tests/test_gpu_finish.py, judged on the restatement alone (tests/restate_finish.py; CPU, no GPU): scene F
is restate.chain_scene("mirror_floor") with restate_finish.F_FINISHES, under the light sets `1custom` and `8`.
  (a) with the default finish the restated rule is restate._shade_lights bit for bit on every hit pixel of levels 0 .. 2;
  (b) every finished object shows at each of levels 0, 1 and 2: at least 100 pixels whose level hit it, whose colour there differs
      from the default finish's and has a component below the 255 clamp;
  (c) every wrong= variant of the restatement (a bug a kernel could have) differs from the rule in some colour bit on at least 100
      hit pixels at level 0 and on at least 10 at level 2.
The bounds are conditions on the inputs, not tolerances: the GPU tests compare bit for bit."""
import numpy as np
import pytest

import restate as RS
import restate_finish as RF

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
