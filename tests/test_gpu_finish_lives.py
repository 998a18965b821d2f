"""Finishes through a scene's life on the GPU, library against library, byte for byte (the pixels themselves:
tests/test_gpu_finish.py).  The small scene of tests/test_gpu_materials.py at 32 x 16 cells -- a mirror, a glass sphere, two
patterned objects, one light, shadows on -- with four finishes, and the 300 spheres of restate_pattern.sorted_scene() at 320 x 180
with a finish on every third sphere, where the copies by sorted position are the ones the kernels read.
  * RTX_OPT_SORTED_STORE 0 against 1, before and after a camera move;
  * rtx_scene_set_spheres on a finished sphere; rtx_scene_remove_objects of the first sphere against a fresh context of the survivors;
  * a device group of three logical ranks against one device, a refused call on the group;
  * RTX_OPT_SUPERSAMPLE 2 against restate_supersample.fold of the library's own 2W x 2H values frame;
  * a graph recorded before rtx_scene_set_finish is refused after it, and one recorded after it replays to the same bytes;
  * rtx_update_half's stream replays (restate_half.replay) to the finished colours."""
import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_half as RH
import restate_pattern as RP
import restate_supersample as SS
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC
import test_gpu_half as TH
import test_gpu_materials as TM

pytestmark = pytest.mark.gpu

W, H = TM.W, TM.H
MODE = TM.MODE
FINISHES = {0: (0.2, 1.0, 0.0, 5), 1: (0.1, 0.8, 1.7, 7), 3: (0.8, 0.3, 1.0, 0), 5: (0.3, 1.0, 0.6, 3)}  # (by creation index; 5: the plane)
STATE = dict(TM.STATE, finish=FINISHES)
SORTED_FINISH = (0.35, 0.7, 1.3, 3)


@pytest.fixture(scope="module")
def R():
    return U.pkg()


def _apply(c, state):
    TM._apply(c, state)
    for i, f in state.get("finish", {}).items():
        c.set_finish(i, [f])


def _context(R, spheres, planes, state, store=-1, devices=None, w=W, h=H):
    c = R.Context(w, h) if devices is None else R.Context(w, h, devices=devices)
    c.set_option(R.OPT_SORTED_STORE, store)
    c.set_scene(spheres, planes)
    c.set_option(R.OPT_SHADOWS, 1)
    c.set_light(R.make_light(pos=(-20.0, 40.0, -10.0)))
    c.set_patterns([R.make_pattern(*t) for t in TM.TABLE])
    _apply(c, state)
    return c


def _frame(R, c, pose=TM.POSES[0]):
    return T._rows(R, c, R.camera_params(W, H, *pose), MODE).tobytes()


def test_the_finishes_show_in_this_view(R):
    seen = set()
    for leave_out in (None, 0, 1, 3, 5):
        state = dict(STATE, finish={i: f for i, f in FINISHES.items() if i != leave_out})
        with _context(R, TM.SPHERES, TM.PLANE, state) as c:
            seen.add(_frame(R, c))
            assert c.get_option(R.STAT_FINISH_FRAMES) == 1 and c.get_option(R.STAT_FINISHED_OBJECTS) == len(state["finish"])
    assert len(seen) == 5


def test_store_and_camera_leave_the_bytes(R):
    frames = {}
    for store in (0, 1):
        with _context(R, TM.SPHERES, TM.PLANE, STATE, store) as c:
            frames[store] = [_frame(R, c, TM.POSES[0]), _frame(R, c, TM.POSES[1]), _frame(R, c, TM.POSES[0])]
            c.set_option(R.OPT_SORTED_STORE, 1 - store)
            frames[store] += [_frame(R, c, TM.POSES[1]), _frame(R, c, TM.POSES[0])]
            assert c.get_option(R.STAT_FINISH_FRAMES) == 5
    a, b = frames[0][0], frames[0][1]
    assert a != b and frames[0] == [a, b, a, b, a] and frames[1] == frames[0]


def _sorted_frames(R, store, finished):
    """The 300-sphere scene under `store`, every third sphere finished (or none): values before and after a camera move."""
    p, sph, pl = RP.sorted_scene()[:3]
    w, h = RP.SORTED_W, RP.SORTED_H
    poses = [TC._params(p), TC._params(O.camera_params(w, h, pos=(1.5, 1.0, -2.0), rot=(0.04, RS.PI32 + 0.03, 0.0)))]
    with R.Context(w, h) as c:
        c.set_option(R.OPT_SORTED_STORE, store)
        c.set_scene(sph, pl)
        c.set_light(R.make_light(pos=(5.0, 40.0, 10.0), diffuse_power=900.0, specular_power=2100.0))
        if finished:
            for i in range(0, RP.SORTED_NS, 3):
                c.set_finish(i, [SORTED_FINISH])
            c.set_finish(RP.SORTED_NS, [(0.2, 1.0, 0.0, 5)])  # the floor: matt
            assert c.get_option(R.STAT_FINISHED_OBJECTS) == RP.SORTED_NS // 3 + 1
        out = [T._rows(R, c, pp, MODE, R.RENDER_VALUES).tobytes() for pp in (poses[0], poses[1], poses[0])]
        assert c.last_kernel.startswith("rtx_shadow_shade<"), c.last_kernel
    return out


def test_the_sorted_copies_carry_the_finishes(R):
    plain = _sorted_frames(R, 1, False)
    off, on = _sorted_frames(R, 0, True), _sorted_frames(R, 1, True)
    assert off[0] != off[1] and off[0] == off[2]
    assert on == off
    # the finishes are in the picture at both poses: many pixels differ from the unfinished frame
    for a, b in zip(plain[:2], on[:2]):
        va, vb = np.frombuffer(a, np.float32).reshape(-1, 8), np.frombuffer(b, np.float32).reshape(-1, 8)
        assert np.array_equal(va[:, :5].view(np.uint32), vb[:, :5].view(np.uint32))  # (distance, glyph value and normal do not depend on a finish)
        assert int((va[:, 5:] != vb[:, 5:]).any(axis=1).sum()) >= 1000


def test_an_edit_keeps_the_finish_and_removal_is_a_fresh_context_of_the_survivors(R):
    n = TM.N
    moved = TM.SPHERES.copy()
    moved[1, 1] += 1.0
    with _context(R, TM.SPHERES, TM.PLANE, STATE) as c:
        before = _frame(R, c)
        c.set_spheres(1, moved[1])
        got = _frame(R, c)
        with _context(R, moved, TM.PLANE, STATE) as fresh:
            assert got == _frame(R, fresh) and got != before
        c.remove_objects([0])
        after = _frame(R, c)
        fin = [c.get_finish(i) for i in range(n - 1)]
        want = [FINISHES.get(i + 1, (0.2, 1.0, 1.0, 5)) for i in range(n - 1)]
        assert [(f.ambient, f.diffuse, f.specular, f.shininess_log2) for f in fin] == [tuple(np.float32(v) for v in w[:3]) + (w[3],) for w in want]
        assert c.get_option(R.STAT_FINISHED_OBJECTS) == 3
    survivors = {name: {i - 1: v for i, v in STATE[name].items() if i != 0} for name in STATE}
    with _context(R, moved[1:], TM.PLANE, survivors) as fresh:
        assert after == _frame(R, fresh) and after != got


def test_a_group_of_three_ranks_gives_the_one_device_frame(R):
    pp = R.camera_params(W, H)
    with _context(R, TM.SPHERES, TM.PLANE, STATE) as c, _context(R, TM.SPHERES, TM.PLANE, STATE, devices=[0, 0, 0]) as g:
        want = c.render_to_host(pp, MODE)
        assert np.array_equal(g.render_to_host(pp, MODE), want)
        with pytest.raises(R.RtxError) as e:  # validated on the root before any rank is touched
            g.set_finish(0, [(0.5, 0.5, 0.5, 5), (0.5, -1.0, 0.5, 5)])
        assert "object 1:" in str(e.value)
        f = g.get_finish(0)
        assert (f.ambient, f.diffuse, f.specular, f.shininess_log2) == (np.float32(0.2), 1.0, 0.0, 5)
        assert np.array_equal(g.render_to_host(pp, MODE), want)
        g.set_finish(2, [(0.6, 0.6, 0.6, 6)])
        c.set_finish(2, [(0.6, 0.6, 0.6, 6)])
        other = c.render_to_host(pp, MODE)
        assert not np.array_equal(other, want) and np.array_equal(g.render_to_host(pp, MODE), other)


def test_supersampling_folds_the_finished_sample_frame(R):
    S = 2
    p = R.camera_params(W, H)
    ps = SS.sample_params(p, S)
    with _context(R, TM.SPHERES, TM.PLANE, STATE, w=S * W, h=S * H) as c:
        samples = T._rows(R, c, ps, MODE, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
        want = SS.fold(samples, W, H, S, float(p.cam_far))
        c.set_option(R.OPT_SUPERSAMPLE, S)
        got = T._rows(R, c, p, MODE, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
        assert c.last_kernel.startswith("rtx_resolve<%d," % S), c.last_kernel
        same = RS.same_floats(got, want)
        assert same.all(), "%d cells differ" % int((~same.all(axis=1)).sum())
        assert c.get_option(R.STAT_FINISH_FRAMES) >= 2
    with _context(R, TM.SPHERES, TM.PLANE, TM.STATE, w=S * W, h=S * H) as c:  # (and the fold is of finished samples)
        c.set_option(R.OPT_SUPERSAMPLE, S)
        assert T._rows(R, c, p, MODE, R.RENDER_VALUES).tobytes() != got.tobytes()


def test_a_graph_recorded_before_a_change_is_refused(R):
    import torch
    pp = R.camera_params(W, H)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with _context(R, TM.SPHERES, TM.PLANE, STATE) as c:
        last = _frame(R, c)  # (render once before capturing: the device copies are uploaded here)
        before = TM._record(R, c, pp, s, buf)
        try:
            assert TM._replay(c, before, s, buf) == last
            c.set_finish(2, [(0.5, 0.9, 1.2, 6)])
            with pytest.raises(R.RtxError) as e:
                c.graph_launch(before, s.cuda_stream)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and "the finishes changed" in str(e.value) and "re-capture" in str(e.value)
        finally:
            c.graph_destroy(before)
        got = _frame(R, c)
        assert got != last
        with _context(R, TM.SPHERES, TM.PLANE, dict(STATE, finish={**FINISHES, 2: (0.5, 0.9, 1.2, 6)})) as fresh:
            assert got == _frame(R, fresh)
        recorded = TM._record(R, c, pp, s, buf)
        try:
            assert TM._replay(c, recorded, s, buf) == got
        finally:
            c.graph_destroy(recorded)


def test_update_half_shows_the_finished_colours(R):
    mode = O.RGB_PIXEL
    console = R.camera_params(W, H)
    console.y = H // 2
    pp = TH.sample_params(R, console)
    assert (int(pp.x), int(pp.y)) == (W, H)
    streams = {}
    for name, state in (("finished", STATE), ("plain", TM.STATE)):
        with _context(R, TM.SPHERES, TM.PLANE, state) as c:
            words = T._rows(R, c, pp, mode, R.RENDER_COMPACT).view(np.uint32)
            stream = bytes(c.update_half(console, mode))
            assert stream == TH.run_half(R, c, mode, W, H // 2, words)
            assert RH.replay(mode, stream, W, H // 2) == RH.keys(mode, W, H // 2, words)
            streams[name] = stream
    assert streams["finished"] != streams["plain"]
