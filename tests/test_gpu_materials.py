"""The three per-object surface attributes on the GPU where they meet: one book, one flag, one upload (csrc/rtx_materials.hpp,
upload_materials in csrc/rtx_render.cpp).  The per-feature files judge each attribute's pixels (tests/test_gpu_reflect.py,
test_gpu_pattern.py, test_gpu_glass.py); here only frames of the library are compared with frames of the library, byte for byte.
The scene: 5 spheres and 1 plane at 32 x 16 cells, the smallest frame with two 16 x 16 tiles on the mirror path; one sphere a
mirror, another glass (ior 1.5; an ior shows where k > 0, so it has a k as well), a third and the plane patterned; one light,
shadows on.  Byte-equal: RTX_OPT_SORTED_STORE 0 and 1, before and after a camera move; after rtx_scene_remove_objects of the first
sphere and a fresh context built from the survivors; after setting one attribute alone and a fresh context in that state.  A graph
recorded before such a setter is refused afterwards, one recorded after it replays.  Scenes this small keep no direction-sorted
copy (it starts at 256 spheres), so the same store and camera comparison runs once more on 300 spheres, where the copies by
sorted position are the ones the kernels read."""
import numpy as np
import pytest

import oracle as O
import util as U
import test_gpu_reflect as T

pytestmark = pytest.mark.gpu

W, H = 32, 16
MODE = O.RGB_ASCII
# five spheres in two columns (x y z r, rgb; a console cell is tall, so the view is narrow) over Scene3D::Init's plane: every object
# shows in both poses
SPHERES = np.array([[-2.5, 3.0, 24.0, 2.4, 255.0, 1.0, 1.0], [2.5, 3.0, 24.0, 2.4, 1.0, 255.0, 1.0], [-2.5, 10.0, 24.0, 2.4, 1.0, 1.0, 255.0],
                    [2.5, 10.0, 24.0, 2.4, 225.0, 210.0, 20.0], [0.0, 17.0, 26.0, 2.4, 225.0, 10.0, 220.0]], dtype=np.float32)
PLANE = np.array([[0.0, -3.0, 30.0, 0.0, 1.0, 0.0, 100.0, 100.0, 100.0, 10.0, 20.0]], dtype=np.float32)
N = len(SPHERES) + len(PLANE)
# by creation index: sphere 0 a mirror, sphere 1 glass, sphere 2 and the plane (5) patterned
STATE = {"k": {0: 0.6, 1: 0.8}, "ior": {1: 1.5}, "slot": {2: 1, 5: 2}}
TABLE = [((0.0, 0.0, 0.0), (0.5, 0.0, 0.5), (20.0, 20.0, 200.0)), ((1.0, 0.0, 2.0), (0.25, 0.25, 0.25), (250.0, 250.0, 250.0))]
POSES = [(None, None), ((0.5, 2.0, -3.0), (0.05, 3.1615927, 0.0))]


@pytest.fixture(scope="module")
def R():
    return U.pkg()


def _context(R, spheres, planes, state, store=-1):
    """A fresh context in `state`: one light, shadows on, the table, every attribute by creation index."""
    c = R.Context(W, H)
    c.set_option(R.OPT_SORTED_STORE, store)
    c.set_scene(spheres, planes)
    c.set_option(R.OPT_SHADOWS, 1)
    c.set_light(R.make_light(pos=(-20.0, 40.0, -10.0)))
    c.set_patterns([R.make_pattern(*t) for t in TABLE])
    _apply(c, state)
    return c


def _apply(c, state):
    for i, k in state["k"].items():
        c.set_reflectivity(i, k)
    for i, ior in state["ior"].items():
        c.set_refraction(i, ior)
    for i, slot in state["slot"].items():
        c.set_object_pattern(i, slot)


def _frame(R, c, pose=POSES[0]):
    return T._rows(R, c, R.camera_params(W, H, *pose), MODE).tobytes()


def _counts(R, c):
    return [c.get_option(o) for o in (R.STAT_REFLECT_FRAMES, R.STAT_PATTERN_FRAMES, R.STAT_REFRACT_FRAMES)]


def _store_and_camera(R, spheres, planes, state):
    """Frames under RTX_OPT_SORTED_STORE 0 and 1 at both poses, each context moving from the first pose to the second and back."""
    frames = {}
    for store in (0, 1):
        with _context(R, spheres, planes, state, store) as c:
            frames[store] = [_frame(R, c, POSES[0]), _frame(R, c, POSES[1]), _frame(R, c, POSES[0])]
            # the option flipped in place: the next launch sorts again (or drops the copy), around the camera it has by then
            c.set_option(R.OPT_SORTED_STORE, 1 - store)
            frames[store] += [_frame(R, c, POSES[1]), _frame(R, c, POSES[0])]
            assert min(_counts(R, c)) >= 5  # every frame took the mirror path, with patterns and with glass
    a, b = frames[0][0], frames[0][1]
    assert a != b, "the camera move changes nothing"
    assert frames[0] == [a, b, a, b, a] and frames[1] == frames[0]
    return a


def test_store_and_camera_leave_the_bytes(R):
    with _context(R, SPHERES, PLANE, {"k": {}, "ior": {}, "slot": {}}) as c:
        plain = _frame(R, c)
        assert _counts(R, c) == [0, 0, 0]
    seen = {plain}
    # each attribute shows in this view, so that the comparisons below compare something
    for leave_out in ("k", "ior", "slot"):
        state = dict(STATE, **{leave_out: {} if leave_out != "k" else {0: 0.6}})
        with _context(R, SPHERES, PLANE, state) as c:
            seen.add(_frame(R, c))
    seen.add(_store_and_camera(R, SPHERES, PLANE, STATE))
    assert len(seen) == 5


def test_store_and_camera_leave_the_bytes_where_the_scene_is_sorted(R):
    p = R.camera_params(W, H)
    sph, _ = R.synth_scene(11, 300, 0, p.element1, p.element2)
    sph = np.concatenate([SPHERES, sph])
    k = {i: 0.5 for i in range(0, len(sph), 3)}
    state = {"k": {**k, **STATE["k"]}, "ior": {**{i: 1.25 for i in list(k)[::2]}, **STATE["ior"]},
             "slot": {**{i: 1 + i % 2 for i in range(1, len(sph), 5)}, len(sph): 2}}
    _store_and_camera(R, sph, PLANE, state)


def test_removal_is_a_fresh_context_of_the_survivors(R):
    with _context(R, SPHERES, PLANE, STATE) as c:
        before = _frame(R, c)
        c.remove_objects([0])
        got = _frame(R, c)
        assert [c.get_reflectivity(i) for i in range(N - 1)] == [float(np.float32(STATE["k"].get(i + 1, 0.0))) for i in range(N - 1)]
        assert [c.get_refraction(i) for i in range(N - 1)] == [STATE["ior"].get(i + 1, 0.0) for i in range(N - 1)]
        assert [c.get_object_pattern(i) for i in range(N - 1)] == [STATE["slot"].get(i + 1, 0) for i in range(N - 1)]
    survivors = {name: {i - 1: v for i, v in STATE[name].items() if i != 0} for name in STATE}
    with _context(R, SPHERES[1:], PLANE, survivors) as fresh:
        want = _frame(R, fresh)
    assert got == want and got != before


# one attribute alone: (name, the setter's arguments, the state afterwards)
ALONE = [("k", lambda c: c.set_reflectivity(3, 0.4), dict(STATE, k={0: 0.6, 1: 0.8, 3: 0.4})),
         ("ior", lambda c: c.set_refraction(0, 2.0), dict(STATE, ior={0: 2.0, 1: 1.5})),
         ("slot", lambda c: c.set_object_pattern(4, 1), dict(STATE, slot={2: 1, 4: 1, 5: 2}))]
STALE_TEXT = {"k": "the reflectivities changed", "ior": "the indices of refraction changed", "slot": "the pattern table or the objects' slots changed"}


def _record(R, c, pp, s, buf):
    c.graph_begin(s.cuda_stream)
    c.render_rows(pp, MODE, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    return c.graph_end(s.cuda_stream)


def _replay(c, g, s, buf):
    buf.fill_(0xEE)
    c.graph_launch(g, s.cuda_stream)
    s.synchronize()
    return buf.cpu().numpy().tobytes()


def test_one_attribute_alone_uploads_all_and_stales_graphs(R):
    import torch
    pp = R.camera_params(W, H)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with _context(R, SPHERES, PLANE, STATE) as c:
        state, last = STATE, _frame(R, c)  # (render once before capturing: the device copies are uploaded here)
        for name, setter, after in ALONE:
            after = {n: {**state[n], **after[n]} for n in state}  # (the setters accumulate on this one context)
            before = _record(R, c, pp, s, buf)
            try:
                assert _replay(c, before, s, buf) == last
                setter(c)
                with pytest.raises(R.RtxError) as e:
                    c.graph_launch(before, s.cuda_stream)
                assert e.value.status == R.ERR_INVALID_ARGUMENT and STALE_TEXT[name] in str(e.value)
            finally:
                c.graph_destroy(before)
            got = _frame(R, c)
            with _context(R, SPHERES, PLANE, after) as fresh:
                assert got == _frame(R, fresh), name
            assert got != last, name
            recorded = _record(R, c, pp, s, buf)
            try:
                assert _replay(c, recorded, s, buf) == got
            finally:
                c.graph_destroy(recorded)
            state, last = after, got
