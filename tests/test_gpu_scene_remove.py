"""Scene objects removed in place -- rtx_scene_remove_objects, rtx_scene_remove_marked_device -- against a yardstick that is never
the code under test: a context F built afresh from the survivors, whose values are read with get_object from the context under
test BEFORE the removal and whose motion and reflectivity are then set on F; and the CPU oracle, whose scene is built in the same
creation order, stepped by its own physics and rebuilt without the removed objects.
   1. removed equals rebuilt: seven removal sets x sorted copy on / off, every mode and output form, brute and binned kernel;
   2. indices: rtx_pick over every cell and rtx_query_rays answer with the NEW creation indices; coincident spheres keep the tie-break;
   3. caches do not survive: cached cell lists, the world grid, a recorded graph;
   4. every shading path reads the removal: lights and shadows, mirrors with shadows in them, the shadow grid; the last mirror gone;
   5. physics steps and rtx_update after a removal;  6. errors are all or nothing;  7. the device form behind a busy stream;
   8. a device group;  9. add, remove, add, edit, remove interleaved.
The planes of every scene have axis-aligned normals: rtx_scene_add_plane normalises what it is given, and only for such a normal is
the normalised value it gave back through get_object certain to normalise to itself bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import restate as RS
import util as U
import test_gpu_chain_lights as TC
import test_gpu_scene_edit as TE

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 96, 40
COUNT = 302                      # the base scene: spheres 0 .. 99, plane 100, spheres 101 .. 300, plane 301
PLANE_A, PLANE_B = 100, 301
STEPS = (0.016, 0.033, 0.25)
MODES = (O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS)


@pytest.fixture(scope="module")
def R():
    return U.pkg()


def _gidx_of_sphere(k):
    """creation index of sphere local k in the base scene"""
    return k if k < 100 else k + 1


# ---------------------------------------------------------------- the yardsticks

def _snapshot(c):
    """Every object of c as get_object / get_reflectivity report it: [(kind, 11 floats, k)]."""
    return [c.get_object(i) + (c.get_reflectivity(i),) for i in range(c.object_count)]


def _fresh(R, objs, w=W, h=H, **kw):
    """A context to which `objs` (a snapshot, or its survivors) are added in their order with their values; then motion and k."""
    F = R.Context(w, h, **kw)
    run = []

    def flush():
        if run:
            F.add_spheres(np.array(run, dtype=np.float32))
            del run[:]

    for kind, v, _ in objs:
        if kind == 2:
            run.append(v[:7])
        else:
            flush()
            F.add_plane(v[0:3], v[3:6], v[6:9], float(v[9]), float(v[10]))
    flush()
    for i, (kind, v, k) in enumerate(objs):
        if kind == 2 and (v[7], v[8]) != (-1.0, 1.0):
            F.set_sphere_motion(i, int(v[7]), float(v[8]))
    if any(k != 0.0 for _, _, k in objs):
        F.set_reflectivity(0, np.array([k for _, _, k in objs], dtype=np.float32))
    return F


def _survivors(objs, removed):
    gone = set(int(i) for i in removed)
    return [o for i, o in enumerate(objs) if i not in gone]


def _new_index(removed, i):
    """THE RULE of include/rtx.h: i - |{r in R : r < i}|."""
    return i - sum(1 for r in removed if r < i)


def _oracle_copy(objs):
    """A new oracle scene of these oracle objects, in their order (through the public add calls: floats round-trip exactly)."""
    s = O.Scene()
    for o in objs:
        if o.type == O.SPHERE:
            s.add_sphere(o.radius, (o.center.x, o.center.y, o.center.z), (o.color.x, o.color.y, o.color.z), o.mover, o.speed)
        else:
            s.add_plane((o.center.x, o.center.y, o.center.z), (o.normal.x, o.normal.y, o.normal.z), (o.color.x, o.color.y, o.color.z),
                        o.width, o.height)
    return s


def _oracle_without(sc, removed):
    gone = set(int(i) for i in removed)
    return _oracle_copy([o for i, o in enumerate(sc.objects()) if i not in gone])


def _oracle_step(sc, dt):
    O.lib().orc_update_objects(sc.ptrs(), sc.count, dt)


_base = {}


def _base_case(R):
    """The base scene's inputs, its oracle scene after the ageing below, the oracle's frame of it, and a sphere the frame shows."""
    if not _base:
        p = R.camera_params(W, H)
        sph, pl = R.synth_scene(41, 300, 2, p.element1, p.element2)
        sc = O.Scene()
        for i, row in enumerate(sph):
            if i == 100:
                q = pl[0]
                sc.add_plane(q[0:3], q[3:6], q[6:9], q[9], q[10])
            sc.add_sphere(row[3], row[0:3], row[4:7])
        q = pl[1]
        sc.add_plane(q[0:3], q[3:6], q[6:9], q[9], q[10])
        assert sc.count == COUNT and sc.objects()[PLANE_A].type == O.PLANE and sc.objects()[PLANE_B].type == O.PLANE
        sc.objects()[40].mover, sc.objects()[40].speed = 3, 2.5
        for dt in STEPS:
            _oracle_step(sc, dt)
        op = U.oracle_params(p)
        before = O.render(op, sc, O.RGB_ASCII)
        visible = None
        for i in range(COUNT):
            if i not in (PLANE_A, PLANE_B) and not np.array_equal(O.render(op, _oracle_without(sc, [i]), O.RGB_ASCII), before):
                visible = i
                break
        assert visible is not None, "the scene shows no sphere: change the scene"
        _base.update(p=p, op=op, sph=sph, pl=pl, sc=sc, before=before, visible=visible)
    return _base


def _aged_base(R, c):
    """The base scene into c, interleaved, then a sphere's motion set and three physics steps: the device values differ from the
    creation values, and only the device knows them."""
    b = _base_case(R)
    sph, pl = b["sph"], b["pl"]
    c.add_spheres(sph[:100])
    c.add_plane(pl[0][0:3], pl[0][3:6], pl[0][6:9], float(pl[0][9]), float(pl[0][10]))
    c.add_spheres(sph[100:])
    c.add_plane(pl[1][0:3], pl[1][3:6], pl[1][6:9], float(pl[1][9]), float(pl[1][10]))
    assert c.object_count == COUNT
    c.set_sphere_motion(40, 3, 2.5)
    for dt in STEPS:
        c.update_objects(dt)
    return b


def _sets(R):
    v = _base_case(R)["visible"]
    return {
        "visible": [v],
        "first_last": [COUNT - 1, 0],
        "run": [_gidx_of_sphere(k) for k in range(254, 259)],          # across the boundary of the kernel's two blocks
        "plane": [PLANE_A],                                             # only .w words change
        "second": list(range(COUNT - 1, 0, -2)),                        # every second object, listed backwards
        "spheres": [i for i in range(COUNT) if i not in (PLANE_A, PLANE_B)],
        "everything": list(np.random.default_rng(5).permutation(COUNT)),
    }


SET_NAMES = ["visible", "first_last", "run", "plane", "second", "spheres", "everything"]


def _remove(c, form, indices):
    """Through the host form, or the device form with the marks written by a torch kernel on a stream of its own behind a
    busy-wait, so that only the ordering the call promises makes them arrive.  Returns what the call says it removed."""
    indices = [int(i) for i in indices]
    if form == "host":
        c.remove_objects(indices)
        return len(indices)
    import torch
    marks = np.zeros(c.object_count, dtype=np.uint8)
    marks[indices] = np.array([1, 255, 7, 128], dtype=np.uint8)[np.arange(len(indices)) % 4]     # any non-zero byte
    src = torch.from_numpy(marks).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda._sleep(2000000)
        d = src * 1
    n = c.remove_marked_device(d.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    return n


def _assert_frames(R, c, F, p, what, kernels=None):
    kernels = kernels if kernels is not None else (R.KERNEL_BRUTE, R.KERNEL_BINNED)
    for kernel in kernels:
        for x in (c, F):
            x.set_option(R.OPT_KERNEL, kernel)
        for mode in MODES:
            got, want = TE._out(R, c, p, mode), TE._out(R, F, p, mode)
            assert np.array_equal(got, want), (what, kernel, O.MODE_NAMES[mode], U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))
        for flags in (R.RENDER_VALUES, R.RENDER_COMPACT):
            assert np.array_equal(TE._out(R, c, p, O.RGB_ASCII, flags), TE._out(R, F, p, O.RGB_ASCII, flags)), (what, kernel, flags)


def _assert_objects(c, F):
    assert c.object_count == F.object_count
    for i in range(F.object_count):
        (ka, a), (kb, b) = c.get_object(i), F.get_object(i)
        assert ka == kb and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, a, b)
        assert c.get_reflectivity(i) == F.get_reflectivity(i), i


# ---------------------------------------------------------------- 1. removed equals rebuilt

@pytest.mark.parametrize("sorted_store", [-1, 0])
@pytest.mark.parametrize("name", SET_NAMES)
def test_removed_equals_rebuilt(R, name, sorted_store):
    removed = _sets(R)[name]
    with R.Context(W, H) as c:
        c.set_option(R.OPT_SORTED_STORE, sorted_store)
        b = _aged_base(R, c)
        p = b["p"]
        got_before = TE._out(R, c, p, O.RGB_ASCII)            # (the sorted copy exists from here on)
        assert np.array_equal(got_before, b["before"]), U.first_diff(got_before, b["before"], 20, W)
        objs = _snapshot(c)
        n0 = c.get_option(R.STAT_SCENE_REMOVED)
        with _fresh(R, _survivors(objs, removed)) as F:
            F.set_option(R.OPT_SORTED_STORE, sorted_store)
            assert _remove(c, "host", removed) == len(removed)
            assert c.object_count == COUNT - len(removed) == F.object_count
            assert c.get_option(R.STAT_SCENE_REMOVED) == n0 + len(removed)
            _assert_frames(R, c, F, p, name)
            _assert_objects(c, F)
            # the rule, object by object, against the values read before the removal
            for i, (kind, v, k) in enumerate(objs):
                if i not in removed:
                    kind2, v2 = c.get_object(_new_index(removed, i))
                    assert kind2 == kind and np.array_equal(v2.view(np.uint32), v.view(np.uint32)), i
        # the oracle: its own scene, stepped by its own physics, without the removed objects
        want = O.render(b["op"], _oracle_without(b["sc"], removed), O.RGB_ASCII)
        if name in ("visible", "second"):
            assert not np.array_equal(want, b["before"]), "the removal changes nothing the frame shows: change the scene"
        for kernel in (R.KERNEL_BRUTE, R.KERNEL_BINNED):
            c.set_option(R.OPT_KERNEL, kernel)
            got = TE._out(R, c, p, O.RGB_ASCII)
            assert np.array_equal(got, want), (name, kernel, U.first_diff(got, want, 20, W))


@pytest.mark.parametrize("name", ["visible", "second", "run"])
def test_spheres_first_against_the_oracle_on_reduced_arrays(R, name):
    """The scene the oracle's from_arrays expresses (spheres first, then planes), no physics: the frame after the removal is
    O.render of the reduced arrays."""
    b = _base_case(R)
    p, sph, pl = b["p"], b["sph"], b["pl"]
    op = b["op"]
    before = O.render(op, O.Scene.from_arrays(sph, pl), O.RGB_ASCII)
    if name == "visible":
        k = next(k for k in range(300) if not np.array_equal(O.render(op, O.Scene.from_arrays(np.delete(sph, k, axis=0), pl), O.RGB_ASCII), before))
        removed = [k]
    elif name == "second":
        removed = list(range(1, 302, 2))        # every second object: 150 spheres and plane 301
    else:
        removed = list(range(254, 259)) + [300]  # the run across the block boundary and the first plane
    keep_s = [i for i in range(300) if i not in removed]
    keep_p = [i - 300 for i in (300, 301) if i not in removed]
    want = O.render(op, O.Scene.from_arrays(sph[keep_s], pl[keep_p]), O.RGB_ASCII)
    if name != "run":
        assert not np.array_equal(want, before), "the removal changes nothing the frame shows: change the scene"
    with R.Context(W, H) as c:
        c.set_scene(sph, pl)
        assert np.array_equal(TE._out(R, c, p, O.RGB_ASCII), before)
        _remove(c, "host", removed)
        for kernel in (R.KERNEL_AUTO, R.KERNEL_BRUTE, R.KERNEL_BINNED):
            c.set_option(R.OPT_KERNEL, kernel)
            got = TE._out(R, c, p, O.RGB_ASCII)
            assert np.array_equal(got, want), (name, kernel, U.first_diff(got, want, 20, W))
        got = TE._out(R, c, p, O.BIT_PIXEL)
        want = O.render(op, O.Scene.from_arrays(sph[keep_s], pl[keep_p]), O.BIT_PIXEL)
        assert np.array_equal(got, want), U.first_diff(got, want, 12, W)


# ---------------------------------------------------------------- 2. indices

def test_pick_and_queries_answer_with_the_new_indices(R):
    rng = np.random.default_rng(13)
    removed = _sets(R)["second"]
    with R.Context(W, H) as c:
        b = _aged_base(R, c)
        p = b["p"]
        objs = _snapshot(c)
        old = {(col, row): c.pick(p, col, row) for row in range(0, H, 4) for col in range(0, W - 1, 5)}
        with _fresh(R, _survivors(objs, removed)) as F:
            _remove(c, "host", removed)
            seen = set()
            for row in range(H):
                for col in range(W - 1):
                    got = c.pick(p, col, row)
                    assert got == F.pick(p, col, row), (col, row)
                    seen.add(got[1])
                    # a cell that showed a survivor before still shows it, under its new index
                    if (col, row) in old and old[(col, row)][1] != R.NO_OBJECT and old[(col, row)][1] not in removed:
                        assert got == (old[(col, row)][0], _new_index(removed, old[(col, row)][1])), (col, row)
            assert len(seen - {R.NO_OBJECT}) >= 20 and max(seen - {R.NO_OBJECT}) < c.object_count
            centres = np.array([v[0:3] for kind, v, _ in _survivors(objs, removed) if kind == 2], dtype=np.float32)
            target = centres[rng.integers(0, len(centres), 4096)] + rng.normal(scale=1.0, size=(4096, 3)).astype(np.float32)
            origin = np.array(p.cam_pos[:], dtype=np.float32) + rng.normal(scale=3.0, size=(4096, 3)).astype(np.float32)
            rays = R.make_rays(origin, target - origin)
            want = F.query_rays(rays, R.QUERY_CLOSEST)
            for check in (0, 1):
                c.set_option(R.OPT_QUERY_CHECK, check)
                got = c.query_rays(rays, R.QUERY_CLOSEST)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), check
            hit = got["index"][got["index"] != R.NO_OBJECT]
            assert hit.size >= 1024 and hit.max() < c.object_count


def test_coincident_spheres_keep_the_tie_break(R):
    """Three spheres in one place, in three colours, created after a plane and a sphere elsewhere: every hit is an exact tie, which
    the lowest surviving creation index wins (RayTracing.cu:123) -- before the removal, after the first of them is removed, and
    after the plane created before them is removed as well.  Against the oracle's frames of the same lists."""
    p = R.camera_params(W, H)
    op = U.oracle_params(p)
    plane = np.array([0, -30, 125, 0, 1, 0, 100, 100, 100, 400, 250], dtype=np.float32)
    far = np.array([30, 10, 150, 4, 9, 200, 90], dtype=np.float32)
    twins = [np.array([0, 0, 60, 8] + rgb, dtype=np.float32) for rgb in ([250, 10, 10], [10, 250, 10], [10, 10, 250])]

    def oracle_frame(objs):
        s = O.Scene()
        for o in objs:
            if o.size == 11:
                s.add_plane(o[0:3], o[3:6], o[6:9], o[9], o[10])
            else:
                s.add_sphere(o[3], o[0:3], o[4:7])
        return O.render(op, s, O.RGB_ASCII)

    objs = [plane, far] + twins             # creation indices: plane 0, far 1, twins 2 3 4
    centre = (H // 2) * W + W // 2
    with R.Context(W, H) as c:
        for o in objs:
            if o.size == 11:
                c.add_plane(o[0:3], o[3:6], o[6:9], float(o[9]), float(o[10]))
            else:
                c.add_sphere(float(o[3]), o[0:3], o[4:7])
        frames = []
        for step, removed in enumerate((None, [2], [0])):
            if removed is not None:
                c.remove_objects(removed)
                objs = [o for i, o in enumerate(objs) if i not in removed]
            want = oracle_frame(objs)
            for kernel in (R.KERNEL_BRUTE, R.KERNEL_BINNED):
                c.set_option(R.OPT_KERNEL, kernel)
                got = TE._out(R, c, p, O.RGB_ASCII)
                assert np.array_equal(got, want), (step, kernel, U.first_diff(got, want, 20, W))
            frames.append(want.reshape(-1, 20)[centre].copy())
            idx = c.pick(p, W // 2, H // 2)[1]
            assert idx == (2, 2, 1)[step], (step, idx)      # the red twin; the green one, now object 2; the same, now object 1
        assert not np.array_equal(frames[0], frames[1])     # red, then green
        assert np.array_equal(frames[1], frames[2])         # ... and still green without the plane


# ---------------------------------------------------------------- 3. caches do not survive

def test_cached_cell_lists_do_not_survive(R):
    removed = _sets(R)["second"]
    with R.Context(W, H) as c:
        b = _aged_base(R, c)
        p = b["p"]
        objs = _snapshot(c)
        with _fresh(R, _survivors(objs, removed)) as F:
            for x in (c, F):
                x.set_option(R.OPT_KERNEL, R.KERNEL_BINNED)
                x.set_option(R.OPT_TWO_LEVEL, 1)
                x.set_option(R.OPT_CELL_REUSE, 1)
            for _ in range(2):                                      # at rest: the lists are cached
                TE._out(R, c, p, O.RGB_ASCII)
            s1 = TE._cell_stats(R, c)
            print("cell lists after two frames at rest:", s1)
            assert s1["builds"] + s1["per_frame"] >= 1, s1
            _remove(c, "host", removed)
            got, want = TE._out(R, c, p, O.RGB_ASCII), TE._out(R, F, p, O.RGB_ASCII)
            assert np.array_equal(got, want), U.first_diff(got, want, 20, W)
            s2 = TE._cell_stats(R, c)
            assert s2["builds"] + s2["per_frame"] > s1["builds"] + s1["per_frame"], (s1, s2)
            want = O.render(b["op"], _oracle_without(b["sc"], removed), O.RGB_ASCII)
            assert np.array_equal(got, want), U.first_diff(got, want, 20, W)


def test_the_world_grid_is_rebuilt_once(R):
    rng = np.random.default_rng(17)
    removed = _sets(R)["run"]
    with R.Context(W, H) as c:
        b = _aged_base(R, c)
        p = b["p"]
        objs = _snapshot(c)
        centres = np.array([v[0:3] for kind, v, _ in objs if kind == 2], dtype=np.float32)
        target = centres[rng.integers(0, len(centres), 512)]
        origin = np.tile(np.array(p.cam_pos[:], dtype=np.float32), (512, 1))
        rays = R.make_rays(origin, target - origin)
        c.query_rays(rays)
        builds = c.get_option(R.STAT_QUERY_GRID_BUILDS)
        c.query_rays(rays)
        assert c.get_option(R.STAT_QUERY_GRID_BUILDS) == builds
        with _fresh(R, _survivors(objs, removed)) as F:
            _remove(c, "host", removed)
            assert c.get_option(R.STAT_QUERY_GRID_BUILDS) == builds
            got = c.query_rays(rays)
            assert c.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
            assert np.array_equal(got.view(np.uint8), F.query_rays(rays).view(np.uint8))
            c.query_rays(rays)
            assert c.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1


def test_recorded_graphs_before_and_after(R):
    import torch
    removed = _sets(R)["second"]
    with R.Context(W, H) as c:
        c.set_option(R.OPT_TWO_LEVEL, 0)       # (a binning pre-pass cannot be recorded)
        b = _aged_base(R, c)
        p = b["p"]
        objs = _snapshot(c)
        st = torch.cuda.Stream()
        buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")

        def record():
            c.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=st.cuda_stream)   # uploads, sorts
            torch.cuda.synchronize()
            c.graph_begin(st.cuda_stream)
            c.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=st.cuda_stream)
            return c.graph_end(st.cuda_stream)

        def replay(g):
            buf.fill_(0xEE)
            torch.cuda.synchronize()
            c.graph_launch(g, st.cuda_stream)
            torch.cuda.synchronize()
            return buf.cpu().numpy()

        g0 = record()
        g1 = None
        try:
            assert np.array_equal(replay(g0), b["before"])
            with _fresh(R, _survivors(objs, removed)) as F:
                F.set_option(R.OPT_TWO_LEVEL, 0)
                _remove(c, "host", removed)
                with pytest.raises(R.RtxError) as e:
                    c.graph_launch(g0, st.cuda_stream)
                assert e.value.status == R.ERR_INVALID_ARGUMENT and "re-capture" in str(e.value)
                g1 = record()
                got, want = replay(g1), TE._out(R, F, p, O.RGB_ASCII)
                assert np.array_equal(got, want), U.first_diff(got, want, 20, W)
                assert not np.array_equal(got, b["before"])
        finally:
            c.graph_destroy(g0)
            if g1 is not None:
                c.graph_destroy(g1)


# ---------------------------------------------------------------- 4. every shading path

MIRROR_SPHERE = 11          # a sphere the camera of the mirror tests sees (asserted with the oracle where it matters)


def _mirror_scene():
    """40 spheres over a floor created in their middle (object 20); spheres are objects 0 .. 19 and 21 .. 40."""
    ns = 40
    rng = np.random.default_rng(11)
    sph = np.concatenate([rng.uniform(-14, 14, (ns, 1)), rng.uniform(1, 8, (ns, 1)), rng.uniform(20, 46, (ns, 1)),
                          rng.uniform(1.0, 2.5, (ns, 1)), np.floor(rng.uniform(30, 256, (ns, 3)))], axis=1).astype(np.float32)
    floor = np.array([0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80], dtype=np.float32)
    return sph, floor


def _mirror_context(R, w, h, sph, floor):
    c = R.Context(w, h)
    c.add_spheres(sph[:20])
    c.add_plane(floor[0:3], floor[3:6], floor[6:9], float(floor[9]), float(floor[10]))
    c.add_spheres(sph[20:])
    return c


def test_every_shading_path_reads_the_removal(R):
    w, h = 64, 32
    op = O.camera_params(w, h, pos=(0.0, 12.0, 0.0), rot=(0.3, RS.PI32, 0.0))
    pp = TC._params(op)
    sph, floor = _mirror_scene()
    lights = RS.light_set(2, positions=RS.SHADOW_POSITIONS["mirror_floor_shadows"][:2], scale=0.6)
    removed = [38, 3, 9, 10, 21, 30]           # around the mirrors: the floor (20 -> 17) and sphere 11 (-> 8) stay
    states = (("two lights, shadows", dict(shadows=1, depth=1, refl_shadows=0, grid=0)),
              ("mirrors two deep, shadows in them", dict(shadows=1, depth=2, refl_shadows=1, grid=0)),
              ("the same through the world grid", dict(shadows=1, depth=2, refl_shadows=1, grid=1)),
              ("the grid without mirrors in the shadows", dict(shadows=1, depth=1, refl_shadows=0, grid=1)))

    def state(x, s):
        x.set_option(R.OPT_SHADOWS, s["shadows"])
        x.set_option(R.OPT_REFLECT_DEPTH, s["depth"])
        x.set_option(R.OPT_REFLECT_SHADOWS, s["refl_shadows"])
        x.set_option(R.OPT_SHADOW_GRID, s["grid"])

    with _mirror_context(R, w, h, sph, floor) as c:
        c.set_reflectivity(20, 0.6)
        c.set_reflectivity(MIRROR_SPHERE, 0.5)
        TC._set_lights(R, c, lights)
        state(c, states[2][1])
        before = TE._out(R, c, pp, O.RGB_ASCII)          # every cache of the path exists
        frames0 = c.get_option(R.STAT_REFLECT_FRAMES)
        assert frames0 > 0
        objs = _snapshot(c)
        with _fresh(R, _survivors(objs, removed), w, h) as F:
            TC._set_lights(R, F, lights)
            _remove(c, "host", removed)
            assert [l.pos[:] for l in c.get_lights()] == [l.pos[:] for l in F.get_lights()] and len(c.get_lights()) == 2
            assert c.get_reflectivity(17) == f32(0.6) and c.get_reflectivity(8) == f32(0.5)
            assert sum(c.get_reflectivity(i) > 0 for i in range(c.object_count)) == 2
            for what, s in states:
                for x in (c, F):
                    state(x, s)
                for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, 0), (O.RGB_ASCII, R.RENDER_VALUES)):
                    got, want = TE._out(R, c, pp, mode, flags), TE._out(R, F, pp, mode, flags)
                    assert np.array_equal(got, want), (what, mode, flags)
                if s["grid"]:
                    assert c.get_option(R.STAT_SHADOW_GRID_FRAMES) > 0
                    assert s["depth"] == 1 or c.last_kernel.startswith("rtx_grid_"), c.last_kernel
            for x in (c, F):
                state(x, states[2][1])
            assert not np.array_equal(TE._out(R, c, pp, O.RGB_ASCII), before)
            assert c.get_option(R.STAT_REFLECT_FRAMES) > frames0


def test_removing_the_only_mirror_leaves_the_mirror_path(R):
    w, h = 64, 32
    op = O.camera_params(w, h, pos=(0.0, 12.0, 0.0), rot=(0.3, RS.PI32, 0.0))
    pp = TC._params(op)
    sph, floor = _mirror_scene()
    full = O.render(op, O.Scene.from_arrays(sph, floor.reshape(1, 11)), O.RGB_ASCII)
    for mirror in (20, MIRROR_SPHERE):          # the floor, a sphere
        with _mirror_context(R, w, h, sph, floor) as c:
            c.set_reflectivity(mirror, 0.5)
            with_mirror = TE._out(R, c, pp, O.RGB_ASCII)
            f0 = c.get_option(R.STAT_REFLECT_FRAMES)
            assert f0 >= 1
            objs = _snapshot(c)
            with _fresh(R, _survivors(objs, [mirror]), w, h) as F:
                _remove(c, "host", [mirror])
                for mode in (O.RGB_ASCII, O.BIT_PIXEL):
                    got, want = TE._out(R, c, pp, mode), TE._out(R, F, pp, mode)
                    assert np.array_equal(got, want), (mirror, mode)
                assert c.get_option(R.STAT_REFLECT_FRAMES) == f0 and F.get_option(R.STAT_REFLECT_FRAMES) == 0
                assert not np.array_equal(TE._out(R, c, pp, O.RGB_ASCII), with_mirror)
                keep = [i for i in range(40) if _gidx_mirror(i) != mirror]
                pl = floor.reshape(1, 11) if mirror != 20 else np.zeros((0, 11), dtype=np.float32)
                # (no mirror is left: the oracle, which knows none, has a say again; creation order does not matter without ties)
                want = O.render(op, O.Scene.from_arrays(sph[keep], pl), O.RGB_ASCII)
                assert not np.array_equal(want, full), "the frame does not show the mirror: change the scene"
                got = TE._out(R, c, pp, O.RGB_ASCII)
                assert np.array_equal(got, want), (mirror, U.first_diff(got, want, 20, w))


def _gidx_mirror(k):
    """creation index of sphere local k in _mirror_context's scene"""
    return k if k < 20 else k + 1


# ---------------------------------------------------------------- 5. physics after a removal

@pytest.mark.parametrize("words", [1, 0])
def test_physics_and_update_after_a_removal(R, words):
    removed = _sets(R)["second"]
    with R.Context(W, H) as c:
        b = _aged_base(R, c)
        p = b["p"]
        objs = _snapshot(c)
        sc = _oracle_without(b["sc"], removed)
        with _fresh(R, _survivors(objs, removed)) as F:
            for x in (c, F):
                x.set_option(R.OPT_UPDATE_WORDS, words)
            first = c.update(p, O.RGB_ASCII).copy()
            _remove(c, "host", removed)
            for mode in (O.RGB_ASCII, O.BIT_ASCII):
                got, want = c.update(p, mode).copy(), F.update(p, mode).copy()
                assert got.size == want.size and np.array_equal(got, want), (mode, got.size, want.size)
                assert np.array_equal(want, O.minimize(mode, O.render(b["op"], sc, mode), W, H)), mode
            assert not np.array_equal(first, c.update(p, O.RGB_ASCII))
            for k, dt in enumerate(STEPS):
                for x in (c, F):
                    x.update_objects(dt)
                _oracle_step(sc, dt)
                got, want = TE._out(R, c, p, O.RGB_ASCII), TE._out(R, F, p, O.RGB_ASCII)
                assert np.array_equal(got, want), (k, U.first_diff(got, want, 20, W))
                want = O.render(b["op"], sc, O.RGB_ASCII)
                assert np.array_equal(got, want), (k, U.first_diff(got, want, 20, W))
            _assert_objects(c, F)
            got, want = c.update(p, O.RGB_ASCII).copy(), F.update(p, O.RGB_ASCII).copy()
            assert got.size == want.size and np.array_equal(got, want)
            # sphere 40 (mover 3, speed 2.5) survived as object 20 and still moves by its own motion
            assert tuple(c.get_object(20)[1][7:9]) == (3.0, 2.5) or tuple(c.get_object(20)[1][7:9]) == (-3.0, 2.5)


# ---------------------------------------------------------------- 6. errors are all or nothing

def test_errors_are_all_or_nothing(R):
    import torch
    with R.Context(W, H) as c:
        b = _aged_base(R, c)
        p = b["p"]
        base = TE._out(R, c, p, O.RGB_ASCII)
        n0 = c.get_option(R.STAT_SCENE_REMOVED)
        L = R.lib()

        def call(indices):
            v = (C.c_uint * len(indices))(*indices)
            return L.rtx_scene_remove_objects(c._h, len(indices), v)

        def unchanged():
            assert c.object_count == COUNT and c.get_option(R.STAT_SCENE_REMOVED) == n0
            assert np.array_equal(TE._out(R, c, p, O.RGB_ASCII), base)

        for indices, named, why in (([COUNT], str(COUNT), "past"), ([3, 7, COUNT, 7], str(COUNT), "past"), ([5, 9, 200, 9, 400], "9", "twice"),
                                    ([0, 0], "0", "twice"), ([0xFFFFFFFF], str(0xFFFFFFFF), "past"), ([301, 100, 301], "301", "twice")):
            assert call(indices) == R.ERR_INVALID_ARGUMENT, indices
            text = (L.rtx_last_error(c._h) or b"").decode()
            assert ("index " + named + " ") in text and why in text, text
        assert L.rtx_scene_remove_objects(c._h, 3, None) == R.ERR_INVALID_ARGUMENT
        assert L.rtx_scene_remove_marked_device(c._h, None, None, None) == R.ERR_INVALID_ARGUMENT
        with pytest.raises(R.RtxError):
            c.remove_objects([1, 2, 1])
        unchanged()
        # n == 0 and marks that are all zero: fine, nothing happens
        assert L.rtx_scene_remove_objects(c._h, 0, None) == R.OK
        c.remove_objects([])
        zeros = torch.zeros(COUNT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = C.c_size_t(99)
        assert L.rtx_scene_remove_marked_device(c._h, zeros.data_ptr(), None, C.byref(n)) == R.OK and n.value == 0
        assert c.remove_marked_device(zeros.data_ptr()) == 0
        unchanged()
        # inside a capture the call would have to wait: refused, on the context's stream and on the stream given
        ones = torch.ones(COUNT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.graph_begin()
        try:
            for bad in (lambda: c.remove_objects([0]), lambda: c.remove_marked_device(ones.data_ptr())):
                with pytest.raises(R.RtxError) as e:
                    bad()
                assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
        finally:
            try:
                c.graph_destroy(c.graph_end())
            except R.RtxError:
                pass
        st = torch.cuda.Stream()
        c.graph_begin(st.cuda_stream)
        try:
            with pytest.raises(R.RtxError) as e:
                c.remove_marked_device(ones.data_ptr(), stream=st.cuda_stream)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
        finally:
            try:
                c.graph_destroy(c.graph_end(st.cuda_stream))
            except R.RtxError:
                pass
        unchanged()
    # an empty scene has no index, and no marks to read
    with R.Context(W, H) as c:
        v = (C.c_uint * 1)(0)
        assert R.lib().rtx_scene_remove_objects(c._h, 1, v) == R.ERR_INVALID_ARGUMENT
        n = C.c_size_t(99)
        assert R.lib().rtx_scene_remove_marked_device(c._h, None, None, C.byref(n)) == R.OK and n.value == 0


# ---------------------------------------------------------------- 7. the device form

@pytest.mark.parametrize("name", ["second", "run", "everything"])
def test_device_form_equals_host_form(R, name):
    removed = _sets(R)[name]
    with R.Context(W, H) as c, R.Context(W, H) as host:
        b = _aged_base(R, c)
        _aged_base(R, host)
        p = b["p"]
        TE._out(R, c, p, O.RGB_ASCII)
        objs = _snapshot(c)
        with _fresh(R, _survivors(objs, removed)) as F:
            assert _remove(c, "device", removed) == len(removed)
            _remove(host, "host", removed)
            assert c.object_count == COUNT - len(removed)
            assert c.get_option(R.STAT_SCENE_REMOVED) == len(removed) == host.get_option(R.STAT_SCENE_REMOVED)
            _assert_frames(R, c, F, p, name, kernels=(R.KERNEL_AUTO,))
            _assert_frames(R, c, host, p, name, kernels=(R.KERNEL_AUTO,))
            _assert_objects(c, F)
            _assert_objects(c, host)


# ---------------------------------------------------------------- 8. a device group

def test_device_group(R):
    Hg = 41
    p = R.camera_params(W, Hg)
    with R.Context(W, Hg, devices=[0, 0, 0]) as g:
        assert [g.group_rows(Hg, r)[1] for r in range(3)] == [13, 14, 14]      # ragged slabs
        _aged_base(R, g)
        g.render_to_host(p, O.RGB_ASCII)
        objs = _snapshot(g)
        total = 0
        for form, removed in (("host", _sets(R)["run"] + [PLANE_A]), ("device", list(range(1, 200, 2)))):
            objs_after = _survivors(objs, removed)
            with _fresh(R, objs_after, W, Hg) as F:
                assert _remove(g, form, removed) == len(removed)
                total += len(removed)
                assert g.object_count == len(objs_after)
                for mode in (O.RGB_ASCII, O.BIT_PIXEL):
                    got, want = g.render_to_host(p, mode), F.render_to_host(p, mode)
                    assert np.array_equal(got, want), (form, mode, U.first_diff(got, want, 20 if mode >= 2 else 12, W))
                assert [g.member_option(r, R.STAT_SCENE_REMOVED) for r in range(3)] == [total] * 3
            objs = objs_after
        # a bad set changes no rank
        before = g.render_to_host(p, O.RGB_ASCII)
        for bad in ([0, g.object_count], [4, 4]):
            with pytest.raises(R.RtxError) as e:
                g.remove_objects(bad)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
        assert [g.member_option(r, R.STAT_SCENE_REMOVED) for r in range(3)] == [total] * 3
        assert np.array_equal(g.render_to_host(p, O.RGB_ASCII), before)
        # physics afterwards: every member steps the replica it compacted
        with _fresh(R, objs, W, Hg) as F:
            for x in (g, F):
                x.update_objects(0.05)
            got, want = g.render_to_host(p, O.RGB_ASCII), F.render_to_host(p, O.RGB_ASCII)
            assert np.array_equal(got, want), U.first_diff(got, want, 20, W)

# ---------------------------------------------------------------- 9. interleaving

def test_add_remove_add_edit_remove(R):
    """No physics here, so the host knows every value: F and the oracle's scene are built from a plain list that the same
    operations are applied to."""
    b = _base_case(R)
    p, op, sph, pl = b["p"], b["op"], b["sph"], b["pl"]
    rng = np.random.default_rng(23)
    world = []                                  # rows of 7 (spheres) or 11 (planes), in creation order

    def add(c, rows):
        for row in rows:
            world.append(np.array(row, dtype=np.float32))
            if len(row) == 7:
                c.add_sphere(float(row[3]), row[0:3], row[4:7])
            else:
                c.add_plane(row[0:3], row[3:6], row[6:9], float(row[9]), float(row[10]))

    def remove(c, indices):
        c.remove_objects(indices)
        for i in sorted(indices, reverse=True):
            del world[i]

    def check(c, what):
        assert c.object_count == len(world)
        s = O.Scene()
        with R.Context(W, H) as F:
            for row in world:
                if row.size == 7:
                    F.add_sphere(float(row[3]), row[0:3], row[4:7])
                    s.add_sphere(row[3], row[0:3], row[4:7])
                else:
                    F.add_plane(row[0:3], row[3:6], row[6:9], float(row[9]), float(row[10]))
                    s.add_plane(row[0:3], row[3:6], row[6:9], row[9], row[10])
            _assert_frames(R, c, F, p, what)
            _assert_objects(c, F)
        want = O.render(op, s, O.RGB_ASCII)
        got = TE._out(R, c, p, O.RGB_ASCII)
        assert np.array_equal(got, want), (what, U.first_diff(got, want, 20, W))

    with R.Context(W, H) as c:
        add(c, list(sph[:120]) + [pl[0]] + list(sph[120:280]))
        TE._out(R, c, p, O.RGB_ASCII)
        remove(c, [5, 119, 120, 121, 279, 0] + list(range(30, 90, 3)))             # 120 is the plane
        check(c, "add, remove")
        add(c, [pl[1]] + list(sph[280:300]) + [pl[0]])                             # (appends pending on the host at the next removal)
        remove(c, [len(world) - 1, 7])
        check(c, "add, remove, add, remove")
        add(c, list(sph[0:3]))
        # an edit of a run of spheres by their NEW indices: what was spheres 130 .. 139 at creation
        first = _new_index([5, 119, 120, 121, 279, 0] + list(range(30, 90, 3)), 131)
        first = _new_index([7], first)
        assert all(world[first + j].size == 7 for j in range(10)) and np.array_equal(world[first], sph[130])
        rows = TE._moved(rng, np.array(world[first:first + 10]), 3.0)
        c.set_spheres(first, rows)
        for j in range(10):
            world[first + j] = rows[j]
        check(c, "edit on renumbered indices")
        remove(c, list(range(first + 2, first + 6)) + [len(world) - 1, 1])
        check(c, "the last removal")
        assert c.get_option(R.STAT_SCENE_REMOVED) == 26 + 2 + 6
