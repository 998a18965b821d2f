"""Scene objects edited in place -- rtx_scene_set_spheres, rtx_scene_set_spheres_device, rtx_scene_set_plane -- against a context
built afresh from the edited values (F) and, where it has a say, the CPU oracle; never against the kernel under test itself:
   1. an edited context renders F's bytes in every mode and output form, host and device form, with and without the sorted copy;
   2. ranges (n = 0, single spheres, 256, 257) and errors (a plane in the range, past the count, inside a capture): all or nothing;
   3. spheres edited onto one another keep the creation-order tie-break;
   4. an animation by edits under two-level culling: the cell lists are reused as under physics steps of that size, and
      RTX_STAT_SCENE_EDIT_MOVE is the true largest displacement, rounded up;
   5. lights, shadows, mirrors, shadows in mirrors and the world grid read the edit (tests/restate.py pins the path the others
      are compared on);
   6. ray queries and rtx_pick;  7. physics steps and edits interleaved, against the oracle;  8. a recorded graph replays the
   edited scene;  9. a device group;  10. rtx_update."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_shadows as RH
import util as U
import test_gpu_chain_lights as TC
import test_gpu_reflect as T

pytestmark = pytest.mark.gpu

f32 = np.float32
FORMS = ["host", "device"]
NO_PLANES = np.zeros((0, 11), dtype=np.float32)


@pytest.fixture(scope="module")
def R():
    return U.pkg()


def _out(R, c, p, mode, flags=0, stream=None):
    """One frame through render_rows into a 0xEE-filled caller buffer (tests/test_gpu_reuse.py::_frame), as numpy bytes."""
    import torch
    W, H = int(p.x), int(p.y)
    S = 32 if flags & R.RENDER_VALUES else (4 if flags & R.RENDER_COMPACT else 20)
    buf = torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if flags == 0 and mode < O.RGB_ASCII:
        flags = R.RENDER_ZERO_TAIL
    c.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream, flags=flags)
    c.synchronize()
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _edit(c, form, first, rows):
    """rows -> spheres first ..., through the host form or the device form; the device form's rows are written by a torch kernel
    on a stream of its own, behind a busy-wait, so that only the ordering the call promises makes them arrive."""
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 7)
    if form == "host":
        c.set_spheres(first, rows)
        return
    import torch
    src = torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda._sleep(2000000)
        d = src * 1.0
    c.set_spheres_device(first, rows.shape[0], d.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()


def _moved(rng, old, shift, radii=True, colours=True):
    """New rows for `old`: centres shifted by up to +-shift per axis, new radii on every second row, new colours."""
    new = old.copy()
    new[:, 0:3] += rng.uniform(-shift, shift, (len(old), 3)).astype(np.float32)
    if radii:
        new[::2, 3] *= rng.uniform(0.6, 1.5, len(new[::2])).astype(np.float32)
    if colours:
        new[:, 4:7] = np.floor(rng.uniform(1, 256, (len(old), 3))).astype(np.float32)
    return new.astype(np.float32)


def _stat_move(R, c):
    return np.array([c.get_option(R.STAT_SCENE_EDIT_MOVE)], dtype=np.uint32).view(np.float32)[0]


def _cell_stats(R, c):
    return {k: c.get_option(v) for k, v in (("builds", R.STAT_CELL_BUILDS), ("prefetches", R.STAT_CELL_PREFETCHES),
                                            ("hits", R.STAT_CELL_HITS), ("per_frame", R.STAT_CELL_PER_FRAME))}


# ---------------------------------------------------------------- 1. edited equals rebuilt

@pytest.mark.parametrize("sorted_store", [-1, 0])
@pytest.mark.parametrize("form", FORMS)
def test_edited_equals_rebuilt(R, form, sorted_store):
    W, H = 96, 40
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(41, 300, 2, p.element1, p.element2)   # (300 >= 256: the direction-sorted copy is live)
    rng = np.random.default_rng(7)
    new = sph.copy()
    new[37:237] = _moved(rng, sph[37:237], 3.0)
    with R.Context(W, H) as c, R.Context(W, H) as F:
        for x in (c, F):
            x.set_option(R.OPT_SORTED_STORE, sorted_store)
        c.set_scene(sph, pl)
        F.set_scene(new, pl)
        for x in (c, F):
            x.set_sphere_motion(40, 3, 2.5)
        before = _out(R, c, p, O.RGB_ASCII)      # (the sorted copy exists from here on)
        n0 = c.get_option(R.STAT_SCENE_EDITS)
        _edit(c, form, 37, new[37:237])
        assert c.get_option(R.STAT_SCENE_EDITS) == n0 + 1
        for mode in (O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS):
            got, want = _out(R, c, p, mode), _out(R, F, p, mode)
            assert np.array_equal(got, want), (O.MODE_NAMES[mode], U.first_diff(got, want, 20 if mode >= 2 else 12, W))
        for flags in (R.RENDER_VALUES, R.RENDER_COMPACT):
            assert np.array_equal(_out(R, c, p, O.RGB_ASCII, flags), _out(R, F, p, O.RGB_ASCII, flags)), flags
        got = _out(R, c, p, O.RGB_ASCII)
        assert not np.array_equal(got, before)
        want = O.render(U.oracle_params(p), O.Scene.from_arrays(new, pl), O.RGB_ASCII)
        assert np.array_equal(got, want), U.first_diff(got, want, 20, W)
        for i in (36, 37, 40, 236, 237):
            kind, o = c.get_object(i)
            assert kind == 2 and np.array_equal(o[:7].view(np.uint32), new[i].view(np.uint32)), i
            assert (o[7], o[8]) == ((3.0, 2.5) if i == 40 else (-1.0, 1.0)), i
        assert np.array_equal(c.get_object(300)[1], F.get_object(300)[1])


# ---------------------------------------------------------------- 2. ranges and errors

def _built(R, W, H, a, plane, b):
    c = R.Context(W, H)
    c.add_spheres(a)
    c.add_plane(plane[0:3], plane[3:6], plane[6:9], float(plane[9]), float(plane[10]))
    c.add_spheres(b)
    return c


def test_ranges_and_errors(R):
    import torch
    W, H = 96, 40
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(43, 600, 1, p.element1, p.element2)
    a, b, plane = sph[:300].copy(), sph[300:].copy(), pl[0]
    rng = np.random.default_rng(9)
    c = _built(R, W, H, a, plane, b)       # creation indices: spheres 0 .. 299, plane 300, spheres 301 .. 600
    try:
        base = _out(R, c, p, O.RGB_ASCII)
        n0 = c.get_option(R.STAT_SCENE_EDITS)
        # n == 0: fine, nothing changes (an empty range anywhere up to the count, rows or no rows)
        c.set_spheres(5, np.zeros((0, 7), dtype=np.float32))
        assert R.lib().rtx_scene_set_spheres(c._h, 300, 0, None) == R.OK
        assert R.lib().rtx_scene_set_spheres_device(c._h, 601, 0, None, None) == R.OK
        assert c.get_option(R.STAT_SCENE_EDITS) == n0 and np.array_equal(_out(R, c, p, O.RGB_ASCII), base)
        # single spheres at both ends, a full block, a block and a tail of one (local indices 300 .. 556, across the plane's index)
        for k, (form, first, n) in enumerate((("host", 0, 1), ("device", 600, 1), ("device", 0, 256), ("host", 301, 257))):
            part, lo = (a, first) if first < 300 else (b, first - 301)
            part[lo:lo + n] = _moved(rng, part[lo:lo + n], 2.0)
            _edit(c, form, first, part[lo:lo + n])
            assert c.get_option(R.STAT_SCENE_EDITS) == n0 + k + 1
            F = _built(R, W, H, a, plane, b)
            try:
                got, want = _out(R, c, p, O.RGB_ASCII), _out(R, F, p, O.RGB_ASCII)
                assert np.array_equal(got, want), (form, first, n, U.first_diff(got, want, 20, W))
            finally:
                F.close()
        base = _out(R, c, p, O.RGB_ASCII)
        n1 = c.get_option(R.STAT_SCENE_EDITS)
        rows = _moved(rng, sph[:5], 5.0)
        d_rows = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        # a plane in the range, a range past the count, a start past the count: refused, named, nothing changes
        for first, n, names in ((298, 5, "300"), (300, 1, "300"), (599, 3, None), (602, 1, None), (0, 1 << 40, None)):
            for call in (lambda: R.lib().rtx_scene_set_spheres(c._h, first, n, rows.ctypes.data),
                         lambda: R.lib().rtx_scene_set_spheres_device(c._h, first, n, d_rows.data_ptr(), None)):
                assert call() == R.ERR_INVALID_ARGUMENT, (first, n)
                text = (R.lib().rtx_last_error(c._h) or b"").decode()
                assert (names in text and "not a sphere" in text) if names else "rtx_scene_count" in text, text
        assert R.lib().rtx_scene_set_spheres(c._h, 0, 1, None) == R.ERR_INVALID_ARGUMENT
        for bad in (0, 299, 301, 601, 1 << 31):
            with pytest.raises(R.RtxError) as e:
                c.set_plane(bad, (0, 0, 0), (0, 1, 0), (1, 2, 3), 1.0, 1.0)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
        assert c.get_option(R.STAT_SCENE_EDITS) == n1 and np.array_equal(_out(R, c, p, O.RGB_ASCII), base)
        # inside a capture the call would have to wait: refused, on the context's stream and on the stream given
        c.graph_begin()
        try:
            for call in (lambda: c.set_spheres(0, rows), lambda: c.set_spheres_device(0, 5, d_rows.data_ptr()),
                         lambda: c.set_plane(300, (0, 0, 0), (0, 1, 0), (1, 2, 3), 1.0, 1.0)):
                with pytest.raises(R.RtxError) as e:
                    call()
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
                c.set_spheres_device(0, 5, d_rows.data_ptr(), stream=st.cuda_stream)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
        finally:
            try:
                c.graph_destroy(c.graph_end(st.cuda_stream))
            except R.RtxError:
                pass
        assert c.get_option(R.STAT_SCENE_EDITS) == n1 and np.array_equal(_out(R, c, p, O.RGB_ASCII), base)
    finally:
        c.close()


# ---------------------------------------------------------------- 3. the tie-break

@pytest.mark.parametrize("form", FORMS)
def test_tie_break_survives(R, form):
    """Spheres edited to the centre and radius of others, in another colour: every hit of such a pair is an exact tie, which the
    FIRST created wins (RayTracing.cu:123) -- twins created after their originals and before them, as in
    tests/test_gpu_reuse.py::test_exact_ties_are_broken_by_creation_order_with_sorted_arrays."""
    W, H = 96, 40
    p = R.camera_params(W, H)
    sph, _ = R.synth_scene(31, 300, 0, p.element1, p.element2)
    rng = np.random.default_rng(23)
    new = sph.copy()
    new[100:130, 0:4] = sph[10:40, 0:4]      # twins created after their originals
    new[0:10, 0:4] = sph[250:260, 0:4]       # ... and before
    new[100:130, 4:7] = np.floor(rng.uniform(1, 256, (30, 3)))
    new[0:10, 4:7] = np.floor(rng.uniform(1, 256, (10, 3)))
    want = O.render(U.oracle_params(p), O.Scene.from_arrays(new, NO_PLANES), O.RGB_ASCII)
    with R.Context(W, H) as c, R.Context(W, H) as F:
        c.set_scene(sph, NO_PLANES)
        F.set_scene(new, NO_PLANES)
        _out(R, c, p, O.RGB_ASCII)
        _edit(c, form, 100, new[100:130])
        _edit(c, form, 0, new[0:10])
        for kernel in (R.KERNEL_AUTO, R.KERNEL_BRUTE):
            for x in (c, F):
                x.set_option(R.OPT_KERNEL, kernel)
            got = _out(R, c, p, O.RGB_ASCII)
            assert np.array_equal(got, _out(R, F, p, O.RGB_ASCII)), kernel
            assert np.array_equal(got, want), (kernel, U.first_diff(got, want, 20, W))


# ---------------------------------------------------------------- 4. cell lists under an animation

def test_cell_lists_under_an_animation_by_edits(R):
    """tests/test_gpu_reuse.py::test_cell_lists_with_bouncing_spheres with edits in place of physics steps: every sphere moves by its
    own vector of length <= 0.1 per frame, in x, y and z.  That test holds physics steps of up to 0.132 per frame to
    hits >= 25 and per_frame == 0 under the same policy; an edit's drift is the true maximum, never more than that bound."""
    import torch
    W, H, n = 320, 180, 2600
    rng = np.random.default_rng(3)
    cur = np.concatenate([rng.uniform(-60, 60, (n, 1)), rng.uniform(-25, 25, (n, 1)), rng.uniform(30, 160, (n, 1)),
                          rng.uniform(0.3, 2.0, (n, 1)), np.floor(rng.uniform(1, 256, (n, 3)))], axis=1).astype(np.float32)
    a, b = R.Context(W, H), R.Context(W, H)
    try:
        for c in (a, b):
            c.set_scene(cur, NO_PLANES)
        b.set_option(R.OPT_KERNEL, R.KERNEL_BRUTE)
        got = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
        want = torch.empty_like(got)
        p = R.camera_params(W, H)

        def frames(what):
            for c, buf in ((a, got), (b, want)):
                buf.fill_(0xEE)
                torch.cuda.synchronize()
                c.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0)
            torch.cuda.synchronize()
            assert torch.equal(got, want), what

        for f in range(40):
            v = rng.normal(size=(n, 3))
            v *= (rng.uniform(0.0, 0.1, (n, 1)) / np.linalg.norm(v, axis=1, keepdims=True))
            new = cur.copy()
            new[:, 0:3] = (cur[:, 0:3].astype(np.float64) + v).astype(np.float32)
            t = float(np.sqrt(((new[:, 0:3].astype(np.float64) - cur[:, 0:3].astype(np.float64)) ** 2).sum(axis=1)).max())
            _edit(a, FORMS[f % 2], 0, new)
            _edit(b, "host", 0, new)
            cur = new
            for c in (a, b):
                moved = float(_stat_move(R, c))
                print("frame %d: largest displacement %.9g, RTX_STAT_SCENE_EDIT_MOVE %.9g" % (f, t, moved))
                assert t <= moved <= t * (1.0 + 2.0 ** -20), (f, t, moved)
            frames("frame %d" % f)
        s = _cell_stats(R, a)
        print("cell lists over 40 edited frames:", s)
        assert s["hits"] >= 25 and s["per_frame"] == 0, s
        assert np.array_equal(got.cpu().numpy(), O.render(U.oracle_params(p), O.Scene.from_arrays(cur, NO_PLANES), O.RGB_ASCII, threads=8))
        # a radius is not motion: the lists start over
        cur[1234, 3] *= f32(1.5)
        for c in (a, b):
            _edit(c, "host", 1234, cur[1234:1235])
            assert c.get_option(R.STAT_SCENE_EDIT_MOVE) == 0x7f800000
        frames("after a radius edit")
        s1 = _cell_stats(R, a)
        assert s1["builds"] + s1["per_frame"] == s["builds"] + s["per_frame"] + 1 and s1["hits"] == s["hits"], (s, s1)
        # a colour is nothing to the lists
        cur[100:400, 4:7] = np.floor(rng.uniform(1, 256, (300, 3)))
        for c in (a, b):
            _edit(c, "device", 100, cur[100:400])
            assert c.get_option(R.STAT_SCENE_EDIT_MOVE) == 0
        frames("after a colour edit")
        s2 = _cell_stats(R, a)
        assert s2["hits"] == s1["hits"] + 1 and s2["builds"] == s1["builds"] and s2["per_frame"] == s1["per_frame"], (s1, s2)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 5. every shading path

def test_every_shading_path_reads_the_edit(R):
    """Three lights, shadows, mirrors three levels deep with shadows in them, then the same through the world grid.  The path
    without the grid is pinned first by tests/restate.py: geometry (t, shadingValue, normal) bit for bit at every visible pixel,
    and the colour bit for bit wherever float64 decides every (level, light) shadow test (restate_shadows.level_sets; a pixel
    within its tolerance band of a silhouette has no independent answer).  Everything else is then compared with F, bytewise."""
    W, H, ns = 64, 32, 40
    op = O.camera_params(W, H, pos=(0.0, 12.0, 0.0), rot=(0.3, RS.PI32, 0.0))
    pp = TC._params(op)
    rng = np.random.default_rng(11)
    sph = np.concatenate([rng.uniform(-14, 14, (ns, 1)), rng.uniform(1, 8, (ns, 1)), rng.uniform(20, 46, (ns, 1)),
                          rng.uniform(1.0, 2.5, (ns, 1)), np.floor(rng.uniform(30, 256, (ns, 3)))], axis=1).astype(np.float32)
    pl = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80]], dtype=np.float32)
    ks = {i: 0.5 for i in range(3, 13)}
    ks[ns] = 0.6
    lights = RS.light_set(3, positions=RS.SHADOW_POSITIONS["mirror_floor_shadows"], scale=0.6)
    new = sph.copy()
    new[5:20] = _moved(rng, sph[5:20], 2.0)
    new[5:20, 1] = np.maximum(new[5:20, 1], f32(1.0))
    new_pl = np.array([[0, -2.5, 30, 0, 2, 0, 90, 140, 100, 80, 80]], dtype=np.float32)   # lowered, recoloured; the normal is normalised

    def state(x, grid):
        x.set_option(R.OPT_SHADOWS, 1)
        x.set_option(R.OPT_REFLECT_DEPTH, 3)
        x.set_option(R.OPT_REFLECT_SHADOWS, 1)
        x.set_option(R.OPT_SHADOW_GRID, grid)

    with R.Context(W, H) as c, R.Context(W, H) as F:
        c.set_scene(sph, pl)
        F.set_scene(new, new_pl)
        for x in (c, F):
            T._set_k(x, ks)
            TC._set_lights(R, x, lights)
            state(x, 1)
        _out(R, c, pp, O.RGB_ASCII)
        builds = c.get_option(R.STAT_QUERY_GRID_BUILDS)
        n0 = c.get_option(R.STAT_SCENE_EDITS)
        _edit(c, "host", 5, new[5:20])
        q = new_pl[0]
        c.set_plane(ns, q[0:3], q[3:6], q[6:9], float(q[9]), float(q[10]))
        assert c.get_option(R.STAT_SCENE_EDITS) == n0 + 2
        assert np.array_equal(c.get_object(ns)[1].view(np.uint32), F.get_object(ns)[1].view(np.uint32))
        # the path without the grid, against the restatement of the edited scene
        state(c, 0)
        got = _out(R, c, pp, O.RGB_ASCII, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
        trace = RS.trace_chain(op, new, new_pl, ks, np.arange(W * H), max_depth=3)
        lev = RH.level_sets(trace, lights, 3)
        want = RH.shade_chain_dark(trace, lights, [l["dset"] for l in lev])[3]
        TC._assert_values(got, trace, [got[:, 5], got[:, 6], got[:, 7]], "edited scene", fields=range(5))
        decided = trace["vis"] & np.logical_and.reduce([l["decided"] for l in lev])
        same = np.logical_and.reduce([RS.same_floats(got[:, 5 + k], want[k]) for k in range(3)])
        print("restatement: %d visible pixels, %d decided by float64 at every level, %d with a level-1 ray" % (
            int(trace["vis"].sum()), int(decided.sum()), trace["rays"][0]))
        assert decided.sum() * 2 >= trace["vis"].sum() and trace["rays"][0] >= 50 and trace["rays"][1] >= 5
        bad = np.nonzero(decided & ~same)[0]
        assert bad.size == 0, "%d decided pixels differ from the restatement, e.g. pixel %d: %r want %r" % (
            bad.size, int(bad[0]), got[bad[0], 5:8], [want[k][bad[0]] for k in range(3)])
        # ... then without and with the grid against F under the same options
        for grid in (0, 1):
            for x in (c, F):
                state(x, grid)
            for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, 0), (O.RGB_ASCII, R.RENDER_VALUES)):
                a, b = _out(R, c, pp, mode, flags), _out(R, F, pp, mode, flags)
                assert np.array_equal(a, b), (grid, mode, flags)
            if grid:
                assert c.get_option(R.STAT_SHADOW_GRID_FRAMES) > 0 and c.last_kernel.startswith("rtx_grid_")
                # one rebuild for the two edits, none after it
                assert c.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
        for i in range(ns + 1):
            assert c.get_reflectivity(i) == f32(ks.get(i, 0.0)), i


# ---------------------------------------------------------------- 6. queries and pick

def test_queries_and_pick_after_an_edit(R):
    W, H = 96, 40
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(47, 300, 1, p.element1, p.element2)
    rng = np.random.default_rng(13)
    with R.Context(W, H) as c, R.Context(W, H) as F:
        c.set_scene(sph, pl)
        # a sphere of the range that is seen somewhere, found before the edit
        seen = None
        for row in range(2, H - 2, 3):
            for col in range(2, W - 2, 3):
                idx = c.pick(p, col, row)[1]
                if 50 <= idx < 150:
                    seen = (col, row, idx)
                    break
            if seen:
                break
        assert seen is not None
        col, row, idx = seen
        new = sph.copy()
        new[50:150] = _moved(rng, sph[50:150], 3.0)
        new[idx, 0] += f32(4000.0)                      # moved out of sight
        _edit(c, "device", 50, new[50:150])
        F.set_scene(new, pl)
        target = new[rng.integers(0, 300, 512), 0:3] + rng.normal(scale=1.0, size=(512, 3)).astype(np.float32)
        origin = np.array(p.cam_pos[:], dtype=np.float32) + rng.normal(scale=3.0, size=(512, 3)).astype(np.float32)
        rays = R.make_rays(origin, target - origin)
        for flags in (R.QUERY_CLOSEST, R.QUERY_ANY):
            got = c.query_rays(rays, flags)
            c.set_option(R.OPT_QUERY_CHECK, 1)
            brute = c.query_rays(rays, flags)
            c.set_option(R.OPT_QUERY_CHECK, 0)
            assert np.array_equal(got.view(np.uint8), brute.view(np.uint8)), flags
            assert np.array_equal(got.view(np.uint8), F.query_rays(rays, flags).view(np.uint8)), flags
            assert (got["index"] != R.NO_OBJECT).sum() >= 128
        assert c.pick(p, col, row)[1] != idx
        assert c.pick(p, col, row) == F.pick(p, col, row)


# ---------------------------------------------------------------- 7. physics and edits interleaved

def test_physics_and_edits_interleaved(R):
    W, H, n = 96, 40, 64
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(53, n, 1, p.element1, p.element2)
    rng = np.random.default_rng(17)
    sc = O.Scene.from_arrays(sph, pl)
    op = U.oracle_params(p)
    with R.Context(W, H) as c:
        c.set_scene(sph, pl)
        for i in range(n):
            mover, speed = (-1, 1)[i % 2], float(rng.integers(100, 400)) / 100.0
            c.set_sphere_motion(i, mover, speed)
            sc.objects()[i].mover, sc.objects()[i].speed = mover, speed

        def step(dt, what):
            c.update_objects(dt)
            O.lib().orc_update_objects(sc.ptrs(), sc.count, dt)
            got, want = _out(R, c, p, O.RGB_ASCII), O.render(op, sc, O.RGB_ASCII)
            assert np.array_equal(got, want), (what, U.first_diff(got, want, 20, W))

        for k, dt in enumerate((0.016, 0.033, 0.25)):
            step(dt, "step %d" % k)
        rows = _moved(rng, sph[10:30], 2.0)
        rows[::3, 1] = f32(14.0)        # outside [-10, 10]: the next step pulls these onto 10 from where they are
        rows[1::6, 1] = f32(-11.5)
        _edit(c, "host", 10, rows)
        for j, r in enumerate(rows):
            o = sc.objects()[10 + j]
            o.center, o.radius, o.color = O.Vec3(*map(float, r[0:3])), float(r[3]), O.Vec3(*map(float, r[4:7]))
        got, want = _out(R, c, p, O.RGB_ASCII), O.render(op, sc, O.RGB_ASCII)
        assert np.array_equal(got, want), U.first_diff(got, want, 20, W)
        for k, dt in enumerate((0.016, 0.033, 0.25)):
            step(dt, "step %d after the edit" % k)
        for j in (0, 1, 2, 3):
            kind, o = c.get_object(10 + j)
            oo = sc.objects()[10 + j]
            assert (o[1], o[7], o[8]) == (f32(oo.center.y), float(oo.mover), f32(oo.speed)), j


# ---------------------------------------------------------------- 8. a recorded graph

def test_recorded_graph_replays_the_edited_scene(R):
    import torch
    W, H = 96, 40
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(59, 40, 1, p.element1, p.element2)
    rng = np.random.default_rng(19)
    new = sph.copy()
    new[8:30] = _moved(rng, sph[8:30], 2.0)
    with R.Context(W, H) as c, R.Context(W, H) as F:
        c.set_scene(sph, pl)
        F.set_scene(new, pl)
        st = torch.cuda.Stream()
        buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
        c.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=st.cuda_stream)   # uploads the scene
        torch.cuda.synchronize()
        c.graph_begin(st.cuda_stream)
        c.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=st.cuda_stream)
        g = c.graph_end(st.cuda_stream)
        try:
            for form in FORMS:
                rows = new[8:30] if form == "host" else sph[8:30]       # there, and back again through the other form
                _edit(c, form, 8, rows)
                buf.fill_(0xEE)
                torch.cuda.synchronize()
                c.graph_launch(g, st.cuda_stream)
                torch.cuda.synchronize()
                ref = F
                if form == "device":
                    ref = R.Context(W, H)
                    ref.set_scene(sph, pl)
                want = _out(R, ref, p, O.RGB_ASCII)
                if ref is not F:
                    ref.close()
                got = buf.cpu().numpy()
                assert np.array_equal(got, want), (form, U.first_diff(got, want, 20, W))
            c.add_sphere(1.0, (0.0, 0.0, 50.0), (9.0, 9.0, 9.0))
            with pytest.raises(R.RtxError) as e:
                c.graph_launch(g, st.cuda_stream)
            assert e.value.status == R.ERR_INVALID_ARGUMENT and "re-capture" in str(e.value)
        finally:
            c.graph_destroy(g)


# ---------------------------------------------------------------- 9. a device group

def test_device_group(R):
    W, H = 96, 41
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(61, 300, 1, p.element1, p.element2)
    rng = np.random.default_rng(29)
    with R.Context(W, H, devices=[0, 0, 0]) as g, R.Context(W, H) as F:
        assert [g.group_rows(H, r)[1] for r in range(3)] == [13, 14, 14]      # ragged slabs
        g.set_scene(sph, pl)
        g.render_to_host(p, O.RGB_ASCII)
        cur = sph.copy()
        for k, form in enumerate(FORMS):
            cur[20:280] = _moved(rng, cur[20:280], 2.0)
            _edit(g, form, 20, cur[20:280])
            F.set_scene(cur, pl)
            for mode in (O.RGB_ASCII, O.BIT_PIXEL):
                got, want = g.render_to_host(p, mode), F.render_to_host(p, mode)
                assert np.array_equal(got, want), (form, mode, U.first_diff(got, want, 20 if mode >= 2 else 12, W))
            assert [g.member_option(r, R.STAT_SCENE_EDITS) for r in range(3)] == [k + 1] * 3
            assert len({g.member_option(r, R.STAT_SCENE_EDIT_MOVE) for r in range(3)}) == 1
        q = np.array([0, -20, 100, 0, 1, 0, 30, 200, 90, 400, 400], dtype=np.float32)
        g.set_plane(300, q[0:3], q[3:6], q[6:9], float(q[9]), float(q[10]))
        F.set_scene(cur, q.reshape(1, 11))
        assert np.array_equal(g.render_to_host(p, O.RGB_ASCII), F.render_to_host(p, O.RGB_ASCII))
        assert [g.member_option(r, R.STAT_SCENE_EDITS) for r in range(3)] == [3] * 3
        # a bad range changes no rank
        before = g.render_to_host(p, O.RGB_ASCII)
        with pytest.raises(R.RtxError) as e:
            g.set_spheres(298, cur[0:3])         # (the plane is object 300, the last one)
        assert e.value.status == R.ERR_INVALID_ARGUMENT and "300" in str(e.value)
        with pytest.raises(R.RtxError):
            g.set_spheres(299, cur[0:5])         # past the count
        with pytest.raises(R.RtxError):
            g.set_plane(5, q[0:3], q[3:6], q[6:9], 1.0, 1.0)
        assert [g.member_option(r, R.STAT_SCENE_EDITS) for r in range(3)] == [3] * 3
        assert np.array_equal(g.render_to_host(p, O.RGB_ASCII), before)


# ---------------------------------------------------------------- 10. rtx_update

@pytest.mark.parametrize("words", [1, 0])
def test_update_after_an_edit(R, words):
    W, H = 96, 40
    p = R.camera_params(W, H)
    sph, pl = R.synth_scene(67, 300, 1, p.element1, p.element2)
    rng = np.random.default_rng(31)
    new = sph.copy()
    new[0:300] = _moved(rng, sph, 2.0)
    with R.Context(W, H) as c, R.Context(W, H) as F:
        for x in (c, F):
            x.set_option(R.OPT_UPDATE_WORDS, words)
        c.set_scene(sph, pl)
        F.set_scene(new, pl)
        first = c.update(p, O.RGB_ASCII).copy()
        _edit(c, "host", 0, new)
        for mode in (O.RGB_ASCII, O.BIT_ASCII):
            got, want = c.update(p, mode).copy(), F.update(p, mode).copy()
            assert got.size == want.size and np.array_equal(got, want), (mode, got.size, want.size)
            assert np.array_equal(want, O.minimize(mode, O.render(U.oracle_params(p), O.Scene.from_arrays(new, pl), mode), W, H)), mode
        assert not np.array_equal(first, c.update(p, O.RGB_ASCII))
