"""The kernels against the reference's own code: what the host build of the reference's sources (oracle/ref_host/) gave for
the cases of tests/ref_cases.py -- read from the recording tests/golden/ref_cases.npz and, where oracle/_ref/ holds the
binaries, also produced live for further cases.  Modes 0 to 3 are compared with the reference's bytes directly; the oracle
is not in those assertions.  RGB_NORMALS differs by a documented platform choice (negative float to uint8_t: the host build
wraps, a GPU saturates) and goes through the oracle in three steps that leave no pixel out.

Nothing here reads the reference's directory.  Frames are at most 120 x 41, scenes at most 1024 objects.
"""
import numpy as np
import pytest

import oracle as O
import ref_cases as RC
import ref_host as RH
import util as U

pytestmark = pytest.mark.gpu

RECORDED, RECORDED_MINIMIZE, (CAM_POSES, CAM_PARAMS) = RC.load_fixture()
LIVE = RH.have_binaries()
LIVE_FUZZ_SEEDS = 40
LIVE_CHUNK = 10

# the brute kernel, and the culling kernels over tile log2 x sub-tiles x two-level x refine
PLANS = [("brute", 0, 0, 0, 0)] + [("binned", tile, sub, two, refine) for tile in (0, 2, 4) for sub in (0, 2) for two in (0, 1)
                                   for refine in (0, 1)]


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(320, 64)
    yield c
    c.close()


def set_plan(R, ctx, plan):
    kernel, tile, sub, two, refine = plan
    ctx.set_option(R.OPT_KERNEL, {"auto": R.KERNEL_AUTO, "brute": R.KERNEL_BRUTE, "binned": R.KERNEL_BINNED}[kernel])
    ctx.set_option(R.OPT_TILE_LOG2_W, tile)
    ctx.set_option(R.OPT_SUBTILES, sub)
    ctx.set_option(R.OPT_TWO_LEVEL, two)
    ctx.set_option(R.OPT_REFINE, refine)


DEFAULT_PLAN = ("auto", 0, 0, -1, -1)
KERNELS_SEEN = {}       # plan -> names of the kernels check_render's frames came from


def load_scene(ctx, c):
    """The case's objects in their creation order, spheres and planes interleaved, with each sphere's mover and speed."""
    ctx.scene_clear()
    for i, o in enumerate(c["objs"]):
        if o["type"] == O.SPHERE:
            assert ctx.add_sphere(float(o["radius"]), [float(v) for v in o["center"]], [float(v) for v in o["color"]]) == i
            ctx.set_sphere_motion(i, int(o["mover"]), float(o["speed"]))
        else:
            assert ctx.add_plane([float(v) for v in o["center"]], [float(v) for v in o["normal"]], [float(v) for v in o["color"]],
                                 float(o["width"]), float(o["height"])) == i


def product_params(c):
    v = c["params"]
    return U.product_params(v[0:16], v[16:19], c["w"], c["h"], v[19], v[20], v[21])


def sphere_ys(ctx, c):
    return np.array([ctx.get_object(i)[1][1] for i in range(len(c["objs"]))], dtype=np.float32)


def normals_frames(c):
    """RGB_NORMALS through the oracle: per step (frame with NORMALS_WRAP: what the host build gives; frame without: what a GPU
    gives), after checking that the two differ only in digit triples whose normal component is negative."""
    w, h = c["w"], c["h"]
    out = []
    for (st, wrap, px), (_, sat, _) in zip(RC.oracle_steps(c, O.NORMALS_WRAP), RC.oracle_steps(c, 0)):
        a, b = wrap.reshape(h, w, 20), sat.reshape(h, w, 20)
        other = np.ones(20, dtype=bool)
        for comp, off in enumerate((7, 11, 15)):
            other[off:off + 3] = False
            differs = (a[:, :, off:off + 3] != b[:, :, off:off + 3]).any(axis=2)
            assert not (differs & ~(px["normal"][:, :, comp] < 0)).any(), "%s: a digit triple of a non-negative normal component differs" % c["name"]
        assert np.array_equal(a[:, :, other], b[:, :, other]), c["name"]
        out.append((wrap, sat))
    return out


def check_render(R, ctx, c, expect):
    """rtx_render_rows under every plan, after every step of the case, and update_objects' y against the reference's."""
    w, h, mode = c["w"], c["h"], c["mode"]
    p = product_params(c)
    load_scene(ctx, c)
    normals = normals_frames(c) if mode == O.RGB_NORMALS else None
    S = 20 if mode >= O.RGB_ASCII else 12
    for k, dt in enumerate(c["dts"]):
        ctx.update_objects(dt)
        assert np.array_equal(sphere_ys(ctx, c).view(np.uint32), expect["states"][k]["y"].view(np.uint32)), \
            "%s step %d: sphere y after update_objects differs from the reference's" % (c["name"], k)
        if normals is not None:
            # 1. the reference equals the oracle with NORMALS_WRAP
            assert RC.frame_matches(expect, k, normals[k][0]), "%s step %d: reference (%s) != oracle with NORMALS_WRAP" % (c["name"], k, expect["source"])
        for plan in PLANS:
            set_plan(R, ctx, plan)
            got = ctx.render_to_host(p, mode)
            what = "%s step %d, %r, kernel %s" % (c["name"], k, plan, ctx.last_kernel)
            KERNELS_SEEN.setdefault(plan, set()).add(ctx.last_kernel)
            if normals is not None:
                # 2. the kernel equals the oracle without it (3. is normals_frames' own check)
                assert np.array_equal(got, normals[k][1]), "%s: kernel != oracle: %s" % (what, U.first_diff(got, normals[k][1], S, w))
            elif "frames" in expect:
                assert np.array_equal(got, expect["frames"][k]), "%s: kernel != reference (%s): %s" % (
                    what, expect["source"], U.first_diff(got, expect["frames"][k], S, w))
            else:
                assert RC.frame_matches(expect, k, got), "%s: the kernel's frame does not hash to the reference's (%s)" % (what, expect["source"])
    set_plan(R, ctx, DEFAULT_PLAN)


def check_update(R, ctx, c, expect):
    """rtx_update with physics, step by step: the stream is the reference's SetDataInBackBuffer bytes, fused Minimize and not."""
    w, h, mode = c["w"], c["h"], c["mode"]
    p = product_params(c)
    normals = normals_frames(c) if mode == O.RGB_NORMALS else None
    before = ctx.get_option(R.OPT_MINIMIZE_FUSED)
    try:
        for fused in (1, 0):
            ctx.set_option(R.OPT_MINIMIZE_FUSED, fused)
            load_scene(ctx, c)
            for k, dt in enumerate(c["dts"]):
                got = np.array(ctx.update(p, mode, dt=dt, run_physics=True))
                what = "%s step %d, fused %d" % (c["name"], k, fused)
                if normals is not None:
                    assert RC.stream_matches(expect, k, O.minimize(mode, normals[k][0], w, h)), what
                    assert np.array_equal(got, O.minimize(mode, normals[k][1], w, h)), what + ": rtx_update != Minimize of the oracle's frame"
                else:
                    assert RC.stream_matches(expect, k, got), "%s: rtx_update's stream (%d bytes) != the reference's (%s)" % (what, got.size, expect["source"])
                assert np.array_equal(sphere_ys(ctx, c).view(np.uint32), expect["states"][k]["y"].view(np.uint32)), what
    finally:
        ctx.set_option(R.OPT_MINIMIZE_FUSED, before)


# ---------------------------------------------------------------------------------------------------- recorded cases

@pytest.mark.parametrize("c", RECORDED, ids=[c["name"] for c in RECORDED])
def test_render_rows_recorded(R, ctx, c):
    check_render(R, ctx, c, c["expect"])


@pytest.mark.parametrize("c", RECORDED, ids=[c["name"] for c in RECORDED])
def test_update_recorded(R, ctx, c):
    check_update(R, ctx, c, c["expect"])


def test_plans_reach_both_kernel_families(R, ctx):
    """The plans are requests; what ran is in the kernel's name: rtx_trace<mode,false> is the brute kernel, <mode,true...> the
    culling one, and per-wave refinement ends the name with ",refine>"."""
    c = [c for c in RECORDED if c["name"].startswith("objects_1024/")][0]
    KERNELS_SEEN.clear()
    check_render(R, ctx, c, c["expect"])
    for plan, names in KERNELS_SEEN.items():
        assert all(n.startswith("rtx_trace<") for n in names), (plan, names)
        assert all(("false" in n) == (plan[0] == "brute") and ("true" in n) == (plan[0] == "binned") for n in names), (plan, names)
    assert any(n.endswith(",refine>") for plan, names in KERNELS_SEEN.items() if plan[4] for n in names), KERNELS_SEEN
    assert not any(n.endswith(",refine>") for plan, names in KERNELS_SEEN.items() if not plan[4] for n in names), KERNELS_SEEN


_PHYSICS = [c for c in RECORDED if c["name"].startswith("physics/")]


@pytest.mark.parametrize("c", _PHYSICS, ids=[c["name"] for c in _PHYSICS])
def test_update_objects_recorded(R, ctx, c):
    """rtx_update_objects alone: y of every sphere after every step, read back with rtx_scene_get_object, against the reference's;
    mover too (rtx_scene_get_object's eighth float)."""
    load_scene(ctx, c)
    for k, dt in enumerate(c["dts"]):
        ctx.update_objects(dt)
        want = c["expect"]["states"][k]
        got = [ctx.get_object(i)[1] for i in range(len(c["objs"]))]
        assert np.array_equal(np.array([g[1] for g in got], dtype=np.float32).view(np.uint32), want["y"].view(np.uint32)), "%s step %d" % (c["name"], k)
        assert [int(g[7]) for g in got] == want["mover"].tolist(), "%s step %d" % (c["name"], k)


def check_minimize(R, ctx, m):
    import torch
    name, mode, w, h, buf, words, stream = m
    d_in = torch.from_numpy(buf).cuda()
    d_words = torch.from_numpy(words.astype(np.uint32).view(np.int32)).cuda()
    d_out = torch.zeros(20 * w * h + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = ctx.get_option(R.OPT_MINIMIZE_FUSED)
    try:
        for fused in (1, 0):
            ctx.set_option(R.OPT_MINIMIZE_FUSED, fused)
            n = ctx.minimize(mode, w, h, d_in=d_in.data_ptr(), d_out=d_out.data_ptr())
            assert np.array_equal(d_out.cpu().numpy()[:n], stream), "%s: rtx_minimize, fused %d: %d bytes, the reference's %d" % (name, fused, n, stream.size)
            d_out.zero_()
            torch.cuda.synchronize()
            n = ctx.minimize_words(mode, w, h, d_words.data_ptr(), d_out=d_out.data_ptr())
            assert np.array_equal(d_out.cpu().numpy()[:n], stream), "%s: rtx_minimize_words, fused %d: %d bytes, the reference's %d" % (name, fused, n, stream.size)
    finally:
        ctx.set_option(R.OPT_MINIMIZE_FUSED, before)


@pytest.mark.parametrize("m", RECORDED_MINIMIZE, ids=[m[0] for m in RECORDED_MINIMIZE])
def test_minimize_recorded(R, ctx, m):
    check_minimize(R, ctx, m)


def test_camera_builder_recorded(R):
    """rtx_camera_params against what Camera3D gave for the fifty poses: matrix, element1, element2, far, all bits."""
    w, h = RC.CAMERA_SIZE
    for pose, want in zip(CAM_POSES, CAM_PARAMS):
        pp = R.camera_params(w, h, [float(v) for v in pose[:3]], [float(v) for v in pose[3:]])
        got = RH.raw_params(np.array(pp.inv_v[:], dtype=np.float32), pp.cam_pos[:], pp.element1, pp.element2, pp.cam_far)
        assert RH.same_bits(got, want), "pose %r" % (pose,)


# ---------------------------------------------------------------------------------------------------- live cases

def _live_cases(chunk):
    if chunk == "objects_1024":
        return [RC.big_scene_case(m) for m in RC.MODES if m != O.RGB_ASCII]      # (RGB_ASCII is recorded)
    return [RC.fuzz_case(s) for s in range(chunk * LIVE_CHUNK, (chunk + 1) * LIVE_CHUNK)]


@pytest.mark.parametrize("chunk", list(range(LIVE_FUZZ_SEEDS // LIVE_CHUNK)) + ["objects_1024"])
def test_render_rows_and_update_live(R, ctx, chunk):
    """Where oracle/_ref/ holds the binaries: the first forty fuzz seeds of tests/test_ref_host.py (frames up to 120 x 41, up to
    700 spheres) and the 1024-object scene in the other modes, run through ref_driver_pinpow now.  Elsewhere the recorded cases
    above are the whole check."""
    if not LIVE:
        return
    for c in _live_cases(chunk):
        expect = RC.expect_from_live(c)
        check_render(R, ctx, c, expect)
        check_update(R, ctx, c, expect)


def test_minimize_live(R, ctx):
    if not LIVE:
        return
    for name, mode, w, h, buf, words in RC.minimize_frames():
        check_minimize(R, ctx, (name, mode, w, h, buf, words, RH.minimize(mode, buf, w, h)))
