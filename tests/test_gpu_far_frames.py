"""The far cut in the trace kernels' table-plane test (csrc/rtx_far.hpp, rtx_trace_body.inc) against the oracle, on the project's
smallest frames (37 x 21: one partial macro tile; 64 x 48: a whole one).  Records and compact pixel words drop, before the
division, the lanes whose hit on a table plane provably lies beyond cam_far -- pixels the record encoder writes as misses either
way -- and a wave none of whose pixels is visible skips the winner's normal and shading (scene c's sphere under the floor and
f17's direct-form floor reach that skip with hits the cut does not remove); the value floats and the closest-hit form (the light
path's first launch) keep the parent's test and shade every hit.

Every frame is byte-equal to the oracle's: records and compact words in the five record modes, from the binned, the brute and the
REFINE kernels, from row 0 and as a slab that starts at row 5, and through the batched entry points.
  a     a floor whose far boundary runs through the frame: some 8 x 8 regions lie wholly beyond far, some straddle it
  b-/b0/b+  the same floor with cam_far one float below, at, and one float above the oracle's distance of a chosen floor pixel:
        that pixel is visible from b0 on and a miss in b-
  c     a plus three spheres: one nearer than far in front of the beyond-far band, one under the floor behind the beyond-far hits
        (beyond far itself), one straddling far
  d*    c under special far values: +inf, 0, negative, NaN, FLT_MAX, a subnormal
  e*    the floor scaled by 1e18 (its far lies past the no-hit distance) and by 1e-18, a floor at y = -1e38 under far 100 (the
        quotient num / far overflows), and floor normals of length 1e-10 and 1e10 (the reference does not normalise n in dn)
  f2    two coincident floors (the creation index decides);  f17  seventeen planes, the floor last: it takes the direct form
The untouched forms: RTX_RENDER_VALUES of a and c equals the oracle's pixel floats bit for bit, the beyond-far pixels included
(they still carry the plane's distance, normal and colour), and frames through the closest-hit launch (one light, shadows on) equal
the oracle's where nothing is shadowed and are lit or dark by the float64 rule of test_gpu_shadows.py where shadows fall."""
import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(37, 21), (64, 48)]
MODES = [O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS]
PLANS = ["binned", "brute", "refine"]
FAR = 66.0
CAM_POS, CAM_ROT = (0.0, 20.0, 0.0), (0.56, float(f32(np.pi)), 0.0)   # 32 units above the floor, pitched down: the floor fills the frame
SUBNORMAL = float(np.uint32(0x007FFFFF).view(f32))

FLOOR = np.array([[0, -12, 150, 0, 1, 0, 100, 160, 60, 4000, 4000]], dtype=f32)
SPHERES = np.array([[-3, 13, 39, 4, 255, 40, 10],       # nearer than far, in front of the beyond-far band
                    [12, -42, 180, 25, 20, 90, 255],    # under the floor: behind the floor's beyond-far hits, beyond far itself
                    [6.3, -3.9, 65.5, 7, 240, 240, 240]], # straddles far
                   dtype=f32)
NO_SPHERES = np.zeros((0, 7), dtype=f32)

CASES = ["a", "b-", "b0", "b+", "c", "d_inf", "d_zero", "d_neg", "d_nan", "d_max", "d_sub", "e_big", "e_small", "e_overflow", "e_n_short", "e_n_long",
         "f2", "f17"]


def _scene(name):
    if name in ("a", "b-", "b0", "b+"):
        return NO_SPHERES, FLOOR
    if name == "c" or name.startswith("d_"):
        return SPHERES, FLOOR
    pl = FLOOR.copy()
    if name in ("e_big", "e_small"):
        s = f32(1e18) if name == "e_big" else f32(1e-18)
        pl[:, :3] *= s
        pl[:, 9:] *= s
        return NO_SPHERES, pl
    if name == "e_overflow":
        pl[0, 1] = f32(-1e38)
        pl[0, 9:] = f32(3e38)
        return NO_SPHERES, pl
    if name in ("e_n_short", "e_n_long"):
        pl[0, 4] = f32(1e-10) if name == "e_n_short" else f32(1e10)
        return SPHERES, pl
    if name == "f2":
        second = FLOOR.copy()
        second[0, 6:9] = [30, 30, 250]
        return SPHERES, np.concatenate([FLOOR, second])
    assert name == "f17"
    patches = []
    for i in range(16):
        # small patches a little above the floor, near and far, in creation order before it: they fill the LDS table
        patches.append([-30 + 4 * i, -11.5 + 0.02 * i, 25 + 6 * i, 0, 1, 0, 10 + 15 * i, 250 - 15 * i, 40, 10, 12])
    return SPHERES, np.concatenate([np.array(patches, dtype=f32), FLOOR])


_cache = {}


def _base(R, shape, scale=1.0):
    return R.camera_params(shape[0], shape[1], pos=tuple(float(f32(v) * f32(scale)) for v in CAM_POS), rot=CAM_ROT)


def _with_far(p, far):
    return U.product_params(np.array(p.inv_v[:], dtype=f32).reshape(4, 4), p.cam_pos[:], int(p.x), int(p.y), p.element1, p.element2, far)


def _chosen_pixel(R, shape):
    """A floor pixel of scene a whose distance no other pixel shares: the one nearest below FAR."""
    _, px = _want(R, shape, "a", O.RGB_ASCII)
    d = px["distance"].copy()
    d[:, -1] = np.inf
    below = np.where((px["hit"] != 0) & (d <= f32(FAR)), d, -np.inf)
    r, c = np.unravel_index(int(np.argmax(below)), below.shape)
    return int(r), int(c), f32(d[r, c])


def _params(R, shape, name):
    p = _base(R, shape, {"e_big": 1e18, "e_small": 1e-18}.get(name, 1.0))
    far = FAR
    if name in ("b-", "b0", "b+"):
        d = _chosen_pixel(R, shape)[2]
        far = float({"b-": np.nextafter(d, f32(0)), "b0": d, "b+": np.nextafter(d, f32(np.inf))}[name])
    elif name.startswith("d_"):
        far = {"d_inf": float("inf"), "d_zero": 0.0, "d_neg": -60.0, "d_nan": float("nan"), "d_max": 3.4028234663852886e38, "d_sub": SUBNORMAL}[name]
    elif name == "e_big":
        far = float(f32(FAR) * f32(1e18))
    elif name == "e_small":
        far = float(f32(FAR) * f32(1e-18))
    elif name == "e_overflow":
        far = 100.0
    return _with_far(p, far)


def _want(R, shape, name, mode):
    """The oracle's frame and per-pixel values of a case, computed once and shared by the plans."""
    key = (shape, name, mode)
    if key not in _cache:
        W, H = shape
        p = _with_far(_base(R, shape), FAR) if name == "a" else _params(R, shape, name)
        sph, pl = _scene(name)
        frame, px = O.render(U.oracle_params(p), O.Scene.from_arrays(sph, pl), mode, want_pixels=True)
        frame.setflags(write=False)
        px.setflags(write=False)
        _cache[key] = (frame, px.reshape(H, W))
    return _cache[key]


def regions(px, far):
    """Of the oracle's pixels, per 8 x 8-aligned region (column W-1 is never traced): how many regions have every pixel a hit
    beyond far, and how many have both a visible pixel and a hit beyond far."""
    H, W = px.shape
    hit = px["hit"] != 0
    beyond = hit & (px["distance"] > f32(far))
    visible = hit & (px["distance"] <= f32(far))
    traced = np.ones((H, W), dtype=bool)
    traced[:, -1] = False
    wholly = straddling = 0
    for r0 in range(0, H, 8):
        for c0 in range(0, W, 8):
            t = traced[r0:r0 + 8, c0:c0 + 8]
            if not t.any():
                continue
            b, v = beyond[r0:r0 + 8, c0:c0 + 8][t], visible[r0:r0 + 8, c0:c0 + 8][t]
            wholly += bool(b.all())
            straddling += bool(b.any() and v.any())
    return wholly, straddling


def check_scenes(R):
    """What the scenes are for, from the oracle's pixels alone (no GPU)."""
    for shape in SHAPES:
        W, H = shape
        _, px = _want(R, shape, "a", O.RGB_ASCII)
        wholly, straddling = regions(px, FAR)
        assert wholly >= 1 and straddling >= 1, (shape, wholly, straddling)
        # b: visibility flips exactly at the chosen pixel
        r, c, d = _chosen_pixel(R, shape)
        assert int((px["distance"][:, :-1] == d).sum()) == 1
        miss = U.miss_record(20)
        recs = {n: _want(R, shape, n, O.RGB_ASCII)[0][:20 * W * H].reshape(H, W, 20) for n in ("b-", "b0", "b+")}
        assert bytes(recs["b-"][r, c]) == bytes(miss) and bytes(recs["b0"][r, c]) != bytes(miss) and bytes(recs["b+"][r, c]) == bytes(recs["b0"][r, c])
        differ = (recs["b-"] != recs["b0"]).any(-1)
        assert int(differ.sum()) == 1 and differ[r, c] and np.array_equal(recs["b0"], recs["b+"])
        # c: the three spheres do what they are there for
        _, pa = _want(R, shape, "a", O.RGB_ASCII)
        _, pc = _want(R, shape, "c", O.RGB_ASCII)
        on_sphere = (pc["hit"] != 0) & (pc["normal"][..., 1] != 1.0)
        on_sphere[:, -1] = False
        floor_beyond = (pa["hit"] != 0) & (pa["distance"] > f32(FAR))
        assert int((on_sphere & floor_beyond & (pc["distance"] < 50.0)).sum()) >= 3          # the near sphere over the beyond-far band
        assert int((on_sphere & (pc["distance"] <= f32(FAR))).sum()) >= 10 and int((on_sphere & (pc["distance"] > f32(FAR))).sum()) >= 3
        # the sphere under the floor is never the closest hit, and every ray that reaches it meets the floor beyond far first
        assert not (on_sphere & (pc["distance"] > 80.0)).any()
        # e: the scaled floors hit nothing the oracle can see, the long normal changes nothing, the short one removes the floor
        assert int((_want(R, shape, "e_big", O.RGB_ASCII)[1]["hit"] != 0).sum()) == 0
        pe = _want(R, shape, "e_small", O.RGB_ASCII)[1]
        assert regions(pe, float(f32(FAR) * f32(1e-18)))[0] >= 1
        assert int(((_want(R, shape, "e_n_short", O.RGB_ASCII)[1]["normal"][..., 1] == 1.0) & (pc["hit"] != 0)).sum()) == 0
        # f17: the floor is plane 16 and is seen; some table patch is seen too
        pf = _want(R, shape, "f17", O.RGB_ASCII)[1]
        vis = (pf["hit"] != 0) & (pf["distance"] <= f32(FAR))
        vis[:, -1] = False
        pfa = _want(R, shape, "c", O.RGB_ASCII)[1]
        assert int((vis & (pf["distance"] < pfa["distance"])).sum()) >= 3                    # a patch of the table in front of the floor
        assert int((vis & (pf["distance"] == pfa["distance"]) & (pf["normal"][..., 1] == 1.0)).sum()) >= 10   # the floor itself


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(64, 48)
    yield c
    c.close()


def _rows(R, c, p, mode, flags, S, row0=0):
    import torch
    W, H = int(p.x), int(p.y)
    buf = torch.full((W * (H - row0) * S,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fill is queued on torch's stream; the library renders on its own)
    c.render_rows(p, mode, row0, H - row0, d_out=buf.data_ptr(), out_row_base=row0, flags=flags)
    c.synchronize()
    return buf.cpu().numpy()


def same_bits_or_both_nan(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _set_plan(R, c, plan):
    c.set_option(R.OPT_KERNEL, R.KERNEL_BRUTE if plan == "brute" else R.KERNEL_BINNED)
    c.set_option(R.OPT_REFINE, 1 if plan == "refine" else 0)


def _reset_plan(R, c):
    c.set_option(R.OPT_KERNEL, R.KERNEL_AUTO)
    c.set_option(R.OPT_REFINE, -1)


def test_the_scenes_show_what_they_are_for(R):
    check_scenes(R)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=["37x21", "64x48"])
def test_records_and_compact_words_match_the_oracle(R, ctx, shape, name, plan):
    W, H = shape
    if name == "a":
        wholly, straddling = regions(_want(R, shape, "a", O.RGB_ASCII)[1], FAR)   # before anything is rendered
        assert wholly >= 1 and straddling >= 1
    p = _params(R, shape, name)
    sph, pl = _scene(name)
    _set_plan(R, ctx, plan)
    ctx.set_scene(sph, pl)
    try:
        for mode in MODES:
            S = 20 if mode >= O.RGB_ASCII else 12
            want = _want(R, shape, name, mode)[0][:S * W * H]
            kind = ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4")
            for row0 in (0, 5):
                got = _rows(R, ctx, p, mode, 0, S, row0)
                kernel = ctx.last_kernel
                assert kernel.startswith("rtx_trace<") and ("true" if plan != "brute" else "false") in kernel, kernel
                assert kernel.endswith(",refine>") == (plan == "refine"), kernel
                assert np.array_equal(got, want[row0 * W * S:]), "%s %s %s records from row %d: %s" % (
                    name, plan, O.MODE_NAMES[mode], row0, U.first_diff(got, want[row0 * W * S:], S, W))
                words = _rows(R, ctx, p, mode, R.RENDER_COMPACT, 4, row0).view(np.uint32)
                assert ctx.last_kernel.endswith(",refine>") == (plan == "refine"), ctx.last_kernel
                back = U.words_to_records(words, S, kind)
                assert np.array_equal(back, want[row0 * W * S:]), "%s %s %s compact words from row %d: %s" % (
                    name, plan, O.MODE_NAMES[mode], row0, U.first_diff(back, want[row0 * W * S:], S, W))
    finally:
        _reset_plan(R, ctx)


@pytest.mark.parametrize("name", ["a", "c", "f17"])
@pytest.mark.parametrize("shape", SHAPES, ids=["37x21", "64x48"])
def test_batched_entries_match_the_oracle(R, ctx, shape, name):
    """rtx_submit_frames and rtx_submit_slabs (one batched launch of rtx_trace_batch) with three cameras that share far."""
    import torch
    W, H = shape
    sph, pl = _scene(name)
    sc = O.Scene.from_arrays(sph, pl)
    cams = [_with_far(R.camera_params(W, H, pos=(CAM_POS[0] + 0.3 * i, CAM_POS[1] + 0.5 * i, CAM_POS[2] - 0.4 * i),
                                      rot=(CAM_ROT[0] + 0.02 * i, CAM_ROT[1] + 0.03 * i, 0.0)), FAR) for i in range(3)]
    ctx.set_option(R.OPT_KERNEL, R.KERNEL_BINNED)
    ctx.set_option(R.OPT_REFINE, 0)
    ctx.set_scene(sph, pl)
    try:
        st = torch.cuda.Stream()
        for mode in (O.RGB_ASCII, O.BIT_PIXEL):
            S = 20 if mode >= O.RGB_ASCII else 12
            want = [O.render(U.oracle_params(q), sc, mode)[:S * W * H] for q in cams]
            bufs = [torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda") for _ in cams]
            torch.cuda.synchronize()
            ctx.submit_frames(cams, mode, [b.data_ptr() for b in bufs], [st.cuda_stream] * 3)
            torch.cuda.synchronize()
            for i, b in enumerate(bufs):
                got = b.cpu().numpy()
                assert np.array_equal(got, want[i]), "%s frames %d: %s" % (name, i, U.first_diff(got, want[i], S, W))
            for flags, Sw in ((0, S), (R.RENDER_COMPACT, 4)):
                slabs = [torch.full((W * (H - 5) * Sw,), 0xEE, dtype=torch.uint8, device="cuda") for _ in cams]
                torch.cuda.synchronize()
                before = ctx.get_option(R.STAT_BATCHED_LAUNCHES)
                ctx.submit_slabs(cams, mode, 5, H - 5, [b.data_ptr() for b in slabs], 5, [st.cuda_stream] * 3, flags=flags)
                torch.cuda.synchronize()
                assert ctx.get_option(R.STAT_BATCHED_LAUNCHES) == before + 1 and "rtx_trace_batch" in ctx.last_kernel, ctx.last_kernel
                for i, b in enumerate(slabs):
                    got = b.cpu().numpy()
                    if flags:
                        got = U.words_to_records(got.view(np.uint32), S, ord("3") if mode == O.RGB_ASCII else ord("4"))
                    assert np.array_equal(got, want[i][5 * W * S:]), "%s slabs %d flags %d: %s" % (name, i, flags, U.first_diff(got, want[i][5 * W * S:], S, W))
    finally:
        _reset_plan(R, ctx)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", ["a", "c"])
@pytest.mark.parametrize("shape", SHAPES, ids=["37x21", "64x48"])
def test_value_floats_keep_the_beyond_far_hits(R, ctx, shape, name, plan):
    W, H = shape
    p = _params(R, shape, name)
    sph, pl = _scene(name)
    _set_plan(R, ctx, plan)
    ctx.set_scene(sph, pl)
    try:
        _, px = _want(R, shape, name, O.RGB_ASCII)
        got = _rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES, 32).view(f32).reshape(H, W, 8)
        traced = np.ones((H, W), dtype=bool)
        traced[:, -1] = False
        hit = (px["hit"] != 0) & traced
        beyond = hit & (px["distance"] > f32(FAR))
        assert int(beyond.sum()) >= 64 and int((beyond & (px["normal"][..., 1] == 1.0)).sum()) >= 64   # the floor's beyond-far pixels are in the comparison
        for what, g, w in (("distance", got[..., 0][traced], px["distance"][traced]),
                           ("shadingValue", got[..., 1][hit], px["shading_value"][hit]), ("normal", got[..., 2:5][hit], px["normal"][hit]),
                           ("colour", got[..., 5:8][hit], px["color"][hit])):
            ok = same_bits_or_both_nan(np.ascontiguousarray(g), np.ascontiguousarray(w))
            assert ok.all(), "%s %s: %s differs on %d of %d values" % (name, plan, what, int((~ok).sum()), ok.size)
        assert not got[:, -1, :].any()
    finally:
        _reset_plan(R, ctx)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", SHAPES, ids=["37x21", "64x48"])
def test_closest_hit_launch_keeps_the_parents_test(R, ctx, shape, plan):
    """Scene c through the light path (kOutHit, then rtx_shadow_shade) under one light: with every pixel lit (RTX_OPT_SHADOW_CHECK 2)
    the frame is the oracle's byte for byte; with shadows falling every pixel is the lit or the dark record, as float64 decides."""
    from test_gpu_shadows import _check_lit_or_dark
    W, H = shape
    p = _params(R, shape, "c")
    sph, pl = _scene("c")
    _set_plan(R, ctx, plan)
    ctx.set_scene(sph, pl)
    try:
        for mode in (O.RGB_ASCII, O.BIT_PIXEL):
            S = 20 if mode >= O.RGB_ASCII else 12
            want = _want(R, shape, "c", mode)[0][:S * W * H]
            ctx.set_light(R.make_light())
            ctx.set_option(R.OPT_SHADOWS, 1)
            ctx.set_option(R.OPT_SHADOW_CHECK, 2)
            got = _rows(R, ctx, p, mode, 0, S)
            assert "rtx_shadow_shade" in ctx.last_kernel, ctx.last_kernel
            assert np.array_equal(got, want), "%s %s: %s" % (plan, O.MODE_NAMES[mode], U.first_diff(got, want, S, W))
            ctx.set_option(R.OPT_SHADOW_CHECK, 0)
            ctx.set_light(R.make_light(pos=(0.0, 50.0, 40.0)))
            _check_lit_or_dark(R, ctx, p, sph, pl, mode)
    finally:
        ctx.set_option(R.OPT_SHADOWS, 0)
        ctx.set_option(R.OPT_SHADOW_CHECK, 0)
        ctx.set_light(None)
        _reset_plan(R, ctx)
