"""Shadow tests through the world grid (RTX_OPT_SHADOW_GRID, include/rtx.h).  The option changes which spheres a shadow segment is
tested against, never the test, so every frame must be the existing path's byte for byte.

The reference of every comparison is the same context with the option 0 and RTX_OPT_SHADOW_CHECK 1: the brute path that tests
every sphere, which is not the code under test.  Whole buffers are compared, in the three output forms (values, records, compact
words) and the four character modes, on frames of 37 x 21 and 64 x 48 cells (ragged 16 x 16 tiles, a newline column).

Scenes, the smallest at which the kernel can still go wrong:
  a  40 spheres, no plane, the light inside the cloud;
  b  300 spheres in a compact cloud -- the direction-sorted store is engaged from 256, so a sphere's position in the trace
     kernels' arrays is not its creation index -- and one sphere large enough for the grid's large list; the reference light
     (1, 50, 0), far outside the box;
  c  b over a floor that reaches far beyond `reach` (three times the box's largest half-extent from its centre);
  d  40 small spheres near the origin under sets of 3 and 8 lights (of powers that suit their distance: D_POWER), one of them one
     ulp in front of a visible hit point: where the coordinates are below 8 an ulp is shorter than 2^-20, the shortest segment
     the walk takes, so that segment is degenerate
     (a light AT the point has dot(n, L - P) = 0: it is dark before any sphere is tested, in both paths);
  e  c with the floor and a quarter of the spheres reflective, depth 1 and 3, RTX_OPT_REFLECT_SHADOWS 0 and 1.
Hit points on spheres lie inside the spheres' box and hence within `reach`: on sphere-only scenes no segment falls back unless
it is degenerate (a, b: exactly 0; d: exactly the one made so), and on c's floor some do.

A comparison must not be empty: judged on the reference frames against the all-lit frame (RTX_OPT_SHADOW_CHECK 2), at least 5 % of
the visible pixels are dark and at least 5 % lit, and the grid has more than one cell."""

import numpy as np
import pytest

import oracle as O
import restate as RS
import restate_shadows as RH
import util as U
import test_gpu_reflect as T
import test_gpu_chain_lights as TC

pytestmark = pytest.mark.gpu

SIZES = [(37, 21), (64, 48)]
FORMS = ["values", "records", "compact"]
NO_HIT = np.float32(99999999.0)


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(640, 360)
    yield c
    c.close()


def _reset(R, c):
    TC._reset(R, c)
    c.set_option(R.OPT_REFLECT_SHADOWS, 0)
    c.set_option(R.OPT_SHADOW_GRID, 0)


# ---------------------------------------------------------------- scenes

def cloud(seed, n, centre, half, r_lo, r_hi):
    rng = np.random.default_rng(seed)
    sph = np.zeros((n, 7), dtype=np.float32)
    sph[:, :3] = np.asarray(centre) + rng.uniform(-1, 1, (n, 3)) * np.asarray(half)
    sph[:, 3] = rng.uniform(r_lo, r_hi, n)
    sph[:, 4:] = np.floor(rng.uniform(1, 256, (n, 3)))
    return sph


NO_PLANES = np.zeros((0, 11), dtype=np.float32)
FLOOR = np.array([[0, -12, 125, 0, 1, 0, 120, 120, 120, 2000, 2000]], dtype=np.float32)


def scene_b():
    sph = cloud(5, 300, (0, 0, 100), (15, 10, 15), 0.8, 2.2)
    big = np.array([[0, 0, 110, 8, 200, 60, 60]], dtype=np.float32)  # (four cells across on every axis and more: the large list)
    return np.concatenate([sph[:150], big, sph[150:]])


def scene(R, name, W, H):
    """(params, spheres, planes, lights as position tuples)"""
    p = R.camera_params(W, H)
    if name == "a":
        sph, pl = U.numpy_synth_scene(11, 40, 0, p.element1, p.element2)
        return p, sph, pl, [(0.0, 0.0, 115.0)]
    if name == "b":
        return p, scene_b(), NO_PLANES, [(1.0, 50.0, 0.0)]
    if name in ("c", "e"):
        return p, scene_b(), FLOOR, [(1.0, 50.0, 0.0)]
    assert name in ("d3", "d8")
    sph = cloud(9, 40, (0, 0, 4.5), (0.8, 0.5, 1.5), 0.1, 0.3)
    others = [(0.0, 3.0, 2.0), (-2.0, 1.0, 1.5), (2.0, 1.5, 1.0), (0.0, -2.0, 1.5), (0.3, 0.2, 1.2), (-1.0, 2.5, 0.5), (1.0, 0.0, 1.0)][:2 if name == "d3" else 7]
    # a visible hit point of a sphere, bit for bit as the shade launch forms it (the restatement's trace), and the light one ulp in
    # front of it: dot(n, L - P) > 0, so the segment is tested, and it is shorter than 2^-20
    op = U.oracle_params(p)
    trace = RS.trace_chain(op, sph, NO_PLANES, {}, np.arange(W * H), max_depth=1)
    idx, P, N, owner = RH.level_points(trace, 0)
    assert np.abs(P).max() < 8.0
    facing = np.nonzero(N[:, 2] < -0.9)[0]
    assert facing.size > 0
    Pq = P[facing[facing.size // 2]].astype(np.float32)
    near = (float(Pq[0]), float(Pq[1]), float(np.nextafter(Pq[2], np.float32(0.0))))
    assert 0.0 < float(Pq[2]) - near[2] < 2.0 ** -20
    pos = [others[0], near] + others[1:]
    return p, sph, NO_PLANES, pos


# d's lights stand 1 to 5 from its spheres, where the reference light's powers (2000 and 3000, meant for a distance of 50) drive every
# channel of every pixel to 255 with and without shadows: a comparison that sees no dark bit.  A five-hundredth of them leaves no
# pixel of the all-lit frame at 255 in all three channels (worked out with tests/restate_shadows.py: 29 / 23 % of the visible pixels
# dark under 3 lights at 37 x 21 / 64 x 48, 47 / 41 % under 8).
D_POWER = 0.002


def _set_lights(R, c, positions, zero=(), scale=1.0):
    """The lights at `positions`, the powers (times `scale`) shared out; those whose index is in `zero` with both powers 0."""
    n = len(positions)
    made = [R.make_light(pos=pos, diffuse_power=0.0 if i in zero else scale * 2000.0 / n, specular_power=0.0 if i in zero else scale * 3000.0 / n)
            for i, pos in enumerate(positions)]
    if n == 1:
        c.set_light(made[0])
    else:
        c.set_lights(made)


def _load(R, c, name, W, H):
    p, sph, pl, lights = scene(R, name, W, H)
    c.set_scene(sph, pl)
    # (d: the light on the sphere's surface lights only the half-space beyond the tangent plane there, which holds next to no visible
    # point -- with powers it would leave no pixel lit.  It gets powers 0 for the comparison the shares are judged on; its segment
    # shows in the fallback count, and test_frames_equal_the_brute_reference compares once more with its powers on.)
    d = name in ("d3", "d8")
    _set_lights(R, c, lights, zero=(1,) if d else (), scale=D_POWER if d else 1.0)
    c.set_option(R.OPT_SHADOWS, 1)
    if name == "e":
        ks = {len(sph): 0.5}  # the floor (created after the spheres)
        ks.update({i: 0.4 for i in range(0, len(sph), 4)})
        T._set_k(c, ks)
    return p, sph, pl


def _frames(R, c, p, modes=T.MODES, forms=FORMS):
    """{(mode, form): bytes} and the kernel names seen"""
    out, names = {}, set()
    for mode in modes:
        for form in forms:
            flags = {"values": R.RENDER_VALUES, "records": 0, "compact": R.RENDER_COMPACT}[form]
            out[(mode, form)] = T._rows(R, c, p, mode, flags)
            names.add(c.last_kernel.split("<")[0])
    return out, names


def _reference(R, c, p, **kw):
    c.set_option(R.OPT_SHADOW_GRID, 0)
    c.set_option(R.OPT_SHADOW_CHECK, 1)
    try:
        return _frames(R, c, p, **kw)
    finally:
        c.set_option(R.OPT_SHADOW_CHECK, 0)


def _on(R, c, p, **kw):
    c.set_option(R.OPT_SHADOW_GRID, 1)
    try:
        return _frames(R, c, p, **kw)
    finally:
        c.set_option(R.OPT_SHADOW_GRID, 0)


def _assert_same(got, want, what):
    for key in want:
        mode, form = key
        S = {"values": 32, "compact": 4}.get(form, 20 if mode >= O.RGB_ASCII else 12)
        assert np.array_equal(got[key], want[key]), "%s, %s %s: %s" % (what, O.MODE_NAMES[mode], form, U.first_diff(got[key], want[key], S, 1 << 30))


def _assert_not_empty(R, c, p, ref, what, render=T._rows):
    """At least 5 % of the reference's visible pixels are dark and 5 % lit (against the all-lit frame); the grid has cells."""
    c.set_option(R.OPT_SHADOW_GRID, 0)
    c.set_option(R.OPT_SHADOW_CHECK, 2)
    lit = render(R, c, p, O.RGB_ASCII, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
    c.set_option(R.OPT_SHADOW_CHECK, 0)
    v = ref[(O.RGB_ASCII, "values")].view(np.float32).reshape(-1, 8)
    W = int(p.x)
    visible = (v[:, 0] != NO_HIT) & (np.arange(len(v)) % W != W - 1) & (v[:, 0] <= np.float32(p.cam_far))
    dark = visible & (v[:, 5:8].view(np.uint32) != lit[:, 5:8].view(np.uint32)).any(axis=1)
    nv, nd = int(visible.sum()), int(dark.sum())
    cells = int(c.get_option(R.STAT_QUERY_GRID_CELLS))
    print("%s: %d visible, %d dark (%.1f %%), %d lit, %d cells" % (what, nv, nd, 100.0 * nd / max(nv, 1), nv - nd, cells))
    assert nv >= 40, what
    assert nd >= 0.05 * nv, "%s: only %d of %d visible pixels are dark" % (what, nd, nv)
    assert nv - nd >= 0.05 * nv, "%s: only %d of %d visible pixels are lit" % (what, nv - nd, nv)
    assert cells > 1, what


# ---------------------------------------------------------------- 1. the frames are the brute path's

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["a", "b", "c", "d3", "d8"])
def test_frames_equal_the_brute_reference(R, ctx, name, size):
    _reset(R, ctx)
    W, H = size
    p, sph, pl = _load(R, ctx, name, W, H)
    what = "scene %s %d x %d" % (name, W, H)
    ref, ref_names = _reference(R, ctx, p)
    assert ref_names == {"rtx_shadow_shade" if name in "abc" else "rtx_lights_shade"}, ref_names
    frames0 = ctx.get_option(R.STAT_SHADOW_GRID_FRAMES)
    got, names = _on(R, ctx, p)
    assert names == {"rtx_grid_shade"}, names
    assert ctx.get_option(R.STAT_SHADOW_GRID_FRAMES) == frames0 + len(got)
    assert ctx.get_option(R.STAT_QUERY_BRUTE) == 0
    fallback = ctx.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS)
    large = ctx.get_option(R.STAT_QUERY_LARGE_SPHERES)
    print(what, "fallback segments", fallback, "large spheres", large, "pairs", ctx.get_option(R.STAT_QUERY_GRID_PAIRS))
    _assert_same(got, ref, what)
    _assert_not_empty(R, ctx, p, ref, what)
    if name in ("b", "c"):
        assert large >= 1 and len(sph) >= 256
    # hit points on spheres lie within `reach`: nothing falls back unless it is degenerate; the far floor does
    if name in ("a", "b"):
        assert fallback == 0
    elif name == "c":
        assert fallback > 0
    else:
        assert fallback == 1
        # once more with the powers of the light on the surface on: its dark bits show in the bytes (next to no pixel stays lit)
        _set_lights(R, ctx, scene(R, name, W, H)[3], scale=D_POWER)
        ref, _ = _reference(R, ctx, p, modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["values", "records"])
        got, _ = _on(R, ctx, p, modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["values", "records"])
        assert ctx.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS) == 1
        _assert_same(got, ref, what + ", every light with powers")
    _reset(R, ctx)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("depth", [1, 3])
def test_mirrors_equal_the_brute_reference(R, ctx, depth, deep, size):
    _reset(R, ctx)
    W, H = size
    p, sph, pl = _load(R, ctx, "e", W, H)
    ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, deep)
    what = "mirrors depth %d, deep shadows %d, %d x %d" % (depth, deep, W, H)
    ref, ref_names = _reference(R, ctx, p)
    want_pts = [int(ctx.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(R.MAX_REFLECT_DEPTH)]
    assert ref_names == {"rtx_lights_chain_shadow_shade" if deep else ("rtx_lights_chain_shade" if depth > 1 else "rtx_reflect_shade")}, ref_names
    got, names = _on(R, ctx, p)
    assert names == {"rtx_grid_chain_shadow_shade" if deep else ("rtx_grid_chain_shade" if depth > 1 else "rtx_grid_reflect_shade")}, names
    pts = [int(ctx.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(R.MAX_REFLECT_DEPTH)]
    print(what, "points per level", pts, "fallback segments", ctx.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS))
    assert pts == want_pts
    assert (pts[0] > 0 and (depth == 1 or pts[1] > 0)) if deep else pts == [0, 0, 0, 0]
    _assert_same(got, ref, what)
    _assert_not_empty(R, ctx, p, ref, what)
    if deep:  # the deeper levels' tests show: without them the frame is another one
        ctx.set_option(R.OPT_REFLECT_SHADOWS, 0)
        off, _ = _on(R, ctx, p, modes=[O.RGB_ASCII], forms=["values"])
        assert not np.array_equal(off[(O.RGB_ASCII, "values")], got[(O.RGB_ASCII, "values")])
    _reset(R, ctx)


def test_three_lights_over_the_floor_and_mirrors(R, ctx):
    """A light set on the chain with the deeper levels tested: every bit of the level words is in use."""
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "e", 64, 48)
    _set_lights(R, ctx, [(1.0, 50.0, 0.0), (0.0, 30.0, 100.0), (-40.0, 20.0, 60.0)])
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    ref, _ = _reference(R, ctx, p)
    got, names = _on(R, ctx, p)
    assert names == {"rtx_grid_chain_shadow_shade"}
    _assert_same(got, ref, "three lights, depth 2")
    _assert_not_empty(R, ctx, p, ref, "three lights, depth 2")
    _reset(R, ctx)


# One context, one stream, another hit-buffer layout at every frame (rtxplan::plan_shading, csrc/rtx_plan.hpp): the buffer is
# reused at a smaller size, grows, and level 0's words move.  (mirrors, depth, RTX_OPT_REFLECT_SHADOWS, RTX_OPT_SHADOW_GRID) ->
# the family that shades and the hit buffer's bytes per pixel, under two lights with shadows on.
LAYOUT_STEPS = [
    ((0, 1, 0, 0), "rtx_lights_shade", 8),
    ((1, 3, 1, 1), "rtx_grid_chain_shadow_shade", 40),
    ((1, 1, 0, 0), "rtx_lights_reflect_shade", 16),
    ((1, 3, 1, 0), "rtx_lights_chain_shadow_shade", 36),
    ((1, 1, 0, 1), "rtx_grid_reflect_shade", 20),
    ((0, 1, 0, 1), "rtx_grid_shade", 12),
    ((0, 1, 0, 0), "rtx_lights_shade", 8),
]
SLAB = (5, 14)  # rows 5 .. 18 of 21: hit indices are relative to row0, and the only tile row has 14 of its 16 rows


def _slab(R, c, p, mode, flags=0):
    import torch
    row0, rows = SLAB
    S = 32 if flags & R.RENDER_VALUES else (20 if mode >= O.RGB_ASCII else 12)
    buf = torch.full((rows * int(p.x) * S,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.render_rows(p, mode, row0, rows, d_out=buf.data_ptr(), out_row_base=row0, flags=flags)
    c.synchronize()
    return buf.cpu().numpy()


def test_one_stream_changes_the_hit_buffer_layout_from_frame_to_frame(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "e", 37, 21)
    mirrors = {len(sph): 0.5}
    mirrors.update({i: 0.4 for i in range(0, len(sph), 4)})
    _set_lights(R, ctx, [(1.0, 50.0, 0.0), (0.0, 30.0, 100.0)])
    keys = [(O.RGB_ASCII, "values"), (O.RGB_ASCII, "records"), (O.BIT_PIXEL, "values"), (O.BIT_PIXEL, "records")]

    def set_step(opts, grid_allowed):
        mirror, depth, deep, grid = opts
        if mirror:
            T._set_k(ctx, mirrors)
        else:
            T._clear_k(ctx, len(sph) + len(pl))
        ctx.set_option(R.OPT_REFLECT_DEPTH, depth)
        ctx.set_option(R.OPT_REFLECT_SHADOWS, deep)
        ctx.set_option(R.OPT_SHADOW_GRID, grid if grid_allowed else 0)

    def render(key):
        mode, form = key
        return _slab(R, ctx, p, mode, R.RENDER_VALUES if form == "values" else 0)

    # the brute reference of every option set, once, before the sequence (so that the sequence alone decides the layouts)
    ref = {}
    for opts, _, _ in LAYOUT_STEPS:
        if opts[:3] in ref:
            continue
        set_step(opts, False)
        ctx.set_option(R.OPT_SHADOW_CHECK, 1)
        ref[opts[:3]] = {key: render(key) for key in keys}
        ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    assert len(ref) == 3
    # the sequence, once per mode and form: every frame another layout
    for key in keys:
        for step, (opts, family, bytes_per_px) in enumerate(LAYOUT_STEPS):
            set_step(opts, True)
            frames0 = ctx.get_option(R.STAT_SHADOW_GRID_FRAMES)
            got = render(key)
            what = "step %d (%s, %d B/px), %s %s" % (step, family, bytes_per_px, O.MODE_NAMES[key[0]], key[1])
            assert ctx.last_kernel.split("<")[0] == family, (what, ctx.last_kernel)
            assert ctx.get_option(R.STAT_SHADOW_GRID_FRAMES) == frames0 + opts[3], what
            _assert_same({key: got}, {key: ref[opts[:3]][key]}, what)
    for opts3 in ref:  # (after the sequence: the grid is built)
        set_step(opts3 + (0,), False)
        _assert_not_empty(R, ctx, p, ref[opts3], "layout steps, mirrors %d depth %d deep %d" % opts3, render=_slab)
    T._clear_k(ctx, len(sph) + len(pl))
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. the option

def test_option_0_is_the_state_before_the_option_existed(R):
    p, sph, pl, lights = scene(R, "c", 64, 48)
    with R.Context(320, 180) as c:  # (a context the option was never set on)
        c.set_scene(sph, pl)
        c.set_option(R.OPT_SHADOWS, 1)

        def frames():
            return [(T._rows(R, c, p, mode, flags).tobytes(), c.last_kernel)
                    for mode, flags in ((O.RGB_ASCII, 0), (O.BIT_ASCII, R.RENDER_COMPACT), (O.RGB_PIXEL, R.RENDER_VALUES))]

        before = frames()
        assert all(k.startswith("rtx_shadow_shade<") for _, k in before)
        assert c.get_option(R.OPT_SHADOW_GRID) == 0 and c.get_option(R.STAT_SHADOW_GRID_FRAMES) == 0
        c.set_option(R.OPT_SHADOW_GRID, 1)
        on = frames()
        assert all(k.startswith("rtx_grid_shade<") for _, k in on) and c.get_option(R.STAT_SHADOW_GRID_FRAMES) == 3
        assert [b for b, _ in on] == [b for b, _ in before]
        c.set_option(R.OPT_SHADOW_GRID, 0)
        assert frames() == before
        assert c.get_option(R.STAT_SHADOW_GRID_FRAMES) == 3


def test_the_value_2_is_refused_and_the_option_keeps_its_value(R, ctx):
    _reset(R, ctx)
    for start in (0, 1):
        ctx.set_option(R.OPT_SHADOW_GRID, start)
        for bad in (2, -1):
            with pytest.raises(R.RtxError) as e:
                ctx.set_option(R.OPT_SHADOW_GRID, bad)
            assert e.value.status == R.ERR_INVALID_ARGUMENT
            assert ctx.get_option(R.OPT_SHADOW_GRID) == start
    for stat in (R.STAT_SHADOW_GRID_FRAMES, R.STAT_SHADOW_GRID_FALLBACK_POINTS):
        with pytest.raises(R.RtxError):
            ctx.set_option(stat, 0)  # (a counter is read-only)
    _reset(R, ctx)


def test_where_it_has_no_effect_the_launches_are_todays(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "c", 64, 48)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    frames0 = ctx.get_option(R.STAT_SHADOW_GRID_FRAMES)
    # checks 1 and 2 stay the brute reference and the all-lit frame
    for check in (1, 2):
        ctx.set_option(R.OPT_SHADOW_CHECK, check)
        with_opt = T._rows(R, ctx, p, O.RGB_ASCII)
        assert ctx.last_kernel.startswith("rtx_shadow_shade<"), ctx.last_kernel
        ctx.set_option(R.OPT_SHADOW_GRID, 0)
        assert np.array_equal(T._rows(R, ctx, p, O.RGB_ASCII), with_opt)
        ctx.set_option(R.OPT_SHADOW_GRID, 1)
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    # shadows off
    ctx.set_option(R.OPT_SHADOWS, 0)
    T._rows(R, ctx, p, O.RGB_ASCII)
    assert "grid" not in ctx.last_kernel and "shadow" not in ctx.last_kernel, ctx.last_kernel
    ctx.set_option(R.OPT_SHADOWS, 1)
    # a scene without spheres
    ctx.set_scene(NO_PLANES[:, :7], pl)
    with_opt = T._rows(R, ctx, p, O.RGB_ASCII)
    assert ctx.last_kernel.startswith("rtx_shadow_shade<"), ctx.last_kernel
    ctx.set_option(R.OPT_SHADOW_GRID, 0)
    assert np.array_equal(T._rows(R, ctx, p, O.RGB_ASCII), with_opt)
    assert ctx.get_option(R.STAT_SHADOW_GRID_FRAMES) == frames0
    _reset(R, ctx)


# ---------------------------------------------------------------- 3. the grid is the queries' own

def _some_rays(R, sph):
    rng = np.random.default_rng(3)
    n = 4096
    o = np.array([0, 0, 100]) + rng.uniform(-1, 1, (n, 3)) * np.array([40, 30, 60])
    d = rng.normal(size=(n, 3))
    return R.make_rays(o.astype(np.float32), d.astype(np.float32))


def test_a_physics_step_rebuilds_once_and_queries_share_the_grid(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "c", 64, 48)
    for i in range(0, len(sph), 2):
        ctx.set_sphere_motion(i, 1, 3.0)
    rays = _some_rays(R, sph)
    before = ctx.query_rays(rays).tobytes()
    builds = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    got, _ = _on(R, ctx, p, modes=[O.RGB_ASCII])
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds, "a frame on the grid the query built rebuilt it"
    assert ctx.query_rays(rays).tobytes() == before
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds
    ref, _ = _reference(R, ctx, p, modes=[O.RGB_ASCII])
    _assert_same(got, ref, "before the step")
    # a step: the next frame rebuilds, once, and is the reference's
    ctx.update_objects(0.2)
    moved, _ = _on(R, ctx, p, modes=[O.RGB_ASCII])
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
    ref2, _ = _reference(R, ctx, p, modes=[O.RGB_ASCII])
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
    _assert_same(moved, ref2, "after a physics step")
    assert not np.array_equal(ref2[(O.RGB_ASCII, "values")], ref[(O.RGB_ASCII, "values")]), "the step moved nothing"
    # ... and the query after the frame finds the grid built
    ctx.set_option(R.OPT_QUERY_CHECK, 1)
    want = ctx.query_rays(rays).tobytes()
    ctx.set_option(R.OPT_QUERY_CHECK, 0)
    assert ctx.query_rays(rays).tobytes() == want
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
    ctx.set_scene(sph, pl)
    _reset(R, ctx)


def test_frames_in_flight_on_three_streams_share_the_grid_across_rebuilds(R, ctx):
    """Six frames a round, queued round-robin on three streams without a wait between them, a physics step between rounds: every
    round rebuilds the grid once -- behind the other streams' frames of the round before -- and every frame is the brute path's."""
    import torch
    _reset(R, ctx)
    W, H = 64, 48
    p, sph, pl = _load(R, ctx, "c", W, H)
    for i in range(0, len(sph), 2):
        ctx.set_sphere_motion(i, 1, 3.0)
    streams = [torch.cuda.Stream() for _ in range(3)]
    kinds = [(O.RGB_ASCII, 0), (O.BIT_PIXEL, 0)]  # (frame i: stream i % 3, kind i % 2 -- every stream renders both)
    builds = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    frames = ctx.get_option(R.STAT_SHADOW_GRID_FRAMES)
    previous = None
    for rnd in range(4):
        bufs = [torch.full((W * H * (20 if kinds[i % 2][0] >= O.RGB_ASCII else 12),), 0xEE, dtype=torch.uint8, device="cuda") for i in range(6)]
        torch.cuda.synchronize()
        ctx.set_option(R.OPT_SHADOW_GRID, 1)
        for i, buf in enumerate(bufs):
            mode, flags = kinds[i % 2]
            ctx.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=streams[i % 3].cuda_stream, flags=flags)
            assert ctx.last_kernel.startswith("rtx_grid_"), ctx.last_kernel
        torch.cuda.synchronize()
        ctx.set_option(R.OPT_SHADOW_GRID, 0)
        assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + rnd + 1
        assert ctx.get_option(R.STAT_SHADOW_GRID_FRAMES) == frames + 6 * (rnd + 1)
        ref, _ = _reference(R, ctx, p, modes=[m for m, _ in kinds], forms=["records"])
        for i, buf in enumerate(bufs):
            mode = kinds[i % 2][0]
            want = ref[(mode, "records")]
            assert np.array_equal(buf.cpu().numpy(), want), "round %d, frame %d (stream %d, %s): %s" % (
                rnd, i, i % 3, O.MODE_NAMES[mode], U.first_diff(buf.cpu().numpy(), want, 20 if mode >= O.RGB_ASCII else 12, 1 << 30))
        if previous is not None:
            assert not np.array_equal(ref[(O.RGB_ASCII, "records")], previous), "the step moved nothing"
        previous = ref[(O.RGB_ASCII, "records")]
        if rnd < 3:
            ctx.update_objects(0.2)
    ctx.set_scene(sph, pl)
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. slabs, ranks, graphs

def test_ragged_slabs_equal_the_frame(R, ctx):
    import torch
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "e", 64, 48)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.set_option(R.OPT_REFLECT_SHADOWS, 1)
    W, H = 64, 48
    ref, _ = _reference(R, ctx, p, modes=[O.RGB_ASCII, O.BIT_PIXEL], forms=["records", "compact"])
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    for (mode, form), want in ref.items():
        flags = R.RENDER_COMPACT if form == "compact" else 0
        S = 4 if form == "compact" else (20 if mode >= O.RGB_ASCII else 12)
        parts = []
        for r0, r1 in ((0, 17), (17, 18), (18, 48)):
            buf = torch.full(((r1 - r0) * W * S,), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.render_rows(p, mode, r0, r1 - r0, d_out=buf.data_ptr(), out_row_base=r0, flags=flags)
            ctx.synchronize()
            assert ctx.last_kernel.startswith("rtx_grid_chain_shadow_shade<"), ctx.last_kernel
            parts.append(buf.cpu().numpy())
        assert np.array_equal(np.concatenate(parts), want), (mode, form)
    _reset(R, ctx)


def test_three_logical_ranks_equal_the_reference(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "c", 64, 48)
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    want = [ctx.render_to_host(p, m).copy() for m in (O.BIT_ASCII, O.RGB_ASCII)]
    ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    with R.Context(64, 48, devices=[0, 0, 0]) as g:
        g.set_scene(sph, pl)
        g.set_option(R.OPT_SHADOWS, 1)
        g.set_option(R.OPT_SHADOW_GRID, 1)
        assert g.get_option(R.OPT_SHADOW_GRID) == 1
        with pytest.raises(R.RtxError):
            g.set_option(R.OPT_SHADOW_GRID, 2)
        assert [g.member_option(r, R.OPT_SHADOW_GRID) for r in range(3)] == [1, 1, 1]
        got = [g.render_to_host(p, m).copy() for m in (O.BIT_ASCII, O.RGB_ASCII)]
        assert all(g.member_kernel(r).startswith("rtx_grid_shade<") for r in range(3)), [g.member_kernel(r) for r in range(3)]
        assert [g.member_option(r, R.STAT_QUERY_GRID_BUILDS) for r in range(3)] == [1, 1, 1]  # every member builds its own grid
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    _reset(R, ctx)


def test_a_capture_refuses_the_grid_path_and_the_context_goes_on(R, ctx):
    import torch
    _reset(R, ctx)
    p, sph, pl = _load(R, ctx, "c", 64, 48)
    W, H = 64, 48
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    want = T._rows(R, ctx, p, O.RGB_ASCII)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(s.cuda_stream)
    with pytest.raises(R.RtxError) as e:
        ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
    # the capture goes on: with the option off the same call is recorded
    ctx.set_option(R.OPT_SHADOW_GRID, 0)
    ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want)
    finally:
        ctx.graph_destroy(g)
    ctx.set_option(R.OPT_SHADOW_GRID, 1)
    assert np.array_equal(T._rows(R, ctx, p, O.RGB_ASCII), want)
    assert ctx.last_kernel.startswith("rtx_grid_shade<")
    _reset(R, ctx)
