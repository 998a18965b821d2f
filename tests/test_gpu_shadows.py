"""The settable light and hard shadows (rtx_scene_set_light, RTX_OPT_SHADOWS): the reference has one constant light and no
shadows (RayTracing.cu:132,143-157), so the oracles here are the library's own frames and a float64 classifier:
  * the default state launches today's kernels: the committed goldens hold and no two-launch frame is counted;
  * the two-launch path with no shadow test (RTX_OPT_SHADOW_CHECK 2) reproduces the one-launch kernels byte for byte;
  * with shadows on every pixel is the lit record (shadows off) or the dark one (both powers 0, shadows off), and which one
    agrees with a float64 evaluation of the shadow rule outside a narrow tolerance band;
  * the culled shadow pass equals the brute one (RTX_OPT_SHADOW_CHECK 1), and every entry point agrees with the plain render."""
import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

MODES = [O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL]


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(7680, 4320)  # (C4)
    yield c
    c.close()


def _reset(R, c):
    c.set_option(R.OPT_SHADOWS, 0)
    c.set_option(R.OPT_SHADOW_CHECK, 0)
    c.set_option(R.OPT_KERNEL, R.KERNEL_AUTO)
    c.set_option(R.OPT_REFINE, -1)
    c.set_option(R.OPT_TWO_LEVEL, -1)
    c.set_option(R.OPT_BATCH, -1)
    c.set_light(None)


def _rows(R, c, p, mode, flags=0, S=None):
    """The whole frame through rtx_render_rows into a caller buffer (records, pixel words or values)."""
    import torch
    W, H = int(p.x), int(p.y)
    if S is None:
        S = 32 if flags & R.RENDER_VALUES else (4 if flags & R.RENDER_COMPACT else (20 if mode >= O.RGB_ASCII else 12))
    buf = torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fill is queued on torch's stream; the library renders on its own)
    c.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, flags=flags)
    c.synchronize()
    return buf.cpu().numpy()


DIRECTED_LIGHT = (0.0, 50.0, 40.0)


def directed_scene(n_small=0):
    """A large sphere above a plane, under the light DIRECTED_LIGHT: its shadow falls on the plane in front of the camera (about 10 %
    of the pixels of directed_params' view).  n_small spheres far to the side, out of every shadow ray's way, give the culling
    something to cull."""
    sph = [[0.0, 8.0, 40.0, 10.0, 200.0, 40.0, 40.0]]
    rng = np.random.default_rng(7)
    for _ in range(n_small):
        sph.append([float(rng.uniform(300, 500)), float(rng.uniform(-20, 20)), float(rng.uniform(100, 300)), 0.5, 50.0, 200.0, 50.0])
    pl = [[0.0, -3.0, 30.0, 0.0, 1.0, 0.0, 120.0, 120.0, 120.0, 80.0, 80.0]]
    return np.array(sph, dtype=np.float32), np.array(pl, dtype=np.float32)


def directed_params(R, W=320, H=180):
    return R.camera_params(W, H, pos=(0.0, 10.0, 0.0), rot=(0.4, float(np.float32(np.pi)), 0.0))


# ---------------------------------------------------------------- 1. default state: today's kernels

@pytest.mark.parametrize("explicit", [False, True])
def test_default_state_keeps_golden_hashes_and_launches(R, ctx, explicit):
    _reset(R, ctx)
    ctx.set_light(R.make_light() if explicit else None)
    gold = U.load_golden()
    for name in ("C1", "C2", "C3", "C4", "C5"):
        p, sph, pl = R.config_inputs(name)
        ctx.set_scene(sph, pl)
        modes = range(5) if name == "C1" else [O.RGB_ASCII]
        for mode in modes:
            key = "%s_%s" % (name, O.MODE_NAMES[mode])
            if key not in gold:
                continue
            got = ctx.render_to_host(p, mode)
            assert O.fnv1a64(got) == gold[key]["frame_fnv1a64"], key
            assert "shadow" not in ctx.last_kernel and "hits" not in ctx.last_kernel
    assert ctx.get_option(R.STAT_SHADOW_FRAMES) == 0


# ---------------------------------------------------------------- 2. two launches, nothing shadowed: bit for bit

@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
@pytest.mark.parametrize("kernel", ["brute", "binned", "refine"])
def test_two_launch_path_lit_equals_one_launch(R, ctx, name, kernel):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ctx.set_option(R.OPT_KERNEL, R.KERNEL_BRUTE if kernel == "brute" else R.KERNEL_BINNED)
    ctx.set_option(R.OPT_REFINE, 1 if kernel == "refine" else -1)
    modes = MODES if name != "C3" else [O.RGB_ASCII]
    for mode in modes:
        for flags in (0, R.RENDER_COMPACT, R.RENDER_VALUES):
            ctx.set_option(R.OPT_SHADOWS, 0)
            want = _rows(R, ctx, p, mode, flags)
            before = ctx.get_option(R.STAT_SHADOW_FRAMES)
            ctx.set_option(R.OPT_SHADOWS, 1)
            ctx.set_option(R.OPT_SHADOW_CHECK, 2)
            got = _rows(R, ctx, p, mode, flags)
            ctx.set_option(R.OPT_SHADOW_CHECK, 0)
            assert ctx.get_option(R.STAT_SHADOW_FRAMES) == before + 1
            assert "rtx_shadow_shade" in ctx.last_kernel
            assert np.array_equal(got, want), "%s %s %s flags %d: %s" % (name, kernel, O.MODE_NAMES[mode], flags,
                                                                        U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))


def _slabs(R, c, p, mode, n, flags=0):
    """The frame as n row slabs, one rtx_render_rows call each into its own buffer, concatenated."""
    import torch
    W, H = int(p.x), int(p.y)
    S = 4 if flags & R.RENDER_COMPACT else (20 if mode >= O.RGB_ASCII else 12)
    out = []
    for k in range(n):
        r0, r1 = H * k // n, H * (k + 1) // n
        buf = torch.full(((r1 - r0) * W * S,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.render_rows(p, mode, r0, r1 - r0, d_out=buf.data_ptr(), out_row_base=r0, flags=flags)
        c.synchronize()
        out.append(buf.cpu().numpy())
    return np.concatenate(out)


@pytest.mark.parametrize("name,slabs", [("C5", 1), ("C4", 8)])
def test_two_launch_path_lit_equals_one_launch_large_configs(R, ctx, name, slabs):
    """C5 (two-level pre-pass and per-wave refinement in the closest-hit form) and C4 as 8 slabs, with the library's own plan."""
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    for flags in (0, R.RENDER_COMPACT):
        ctx.set_option(R.OPT_SHADOWS, 0)
        want = _slabs(R, ctx, p, O.RGB_ASCII, slabs, flags)
        if flags == 0 and slabs == 1:
            assert O.fnv1a64(want[:20 * int(p.x) * int(p.y)]) == U.load_golden()["%s_RGB_ASCII" % name]["frame_fnv1a64"]
        ctx.set_option(R.OPT_SHADOWS, 1)
        ctx.set_option(R.OPT_SHADOW_CHECK, 2)
        got = _slabs(R, ctx, p, O.RGB_ASCII, slabs, flags)
        ctx.set_option(R.OPT_SHADOW_CHECK, 0)
        assert "rtx_shadow_shade" in ctx.last_kernel
        assert np.array_equal(got, want), "%s flags %d: %s" % (name, flags, U.first_diff(got, want, 20, int(p.x)))


# ---------------------------------------------------------------- 3. shadows on: lit or dark, as a float64 classifier says

def _rays64(p):
    """Primary ray directions in float64 (RayTracing.cu:16-23)."""
    W, H = int(p.x), int(p.y)
    M = np.array(p.inv_v[:], dtype=np.float64).reshape(4, 4)
    cols = np.arange(W, dtype=np.float64)
    rows = np.arange(H, dtype=np.float64)
    vx = ((2 * cols - W) / W) * p.element1
    vy = ((H - 2 * rows) / H) * p.element2
    VX, VY = np.meshgrid(vx, vy)
    d = np.stack([M[k, 0] * VX + M[k, 1] * VY + M[k, 2] for k in range(3)], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def classify64(p, sph, pl, values, light_pos, pix, rel=1e-5):
    """For the pixels `pix` (flat indices): 1 shadowed, 0 lit, -1 ambiguous (within the tolerance band of some test), -2 not a
    visible hit."""
    W, H = int(p.x), int(p.y)
    v = values.view(np.float32).reshape(H * W, 8)[pix].astype(np.float64)
    t, N = v[:, 0], v[:, 2:5]
    vis = (t <= p.cam_far) & (pix % W != W - 1)
    o = np.array(p.cam_pos[:], dtype=np.float64)
    P = o + _rays64(p).reshape(H * W, 3)[pix] * np.where(vis, t, 0.0)[:, None]
    L = np.array(light_pos, dtype=np.float64)
    toL = L - P
    seg = np.linalg.norm(toL, axis=-1)
    scale = seg + 1e-9
    out = np.zeros(len(pix), dtype=np.int64)
    s_self = np.einsum("nk,nk->n", N, toL)
    shadow = s_self <= 0
    amb = np.abs(s_self) < rel * scale
    # the hit object, excluded from its own test: the one whose surface P lies nearest (fp32 hit points of small, distant spheres
    # can sit well off the surface); ambiguous when a second surface is about as near
    sph64, pl64 = sph.astype(np.float64), pl.astype(np.float64)
    sd = [np.abs(np.linalg.norm(P - c[:3], axis=-1) - c[3]) for c in sph64] + [np.abs((P - q[:3]) @ q[3:6]) for q in pl64]
    sd = np.stack(sd) if sd else np.full((1, len(pix)), np.inf)
    order = np.argsort(sd, axis=0)
    owner = order[0]
    if sd.shape[0] > 1:
        d1, d2 = np.take_along_axis(sd, order[:1], 0)[0], np.take_along_axis(sd, order[1:2], 0)[0]
        amb |= d2 < 2.0 * d1 + 1e-6 * (1.0 + np.abs(P).sum(-1))
    for j, c in enumerate(sph64):
        C, r = c[:3], c[3]
        w = C - P
        own = owner == j
        s = np.clip(np.einsum("nk,nk->n", w, toL) / np.maximum(seg * seg, 1e-300), 0, 1)
        dist = np.linalg.norm(w - toL * s[:, None], axis=-1)
        shadow |= (dist < r) & ~own
        amb |= (np.abs(dist - r) < rel * scale + 1e-4 * r) & ~own
    for j, q in enumerate(pl64):
        pp, n, w_, h_ = q[:3], q[3:6], q[9], q[10]
        own = owner == len(sph64) + j
        sP = (P - pp) @ n
        sL = float(np.dot(L - pp, n))
        cross = (sP * sL < 0) & ~own
        f = np.where(cross, sP / np.where(cross, sP - sL, 1.0), 0.0)
        X = P + toL * f[:, None]
        inside = (X[:, 0] > pp[0] - w_ / 2) & (X[:, 0] < pp[0] + w_ / 2) & (X[:, 2] > pp[2] - h_ / 2) & (X[:, 2] < pp[2] + h_ / 2)
        shadow |= cross & inside
        edge = np.minimum.reduce([np.abs(X[:, 0] - (pp[0] - w_ / 2)), np.abs(X[:, 0] - (pp[0] + w_ / 2)),
                                  np.abs(X[:, 2] - (pp[2] - h_ / 2)), np.abs(X[:, 2] - (pp[2] + h_ / 2))])
        amb |= cross & (edge < rel * scale)
        amb |= (np.abs(sP) < rel * scale) & ~own
    out[shadow] = 1
    out[amb] = -1
    out[~vis] = -2
    return out


def _check_lit_or_dark(R, c, p, sph, pl, mode, min_shadow=0.0):
    W, H = int(p.x), int(p.y)
    S = 20 if mode >= O.RGB_ASCII else 12
    light = c.get_light()
    c.set_option(R.OPT_SHADOWS, 0)
    lit = _rows(R, c, p, mode).reshape(H, W, S)
    values = _rows(R, c, p, mode, R.RENDER_VALUES)
    c.set_light(R.make_light(pos=tuple(light.pos), diffuse_rgb=tuple(light.diffuse_rgb), diffuse_power=0.0,
                             specular_rgb=tuple(light.specular_rgb), specular_power=0.0))
    dark = _rows(R, c, p, mode).reshape(H, W, S)
    c.set_light(light)
    c.set_option(R.OPT_SHADOWS, 1)
    got = _rows(R, c, p, mode).reshape(H, W, S)
    is_lit = (got == lit).all(-1)
    is_dark = (got == dark).all(-1)
    assert (is_lit | is_dark).all(), "pixels that are neither the lit nor the dark record: %d" % int((~(is_lit | is_dark)).sum())
    # every pixel of a small frame; a fixed-seed sample of 40 000 of a large one (the classifier is float64 numpy over all objects)
    pix = np.arange(W * H) if W * H <= 60000 else np.sort(np.random.default_rng(11).choice(W * H, 40000, replace=False))
    cls = classify64(p, sph, pl, values, tuple(light.pos), pix)
    is_lit, is_dark = is_lit.reshape(-1)[pix], is_dark.reshape(-1)[pix]
    differ = ~(lit == dark).all(-1).reshape(-1)[pix]
    decided = differ & (cls >= 0)
    wrong = decided & ((cls == 1) != (is_dark & ~is_lit))
    assert int(wrong.sum()) == 0, "pixels classified against the float64 rule: %d of %d (first: %s)" % (
        int(wrong.sum()), int(decided.sum()), pix[wrong][:5])
    ambiguous = differ & (cls == -1)
    assert ambiguous.sum() < 0.001 * len(pix), "ambiguous pixels: %d of %d" % (int(ambiguous.sum()), len(pix))
    if min_shadow:
        assert (cls == 1).sum() >= min_shadow * len(pix)  # (shadowed by the rule, whether or not the record shows it)
    return got


@pytest.mark.parametrize("mode", MODES)
def test_shadows_lit_or_dark_directed_scene(R, ctx, mode):
    _reset(R, ctx)
    sph, pl = directed_scene()
    ctx.set_scene(sph, pl)
    ctx.set_light(R.make_light(pos=DIRECTED_LIGHT))
    _check_lit_or_dark(R, ctx, directed_params(R), sph, pl, mode, min_shadow=0.05)


@pytest.mark.parametrize("which", ["C1", "C2", "default"])
def test_shadows_lit_or_dark_configs(R, ctx, which):
    _reset(R, ctx)
    if which == "default":
        ctx.set_reference_default_scene()
        p = R.camera_params(400, 150)
        sph = np.array([[0, 10, 20, 7, 255, 1, 1], [5, 10, 20, 6, 1, 255, 1], [10, 10, 40, 10, 1, 1, 255], [5, 10, 20, 3, 225, 210, 20],
                        [-5, 10, 40, 4, 225, 10, 220]], dtype=np.float32)
        pl = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 10, 20]], dtype=np.float32)
    else:
        p, sph, pl = R.config_inputs(which)
        ctx.set_scene(sph, pl)
    _check_lit_or_dark(R, ctx, p, sph, pl, O.RGB_ASCII)
    # a moved light, coloured
    ctx.set_light(R.make_light(pos=(-20.0, 80.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=2500.0))
    _check_lit_or_dark(R, ctx, p, sph, pl, O.BIT_ASCII)


@pytest.mark.parametrize("check", [0, 1])
def test_list_refills_keep_records_exact(R, ctx, check):
    """3 001 spheres: the brute pass (every sphere a candidate) refills the 1 024-entry LDS list three times per workgroup, the
    culled one walks six steps.  Every record must still be the lit or the dark one (a list overrunning its LDS array would
    corrupt the glyph and digit tables next to it) and agree with the float64 rule."""
    _reset(R, ctx)
    sph, pl = directed_scene(n_small=3000)
    ctx.set_scene(sph, pl)
    ctx.set_light(R.make_light(pos=DIRECTED_LIGHT))
    ctx.set_option(R.OPT_SHADOW_CHECK, check)
    _check_lit_or_dark(R, ctx, directed_params(R), sph, pl, O.RGB_ASCII if check else O.BIT_ASCII, min_shadow=0.05)
    _reset(R, ctx)


def test_physics_steps_keep_the_rule(R, ctx):
    _reset(R, ctx)
    sph, pl = directed_scene()
    ctx.set_scene(sph, pl)
    ctx.set_light(R.make_light(pos=DIRECTED_LIGHT))
    p = directed_params(R)
    for _ in range(3):
        ctx.update_objects(0.05)
        ctx.synchronize()
        cur = np.array([ctx.get_object(0)[1][:4]], dtype=np.float32)
        cur = np.concatenate([cur, sph[:, 4:7]], axis=1)
        _check_lit_or_dark(R, ctx, p, cur, pl, O.RGB_ASCII)


# ---------------------------------------------------------------- 4. culled == brute

@pytest.mark.parametrize("seed,n", [(1, 300), (2, 1500), (3, 3000), (4, 40)])
def test_culled_equals_brute(R, ctx, seed, n):
    _reset(R, ctx)
    p = R.camera_params(480, 270, pos=(0.3 * seed, 2.0, -5.0), rot=(0.1, float(np.float32(np.pi)), 0.0))
    sph, pl = R.synth_scene(seed, n, 1 + seed % 3, p.element1, p.element2)
    ctx.set_scene(sph, pl)
    ctx.set_light(R.make_light(pos=(10.0 * seed, 60.0, 40.0)))
    ctx.set_option(R.OPT_SHADOWS, 1)
    for mode in (O.RGB_ASCII, O.BIT_PIXEL):
        culled = _rows(R, ctx, p, mode)
        ctx.set_option(R.OPT_SHADOW_CHECK, 1)
        brute = _rows(R, ctx, p, mode)
        ctx.set_option(R.OPT_SHADOW_CHECK, 0)
        assert np.array_equal(culled, brute), U.first_diff(culled, brute, 20 if mode >= 2 else 12, int(p.x))


def _fuzz_case(R, seed, W=480, H=270):
    """A camera, scene and light from seed: fuzz_cases' scenes (spheres large and far, tiny, around and behind the camera,
    containing it; up to 20 planes) under a light somewhere around them."""
    import fuzz_cases as F
    g = np.random.default_rng(seed)
    pos = [float(v) for v in g.uniform(-30, 30, 3)]
    p = R.camera_params(W, H, pos, (0.0, float(np.pi), 0.0))
    M = F.general_matrix(g)
    F._set_matrix(p, M)
    sph, pl = F.scene(g, p, F._matrix_of(p), pos, W, H, 12000)
    light = [float(v) for v in np.asarray(pos) + g.uniform(-80, 80, 3)]
    return p, sph, pl, light


def _fuzz_seeds(R):
    """A fixed share of the fuzz cases: the first three seeds with at least 2048 spheres (where the trace plans two-level
    lists) and the first three with fewer."""
    big, small = [], []
    for seed in range(1000, 1200):
        n = len(_fuzz_case(R, seed, 16, 16)[1])
        (big if n >= 2048 else small).append(seed)
        if len(big) >= 3 and len(small) >= 3:
            break
    return big[:3] + small[:3]


def test_culled_equals_brute_over_fuzz_cases(R, ctx):
    _reset(R, ctx)
    seeds = _fuzz_seeds(R)
    assert len(seeds) == 6
    for seed in seeds:
        p, sph, pl, light = _fuzz_case(R, seed)
        ctx.set_scene(sph, pl)
        ctx.set_light(R.make_light(pos=tuple(light)))
        ctx.set_option(R.OPT_SHADOWS, 1)
        for mode in (O.RGB_ASCII, O.BIT_ASCII):
            ctx.set_option(R.OPT_SHADOW_CHECK, 0)
            culled = _rows(R, ctx, p, mode)
            ctx.set_option(R.OPT_SHADOW_CHECK, 1)
            brute = _rows(R, ctx, p, mode)
            assert np.array_equal(culled, brute), "seed %d (%d spheres, %d planes) %s: %s" % (
                seed, len(sph), len(pl), O.MODE_NAMES[mode], U.first_diff(culled, brute, 20 if mode >= 2 else 12, int(p.x)))
        ctx.set_option(R.OPT_SHADOW_CHECK, 0)
    _reset(R, ctx)


def test_directed_scene_culls_the_far_spheres(R, ctx):
    _reset(R, ctx)
    sph, pl = directed_scene(n_small=3000)
    ctx.set_scene(sph, pl)
    ctx.set_light(R.make_light(pos=DIRECTED_LIGHT))
    p = directed_params(R)
    ctx.set_option(R.OPT_SHADOWS, 1)
    culled = _rows(R, ctx, p, O.RGB_ASCII)
    longest = ctx.get_option(R.STAT_SHADOW_LONGEST_LIST)
    # the small spheres sit at x >= 300, far beyond every segment from the light (x = 0) to the hit points around the big sphere
    # and on the plane (|x| <= 40): the cones of those tiles list the big sphere alone
    assert longest < 0.1 * len(sph), longest
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = _rows(R, ctx, p, O.RGB_ASCII)
    assert ctx.get_option(R.STAT_SHADOW_LONGEST_LIST) == len(sph)
    assert np.array_equal(culled, brute)


# ---------------------------------------------------------------- 5. every entry point agrees

def _shadow_setup(R, c, name="C1"):
    p, sph, pl = R.config_inputs(name)
    c.set_scene(sph, pl)
    c.set_light(R.make_light(pos=(5.0, 40.0, 10.0)))
    c.set_option(R.OPT_SHADOWS, 1)
    return p


def test_update_equals_minimized_render(R, ctx):
    import torch
    _reset(R, ctx)
    p = _shadow_setup(R, ctx)
    W, H = int(p.x), int(p.y)
    for mode in MODES:
        rec = torch.from_numpy(_rows(R, ctx, p, mode, S=20)).cuda()
        out = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n2 = ctx.minimize(mode, W, H, d_in=rec.data_ptr(), d_out=out.data_ptr())
        want = out[:n2].cpu().numpy()
        for words, host_write in ((1, -1), (0, 0), (1, 1)):
            ctx.set_option(R.OPT_UPDATE_WORDS, words)
            ctx.set_option(R.OPT_UPDATE_HOST_WRITE, host_write)
            got = np.array(ctx.update(p, mode))
            assert np.array_equal(got, want), "Update words=%d host_write=%d mode %s" % (words, host_write, O.MODE_NAMES[mode])
    ctx.set_option(R.OPT_UPDATE_WORDS, -1)
    ctx.set_option(R.OPT_UPDATE_HOST_WRITE, -1)


def test_pipelined_updates_equal_blocking(R, ctx):
    _reset(R, ctx)
    p0 = _shadow_setup(R, ctx)
    W, H = int(p0.x), int(p0.y)
    cams = [R.camera_params(W, H, pos=(0.5 * i, 0.2 * i, 0.0)) for i in range(4)]
    want = [np.array(ctx.update(c, O.RGB_ASCII)).copy() for c in cams]
    bufs = [ctx.host_alloc(20 * W * H) for _ in range(2)]  # (pointer, numpy view) pairs
    try:
        got = []
        t = [ctx.update_begin(cams[0], O.RGB_ASCII, bufs[0][0])]
        for i in range(1, 4):
            t.append(ctx.update_begin(cams[i], O.RGB_ASCII, bufs[i % 2][0]))
            n = ctx.update_end(t[i - 1])
            got.append(bufs[(i - 1) % 2][1][:n].copy())
        n = ctx.update_end(t[3])
        got.append(bufs[1][1][:n].copy())
    finally:
        for b in bufs:
            ctx.host_free(b[0])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_submit_frames_streams_slabs_compact_and_graphs(R, ctx):
    import torch
    _reset(R, ctx)
    p0 = _shadow_setup(R, ctx, "C2")
    W, H = int(p0.x), int(p0.y)
    cams = [R.camera_params(W, H, pos=(0.4 * i, -0.2 * i, 0.1 * i)) for i in range(4)]
    want = [_rows(R, ctx, c, O.RGB_ASCII) for c in cams]
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.full((20 * W * H,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    ctx.submit_frames(cams, O.RGB_ASCII, [b.data_ptr() for b in bufs], [s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    for b, w in zip(bufs, want):
        assert np.array_equal(b.cpu().numpy(), w)
    # slabs, batched or not (the batched launch declines while the shadow path is in use)
    row0, rows = H // 3, H // 3
    st = torch.cuda.Stream()
    for batch in (-1, 0):
        ctx.set_option(R.OPT_BATCH, batch)
        sl = [torch.full((20 * W * rows,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        ctx.submit_slabs(cams, O.RGB_ASCII, row0, rows, [b.data_ptr() for b in sl], row0, [st.cuda_stream] * 4)
        torch.cuda.synchronize()
        for b, w in zip(sl, want):
            assert np.array_equal(b.cpu().numpy(), w[20 * W * row0:20 * W * (row0 + rows)])
    ctx.set_option(R.OPT_BATCH, -1)
    # compact words, expanded
    words = torch.from_numpy(_rows(R, ctx, cams[1], O.RGB_ASCII, R.RENDER_COMPACT)).cuda()
    rec = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.expand(O.RGB_ASCII, words.data_ptr(), rec.data_ptr(), [(0, 0, W * H)])
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(rec.cpu().numpy(), want[1])
    # a recorded graph keeps the light and shadows it was recorded with
    buf = torch.full((20 * W * H,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(st.cuda_stream)
    ctx.render_rows(cams[2], O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=st.cuda_stream)
    g = ctx.graph_end(st.cuda_stream)
    ctx.set_option(R.OPT_SHADOWS, 0)
    ctx.set_light(None)
    buf.fill_(0xEE)
    torch.cuda.synchronize()
    ctx.graph_launch(g, st.cuda_stream)
    torch.cuda.synchronize()
    ctx.graph_destroy(g)
    assert np.array_equal(buf.cpu().numpy(), want[2])


@pytest.mark.parametrize("ranks", [3, 8])
def test_device_group_equals_plain_context(R, ctx, ranks):
    import torch
    _reset(R, ctx)
    p = _shadow_setup(R, ctx, "C2")
    W, H = int(p.x), int(p.y)
    want = _rows(R, ctx, p, O.RGB_ASCII)
    want_stream = np.array(ctx.update(p, O.RGB_ASCII)).copy()
    with R.Context(W, H, devices=[0] * ranks) as g:
        _shadow_setup(R, g, "C2")
        assert g.member_option(ranks - 1, R.OPT_SHADOWS) == 1
        for wire in (R.WIRE_COMPACT, R.WIRE_RECORDS):
            g.set_option(R.OPT_GROUP_WIRE, wire)
            got = g.render_to_host(p, O.RGB_ASCII)
            assert np.array_equal(got, want)
        for direct in (0, 1):
            g.set_option(R.OPT_GROUP_UPDATE, direct)
            assert np.array_equal(np.array(g.update(p, O.RGB_ASCII)), want_stream)
        assert g.member_option(ranks - 1, R.STAT_SHADOW_FRAMES) > 0


# ---------------------------------------------------------------- 7. the light API

def test_light_api(R, ctx):
    _reset(R, ctx)
    l = ctx.get_light()
    assert list(l.pos) == [1.0, 50.0, 0.0] and l.diffuse_power == 2000.0 and l.specular_power == 3000.0
    ctx.set_light(R.make_light(pos=(3.0, 4.0, 5.0), diffuse_rgb=(0.5, 0.25, 1.0), diffuse_power=10.0, specular_rgb=(0.0, 1.0, 2.0), specular_power=7.0))
    l = ctx.get_light()
    assert list(l.pos) == [3.0, 4.0, 5.0] and list(l.diffuse_rgb) == [0.5, 0.25, 1.0] and list(l.specular_rgb) == [0.0, 1.0, 2.0]
    for bad in (dict(pos=(float("nan"), 0.0, 0.0)), dict(diffuse_power=-1.0), dict(specular_rgb=(0.0, -0.5, 0.0)), dict(diffuse_power=float("inf"))):
        with pytest.raises(R.RtxError) as e:
            ctx.set_light(R.make_light(**bad))
        assert e.value.status == R.ERR_INVALID_ARGUMENT
    assert list(ctx.get_light().pos) == [3.0, 4.0, 5.0]  # a refused light leaves the one in use
    ctx.scene_clear()
    assert list(ctx.get_light().pos) == [3.0, 4.0, 5.0]  # context state, not scene
    for opt, bad in ((R.OPT_SHADOWS, 2), (R.OPT_SHADOW_CHECK, 3), (R.OPT_SHADOWS, -1)):
        with pytest.raises(R.RtxError):
            ctx.set_option(opt, bad)
    # RGB_NORMALS and SDL ignore light and shadows
    p, sph, pl = R.config_inputs("C1")
    ctx.set_scene(sph, pl)
    ctx.set_light(None)
    want = _rows(R, ctx, p, O.RGB_NORMALS)
    ctx.set_light(R.make_light(pos=(0.0, 10.0, 0.0)))
    ctx.set_option(R.OPT_SHADOWS, 1)
    assert np.array_equal(_rows(R, ctx, p, O.RGB_NORMALS), want)
    assert np.array_equal(ctx.render_to_host(p, O.RGB_NORMALS), want)
    sdl = _rows(R, ctx, p, O.SDL, S=20)
    assert (sdl == 0xEE).all()
    _reset(R, ctx)
