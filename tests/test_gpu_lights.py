"""Several point lights (rtx_scene_set_lights): the reference has one constant light (RayTracing.cu:132,143-157), so the oracles
are the library's own one-light kernels, a numpy float32 restatement of the summed shading and the float64 shadow rule:
  1. a set of one light is rtx_scene_set_light's: the same bytes, the same kernels; the default state keeps the goldens;
  2. the several-lights kernels with one light (RTX_OPT_LIGHTS_CHECK 1) equal the one-light kernels byte for byte;
  3. the sum res = (res + diffuse_i * od) + specular_i * 1.0f over the lights in order, bit for bit;
  4. shadows per light: every pixel shows the frame of exactly one set of dark lights, the set float64 decides where it can;
  5. the culled walk equals the brute one with 2, 3 and 8 lights, and on the mirror path;
  6. every entry point agrees with rtx_render_rows under 3 lights with shadows;
  7. the API."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import util as U
from restate import _pow32, _shade_lights  # (moved to tests/restate.py)
from test_gpu_reflect import _closest, _dot, _normal, _nrm, _scene_k, _set_k, _clear_k
from test_gpu_shadows import _check_lit_or_dark, _fuzz_case, _fuzz_seeds, _rays64, directed_params, directed_scene

pytestmark = pytest.mark.gpu

MODES = [O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL]
f32 = np.float32

DEFAULT_SPH = np.array([[0, 10, 20, 7, 255, 1, 1], [5, 10, 20, 6, 1, 255, 1], [10, 10, 40, 10, 1, 1, 255], [5, 10, 20, 3, 225, 210, 20],
                        [-5, 10, 40, 4, 225, 10, 220]], dtype=np.float32)
DEFAULT_PL = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 10, 20]], dtype=np.float32)


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
    c.set_option(R.OPT_REFLECT_CHECK, 0)
    c.set_option(R.OPT_LIGHTS_CHECK, 0)
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


def _tuple(l):
    return (tuple(l.pos), tuple(l.diffuse_rgb), float(l.diffuse_power), tuple(l.specular_rgb), float(l.specular_power))


def _dark(R, l):
    """The light with both powers 0: what a pixel shadowed from it is shaded with."""
    return R.make_light(pos=tuple(l.pos), diffuse_rgb=tuple(l.diffuse_rgb), diffuse_power=0.0, specular_rgb=tuple(l.specular_rgb), specular_power=0.0)


COLOURS = [(1.0, 0.5, 0.25), (0.25, 1.0, 0.5), (0.5, 0.25, 1.0), (1.0, 1.0, 0.5), (0.75, 0.5, 1.0), (0.5, 1.0, 1.0), (1.0, 0.75, 0.75), (0.3, 0.6, 0.9)]


def _light_set(R, n, positions=None, zero=None, scale=1.0):
    """n lights with distinct colours and powers around the scene (or at `positions`); light `zero` has both powers 0."""
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / 8.0
        pos = positions[i] if positions is not None else (1.0 + 45.0 * np.sin(a), 50.0 + 4.0 * i, 20.0 - 45.0 * np.cos(a))
        dp, sp = scale * (500.0 + 170.0 * i), scale * (1400.0 - 150.0 * i)
        if zero == i:
            dp = sp = 0.0
        out.append(R.make_light(pos=tuple(float(v) for v in pos), diffuse_rgb=COLOURS[i], diffuse_power=dp,
                                specular_rgb=COLOURS[(i + 3) % 8], specular_power=sp))
    return out


SHADOW_LIGHT = dict(pos=(5.0, 40.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=2500.0)


# ---------------------------------------------------------------- 1. one light is today's

@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_set_of_one_light_is_set_light(R, ctx, name):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    for light in (R.make_light(), R.make_light(**SHADOW_LIGHT)):
        for shadows in (0, 1):
            ctx.set_option(R.OPT_SHADOWS, shadows)
            for mode in (O.RGB_ASCII, O.BIT_PIXEL):
                ctx.set_light(light)
                want = _rows(R, ctx, p, mode)
                want_kernel = ctx.last_kernel
                ctx.set_lights([light])
                assert ctx.get_option(R.STAT_LIGHTS) == 1
                got = _rows(R, ctx, p, mode)
                assert ctx.last_kernel == want_kernel and "rtx_lights_" not in ctx.last_kernel
                assert np.array_equal(got, want)
    _reset(R, ctx)


def test_default_state_keeps_golden_hashes_and_launches(R, ctx):
    _reset(R, ctx)
    ctx.set_lights([R.make_light()])
    before = ctx.get_option(R.STAT_SHADOW_FRAMES)
    gold = U.load_golden()
    for name in ("C1", "C2", "C3", "C4", "C5"):
        p, sph, pl = R.config_inputs(name)
        ctx.set_scene(sph, pl)
        for mode in (range(5) if name == "C1" else [O.RGB_ASCII]):
            key = "%s_%s" % (name, O.MODE_NAMES[mode])
            if key not in gold:
                continue
            got = ctx.render_to_host(p, mode)
            assert O.fnv1a64(got) == gold[key]["frame_fnv1a64"], key
            assert "shadow" not in ctx.last_kernel and "hits" not in ctx.last_kernel and "lights" not in ctx.last_kernel
    assert ctx.get_option(R.STAT_SHADOW_FRAMES) == before


# ---------------------------------------------------------------- 2. the new kernels with one light equal the old ones

def _check_vs_plain(R, c, render, what, kernel="rtx_lights_shade"):
    """render() with RTX_OPT_LIGHTS_CHECK 0, then 1: the same bytes, the second from the several-lights kernels."""
    c.set_option(R.OPT_LIGHTS_CHECK, 0)
    want = render()
    assert "rtx_lights_" not in c.last_kernel
    c.set_option(R.OPT_LIGHTS_CHECK, 1)
    frames = c.get_option(R.STAT_SHADOW_FRAMES) + c.get_option(R.STAT_REFLECT_FRAMES)
    got = render()
    c.set_option(R.OPT_LIGHTS_CHECK, 0)
    assert kernel in c.last_kernel, c.last_kernel
    assert c.get_option(R.STAT_SHADOW_FRAMES) + c.get_option(R.STAT_REFLECT_FRAMES) > frames
    assert np.array_equal(got, want), what


SHADOW_STATES = [(0, 0), (1, 0), (1, 1)]  # (RTX_OPT_SHADOWS, RTX_OPT_SHADOW_CHECK)


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
@pytest.mark.parametrize("kernel", ["brute", "binned", "refine"])
def test_lights_kernels_with_one_light_equal_one_light_kernels(R, ctx, name, kernel):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ctx.set_option(R.OPT_KERNEL, R.KERNEL_BRUTE if kernel == "brute" else R.KERNEL_BINNED)
    ctx.set_option(R.OPT_REFINE, 1 if kernel == "refine" else -1)
    modes = MODES if name != "C3" else [O.RGB_ASCII]
    for li, light in enumerate((None, R.make_light(**SHADOW_LIGHT))):
        ctx.set_light(light)
        for shadows, check in SHADOW_STATES:
            ctx.set_option(R.OPT_SHADOWS, shadows)
            ctx.set_option(R.OPT_SHADOW_CHECK, check)
            for mode in modes:
                for flags in (0, R.RENDER_COMPACT, R.RENDER_VALUES):
                    _check_vs_plain(R, ctx, lambda: _rows(R, ctx, p, mode, flags),
                                    "%s %s light %d shadows %d/%d %s flags %d" % (name, kernel, li, shadows, check, O.MODE_NAMES[mode], flags))
    _reset(R, ctx)


@pytest.mark.parametrize("name,slabs", [("C5", 1), ("C4", 8)])
def test_lights_kernels_with_one_light_large_configs(R, ctx, name, slabs):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ctx.set_light(R.make_light(**SHADOW_LIGHT))
    for shadows, check in SHADOW_STATES:
        ctx.set_option(R.OPT_SHADOWS, shadows)
        ctx.set_option(R.OPT_SHADOW_CHECK, check)
        for flags in (0, R.RENDER_COMPACT):
            _check_vs_plain(R, ctx, lambda: _slabs(R, ctx, p, O.RGB_ASCII, slabs, flags), "%s shadows %d/%d flags %d" % (name, shadows, check, flags))
    _reset(R, ctx)


def _c2_floor(R, c):
    _reset(R, c)
    p, sph, pl = R.config_inputs("C2")
    c.set_scene(sph, pl)
    ks = _scene_k("C2", sph, pl, "floor+quarter")
    _set_k(c, ks)
    return p, sph, pl, ks


def test_lights_kernels_with_one_light_on_the_mirror_path(R, ctx):
    p, sph, pl, ks = _c2_floor(R, ctx)
    try:
        for li, light in enumerate((None, R.make_light(**SHADOW_LIGHT))):
            ctx.set_light(light)
            for shadows, check in SHADOW_STATES:
                ctx.set_option(R.OPT_SHADOWS, shadows)
                ctx.set_option(R.OPT_SHADOW_CHECK, check)
                for mode in MODES:
                    for flags in (0, R.RENDER_COMPACT, R.RENDER_VALUES):
                        _check_vs_plain(R, ctx, lambda: _rows(R, ctx, p, mode, flags),
                                        "mirror light %d shadows %d/%d %s flags %d" % (li, shadows, check, O.MODE_NAMES[mode], flags),
                                        kernel="rtx_lights_reflect_shade")
    finally:
        _clear_k(ctx, len(sph) + len(pl))
        _reset(R, ctx)


# ---------------------------------------------------------------- 3. the sum, bit for bit

def restate(p, sph, pl, lights, pix, ks=None):
    """The primary hit and the colour of the pixels `pix` (flat indices) under `lights`, shadows off; with ks ({creation index: k})
    the mirror blend of tests/test_gpu_reflect.py::restate on top, the secondary hit shaded by the same sum."""
    W, H = int(p.x), int(p.y)
    col, row = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
    m = np.array(p.inv_v[:], dtype=np.float32)
    fW, fH = f32(W), f32(H)
    vx = (((f32(2.0) * col) - fW) / fW) * f32(p.element1)
    vy = ((fH - row * f32(2.0)) / fH) * f32(p.element2)
    w = [((m[4 * k] * vx + m[4 * k + 1] * vy) + m[4 * k + 2]) + m[4 * k + 3] * f32(0.0) for k in range(3)]
    D = _nrm(*w)
    n = len(pix)
    O3 = tuple(np.full(n, f32(p.cam_pos[k]), dtype=np.float32) for k in range(3))
    a = _dot(D, D)
    t, gid = _closest(O3, D, sph, pl, a, f32(4.0) * a, f32(1.0) / (f32(2.0) * a))
    P = tuple(O3[k] + D[k] * t for k in range(3))
    normal = _normal(P, sph, pl, gid)
    odall = np.concatenate([sph[:, 4:7], pl[:, 6:9]]).astype(np.float32) / f32(255.0)
    od = odall[np.maximum(gid, 0)]
    cl = _shade_lights(O3, D, t, normal, [od[:, k] for k in range(3)], lights)
    refl = np.zeros(n, dtype=bool)
    if ks:
        kk = np.zeros(len(sph) + len(pl), dtype=np.float32)
        for i, v in ks.items():
            kk[i] = f32(v)
        k = np.where(gid >= 0, kk[np.maximum(gid, 0)], f32(0.0))
        refl = (gid >= 0) & (t <= f32(p.cam_far)) & (pix % W != W - 1) & (k > f32(0.0))
        N = _nrm(*normal)
        V = _nrm(*(D[j] * f32(-1.0) for j in range(3)))
        c = f32(2.0) * _dot(N, V)
        Rd = tuple(N[j] * c - V[j] for j in range(3))
        a2 = _dot(Rd, Rd)
        t2, g2 = _closest(P, Rd, sph, pl, a2, f32(4.0) * a2, f32(1.0) / (f32(2.0) * a2), exclude=gid)
        P2 = tuple(P[j] + Rd[j] * t2 for j in range(3))
        n2 = _normal(P2, sph, pl, g2)
        od2 = odall[np.maximum(g2, 0)]
        cr = _shade_lights(P, Rd, t2, n2, [od2[:, j] for j in range(3)], lights)
        cr = [np.where(g2 >= 0, cr[j], f32(0.0)) for j in range(3)]
        wgt = f32(1.0) - k
        for j in range(3):
            v = cl[j] * wgt + cr[j] * k
            cl[j] = np.where(refl, np.where(f32(255.0) < v, f32(255.0), v), cl[j]).astype(np.float32)
    return t, gid, refl, cl


def _check_exact(R, c, p, sph, pl, lights, pix, ks=None):
    c.set_lights(lights)
    vals = _rows(R, c, p, O.RGB_ASCII, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)[pix]
    assert "rtx_lights_" in c.last_kernel
    with np.errstate(all="ignore"):
        t, gid, refl, colour = restate(p, sph, pl, lights, pix, ks)
    vis = (gid >= 0) & (pix % int(p.x) != int(p.x) - 1)  # (column W-1 holds the row's terminator, no values)
    assert vis.sum() > 0
    assert np.array_equal(vals[vis, 0].view(np.uint32), t[vis].view(np.uint32)), "primary t differs"
    for j in range(3):
        got, want = vals[vis, 5 + j], colour[j][vis]
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, "%d lights: colour %d differs at %d pixels, e.g. got %r want %r" % (len(lights), j, bad.size, got[bad[:3]], want[bad[:3]])
    return vis, refl, colour


LIGHT_SETS = [(2, None), (2, 0), (3, 1), (8, 4)]  # (lights, which one has both powers 0)


@pytest.mark.parametrize("which", ["default", "C1", "C2"])
@pytest.mark.parametrize("n,zero", LIGHT_SETS)
def test_sum_over_lights_bit_for_bit(R, ctx, which, n, zero):
    _reset(R, ctx)
    if which == "default":
        ctx.set_reference_default_scene()
        p, sph, pl = R.camera_params(400, 150), DEFAULT_SPH, DEFAULT_PL
        pix = np.arange(400 * 150)
    else:
        p, sph, pl = R.config_inputs(which)
        ctx.set_scene(sph, pl)
        pix = np.sort(np.random.default_rng(5).choice(int(p.x) * int(p.y), size=20000, replace=False))
    # powers low enough that the sum stays below the clamp on a good part of the frame, high enough that every light shows
    lights = _light_set(R, n, zero=zero, scale=0.6 if n < 8 else 0.25)
    vis, _, colour = _check_exact(R, ctx, p, sph, pl, lights, pix)
    unclamped = np.minimum.reduce([colour[j][vis] for j in range(3)]) < f32(255.0)
    assert unclamped.sum() > 0.05 * vis.sum(), "the clamp hides the sum on most pixels: %d of %d below it" % (unclamped.sum(), vis.sum())
    # order matters: the reversed set matches its own restatement, and is a different frame
    _, _, reversed_colour = _check_exact(R, ctx, p, sph, pl, lights[::-1], pix)
    if zero is None:
        assert any((colour[j][vis].view(np.uint32) != reversed_colour[j][vis].view(np.uint32)).any() for j in range(3))
    _reset(R, ctx)


# ---------------------------------------------------------------- 4. shadows per light

def classify64(p, sph, pl, values, light_pos, pix, rel=1e-5):
    """For the pixels `pix` (flat indices): 1 shadowed, 0 lit, -1 ambiguous (within the tolerance band of some test), -2 not a
    visible hit.  (tests/test_gpu_shadows.py::classify64, copied.)"""
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


def _check_shadow_sets(R, c, p, sph, pl, lights, mode, min_share=0.0):
    """Shadows on under `lights`: every pixel's record is F_S's for some set S of dark lights, and where float64 decides every light
    the decided set is one of them.  F_S: shadows off, the lights of S with both powers 0 (a shadowed light contributes +0.0)."""
    W, H = int(p.x), int(p.y)
    S_rec = 20 if mode >= O.RGB_ASCII else 12
    nl = len(lights)
    pix = np.arange(W * H) if W * H <= 60000 else np.sort(np.random.default_rng(11).choice(W * H, 40000, replace=False))
    # the inputs, not the code under test, decide how many pixels are ambiguous: each light alone through the one-light path
    # stays under the cap tests/test_gpu_shadows.py holds one light to (and is lit or dark as float64 says)
    for l in lights:
        c.set_light(l)
        _check_lit_or_dark(R, c, p, sph, pl, mode)
        assert "rtx_lights_" not in c.last_kernel
    c.set_lights(lights)
    c.set_option(R.OPT_SHADOWS, 0)
    values = _rows(R, c, p, mode, R.RENDER_VALUES)
    frames = {}
    for bits in range(1 << nl):
        c.set_lights([_dark(R, l) if (bits >> i) & 1 else l for i, l in enumerate(lights)])
        frames[bits] = _rows(R, c, p, mode).reshape(H * W, S_rec)[pix]
    c.set_lights(lights)
    c.set_option(R.OPT_SHADOWS, 1)
    got = _rows(R, c, p, mode).reshape(H * W, S_rec)[pix]
    assert "rtx_lights_shade" in c.last_kernel
    match = {bits: (got == f).all(-1) for bits, f in frames.items()}
    some = np.logical_or.reduce(list(match.values()))
    assert some.all(), "pixels that are no F_S: %d (first: %s)" % (int((~some).sum()), pix[~some][:5])
    cls = [classify64(p, sph, pl, values, tuple(l.pos), pix) for l in lights]
    decided = np.logical_and.reduce([k >= 0 for k in cls])
    dset = sum(((k == 1).astype(np.int64) << i) for i, k in enumerate(cls))
    ok = np.zeros(len(pix), dtype=bool)
    for bits, m in match.items():
        ok |= m & (dset == bits)
    wrong = decided & ~ok
    assert int(wrong.sum()) == 0, "pixels shaded against the float64 rule: %d of %d (first: %s, decided sets %s)" % (
        int(wrong.sum()), int(decided.sum()), pix[wrong][:5], dset[wrong][:5])
    # ambiguous for at least one light, where that light shows at all (as the one-light test counts them)
    amb = np.zeros(len(pix), dtype=bool)
    for i, k in enumerate(cls):
        amb |= (k == -1) & ~(frames[0] == frames[1 << i]).all(-1)
    print("%d lights, %s: ambiguous %d of %d; shadowed from exactly one light %s, from two or more %d" % (
        nl, O.MODE_NAMES[mode], int(amb.sum()), len(pix), [int((decided & (dset == (1 << i))).sum()) for i in range(nl)],
        int((decided & (dset & (dset - 1) != 0)).sum())))
    assert amb.sum() <= 0.001 * nl * len(pix), "ambiguous pixels: %d of %d" % (int(amb.sum()), len(pix))
    if min_share:
        for i in range(nl):
            assert (decided & (dset == (1 << i))).sum() >= min_share * len(pix), "light %d alone" % i
        assert (decided & (dset & (dset - 1) != 0)).sum() >= min_share * len(pix), "two or more"


DIRECTED_LIGHTS = [(0.0, 50.0, 40.0), (-30.0, 40.0, 20.0), (30.0, 40.0, 20.0)]


@pytest.mark.parametrize("mode", [O.RGB_ASCII, O.BIT_ASCII])
def test_shadows_per_light_directed_scene(R, ctx, mode):
    _reset(R, ctx)
    sph, pl = directed_scene()
    ctx.set_scene(sph, pl)
    lights = _light_set(R, 3, positions=DIRECTED_LIGHTS)
    _check_shadow_sets(R, ctx, directed_params(R), sph, pl, lights, mode, min_share=0.01)
    _reset(R, ctx)


TWO_LIGHTS = [(5.0, 40.0, 10.0), (-20.0, 80.0, 10.0)]


@pytest.mark.parametrize("mode", [O.RGB_ASCII, O.BIT_ASCII])
def test_shadows_per_light_c1(R, ctx, mode):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C1")
    ctx.set_scene(sph, pl)
    _check_shadow_sets(R, ctx, p, sph, pl, _light_set(R, 2, positions=TWO_LIGHTS, scale=2.0), mode, min_share=0.01)
    _reset(R, ctx)


def test_shadows_per_light_c2_sample(R, ctx):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C2")
    ctx.set_scene(sph, pl)
    _check_shadow_sets(R, ctx, p, sph, pl, _light_set(R, 2, positions=TWO_LIGHTS, scale=2.0), O.RGB_ASCII)
    _reset(R, ctx)


# ---------------------------------------------------------------- 5. culled == brute

def _culled_vs_brute(R, c, p, modes, what):
    c.set_option(R.OPT_SHADOWS, 1)
    for mode in modes:
        c.set_option(R.OPT_SHADOW_CHECK, 0)
        culled = _rows(R, c, p, mode)
        assert "rtx_lights_" in c.last_kernel
        c.set_option(R.OPT_SHADOW_CHECK, 1)
        brute = _rows(R, c, p, mode)
        c.set_option(R.OPT_SHADOW_CHECK, 0)
        assert np.array_equal(culled, brute), "%s %s: %s" % (what, O.MODE_NAMES[mode], U.first_diff(culled, brute, 20 if mode >= 2 else 12, int(p.x)))


@pytest.mark.parametrize("nl", [2, 3, 8])
@pytest.mark.parametrize("seed,n", [(1, 300), (2, 1500), (3, 3000), (4, 40)])
def test_culled_equals_brute(R, ctx, seed, n, nl):
    _reset(R, ctx)
    p = R.camera_params(480, 270, pos=(0.3 * seed, 2.0, -5.0), rot=(0.1, float(np.float32(np.pi)), 0.0))
    sph, pl = R.synth_scene(seed, n, 1 + seed % 3, p.element1, p.element2)
    ctx.set_scene(sph, pl)
    g = np.random.default_rng(100 + seed)
    positions = [(10.0 * seed, 60.0, 40.0)] + [tuple(float(v) for v in g.uniform((-80, 5, -20), (80, 90, 120))) for _ in range(nl - 1)]
    ctx.set_lights(_light_set(R, nl, positions=positions))
    _culled_vs_brute(R, ctx, p, (O.RGB_ASCII, O.BIT_PIXEL), "seed %d, %d lights" % (seed, nl))
    _reset(R, ctx)


@pytest.mark.parametrize("nl", [2, 3, 8])
def test_culled_equals_brute_over_fuzz_cases(R, ctx, nl):
    _reset(R, ctx)
    seeds = _fuzz_seeds(R)
    assert len(seeds) == 6
    for seed in seeds:
        p, sph, pl, light = _fuzz_case(R, seed)
        ctx.set_scene(sph, pl)
        # the further lights as _fuzz_case places its one: somewhere within 80 of the camera on every axis
        g = np.random.default_rng(seed + 7000)
        cam = np.array(p.cam_pos[:3], dtype=np.float64)
        positions = [tuple(light)] + [tuple(float(v) for v in cam + g.uniform(-80, 80, 3)) for _ in range(nl - 1)]
        ctx.set_lights(_light_set(R, nl, positions=positions))
        _culled_vs_brute(R, ctx, p, (O.RGB_ASCII, O.BIT_ASCII), "fuzz seed %d (%d spheres, %d planes), %d lights" % (seed, len(sph), len(pl), nl))
    _reset(R, ctx)


@pytest.mark.parametrize("nl", [2, 3, 8])
def test_directed_scene_culls_the_far_spheres_and_refills(R, ctx, nl):
    _reset(R, ctx)
    sph, pl = directed_scene(n_small=3000)
    ctx.set_scene(sph, pl)
    # every light above the big sphere and the plane (|x| <= 40): the small spheres at x >= 300 are out of every segment's way
    positions = DIRECTED_LIGHTS + [(-15.0, 60.0, 50.0), (15.0, 60.0, 50.0), (0.0, 45.0, 10.0), (-25.0, 55.0, 45.0), (25.0, 55.0, 45.0)]
    ctx.set_lights(_light_set(R, nl, positions=positions[:nl]))
    p = directed_params(R)
    ctx.set_option(R.OPT_SHADOWS, 1)
    culled = _rows(R, ctx, p, O.RGB_ASCII)
    longest = ctx.get_option(R.STAT_SHADOW_LONGEST_LIST)
    assert longest < 0.1 * len(sph), longest
    ctx.set_option(R.OPT_SHADOW_CHECK, 1)
    brute = _rows(R, ctx, p, O.RGB_ASCII)
    assert ctx.get_option(R.STAT_SHADOW_LONGEST_LIST) == len(sph)  # (a sphere kept for several lights is one entry)
    assert np.array_equal(culled, brute)
    _reset(R, ctx)


def test_mirror_path_culled_equals_brute_with_three_lights(R, ctx):
    p, sph, pl, ks = _c2_floor(R, ctx)
    try:
        ctx.set_lights(_light_set(R, 3))
        for shadows in (0, 1):
            ctx.set_option(R.OPT_SHADOWS, shadows)
            for mode in (O.RGB_ASCII, O.BIT_ASCII):
                ctx.set_option(R.OPT_REFLECT_CHECK, 0)
                culled = _rows(R, ctx, p, mode)
                assert "rtx_lights_reflect_shade" in ctx.last_kernel
                ctx.set_option(R.OPT_REFLECT_CHECK, 1)
                brute = _rows(R, ctx, p, mode)
                ctx.set_option(R.OPT_REFLECT_CHECK, 0)
                assert np.array_equal(culled, brute)
    finally:
        _clear_k(ctx, len(sph) + len(pl))
        _reset(R, ctx)


def test_mirror_blend_under_three_lights_bit_for_bit(R, ctx):
    _reset(R, ctx)
    p = R.camera_params(320, 180)
    ctx.set_reference_default_scene()
    ks = {0: 0.3, 2: 0.8, 4: 1.0, 5: 0.6}
    _set_k(ctx, ks)
    try:
        _, refl, _ = _check_exact(R, ctx, p, DEFAULT_SPH, DEFAULT_PL, _light_set(R, 3, zero=1, scale=0.6), np.arange(320 * 180), ks=ks)
        assert "rtx_lights_reflect_shade" in ctx.last_kernel
        assert refl.sum() > 1000
    finally:
        _clear_k(ctx, len(DEFAULT_SPH) + len(DEFAULT_PL))
        _reset(R, ctx)


# ---------------------------------------------------------------- 6. every entry point agrees

def _three_lights_setup(R, c, name="C1"):
    p, sph, pl = R.config_inputs(name)
    c.set_scene(sph, pl)
    c.set_lights(_light_set(R, 3, positions=[(5.0, 40.0, 10.0), (-20.0, 80.0, 10.0), (30.0, 50.0, 60.0)], scale=1.5))
    c.set_option(R.OPT_SHADOWS, 1)
    return p


def test_update_equals_minimized_render(R, ctx):
    import torch
    _reset(R, ctx)
    p = _three_lights_setup(R, ctx)
    W, H = int(p.x), int(p.y)
    for mode in MODES:
        rec = torch.from_numpy(_rows(R, ctx, p, mode, S=20)).cuda()
        assert "rtx_lights_shade" in ctx.last_kernel
        out = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n2 = ctx.minimize(mode, W, H, d_in=rec.data_ptr(), d_out=out.data_ptr())
        want = out[:n2].cpu().numpy()
        for words, host_write in ((1, -1), (0, 0), (1, 1), (0, 1)):
            ctx.set_option(R.OPT_UPDATE_WORDS, words)
            ctx.set_option(R.OPT_UPDATE_HOST_WRITE, host_write)
            got = np.array(ctx.update(p, mode))
            assert np.array_equal(got, want), "Update words=%d host_write=%d mode %s" % (words, host_write, O.MODE_NAMES[mode])
    ctx.set_option(R.OPT_UPDATE_WORDS, -1)
    ctx.set_option(R.OPT_UPDATE_HOST_WRITE, -1)
    _reset(R, ctx)


def test_pipelined_updates_equal_blocking(R, ctx):
    _reset(R, ctx)
    p0 = _three_lights_setup(R, ctx)
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
    _reset(R, ctx)


def test_submit_frames_streams_slabs_compact_and_graphs(R, ctx):
    import torch
    _reset(R, ctx)
    p0 = _three_lights_setup(R, ctx, "C2")
    W, H = int(p0.x), int(p0.y)
    cams = [R.camera_params(W, H, pos=(0.4 * i, -0.2 * i, 0.1 * i)) for i in range(4)]
    want = [_rows(R, ctx, c, O.RGB_ASCII) for c in cams]
    assert "rtx_lights_shade" in ctx.last_kernel
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.full((20 * W * H,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    ctx.submit_frames(cams, O.RGB_ASCII, [b.data_ptr() for b in bufs], [s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    for b, w in zip(bufs, want):
        assert np.array_equal(b.cpu().numpy(), w)
    # slabs, batched or not (the batched launch declines on this path)
    row0, rows = H // 3, H // 3
    st = torch.cuda.Stream()
    for batch in (-1, 0):
        ctx.set_option(R.OPT_BATCH, batch)
        batched = ctx.get_option(R.STAT_BATCHED_LAUNCHES)
        sl = [torch.full((20 * W * rows,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        ctx.submit_slabs(cams, O.RGB_ASCII, row0, rows, [b.data_ptr() for b in sl], row0, [st.cuda_stream] * 4)
        torch.cuda.synchronize()
        assert ctx.get_option(R.STAT_BATCHED_LAUNCHES) == batched
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
    # a graph recorded with 3 lights still shows 3 lights after the set has changed
    buf = torch.full((20 * W * H,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(st.cuda_stream)
    ctx.render_rows(cams[2], O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=st.cuda_stream)
    g = ctx.graph_end(st.cuda_stream)
    ctx.set_light(None)
    assert ctx.get_option(R.STAT_LIGHTS) == 1
    buf.fill_(0xEE)
    torch.cuda.synchronize()
    ctx.graph_launch(g, st.cuda_stream)
    torch.cuda.synchronize()
    ctx.graph_destroy(g)
    assert np.array_equal(buf.cpu().numpy(), want[2])
    # launches queued afterwards see the change
    one = _rows(R, ctx, cams[2], O.RGB_ASCII)
    assert "rtx_lights_" not in ctx.last_kernel and not np.array_equal(one, want[2])
    _reset(R, ctx)


@pytest.mark.parametrize("ranks", [3, 8])
def test_device_group_equals_plain_context(R, ctx, ranks):
    _reset(R, ctx)
    p = _three_lights_setup(R, ctx, "C2")
    W, H = int(p.x), int(p.y)
    want = _rows(R, ctx, p, O.RGB_ASCII)
    want_stream = np.array(ctx.update(p, O.RGB_ASCII)).copy()
    with R.Context(W, H, devices=[0] * ranks) as g:
        _three_lights_setup(R, g, "C2")
        assert g.member_option(ranks - 1, R.STAT_LIGHTS) == 3
        for wire in (R.WIRE_COMPACT, R.WIRE_RECORDS):
            g.set_option(R.OPT_GROUP_WIRE, wire)
            got = g.render_to_host(p, O.RGB_ASCII)
            assert np.array_equal(got, want)
        for direct in (0, 1):
            g.set_option(R.OPT_GROUP_UPDATE, direct)
            assert np.array_equal(np.array(g.update(p, O.RGB_ASCII)), want_stream)
        assert g.member_option(ranks - 1, R.STAT_SHADOW_FRAMES) > 0
        # all or nothing on a group: a bad light in the list touches no rank
        bad = _light_set(R, 2)
        bad[1].pos[0] = float("nan")
        with pytest.raises(R.RtxError):
            g.set_lights(bad)
        assert g.member_option(ranks - 1, R.STAT_LIGHTS) == 3 and g.get_option(R.STAT_LIGHTS) == 3
        g.set_light(None)
        assert g.member_option(ranks - 1, R.STAT_LIGHTS) == 1
    _reset(R, ctx)


# ---------------------------------------------------------------- 7. the API

def test_lights_api(R, ctx):
    _reset(R, ctx)
    assert ctx.get_option(R.STAT_LIGHTS) == 1 and [_tuple(l) for l in ctx.get_lights()] == [_tuple(R.make_light())]
    for n in (1, 2, 5, 8):
        lights = _light_set(R, n, zero=n // 2)
        ctx.set_lights(lights)
        assert [_tuple(l) for l in ctx.get_lights()] == [_tuple(l) for l in lights]  # what was stored, in order
        assert ctx.get_option(R.STAT_LIGHTS) == n
        assert _tuple(ctx.get_light()) == _tuple(lights[0])
    lights = _light_set(R, 3)
    ctx.set_lights(lights)
    kept = [_tuple(l) for l in lights]
    lib = R.lib()
    arr = (R.Light * 9)()
    for i in range(9):
        C.memmove(C.byref(arr[i]), C.byref(R.make_light(pos=(float(i), 1.0, 2.0))), C.sizeof(R.Light))
    assert lib.rtx_scene_set_lights(ctx._h, 0, arr) == R.ERR_INVALID_ARGUMENT
    assert lib.rtx_scene_set_lights(ctx._h, 9, arr) == R.ERR_INVALID_ARGUMENT
    assert lib.rtx_scene_set_lights(ctx._h, 3, None) == R.ERR_INVALID_ARGUMENT
    for field, value in (("pos", float("nan")), ("diffuse_power", -1.0), ("specular_power", float("inf"))):
        bad = _light_set(R, 3)
        if field == "pos":
            bad[2].pos[1] = value  # a NaN in light 2 of 3
        else:
            setattr(bad[2], field, value)
        with pytest.raises(R.RtxError) as e:
            ctx.set_lights(bad)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
    with pytest.raises(R.RtxError):
        ctx.set_lights([])
    with pytest.raises(R.RtxError):
        ctx.set_lights(_light_set(R, 8) + [R.make_light()])
    assert [_tuple(l) for l in ctx.get_lights()] == kept  # refused calls leave the set as it was
    # rtx_scene_get_lights: min(capacity, n) lights, always the count
    n = C.c_size_t(0)
    two = (R.Light * 2)()
    assert lib.rtx_scene_get_lights(ctx._h, 2, two, C.byref(n)) == 0 and n.value == 3
    assert _tuple(two[1]) == kept[1]
    n = C.c_size_t(0)
    assert lib.rtx_scene_get_lights(ctx._h, 0, None, C.byref(n)) == 0 and n.value == 3
    ctx.scene_clear()
    assert [_tuple(l) for l in ctx.get_lights()] == kept  # context state, not scene
    for bad in (2, -1):
        with pytest.raises(R.RtxError):
            ctx.set_option(R.OPT_LIGHTS_CHECK, bad)
    with pytest.raises(R.RtxError):
        ctx.set_option(R.STAT_LIGHTS, 2)  # read-only
    # RGB_NORMALS and SDL are unchanged by any set
    p, sph, pl = R.config_inputs("C1")
    ctx.set_scene(sph, pl)
    ctx.set_light(None)
    want = _rows(R, ctx, p, O.RGB_NORMALS)
    ctx.set_lights(lights)
    ctx.set_option(R.OPT_SHADOWS, 1)
    assert np.array_equal(_rows(R, ctx, p, O.RGB_NORMALS), want)
    assert "rtx_lights_" not in ctx.last_kernel
    assert np.array_equal(ctx.render_to_host(p, O.RGB_NORMALS), want)
    sdl = _rows(R, ctx, p, O.SDL, S=20)
    assert (sdl == 0xEE).all()
    # set_light(None): one light again, and today's launches
    lit3 = _rows(R, ctx, p, O.RGB_ASCII)
    assert "rtx_lights_shade" in ctx.last_kernel
    ctx.set_light(None)
    assert ctx.get_option(R.STAT_LIGHTS) == 1
    _rows(R, ctx, p, O.RGB_ASCII)
    assert "rtx_shadow_shade" in ctx.last_kernel
    ctx.set_option(R.OPT_SHADOWS, 0)
    frames = ctx.get_option(R.STAT_SHADOW_FRAMES)
    one = _rows(R, ctx, p, O.RGB_ASCII)
    assert ctx.get_option(R.STAT_SHADOW_FRAMES) == frames and "rtx_trace" in ctx.last_kernel
    assert not np.array_equal(one, lit3)
    _reset(R, ctx)
