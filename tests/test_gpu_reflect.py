"""One-bounce mirrors (rtx_scene_set_reflectivity, RTX_OPT_REFLECT_CHECK).  The reference has no reflections (RayTracing.cu:635
plans a recursive RayTrace), so the oracles are the library's own frames, a numpy float32 restatement and a float64 rule:
  * with k = 0 everywhere every entry point launches today's kernels and the goldens hold;
  * the three-launch path with nothing reflective (RTX_OPT_REFLECT_CHECK 2) gives the bytes of the launches it replaces;
  * the culled secondary pass equals the brute one (RTX_OPT_REFLECT_CHECK 1), byte for byte;
  * a numpy float32 restatement of the issue's arithmetic (one numpy op per IEEE op, in kernel order) finds the same primary t
    and the same colour floats bit for bit;
  * the reflected winner agrees with float64 wherever float64 is clear about it;
  * every entry point agrees with the plain render, and the API validates all or nothing."""

import numpy as np
import pytest

import oracle as O
import util as U
from restate import _closest, _dot, _normal, _nrm, _scene_k, _shade, f32  # (the restatement's helpers live in tests/restate.py)

pytestmark = pytest.mark.gpu

MODES = [O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL]


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(3840, 2160)
    yield c
    c.close()


def _reset(R, c):
    for opt, v in ((R.OPT_SHADOWS, 0), (R.OPT_SHADOW_CHECK, 0), (R.OPT_REFLECT_CHECK, 0), (R.OPT_KERNEL, R.KERNEL_AUTO), (R.OPT_REFINE, -1),
                   (R.OPT_TWO_LEVEL, -1), (R.OPT_BATCH, -1)):
        c.set_option(opt, v)
    c.set_light(None)


def _rows(R, c, p, mode, flags=0):
    import torch
    W, H = int(p.x), int(p.y)
    S = 32 if flags & R.RENDER_VALUES else (4 if flags & R.RENDER_COMPACT else (20 if mode >= O.RGB_ASCII else 12))
    buf = torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, flags=flags)
    c.synchronize()
    return buf.cpu().numpy()


def _slabs(R, c, p, mode, n, flags=0):
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


def _set_k(c, ks):
    """ks: {creation index: k}"""
    for i, k in ks.items():
        c.set_reflectivity(int(i), float(k))


def _clear_k(c, n):
    c.set_reflectivity(0, np.zeros(n, dtype=np.float32))


# ---------------------------------------------------------------- 1. default state: today's kernels

GOLDEN_KEYS = {"C1": ["C1_BIT_ASCII", "C1_BIT_PIXEL", "C1_RGB_ASCII", "C1_RGB_PIXEL", "C1_RGB_NORMALS"], "C2": ["C2_BIT_ASCII", "C2_RGB_ASCII"],
               "C3": ["C3_RGB_ASCII"], "C4": ["C4_RGB_ASCII"], "C5": ["C5_RGB_ASCII"]}


def test_default_state_keeps_golden_hashes_and_launches(R, ctx):
    _reset(R, ctx)
    gold = U.load_golden()
    frames0 = ctx.get_option(R.STAT_REFLECT_FRAMES)
    mode_of = {name: m for m, name in enumerate(O.MODE_NAMES)}
    for name, keys in GOLDEN_KEYS.items():
        p, sph, pl = R.config_inputs(name)
        big = name == "C4"  # (7680 x 4320: its own context, as 8 slabs)
        c = R.Context(int(p.x), int(p.y)) if big else ctx
        try:
            if big:
                _reset(R, c)
            c.set_scene(sph, pl)
            n = len(sph) + len(pl)
            c.set_reflectivity(0, np.full(n, 0.5, dtype=np.float32))  # set, then reset to 0
            _clear_k(c, n)
            for key in keys:
                assert key in gold, key
                mode = mode_of[key[len(name) + 1:]]
                got = _slabs(R, c, p, mode, 8) if big else c.render_to_host(p, mode)
                assert O.fnv1a64(got) == gold[key]["frame_fnv1a64"], key
                assert "reflect" not in c.last_kernel and "shadow" not in c.last_kernel and "hits" not in c.last_kernel
            if not big:
                c.set_option(R.OPT_SHADOWS, 1)
                c.render_to_host(p, O.RGB_ASCII)
                assert "rtx_shadow_shade" in c.last_kernel
                c.set_option(R.OPT_SHADOWS, 0)
            assert c.get_option(R.STAT_REFLECT_FRAMES) == (0 if big else frames0)
        finally:
            if big:
                c.close()


# ---------------------------------------------------------------- 2. the path with nothing reflective: the replaced launches' bytes

@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
@pytest.mark.parametrize("kernel", ["brute", "binned", "refine"])
def test_reflect_path_neutral_without_mirrors(R, ctx, name, kernel):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ctx.set_option(R.OPT_KERNEL, R.KERNEL_BRUTE if kernel == "brute" else R.KERNEL_BINNED)
    ctx.set_option(R.OPT_REFINE, 1 if kernel == "refine" else -1)
    modes = MODES if name != "C3" else [O.RGB_ASCII]
    for shadows in (0, 1):
        ctx.set_option(R.OPT_SHADOWS, shadows)
        for mode in modes:
            for flags in (0, R.RENDER_COMPACT, R.RENDER_VALUES):
                ctx.set_option(R.OPT_REFLECT_CHECK, 0)
                want = _rows(R, ctx, p, mode, flags)
                before = ctx.get_option(R.STAT_REFLECT_FRAMES)
                ctx.set_option(R.OPT_REFLECT_CHECK, 2)
                got = _rows(R, ctx, p, mode, flags)
                assert ctx.get_option(R.STAT_REFLECT_FRAMES) == before + 1
                assert "rtx_reflect_shade" in ctx.last_kernel
                assert np.array_equal(got, want), "%s %s shadows %d %s flags %d: %s" % (
                    name, kernel, shadows, O.MODE_NAMES[mode], flags, U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)


# ---------------------------------------------------------------- 3. culled equals brute

def _culled_vs_brute(R, c, p, modes, shadows_list=(0, 1), slabs=1):
    for shadows in shadows_list:
        c.set_option(R.OPT_SHADOWS, shadows)
        for mode in modes:
            c.set_option(R.OPT_REFLECT_CHECK, 1)
            want = _slabs(R, c, p, mode, slabs)
            c.set_option(R.OPT_REFLECT_CHECK, 0)
            got = _slabs(R, c, p, mode, slabs)
            assert "rtx_reflect_shade" in c.last_kernel
            assert np.array_equal(got, want), "shadows %d %s: %s" % (shadows, O.MODE_NAMES[mode], U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))
    c.set_option(R.OPT_SHADOWS, 0)


@pytest.mark.parametrize("name,variant", [("C1", "quarter"), ("C2", "floor"), ("C2", "floor+quarter"), ("C3", "room")])
def test_culled_equals_brute_configs(R, ctx, name, variant):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ks = _scene_k(name, sph, pl, variant)
    _set_k(ctx, ks)
    modes = [O.BIT_ASCII, O.RGB_ASCII] if name != "C3" else [O.RGB_ASCII]
    _culled_vs_brute(R, ctx, p, modes)
    if variant in ("floor", "room"):
        # the cull works on real frames: the worst tile of a plane mirror keeps well under half the spheres; brute keeps all
        ctx.render_to_host(p, O.RGB_ASCII)
        longest = ctx.get_option(R.STAT_REFLECT_LONGEST_LIST)
        ctx.set_option(R.OPT_REFLECT_CHECK, 1)
        ctx.render_to_host(p, O.RGB_ASCII)
        brute = ctx.get_option(R.STAT_REFLECT_LONGEST_LIST)
        ctx.set_option(R.OPT_REFLECT_CHECK, 0)
        assert brute == len(sph)
        assert 0 < longest < len(sph) // 2 and longest < brute, (longest, brute)


def test_culled_equals_brute_default_scene_and_refills(R, ctx):
    _reset(R, ctx)
    p = R.camera_params(640, 360)
    ctx.set_reference_default_scene()
    ctx.set_reflectivity(0, np.array([0.3, 0.0, 0.8, 0.0, 1.0, 0.6], dtype=np.float32))
    _culled_vs_brute(R, ctx, p, MODES)
    # 3000 spheres: the LDS list (1024) refills; under RTX_OPT_REFLECT_CHECK 1 every workgroup lists every sphere
    sph, pl = U.numpy_synth_scene(77, 3000, 6, p.element1, p.element2)
    ctx.set_scene(sph, pl)
    rng = np.random.default_rng(5)
    ctx.set_reflectivity(0, rng.uniform(0, 1, len(sph) + len(pl)).astype(np.float32) * (rng.uniform(0, 1, len(sph) + len(pl)) < 0.5))
    _culled_vs_brute(R, ctx, p, [O.BIT_ASCII, O.RGB_PIXEL])
    ctx.set_option(R.OPT_REFLECT_CHECK, 1)
    ctx.render_to_host(p, O.RGB_ASCII)
    assert ctx.get_option(R.STAT_REFLECT_LONGEST_LIST) == 3000
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)


@pytest.mark.parametrize("seed", range(6))
def test_culled_equals_brute_random_scenes(R, ctx, seed):
    _reset(R, ctx)
    rng = np.random.default_rng(100 + seed)
    W, H = [(320, 180), (400, 300), (640, 360)][seed % 3]
    p = R.camera_params(W, H, pos=(float(rng.uniform(-5, 5)), float(rng.uniform(0, 15)), float(rng.uniform(-5, 5))),
                        rot=(float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.5, 0.5)), 0.0))
    sph, pl = U.numpy_synth_scene(1000 + seed, int(rng.integers(1, 600)), int(rng.integers(0, 7)), p.element1, p.element2)
    ctx.set_scene(sph, pl)
    n = len(sph) + len(pl)
    ctx.set_reflectivity(0, (rng.uniform(0, 1, n) * (rng.uniform(0, 1, n) < 0.6)).astype(np.float32))
    _culled_vs_brute(R, ctx, p, [O.BIT_PIXEL, O.RGB_ASCII])


def test_culled_equals_brute_fuzz_cases(R, ctx):
    """A bounded, fixed-seed share of tests/fuzz_cases.py's scenes (general and slightly non-orthonormal camera matrices, spheres
    around and containing the camera, large and far ones, tiny radii, up to 20 planes) with random k."""
    import fuzz_cases as F
    for seed in range(12):
        _reset(R, ctx)
        g = np.random.default_rng(9000 + seed)
        W, H = [(640, 360), (333, 77), (400, 150), (97, 301)][seed % 4]
        pos = [float(v) for v in g.uniform(-30, 30, 3)]
        p = R.camera_params(W, H, pos, (0.0, float(np.pi), 0.0))
        M = F.general_matrix(g)
        fov = float(g.choice([1.0, 0.5, 2.0]))
        p.element1 = float(p.element1) * fov
        p.element2 = float(p.element2) * fov
        F._set_matrix(p, M)
        sph, pl = F.scene(g, p, F._matrix_of(p), pos, W, H, max_spheres=3000)
        ctx.set_scene(sph, pl)
        n = len(sph) + len(pl)
        k = (g.uniform(0, 1, n) * (g.uniform(0, 1, n) < 0.5)).astype(np.float32)
        k[int(g.integers(0, n))] = 0.75  # (at least one mirror: small scenes could draw none)
        ctx.set_reflectivity(0, k)
        _culled_vs_brute(R, ctx, p, [O.BIT_ASCII, O.RGB_ASCII], shadows_list=(seed % 2,))


# ---------------------------------------------------------------- 4. exact against a numpy float32 restatement

def restate(p, sph, pl, ks, pix):
    """Steps 1-6 for the pixels `pix` (flat indices): the primary t and the blended colour (the local colour without shadows)."""
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
    hitm = gid >= 0
    P = tuple(O3[k] + D[k] * t for k in range(3))
    normal = _normal(P, sph, pl, gid)
    odall = np.concatenate([sph[:, 4:7], pl[:, 6:9]]).astype(np.float32) / f32(255.0)
    od = odall[np.maximum(gid, 0)]
    cl = _shade(O3, D, t, normal, [od[:, k] for k in range(3)])
    kk = np.zeros(len(sph) + len(pl), dtype=np.float32)
    for i, v in ks.items():
        kk[i] = f32(v)
    k = np.where(hitm, kk[np.maximum(gid, 0)], f32(0.0))
    refl = hitm & (t <= f32(p.cam_far)) & (pix % W != W - 1) & (k > f32(0.0))
    # the mirror (steps 1-2) and the secondary ray (step 3)
    N = _nrm(*normal)
    V = _nrm(*(D[j] * f32(-1.0) for j in range(3)))
    c = f32(2.0) * _dot(N, V)
    Rd = tuple(N[j] * c - V[j] for j in range(3))
    a2 = _dot(Rd, Rd)
    t2, g2 = _closest(P, Rd, sph, pl, a2, f32(4.0) * a2, f32(1.0) / (f32(2.0) * a2), exclude=gid)
    P2 = tuple(P[j] + Rd[j] * t2 for j in range(3))
    n2 = _normal(P2, sph, pl, g2)
    od2 = odall[np.maximum(g2, 0)]
    cr = _shade(P, Rd, t2, n2, [od2[:, j] for j in range(3)])
    cr = [np.where(g2 >= 0, cr[j], f32(0.0)) for j in range(3)]
    wgt = f32(1.0) - k
    blend = []
    for j in range(3):
        v = cl[j] * wgt + cr[j] * k
        blend.append(np.where(f32(255.0) < v, f32(255.0), v).astype(np.float32))
    colour = [np.where(refl, blend[j], cl[j]) for j in range(3)]
    return t, gid, refl, colour, (P, Rd, t2, g2)


def _check_exact(R, c, p, sph, pl, ks, pix):
    vals = _rows(R, c, p, O.RGB_ASCII, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)[pix]
    t, gid, refl, colour, _ = restate(p, sph, pl, ks, pix)
    vis = (gid >= 0) & (pix % int(p.x) != int(p.x) - 1)  # (column W-1 holds the row's terminator, no values)
    assert np.array_equal(vals[vis, 0].view(np.uint32), t[vis].view(np.uint32)), "primary t differs"
    for j in range(3):
        got, want = vals[vis, 5 + j], colour[j][vis]
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, "colour %d differs at %d pixels, e.g. got %r want %r" % (j, bad.size, got[bad[:3]], want[bad[:3]])
    return int(refl.sum())


def test_exact_default_scene_every_reflective_pixel(R, ctx):
    _reset(R, ctx)
    p = R.camera_params(320, 180)
    ctx.set_reference_default_scene()
    ks = {0: 0.3, 2: 0.8, 4: 1.0, 5: 0.6}
    _set_k(ctx, ks)
    sph = np.array([[0, 10, 20, 7, 255, 1, 1], [5, 10, 20, 6, 1, 255, 1], [10, 10, 40, 10, 1, 1, 255], [5, 10, 20, 3, 225, 210, 20],
                    [-5, 10, 40, 4, 225, 10, 220]], dtype=np.float32)
    pl = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 10, 20]], dtype=np.float32)
    n = _check_exact(R, ctx, p, sph, pl, ks, np.arange(320 * 180))
    assert n > 1000


@pytest.mark.parametrize("name,variant,sample", [("C1", "quarter", 0), ("C2", "floor", 40000), ("C3", "room", 40000)])
def test_exact_configs(R, ctx, name, variant, sample):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ks = _scene_k(name, sph, pl, variant)
    _set_k(ctx, ks)
    W, H = int(p.x), int(p.y)
    pix = np.arange(W * H) if sample == 0 else np.sort(np.random.default_rng(3).choice(W * H, size=sample, replace=False))
    n = _check_exact(R, ctx, p, sph, pl, ks, pix)
    assert n > 0


# ---------------------------------------------------------------- 5. the float64 rule

def test_reflected_winner_agrees_with_float64(R, ctx):
    """A mirror floor (k = 1) under a few coloured spheres, the camera looking down: where float64 is clear about the secondary
    ray's winner, the restatement (equal to the kernel's colours: section 4) picks the same one."""
    _reset(R, ctx)
    p = R.camera_params(320, 180, pos=(0.0, 12.0, 0.0), rot=(0.3, float(np.float32(np.pi)), 0.0))
    sph = np.array([[-7, 4, 30, 4, 230, 40, 40], [0, 5, 36, 5, 40, 230, 40], [8, 4, 30, 4, 40, 40, 230], [2, 3, 22, 2.5, 230, 230, 40]],
                   dtype=np.float32)
    pl = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80]], dtype=np.float32)
    ctx.set_scene(sph, pl)
    ks = {4: 1.0}
    _set_k(ctx, ks)
    pix = np.arange(320 * 180)
    _check_exact(R, ctx, p, sph, pl, ks, pix)
    t, gid, refl, colour, (P, Rd, t2, g2) = restate(p, sph, pl, ks, pix)
    P64 = np.stack([x.astype(np.float64) for x in P], -1)[refl]
    R64 = np.stack([x.astype(np.float64) for x in Rd], -1)[refl]
    best = np.full(len(P64), np.inf)
    win = np.full(len(P64), -1)
    amb = np.zeros(len(P64), dtype=bool)
    for j, s in enumerate(sph.astype(np.float64)):
        w = P64 - s[:3]
        a = np.einsum("nk,nk->n", R64, R64)
        b = 2 * np.einsum("nk,nk->n", R64, w)
        cc = np.einsum("nk,nk->n", w, w) - s[3] ** 2
        disc = b * b - 4 * a * cc
        tt = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
        # ambiguous: grazing (the discriminant near 0 against its terms) or starting on the surface
        amb |= (np.abs(disc) < 1e-4 * (b * b + np.abs(4 * a * cc))) | (np.abs(cc) < 1e-4 * (s[3] ** 2))
        hit = (disc >= 0) & (tt >= 0)
        amb |= hit & (np.abs(tt - best) < 1e-4 * (1 + np.abs(tt)))
        take = hit & (tt < best)
        best = np.where(take, tt, best)
        win = np.where(take, j, win)
    got = g2[refl]
    clear = ~amb
    share = (got >= 0).sum() / len(pix)
    assert share >= 0.05, "only %.3f of the pixels show a reflected sphere" % share
    assert amb.sum() < 0.001 * len(pix), "%d ambiguous pixels" % amb.sum()
    assert np.array_equal(got[clear], win[clear]), "%d pixels disagree" % (got[clear] != win[clear]).sum()


# ---------------------------------------------------------------- 6. every entry point

@pytest.fixture()
def c2_floor(R, ctx):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C2")
    ctx.set_scene(sph, pl)
    _set_k(ctx, _scene_k("C2", sph, pl, "floor+quarter"))
    return p, sph, pl


def test_render_equals_slabs_and_submit_frames(R, ctx, c2_floor):
    import torch
    p, sph, pl = c2_floor
    W, H = int(p.x), int(p.y)
    whole = ctx.render_to_host(p, O.RGB_ASCII)
    assert "rtx_reflect_shade" in ctx.last_kernel
    assert np.array_equal(_slabs(R, ctx, p, O.RGB_ASCII, 8), whole[:20 * W * H])
    ps = [R.camera_params(W, H, pos=(0.0, 2.0 * k, -1.0 * k), rot=(0.05 * k, 0.1 * k, 0.0)) for k in range(3)]
    want = [_rows(R, ctx, q, O.RGB_ASCII) for q in ps]
    streams = [torch.cuda.Stream() for _ in range(3)]
    bufs = [torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    ctx.submit_frames(ps, O.RGB_ASCII, [b.data_ptr() for b in bufs], [s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(bufs[k].cpu().numpy(), want[k]), k


def test_graph_replays_and_is_refused_after_a_change(R, ctx, c2_floor):
    import torch
    p, sph, pl = c2_floor
    W, H = int(p.x), int(p.y)
    want = _rows(R, ctx, p, O.RGB_ASCII)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(s.cuda_stream)
    ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want)
        ctx.set_reflectivity(len(sph), 0.25)
        with pytest.raises(R.RtxError) as e:
            ctx.graph_launch(g, s.cuda_stream)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
    finally:
        ctx.graph_destroy(g)


@pytest.mark.parametrize("words", [0, 1])
def test_update_equals_minimize(R, ctx, c2_floor, words):
    import torch
    p, sph, pl = c2_floor
    W, H = int(p.x), int(p.y)
    ctx.set_option(R.OPT_UPDATE_WORDS, words)
    try:
        frame = _rows(R, ctx, p, O.RGB_ASCII)
        d = torch.from_numpy(frame).cuda()
        out = torch.zeros(40 * W * H, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = ctx.minimize(O.RGB_ASCII, W, H, d_in=d.data_ptr(), d_out=out.data_ptr())
        ctx.synchronize()
        want = bytes(out[:n].cpu().numpy())
        got = bytes(ctx.update(p, O.RGB_ASCII))
        assert "rtx_reflect_shade" in ctx.last_kernel or "rtx_min" in ctx.last_kernel
        assert got == want
        ptr, arr = ctx.host_alloc(20 * W * H + 64)
        try:
            t = ctx.update_begin(p, O.RGB_ASCII, ptr)
            m = ctx.update_end(t)
            assert bytes(arr[:m]) == got
        finally:
            ctx.host_free(ptr)
    finally:
        ctx.set_option(R.OPT_UPDATE_WORDS, -1)


def test_physics_keeps_culled_equal_to_brute(R, ctx, c2_floor):
    p, sph, pl = c2_floor
    for _ in range(3):
        ctx.update_objects(0.05)
        _culled_vs_brute(R, ctx, p, [O.RGB_ASCII], shadows_list=(0,))


@pytest.mark.parametrize("ranks", [3, 8])
def test_device_group_equals_plain_context(R, ranks):
    p, sph, pl = R.config_inputs("C1")
    ks = _scene_k("C1", sph, pl, "quarter")
    ks[len(sph)] = 0.6
    outs = []
    for devices in (None, [0] * ranks):
        c = R.Context(int(p.x), int(p.y), devices=devices)
        try:
            c.set_scene(sph, pl)
            _set_k(c, ks)
            outs.append([c.render_to_host(p, m) for m in (O.BIT_ASCII, O.RGB_ASCII)])
            with pytest.raises(R.RtxError):
                c.set_reflectivity(0, [0.5, 2.0])  # all or nothing, before any rank is touched
            assert c.get_reflectivity(0) == np.float32(ks.get(0, 0.0))
        finally:
            c.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 7. API

def test_api_validation_and_lifecycle(R, ctx):
    _reset(R, ctx)
    ctx.set_reference_default_scene()
    n = 6
    assert [ctx.get_reflectivity(i) for i in range(n)] == [0.0] * n
    ctx.set_reflectivity(1, [0.25, 0.5])
    assert ctx.get_reflectivity(1) == 0.25 and ctx.get_reflectivity(2) == 0.5
    for bad_first, bad in ((0, [0.1, float("nan")]), (0, [0.1, -0.1]), (0, [1.5]), (0, [float("inf")]), (5, [0.1, 0.1]), (6, [0.1])):
        with pytest.raises(R.RtxError) as e:
            ctx.set_reflectivity(bad_first, bad)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
        assert [ctx.get_reflectivity(i) for i in range(n)] == [0.0, 0.25, 0.5, 0.0, 0.0, 0.0]
    with pytest.raises(R.RtxError):
        ctx.get_reflectivity(n)
    for v in (0, 1, 2):
        ctx.set_option(R.OPT_REFLECT_CHECK, v)
        assert ctx.get_option(R.OPT_REFLECT_CHECK) == v
    with pytest.raises(R.RtxError):
        ctx.set_option(R.OPT_REFLECT_CHECK, 3)
    ctx.set_option(R.OPT_REFLECT_CHECK, 0)
    # statistics: one launch set per rtx_render_rows call
    p = R.camera_params(320, 180)
    f0 = ctx.get_option(R.STAT_REFLECT_FRAMES)
    ctx.render_to_host(p, O.RGB_ASCII)
    _slabs(R, ctx, p, O.BIT_ASCII, 4)
    assert ctx.get_option(R.STAT_REFLECT_FRAMES) == f0 + 5
    ctx.render_to_host(p, O.RGB_NORMALS)
    assert ctx.get_option(R.STAT_REFLECT_FRAMES) == f0 + 5 and "reflect" not in ctx.last_kernel
    # clear forgets; new objects start at 0
    ctx.scene_clear()
    ctx.set_reference_default_scene()
    assert [ctx.get_reflectivity(i) for i in range(n)] == [0.0] * n


def test_reflectivity_follows_its_sphere_through_sort_and_physics(R, ctx):
    """>= 256 spheres: the trace kernels index the direction-sorted copy; a reflective sphere must stay reflective there."""
    _reset(R, ctx)
    p = R.camera_params(640, 360)
    sph, pl = U.numpy_synth_scene(9, 600, 1, p.element1, p.element2)
    ctx.set_scene(sph, pl)
    rng = np.random.default_rng(4)
    ks = {int(i): float(rng.uniform(0.2, 1.0)) for i in rng.choice(len(sph), 150, replace=False)}
    ks[len(sph)] = 0.5
    _set_k(ctx, ks)
    vals = _rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES)  # (sorts the scene at this launch)
    pix = np.sort(rng.choice(640 * 360, 20000, replace=False))
    _check_exact(R, ctx, p, sph, pl, ks, pix)
    # with the sorted store off the kernels index by sphere: the same frame
    ctx.set_option(R.OPT_SORTED_STORE, 0)
    try:
        assert np.array_equal(_rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES), vals)
    finally:
        ctx.set_option(R.OPT_SORTED_STORE, -1)
    for _ in range(2):
        ctx.update_objects(0.1)
        _culled_vs_brute(R, ctx, p, [O.RGB_ASCII], shadows_list=(0,))
