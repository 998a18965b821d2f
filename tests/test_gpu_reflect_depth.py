"""Mirrors that see mirrors (RTX_OPT_REFLECT_DEPTH, RTX_OPT_REFLECT_DEPTH_CHECK, RTX_STAT_REFLECT_RAYS).  The reference has no
reflections (RayTracing.cu:635 plans a recursive RayTrace), so the oracles are the library's own frames, a depth-general numpy
float32 restatement of the rule at rtx_scene_set_reflectivity and a float64 rule:
  * at depth 1 (the default) every launch and byte is the one-bounce path's; the chain kernels at depth 1
    (RTX_OPT_REFLECT_DEPTH_CHECK 1) give the bytes of the launches they replace, and so do they at depth 4 with nothing reflective;
  * the restatement (one numpy op per IEEE op, level by level, folded from the deepest level inwards) finds the same primary t and
    the same colour floats bit for bit at depths 1-4, and its ray counts per level equal RTX_STAT_REFLECT_RAYS;
  * a level's winner agrees with float64 wherever float64 is clear about it;
  * culled equals brute (RTX_OPT_REFLECT_CHECK 1) at depths 2 and 4;
  * every entry point honours the depth, a recorded graph keeps the depth it was recorded with;
  * the options validate and change nothing when refused."""

import numpy as np
import pytest

import oracle as O
import util as U
import test_gpu_reflect as T
from test_gpu_reflect import _closest, _dot, _normal, _nrm, _rows, _scene_k, _set_k, _shade, _slabs, f32

pytestmark = pytest.mark.gpu

MODES = T.MODES


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(3840, 2160)
    yield c
    c.close()


def _reset(R, c):
    T._reset(R, c)
    c.set_option(R.OPT_REFLECT_DEPTH, 1)
    c.set_option(R.OPT_REFLECT_DEPTH_CHECK, 0)
    c.set_option(R.OPT_LIGHTS_CHECK, 0)


def _three_lights(R):
    return [R.make_light(pos=(5.0, 40.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=900.0, specular_rgb=(0.2, 1.0, 0.4), specular_power=2100.0),
            R.make_light(pos=(-20.0, 80.0, 10.0), diffuse_rgb=(0.3, 0.6, 1.0), diffuse_power=1500.0, specular_rgb=(1.0, 1.0, 1.0), specular_power=1200.0),
            R.make_light(pos=(30.0, 50.0, 60.0), diffuse_rgb=(1.0, 1.0, 0.5), diffuse_power=700.0, specular_rgb=(1.0, 0.3, 0.3), specular_power=1800.0)]


def _ray_stats(R, c):
    return [int(c.get_option(R.STAT_REFLECT_RAYS + l)) for l in range(R.MAX_REFLECT_DEPTH)]


# ---------------------------------------------------------------- 1. neutral

def test_default_depth_keeps_launches_and_golden_hashes(R, ctx):
    _reset(R, ctx)
    assert ctx.get_option(R.OPT_REFLECT_DEPTH) == 1 and ctx.get_option(R.OPT_REFLECT_DEPTH_CHECK) == 0
    gold = U.load_golden()
    mode_of = {name: m for m, name in enumerate(O.MODE_NAMES)}
    for name, keys in (("C1", T.GOLDEN_KEYS["C1"]), ("C2", T.GOLDEN_KEYS["C2"])):
        p, sph, pl = R.config_inputs(name)
        ctx.set_scene(sph, pl)
        for key in keys:
            got = ctx.render_to_host(p, mode_of[key[len(name) + 1:]])
            assert O.fnv1a64(got) == gold[key]["frame_fnv1a64"], key
            assert "reflect" not in ctx.last_kernel and "chain" not in ctx.last_kernel and "hits" not in ctx.last_kernel
    # on the mirror path the default depth launches the one-bounce kernels
    p, sph, pl = R.config_inputs("C1")
    ctx.set_scene(sph, pl)
    _set_k(ctx, _scene_k("C1", sph, pl, "quarter"))
    ctx.render_to_host(p, O.RGB_ASCII)
    assert ctx.last_kernel.startswith("rtx_reflect_shade<")
    assert _ray_stats(R, ctx) == [0, 0, 0, 0]
    ctx.set_lights(_three_lights(R))
    ctx.render_to_host(p, O.RGB_ASCII)
    assert ctx.last_kernel.startswith("rtx_lights_reflect_shade<")
    ctx.set_light(None)


@pytest.mark.parametrize("name,variant", [("C1", "quarter"), ("C2", "floor"), ("C2", "floor+quarter"), ("C3", "room")])
def test_chain_kernels_at_depth_1_give_the_replaced_launches_bytes(R, ctx, name, variant):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    _set_k(ctx, _scene_k(name, sph, pl, variant))
    # every character mode and output form on C1 and on C2 floor+quarter's records; RGB_ASCII in every form elsewhere
    combos = [(m, fl) for m in MODES for fl in (0, R.RENDER_COMPACT, R.RENDER_VALUES)] if name == "C1" else \
             [(O.RGB_ASCII, fl) for fl in (0, R.RENDER_COMPACT, R.RENDER_VALUES)] + ([(m, 0) for m in MODES if m != O.RGB_ASCII] if variant == "floor+quarter" else [])
    for nl in (1, 3):
        if nl == 3:
            ctx.set_lights(_three_lights(R))
        for shadows in (0, 1):
            ctx.set_option(R.OPT_SHADOWS, shadows)
            for mode, flags in combos:
                ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, 0)
                want = _rows(R, ctx, p, mode, flags)
                assert ("rtx_reflect_shade<" if nl == 1 else "rtx_lights_reflect_shade<") in ctx.last_kernel
                ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, 1)
                got = _rows(R, ctx, p, mode, flags)
                assert ctx.last_kernel.startswith("rtx_lights_chain_shade<")
                assert np.array_equal(got, want), "%s %s lights %d shadows %d %s flags %d: %s" % (
                    name, variant, nl, shadows, O.MODE_NAMES[mode], flags, U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))
    ctx.set_light(None)
    _reset(R, ctx)


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_depth_4_without_mirrors_gives_the_replaced_launches_bytes(R, ctx, name):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 4)
    for shadows in (0, 1):
        ctx.set_option(R.OPT_SHADOWS, shadows)
        for mode in MODES:
            for flags in (0, R.RENDER_COMPACT, R.RENDER_VALUES):
                ctx.set_option(R.OPT_REFLECT_CHECK, 0)
                want = _rows(R, ctx, p, mode, flags)
                assert "chain" not in ctx.last_kernel and "reflect" not in ctx.last_kernel
                ctx.set_option(R.OPT_REFLECT_CHECK, 2)
                got = _rows(R, ctx, p, mode, flags)
                assert ctx.last_kernel.startswith("rtx_lights_chain_shade<")
                assert _ray_stats(R, ctx) == [0, 0, 0, 0]
                assert np.array_equal(got, want), "%s shadows %d %s flags %d: %s" % (
                    name, shadows, O.MODE_NAMES[mode], flags, U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))
    _reset(R, ctx)


# ---------------------------------------------------------------- 2. exact against a depth-general numpy float32 restatement

def restate_chain(p, sph, pl, ks, pix, max_depth=4):
    """The rule of rtx_scene_set_reflectivity for the pixels `pix`, traced to `max_depth` levels once.  Returns the primary
    (t, gid), and per level j = 0 .. max_depth: exists[j] (bool per pixel), local[j] (3 arrays), k[j], and for j >= 1 the ray
    (P, Rd), its hit (t, gid) and the object it left.  colour_at(d) folds the first d levels."""
    W = int(p.x)
    col, row = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
    m = np.array(p.inv_v[:], dtype=np.float32)
    fW, fH = f32(W), f32(int(p.y))
    vx = (((f32(2.0) * col) - fW) / fW) * f32(p.element1)
    vy = ((fH - row * f32(2.0)) / fH) * f32(p.element2)
    w = [((m[4 * k] * vx + m[4 * k + 1] * vy) + m[4 * k + 2]) + m[4 * k + 3] * f32(0.0) for k in range(3)]
    D = _nrm(*w)
    n = len(pix)
    O3 = tuple(np.full(n, f32(p.cam_pos[k]), dtype=np.float32) for k in range(3))
    a = _dot(D, D)
    with np.errstate(all="ignore"):
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
    k0 = np.where(hitm, kk[np.maximum(gid, 0)], f32(0.0)).astype(np.float32)
    chain = hitm & (t <= f32(p.cam_far)) & (pix % W != W - 1) & (k0 > f32(0.0))
    levels = [dict(exists=np.ones(n, dtype=bool), local=cl, k=k0)]
    # the state of level j for the pixels of idx: ray (origin, direction), t, normal, object
    idx = np.nonzero(chain)[0]
    cur = dict(O=tuple(x[idx] for x in O3), D=tuple(x[idx] for x in D), t=t[idx], normal=tuple(x[idx] for x in normal), gid=gid[idx])
    for j in range(max_depth):
        ex = np.zeros(n, dtype=bool)
        ex[idx] = True
        loc = [np.zeros(n, dtype=np.float32) for _ in range(3)]
        kj = np.zeros(n, dtype=np.float32)
        lev = dict(exists=ex, local=loc, k=kj, idx=idx)
        with np.errstate(all="ignore"):
            # mirror_ray: N = normalize(normal_j), V = normalize(-D), c = 2 (N . V), R = N c - V, from P = O + D t
            N = _nrm(*cur["normal"])
            V = _nrm(*(cur["D"][q] * f32(-1.0) for q in range(3)))
            c = f32(2.0) * _dot(N, V)
            Pj = tuple(cur["O"][q] + cur["D"][q] * cur["t"] for q in range(3))
            Rd = tuple(N[q] * c - V[q] for q in range(3))
            a2 = _dot(Rd, Rd)
            t2, g2 = _closest(Pj, Rd, sph, pl, a2, f32(4.0) * a2, f32(1.0) / (f32(2.0) * a2), exclude=cur["gid"])
            P2 = tuple(Pj[q] + Rd[q] * t2 for q in range(3))
            n2 = _normal(P2, sph, pl, g2)
            od2 = odall[np.maximum(g2, 0)]
            cr = _shade(Pj, Rd, t2, n2, [od2[:, q] for q in range(3)])
        for q in range(3):
            loc[q][idx] = np.where(g2 >= 0, cr[q], f32(0.0))
        k2 = np.where(g2 >= 0, kk[np.maximum(g2, 0)], f32(0.0)).astype(np.float32)
        kj[idx] = k2
        lev.update(P=Pj, Rd=Rd, t=t2, gid=g2, left=cur["gid"])
        levels.append(lev)
        go = (g2 >= 0) & (k2 > f32(0.0))
        idx = idx[go]
        cur = dict(O=tuple(x[go] for x in Pj), D=tuple(x[go] for x in Rd), t=t2[go], normal=tuple(x[go] for x in n2), gid=g2[go])

    def colour_at(depth):
        C = [x.copy() for x in levels[depth]["local"]]
        for j in range(depth - 1, -1, -1):
            kj_, wj = levels[j]["k"], f32(1.0) - levels[j]["k"]
            nxt = levels[j + 1]["exists"]
            out = []
            for q in range(3):
                with np.errstate(all="ignore"):
                    v = levels[j]["local"][q] * wj + C[q] * kj_
                v = np.where(f32(255.0) < v, f32(255.0), v).astype(np.float32)
                out.append(np.where(nxt, v, levels[j]["local"][q]))
            C = out
        return C

    return t, gid, levels, colour_at


def _check_exact_depths(R, c, p, sph, pl, ks, pix, whole_frame):
    """Depths 1 .. 4 against the restatement; returns the restatement's rays per level and the frames' colour bits per depth."""
    W = int(p.x)
    t, gid, levels, colour_at = restate_chain(p, sph, pl, ks, pix)
    counts = [int(levels[l]["exists"].sum()) for l in range(1, 5)]
    print("restatement: rays per level", counts)
    vis = (gid >= 0) & (pix % W != W - 1)  # (column W-1 holds the row's terminator, no values)
    bits = []
    for depth in (1, 2, 3, 4):
        c.set_option(R.OPT_REFLECT_DEPTH, depth)
        vals = _rows(R, c, p, O.RGB_ASCII, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)[pix]
        assert ("rtx_reflect_shade<" if depth == 1 else "rtx_lights_chain_shade<") in c.last_kernel
        assert np.array_equal(vals[vis, 0].view(np.uint32), t[vis].view(np.uint32)), "depth %d: primary t differs" % depth
        want = colour_at(depth)
        for j in range(3):
            g, w = vals[vis, 5 + j], want[j][vis]
            bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
            assert bad.size == 0, "depth %d: colour %d differs at %d pixels, e.g. got %r want %r" % (depth, j, bad.size, g[bad[:3]], w[bad[:3]])
        bits.append(vals[:, 5:8].copy().view(np.uint32))
        if whole_frame:
            stats = _ray_stats(R, c)
            print("depth", depth, "RTX_STAT_REFLECT_RAYS", stats)
            assert stats == ([0, 0, 0, 0] if depth == 1 else counts[:depth] + [0] * (4 - depth)), (depth, stats, counts)
    # a pixel's colour can only change from depth d-1 to d where it has a level-d ray
    for d in (2, 3, 4):
        changed = (bits[d - 1] != bits[d - 2]).any(axis=1) & vis
        print("colour bits changed from depth %d to %d at %d pixels; level-%d rays: %d" % (d - 1, d, int(changed.sum()), d, counts[d - 1]))
        assert not (changed & ~levels[d]["exists"]).any()
    assert (bits[1] != bits[0]).any(), "the depth-2 frame equals the depth-1 frame"
    c.set_option(R.OPT_REFLECT_DEPTH, 1)
    return counts


DEFAULT_SPH = np.array([[0, 10, 20, 7, 255, 1, 1], [5, 10, 20, 6, 1, 255, 1], [10, 10, 40, 10, 1, 1, 255], [5, 10, 20, 3, 225, 210, 20],
                        [-5, 10, 40, 4, 225, 10, 220]], dtype=np.float32)
DEFAULT_PL = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 10, 20]], dtype=np.float32)


def _mirror_floor_scene(R):
    """The scene of test_reflected_winner_agrees_with_float64 (test_gpu_reflect.py): a floor under four spheres, the camera looking down."""
    p = R.camera_params(320, 180, pos=(0.0, 12.0, 0.0), rot=(0.3, float(np.float32(np.pi)), 0.0))
    sph = np.array([[-7, 4, 30, 4, 230, 40, 40], [0, 5, 36, 5, 40, 230, 40], [8, 4, 30, 4, 40, 40, 230], [2, 3, 22, 2.5, 230, 230, 40]],
                   dtype=np.float32)
    pl = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80]], dtype=np.float32)
    ks = {0: .5, 1: .5, 2: .5, 3: .5, 4: 1.0}
    return p, sph, pl, ks


def test_exact_default_scene_every_pixel_depths_1_to_4(R, ctx):
    _reset(R, ctx)
    p = R.camera_params(320, 180)
    ctx.set_reference_default_scene()
    ks = {0: 0.3, 2: 0.8, 4: 1.0, 5: 0.6}
    _set_k(ctx, ks)
    counts = _check_exact_depths(R, ctx, p, DEFAULT_SPH, DEFAULT_PL, ks, np.arange(320 * 180), True)
    assert counts[1] >= 500 and counts[2] >= 200 and counts[3] >= 50, counts


def test_exact_mirror_floor_every_pixel_depths_1_to_4(R, ctx):
    _reset(R, ctx)
    p, sph, pl, ks = _mirror_floor_scene(R)
    ctx.set_scene(sph, pl)
    _set_k(ctx, ks)
    counts = _check_exact_depths(R, ctx, p, sph, pl, ks, np.arange(320 * 180), True)
    assert counts[1] >= 5000 and counts[2] >= 2000 and counts[3] >= 1000, counts


def test_exact_c3_room_sample_depths_1_to_4(R, ctx):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C3")
    ctx.set_scene(sph, pl)
    ks = _scene_k("C3", sph, pl, "room")
    _set_k(ctx, ks)
    W, H = int(p.x), int(p.y)
    pix = np.sort(np.random.default_rng(3).choice(W * H, size=40000, replace=False))
    counts = _check_exact_depths(R, ctx, p, sph, pl, ks, pix, False)
    assert counts[0] > 0


# ---------------------------------------------------------------- 3. the float64 rule

def float64_winners(sph, pl, levels, which=(1, 2, 3)):
    """Per level of `which`: (level, rays, ambiguous rays, clear rays whose float64 winner differs from the restatement's)."""
    out = []
    ns = len(sph)
    for l in which:
        lev = levels[l]
        n = len(lev["idx"])
        assert n > 0
        P64 = np.stack([x.astype(np.float64) for x in lev["P"]], -1)
        R64 = np.stack([x.astype(np.float64) for x in lev["Rd"]], -1)
        left = lev["left"]
        best = np.full(n, np.inf)
        win = np.full(n, -1)
        amb = np.zeros(n, dtype=bool)
        a = np.einsum("nk,nk->n", R64, R64)
        for j, s in enumerate(sph.astype(np.float64)):
            other = left != j  # (the object the ray leaves is not tested)
            w = P64 - s[:3]
            b = 2 * np.einsum("nk,nk->n", R64, w)
            cc = np.einsum("nk,nk->n", w, w) - s[3] ** 2
            disc = b * b - 4 * a * cc
            tt = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            amb |= other & ((np.abs(disc) < 1e-4 * (b * b + np.abs(4 * a * cc))) | (np.abs(cc) < 1e-4 * (s[3] ** 2)))
            hit = other & (disc >= 0) & (tt >= 0)
            amb |= hit & (np.abs(tt - best) < 1e-4 * (1 + np.abs(tt)))
            take = hit & (tt < best)
            best = np.where(take, tt, best)
            win = np.where(take, j, win)
        for q, pp in enumerate(pl.astype(np.float64)):
            other = left != ns + q
            nn = pp[3:6]
            dn = R64 @ nn
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = ((pp[:3] - P64) @ nn) / dn
            hx, hz = P64[:, 0] + R64[:, 0] * tt, P64[:, 2] + R64[:, 2] * tt
            hw, hh = pp[9] * 0.5, pp[10] * 0.5
            inside = (np.abs(hx - pp[0]) < hw) & (np.abs(hz - pp[2]) < hh)
            near_edge = (np.abs(np.abs(hx - pp[0]) - hw) < 1e-3) | (np.abs(np.abs(hz - pp[2]) - hh) < 1e-3)
            amb |= other & (np.abs(dn) < 1e-4)
            cand = other & (dn < 0) & (tt > 0)
            amb |= cand & near_edge
            hit = cand & inside
            amb |= hit & (np.abs(tt - best) < 1e-4 * (1 + np.abs(tt)))
            take = hit & (tt < best)
            best = np.where(take, tt, best)
            win = np.where(take, ns + q, win)
        got = lev["gid"]
        clear = ~amb
        out.append((l, n, int(amb.sum()), int((got[clear] != win[clear]).sum())))
    return out


def test_chain_winners_agree_with_float64(R, ctx):
    """The mirror floor scene, levels 1-3: where float64 is clear about a ray's winner, the restatement (equal to the kernel's
    colours at every depth: section 2) picks the same one.  Ambiguous, as in the level-1 test: a grazing sphere, a start on a
    sphere's surface, two hits within 1e-4; for the plane |d . n| < 1e-4 or a hit within 1e-3 of an edge.
    CPU check on the restatement's rays: 10, 4 and 0 ambiguous rays at levels 1, 2, 3 (at most 0.07 %), no disagreement."""
    _reset(R, ctx)
    p, sph, pl, ks = _mirror_floor_scene(R)
    ctx.set_scene(sph, pl)
    _set_k(ctx, ks)
    pix = np.arange(320 * 180)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    vals = _rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES).view(np.float32).reshape(-1, 8)
    t, gid, levels, colour_at = restate_chain(p, sph, pl, ks, pix, max_depth=3)
    vis = (gid >= 0) & (pix % 320 != 319)
    want = colour_at(3)
    for j in range(3):
        assert np.array_equal(vals[vis, 5 + j].view(np.uint32), want[j][vis].view(np.uint32))
    for l, n, n_amb, n_bad in float64_winners(sph, pl, levels):
        print("level %d: %d rays, %d ambiguous (%.3f %%), %d disagree" % (l, n, n_amb, 100.0 * n_amb / n, n_bad))
        assert n_amb <= 0.005 * n, "level %d: %d of %d rays ambiguous" % (l, n_amb, n)
        assert n_bad == 0, "level %d: %d rays disagree" % (l, n_bad)
    ctx.set_option(R.OPT_REFLECT_DEPTH, 1)


# ---------------------------------------------------------------- 4. culled equals brute

def _culled_vs_brute(R, c, p, modes, depths=(2, 4), shadows_list=(0,), slabs=1):
    for depth in depths:
        c.set_option(R.OPT_REFLECT_DEPTH, depth)
        for shadows in shadows_list:
            c.set_option(R.OPT_SHADOWS, shadows)
            for mode in modes:
                c.set_option(R.OPT_REFLECT_CHECK, 1)
                want = _slabs(R, c, p, mode, slabs)
                brute_rays = _ray_stats(R, c)
                c.set_option(R.OPT_REFLECT_CHECK, 0)
                got = _slabs(R, c, p, mode, slabs)
                assert c.last_kernel.startswith("rtx_lights_chain_shade<")
                if slabs == 1:
                    assert _ray_stats(R, c) == brute_rays
                assert np.array_equal(got, want), "depth %d shadows %d %s: %s" % (
                    depth, shadows, O.MODE_NAMES[mode], U.first_diff(got, want, 20 if mode >= 2 else 12, int(p.x)))
    c.set_option(R.OPT_SHADOWS, 0)
    c.set_option(R.OPT_REFLECT_DEPTH, 1)


@pytest.mark.parametrize("name,variant", [("C1", "quarter"), ("C2", "floor+quarter"), ("C3", "room")])
def test_culled_equals_brute_configs(R, ctx, name, variant):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs(name)
    ctx.set_scene(sph, pl)
    _set_k(ctx, _scene_k(name, sph, pl, variant))
    _culled_vs_brute(R, ctx, p, [O.BIT_ASCII, O.RGB_ASCII] if name == "C1" else [O.RGB_ASCII], shadows_list=(0, 1) if name != "C3" else (0,))


def test_culled_equals_brute_refills(R, ctx):
    """3000 spheres: the LDS list (1024) refills at every level; under RTX_OPT_REFLECT_CHECK 1 every workgroup lists every sphere."""
    _reset(R, ctx)
    p = R.camera_params(640, 360)
    sph, pl = U.numpy_synth_scene(77, 3000, 6, p.element1, p.element2)
    ctx.set_scene(sph, pl)
    rng = np.random.default_rng(5)
    ctx.set_reflectivity(0, rng.uniform(0, 1, len(sph) + len(pl)).astype(np.float32) * (rng.uniform(0, 1, len(sph) + len(pl)) < 0.5))
    _culled_vs_brute(R, ctx, p, [O.BIT_ASCII, O.RGB_PIXEL])
    ctx.set_option(R.OPT_REFLECT_DEPTH, 4)
    ctx.set_option(R.OPT_REFLECT_CHECK, 1)
    ctx.render_to_host(p, O.RGB_ASCII)
    assert ctx.get_option(R.STAT_REFLECT_LONGEST_LIST) == 3000  # (the maximum over the levels, not their sum)
    assert _ray_stats(R, ctx)[1] > 0
    _reset(R, ctx)


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
    _culled_vs_brute(R, ctx, p, [O.BIT_PIXEL, O.RGB_ASCII], shadows_list=(seed % 2,))


# ---------------------------------------------------------------- 5. every entry point, at depth 3

@pytest.fixture()
def c2_depth3(R, ctx):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C2")
    ctx.set_scene(sph, pl)
    _set_k(ctx, _scene_k("C2", sph, pl, "floor+quarter"))
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    yield p, sph, pl
    _reset(R, ctx)


def test_render_equals_slabs_and_submit_frames(R, ctx, c2_depth3):
    import torch
    p, sph, pl = c2_depth3
    W, H = int(p.x), int(p.y)
    whole = ctx.render_to_host(p, O.RGB_ASCII)
    assert ctx.last_kernel.startswith("rtx_lights_chain_shade<")
    rays = _ray_stats(R, ctx)
    assert rays[0] > 0 and rays[1] > 0 and rays[3] == 0, rays
    assert np.array_equal(_slabs(R, ctx, p, O.RGB_ASCII, 8), whole[:20 * W * H])
    ctx.set_option(R.OPT_REFLECT_DEPTH, 1)
    assert not np.array_equal(ctx.render_to_host(p, O.RGB_ASCII), whole), "depth 3 renders the depth-1 frame"
    ctx.set_option(R.OPT_REFLECT_DEPTH, 3)
    ps = [R.camera_params(W, H, pos=(0.0, 2.0 * k, -1.0 * k), rot=(0.05 * k, 0.1 * k, 0.0)) for k in range(3)]
    want = [_rows(R, ctx, q, O.RGB_ASCII) for q in ps]
    streams = [torch.cuda.Stream() for _ in range(3)]
    bufs = [torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    ctx.submit_frames(ps, O.RGB_ASCII, [b.data_ptr() for b in bufs], [s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(bufs[k].cpu().numpy(), want[k]), k


def test_graph_keeps_the_depth_it_was_recorded_with(R, ctx, c2_depth3):
    import torch
    p, sph, pl = c2_depth3
    W, H = int(p.x), int(p.y)
    want3 = _rows(R, ctx, p, O.RGB_ASCII)
    s = torch.cuda.Stream()
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin(s.cuda_stream)
    ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    try:
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want3)
        # the option changes: launches queued afterwards see it, the graph does not
        ctx.set_option(R.OPT_REFLECT_DEPTH, 1)
        want1 = _rows(R, ctx, p, O.RGB_ASCII)
        assert not np.array_equal(want1, want3)
        buf.zero_()
        torch.cuda.synchronize()
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want3)
        ctx.set_option(R.OPT_REFLECT_DEPTH, 4)
        _rows(R, ctx, p, O.RGB_ASCII)  # (a direct launch that grows a hit buffer must not disturb the graph's)
        buf.zero_()
        torch.cuda.synchronize()
        ctx.graph_launch(g, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want3)
    finally:
        ctx.graph_destroy(g)


@pytest.mark.parametrize("words", [0, 1])
def test_update_equals_minimize(R, ctx, c2_depth3, words):
    import torch
    p, sph, pl = c2_depth3
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
        assert "rtx_lights_chain_shade" in ctx.last_kernel or "rtx_min" in ctx.last_kernel
        assert got == want
        ptr, arr = ctx.host_alloc(20 * W * H + 64)
        try:
            tk = ctx.update_begin(p, O.RGB_ASCII, ptr)
            m = ctx.update_end(tk)
            assert bytes(arr[:m]) == got
        finally:
            ctx.host_free(ptr)
    finally:
        ctx.set_option(R.OPT_UPDATE_WORDS, -1)


def test_physics_keeps_culled_equal_to_brute(R, ctx, c2_depth3):
    p, sph, pl = c2_depth3
    for _ in range(3):
        ctx.update_objects(0.05)
        _culled_vs_brute(R, ctx, p, [O.RGB_ASCII], depths=(3,))


@pytest.mark.parametrize("ranks", [3, 8])
def test_device_group_equals_plain_context(R, ranks):
    p, sph, pl = R.config_inputs("C2")
    ks = _scene_k("C2", sph, pl, "floor+quarter")
    outs = []
    for devices in (None, [0] * ranks):
        c = R.Context(int(p.x), int(p.y), devices=devices)
        try:
            c.set_scene(sph, pl)
            _set_k(c, ks)
            c.set_option(R.OPT_REFLECT_DEPTH, 3)
            assert c.get_option(R.OPT_REFLECT_DEPTH) == 3
            with pytest.raises(R.RtxError):
                c.set_option(R.OPT_REFLECT_DEPTH, 5)
            assert c.get_option(R.OPT_REFLECT_DEPTH) == 3
            outs.append([c.render_to_host(p, m) for m in (O.BIT_ASCII, O.RGB_ASCII)])
        finally:
            c.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 6. validation

def test_option_validation_and_stats(R, ctx):
    _reset(R, ctx)
    for good in (1, 2, 3, 4, 2):
        ctx.set_option(R.OPT_REFLECT_DEPTH, good)
        assert ctx.get_option(R.OPT_REFLECT_DEPTH) == good
    for bad in (0, 5, -1):
        with pytest.raises(R.RtxError) as e:
            ctx.set_option(R.OPT_REFLECT_DEPTH, bad)
        assert e.value.status == R.ERR_INVALID_ARGUMENT
        assert ctx.get_option(R.OPT_REFLECT_DEPTH) == 2
    for v in (0, 1):
        ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, v)
        assert ctx.get_option(R.OPT_REFLECT_DEPTH_CHECK) == v
    with pytest.raises(R.RtxError) as e:
        ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, 2)
    assert e.value.status == R.ERR_INVALID_ARGUMENT
    assert ctx.get_option(R.OPT_REFLECT_DEPTH_CHECK) == 1
    ctx.set_option(R.OPT_REFLECT_DEPTH_CHECK, 0)
    with pytest.raises(R.RtxError):
        ctx.set_option(R.OPT_REFLECT_CHECK, 3)  # (keeps its three values)
    # the stats: counts after a set on the chain kernels, 0 after a depth-1 set
    p = R.camera_params(320, 180)
    ctx.set_reference_default_scene()
    _set_k(ctx, {0: 0.3, 2: 0.8, 4: 1.0, 5: 0.6})
    ctx.set_option(R.OPT_REFLECT_DEPTH, 2)
    ctx.render_to_host(p, O.RGB_ASCII)
    rays = _ray_stats(R, ctx)
    assert rays[0] > 0 and rays[1] > 0 and rays[2:] == [0, 0], rays
    ctx.set_option(R.OPT_REFLECT_DEPTH, 1)
    ctx.render_to_host(p, O.RGB_ASCII)
    assert ctx.last_kernel.startswith("rtx_reflect_shade<")
    assert _ray_stats(R, ctx) == [0, 0, 0, 0]
    ctx.render_to_host(p, O.RGB_NORMALS)  # unaffected by any depth
    ctx.set_option(R.OPT_REFLECT_DEPTH, 4)
    want = ctx.render_to_host(p, O.RGB_NORMALS)
    assert "reflect" not in ctx.last_kernel and "chain" not in ctx.last_kernel
    ctx.set_option(R.OPT_REFLECT_DEPTH, 1)
    assert np.array_equal(ctx.render_to_host(p, O.RGB_NORMALS), want)
    _reset(R, ctx)
