"""Ray queries (rtx_query_rays, rtx_query_rays_host, rtx_pick; RTX_OPT_QUERY_CHECK).  The reference has none
(RayTracingManager.cu:21,46-51 plans the culling and never builds it), so the oracles are the library's own brute kernel, a numpy
float32 restatement and a float64 rule.  Every comparison is byte for byte:
  * the grid's answers equal the brute kernel's (RTX_OPT_QUERY_CHECK 1) on C1, C2, C3, C5 and the reference's default scene, closest
    and any-hit, for 2^18 rays per set (C5 as well: its brute launch is 2^18 x 65 536 tests, well inside the usual per-test time);
    finite rays within reach never take the fallback;
  * a numpy float32 restatement (one numpy op per IEEE op, in kernel order) finds the same t bits and creation index, and the
    float64 winner agrees wherever float64 is clear about it;
  * ties go to the lower creation index; large spheres, pathological scenes and empty scenes; the grid's lifecycle; rtx_pick;
    argument validation, graph capture and device groups."""
import time

import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

f32 = np.float32
N_RAYS = 1 << 18
NO_HIT_BITS = np.float32(99999999.0).view(np.uint32)


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(1920, 1080)
    yield c
    c.close()


def _reset(R, c):
    for opt, v in ((R.OPT_QUERY_CHECK, 0), (R.OPT_QUERY_LOAD, 0), (R.OPT_SHADOWS, 0), (R.OPT_REFLECT_CHECK, 0), (R.OPT_KERNEL, R.KERNEL_AUTO)):
        c.set_option(opt, v)
    c.set_light(None)


def _scene(R, c, name):
    if name == "default":
        c.set_reference_default_scene()
        p = R.camera_params(400, 150)
        sph = np.array([[0, 10, 20, 7], [5, 10, 20, 6], [10, 10, 40, 10], [5, 10, 20, 3], [-5, 10, 40, 4]], dtype=np.float32)
        sph = np.concatenate([sph, np.ones((5, 3), np.float32)], axis=1)
        pl = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 10, 20]], dtype=np.float32)
        return p, sph, pl
    p, sph, pl = R.config_inputs(name)
    c.set_scene(sph, pl)
    return p, sph, pl


def _bytes(h):
    return np.ascontiguousarray(h).view(np.uint8)


def _both(R, c, rays, flags):
    """(grid answers, brute answers, fallback rays of the grid call)"""
    c.set_option(R.OPT_QUERY_CHECK, 0)
    got = c.query_rays(rays, flags)
    fb = c.get_option(R.STAT_QUERY_FALLBACK_RAYS)
    kernel = c.last_kernel
    c.set_option(R.OPT_QUERY_CHECK, 1)
    want = c.query_rays(rays, flags)
    assert "brute" in c.last_kernel
    c.set_option(R.OPT_QUERY_CHECK, 0)
    return got, want, fb, kernel


def _assert_equal(got, want, what):
    if not np.array_equal(_bytes(got), _bytes(want)):
        bad = np.nonzero((got["t"].view(np.uint32) != want["t"].view(np.uint32)) | (got["index"] != want["index"]))[0]
        raise AssertionError("%s: %d of %d answers differ, e.g. ray %d: grid %r brute %r" % (what, bad.size, len(got), bad[0], got[bad[0]], want[bad[0]]))


# ---------------------------------------------------------------- ray sets

def _nrm(x, y, z):
    inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
    return x * inv, y * inv, z * inv


def primary_rays(R, p, pix):
    """The primary rays of pixels `pix` (flat indices), as the trace kernels form them (RayTracing.cu:12-23), tmax = cam_far."""
    W, H = int(p.x), int(p.y)
    col, row = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
    m = np.array(p.inv_v[:], dtype=np.float32)
    fW, fH = f32(W), f32(H)
    vx = (((f32(2.0) * col) - fW) / fW) * f32(p.element1)
    vy = ((fH - row * f32(2.0)) / fH) * f32(p.element2)
    w = [((m[4 * k] * vx + m[4 * k + 1] * vy) + m[4 * k + 2]) + m[4 * k + 3] * f32(0.0) for k in range(3)]
    D = np.stack(_nrm(*w), -1)
    o = np.tile(np.array(p.cam_pos[:], dtype=np.float32), (len(pix), 1))
    return R.make_rays(o, D, tmax=f32(p.cam_far))


def _box(sph):
    lo = (sph[:, :3] - np.abs(sph[:, 3:4])).min(0).astype(np.float64)
    hi = (sph[:, :3] + np.abs(sph[:, 3:4])).max(0).astype(np.float64)
    return lo, hi


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ray_set(R, which, p, sph, rng, n=N_RAYS):
    lo, hi = _box(sph)
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    if which == "a":  # the camera's primary rays of a frame (n pixels, evenly spread; a 1080p frame where the config's is smaller than n)
        if int(p.x) * int(p.y) < n:
            p = R.camera_params(1920, 1080)
        W, H = int(p.x), int(p.y)
        return primary_rays(R, p, np.linspace(0, W * H - 1, num=min(n, W * H)).astype(np.int64))
    if which == "b":  # random origins in twice the scene box, random directions of random length
        o = ctr + rng.uniform(-2, 2, (n, 3)) * half
        return R.make_rays(o, _unit(rng, n) * rng.uniform(0.2, 5.0, (n, 1)))
    if which == "c":  # what a secondary ray looks like: from a sphere's surface, mirrored, the sphere itself skipped
        j = rng.integers(0, len(sph), n)
        nrm = _unit(rng, n)
        o = sph[j, :3].astype(np.float64) + nrm * np.abs(sph[j, 3:4])
        v = _unit(rng, n)
        v = np.where((np.einsum("nk,nk->n", v, nrm) > 0)[:, None], -v, v)  # incoming: against the normal
        d = v - 2 * np.einsum("nk,nk->n", v, nrm)[:, None] * nrm
        return R.make_rays(o, d, skip=j.astype(np.uint32))
    if which == "d":  # segments between random point pairs
        A = ctr + rng.uniform(-2, 2, (n, 3)) * half
        B = ctr + rng.uniform(-2, 2, (n, 3)) * half
        return R.make_rays(A, B - A, tmax=f32(1.0))
    raise ValueError(which)


def _grid_geometry(R, c):
    v = [c.get_option(R.STAT_QUERY_GRID_GEOMETRY + k) for k in range(9)]
    lo = np.array(v[0:3], dtype=np.uint32).view(np.float32)
    cs = np.array(v[3:6], dtype=np.uint32).view(np.float32)
    return lo, cs, [int(x) for x in v[6:9]]


def directed_set(R, c, p, sph, rng):
    """(rays, how many of them the walk is not proved for).  Needs a built grid (its cell faces and corners)."""
    lo, cs, n = _grid_geometry(R, c)
    blo, bhi = _box(sph)
    ctr, half = (blo + bhi) / 2, (bhi - blo) / 2
    hmax = half.max()

    def edge(k, i):
        return f32(lo[k] + f32(f32(i) * cs[k]))

    O_, D_, T_, S_ = [], [], [], []

    def add(o, d, tmax=np.inf, skip=0xFFFFFFFF):
        O_.append(np.asarray(o, dtype=np.float32))
        D_.append(np.asarray(d, dtype=np.float32))
        T_.append(f32(tmax))
        S_.append(skip)

    m = 3000
    for _ in range(m):  # axis-parallel, zero components of both signs, some lying in a cell face
        ax = int(rng.integers(0, 3))
        o = ctr + rng.uniform(-1.5, 1.5, 3) * half
        d = np.zeros(3)
        d[ax] = rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 10)
        d[(ax + 1) % 3] = rng.choice([0.0, -0.0])
        if rng.random() < 0.5:
            k = (ax + 1) % 3
            o[k] = edge(k, int(rng.integers(0, n[k] + 1)))
        add(o, d)
    for _ in range(m):  # in a cell face, any direction inside it
        ax = int(rng.integers(0, 3))
        o = ctr + rng.uniform(-1.5, 1.5, 3) * half
        o[ax] = edge(ax, int(rng.integers(0, n[ax] + 1)))
        d = rng.normal(size=3)
        d[ax] = 0.0
        add(o, d)
    for _ in range(m):  # through a cell corner, or from one
        cn = np.array([edge(k, int(rng.integers(0, n[k] + 1))) for k in range(3)], dtype=np.float64)
        o = ctr + rng.uniform(-2, 2, 3) * half
        if rng.random() < 0.3:
            add(cn, rng.normal(size=3))
        else:
            add(o, cn - o)
    for _ in range(m):  # from inside spheres
        j = int(rng.integers(0, len(sph)))
        o = sph[j, :3] + _unit(rng, 1)[0] * abs(sph[j, 3]) * rng.uniform(0, 1)
        add(o, rng.normal(size=3))
    for _ in range(m):  # from outside the box, pointing away from it and at it
        ax = int(rng.integers(0, 3))
        sgn = rng.choice([-1.0, 1.0])
        o = ctr + rng.uniform(-1, 1, 3) * half
        o[ax] = ctr[ax] + sgn * (half[ax] + rng.uniform(0.01, 1.5) * hmax)
        d = rng.normal(size=3)
        d[ax] = sgn * abs(d[ax]) * (1 if rng.random() < 0.7 else -1)
        add(o, d)
    for _ in range(m):  # far limits: 0, a denormal, NaN, negative, just around a hit
        j = int(rng.integers(0, len(sph)))
        o = ctr + rng.uniform(-2, 2, 3) * half
        tm = [0.0, 1e-42, np.nan, -1.0, -0.0, float(rng.uniform(0, 1.5)), np.inf][int(rng.integers(0, 7))]
        add(o, sph[j, :3] - o, tmax=tm)
    n_walkable = len(O_)
    # the walk is not proved for these: every object is tested
    far = ctr + np.array([0.0, 0.0, 3.5 * hmax])
    degenerate = [
        ((np.nan, 0, 0), (0, 0, 1)), ((np.inf, 0, 0), (0, 0, 1)), ((0, -np.inf, 0), (0, 1, 0)), (ctr, (np.nan, 0, 1)), (ctr, (0, np.inf, 0)),
        (ctr, (0, 0, 0)), (ctr, (-0.0, 0.0, -0.0)), (ctr, (1e-8, 0, 0)), (ctr, (0, 3e6, 0)), (ctr, (1e-30, 1e-30, 0)), (far, (0, 0, -1)),
        (far, (0, 0, 1)), (ctr - np.array([3.01 * hmax, 0, 0]), (1, 0.01, 0.02)), (ctr, (3e38, 3e38, 0)),
    ]
    for rep in range(40):
        for o, d in degenerate:
            add(o, d, tmax=[np.inf, 1.0][rep % 2])
    rays = R.make_rays(np.stack(O_), np.stack(D_), tmax=np.array(T_, dtype=np.float32), skip=np.array(S_, dtype=np.uint32))
    # interleave, so that a wave holds walkable and unwalkable rays side by side
    perm = rng.permutation(len(rays))
    return rays[perm], len(rays) - n_walkable


# ---------------------------------------------------------------- 5. grid equals brute

@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C5", "default"])
def test_grid_equals_brute(R, ctx, name):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, name)
    rng = np.random.default_rng(100 + len(sph))
    for which in "abcd":
        rays = ray_set(R, which, p, sph, rng)
        assert len(rays) >= N_RAYS
        for flags in (R.QUERY_CLOSEST, R.QUERY_ANY):
            got, want, fb, kernel = _both(R, ctx, rays, flags)
            assert "grid" in kernel, kernel
            _assert_equal(got, want, "%s set (%s) flags %d" % (name, which, flags))
            assert fb == 0, "%s set (%s): %d finite rays took the fallback" % (name, which, fb)
            if flags == R.QUERY_ANY:
                hit = got["index"] != R.NO_OBJECT
                assert np.all(got["index"][hit] == R.SOME_OBJECT) and np.all(got["t"][hit] == 0)
                assert np.all(got["t"][~hit].view(np.uint32) == NO_HIT_BITS)
        print("%s set %s: %.3f of the rays hit something" % (name, which, float((got["index"] != R.NO_OBJECT).mean())))
    assert ctx.get_option(R.STAT_QUERY_BRUTE) == 0 and ctx.get_option(R.STAT_QUERY_GRID_CELLS) >= 1
    rays, n_deg = directed_set(R, ctx, p, sph, rng)
    for flags in (R.QUERY_CLOSEST, R.QUERY_ANY):
        got, want, fb, kernel = _both(R, ctx, rays, flags)
        _assert_equal(got, want, "%s directed set flags %d" % (name, flags))
        assert fb == n_deg, "%s directed set: %d fallback rays, %d degenerate rays put in" % (name, fb, n_deg)
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) >= 1


def test_closest_and_any_agree(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C2")
    rays = ray_set(R, "b", p, sph, np.random.default_rng(3), 1 << 16)
    near = ctx.query_rays(rays, R.QUERY_CLOSEST)
    anyh = ctx.query_rays(rays, R.QUERY_ANY)
    assert np.array_equal(near["index"] != R.NO_OBJECT, anyh["index"] == R.SOME_OBJECT)


# ---------------------------------------------------------------- 6. an independent restatement

def np_closest(rays, sph, pl):
    """Lexicographic minimum of (t, creation index) over every sphere and plane (spheres were created first), in numpy float32, one
    numpy operation per IEEE operation of the kernels: (t, index), index -1 without a hit."""
    n = len(rays)
    o = [rays["o"][:, k].copy() for k in range(3)]
    d = [rays["d"][:, k].copy() for k in range(3)]
    tmax, skip = rays["tmax"], rays["skip"].astype(np.int64)
    a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    fourA = f32(4.0) * a
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        divTwoA = f32(1.0) / (f32(2.0) * a)
    bt = np.full(n, f32(99999999.0), dtype=np.float32)
    bid = np.full(n, -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j, s in enumerate(sph.astype(np.float32)):
            ox, oy, oz = o[0] - s[0], o[1] - s[1], o[2] - s[2]
            cc = ((ox * ox + oy * oy) + oz * oz) - s[3] * s[3]
            sd = (d[0] * ox + d[1] * oy) + d[2] * oz
            q = sd * sd - a * cc
            b = f32(2.0) * sd
            disc = b * b - fourA * cc
            t2 = (-b - np.sqrt(np.maximum(disc, f32(0.0)))) * divTwoA
            hit = ~(q < f32(-1e-30)) & ~(disc < f32(0.0)) & ~(t2 < f32(0.0)) & ~np.isnan(disc)
            hit &= (t2 <= tmax) & (skip != j)
            take = hit & ((t2 < bt) | ((t2 == bt) & ((bid < 0) | (j < bid))))
            bt = np.where(take, t2, bt)
            bid = np.where(take, j, bid)
        for k, P in enumerate(pl.astype(np.float32)):
            gi = len(sph) + k
            dn = (d[0] * P[3] + d[1] * P[4]) + d[2] * P[5]
            num = ((P[0] - o[0]) * P[3] + (P[1] - o[1]) * P[4]) + (P[2] - o[2]) * P[5]
            t1 = num / dn
            hx, hz = o[0] + d[0] * t1, o[2] + d[2] * t1
            hw, hh = P[9] * f32(0.5), P[10] * f32(0.5)
            hit = ~((dn > f32(0.0)) | (np.abs(dn - f32(0.0)) < f32(1.1920928955078125e-7))) & ~(t1 <= f32(0.0)) & ~np.isnan(t1)
            hit &= ~(((hx <= P[0] - hw) | (hx >= P[0] + hw)) | ((hz <= P[2] - hh) | (hz >= P[2] + hh)))
            hit &= (t1 <= tmax) & (skip != gi)
            take = hit & ((t1 < bt) | ((t1 == bt) & ((bid < 0) | (gi < bid))))
            bt = np.where(take, t1, bt)
            bid = np.where(take, gi, bid)
    return bt, bid


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_equals_numpy_restatement(R, ctx, name):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, name)
    rng = np.random.default_rng(7)
    for which in "abcd":
        rays = ray_set(R, which, p, sph, rng, 1 << 14)
        rays = rays[rng.choice(len(rays), size=4096, replace=False)]
        got = ctx.query_rays(rays)
        t, gid = np_closest(rays, sph, pl)
        want_idx = np.where(gid < 0, R.NO_OBJECT, gid).astype(np.uint32)
        bad = np.nonzero((got["t"].view(np.uint32) != t.view(np.uint32)) | (got["index"] != want_idx))[0]
        assert bad.size == 0, "%s set %s: %d rays differ, e.g. %d: got %r want (%r, %d)" % (name, which, bad.size, bad[0], got[bad[0]], t[bad[0]], gid[bad[0]])
        assert (gid >= 0).mean() > 0.05, "set %s hits too little to mean anything" % which


def test_winner_agrees_with_float64(R, ctx):
    """Where float64 is clear about the closest sphere (no grazing, no start on a surface, no near tie), the query names it."""
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C2")
    rng = np.random.default_rng(8)
    for which in "abd":
        rays = ray_set(R, which, p, sph, rng, 1 << 13)
        rays["tmax"] = np.inf
        got = ctx.query_rays(rays)
        t32, gid32 = np_closest(rays, sph, np.zeros((0, 11), np.float32))
        O64, D64 = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
        # What fp32 can blur (csrc/rtx_grid.hpp): the discriminant by 4 kappa a |o - c|^2, kappa = 2e-6, hence t by
        # kappa |o - c|^2 / sqrt(disc) and a few ulps of itself.  A ray is ambiguous when some sphere's discriminant or start is within
        # five times that of zero while the sphere is no further along the ray than the winner, or when a sphere other than the winner comes
        # within five times the two t errors of the winner's t.
        a = np.einsum("nk,nk->n", D64, D64)
        S64 = sph.astype(np.float64)

        def one(s):
            w = O64 - s[:3]
            oo = np.einsum("nk,nk->n", w, w)
            b = 2 * np.einsum("nk,nk->n", D64, w)
            cc = oo - s[3] ** 2
            disc = b * b - 4 * a * cc
            tt = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            grazing = (np.abs(disc) < 4e-5 * a * oo) | (np.abs(cc) < 1e-5 * oo)
            tca = -b / (2 * a)  # closest approach; a grazing hit is reported within sqrt(4e-5 a oo) / 2a before it
            first = tca - 3.2e-3 * np.sqrt(oo / a) - 1e-5 * np.abs(tca)
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.where(disc > 0, 1e-5 * oo / np.sqrt(np.maximum(disc, 1e-300)), np.inf) + 1e-5 * np.abs(tt)
            return (disc >= 0) & (tt >= 0), tt, err, grazing & (tca + 3.2e-3 * np.sqrt(oo / a) >= 0), first

        best = np.full(len(rays), np.inf)
        best_err = np.zeros(len(rays))
        win = np.full(len(rays), -1)
        amb = np.zeros(len(rays), dtype=bool)
        for j, s in enumerate(S64):
            hit, tt, err, grazing, first = one(s)
            take = hit & (tt < best)
            best = np.where(take, tt, best)
            best_err = np.where(take, err, best_err)
            win = np.where(take, j, win)
        for j, s in enumerate(S64):
            hit, tt, err, grazing, first = one(s)
            amb |= hit & (win != j) & (tt - err < best + best_err)
            amb |= grazing & (first < best + best_err)
        # planes out of the comparison: rays whose query winner is a plane are compared on the spheres alone through the restatement
        sph_win = np.where(gid32 < 0, -1, gid32)
        on_sphere = (got["index"] < len(sph)) | (got["index"] == R.NO_OBJECT)
        clear = ~amb
        assert amb.sum() < 0.2 * len(rays), "%d ambiguous rays" % amb.sum()
        assert np.array_equal(sph_win[clear], win[clear]), "set %s: %d rays disagree with float64" % (which, (sph_win[clear] != win[clear]).sum())
        got_idx = np.where(got["index"] == R.NO_OBJECT, -1, got["index"].astype(np.int64))
        sel = clear & on_sphere
        assert np.array_equal(got_idx[sel], win[sel])


# ---------------------------------------------------------------- 7. ties

def test_ties_go_to_the_lower_creation_index(R, ctx):
    _reset(R, ctx)
    ctx.scene_clear()
    a = ctx.add_sphere(2.0, (0.0, 0.0, 30.0), (255.0, 0.0, 0.0))
    ctx.add_plane((0.0, -5.0, 30.0), (0.0, 1.0, 0.0), (100.0, 100.0, 100.0), 50.0, 50.0)
    ctx.add_sphere(1.0, (9.0, 0.0, 30.0), (0.0, 255.0, 0.0))
    b = ctx.add_sphere(2.0, (0.0, 0.0, 30.0), (0.0, 0.0, 255.0))  # the twin of a, created later
    assert a == 0 and b == 3
    rng = np.random.default_rng(1)
    o = rng.uniform(-1, 1, (4096, 3)) * (6, 6, 6) + (0, 0, 15)
    rays = R.make_rays(o, (0, 0, 30) - o + rng.uniform(-1.5, 1.5, (4096, 3)))
    for check in (0, 1):
        ctx.set_option(R.OPT_QUERY_CHECK, check)
        h = ctx.query_rays(rays)
        assert (h["index"] == a).sum() > 2000 and not np.any(h["index"] == b)
        skipped = rays.copy()
        skipped["skip"] = a
        h2 = ctx.query_rays(skipped)
        on_a = h["index"] == a
        assert np.all(h2["index"][on_a] == b) and np.array_equal(h2["t"][on_a].view(np.uint32), h["t"][on_a].view(np.uint32))
    ctx.set_option(R.OPT_QUERY_CHECK, 0)


# ---------------------------------------------------------------- 8. large spheres and pathological scenes

BUILD_SECONDS = 20.0  # per pathological scene, first query included: a normal build is two waits and five small launches (milliseconds);
                      # a build that degenerated into cells x spheres (2^21 x 1024 box tests and as many list entries) would pass this many times


def _pathological(R, ctx, sph, pl, large, rng, n=1 << 15):
    ctx.set_scene(sph, pl)
    box = sph if len(sph) else np.array([[0, 0, 100, 50, 0, 0, 0]], dtype=np.float32)
    p = R.camera_params(320, 180)
    t0 = time.time()
    ctx.query_rays(ray_set(R, "b", p, box, rng, 64))
    took = time.time() - t0
    assert took < BUILD_SECONDS, "the build took %.1f s" % took
    if large is not None:
        assert ctx.get_option(R.STAT_QUERY_LARGE_SPHERES) == large
    for which in "abd":
        rays = ray_set(R, which, p, box, rng, n)
        for flags in (R.QUERY_CLOSEST, R.QUERY_ANY):
            got, want, fb, _ = _both(R, ctx, rays, flags)
            _assert_equal(got, want, "set %s flags %d" % (which, flags))
    return got


def test_one_sphere_enclosing_the_scene(R, ctx):
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C2")
    big = np.array([[0, 0, 120, 400, 9, 9, 9]], dtype=np.float32)
    _pathological(R, ctx, np.concatenate([big, sph]), pl, 1, np.random.default_rng(2))
    assert ctx.get_option(R.STAT_QUERY_BRUTE) == 0
    # from inside the big sphere it is never hit (Sphere.cu:52-66); from outside it is
    out = ctx.query_rays(R.make_rays([(0, 0, -400)], [(0, 0, 1)]))
    assert out["index"][0] == 0


def test_concentric_spheres(R, ctx):
    _reset(R, ctx)
    sph = np.zeros((1024, 7), dtype=np.float32)
    sph[:, :3] = (3, 4, 50)
    sph[:, 3] = np.linspace(0.01, 20, 1024)
    _pathological(R, ctx, sph, np.zeros((0, 11), np.float32), None, np.random.default_rng(3))
    # more than 256 of them cover more than 64 cells: the context says it answers with the brute kernel
    large, brute = ctx.get_option(R.STAT_QUERY_LARGE_SPHERES), ctx.get_option(R.STAT_QUERY_BRUTE)
    assert (large > 256) == (brute == 1)
    out = ctx.query_rays(R.make_rays([(3, 4, 0)], [(0, 0, 1)]))
    assert out["index"][0] == 1023


def test_all_spheres_in_one_cell(R, ctx):
    _reset(R, ctx)
    rng = np.random.default_rng(4)
    sph = np.zeros((1024, 7), dtype=np.float32)
    sph[:, :3] = (10, -5, 80) + rng.uniform(-1e-3, 1e-3, (1024, 3))
    sph[:, 3] = rng.uniform(1e-4, 2e-4, 1024)
    sph[0] = (-60, 30, 150, 1, 0, 0, 0)  # one far away, so that the box is large and the rest shares a cell
    ctx.set_scene(sph, np.zeros((0, 11), np.float32))
    _pathological(R, ctx, sph, np.zeros((0, 11), np.float32), 0, rng)
    aim = R.make_rays(np.tile((10, -5, 0), (1024, 1)), sph[:, :3] - (10, -5, 0))
    got, want, fb, _ = _both(R, ctx, aim, R.QUERY_CLOSEST)
    _assert_equal(got, want, "aimed at the cluster")
    assert (got["index"] != R.NO_OBJECT).mean() > 0.5


def test_single_sphere_planes_only_and_nothing(R, ctx):
    _reset(R, ctx)
    rng = np.random.default_rng(5)
    one = np.array([[1, 2, 30, 3, 200, 100, 50]], dtype=np.float32)
    p, _, pl = R.config_inputs("C3")
    got = _pathological(R, ctx, one, pl, 0, rng)
    out = ctx.query_rays(R.make_rays([(1, 2, 0)], [(0, 0, 2)]))
    assert out["index"][0] == 0 and out["t"][0] == 13.5
    # planes only
    got = _pathological(R, ctx, np.zeros((0, 7), np.float32), pl, 0, rng)
    assert (got["index"] != R.NO_OBJECT).mean() > 0.05 and ctx.get_option(R.STAT_QUERY_GRID_CELLS) == 0
    # no objects at all
    got = _pathological(R, ctx, np.zeros((0, 7), np.float32), np.zeros((0, 11), np.float32), 0, rng)
    assert np.all(got["index"] == R.NO_OBJECT) and np.all(got["t"].view(np.uint32) == NO_HIT_BITS)


def test_scaled_scenes_and_non_finite_spheres(R, ctx):
    """Scenes scaled by 1e18 and 1e-18 have no grid (coordinates beyond 2^50 / below 2^-50) and are answered by the brute kernel; by
    1e6 and 1e-6 they have one; a sphere moved to NaN is kept in the large list."""
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C2")
    rng = np.random.default_rng(6)
    for scale, brute in ((1e18, 1), (1e-18, 1), (1e6, 0), (1e-6, 0)):
        s2, p2 = sph.copy(), pl.copy()
        s2[:, :4] *= f32(scale)
        p2[:, :3] *= f32(scale)
        p2[:, 9:11] *= f32(scale)
        ctx.set_scene(s2, p2)
        rays = ray_set(R, "b", p, s2, rng, 1 << 14)
        for flags in (R.QUERY_CLOSEST, R.QUERY_ANY):
            got, want, fb, _ = _both(R, ctx, rays, flags)
            _assert_equal(got, want, "scale %g" % scale)
        assert ctx.get_option(R.STAT_QUERY_BRUTE) == brute, scale
        if not brute:
            assert fb == 0 and (got["index"] != R.NO_OBJECT).mean() > 0.02
    s3 = sph.copy()
    s3[5, 1] = np.nan
    s3[9, 3] = np.inf
    ctx.set_scene(s3, pl)
    rays = ray_set(R, "b", p, sph, rng, 1 << 14)
    got, want, fb, _ = _both(R, ctx, rays, R.QUERY_CLOSEST)
    _assert_equal(got, want, "non-finite spheres")
    assert ctx.get_option(R.STAT_QUERY_LARGE_SPHERES) == 2 and fb == 0


# ---------------------------------------------------------------- 9. lifecycle

def test_builds_are_counted_and_follow_the_scene(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C2")
    rng = np.random.default_rng(9)
    rays = ray_set(R, "b", p, sph, rng, 1 << 15)
    b0 = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    first = ctx.query_rays(rays)
    second = ctx.query_rays(rays, R.QUERY_ANY)
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == b0 + 1, "two queries on one scene build once"
    ctx.set_option(R.OPT_QUERY_CHECK, 1)
    ctx.query_rays(rays)
    ctx.set_option(R.OPT_QUERY_CHECK, 0)
    ctx.query_rays(rays)
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == b0 + 1
    # an added sphere is found
    new = ctx.add_sphere(30.0, (0.0, 0.0, 120.0), (1.0, 2.0, 3.0))
    got, want, fb, _ = _both(R, ctx, rays, R.QUERY_CLOSEST)
    _assert_equal(got, want, "after rtx_scene_add_sphere")
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == b0 + 2 and np.any(got["index"] == new)
    # physics: every sphere moves in y; the next query sees them where they are
    for i in range(0, len(sph), 3):
        ctx.set_sphere_motion(i, 1 if i % 2 else -1, 3.0 + (i % 7))
    for step in range(3):
        ctx.update_objects(0.37)
        got, want, fb, _ = _both(R, ctx, rays, R.QUERY_CLOSEST)
        _assert_equal(got, want, "after rtx_update_objects %d" % step)
        assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == b0 + 3 + step and fb == 0
    assert not np.array_equal(_bytes(got), _bytes(first))
    # clear and re-add
    ctx.scene_clear()
    assert np.all(ctx.query_rays(rays[:1000])["index"] == R.NO_OBJECT)
    ctx.set_scene(sph, pl)
    again = ctx.query_rays(rays)
    _assert_equal(again, first, "after rtx_scene_clear and the same scene again")
    # a direction re-sort (a render from elsewhere after an edit re-sorts the copies the trace kernels read): answers unchanged
    ctx.render_to_host(p, O.RGB_ASCII)
    ctx.add_sphere(0.5, (0.0, 0.0, -50.0), (1.0, 1.0, 1.0))
    p2 = R.camera_params(int(p.x), int(p.y), pos=(40.0, 5.0, 100.0), rot=(0.2, 1.0, 0.0))
    ctx.render_to_host(p2, O.RGB_ASCII)
    got, want, fb, _ = _both(R, ctx, rays, R.QUERY_CLOSEST)
    _assert_equal(got, want, "after a direction re-sort")
    assert second is not None


def test_indices_follow_a_sphere_through_sort_and_physics(R, ctx):
    """A marked sphere among C2's, found by a ray aimed at it: before and after the direction sort (a render) and a physics step the
    query names its creation index and rtx_scene_get_object of that index gives the sphere the ray hit."""
    _reset(R, ctx)
    p, sph, pl = R.config_inputs("C2")
    ctx.set_scene(sph[:500], pl)
    mark = ctx.add_sphere(1.5, (2.0, 3.0, 20.0), (9.0, 8.0, 7.0))
    ctx.add_spheres(sph[500:])
    ctx.set_sphere_motion(mark, 1, 2.0)
    ray = R.make_rays([(2.0, 3.0, 0.0)], [(0.0, 0.0, 1.0)])
    assert ctx.query_rays(ray)["index"][0] == mark
    ctx.render_to_host(p, O.RGB_ASCII)  # (sorts the copies the trace kernels read)
    assert ctx.query_rays(ray)["index"][0] == mark
    ctx.update_objects(0.5)
    kind, v = ctx.get_object(mark)
    ray2 = R.make_rays([(v[0], v[1], 0.0)], [(0.0, 0.0, 1.0)])
    h = ctx.query_rays(ray2)
    assert h["index"][0] == mark and h["t"][0] == f32(v[2]) - f32(v[3])
    assert ctx.pick(p, 0, 0)[1] != mark


def test_queries_between_frames_leave_the_golden_hashes(R, ctx):
    _reset(R, ctx)
    gold = U.load_golden()
    mode_of = {name: m for m, name in enumerate(O.MODE_NAMES)}
    rng = np.random.default_rng(10)
    for name, keys in (("C1", ["C1_BIT_ASCII", "C1_RGB_ASCII", "C1_RGB_NORMALS"]), ("C2", ["C2_BIT_ASCII", "C2_RGB_ASCII"]), ("C3", ["C3_RGB_ASCII"]),
                       ("C5", ["C5_RGB_ASCII"])):
        p, sph, pl = R.config_inputs(name)
        c = ctx if int(p.x) <= 1920 else R.Context(int(p.x), int(p.y))
        try:
            c.set_scene(sph, pl)
            rays = ray_set(R, "b", p, sph, rng, 1 << 12)
            for key in keys:
                c.query_rays(rays)
                got = c.render_to_host(p, mode_of[key[len(name) + 1:]])
                c.pick(p, 5, 5)
                assert O.fnv1a64(got) == gold[key]["frame_fnv1a64"], key
        finally:
            if c is not ctx:
                c.close()


# ---------------------------------------------------------------- 10. rtx_pick

@pytest.mark.parametrize("name", ["default", "C1"])
def test_pick_names_the_object_under_a_cell(R, ctx, name):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, name)
    W, H = int(p.x), int(p.y)
    cols, rows = np.arange(0, W - 1, max(1, W // 40)), np.arange(0, H, max(1, H // 24))
    pix = (rows[:, None] * W + cols[None, :]).reshape(-1)
    t, gid = np_closest(primary_rays(R, p, pix), sph, pl)
    seen = set()
    for k, px in enumerate(pix):
        pt, pi = ctx.pick(p, int(px % W), int(px // W))
        want = R.NO_OBJECT if gid[k] < 0 else int(gid[k])
        assert pi == want and f32(pt).view(np.uint32) == t[k].view(np.uint32), (int(px % W), int(px // W), pt, pi, t[k], gid[k])
        seen.add(pi)
    assert R.NO_OBJECT in seen and len(seen) >= 3
    for col, row in ((W - 1, 0), (W, 0), (0, H), (1 << 40, 0)):
        with pytest.raises(R.RtxError) as e:
            ctx.pick(p, col, row)
        assert e.value.status == R.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- 11. validation, capture, groups, device pointers

def test_argument_validation(R, ctx):
    import ctypes as C
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C1")
    L = R.lib()
    rays = ray_set(R, "b", p, sph, np.random.default_rng(0), 16)
    hits = np.zeros(16, dtype=R.RAY_HIT_DTYPE)
    b0 = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    assert L.rtx_query_rays_host(ctx._h, 0, None, None, 0) == R.OK
    assert L.rtx_query_rays(ctx._h, 0, None, None, 0, None) == R.OK
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == b0, "n = 0 launches and builds nothing"
    assert len(ctx.query_rays(rays[:0])) == 0
    for args in ((16, None, hits.ctypes.data, 0), (16, rays.ctypes.data, None, 0), (16, rays.ctypes.data, hits.ctypes.data, 2),
                 (16, rays.ctypes.data, hits.ctypes.data, 0x80000001)):
        assert L.rtx_query_rays_host(ctx._h, *args) == R.ERR_INVALID_ARGUMENT
        assert len(L.rtx_last_error(ctx._h)) > 10
        assert L.rtx_query_rays(ctx._h, *args, None) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_query_rays_host(None, 16, rays.ctypes.data, hits.ctypes.data, 0) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_pick(ctx._h, None, 0, 0, C.byref(R.RayHit())) == R.ERR_INVALID_ARGUMENT
    assert L.rtx_pick(ctx._h, C.byref(p), 0, 0, None) == R.ERR_INVALID_ARGUMENT
    for opt, bad in ((R.OPT_QUERY_CHECK, 2), (R.OPT_QUERY_CHECK, -1), (R.OPT_QUERY_LOAD, -1), (R.OPT_QUERY_LOAD, 5000)):
        with pytest.raises(R.RtxError):
            ctx.set_option(opt, bad)
    assert ctx.get_option(R.OPT_QUERY_CHECK) == 0


def test_device_pointers_streams_and_graph_capture(R, ctx):
    import torch
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C2")
    rays = ray_set(R, "c", p, sph, np.random.default_rng(12), 1 << 16)
    want = ctx.query_rays(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(len(rays) * 8, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.query_rays_device(len(rays), d_rays.data_ptr(), d_hits.data_ptr(), R.QUERY_CLOSEST, s.cuda_stream)
    s.synchronize()
    _assert_equal(d_hits.cpu().numpy().view(R.RAY_HIT_DTYPE), want, "device pointers on a stream of the caller")
    # a physics step on the context's stream, then a query on the caller's: the rebuild is ordered between them
    for i in range(0, len(sph), 2):
        ctx.set_sphere_motion(i, 1, 4.0)
    builds = ctx.get_option(R.STAT_QUERY_GRID_BUILDS)
    ctx.update_objects(0.3)
    ctx.query_rays_device(len(rays), d_rays.data_ptr(), d_hits.data_ptr(), R.QUERY_ANY, s.cuda_stream)
    s.synchronize()
    assert ctx.get_option(R.STAT_QUERY_GRID_BUILDS) == builds + 1
    ctx.set_option(R.OPT_QUERY_CHECK, 1)
    _assert_equal(d_hits.cpu().numpy().view(R.RAY_HIT_DTYPE), ctx.query_rays(rays, R.QUERY_ANY), "after a physics step, on a stream of the caller")
    ctx.set_option(R.OPT_QUERY_CHECK, 0)
    # inside a capture: refused, and the capture goes on
    W, H = int(p.x), int(p.y)
    buf = torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda")
    ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    s.synchronize()
    ctx.graph_begin(s.cuda_stream)
    with pytest.raises(R.RtxError) as e:
        ctx.query_rays_device(len(rays), d_rays.data_ptr(), d_hits.data_ptr(), R.QUERY_CLOSEST, s.cuda_stream)
    assert e.value.status == R.ERR_INVALID_ARGUMENT and "capture" in str(e.value)
    ctx.render_rows(p, O.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=s.cuda_stream)
    g = ctx.graph_end(s.cuda_stream)
    ctx.graph_destroy(g)
    ctx.set_scene(sph, pl)


def test_device_group_answers_like_a_plain_context(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C2")
    rng = np.random.default_rng(13)
    rays = ray_set(R, "b", p, sph, rng, 1 << 15)
    want = ctx.query_rays(rays)
    want_any = ctx.query_rays(rays, R.QUERY_ANY)
    with R.Context(1920, 1080, devices=[0, 0, 0]) as g:
        assert g.group_size == 3
        g.set_scene(sph, pl)
        _assert_equal(g.query_rays(rays), want, "device group, closest")
        _assert_equal(g.query_rays(rays, R.QUERY_ANY), want_any, "device group, any")
        assert g.pick(p, 100, 100) == ctx.pick(p, 100, 100)
        g.update_objects(0.25)
        ctx.update_objects(0.25)
        _assert_equal(g.query_rays(rays), ctx.query_rays(rays), "device group after a physics step")
    ctx.set_scene(sph, pl)


def test_grid_load_option_changes_cells_not_answers(R, ctx):
    _reset(R, ctx)
    p, sph, pl = _scene(R, ctx, "C3")
    rays = ray_set(R, "c", p, sph, np.random.default_rng(14), 1 << 15)
    want = ctx.query_rays(rays)
    cells = {0: ctx.get_option(R.STAT_QUERY_GRID_CELLS)}
    for load in (8, 64, 256):
        ctx.set_option(R.OPT_QUERY_LOAD, load)
        _assert_equal(ctx.query_rays(rays), want, "load %d/16" % load)
        cells[load] = ctx.get_option(R.STAT_QUERY_GRID_CELLS)
    ctx.set_option(R.OPT_QUERY_LOAD, 0)
    assert cells[8] > cells[64] > cells[256] >= 1
