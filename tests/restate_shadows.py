"""Shadows seen in mirrors (RTX_OPT_REFLECT_SHADOWS) restated: plain numpy on top of tests/restate.py, no GPU, no torch.
  * shade_chain_dark: restate.shade_chain with a set of dark lights per LEVEL (include/rtx.h at RTX_OPT_REFLECT_SHADOWS: local_j is
    the Blinn-Phong colour with the lights level j is shadowed from at both powers 0; the fold is unchanged);
  * classify64_points: tests/test_gpu_lights.py::classify64's float64 decision at given points, the owner given, not guessed;
  * level_sets: per level of a traced chain the set of lights float64 puts each hit point in shadow from;
  * the scenes and lights tests/test_host_reflect_shadows.py states its input conditions on and tests/test_gpu_reflect_shadows.py
    renders."""
import itertools

import numpy as np

import oracle as O
import restate as RS

f32 = np.float32

# ---------------------------------------------------------------- the colour under a dark set per level


def _level_local(trace, lights, j, S):
    """local_j of every pixel (full-size arrays) with the lights of S at both powers 0; j >= 1: black where level j hit nothing
    or does not exist.  Cached per (level, set) for one light set at a time."""
    key = tuple(RS.light_tuple(l) for l in lights)
    cache = trace.setdefault("_dark_locals", {})
    if cache.get("key") != key:
        cache.clear()
        cache["key"] = key
    if (j, S) not in cache:
        lev = trace["levels"][j]
        ls = [RS.dark(l) if (S >> i) & 1 else l for i, l in enumerate(lights)]
        with np.errstate(all="ignore"):
            sh = RS._shade_lights(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], ls)
        if j == 0:
            cache[(j, S)] = sh
        else:
            loc = [np.zeros(trace["n"], dtype=np.float32) for _ in range(3)]
            for q in range(3):
                loc[q][lev["idx"]] = np.where(lev["gid"] >= 0, sh[q], f32(0.0))
            cache[(j, S)] = loc
    return cache[(j, S)]


def _local_under(trace, lights, j, d):
    """local_j with the per-pixel (array) or common (int) dark set d."""
    if np.isscalar(d) or np.ndim(d) == 0:
        return _level_local(trace, lights, j, int(d))
    d = np.asarray(d).astype(np.int64)
    out = [np.zeros(trace["n"], dtype=np.float32) for _ in range(3)]
    for S in np.unique(d):
        loc = _level_local(trace, lights, j, int(S))
        m = d == S
        for q in range(3):
            out[q][m] = loc[q][m]
    return out


def shade_chain_dark(trace, lights, dark):
    """restate.shade_chain with a set of dark lights per level: dark[j], j = 0 .. max_depth, is an int (bit i: light i) or an array
    of them per pixel of the trace; level j is shaded with those lights at both powers 0.  {depth: [r, g, b]}.  With
    dark = [S, 0, 0, 0, 0] this is shade_chain(trace, lights, dark0=S) bit for bit."""
    L = trace["levels"]
    assert len(dark) >= trace["max_depth"] + 1
    local = [_local_under(trace, lights, j, dark[j]) for j in range(trace["max_depth"] + 1)]
    k = [L[0]["k"]]
    for lev in L[1:]:
        kj = np.zeros(trace["n"], dtype=np.float32)
        kj[lev["idx"]] = lev["k"]
        k.append(kj)
    out = {}
    for depth in range(1, trace["max_depth"] + 1):
        C = [x.copy() for x in local[depth]]
        for j in range(depth - 1, -1, -1):
            kj, wj = k[j], f32(1.0) - k[j]
            nxt = L[j + 1]["exists"]
            folded = []
            for q in range(3):
                with np.errstate(all="ignore"):
                    v = local[j][q] * wj + C[q] * kj
                v = np.where(f32(255.0) < v, f32(255.0), v).astype(np.float32)
                folded.append(np.where(nxt, v, local[j][q]))
            C = folded
        out[depth] = C
    return out


def combinations(nl, depth):
    """Every assignment of a dark set to levels 0 .. depth: tuples of depth + 1 ints below 2^nl."""
    return list(itertools.product(range(1 << nl), repeat=depth + 1))


# ---------------------------------------------------------------- float64 decides


def classify64_points(P, N, owner_gid, sph, pl, light_pos, rel=1e-5):
    """tests/test_gpu_lights.py::classify64's decision at the points P (n, 3) with normals N (n, 3), each on the object owner_gid
    (creation index: spheres first, then planes), which is excluded from its own test: 1 shadowed, 0 lit, -1 ambiguous (within the
    tolerance band of some test).  No far limit and no visibility enter: the caller selects the points."""
    P, N = np.asarray(P, dtype=np.float64).reshape(-1, 3), np.asarray(N, dtype=np.float64).reshape(-1, 3)
    owner = np.asarray(owner_gid).astype(np.int64)
    sph64, pl64 = np.asarray(sph, dtype=np.float64).reshape(-1, 7), np.asarray(pl, dtype=np.float64).reshape(-1, 11)
    L = np.array(light_pos, dtype=np.float64)
    toL = L - P
    seg = np.linalg.norm(toL, axis=-1)
    scale = seg + 1e-9
    s_self = np.einsum("nk,nk->n", N, toL)
    shadow = s_self <= 0
    amb = np.abs(s_self) < rel * scale
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
    out = np.zeros(len(P), dtype=np.int64)
    out[shadow] = 1
    out[amb] = -1
    return out


def level_points(trace, j):
    """The hit points of level j the rule tests: (idx into the trace's pixels, P, N, owner) for the pixels whose level j exists and
    hit an object -- and, at level 0, is visible within the far distance.  P = O + D t in fp32, as shade_lights forms it."""
    lev = trace["levels"][j]
    ok = lev["gid"] >= 0
    if j == 0:
        ok = ok & trace["vis"] & (lev["t"] <= f32(trace["p"].cam_far))
    with np.errstate(all="ignore"):
        P = np.stack([(lev["O"][q] + lev["D"][q] * lev["t"])[ok] for q in range(3)], axis=1)
    N = np.stack([lev["normal"][q][ok] for q in range(3)], axis=1)
    return lev["idx"][ok], P, N, lev["gid"][ok]


def level_sets(trace, lights, depth):
    """Per level j = 0 .. depth, full-size arrays: tested (level j has a point the rule tests), dset (the lights float64 puts it in
    shadow from, 0 elsewhere), decided (every light decided; True where nothing is tested), facing_dark (dark for some light the
    point faces: occlusion by another object, not self-shadow), ambiguous (count of (pixel, light) pairs)."""
    out = []
    for j in range(depth + 1):
        idx, P, N, owner = level_points(trace, j)
        n = trace["n"]
        tested = np.zeros(n, dtype=bool)
        tested[idx] = True
        dset = np.zeros(n, dtype=np.int64)
        decided = np.ones(n, dtype=bool)
        facing_dark = np.zeros(n, dtype=bool)
        amb = 0
        for i, l in enumerate(lights):
            k = classify64_points(P, N, owner, trace["sph"], trace["pl"], l.pos)
            dset[idx] |= (k == 1).astype(np.int64) << i
            decided[idx] &= k >= 0
            amb += int((k == -1).sum())
            faces = np.einsum("nk,nk->n", N.astype(np.float64), np.array(l.pos, dtype=np.float64) - P.astype(np.float64)) > 0
            facing_dark[idx] |= (k == 1) & faces
        out.append(dict(tested=tested, dset=dset, decided=decided, facing_dark=facing_dark, ambiguous=amb))
    return out


# ---------------------------------------------------------------- scenes and lights

SCENES = ["mirror_floor_shadows", "directed", "wall"]
# (lights, depth) of the float64 test: at most 64 combinations of dark sets per pixel
CASES = [(1, 4), (2, 2), (3, 1)]
WALL_POSITIONS = [(4.0, 45.0, 12.0), (-25.0, 35.0, 25.0), (28.0, 40.0, 18.0)]


def scene(name, W=320, H=180):
    """(oracle params, spheres, planes, ks, pixels): restate.chain_scene's two shadow scenes, and `wall` (at any frame size): the
    default spheres over a floor, a reflective vertical plane behind them facing the camera -- its level-1 points lie on the floor,
    inside the spheres' shadows, and on the spheres' far sides."""
    if name != "wall":
        assert (W, H) == (320, 180)
        return RS.chain_scene(name)
    p = O.camera_params(W, H, pos=(0.0, 14.0, -6.0), rot=(0.25, RS.PI32, 0.0))
    floor = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 70, 70]], dtype=np.float32)
    wall = np.array([[0, 10, 58, 0, 0, -1, 140, 150, 160, 70, 4]], dtype=np.float32)
    pl = np.concatenate([floor, wall])
    ns = len(RS.DEFAULT_SPH)
    return p, RS.DEFAULT_SPH, pl, {ns + 1: 0.7, 0: 0.3}, np.arange(W * H)


def lights(name, n):
    if name != "wall":
        return RS.shadow_lights(name, n)
    if n == 1:
        return [RS.CUSTOM_LIGHT._replace(pos=WALL_POSITIONS[0])]
    return RS.light_set(n, positions=WALL_POSITIONS[:n], scale=0.6)


_traced = {}


def traced(name):
    """(params, spheres, planes, ks, pixels, trace) of a scene, traced once per process."""
    if name not in _traced:
        p, sph, pl, ks, pix = scene(name)
        _traced[name] = (p, sph, pl, ks, pix, RS.trace_chain(p, sph, pl, ks, pix))
    return _traced[name]


_sets = {}


def sets(name, nl, depth):
    """level_sets of a scene under its nl lights, once per process: (trace, lights, per-level dicts)."""
    key = (name, nl, depth)
    if key not in _sets:
        trace = traced(name)[5]
        ls = lights(name, nl)
        _sets[key] = (trace, ls, level_sets(trace, ls, depth))
    return _sets[key]
