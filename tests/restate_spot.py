"""Spot lights (include/rtx.h at rtx_scene_set_spots; csrc/rtx_spot.hpp, csrc/rtx_lights.hpp) restated in numpy on top of
tests/restate.py, tests/restate_finish.py and tests/restate_glass.py: one float32 operation per IEEE operation of the kernels, no
GPU, no torch.
  * stored: what rtx_scene_set_spots keeps of a cone -- the axis normalised in double, the two cosines, inv by one fp32 division;
  * weight: w of the rule for the lightDir the shading forms; shade_lights_spot: restate_finish.shade_lights_finish with both
    powers of light i times w_i (with the default finish and no cone it is restate._shade_lights bit for bit);
  * shade_chain_spot / shade_plain_spot: restate_finish.shade_chain_finish's fold with every level shaded under the cones;
  * dark_sets_spot: restate_glass.dark_sets with the lights a point lies outside the cone of (s not above 0) added -- the kernels
    do not test those segments, and a dark light enters with the float dpow * 0.0f is;
  * `wrong=` restates one bug a kernel could have, for tests/test_host_restate_spot.py to show that the scene would let it be seen;
  * the scene: restate.chain_scene("mirror_floor_shadows") under restate.shadow_lights(name, 3), each light a cone aimed from the
    light at one point (CONES).
tests/test_host_restate_spot.py states the input conditions of the GPU tests on this file alone."""
import math

import numpy as np

import restate as RS
import restate_finish as RF
import restate_glass as RG

f32 = np.float32

WRONG = ("axis_not_negated", "inner_for_outer", "linear", "level0_only", "light0_weight", "diffuse_only")

SCENE = "mirror_floor_shadows"
# per light of restate.shadow_lights(SCENE, 3): the point the cone is aimed at, the outer and the inner angle in degrees
CONES = [((0.0, 2.0, 32.0), 14.0, 8.0), ((-6.0, 0.0, 28.0), 20.0, 12.0), ((8.0, 0.0, 34.0), 16.0, 15.0)]


def cone(light, target, outer_deg, inner_deg):
    """The rtx_spot (dir, cos_outer, cos_inner) of a cone aimed from `light` at `target`: what a caller hands rtx_scene_set_spots."""
    d = tuple(float(f32(target[k]) - f32(light.pos[k])) for k in range(3))
    return (d, float(f32(math.cos(math.radians(outer_deg)))), float(f32(math.cos(math.radians(inner_deg)))))


def scene_cones(lights, cones=CONES):
    return [cone(l, *c) for l, c in zip(lights, cones)]


def is_point(spot):
    return spot is None or all(float(v) == 0.0 for v in spot[0])


def stored(spot):
    """(ax, ay, az, cos_outer, cos_inner, inv) as float32, or None for a point light."""
    if is_point(spot):
        return None
    d = np.array(spot[0], dtype=np.float32).astype(np.float64)
    length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    a = (d / length).astype(np.float32)
    co, ci = f32(spot[1]), f32(spot[2])
    return (a[0], a[1], a[2], co, ci, f32(1.0) / (ci - co))


def edge(ld, sp, wrong=None):
    """s of the rule per pixel for the unit directions ld towards the light; sp = stored(spot), not None."""
    ax, ay, az, co, ci, inv = sp
    m = (ax * ld[0] + ay * ld[1]) + az * ld[2]
    c = m if wrong == "axis_not_negated" else -m
    x = (c - (ci if wrong == "inner_for_outer" else co)) * inv
    with np.errstate(invalid="ignore"):
        return np.where(x > f32(0.0), np.where(x < f32(1.0), x, f32(1.0)), f32(0.0)).astype(np.float32)


def weight(ld, sp, wrong=None):
    """w of the rule per pixel; exactly 1 for a point light (sp None)."""
    if sp is None:
        return np.ones(np.shape(ld[0]), dtype=np.float32)
    s = edge(ld, sp, wrong)
    if wrong == "linear":
        return s
    return ((s * s) * (f32(3.0) - f32(2.0) * s)).astype(np.float32)


def light_dirs(O3, D, t, lights):
    """Per light the shading's lightDir after its normalise, for the points O + D t."""
    point = tuple(O3[k] + D[k] * t for k in range(3))
    return [RS._nrm(*(f32(l.pos[k]) - point[k] for k in range(3))) for l in lights]


def shade_lights_spot(O3, D, t, normal, od, lights, spots, fin, dark=0, wrong=None):
    """restate_finish.shade_lights_finish with the powers of light i replaced by dpow_i * w_i and spow_i * w_i.  spots: a list of
    rtx_spot tuples (or None) per light, or None: no cones."""
    assert wrong is None or wrong in WRONG
    ka, kd, ks, m = fin
    dark = np.asarray(dark).astype(np.int64)
    sps = [stored(s) for s in spots] if spots is not None else [None] * len(lights)
    point = tuple(O3[k] + D[k] * t for k in range(3))
    view = RS._nrm(*(D[k] * f32(-1.0) for k in range(3)))
    nn = RS._nrm(*normal)
    nv = RS._nrm(*view)
    res = [ka * od[k] for k in range(3)]
    w0 = None
    for i, l in enumerate(lights):
        lit = ((dark >> i) & 1) == 0
        dpow = np.where(lit, f32(l.diffuse_power), f32(0.0)).astype(np.float32)
        spow = np.where(lit, f32(l.specular_power), f32(0.0)).astype(np.float32)
        ld = tuple(f32(l.pos[k]) - point[k] for k in range(3))
        dist = np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])
        dist = dist * dist
        divd = f32(1.0) / dist
        ld = RS._nrm(*ld)
        w = weight(ld, sps[i], wrong)
        if wrong == "light0_weight":
            w0 = w if i == 0 else w0
            w = w0
        dpow = dpow * w
        if wrong != "diffuse_only":
            spow = spow * w
        di = np.clip(RS._dot(nn, ld), f32(0.0), f32(1.0))
        h = RS._nrm(ld[0] + nv[0], ld[1] + nv[1], ld[2] + nv[2])
        si = RF.power(np.clip(RS._dot(nn, h), f32(0.0), f32(1.0)), m)
        for k in range(3):
            diffuse = ((f32(l.diffuse_rgb[k]) * di) * dpow) * divd
            spec = (((f32(l.specular_rgb[k]) * si) * spow) * divd) * ks
            res[k] = (res[k] + (diffuse * kd) * od[k]) + spec
    out = []
    for k in range(3):
        r = res[k] * f32(255.0)
        out.append(np.where(f32(255.0) < r, f32(255.0), r).astype(np.float32))
    return out


def level_local(trace, lights, spots, finishes, j, dark=0, wrong=None):
    """local_j of every pixel as full-size arrays under the cones; j >= 1: black where level j does not exist or hit nothing."""
    lev = trace["levels"][j]
    d = np.asarray(dark)
    if d.ndim:
        d = d[lev["idx"]]
    if wrong == "level0_only" and j >= 1:
        spots = None
    with np.errstate(all="ignore"):
        sh = shade_lights_spot(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights, spots, RF.level_finish(trace, finishes, j), d, wrong)
    if j == 0:
        return sh
    loc = [np.zeros(trace["n"], dtype=np.float32) for _ in range(3)]
    for q in range(3):
        loc[q][lev["idx"]] = np.where(lev["gid"] >= 0, sh[q], f32(0.0))
    return loc


def shade_chain_spot(trace, lights, spots, finishes=None, dark0=0, deep_dark=None, wrong=None, depths=None):
    """The colour floats of every pixel of `trace` at depths 1 .. max_depth (or `depths`), {depth: [r, g, b]}:
    restate_finish.shade_chain_finish's fold with each level shaded under the cones.  dark0 / deep_dark as there."""
    L = trace["levels"]
    top = max(depths) if depths else trace["max_depth"]
    local = [level_local(trace, lights, spots, finishes, j, dark0 if j == 0 else (0 if deep_dark is None else deep_dark[j - 1]), wrong)
             for j in range(top + 1)]
    k = [L[0]["k"]]
    for lev in L[1:top + 1]:
        kj = np.zeros(trace["n"], dtype=np.float32)
        kj[lev["idx"]] = lev["k"]
        k.append(kj)
    out = {}
    for depth in (depths or range(1, top + 1)):
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


def shade_plain_spot(trace, lights, spots, finishes=None, dark0=0, wrong=None):
    """The colour floats of a frame without mirrors: level 0 alone."""
    return level_local(trace, lights, spots, finishes, 0, dark0, wrong)


def level_weights(trace, lights, spots, j):
    """[w_i over lev["idx"]] per light at level j."""
    lev = trace["levels"][j]
    with np.errstate(all="ignore"):
        lds = light_dirs(lev["O"], lev["D"], lev["t"], lights)
        return [weight(lds[i], stored(spots[i])) for i in range(len(lights))]


def outside_sets(trace, lights, spots):
    """Per level, per pixel: the lights (bit i) whose cone the level's hit point lies outside of -- the rule's s is not above 0."""
    out = []
    for lev in trace["levels"]:
        d = np.zeros(trace["n"], dtype=np.int64)
        with np.errstate(all="ignore"):
            lds = light_dirs(lev["O"], lev["D"], lev["t"], lights)
            for i, sp in enumerate(spots or []):
                st = stored(sp)
                if st is not None:
                    d[lev["idx"]] |= (~(edge(lds[i], st) > f32(0.0)) & (lev["gid"] >= 0)).astype(np.int64) << i
        out.append(d)
    return out


def dark_sets_spot(trace, lights, spots, deep):
    """restate_glass.dark_sets with the out-of-cone lights added at the levels it tests (level 0 within the far distance; the deeper
    levels only when `deep`)."""
    dark = RG.dark_sets(trace, lights, deep)
    outside = outside_sets(trace, lights, spots)
    out = []
    for j, d in enumerate(dark):
        if j == 0:
            lev = trace["levels"][0]
            ok = (lev["gid"] >= 0) & trace["vis"] & (lev["t"] <= f32(trace["p"].cam_far))
            out.append(d | np.where(ok, outside[0], 0))
        else:
            out.append(d | outside[j] if deep else d)
    return out


def classes(trace, lights, spots, j):
    """Per light (w = 0, 0 < w < 1, w = 1) over the hit pixels of level j."""
    lev = trace["levels"][j]
    hit = lev["gid"] >= 0
    out = []
    for w in level_weights(trace, lights, spots, j):
        w = w[hit]
        out.append((int((w == 0).sum()), int(((w > 0) & (w < 1)).sum()), int((w == 1).sum())))
    return out


_cache = {}


def scene(name=SCENE):
    """(params, spheres, planes, ks, pixels, trace, trace without mirrors) of the scene, traced once per process."""
    if name not in _cache:
        p, sph, pl, ks, pix, trace = RF.scene_f(name)
        _cache[name] = (p, sph, pl, ks, pix, trace, RS.trace_chain(p, sph, pl, {}, pix, max_depth=1))
    return _cache[name]
