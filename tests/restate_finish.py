"""Per-object surface finish (include/rtx.h at rtx_scene_set_finish; csrc/rtx_finish.hpp) restated in numpy on top of
tests/restate.py: one float32 operation per IEEE operation of the kernels, no GPU, no torch.
  * shade_lights_finish: restate._shade_lights with ka, kd, ks and the exponent 2^m per pixel;
  * shade_chain_finish: restate.shade_chain / restate_shadows.shade_chain_dark's fold with each level shaded under the finish of
    the object it hit (lev["gid"]); it takes the traces of restate.trace_chain, restate_pattern.patterned and
    restate_glass.trace_chain_glass as they are;
  * `wrong=` restates one bug a kernel could have, for tests/test_host_restate_finish.py to show that scene F would let it be seen;
  * scene F: restate.chain_scene("mirror_floor") with four finishes that are not the default;
  * the inputs of tests/test_gpu_finish_edges.py, where the question is which object's finish a lane reads: C_FINISHES and
    d_finishes() for restate_glass.scene_c() and scene_d(), creation_orders (the same scene created with spheres and planes
    interleaved), scene E (scene F's geometry, dim, with the weights 0 and 16 and every m the other scenes leave out), and WRONG_LOOKUP,
    four lookups a kernel could get wrong.
tests/test_host_restate_finish.py states the input conditions of the GPU tests on this file alone."""
import numpy as np

import restate as RS
import restate_glass as RG

f32 = np.float32

DEFAULT = (0.2, 1.0, 1.0, 5)  # the reference's call-site constants: what every new object has
WRONG = ("kd_on_od", "kd_in_power", "ks_in_power", "m+1", "powf32", "sum_order")
# which finish a level reads, got wrong: every plane reads plane 0's; the levels >= 1 of a chain read that of the object level 0
# hit; sphere i reads that of the sphere at sorted position i (sorted_permutation); m = 8 is shaded as m = 7
WRONG_LOOKUP = ("plane0", "level0", "unsorted", "m_cap7")

# scene F: restate.chain_scene("mirror_floor") with these finishes by creation index; sphere 2 keeps the default.  The weights are
# not powers of two: a power of two commutes with rounding and would hide an association error.
F_FINISHES = {0: (0.2, 1.0, 0.0, 5), 1: (0.1, 0.8, 1.7, 7), 3: (0.8, 0.3, 1.0, 0), 4: (0.3, 1.0, 0.6, 3)}


def finish_arrays(finishes, gid):
    """(ka, kd, ks, m) per pixel from `finishes` ({creation index: (ka, kd, ks, m)}, or None: every object the default) and the
    creation index each pixel hit (-1: none, shaded with the default and thrown away by the caller)."""
    gid = np.asarray(gid)
    n_obj = int(max(gid.max(initial=-1), max(finishes) if finishes else -1)) + 1
    table = np.tile(np.array(DEFAULT, dtype=np.float64), (max(n_obj, 1), 1))
    for i, f in (finishes or {}).items():
        table[i] = f
    rows = table[np.maximum(gid, 0)]
    return rows[:, 0].astype(np.float32), rows[:, 1].astype(np.float32), rows[:, 2].astype(np.float32), rows[:, 3].astype(np.int64)


def power(x, m, in_float=False):
    """x^(2^m), m per pixel: m squarings in double, rounded once to float (in_float: the squarings in float32, a wrong variant)."""
    d = x.astype(np.float32 if in_float else np.float64)
    for s in range(int(m.max(initial=0))):
        d = np.where(s < m, d * d, d)
    return d.astype(np.float32)


def shade_lights_finish(O3, D, t, normal, od, lights, fin, dark=0, wrong=None):
    """The rule of rtx_scene_set_finish: res = ka * od; per light, in order, res = (res + (diffuse_i * kd) * od) + specular_i * ks
    with the 2^m-th power in specular_i; res * 255.0f; minf(255.0f, res).  fin = (ka, kd, ks, m) per pixel; `dark` an int or an
    array per pixel: bit i puts light i in with both powers 0."""
    assert wrong is None or wrong in WRONG
    ka, kd, ks, m = fin
    dark = np.asarray(dark).astype(np.int64)
    point = tuple(O3[k] + D[k] * t for k in range(3))
    view = RS._nrm(*(D[k] * f32(-1.0) for k in range(3)))
    nn = RS._nrm(*normal)
    nv = RS._nrm(*view)
    res = [ka * od[k] for k in range(3)]
    for i, l in enumerate(lights):
        lit = ((dark >> i) & 1) == 0
        dpow = np.where(lit, f32(l.diffuse_power), f32(0.0)).astype(np.float32)
        spow = np.where(lit, f32(l.specular_power), f32(0.0)).astype(np.float32)
        ld = tuple(f32(l.pos[k]) - point[k] for k in range(3))
        dist = np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])
        dist = dist * dist
        divd = f32(1.0) / dist
        ld = RS._nrm(*ld)
        di = np.clip(RS._dot(nn, ld), f32(0.0), f32(1.0))
        h = RS._nrm(ld[0] + nv[0], ld[1] + nv[1], ld[2] + nv[2])
        si = power(np.clip(RS._dot(nn, h), f32(0.0), f32(1.0)), m + 1 if wrong == "m+1" else m, in_float=wrong == "powf32")
        for k in range(3):
            if wrong == "kd_in_power":
                term = (((f32(l.diffuse_rgb[k]) * di) * (dpow * kd)) * divd) * od[k]
            else:
                diffuse = ((f32(l.diffuse_rgb[k]) * di) * dpow) * divd
                term = diffuse * (kd * od[k]) if wrong == "kd_on_od" else (diffuse * kd) * od[k]
            if wrong == "ks_in_power":
                spec = ((f32(l.specular_rgb[k]) * si) * (spow * ks)) * divd
            else:
                spec = (((f32(l.specular_rgb[k]) * si) * spow) * divd) * ks
            res[k] = res[k] + (term + spec) if wrong == "sum_order" else (res[k] + term) + spec
    out = []
    for k in range(3):
        r = res[k] * f32(255.0)
        out.append(np.where(f32(255.0) < r, f32(255.0), r).astype(np.float32))
    return out


def level_finish(trace, finishes, j, wrong=None):
    """(ka, kd, ks, m) per ray of level j: the finish of the object the level hit, or what one of WRONG_LOOKUP would read there."""
    assert wrong is None or wrong in WRONG_LOOKUP
    lev = trace["levels"][j]
    gid = lev["gid"]
    fin = dict(finishes or {})
    ns = len(trace["sph"])
    if wrong == "plane0":
        fin = {i: f for i, f in fin.items() if i < ns}
        if ns in (finishes or {}):
            fin.update({ns + q: finishes[ns] for q in range(len(trace["pl"]))})
    elif wrong == "level0" and j >= 1:
        gid = np.where(gid >= 0, trace["levels"][0]["gid"][lev["idx"]], gid)
    elif wrong == "unsorted":
        perm = sorted_permutation(ns)
        fin = {i: f for i, f in fin.items() if i >= ns}
        fin.update({i: finishes[int(perm[i])] for i in range(ns) if int(perm[i]) in (finishes or {})})
    elif wrong == "m_cap7":
        fin = {i: (f[0], f[1], f[2], min(f[3], 7)) for i, f in fin.items()}
    return finish_arrays(fin, gid)


def level_local(trace, lights, finishes, j, dark=0, wrong=None):
    """local_j of every pixel as full-size arrays under the finish of the object level j hit; j >= 1: black where level j does not
    exist or hit nothing.  `dark`: an int, or an array over the trace's pixels.  `wrong`: one of WRONG (the rule) or of WRONG_LOOKUP
    (which object's finish a level reads)."""
    lev = trace["levels"][j]
    d = np.asarray(dark)
    if d.ndim:
        d = d[lev["idx"]]
    lookup, wrong = (wrong, None) if wrong in WRONG_LOOKUP else (None, wrong)
    with np.errstate(all="ignore"):
        sh = shade_lights_finish(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights, level_finish(trace, finishes, j, lookup), d, wrong)
    if j == 0:
        return sh
    loc = [np.zeros(trace["n"], dtype=np.float32) for _ in range(3)]
    for q in range(3):
        loc[q][lev["idx"]] = np.where(lev["gid"] >= 0, sh[q], f32(0.0))
    return loc


def shade_chain_finish(trace, lights, finishes, dark0=0, deep_dark=None, wrong=None):
    """The colour floats of every pixel of `trace` at depths 1 .. max_depth, {depth: [r, g, b]}: restate.shade_chain's fold, each
    level shaded with the finish of the object it hit.  dark0: the lights level 0 is shadowed from (an int or an array per pixel);
    deep_dark: None (the deeper levels under every light), or the same per level j >= 1 at deep_dark[j - 1] -- so that
    restate_glass.dark_sets' list d goes in as dark0=d[0], deep_dark=d[1:]."""
    L = trace["levels"]
    local = [level_local(trace, lights, finishes, j, dark0 if j == 0 else (0 if deep_dark is None else deep_dark[j - 1]), wrong)
             for j in range(trace["max_depth"] + 1)]
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


def shade_plain_finish(trace, lights, finishes, dark0=0, wrong=None):
    """The colour floats of a frame without mirrors: level 0 alone."""
    return level_local(trace, lights, finishes, 0, dark0, wrong)


_cache = {}


def scene_f(name="mirror_floor"):
    """(params, spheres, planes, ks, pixels, trace) of scene F (or of its shadow twin, whose floor keeps 0.4 of its own colour),
    traced once per process."""
    if name not in _cache:
        p, sph, pl, ks, pix = RS.chain_scene(name)
        _cache[name] = (p, sph, pl, ks, pix, RS.trace_chain(p, sph, pl, ks, pix))
    return _cache[name]


# ---------------------------------------------------------------- which object's finish: the inputs of tests/test_gpu_finish_edges.py

# scene C (restate_glass.scene_c: glass that overlaps, a sphere sunk into the floor, rays that start inside other objects) with a
# finish on every object but sphere 6; the floor and the sheet, planes 0 and 1, carry different ones
C_FINISHES = {0: (0.3, 0.7, 1.4, 3), 1: (0.6, 1.2, 0.3, 0), 2: (0.15, 0.9, 1.1, 7), 3: (0.45, 0.6, 0.7, 6), 4: (0.7, 0.35, 1.3, 2),
              5: (0.1, 1.1, 0.9, 4), 7: (0.35, 0.85, 0.45, 1), RG.C_FLOOR: (0.55, 0.65, 1.6, 3), RG.C_SHEET: (0.05, 1.3, 0.35, 7)}


def power_of_two(v):
    return v > 0.0 and np.frexp(f32(v))[0] == 0.5


def d_finishes():
    """Scene D (restate_glass.scene_d: 300 spheres, the direction-sorted copies exist): a finish on every third sphere and on the
    floor, ka in [0, 1], kd in [0.2, 1.5], ks in [0, 2], m in 0 .. 8, drawn from default_rng(23); no weight a power of two."""
    rng = np.random.default_rng(23)
    out = {}
    for i in list(range(0, RG.D_NS, 3)) + [RG.D_FLOOR]:
        while True:
            f = (float(rng.uniform(0.0, 1.0)), float(rng.uniform(0.2, 1.5)), float(rng.uniform(0.0, 2.0)), int(rng.integers(0, 9)))
            if not any(power_of_two(v) for v in f[:3]):
                break
        out[i] = f
    return out


def sorted_permutation(ns):
    """A fixed permutation of ns spheres, standing for the order of a sorted copy: position i holds sphere sorted_permutation(ns)[i]."""
    return np.random.default_rng(37).permutation(ns)


def creation_orders(ns, npl):
    """Orders to create ns spheres and npl >= 2 planes in that keep the spheres' and the planes' own order -- so the kernels' arrays
    and the restated trace stay as they are -- but interleave them: [(order, index)], order a list of ("s", i) and ("p", q),
    index[restatement's index (spheres first, then planes)] = creation index.
      0: plane 0, the first half of the spheres, plane 1, the other spheres, the other planes;
      1: sphere 0, plane 0, spheres up to a third, plane 1, the other spheres, the other planes."""
    assert ns >= 3 and npl >= 2
    out = []
    for lead, cut in ((0, ns // 2), (1, max(2, ns // 3))):
        order = [("s", i) for i in range(lead)] + [("p", 0)] + [("s", i) for i in range(lead, cut)] + [("p", 1)]
        order += [("s", i) for i in range(cut, ns)] + [("p", q) for q in range(2, npl)]
        index = np.zeros(ns + npl, dtype=np.int64)
        for c, (kind, i) in enumerate(order):
            index[i if kind == "s" else ns + i] = c
        out.append((order, index))
    return out


def by_creation(values, index):
    """{restatement's index: value} as {creation index: value}."""
    return {int(index[i]): v for i, v in values.items()}


# scene E, the ends of the ranges: scene F's geometry with every colour component divided by 24, od <= 0.04, so that a weight of 16
# leaves room below the 255 clamp.  Each of ka, kd and ks is 0 on one object and 16 on one, m takes the values scenes C, D and F
# leave thin; sphere 3's specular weight is given as -0.0 (stored and shaded as +0.0).
E_DIVISOR = 24.0
E_FINISHES = {0: (0.0, 16.0, 0.7, 1), 1: (0.3, 0.9, 1.9, 8), 2: (16.0, 0.0, 0.9, 2), 3: (0.3, 1.1, -0.0, 6), 4: (0.25, 1.3, 16.0, 4)}
E_MINUS_ZERO = 3
E_ENDS = {("ka", 0): 0, ("ka", 16): 2, ("kd", 0): 2, ("kd", 16): 0, ("ks", 0): 3, ("ks", 16): 4}  # (weight, end) -> the object
E_M8 = 1


def scene_e():
    """(params, spheres, planes, ks, pixels, trace, trace without mirrors) of scene E, traced once per process."""
    if "e" not in _cache:
        p, sph, pl, ks, pix = RS.chain_scene("mirror_floor")
        sph, pl = sph.copy(), pl.copy()
        sph[:, 4:7] = sph[:, 4:7] / f32(E_DIVISOR)
        pl[:, 6:9] = pl[:, 6:9] / f32(E_DIVISOR)
        _cache["e"] = (p, sph, pl, ks, pix, RS.trace_chain(p, sph, pl, ks, pix), RS.trace_chain(p, sph, pl, {}, pix, max_depth=1))
    return _cache["e"]
