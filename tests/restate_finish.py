"""Per-object surface finish (include/rtx.h at rtx_scene_set_finish; csrc/rtx_finish.hpp) restated in numpy on top of
tests/restate.py: one float32 operation per IEEE operation of the kernels, no GPU, no torch.
  * shade_lights_finish: restate._shade_lights with ka, kd, ks and the exponent 2^m per pixel;
  * shade_chain_finish: restate.shade_chain / restate_shadows.shade_chain_dark's fold with each level shaded under the finish of
    the object it hit (lev["gid"]); it takes the traces of restate.trace_chain, restate_pattern.patterned and
    restate_glass.trace_chain_glass as they are;
  * `wrong=` restates one bug a kernel could have, for tests/test_host_restate_finish.py to show that scene F would let it be seen;
  * scene F: restate.chain_scene("mirror_floor") with four finishes that are not the default.
tests/test_host_restate_finish.py states the input conditions of the GPU tests on this file alone."""
import numpy as np

import restate as RS

f32 = np.float32

DEFAULT = (0.2, 1.0, 1.0, 5)  # the reference's call-site constants: what every new object has
WRONG = ("kd_on_od", "kd_in_power", "ks_in_power", "m+1", "powf32", "sum_order")

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


def level_local(trace, lights, finishes, j, dark=0, wrong=None):
    """local_j of every pixel as full-size arrays under the finish of the object level j hit; j >= 1: black where level j does not
    exist or hit nothing.  `dark`: an int, or an array over the trace's pixels."""
    lev = trace["levels"][j]
    d = np.asarray(dark)
    if d.ndim:
        d = d[lev["idx"]]
    with np.errstate(all="ignore"):
        sh = shade_lights_finish(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights, finish_arrays(finishes, lev["gid"]), d, wrong)
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


def shade_plain_finish(trace, lights, finishes, dark0=0):
    """The colour floats of a frame without mirrors: level 0 alone."""
    return level_local(trace, lights, finishes, 0, dark0)


_cache = {}


def scene_f(name="mirror_floor"):
    """(params, spheres, planes, ks, pixels, trace) of scene F (or of its shadow twin, whose floor keeps 0.4 of its own colour),
    traced once per process."""
    if name not in _cache:
        p, sph, pl, ks, pix = RS.chain_scene(name)
        _cache[name] = (p, sph, pl, ks, pix, RS.trace_chain(p, sph, pl, ks, pix))
    return _cache[name]
