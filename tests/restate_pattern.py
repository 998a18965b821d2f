"""Checker patterns (include/rtx.h at rtx_scene_set_patterns) restated in numpy, one float32 operation per IEEE operation of
csrc/rtx_pattern.hpp::pattern_odd, and the scenes tests/test_gpu_pattern.py renders.  `patterned` rewrites the `od` of every level
of a restate.trace_chain result; restate.shade_chain and restate_shadows.shade_chain_dark read lev["od"], so they serve unchanged.
tests/test_host_restate_pattern.py states the input conditions of the GPU tests on this file alone."""
import collections

import numpy as np

import restate as RS
import util as U

f32 = np.float32

Pattern = collections.namedtuple("Pattern", "origin freq rgb")

# scene A: restate.chain_scene("mirror_floor") -- spheres 0 .. 3, the floor is object 4 -- with a two-axis checker on the floor and a
# three-axis one on spheres 1 and 3
SCENE_A_TABLE = [Pattern((0.37, 0.0, 0.41), (0.25, 0.0, 0.25), (20.0, 20.0, 20.0)),
                 Pattern((0.13, 0.29, 0.07), (0.5, 0.5, 0.5), (250.0, 250.0, 250.0))]
SCENE_A_SLOTS = {4: 1, 1: 2, 3: 2}
SCENE_A_OBJECTS = (4, 1, 3)


def slot_array(slots, n):
    """slots: {creation index: slot} or an array of n ints -> uint8 array of n."""
    if isinstance(slots, dict):
        out = np.zeros(n, dtype=np.uint8)
        for i, s in slots.items():
            out[i] = s
        return out
    out = np.asarray(slots, dtype=np.uint8)
    assert out.shape == (n,)
    return out


def odd(P, pat):
    """The rule: u_q = (P_q - origin_q) * freq_q; f = (floor(u_x) + floor(u_y)) + floor(u_z); h = f - 2 * floor(f * 0.5); h != 0
    (a NaN h is odd).  P: three float32 arrays."""
    with np.errstate(all="ignore"):
        fl = []
        for q in range(3):
            u = (P[q] - f32(pat.origin[q])) * f32(pat.freq[q])
            fl.append(np.floor(u).astype(np.float32))
        f = (fl[0] + fl[1]) + fl[2]
        h = f - f32(2.0) * np.floor(f * f32(0.5)).astype(np.float32)
        return h != f32(0.0)


def level_parity(lev, table, slots):
    """Per pixel of a level: (slot of the hit object, 0 without a hit or a pattern; whether the hit point's cell is odd)."""
    gid = lev["gid"]
    slot = np.where(gid >= 0, slots[np.maximum(gid, 0)], 0).astype(np.int64)
    with np.errstate(all="ignore"):
        P = tuple((lev["O"][q] + lev["D"][q] * lev["t"]).astype(np.float32) for q in range(3))
    is_odd = np.zeros(len(gid), dtype=bool)
    for s in range(1, len(table) + 1):
        m = slot == s
        if m.any():
            is_odd[m] = odd(tuple(x[m] for x in P), table[s - 1])
    return slot, is_odd


def patterned(trace, table, slots):
    """A copy of a restate.trace_chain result in which every level's od follows the rule: the level's object o_j at its hit point
    P_j = O_j + D_j * t_j.  table: Pattern values (entry i serves slot i + 1); slots: {creation index: slot} or an array."""
    n_obj = len(trace["sph"]) + len(trace["pl"])
    slots = slot_array(slots, n_obj)
    assert slots.max(initial=0) <= len(table)
    out = dict(trace)
    out["_deep"] = {}
    out.pop("_dark_locals", None)
    out["levels"] = []
    for lev in trace["levels"]:
        new = dict(lev)
        slot, is_odd = level_parity(lev, table, slots)
        od = []
        for q in range(3):
            od2 = np.array([f32(0.0)] + [f32(t.rgb[q]) / f32(255.0) for t in table], dtype=np.float32)[slot]
            od.append(np.where((slot > 0) & is_odd, od2, lev["od"][q]).astype(np.float32))
        new["od"] = od
        out["levels"].append(new)
    return out


def parity_counts(trace, table, slots, obj, level):
    """(pixels of `obj` at `level` in even cells, in odd cells): at level 0 the visible ones within the far distance."""
    slots = slot_array(slots, len(trace["sph"]) + len(trace["pl"]))
    lev = trace["levels"][level]
    _, is_odd = level_parity(lev, table, slots)
    m = lev["gid"] == obj
    if level == 0:
        m = m & trace["vis"] & (lev["t"] <= f32(trace["p"].cam_far))
    return int((m & ~is_odd).sum()), int((m & is_odd).sum())


_scene_a = {}


def scene_a():
    """(params, spheres, planes, ks, pixels, trace, patterned trace) of scene A, traced once per process."""
    if not _scene_a:
        p, sph, pl, ks, pix = RS.chain_scene("mirror_floor")
        trace = RS.trace_chain(p, sph, pl, ks, pix)
        _scene_a["v"] = (p, sph, pl, ks, pix, trace, patterned(trace, SCENE_A_TABLE, SCENE_A_SLOTS))
    return _scene_a["v"]


# the sorted-store scene: 300 spheres over a floor (the direction-sorted copies exist from 256 on), slot 2 of scene A's table on
# every sphere whose index is a multiple of 3
SORTED_W, SORTED_H, SORTED_NS = 320, 180, 300
_sorted = {}


def sorted_scene():
    """(params, spheres, planes, slots, trace, patterned trace)."""
    import oracle as O
    if not _sorted:
        p = O.camera_params(SORTED_W, SORTED_H)
        sph, pl = U.numpy_synth_scene(7, SORTED_NS, 1, p.element1, p.element2)
        slots = np.zeros(SORTED_NS + 1, dtype=np.uint8)
        slots[0:SORTED_NS:3] = 2
        trace = RS.trace_chain(p, sph, pl, {}, np.arange(SORTED_W * SORTED_H), max_depth=1)
        _sorted["v"] = (p, sph, pl, slots, trace, patterned(trace, SCENE_A_TABLE, slots))
    return _sorted["v"]
