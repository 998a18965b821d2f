"""Objects that cast no shadow (rtx_scene_set_shadow_casting) restated: plain numpy on top of tests/restate_shadows.py, no GPU, no
torch.  The rule (include/rtx.h) changes one thing in the shadow test: which objects count as occluders.  So:
  * classify64_points: restate_shadows.classify64_points with a `casts` mask by creation index -- the same float64 decision over the
    objects that cast, the owner excluded as before (its self-shadow, the dot <= 0 test, stays whatever its flag);
  * level_sets: restate_shadows.level_sets under the mask;
  * even_spheres: the mask the tests use, U = the even-numbered spheres cast no shadow;
  * oracle_scene, seen_alike: the scene of the GPU tests' second oracle (non-casting = removed wherever both scenes are seen alike)
    and the CPU trace's count of such pixels;
  * lit_again: the (point, light) pairs the mask lights again, and the ambiguous ones, per scene."""
import numpy as np

import oracle as O
import restate as RS
import restate_shadows as RH


def classify64_points(P, N, owner_gid, sph, pl, light_pos, casts, rel=1e-5):
    """restate_shadows.classify64_points over the objects whose `casts` entry (creation index: spheres first, then planes) is not 0.
    With all ones it is that function, argument for argument."""
    sph, pl = np.asarray(sph).reshape(-1, 7), np.asarray(pl).reshape(-1, 11)
    casts = np.asarray(casts).astype(bool)
    ns, n = len(sph), len(sph) + len(pl)
    assert casts.shape == (n,)
    # the creation index of a casting object among the casting objects; -1 for an owner that does not cast (nothing to exclude)
    new_of = np.full(n + 1, -1, dtype=np.int64)
    new_of[np.flatnonzero(casts)] = np.arange(int(casts.sum()))
    owner = np.asarray(owner_gid).astype(np.int64)
    owner = new_of[np.where((owner >= 0) & (owner < n), owner, n)]
    return RH.classify64_points(P, N, owner, sph[casts[:ns]], pl[casts[ns:]], light_pos, rel)


def level_sets(trace, lights, depth, casts):
    """restate_shadows.level_sets with the mask: per level j = 0 .. depth the dicts it returns (tested, dset, decided, facing_dark,
    ambiguous)."""
    out = []
    for j in range(depth + 1):
        idx, P, N, owner = RH.level_points(trace, j)
        n = trace["n"]
        tested = np.zeros(n, dtype=bool)
        tested[idx] = True
        dset = np.zeros(n, dtype=np.int64)
        decided = np.ones(n, dtype=bool)
        facing_dark = np.zeros(n, dtype=bool)
        amb = 0
        for i, l in enumerate(lights):
            k = classify64_points(P, N, owner, trace["sph"], trace["pl"], l.pos, casts)
            dset[idx] |= (k == 1).astype(np.int64) << i
            decided[idx] &= k >= 0
            amb += int((k == -1).sum())
            faces = np.einsum("nk,nk->n", N.astype(np.float64), np.array(l.pos, dtype=np.float64) - P.astype(np.float64)) > 0
            facing_dark[idx] |= (k == 1) & faces
        out.append(dict(tested=tested, dset=dset, decided=decided, facing_dark=facing_dark, ambiguous=amb))
    return out


def even_spheres(ns, n_planes):
    """U: the even-numbered spheres cast no shadow; every other object does."""
    casts = np.ones(ns + n_planes, dtype=np.uint8)
    casts[0:ns:2] = 0
    return casts


_sets = {}


def sets(name, nl, depth):
    """(trace, lights, casts, level_sets under all ones, level_sets under U) of a scene of restate_shadows, once per process."""
    key = (name, nl, depth)
    if key not in _sets:
        trace, ls, full = RH.sets(name, nl, depth)
        casts = even_spheres(len(trace["sph"]), len(trace["pl"]))
        _sets[key] = (trace, ls, casts, full, level_sets(trace, ls, depth, casts))
    return _sets[key]


def lit_again(name, nl, depth):
    """Over the levels 0 .. depth of a scene under its nl lights and U: (tested pairs, pairs dark with every object casting and lit
    under U -- both decided --, ambiguous pairs under either mask, pixels whose dark set at some level differs)."""
    trace, ls, casts, full, masked = sets(name, nl, depth)
    tested = lit = 0
    differ = np.zeros(trace["n"], dtype=bool)
    for a, b in zip(full, masked):
        tested += int(a["tested"].sum()) * nl
        both = a["decided"] & b["decided"]
        gone = a["dset"] & ~b["dset"]
        lit += sum(int((((gone >> i) & 1) != 0)[both].sum()) for i in range(nl))
        differ |= both & (a["dset"] != b["dset"])
    amb = max(sum(l["ambiguous"] for l in full), sum(l["ambiguous"] for l in masked))
    return tested, lit, amb, differ


# ---------------------------------------------------------------- the second oracle's scene

ORACLE_W, ORACLE_H = 160, 90


def oracle_scene():
    """(params, spheres, planes, U): the default spheres over a floor, seen from above, and a lid -- a plane above the scene, under
    the lights, facing down; U = the even-numbered spheres and the lid."""
    # (the camera high and far back: the lid is out of view and the spheres are small, so that most pixels see the same object with
    # and without U; from the first light of restate_shadows' wall scene, (4, 45, 12), the lid's shadow covers the whole floor)
    p = O.camera_params(ORACLE_W, ORACLE_H, pos=(0.0, 30.0, -30.0), rot=(0.4, RS.PI32, 0.0))
    floor = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 70, 70]], dtype=np.float32)
    lid = np.array([[4, 30, 16, 0, -1, 0, 90, 120, 150, 30, 30]], dtype=np.float32)
    pl = np.concatenate([floor, lid])
    ns = len(RS.DEFAULT_SPH)
    return p, RS.DEFAULT_SPH, pl, list(range(0, ns, 2)) + [ns + 1]


def seen_alike():
    """(visible pixels of scene A, those of them whose level-0 distance and normal are bit-equal in scene B = A without U), by the
    CPU trace."""
    p, sph, pl, u = oracle_scene()
    pix = np.arange(ORACLE_W * ORACLE_H)
    keep_s = [i for i in range(len(sph)) if i not in u]
    keep_p = [i for i in range(len(pl)) if i + len(sph) not in u]
    a = RS.trace_chain(p, sph, pl, {}, pix)
    b = RS.trace_chain(p, sph[keep_s], pl[keep_p], {}, pix)
    la, lb = a["levels"][0], b["levels"][0]
    alike = la["t"].view(np.uint32) == lb["t"].view(np.uint32)
    for q in range(3):
        alike &= la["normal"][q].view(np.uint32) == lb["normal"][q].view(np.uint32)
    return int(a["vis"].sum()), int((alike & a["vis"]).sum())
