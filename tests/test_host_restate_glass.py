"""tests/restate_glass.py judged on the CPU, so that tests/test_gpu_glass.py cannot pass vacuously: with every ior 0 it is
restate.trace_chain bit for bit; the two scenes of the GPU tests have refracted rays at levels 1 to 3, glass rays that reach the
(patterned) floor and a mirror, a glass sphere seen in a mirror, chords that depend on the radius, and shadows at every level; and
the closed form of the rule agrees with two float64 Snell refractions along the chains of scene A."""
import numpy as np
import pytest

import restate as RS
import restate_glass as RG
import restate_pattern as RP

f32 = np.float32


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and bool(RS.same_floats(a, b).all())
    return np.array_equal(a, b)


@pytest.mark.parametrize("name", ["default", "mirror_floor", "directed"])
def test_every_ior_zero_is_trace_chain_bit_for_bit(name):
    p, sph, pl, ks, pix = RS.chain_scene(name)
    pix = pix[::7]
    want = RS.trace_chain(p, sph, pl, ks, pix)
    got = RG.trace_chain_glass(p, sph, pl, ks, {}, pix)
    assert got["rays"] == want["rays"] and want["rays"][1] > 0
    for key in ("t", "gid", "sv", "hit", "vis"):
        assert _same(got[key], want[key]), key
    for q in range(3):
        assert _same(got["normal"][q], want["normal"][q])
    for j, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        for key in w:
            if isinstance(w[key], (tuple, list)):
                for q in range(3):
                    assert _same(g[key][q], w[key][q]), (j, key, q)
            else:
                assert _same(g[key], w[key]), (j, key)
        if j >= 1:
            assert not g["glass"].any()


@pytest.mark.parametrize("scene", ["a", "b"])
def test_refracted_rays_at_levels_1_to_3(scene):
    trace = getattr(RG, "scene_" + scene)()[6]
    for j in (1, 2, 3):
        lev = trace["levels"][j]
        assert lev["glass"].sum() >= 1 and (lev["glass"] & (lev["gid"] >= 0)).sum() >= 1, (scene, j)
    # mirrored rays beside them: both cases of the rule are in every frame
    assert (~trace["levels"][1]["glass"]).sum() >= 10


def test_scene_a_input_conditions():
    p, sph, pl, ks, iors, pix, trace = RG.scene_a()
    ns = len(sph)
    L = trace["levels"]
    # every kind of glass object is left by a refracted ray: ior 1.0, 1.5, 4.0 and the sheet
    left = set()
    for lev in L[1:]:
        left |= set(np.unique(lev["left"][lev["glass"]]).tolist())
    assert left == {0, 1, 2, RG.A_SHEET}
    # a glass ray reaches the patterned floor, in cells of both parities
    table, slots = RP.SCENE_A_TABLE[:1], RP.slot_array({RG.A_FLOOR: 1}, ns + len(pl))
    l1 = L[1]
    on_floor = l1["glass"] & (l1["gid"] == RG.A_FLOOR)
    _, is_odd = RP.level_parity(l1, table, slots)
    assert (on_floor & is_odd).sum() >= 20 and (on_floor & ~is_odd).sum() >= 20
    # a glass ray reaches a mirror, and the mirror's ray goes on
    assert (l1["glass"] & (l1["gid"] == RG.A_MIRROR)).sum() >= 20
    assert (L[2]["left"] == RG.A_MIRROR).sum() >= 20
    # a glass sphere is seen in a mirror: a mirrored ray hits it, and the next level leaves it refracted
    seen = sum(int((~lev["glass"] & np.isin(lev["gid"], [0, 1, 2])).sum()) for lev in L[1:])
    assert seen >= 20
    assert (~L[2]["glass"] & np.isin(L[2]["gid"], [0, 1, 2])).sum() >= 10 and (L[3]["glass"] & np.isin(L[3]["left"], [0, 1, 2])).sum() >= 10
    # both k of the glass spheres show: 0.3 and 1.0
    assert {float(v) for v in np.unique(L[0]["k"][np.isin(L[0]["gid"], [0, 1])])} == {1.0, float(f32(0.3))}
    # the colours differ from the same scene with mirrors only on a sixth of the frame at least
    mirrors = RS.trace_chain(p, sph, pl, ks, pix)
    cg = RS.shade_chain(trace, [RS.reference_light()])[4]
    cm = RS.shade_chain(mirrors, [RS.reference_light()])[4]
    differs = np.logical_or.reduce([cg[q] != cm[q] for q in range(3)]) & trace["vis"]
    assert differs.sum() >= 150


def test_the_chord_follows_the_radius():
    p, sph, pl, ks, iors, pix, trace = RG.scene_a()
    edited = sph.copy()
    edited[0, 3] = 3.25
    other = RG.trace_chain_glass(p, edited, pl, ks, iors, pix)
    a, b = RS.shade_chain(trace, [RS.reference_light()])[2], RS.shade_chain(other, [RS.reference_light()])[2]
    assert (np.logical_or.reduce([a[q] != b[q] for q in range(3)]) & trace["vis"]).sum() >= 10  # (the sphere covers some 20 pixels)
    # rays leave the edited sphere through its far side: the chord is 2 r ct with the new r
    l0, l1 = other["levels"][0], other["levels"][1]
    sel = l1["glass"] & (l1["left"] == 0)
    assert sel.sum() >= 5
    P = [(l0["O"][q] + l0["D"][q] * l0["t"])[l1["idx"][sel]] for q in range(3)]
    chord = np.sqrt(sum((l1["O"][q][sel].astype(np.float64) - P[q]) ** 2 for q in range(3)))
    assert (chord > 0.5 * 3.25).all() and (chord <= 2 * 3.25 * (1 + 1e-6)).all()


@pytest.mark.parametrize("nl", [1, 3])
def test_shadows_are_in_the_picture_at_every_level(nl):
    trace = RG.scene_a()[6]
    dark = RG.dark_sets(trace, RG.lights_a(nl), True)
    assert len(dark) == 5
    for j in (0, 1, 2):
        lev = trace["levels"][j]
        tested = np.zeros(trace["n"], dtype=bool)
        tested[lev["idx"][lev["gid"] >= 0]] = True
        assert (dark[j][tested] != 0).sum() >= 10 and (dark[j][tested] == 0).sum() >= 10, j
        assert not dark[j][~tested].any()
    # a point behind glass is shadowed by it: glass occludes like any object
    l1 = trace["levels"][1]
    behind = l1["glass"] & (l1["gid"] == RG.A_FLOOR)
    assert (dark[1][l1["idx"][behind]] != 0).sum() >= 5


def test_the_closed_form_agrees_with_two_snell_refractions_in_float64():
    """Along scene A's chains: every ray that leaves a glass sphere against float64 -- refract at entry, intersect the sphere,
    refract at exit.  The fp32 inputs (P, N, V) are taken as exact; the bound is the issue's figures for fp32 (3.1e-6 of r for the
    exit point, 2.0e-6 for the direction) times four."""
    p, sph, pl, ks, iors, pix, trace = RG.scene_a()
    ii = RS.k_array(iors, len(sph) + len(pl))
    worst_o = worst_d = 0.0
    n_checked = 0
    for j in range(1, 4):
        prev, lev = trace["levels"][j - 1], trace["levels"][j]
        sel = lev["glass"] & (lev["left"] < len(sph))
        if not sel.any():
            continue
        pos = np.searchsorted(prev["idx"], lev["idx"][sel])
        with np.errstate(all="ignore"):
            Nf = RS._nrm(*(prev["normal"][q][pos] for q in range(3)))
            Vf = RS._nrm(*(prev["D"][q][pos] * f32(-1.0) for q in range(3)))
            Pf = tuple(prev["O"][q][pos] + prev["D"][q][pos] * prev["t"][pos] for q in range(3))
        N, V, P = (np.stack(x, axis=1).astype(np.float64) for x in (Nf, Vf, Pf))
        obj = lev["left"][sel]
        r = sph[obj, 3].astype(np.float64)
        C = P - N * r[:, None]  # the centre the normal points away from
        eta = 1.0 / ii[obj].astype(np.float64)
        ci = np.einsum("nk,nk->n", N, V)
        keep = ci >= 0.05
        ct = np.sqrt(1.0 - eta * eta * (1.0 - ci * ci))
        T = N * (eta * ci - ct)[:, None] - V * eta[:, None]
        T /= np.linalg.norm(T, axis=1)[:, None]
        # the chord: P + T s on the sphere again
        s = -2.0 * np.einsum("nk,nk->n", P - C, T)
        X = P + T * s[:, None]
        N2 = -(X - C) / r[:, None]  # the normal against the ray inside
        e2 = ii[obj].astype(np.float64)
        c2 = -np.einsum("nk,nk->n", N2, T)
        k2 = 1.0 - e2 * e2 * (1.0 - c2 * c2)
        assert (k2[keep] > 0).all()  # no total internal reflection
        Dout = T * e2[:, None] + N2 * (e2 * c2 - np.sqrt(np.maximum(k2, 0.0)))[:, None]
        got_o = np.stack([lev["O"][q][sel] for q in range(3)], axis=1).astype(np.float64)
        got_d = np.stack([lev["D"][q][sel] for q in range(3)], axis=1).astype(np.float64)
        worst_o = max(worst_o, float((np.linalg.norm(got_o - X, axis=1) / r)[keep].max()))
        worst_d = max(worst_d, float(np.linalg.norm(got_d - Dout, axis=1)[keep].max()))
        n_checked += int(keep.sum())
    print("checked %d rays: exit point %.3g of r, direction %.3g" % (n_checked, worst_o, worst_d))
    assert n_checked >= 200
    assert worst_o <= 4 * 3.1e-6 and worst_d <= 4 * 2.0e-6
