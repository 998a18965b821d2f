"""tests/grid_cases.py without a GPU: from the float64 side alone, every class of scenes, rays and segments that
tests/test_gpu_grid_check.py runs on the device holds what it is there for, and float64 leaves undecided no more than the GPU file
allows (2 %: of a case's spheres for L3, of its rays and segments outside the classes built on the fp32 tests' threshold for Q)."""
import numpy as np
import pytest

import grid_cases as GC

F32 = np.float32
CAP = 0.02


def _plan(name):
    geom, load = GC.scene(name)
    return geom, load, GC.plan_of(geom, load)


def test_names_and_loads():
    assert set(GC.NAMES) == set(GC.scenes()) and set(GC.WALKED) <= set(GC.NAMES) and set(GC.PRODUCT) <= set(GC.NAMES)
    assert [len(GC.scene(n)[0]) for n in ("n1", "n255", "n256", "n257", "n1025")] == [1, 255, 256, 257, 1025]
    assert max(len(GC.scene(n)[0]) for n in GC.NAMES) == 2048
    for name in GC.PRODUCT:
        assert GC.scene(name)[1] * 16.0 in range(1, 65), name
    for name in GC.WALKED:
        g = _plan(name)[2]
        assert g["ok"] == 1 and int(g["n"].max()) <= 64, (name, g["n"])


def test_cell_counts():
    cells = {n: GC.n_cells(_plan(n)[2]) for n in GC.NAMES}
    assert cells["n1"] == 1 and cells["c1025"] == 1025 and cells["cap"] == 1 << 21, cells
    assert all(1 < cells[n] < 1024 for n in ("n255", "n256", "n257", "dense", "large256")), cells
    assert cells["half"] > 2048
    # the cap's loop: three roundings whose product passes 2^21, one axis halved
    g = _plan("halve")[2]
    assert g["halved"] and (1 << 20) < cells["halve"] <= (1 << 21) and not _plan("cap")[2]["halved"]
    # sort takes at most 4096 workgroups of four waves: a wave per cell up to 16384 cells, the stride loop beyond
    assert cells["cap"] > 16384 and cells["halve"] > 16384 and cells["fine"] > 16384


def test_scales_and_degenerate_boxes():
    for name, lo, hi in (("s1e-6", 1e-6, 2e-5), ("n257", 1.0, 20.0), ("s1e6", 1e6, 2e7)):
        g = _plan(name)[2]
        assert lo < float(g["reach"]) / 3.0 < hi, name
    geom, _, g = _plan("off1e4")
    assert np.abs(g["ctr"]).min() > 9.0e3 and float(g["reach"]) < 20.0
    geom, _, g = _plan("flat")
    assert g["n"][2] == 1 and g["n"][0] > 8 and np.ptp(geom[:, 2]) == 0
    geom, _, g = _plan("point")
    assert (geom == geom[0]).all() and geom[0, 3] == 0 and g["ok"] == 1
    # radii comparable to the box: kRel R and kappa D^2 are far above the coordinates' rounding
    geom, _, g = _plan("bigr")
    h, a = GC.half64(g, geom)
    assert (GC.K_REL * h > 100 * 2.0 ** -24 * np.abs(geom[:, :3]).max()).all()
    geom, _, g = _plan("negr")
    assert (geom[:, 3] < 0).sum() >= 30 and np.isneginf(geom[:, 3]).sum() == 2 and np.isnan(geom[:, :3]).any(1).sum() == 2 and np.isinf(geom[:, :3]).any(1).sum() == 2
    assert GC.bounds32(geom)[2] == len(geom) - 8 and (GC.large64(g, geom)[40:48] == 1).all()


def test_long_lists_and_large_spheres():
    geom, _, g = _plan("dense")
    must, may, finite = GC.ranges64(g, geom)
    one = (must[:1024, :, 0] == must[:1024, :, 1]).all(1)  # (a cluster sphere's box within one cell: the same for all)
    cell = must[:1024, :, 0][one]
    assert len(np.unique(cell, axis=0)) <= 8 and np.unique(cell, axis=0, return_counts=True)[1].max() > 256
    for name, want in (("large256", 256), ("large257", 257), ("fine", 300)):
        geom, _, g = _plan(name)
        v = GC.large64(g, geom)
        assert (v == 1).sum() == want and (v == -1).sum() == 0, (name, np.bincount(v + 1))
    # exactly kLargeCells cells is still small
    geom, _, g = _plan("point")
    must, may, _ = GC.ranges64(g, geom)
    assert (np.prod(must[:, :, 1] - must[:, :, 0] + 1, axis=1) == 64).all() and (np.prod(may[:, :, 1] - may[:, :, 0] + 1, axis=1) == 64).all()


def test_scenes_without_a_grid():
    geom, _, g = _plan("nofinite")
    assert GC.bounds32(geom)[2] == 0 and g["ok"] == 0
    geom, _, g = _plan("huge")
    assert GC.bounds32(geom)[2] == len(geom) and g["ok"] == 0 and np.abs(geom[:, :3]).max() > 2.0 ** 50
    rays = GC.nogrid_rays("huge", geom)
    best, decided = GC.closest64(rays, geom)
    o, d, tmax, skip = GC.split(rays)
    assert decided.mean() >= 0.9 and (best[decided] != GC.NONE).sum() >= 40 and (~(tmax >= 0)).sum() >= 60 and (skip != GC.NONE).sum() >= 30
    assert GC.walkable64(g, o, d).sum() == 0


@pytest.mark.parametrize("name", [n for n in GC.NAMES if n not in GC.NOGRID])
def test_large_is_decided(name):
    geom, _, g = _plan(name)
    v = GC.large64(g, geom)
    assert (v == -1).mean() <= CAP, (name, np.bincount(v + 1, minlength=3))


def test_boxes_ending_on_an_edge():
    geom, _, g = _plan("onedge")
    on = past = 0
    for j in range(200, 248):
        h = GC.sphere_half32(g, geom[j, :3], abs(geom[j, 3]))
        for k in range(3):
            e = GC.edges(g, k)
            for end in (float(F32(geom[j, k] + h)), float(F32(geom[j, k] - h))):
                on += int(end in e)
                by = np.abs(e - end).min() / float(h)  # (past the nearest boundary by a share of h between the allowance and kRel)
                past += int(1e-5 < by < 0.5 * GC.K_REL and (end > geom[j, k]) == (end > e[np.abs(e - end).argmin()]))
    assert on >= 20 and past >= 20, (on, past)


@pytest.mark.parametrize("name", GC.WALKED)
def test_rays(name):
    geom, _, g = _plan(name)
    rays, cls, eps, far = GC.rays_of(name, geom, g)
    assert np.bincount(cls, minlength=len(GC.CLASSES)).max() <= 4096
    o, d, tmax, skip = GC.split(rays)
    C = {c: cls == i for i, c in enumerate(GC.CLASSES)}
    for c in ("axis", "tiny", "faces", "outside", "tmax", "ulp", "broken", "random"):
        assert C[c].sum() >= 50, (name, c)
    best, decided = GC.closest64(rays, geom)
    core = ~(C["grazing"] | C["skip"] | C["ulp"])
    assert (~decided[core]).mean() <= CAP, (name, (~decided[core]).sum(), core.sum())
    has_spheres = (np.isfinite(geom).all(1) & (geom[:, 3] != 0)).any()
    if has_spheres:
        t, clear = GC.hits64(rays, geom)
        hit = np.isfinite(t).any(1)
        n_sph = (np.isfinite(geom).all(1) & (geom[:, 3] != 0)).sum()
        n_sph = n_sph if 14 * n_sph <= 4096 else 96  # (every sphere while the class stays within 4096 rays)
        assert C["grazing"].sum() == 14 * n_sph and (C["grazing"] & far).sum() >= 5 * n_sph and (C["grazing"] & ~far).sum() >= 5 * n_sph
        assert (C["grazing"] & (eps < 0) & hit).sum() >= 5 * n_sph and (C["grazing"] & (eps > 0)).sum() >= 3 * n_sph
        assert set(np.abs(eps[C["grazing"]])) == set(GC.EPS)
        assert decided[C["grazing"]].sum() >= 0.25 * C["grazing"].sum()
        near = C["grazing"] & ~far & (np.abs(eps) >= 1e-4)  # (from close by the allowance is far below 2 eps r^2)
        assert near.sum() >= 0.15 * C["grazing"].sum() and (~decided[near]).mean() <= CAP, (name, (~decided[near]).sum(), near.sum())
        assert (best[C["random"] & decided] != GC.NONE).sum() >= (1 if name == "dense" else 50)  # (dense: two spheres of a size to aim at)
        free = np.array(rays[C["skip"]], copy=True)
        free[:, 7] = np.array([GC.NONE], np.uint32).view(F32)[0]
        b2, d2 = GC.closest64(free, geom)
        assert (d2 & (b2 == skip[C["skip"]].astype(np.int64))).sum() >= (3 if name == "n1" else 8)  # (float64 decides, and no other sphere is in front; n1 has 14 grazing rays)
    # zero components of both signs; components either side of kTinyDir dmax; a either side of the limits; origins either side of reach
    assert (C["axis"] & (d == 0).any(1) & np.signbit(d).any(1)).sum() >= 20
    with np.errstate(all="ignore"):
        ratio = np.sort(np.abs(d), axis=1)[:, 1] / np.abs(d).max(1)
        a = (d * d).sum(1)
        off = (np.abs(o - g["ctr"].astype(np.float64)) / float(g["reach"])).max(1)
    tiny = ratio[C["tiny"]]
    assert (tiny == GC.K_TINY).sum() >= 5 and ((tiny > GC.K_TINY) & (tiny < GC.K_TINY * 1.001)).sum() >= 5 and ((tiny < GC.K_TINY) & (tiny > GC.K_TINY * 0.999)).sum() >= 5
    ulp = C["ulp"]
    for lim in (GC.MIN_A, GC.MAX_A):
        assert (ulp & (a == lim)).sum() >= 3 and (ulp & (a < lim) & (a > lim * 0.999)).sum() >= 3 and (ulp & (a > lim) & (a < lim * 1.001)).sum() >= 3, (name, lim)
    assert (ulp & (off > 1.0) & (off < 1.001)).sum() >= 3 and (ulp & (off <= 1.0) & (off > 0.999)).sum() >= 3
    w = GC.walkable64(g, o, d)
    assert (w[ulp] == -1).mean() >= 0.5 and (w[~ulp] == -1).mean() <= 0.01
    assert (w == 0).sum() >= 40 and (w == 1).sum() >= 0.8 * len(rays)
    with np.errstate(invalid="ignore"):
        dead = ~(tmax >= 0)
    assert (dead & (w == 0)).sum() >= 10 and (~dead & (w == 0)).sum() >= 20 and np.isnan(tmax).sum() >= 10 and (tmax < 0).sum() >= 10
    meets = GC.meets64(g, o, d, tmax)
    assert ((w == 1) & (meets == 0)).sum() >= 50 and ((w == 1) & (meets == 1)).sum() >= 0.3 * len(rays)
    assert (C["outside"] & (meets == 1)).sum() >= 20 and (C["outside"] & (meets == 0)).sum() >= 20
    assert (C["tmax"] & np.isfinite(tmax)).sum() == C["tmax"].sum()
    assert (~np.isfinite(o).all(1)).sum() >= 8 and (~np.isfinite(d).all(1)).sum() >= 8


@pytest.mark.parametrize("name", GC.WALKED)
def test_segments(name):
    geom, _, g = _plan(name)
    P, L, own, cls = GC.segments_of(name, geom, g)
    assert len(P) <= 4096
    C = {c: cls == i for i, c in enumerate(GC.SEG_CLASSES)}
    for c in ("point", "short", "long", "beyond", "random"):
        assert C[c].sum() >= 30, (name, c)
    toL = (L - P).astype(np.float64)
    a = (toL * toL).sum(1)
    assert (a[C["point"]] == 0).all() and (a[C["short"]] > 0).all() and (a[C["long"]] > GC.MAX_A).all()
    # (an ulp of a coordinate below 8 is at most 2^-21; in [8, 16) it is 2^-20: a is the limit itself, and walkable; at 1e4 it is 1e-3)
    low = np.abs(P[C["short"]]).max(1) < 8.0
    assert (a[C["short"]][low] < GC.MIN_A).all() and (name in ("off1e4", "s1e6", "dense") or low.mean() >= 0.3)
    off = (np.abs(P.astype(np.float64) - g["ctr"].astype(np.float64)) / float(g["reach"])).max(1)
    assert (off[C["beyond"]] > 1.0).all()
    want = GC.dark64(P, L, own, geom)
    core = ~(C["grazing"] | C["ending"] | C["own"])
    assert (want[core] == -1).mean() <= CAP
    if C["own"].any():
        n_sph = min(48, (np.isfinite(geom).all(1) & (geom[:, 3] != 0)).sum())
        assert C["grazing"].sum() >= 4 * n_sph and C["ending"].sum() >= 4 * n_sph and C["own"].sum() >= 4 * n_sph
        assert (own[C["own"]] != GC.NONE).all() and (own[~C["own"]] == GC.NONE).all()
        # the own sphere would darken its segment: without it most are lit
        free = GC.dark64(P[C["own"]], L[C["own"]], np.full(C["own"].sum(), GC.NONE, np.uint32), geom)
        assert (free == 1).mean() >= (0.4 if name == "dense" else 0.9)  # (dense: from the rim a radius of 1e-5 is below what float64 may call)
        # (negr: a sphere of infinite radius about a finite centre darkens every segment)
        assert (want == 1).sum() >= 5 and ((want == 0).sum() >= 20 or name == "negr")
