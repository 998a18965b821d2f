"""The inputs of tests/test_gpu_tile_bound.py, judged by the float64 rules of tests/tile_cases.py alone (no GPU, no device code):
every parametrised case of the GPU file has something for each of its assertions to bite on -- a sphere the doubled-margin rule
keeps and one it rejects (T), a sphere within r of an open segment or ray (S2), a shadowed and a lit point, a winner (E, M), more
than one filling above 1024 kept spheres (W) -- and leaves at most 2 % of its (point, light) pairs or rays undecided."""
import numpy as np
import pytest

import tile_cases as TC


@pytest.fixture(scope="module")
def shadow_spheres():
    return TC.shadow_sphere_cases()


@pytest.fixture(scope="module")
def shadow_walks():
    return TC.shadow_walk_cases()


@pytest.fixture(scope="module")
def mirror_spheres():
    return TC.bundle_cases(True)


@pytest.fixture(scope="module")
def mirror_walks():
    return TC.mirror_walk_cases()


def test_cone_cases_are_decided():
    """Every cone case is clearly degenerate or clearly not (never within a band of a threshold), and each kind is there."""
    ts, index = TC.cone_cases()
    seen = {True: 0, False: 0}
    for key, k in index.items():
        t = ts.tile(k)
        if not t["open"].any():
            continue
        d = TC.cone_degenerate64(t["lights"][0], t["P"][t["open"]])
        assert d is not None, key
        seen[d] += 1
        if key[0] in ("huge", "nan", "at_point", "over90") and (key[0] != "over90" or t["open"].sum() > 1):
            assert d is True, key
        if key[0] in ("far", "near", "under90"):
            assert d is False, key
    assert seen[True] >= 30 and seen[False] >= 30, seen


@pytest.mark.parametrize("scale", TC.SCALES)
@pytest.mark.parametrize("placement", TC.TIGHT_PLACEMENTS)
def test_shadow_sphere_cases(shadow_spheres, placement, scale):
    ts, index = shadow_spheres
    for pattern in TC.SPHERE_PATTERNS:
        t = ts.tile(index[(placement, scale, pattern)])
        assert TC.cone_degenerate64(t["lights"][0], t["P"][t["open"]]) is False
        c = TC.shadow_counts(t)
        finite = np.isfinite(t["sph"]).all(-1)
        assert (c["keep"] & finite).sum() >= 1 and (~c["keep"]).sum() >= 1, (pattern, int(c["keep"].sum()))
        assert c["near"].sum() >= 1 and (~c["near"] & finite).sum() >= 1, pattern
        assert not (c["near"] & ~c["keep"]).any(), "the doubled-margin rule rejects a sphere within r of a segment"


@pytest.mark.parametrize("mode", TC.WALK_MODES)
@pytest.mark.parametrize("count", TC.WALK_COUNTS)
def test_shadow_walk_cases(shadow_walks, count, mode):
    ts, index = shadow_walks
    t = ts.tile(index[(count, mode, 1 if mode == "brute" else 0)])
    assert len(t["sph"]) == count
    c = TC.shadow_counts(t)
    kept = int(c["keep"].sum())
    if mode == "brute":
        assert t["brute"] == 1
    elif mode == "half":
        assert count // 3 <= kept <= (2 * count + 2) // 3, kept
    else:
        assert kept < 10
    if count > 1024 and mode == "brute":
        assert count > TC.TILE_LIST  # more than one filling
    if count >= 255 and mode != "few":
        assert (c["decision"] == 1).sum() >= 1 and (c["decision"] == 0).sum() >= 1
    assert (c["decision"] == -1).sum() <= 0.02 * 256, int((c["decision"] == -1).sum())


@pytest.mark.parametrize("n_planes", (0, 2))
@pytest.mark.parametrize("nl", TC.DARK_LIGHTS)
def test_dark_cases(nl, n_planes):
    ts, index = TC.dark_cases()
    t = ts.tile(index[(nl, n_planes, 0)])
    k = TC.dark_decisions(t)
    o = t["open"]
    assert (k[o] == -1).sum() <= 0.02 * o.sum() * nl, int((k[o] == -1).sum())
    for i in range(nl):
        assert (k[o, i] == 1).sum() >= 1, i
        if not (nl >= 3 and i == 2):
            assert (k[o, i] == 0).sum() >= 1, i
    if nl >= 3:  # the light no point faces
        L = t["lights"][2]
        assert (np.einsum("nk,nk->n", t["N"][o], L - t["P"][o]) < -1.0).all()
    if nl >= 2:
        assert np.array_equal(t["lights"][0], t["lights"][1])
    assert (t["id"][o] & 0x80000000).any() == (n_planes == 2) and (~t["id"][o] & 0x80000000).any()


@pytest.mark.parametrize("scale", TC.SCALES)
@pytest.mark.parametrize("name", TC.RAY_SETS)
def test_ray_set_cases(mirror_spheres, name, scale):
    ts, index = mirror_spheres
    t = ts.tile(index[(name, scale)])
    c = TC.mirror_counts(t)
    want_groups = {"fan": 1, "two_fans": 2, "corner": 3, "five_clusters": 4, "identical": 1, "t255": 1, "none": 0}
    if name in want_groups:
        assert len(c["groups"]) == want_groups[name], len(c["groups"])
    if name in ("zero_dir", "inf_dir", "nan_origin"):  # u = 0 is within 60 degrees of nothing: the ray is a group of its own
        assert len(c["groups"]) == 2 and list(c["groups"][1]) == [{"zero_dir": 37, "inf_dir": 130, "nan_origin": 200}[name]]
    if name == "five_clusters":  # the last bundle takes two clusters: wider than 60 degrees
        last = c["groups"][3]
        assert TC.group64(t["O"][last], t["D"][last])["maxang"] > np.pi / 3 - 0.2
    assert c["closest"] >= 1.0e-3, c["closest"]
    deg = [TC.group_degenerate64(t["O"][g], t["D"][g]) for g in c["groups"]]
    assert None not in deg
    if name in ("zero_dir", "inf_dir", "nan_origin"):
        assert True in deg
    for g, d in zip(c["groups"], deg):  # C2 as it is stated needs maxang (1 + K) + A <= maxang + 2 A
        assert d or TC.group64(t["O"][g], t["D"][g])["maxang"] < 1.0
    if name in ("fan", "two_fans", "corner", "identical", "t255"):
        assert deg == [False] * len(deg)
        finite = np.isfinite(t["sph"]).all(-1)
        assert (c["keep"] & finite).sum() >= 1 and (~c["keep"]).sum() >= 1, int(c["keep"].sum())
        assert c["near"].sum() >= 1 and (~c["near"] & finite).sum() >= 1
        assert not (c["near"] & ~c["keep"]).any(), "the doubled-margin rule rejects a sphere within r of a ray"


@pytest.mark.parametrize("mode", TC.WALK_MODES)
@pytest.mark.parametrize("count", TC.WALK_COUNTS)
def test_mirror_walk_cases(mirror_walks, count, mode):
    ts, index = mirror_walks
    t = ts.tile(index[(count, mode, 1 if mode == "brute" else 0)])
    c = TC.mirror_counts(t)
    kept = int(c["keep"].sum())
    if mode == "half":
        assert count // 3 <= kept <= (2 * count + 2) // 3, kept
    elif mode == "few":
        assert kept < 10
    win, _, decided = TC.closest64(t["O"], t["D"], t["id"], t["sph"], t["creation"], t["planes"])
    assert (~decided).sum() <= 0.02 * 256, int((~decided).sum())
    assert ((win != 0xffffffff) & decided).sum() >= 1
    if count >= 255 and mode != "few":
        assert ((win & 0x80000000) == 0).sum() >= 1, "no ray's winner is a sphere"


def test_mirror_special_cases(mirror_walks):
    ts, index = mirror_walks
    t = ts.tile(index[("coincident", 0)])
    win, _, decided = TC.closest64(t["O"], t["D"], t["id"], t["sph"], t["creation"], t["planes"])
    hit = decided & (win != 0xffffffff)
    assert hit.sum() >= 50 and (win[hit] >= 40).all()  # the later position was created first
    assert (~decided).sum() <= 0.02 * 256
    t = ts.tile(index[("own", 0)])
    assert (t["id"] != 0xffffffff).sum() >= 50
    win, _, decided = TC.closest64(t["O"], t["D"], t["id"], t["sph"], t["creation"], t["planes"])
    assert (win != t["id"])[t["id"] != 0xffffffff].all()
    assert (~decided).sum() <= 0.02 * 256
