"""The tile passes' culling -- light_cone, build_bundles, walk_spheres and lights_dark_set of rtx_tile_pass.inc, with
rtxshadow::may_occlude and rtxreflect::may_hit -- run on the GPU on tiles of the test's making (tests/gpu_checks/tile_check.hip: the
production text, one 256-thread workgroup per tile, a class of cases per launch) and held to float64 (tests/tile_cases.py, whose
docstring states the formulas) and to the production exact tests.  tests/test_host_tile_bound.py shows, without a GPU, that no case
is vacuous; the counts are asserted here again before each assertion they belong to.

  U   every thread holds the same bits of the cone and the same verdict; the verdict is false exactly when nothing is pending or
      there is no sphere.
  C1  every open point's float64 angle from the device's axis is <= theta and its distance <= dmax; every ray of a float64 group
      has its origin within rho of the device's centre and its direction within theta of the device's axis.
  C2  theta <= the float64 maximum about the device's axis + 2 kAngleMargin; dmax, rho <= the float64 maximum (1 + 2 kRelMargin)
      (+ 1e-30 for dmax); the device's axis within kAngleMargin of the float64 normalised sum.  (For a bundle theta = maxang (1 +
      kRelMargin) + kAngleMargin, which is within the bound while maxang <= 1 rad; the host file asserts that of every group.)
  D   a degenerate case -- a point at the light, a light inside the points' hull, theta past 90 degrees, coordinates whose squares
      overflow, a NaN point; a zero, infinite or NaN ray -- gives `all`, and with it every sphere is listed; a non-finite sphere is
      always listed.
  G   the number of bundles is that of the float64 grouping rule (tile_cases.groups64), and by C1 and C2 each bundle holds that
      rule's members and is no wider than they are.
  S1  a sphere that segment_hits_sphere / secondary_sphere_hit (the production tests) reports for an open point or ray is listed.
  S2  a sphere within r of an open segment, or of an open ray at s >= 0, in float64 is listed.
  T   a sphere is not listed when the header's keep condition, in float64 about the device's axis (and centre) with every margin
      doubled (tile_cases.keep_cone64, keep_bundle64), rejects it.
  W   over all fillings every kept sphere appears exactly once and no other does; what is kept is what the flat may_occlude /
      may_hit keeps for the device's cone or bundles; the float4 listed at a position is sph_geom[position] bit for bit; no
      filling exceeds kTileList; `longest` equals the number kept; above 1024 kept spheres there are at least two fillings.
  E   shadowed / dark under culling equals brute bit for bit, and equals restate_shadows.classify64_points (the rule of
      test_float64_decides_every_level) wherever that decides; at most 2 % of a case's (point, light) pairs are undecided.
  M   (bt, bid) under culling equals brute bit for bit; the winner is tile_cases.closest64's where that decides (at most 2 %
      undecided); of two coincident spheres the one created first wins; a ray's own object never wins.

The dark set has no recording mode (its flush is a lambda inside lights_dark_set): it is held to E and to `longest`.
"""
import ctypes as C
import os

import numpy as np
import pytest

import tile_cases as TC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
P32, PF, PV = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p


# ---------------------------------------------------------------------------------------------- the library

class TileIn(C.Structure):
    _fields_ = [("tiles", PV), ("ntiles", C.c_uint32), ("npts", C.c_uint32), ("flags", PV), ("P", PV), ("N", PV), ("id", PV), ("O", PV), ("D", PV),
                ("sph_geom", PV), ("sph_od", PV), ("nsph", C.c_uint32), ("pl_a", PV), ("pl_b", PV), ("pl_od", PV), ("npl", C.c_uint32), ("lights", PV),
                ("nlights", C.c_uint32)]


class TileOut(C.Structure):
    _fields_ = [("verdict", PV), ("cone", PV), ("flag", PV), ("hit", PV), ("nb", PV), ("bundle", PV), ("longest", PV), ("nfill", PV), ("rec_n", PV),
                ("rec", PV), ("nrec", C.c_uint32)]


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


class Lib:
    """ctypes face of libtile_check.so.  A TileSet in, a dict of arrays out; a non-zero status is an error of the test's plumbing."""

    def __init__(self, so):
        self.so = so

    def arguments(self, ts):
        p = ts.packed()
        n = len(ts)
        tin = TileIn(_p(p["tiles"]), n, 256, _p(p["flags"]), _p(p["P"]), _p(p["N"]), _p(p["id"]), _p(p["O"]), _p(p["D"]), _p(p["sph_geom"]), _p(p["sph_od"]),
                     len(p["sph_geom"]), _p(p["pl_a"]), _p(p["pl_b"]), _p(p["pl_od"]), len(p["pl_a"]), _p(p["lights"]), len(p["lights"]))
        out = dict(verdict=np.zeros((n, 256), np.uint32), cone=np.zeros((n, 256, 7), np.uint32), flag=np.zeros((n, 256), np.uint32),
                   hit=np.zeros((n, 256, 2), np.uint32), nb=np.zeros((n, 256), np.uint32), bundle=np.zeros((n, 4, 10), np.uint32),
                   longest=np.zeros(n, np.uint32), nfill=np.zeros(n, np.uint32), rec_n=np.zeros(n, np.uint32), rec=np.zeros((max(p["nrec"], 1), 8), np.uint32))
        tout = TileOut(*[_p(out[k]) for k in ("verdict", "cone", "flag", "hit", "nb", "bundle", "longest", "nfill", "rec_n", "rec")], p["nrec"])
        return p, tin, out, tout

    def run(self, entry, ts):
        p, tin, out, tout = self.arguments(ts)
        rc = getattr(self.so, entry)(C.byref(tin), C.byref(tout))
        assert rc == 0, (entry, rc)
        out["tiles"] = p["tiles"]
        return out

    def exact(self, kind, A, B, sph):
        """(ns, npts) bytes: the production exact test of point / ray p against sphere j."""
        A, B, sph = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32), np.ascontiguousarray(sph, F32)
        out = np.zeros((len(sph), len(A)), np.uint8)
        if out.size:
            rc = self.so.rtx_tile_exact(C.c_int(kind), _p(A), _p(B), C.c_uint(len(A)), _p(sph), C.c_uint(len(sph)), _p(out))
            assert rc == 0, rc
        return out

    def may_occlude(self, cone7, L, sph):
        sph, cone7, L = np.ascontiguousarray(sph, F32), np.ascontiguousarray(cone7, np.uint32), np.ascontiguousarray(L, F32)
        pairs = np.ascontiguousarray(np.stack([np.zeros(len(sph), np.uint32), np.arange(len(sph), dtype=np.uint32)], axis=1))
        out = np.zeros(len(sph), np.uint32)
        rc = self.so.rtx_tile_may_occlude(_p(cone7), _p(L), C.c_uint(1), _p(sph), C.c_uint(len(sph)), _p(pairs), C.c_uint(len(sph)), _p(out))
        assert rc == 0, rc
        return out.astype(bool)

    def may_hit(self, bundles, sph):
        sph, bundles = np.ascontiguousarray(sph, F32), np.ascontiguousarray(bundles, np.uint32).reshape(-1, 10)
        nb, ns = len(bundles), len(sph)
        pairs = np.ascontiguousarray(np.stack([np.repeat(np.arange(nb, dtype=np.uint32), ns), np.tile(np.arange(ns, dtype=np.uint32), nb)], axis=1))
        out = np.zeros(nb * ns, np.uint32)
        rc = self.so.rtx_tile_may_hit(_p(bundles), C.c_uint(nb), _p(sph), C.c_uint(ns), _p(pairs), C.c_uint(nb * ns), _p(out))
        assert rc == 0, rc
        return out.reshape(nb, ns).astype(bool).any(0)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    # (RTX_TILE_CHECK_LIB: another build of the library -- profiles/r23_tile_bound.txt ran this file over eight mutated ones)
    path = os.environ.get("RTX_TILE_CHECK_LIB") or os.path.join(HERE, "gpu_checks", "libtile_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    return Lib(C.CDLL(path))


def _f(words):
    return np.ascontiguousarray(words, np.uint32).view(F32).astype(np.float64)


# ---------------------------------------------------------------------------------------------- the assertions

def check_uniform(out, k, t):
    """U; returns (verdict, the cone's seven words)."""
    v, c = out["verdict"][k], out["cone"][k]
    assert (v == v[0]).all(), "the verdict differs between threads"
    assert (c == c[0]).all(), "the cone differs between threads: %s" % (np.flatnonzero((c != c[0]).any(1))[:8],)
    assert bool(v[0]) == bool(t["open"].any() and len(t["sph"]) != 0)
    return bool(v[0]), c[0]


def check_cone(cone7, t, what):
    """C1, C2 and D of one tile's cone; returns (all, axis)."""
    L, P = t["lights"][0], t["P"][t["open"]]
    axis, theta, dmax, slack = _f(cone7[0:3]), float(_f(cone7[3:4])[0]), float(_f(cone7[4:5])[0]), float(_f(cone7[5:6])[0])
    all_ = bool(cone7[6])
    deg = True if t["brute"] else TC.cone_degenerate64(L, P)
    assert deg is not None, what
    if deg:
        assert all_, "%s: a degenerate cone does not keep everything (theta %r dmax %r slack %r)" % (what, theta, dmax, slack)
        return all_, axis
    assert not all_, "%s: a cone with a clear axis under 90 degrees keeps everything (theta %r dmax %r slack %r)" % (what, theta, dmax, slack)
    c = TC.cone64(L, P, axis)
    assert abs(TC.norm(axis) - 1.0) < 1e-5
    assert (c["ang"] <= theta).all(), "%s C1: a point %g rad outside theta" % (what, (c["ang"] - theta).max())
    assert (c["dist"] <= dmax).all(), "%s C1: a point beyond dmax by %g" % (what, (c["dist"] - dmax).max())
    assert theta <= c["maxang"] + 2.0 * TC.K_ANG, "%s C2: theta %r, float64 maximum %r" % (what, theta, c["maxang"])
    assert dmax <= c["maxdist"] * (1.0 + 2.0 * TC.K_REL) + 1e-30, "%s C2: dmax %r, float64 maximum %r" % (what, dmax, c["maxdist"])
    off = float(TC.angle(axis, c["axis64"]))
    assert off <= TC.K_ANG, "%s C2: the axis is %g rad from the float64 normalised sum" % (what, off)
    return all_, axis


def check_bundles(out, k, t, what):
    """G, C1, C2, D of one tile's bundles; returns [(all, centre, axis)] per bundle."""
    nb = out["nb"][k]
    assert (nb == nb[0]).all(), "the number of bundles differs between threads"
    groups, closest = TC.groups64(t["open"], t["O"], t["D"], bool(t["brute"]))
    assert closest >= 1.0e-3, closest
    assert int(nb[0]) == len(groups), "%s G: %d bundles, the float64 rule has %d" % (what, int(nb[0]), len(groups))
    res = []
    for g, members in enumerate(groups):
        w = out["bundle"][k, g]
        centre, rho, axis, theta, all_ = _f(w[0:3]), float(_f(w[3:4])[0]), _f(w[4:7]), float(_f(w[7:8])[0]), bool(w[9])
        O, D = t["O"][members], t["D"][members]
        deg = True if t["brute"] else TC.group_degenerate64(O, D)
        assert deg is not None, what
        res.append((all_, centre, axis))
        if deg:
            assert all_, "%s D: bundle %d is degenerate and does not keep everything" % (what, g)
            continue
        assert not all_, "%s: bundle %d of %d rays with a clear axis keeps everything (theta %r rho %r)" % (what, g, len(members), theta, rho)
        c = TC.group64(O, D, centre, axis)
        ref = TC.group64(O, D)
        assert (c["dist"] <= rho).all(), "%s C1: bundle %d, an origin %g outside rho" % (what, g, (c["dist"] - rho).max())
        assert (c["ang"] <= theta).all(), "%s C1: bundle %d, a ray %g rad outside theta" % (what, g, (c["ang"] - theta).max())
        assert theta <= c["maxang"] + 2.0 * TC.K_ANG, "%s C2: bundle %d, theta %r, float64 maximum %r" % (what, g, theta, c["maxang"])
        assert rho <= c["maxdist"] * (1.0 + 2.0 * TC.K_REL), "%s C2: bundle %d, rho %r, float64 maximum %r" % (what, g, rho, c["maxdist"])
        assert float(TC.angle(axis, ref["axis64"])) <= TC.K_ANG, "%s C2: bundle %d, the axis is off the float64 sum" % (what, g)
        # (the centre is a float32 mean: eight pairwise additions and a division, each within 2^-24 of partial sums below |O|_1)
        scale = np.abs(O).sum(-1).max()
        assert TC.norm(centre - O.mean(0)) <= 1e-5 * scale, "%s: bundle %d, the centre is off the float64 mean" % (what, g)
    return res


def listed_of(out, k, t, what, kept_flat=None):
    """W's accounting of one tile's record; returns the boolean vector of listed spheres."""
    ns = len(t["sph"])
    off, total = int(out["tiles"][k][6]), int(out["rec_n"][k])
    assert total <= ns, "%s W: %d entries for %d spheres" % (what, total, ns)
    rec = out["rec"][off:off + total]
    pos = rec[:, 0]
    assert (pos < ns).all(), "%s W: a position past the scene" % what
    count = np.bincount(pos, minlength=ns)
    assert (count <= 1).all(), "%s W: sphere %d is listed %d times" % (what, int(count.argmax()), int(count.max()))
    listed = count == 1
    assert np.array_equal(rec[:, 1:5], t["sph32"].view(np.uint32)[pos]), "%s W: a list entry is not sph_geom[position]" % what
    assert (rec[:, 5] == 0).all()
    for f in range(int(out["nfill"][k])):
        slots = np.sort(rec[rec[:, 6] == f, 7])
        assert len(slots) <= TC.TILE_LIST and np.array_equal(slots, np.arange(len(slots))), "%s W: filling %d has slots %s" % (what, f, slots[:8])
    assert (rec[:, 6] < max(int(out["nfill"][k]), 1)).all()
    assert int(out["longest"][k]) == total == int(listed.sum()), "%s W: longest %d, recorded %d, listed %d" % (what, int(out["longest"][k]), total, int(listed.sum()))
    if total > TC.TILE_LIST:
        assert int(out["nfill"][k]) >= 2
    if kept_flat is not None:
        diff = np.flatnonzero(listed != kept_flat)
        assert diff.size == 0, "%s W: spheres %s are %s but the flat keep condition says otherwise" % (what, diff[:8], "listed" if listed[diff[0]] else "dropped")
    return listed


def check_spheres(listed, keep64, near64, hit, sph, all_, what, counts):
    """S1, S2, T and D of one tile's listed spheres; counts accumulates the case's non-vacuity."""
    finite = np.isfinite(sph).all(-1)
    assert listed[~finite].all(), "%s D: a non-finite sphere is dropped" % what
    if all_:
        assert listed.all(), "%s D: `all` and %d spheres dropped" % (what, int((~listed).sum()))
        return
    bad = np.flatnonzero(hit & ~listed)
    assert bad.size == 0, "%s S1: spheres %s are hit by the production test and not listed" % (what, bad[:8])
    bad = np.flatnonzero(near64 & ~listed)
    assert bad.size == 0, "%s S2: spheres %s lie within r in float64 and are not listed: %s" % (what, bad[:8], sph[bad[:3]])
    bad = np.flatnonzero(~keep64 & listed)
    assert bad.size == 0, "%s T: spheres %s are listed though the doubled-margin rule rejects them: %s" % (what, bad[:8], sph[bad[:3]])
    counts["kept"] += int((keep64 & finite).sum())
    counts["culled"] += int((~keep64).sum())
    counts["near"] += int(near64.sum())
    counts["hit"] += int(hit.sum())


# ---------------------------------------------------------------------------------------------- cones

@pytest.fixture(scope="module")
def cones(lib):
    ts, index = TC.cone_cases()
    return ts, index, lib.run("rtx_tile_cone", ts)


@pytest.mark.parametrize("scale", TC.SCALES)
@pytest.mark.parametrize("placement", TC.PLACEMENTS)
def test_cone(cones, placement, scale):
    """U, C1, C2, D over the six sets of open points."""
    ts, index, out = cones
    seen = 0
    for pattern in TC.PATTERNS:
        k = index[(placement, scale, pattern)]
        t = ts.tile(k)
        have, cone7 = check_uniform(out, k, t)
        assert have == (pattern != "none")
        if have:
            check_cone(cone7, t, "%s %g %s" % (placement, scale, pattern))
            seen += 1
    assert seen == 5


@pytest.mark.parametrize("kind", ("huge", "nan", "no_spheres", "brute"))
def test_cone_specials(cones, kind):
    ts, index, out = cones
    for pattern in TC.PATTERNS:
        k = index[(kind, pattern)]
        t = ts.tile(k)
        have, cone7 = check_uniform(out, k, t)
        assert have == (pattern != "none" and kind != "no_spheres")
        if have:
            all_, _ = check_cone(cone7, t, "%s %s" % (kind, pattern))
            assert all_


# ---------------------------------------------------------------------------------------------- shadow walk: the spheres class

@pytest.fixture(scope="module")
def shadow_spheres(lib):
    ts, index = TC.shadow_sphere_cases()
    return ts, index, lib.run("rtx_tile_shadow_walk", ts)


def _shadow_tile(lib, ts, out, k, what, counts):
    t = ts.tile(k)
    have, cone7 = check_uniform(out, k, t)
    assert have
    all_, axis = check_cone(cone7, t, what)
    L = t["lights"][0]
    listed = listed_of(out, k, t, what, lib.may_occlude(cone7, ts.lights[k][0], t["sph32"]))
    o = t["open"]
    hit = lib.exact(0, ts.rows[k]["P"][o], np.broadcast_to(ts.lights[k][0], (int(o.sum()), 3)), t["sph32"]).any(1)
    if all_:
        check_spheres(listed, None, None, hit, t["sph"], True, what, counts)
    else:
        c = TC.shadow_counts(t, axis, decide=False)
        check_spheres(listed, c["keep"], c["near"], hit, t["sph"], False, what, counts)
    return all_


@pytest.mark.parametrize("scale", TC.SCALES)
@pytest.mark.parametrize("placement", TC.TIGHT_PLACEMENTS)
def test_shadow_spheres(lib, shadow_spheres, placement, scale):
    """S1, S2, T, W (and U, C1, C2 again) with spheres at the cone's rim, beyond dmax, grazing segments, about the light."""
    ts, index, out = shadow_spheres
    for pattern in TC.SPHERE_PATTERNS:
        counts = dict(kept=0, culled=0, near=0, hit=0)
        assert not _shadow_tile(lib, ts, out, index[(placement, scale, pattern)], "%s %g %s" % (placement, scale, pattern), counts)
        assert counts["kept"] >= 1 and counts["culled"] >= 1 and counts["near"] >= 1 and counts["hit"] >= 1, counts


@pytest.mark.parametrize("placement,scale", [(p, s) for p in TC.KEEP_ALL_PLACEMENTS for s in TC.SCALES] + [("huge", 1.0e37), ("nan", 1.0)])
def test_shadow_spheres_degenerate(lib, shadow_spheres, placement, scale):
    """D: every sphere is listed."""
    ts, index, out = shadow_spheres
    keys = [(placement, scale, pattern) for pattern in TC.SPHERE_PATTERNS if (placement, scale, pattern) in index]
    assert len(keys) >= 2
    for key in keys:
        counts = dict(kept=0, culled=0, near=0, hit=0)
        assert _shadow_tile(lib, ts, out, index[key], "%s %g %s" % key, counts)
        assert int(out["longest"][index[key]]) == len(ts.sph[index[key]]) > 100


# ---------------------------------------------------------------------------------------------- shadow walk: the counts

@pytest.fixture(scope="module")
def shadow_walks(lib):
    ts, index = TC.shadow_walk_cases()
    return ts, index, lib.run("rtx_tile_shadow_walk", ts)


@pytest.mark.parametrize("mode", TC.WALK_MODES)
@pytest.mark.parametrize("count", TC.WALK_COUNTS)
def test_shadow_walk(lib, shadow_walks, count, mode):
    """W and E at every count the list's accounting turns on."""
    ts, index, out = shadow_walks
    what = "%d %s" % (count, mode)
    k, kb = index[(count, mode, 1 if mode == "brute" else 0)], index[(count, mode, 1)]
    t = ts.tile(k)
    have, cone7 = check_uniform(out, k, t)
    assert have == (count != 0)
    for kk in {k, kb}:
        if count:
            listed = listed_of(out, kk, ts.tile(kk), what, lib.may_occlude(out["cone"][kk][0], ts.lights[kk][0], t["sph32"]))
            if ts.tile(kk)["brute"]:
                assert listed.all() and int(out["nfill"][kk]) == (1 if count <= 1024 else (2 if count <= 2048 else 3))
        else:
            assert int(out["rec_n"][kk]) == 0 and int(out["longest"][kk]) == 0 and int(out["nfill"][kk]) == 0
    if count:
        kept = int(out["longest"][k])
        if mode == "half":
            assert count // 3 <= kept <= (2 * count + 2) // 3, kept
        elif mode == "few":
            assert kept < 10
        if kept > TC.TILE_LIST:
            assert int(out["nfill"][k]) >= 2
    got, brute = out["flag"][k], out["flag"][kb]
    assert np.array_equal(got, brute), "%s E: culled differs from brute at threads %s" % (what, np.flatnonzero(got != brute)[:8])
    want = TC.shadow_counts(t)["decision"]
    decided = want >= 0
    assert (~decided).sum() <= 0.02 * 256
    if count >= 255 and mode != "few":
        assert (want == 1).sum() >= 1 and (want == 0).sum() >= 1
    bad = np.flatnonzero(decided & (got != np.maximum(want, 0)))
    assert bad.size == 0, "%s E: threads %s differ from float64 (device %s, float64 %s)" % (what, bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------------------------------------- the dark set

@pytest.fixture(scope="module")
def darks(lib):
    ts, index = TC.dark_cases()
    return ts, index, lib.run("rtx_tile_dark_set", ts)


@pytest.mark.parametrize("n_planes", (0, 2))
@pytest.mark.parametrize("nl", TC.DARK_LIGHTS)
def test_dark_set(darks, nl, n_planes):
    """E for lights_dark_set: culled = brute = float64, per light."""
    ts, index, out = darks
    k, kb = index[(nl, n_planes, 0)], index[(nl, n_planes, 1)]
    t = ts.tile(k)
    got, brute = out["flag"][k], out["flag"][kb]
    assert np.array_equal(got, brute), "culled differs from brute at threads %s" % (np.flatnonzero(got != brute)[:8],)
    assert (got >> nl == 0).all() and (got[~t["open"]] == 0).all()
    want = TC.dark_decisions(t)
    o = t["open"]
    assert (want[o] == -1).sum() <= 0.02 * o.sum() * nl
    for i in range(nl):
        bit = (got >> i) & 1
        assert (want[o, i] == 1).sum() >= 1
        bad = np.flatnonzero(o & (want[:, i] >= 0) & (bit != np.maximum(want[:, i], 0)))
        assert bad.size == 0, "light %d: threads %s differ from float64 (device %s, float64 %s)" % (i, bad[:8], bit[bad[:8]], want[bad[:8], i])
    # the lists: brute lists every sphere once (no light without an open pixel has a cone, yet some light has one); culling fewer
    assert int(out["longest"][kb]) == len(t["sph"]) and 1 <= int(out["longest"][k]) < len(t["sph"])


# ---------------------------------------------------------------------------------------------- bundles

@pytest.fixture(scope="module")
def bundles(lib):
    ts, index = TC.bundle_cases(False)
    return ts, index, lib.run("rtx_tile_bundles", ts)


@pytest.mark.parametrize("scale", TC.SCALES)
@pytest.mark.parametrize("name", TC.RAY_SETS + ("brute",))
def test_bundles(bundles, name, scale):
    """G, C1, C2, D."""
    ts, index, out = bundles
    k = index[(name, scale)]
    res = check_bundles(out, k, ts.tile(k), "%s %g" % (name, scale))
    want = {"fan": 1, "two_fans": 2, "corner": 3, "five_clusters": 4, "identical": 1, "t255": 1, "zero_dir": 2, "inf_dir": 2, "nan_origin": 2, "none": 0,
            "brute": 1}
    assert len(res) == want[name]
    if name in ("zero_dir", "inf_dir", "nan_origin", "brute"):
        assert res[-1][0]


# ---------------------------------------------------------------------------------------------- mirror walk: the spheres class

@pytest.fixture(scope="module")
def mirror_spheres(lib):
    ts, index = TC.bundle_cases(True)
    return ts, index, lib.run("rtx_tile_mirror_walk", ts)


@pytest.mark.parametrize("scale", TC.SCALES)
@pytest.mark.parametrize("name", TC.RAY_SETS + ("brute",))
def test_mirror_spheres(lib, mirror_spheres, name, scale):
    """S1, S2, T, D, W (and G, C1, C2 again) with spheres at the bundles' rims and balls, grazing rays, about the origins."""
    ts, index, out = mirror_spheres
    k = index[(name, scale)]
    t = ts.tile(k)
    what = "%s %g" % (name, scale)
    res = check_bundles(out, k, t, what)
    if not res:
        assert int(out["rec_n"][k]) == 0 and int(out["longest"][k]) == 0
        assert (out["hit"][k, :, 1] == 0xffffffff).all()
        return
    listed = listed_of(out, k, t, what, lib.may_hit(out["bundle"][k, :len(res)], t["sph32"]))
    o = t["open"]
    hit = lib.exact(1, ts.rows[k]["O"][o], ts.rows[k]["D"][o], t["sph32"]).any(1)
    counts = dict(kept=0, culled=0, near=0, hit=0)
    all_ = any(r[0] for r in res)
    c = TC.mirror_counts(t, [(r[1], r[2]) for r in res])
    check_spheres(listed, c["keep"], c["near"], hit, t["sph"], all_, what, counts)
    if name in ("fan", "two_fans", "corner", "identical", "t255"):
        assert not all_
        assert counts["kept"] >= 1 and counts["culled"] >= 1 and counts["near"] >= 1 and counts["hit"] >= 1, counts
    if name in ("zero_dir", "inf_dir", "nan_origin", "brute"):
        assert all_ and listed.all()


# ---------------------------------------------------------------------------------------------- mirror walk: the counts

@pytest.fixture(scope="module")
def mirror_walks(lib):
    ts, index = TC.mirror_walk_cases()
    return ts, index, lib.run("rtx_tile_mirror_walk", ts)


def _winners(ts, out, k, kb, what):
    """M of one tile against its brute twin and float64; returns (device winner, float64 winner, decided)."""
    t = ts.tile(k)
    assert np.array_equal(out["hit"][k], out["hit"][kb]), "%s M: culled differs from brute at threads %s" % (
        what, np.flatnonzero((out["hit"][k] != out["hit"][kb]).any(1))[:8])
    bid = out["hit"][k, :, 1]
    win, _, decided = TC.closest64(t["O"], t["D"], t["id"], t["sph"], t["creation"], t["planes"])
    o = t["open"]
    assert (~decided[o]).sum() <= 0.02 * 256
    bad = np.flatnonzero(o & decided & (bid != win))
    assert bad.size == 0, "%s M: threads %s: device winners %s, float64 %s" % (what, bad[:8], bid[bad[:8]], win[bad[:8]])
    assert (bid[o] != t["id"][o])[bid[o] != 0xffffffff].all(), "%s M: a ray's own object wins" % what
    return bid, win, decided


@pytest.mark.parametrize("mode", TC.WALK_MODES)
@pytest.mark.parametrize("count", TC.WALK_COUNTS)
def test_mirror_walk(lib, mirror_walks, count, mode):
    """W and M at every count the list's accounting turns on."""
    ts, index, out = mirror_walks
    what = "%d %s" % (count, mode)
    k, kb = index[(count, mode, 1 if mode == "brute" else 0)], index[(count, mode, 1)]
    t = ts.tile(k)
    for kk in {k, kb}:
        res = check_bundles(out, kk, ts.tile(kk), what)
        assert len(res) == 1
        if count:
            listed = listed_of(out, kk, ts.tile(kk), what, lib.may_hit(out["bundle"][kk, :1], t["sph32"]))
            if ts.tile(kk)["brute"]:
                assert listed.all() and int(out["nfill"][kk]) == (1 if count <= 1024 else (2 if count <= 2048 else 3))
        else:
            assert int(out["rec_n"][kk]) == 0 and int(out["longest"][kk]) == 0
    if count:
        kept = int(out["longest"][k])
        if mode == "half":
            assert count // 3 <= kept <= (2 * count + 2) // 3, kept
        elif mode == "few":
            assert kept < 10
    bid, win, decided = _winners(ts, out, k, kb, what)
    assert (decided & (win != 0xffffffff)).sum() >= 1
    if count >= 255 and mode != "few":
        assert ((bid & 0x80000000) == 0).sum() >= 1


def test_mirror_ties_and_own_object(mirror_walks):
    """M: of two coincident spheres the one created first wins, whatever its position; a ray's own object never wins."""
    ts, index, out = mirror_walks
    bid, win, decided = _winners(ts, out, index[("coincident", 0)], index[("coincident", 1)], "coincident")
    hit = bid != 0xffffffff
    assert hit.sum() >= 50 and (bid[hit] >= 40).all(), bid[hit & (bid < 40)][:8]
    k = index[("own", 0)]
    bid, win, decided = _winners(ts, out, k, index[("own", 1)], "own")
    own = ts.tile(k)["id"]
    assert (own != 0xffffffff).sum() >= 50 and (bid != own)[own != 0xffffffff].all()


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals(lib):
    """-2 and no launch: more than 256 points, an id past the tile's spheres that is no plane, 0 or 9 lights, null pointers."""
    def one():
        ts = TC.TileSet()
        open_, P, L = TC.shadow_tile(np.random.default_rng(1), "all", 1.0, "far")
        ts.add(open_, P=P, N=P, ids=np.zeros(256, np.uint32), O=P, D=P, lights=np.tile(L, (8, 1)), spheres=np.array([[0.0, 0.0, 0.0, 1.0]]))
        return ts

    entries = ("rtx_tile_cone", "rtx_tile_shadow_walk", "rtx_tile_dark_set", "rtx_tile_bundles", "rtx_tile_mirror_walk")
    for entry in entries:
        fn = getattr(lib.so, entry)
        p, tin, out, tout = lib.arguments(one())
        assert fn(C.byref(tin), C.byref(tout)) == 0, entry
        assert fn(None, C.byref(tout)) == -2 and fn(C.byref(tin), None) == -2
        tin.npts = 257
        assert fn(C.byref(tin), C.byref(tout)) == -2, entry
        for field in ("tiles", "flags"):
            p, tin, out, tout = lib.arguments(one())
            setattr(tin, field, None)
            assert fn(C.byref(tin), C.byref(tout)) == -2, (entry, field)
    for entry in ("rtx_tile_shadow_walk", "rtx_tile_dark_set", "rtx_tile_mirror_walk"):
        p, tin, out, tout = lib.arguments(one())
        p["id"][17] = 1  # the tile has one sphere
        assert getattr(lib.so, entry)(C.byref(tin), C.byref(tout)) == -2, entry
        p["id"][17] = 0x80000005  # a plane
        assert getattr(lib.so, entry)(C.byref(tin), C.byref(tout)) == 0, entry
    for nl in (0, 9):
        p, tin, out, tout = lib.arguments(one())
        p["tiles"][0, 5] = nl
        assert lib.so.rtx_tile_dark_set(C.byref(tin), C.byref(tout)) == -2, nl
    for field, entry in (("P", "rtx_tile_cone"), ("lights", "rtx_tile_shadow_walk"), ("N", "rtx_tile_dark_set"), ("O", "rtx_tile_bundles"),
                         ("D", "rtx_tile_mirror_walk"), ("id", "rtx_tile_mirror_walk")):
        p, tin, out, tout = lib.arguments(one())
        setattr(tin, field, None)
        assert getattr(lib.so, entry)(C.byref(tin), C.byref(tout)) == -2, (entry, field)
    for field, entry in (("cone", "rtx_tile_cone"), ("flag", "rtx_tile_dark_set"), ("bundle", "rtx_tile_bundles"), ("hit", "rtx_tile_mirror_walk"),
                         ("rec", "rtx_tile_shadow_walk"), ("longest", "rtx_tile_dark_set")):
        p, tin, out, tout = lib.arguments(one())
        setattr(tout, field, None)
        assert getattr(lib.so, entry)(C.byref(tin), C.byref(tout)) == -2, (entry, field)
    assert lib.so.rtx_tile_exact(C.c_int(2), None, None, C.c_uint(1), None, C.c_uint(1), None) == -2
    assert lib.so.rtx_tile_may_hit(None, C.c_uint(1), None, C.c_uint(1), None, C.c_uint(1), None) == -2
    assert lib.so.rtx_tile_may_occlude(None, None, C.c_uint(1), None, C.c_uint(1), None, C.c_uint(1), None) == -2
