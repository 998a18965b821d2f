"""The judge of the roll-call scenes (tests/rollcall_cases.py), on the CPU alone, so that tests/test_gpu_rollcall.py never runs on an
input that could hide a dropped item:

  * in float64, every sphere meant to own a pixel is the nearest hit on it: its own ray passes within 0.01 r of the centre, every
    foreign pixel ray misses every sphere by at least 1.5 r, and a filler or plane behind an owner is at least 1 % farther in t;
    the oracle's frame reports that hit on that pixel, its distance within 1e-4 relative of float64's; every plane of a plane
    case wins its pixel in the oracle's frame;
  * the candidate counts the cases state are known, not hoped for: against cull_geometry.Pyramid and margin64 every sphere is
    either certainly kept or certainly culled -- clear of the documented margin by 0.1 pixel pitch -- for every stated macro tile,
    cell and 64-pixel wave region, with ZERO undecided spheres, and the kept ones number what the case states;
  * the thresholds the sweeps cross stand in the sources as the cases module restates them, and the tile shapes and cell grids
    it assumes are rtxplan::plan_tiles' / plan_cells' own (a small program compiled from csrc/rtx_plan.hpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cull_geometry as CG
import oracle as O
import rollcall_cases as RC
import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-in-windows-console_amd", "csrc")


# ---------------------------------------------------------------------------------------------- the sources

def test_thresholds_stand_in_the_sources_as_the_sweeps_restate_them():
    """Whoever changes one of these lines is told here that the sweeps of tests/test_gpu_rollcall.py are stale."""
    text = {}
    for name, line in RC.SOURCE_LINES:
        if name not in text:
            text[name] = open(os.path.join(CSRC, name)).read()
        assert text[name].count(line) >= 1, "%s no longer has the line %r: rollcall_cases.py restates it" % (name, line)
    assert RC.K_CHUNK == 2 * RC.K_THREADS
    assert RC.TILE_K[RC.CAP_CULL][0] == RC.CAP_CULL - RC.K_CHUNK - 1 and RC.TILE_K[RC.CAP_REFINE][-1] == 2 * RC.CAP_REFINE + 1
    assert float(U.pkg().camera_params(65, 64).cam_far) == RC.FAR


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rollcall") / "rollcall_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "host", "rollcall_plan.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("frame,plan", sorted(RC.SHAPES))
def test_tile_shapes_and_cell_grids_are_the_planners_own(plan_program, frame, plan):
    (W, H), (opts, _) = frame, RC.PLANS[plan]
    mw, mh, nsub, refine, cells = RC.SHAPES[(frame, plan)]
    _, tile, sub, two, ref = opts
    for pose in ("default", "rolled"):
        cam = CG.camera(W, H, pose)
        for ns in (0, 9, 300, 1537, 5636):   # (with the sub-tile count given, neither depends on the scene's size)
            args = [W, H, H, ns, "%.9g" % cam.packed[19], "%.9g" % cam.packed[20], sub, tile, ref, 0] + ["%.9g" % v for v in cam.packed[:16]]
            out = subprocess.run([plan_program] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
            assert out.returncode == 0, out.stdout
            lw, lnx, got_nsub, got_mw, got_mh, gx, gy, got_refine, cgx, cgy, cells_x, cells_y, cell_w, cell_h, cap = (int(v) for v in out.stdout.split())
            assert (got_mw, got_mh, got_nsub, got_refine) == (mw, mh, nsub, refine), (pose, ns, out.stdout)
            assert (gx, gy) == (-(-W // mw), -(-H // mh))
            if cells is not None:
                assert two == 1 and (cells_x, cells_y, cell_w, cell_h) == cells and (cgx, cgy) == (0, 0), (pose, ns, out.stdout)


# ---------------------------------------------------------------------------------------------- the judge

def _sphere_t(o, w, centre, r):
    """Float64 distance along unit ray w from o to the sphere, or inf."""
    v = centre - o
    b = (v * w).sum(-1)
    disc = r * r - ((v * v).sum(-1) - b * b)
    with np.errstate(invalid="ignore"):
        t = b - np.sqrt(disc)
    return np.where((disc >= 0.0) & (t > 0.0), t, np.inf)


def _plane_t(o, w, pl):
    """Plane::Trace in float64 for unit rays w (n, 3) against planes (m, 11): (n, m) distances, inf where it reports no hit."""
    p, n = pl[:, 0:3], pl[:, 3:6]
    dn = w @ n.T
    num = ((p - o) * n).sum(1)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = num / dn
    hx = o[0] + w[:, 0:1] * t
    hz = o[2] + w[:, 2:3] * t
    hw, hh = 0.5 * pl[:, 9][None, :], 0.5 * pl[:, 10][None, :]
    ok = (dn < -1.2e-7) & (t > 0.0) & (hx > p[:, 0] - hw) & (hx < p[:, 0] + hw) & (hz > p[:, 2] - hh) & (hz < p[:, 2] + hh)
    return np.where(ok, t, np.inf)


def judge(case):
    """Asserts everything the module's docstring lists for one case; returns (spheres judged against regions, undecided)."""
    W, H, cam = case.W, case.H, case.cam
    o = cam.pos
    w_all = case.dirs.reshape(-1, 3)
    s64 = case.sph.astype(np.float64)
    centre, r = s64[:, :3], s64[:, 3]
    pl64 = case.planes.astype(np.float64)
    ns = len(s64)
    what = case.name
    if ns:
        v = centre - o
        dist = np.linalg.norm(v, axis=1)
        own = w_all[case.pix]
        # its own ray passes within 0.01 r of the centre
        off = np.linalg.norm(np.cross(v, own), axis=1)
        assert (off <= 0.01 * r).all(), "%s: a sphere's own ray passes %.3g r from its centre" % (what, (off / r).max())
        # every foreign pixel ray misses it by at least 1.5 r: the angle to the centre's direction exceeds asin(1.5 r / |O|)
        vhat = v / dist[:, None]
        thr = np.sqrt(1.0 - (1.5 * r / dist) ** 2)
        for a in range(0, ns, 512):
            cosang = vhat[a:a + 512] @ w_all.T
            near = cosang > thr[a:a + 512, None]
            near[np.arange(len(cosang)), case.pix[a:a + 512]] = False
            assert not near.any(), "%s: a foreign pixel ray passes within 1.5 r of sphere %d" % (what, a + int(np.flatnonzero(near.any(1))[0]))
        # on a pixel the owner is the nearest by 1 %, in front of far
        t_own = _sphere_t(o, own, centre, r)
        assert np.isfinite(t_own).all() and (t_own[case.owner] <= 0.999 * RC.FAR).all() and (t_own <= 0.999 * RC.FAR).all()
        t_of_pixel = np.full(W * H, np.inf)
        t_of_pixel[case.pix[case.owner]] = t_own[case.owner]
        assert (t_own[~case.owner] >= 1.01 * t_of_pixel[case.pix[~case.owner]]).all(), "%s: a filler is not 1 %% behind its owner" % what
        fillers = np.flatnonzero(~case.owner)
        for p in np.unique(case.pix[fillers]):      # fillers of one pixel differ in t too: the one that shows for a lost owner is known
            ts = np.sort(t_own[fillers[case.pix[fillers] == p]])
            assert (np.diff(ts) >= 0.01 * ts[:-1]).all()
        if len(pl64):
            tp = _plane_t(o, w_all[case.pix[case.owner]], pl64).min(1)
            assert (tp >= 1.01 * t_own[case.owner]).all(), "%s: a plane is not 1 %% behind an owner" % what
    else:
        t_of_pixel = np.full(W * H, np.inf)
    # planes: each the nearest object on its own pixel, by 1 %
    t_plane = np.zeros(0)
    if len(pl64):
        assert not np.isin(case.plane_pix, case.pix).any() and len(np.unique(case.plane_pix)) == len(pl64)
        tp = _plane_t(o, w_all[case.plane_pix], pl64)
        t_plane = tp[np.arange(len(pl64)), np.arange(len(pl64))]
        assert np.isfinite(t_plane).all() and (t_plane <= 0.999 * RC.FAR).all(), "%s: a plane misses its own pixel" % what
        tp[np.arange(len(pl64)), np.arange(len(pl64))] = np.inf
        assert (tp.min(1) >= 1.01 * t_plane).all() if len(pl64) > 1 else True
    # the oracle's frame reports those hits
    _, px = O.render(U.oracle_params(case.params()), O.Scene.from_arrays(case.sph, case.planes), O.RGB_ASCII, want_pixels=True)
    px = px.reshape(-1)
    want = t_of_pixel.copy()
    want[case.plane_pix] = t_plane
    hit = np.isfinite(want)
    assert (px["hit"][hit] != 0).all(), "%s: the oracle misses an owned pixel" % what
    assert (np.abs(px["distance"][hit].astype(np.float64) - want[hit]) <= 1.0e-4 * want[hit]).all(), "%s: the oracle's distance on an owned pixel" % what
    traced = np.arange(W * H) % W != W - 1
    assert (px["hit"][~hit & traced] == 0).all(), "%s: the oracle hits something on a pixel nobody owns" % what
    # the stated counts: certainly kept or certainly culled, nothing undecided
    judged = undecided = 0
    if case.counts:
        otc = o - centre
        margin = CG.margin64(r, dist)
        slack = 0.1 * case.pitch * dist
        for rect, stated in case.counts:
            d = otc @ CG.Pyramid(cam, rect).n.T
            kept = (d < (margin - slack)[:, None]).all(1)
            culled = (d > (margin + slack)[:, None]).any(1)
            judged += ns
            undecided += int((~kept & ~culled).sum())
            assert int(kept.sum()) == stated and int(kept.sum()) == case.count_in(rect), \
                "%s: rectangle %r keeps %d spheres for certain, the case states %d" % (what, rect, int(kept.sum()), stated)
    return judged, undecided


CASES = RC.all_cases()


def test_every_sweep_value_has_its_case():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert len([c for c in CASES if c.name.startswith("size ")]) == len(RC.SIZES) + 4
    assert {len(c.sph) for c in CASES if c.name.startswith("size ") and "permuted default" in c.name} == set(RC.SIZES)


@pytest.mark.parametrize("case", CASES, ids=[c.name.replace(" ", "-") for c in CASES])
def test_every_object_owns_its_pixel_and_every_count_is_known(case):
    judged, undecided = judge(case)
    print("%s: %d spheres, %d planes, %d stated rectangles, %d sphere-rectangle pairs judged, %d undecided"
          % (case.name, len(case.sph), len(case.planes), len(case.counts), judged, undecided))
    assert undecided == 0
    if case.name.split()[0] in ("tile", "wave", "gate", "cell"):
        assert judged > 0
