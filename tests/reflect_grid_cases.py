"""The scenes of the RTX_OPT_REFLECT_GRID tests (tests/test_host_reflect_grid.py on the CPU, tests/test_gpu_reflect_grid.py on the GPU)
and what the restatement (tests/restate.py::trace_chain) says of them: rays per level, winners, and on which side of the grid's
`reach` every secondary ray starts.  Frames are 37 x 21 and 64 x 48 cells, the camera the default pose.

  a  U.numpy_synth_scene(11, 40, 0, ...): 40 spheres, no plane, every second sphere a mirror (k = 0.4): curved mirrors, every origin
     inside the spheres' box;
  b  scene_b() of tests/test_gpu_shadow_grid.py: 300 spheres and the one large-list sphere at index 150 -- the direction sort is
     engaged, so a sphere's position is not its creation index -- and copies of spheres 142 and 12 in another colour appended as
     creation indices 301 and 302: coincident twins, whose ties the lower creation index must win under the sort.  Spheres 142
     and 12 win 3 level-1 hits at either size, and no choice of reflectivities gives them more than 3 at 37 x 21 (with every
     sphere a mirror: 3 and 5), so copies of spheres 31, 15 and 203 -- the spheres that win the most level-1 hits -- follow as 303,
     304 and 305: more pairs, none taken away.  Every second sphere of 0 .. 300 has k = 0.4, the large one 0.6, the copies 0; no plane;
  c  b over FLOOR (k = 0.5), the last object: floor points near the cloud start walkable rays, those further out than `reach` fall back."""
import functools

import numpy as np

import restate as RS
import util as U
from test_gpu_shadow_grid import FLOOR, NO_PLANES, scene_b

SIZES = [(37, 21), (64, 48)]
NAMES = ["a", "b", "c"]
LARGE = 150            # scene b's large-list sphere
TWINS = {301: 142, 302: 12, 303: 31, 304: 15, 305: 203}  # later twin -> earlier twin
MAX_DEPTH = 4
BOUNDARY_REL = 1.0e-4  # origins this close (relative) to `reach` count as on neither side


def scene(name, W, H):
    """(params, spheres (n, 7), planes (m, 11), {creation index: k})"""
    p = U.pkg().camera_params(W, H)
    if name == "a":
        sph, pl = U.numpy_synth_scene(11, 40, 0, p.element1, p.element2)
        return p, sph, pl, {i: 0.4 for i in range(0, len(sph), 2)}
    base = scene_b()
    assert len(base) == 301 and base[LARGE, 3] == 8.0
    twins = base[[TWINS[g] for g in sorted(TWINS)]].copy()
    twins[:, 4:] = [[10.0, 250.0, 10.0], [250.0, 10.0, 250.0], [10.0, 10.0, 250.0], [250.0, 250.0, 10.0], [10.0, 250.0, 250.0]]
    sph = np.concatenate([base, twins])
    ks = {i: 0.4 for i in range(0, 301, 2)}
    ks[LARGE] = 0.6
    if name == "b":
        return p, sph, NO_PLANES, ks
    assert name == "c"
    ks[len(sph)] = 0.5  # the floor, created after the spheres
    return p, sph, FLOOR, ks


def reach_of(sph):
    """(ctr[3], reach) of the grid over `sph`, in fp32 as rtxgrid::plan_grid forms them from the spheres' boxes c +- |r|."""
    f = np.float32
    c, r = sph[:, :3].astype(f), np.abs(sph[:, 3].astype(f))
    blo, bhi = (c - r[:, None]).min(axis=0), (c + r[:, None]).max(axis=0)
    ctr = f(0.5) * blo + f(0.5) * bhi
    hmax = (f(0.5) * bhi - f(0.5) * blo).max()
    return ctr.astype(f), f(f(3.0) * hmax)


@functools.lru_cache(maxsize=None)
def facts(name, W, H):
    """What the restatement says of scene `name` at W x H (traced once per process, shared by every test that asks)."""
    p, sph, pl, ks = scene(name, W, H)
    trace = RS.trace_chain(U.oracle_params(p), sph, pl, ks, np.arange(W * H), max_depth=MAX_DEPTH)
    ns = len(sph)
    ctr, reach = reach_of(sph)
    inside, beyond, unsure = [], [], []
    for lev in trace["levels"][1:]:
        o = np.stack([np.asarray(x, dtype=np.float32) for x in lev["O"]], axis=1).reshape(-1, 3)
        m = np.abs(o - ctr).max(axis=1) if len(o) else np.zeros(0, dtype=np.float32)
        lo, hi = np.float64(reach) * (1.0 - BOUNDARY_REL), np.float64(reach) * (1.0 + BOUNDARY_REL)
        inside.append(int((m <= lo).sum()))
        beyond.append(int((m > hi).sum()))
        unsure.append(int(((m > lo) & (m <= hi)).sum()))
    l1 = trace["levels"][1]
    g1, left1 = np.asarray(l1["gid"]), np.asarray(l1["left"])
    return dict(p=p, sph=sph, pl=pl, ks=ks, ns=ns, trace=trace, rays=list(trace["rays"]),
                sphere_hits1=int(((g1 >= 0) & (g1 < ns)).sum()), winners1=g1, left1=left1,
                inside=inside, beyond=beyond, unsure=unsure)
