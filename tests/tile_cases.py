"""Tiles for the direct check of the tile passes' culling (tests/gpu_checks/tile_check.hip, tests/test_gpu_tile_bound.py), and the
float64 rules they are held to.  No device code and no GPU: tests/test_host_tile_bound.py runs the generators and the rules alone
and asserts that no case is vacuous before a GPU is involved.

Everything is built in float64, rounded to float32 once, and judged from the rounded values: a generator only places things, the
rules classify them.  The rules (K = kRelMargin = 1e-4, A = kAngleMargin = 1e-4 rad, kappa = 2e-6, the headers' constants):

  cone64 / group64   the float64 maxima of angle and distance of the open points (rays) about a given axis (and centre).
  keep_cone64        rtx_shadow.hpp's keep condition with every margin doubled, on the float64 cone about the DEVICE's axis:
                       dmax = maxdist (1 + 2K) + 1e-30, theta = maxang + 2A, slack = 2e-5 (|L|_1 + dmax),
                       R = |r| (1 + 2K) + 2K D + slack, D = |C - L|;
                       kept when !(D > R), or D - R <= dmax and phi <= theta + asin(R / D) + 2A.
  keep_bundle64      rtx_reflect.hpp's, likewise, about the device's centre and axis:
                       rho = maxdist (1 + 2K), theta = maxang (1 + 2K) + 2A, slack = 2e-5 (|O|_1 + rho),
                       re = sqrt(r^2 (1 + 2 kappa) + 2 kappa (D + rho)^2), R = re (1 + 2K) + 2K D + rho + slack;
                       kept when !(D > R), or phi <= theta + asin(R / D) + 2A.
  A sphere either rule rejects (for every bundle) must not be listed (T); a sphere within r of an open segment, or of an open ray
  at s >= 0, must be (S2).
"""
import numpy as np

F32 = np.float32
K_REL = float(F32(1.0e-4))
K_ANG = float(F32(1.0e-4))
KAPPA = float(F32(2.0e-6))
HALF_PI = float(F32(1.57079632679))
TILE_LIST = 1024
NO_HIT = float(F32(99999999.0))

PATTERNS = ("all", "t255", "t0", "wave1", "scattered17", "none")
SCALES = (1.0e-3, 1.0, 1.0e4)
WALK_COUNTS = (0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 2600)
WALK_MODES = ("brute", "half", "few")
MARGIN_STEPS = (0.5, 0.9, 2.5, 10.0)
GAPS = (1.0e-6, 1.0e-5, 1.0e-3)


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(F32)


def f64(x):
    return np.asarray(x, dtype=F32).astype(np.float64)


def norm(v):
    with np.errstate(all="ignore"):
        return np.sqrt((v * v).sum(-1))


def angle(a, b):
    """atan2(|a x b|, a . b) along the last axis, broadcasting."""
    with np.errstate(all="ignore"):
        return np.arctan2(norm(np.cross(a, b)), (a * b).sum(-1))


def any_perp(rng, d):
    d = d / norm(d)
    v = rng.standard_normal(3)
    v -= d * (v @ d)
    return v / norm(v)


def unit_at(axis, e1, phi, psi):
    """The unit vector at angle phi from `axis`, turned by psi about it (e1 a unit vector perpendicular to axis)."""
    e2 = np.cross(axis, e1)
    return np.cos(phi) * axis + np.sin(phi) * (np.cos(psi) * e1 + np.sin(psi) * e2)


# ---------------------------------------------------------------------------------------------- the launch's arrays

class TileSet:
    """The tiles of one launch.  add() takes one tile: 256 flags, points, normals, ids, ray origins and directions (what a class
    does not use may be None), its spheres (n, 4) with their creation indices, its lights (k, 3), brute and the planes it sees."""

    def __init__(self, planes=None):
        self.tiles, self.rows, self.sph, self.sph_ci, self.lights, self.meta = [], [], [], [], [], []
        self.nsph = self.nlights = self.nrec = 0
        self.planes = np.zeros((0, 11)) if planes is None else np.asarray(planes, dtype=np.float64)  # p(3) n(3) colour(3) w h

    def add(self, open_, P=None, N=None, ids=None, O=None, D=None, spheres=None, creation=None, lights=None, brute=0, np_=0, **meta):
        z3 = np.zeros((256, 3), F32)
        row = dict(flags=np.asarray(open_).astype(np.uint32), P=z3 if P is None else f32(P), N=z3 if N is None else f32(N),
                   id=np.full(256, 0xffffffff, np.uint32) if ids is None else np.asarray(ids).astype(np.uint32),
                   O=z3 if O is None else f32(O), D=z3 if D is None else f32(D))
        sph = np.zeros((0, 4), F32) if spheres is None else f32(spheres).reshape(-1, 4)
        ci = np.arange(len(sph), dtype=np.uint32) if creation is None else np.asarray(creation).astype(np.uint32)
        lig = np.zeros((1, 3), F32) if lights is None else f32(lights).reshape(-1, 3)
        self.tiles.append([self.nsph, len(sph), np_, brute, self.nlights, len(lig), self.nrec, len(sph)])
        self.rows.append(row)
        self.sph.append(sph)
        self.sph_ci.append(ci)
        self.lights.append(lig)
        self.nsph += len(sph)
        self.nlights += len(lig)
        self.nrec += len(sph)
        self.meta.append(meta)
        return len(self.tiles) - 1

    def __len__(self):
        return len(self.tiles)

    def tile(self, k):
        """The rounded inputs of tile k in float64 (what the rules read), with the float32 spheres beside them."""
        r = self.rows[k]
        return dict(open=r["flags"].astype(bool), P=f64(r["P"]), N=f64(r["N"]), id=r["id"], O=f64(r["O"]), D=f64(r["D"]), sph32=self.sph[k],
                    sph=f64(self.sph[k]), creation=self.sph_ci[k], lights=f64(self.lights[k]), brute=self.tiles[k][3], np=self.tiles[k][2],
                    planes=self.planes[:self.tiles[k][2]], **self.meta[k])

    def packed(self):
        cat = lambda key: np.ascontiguousarray(np.concatenate([r[key] for r in self.rows]))
        sph = np.concatenate(self.sph) if self.nsph else np.zeros((0, 4), F32)
        od = np.zeros((len(sph), 4), F32)
        if self.nsph:
            od[:, 3] = np.concatenate(self.sph_ci).view(F32)
        pl = self.planes
        pl_a = f32(np.concatenate([pl[:, 0:3], pl[:, 9:10]], axis=1)) if len(pl) else np.zeros((0, 4), F32)
        pl_b = f32(np.concatenate([pl[:, 3:6], pl[:, 10:11]], axis=1)) if len(pl) else np.zeros((0, 4), F32)
        pl_od = np.zeros((len(pl), 4), F32)
        pl_od[:, 3] = (np.arange(len(pl), dtype=np.uint32) + 0x100000).view(F32)  # planes come after every sphere
        return dict(tiles=np.asarray(self.tiles, dtype=np.uint32), flags=cat("flags"), P=cat("P"), N=cat("N"), id=cat("id"), O=cat("O"), D=cat("D"),
                    sph_geom=np.ascontiguousarray(sph), sph_od=od, pl_a=np.ascontiguousarray(pl_a), pl_b=np.ascontiguousarray(pl_b), pl_od=pl_od,
                    lights=np.ascontiguousarray(np.concatenate(self.lights)), nrec=self.nrec)


# ---------------------------------------------------------------------------------------------- float64 rules: shadows

def open_mask(rng, pattern):
    m = np.zeros(256, bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "t255":
        m[255] = True
    elif pattern == "t0":
        m[0] = True
    elif pattern == "wave1":
        m[64:128] = True
    elif pattern == "scattered17":
        m[rng.choice(256, 17, replace=False)] = True
    return m


def cone64(L, P, axis=None):
    """Float64 maxima of the open points P (n, 3) seen from L about `axis` (None: the float64 normalised sum of the directions)."""
    v = P - L
    d = norm(v)
    with np.errstate(all="ignore"):
        u = v / d[:, None]
    s = u.sum(0)
    axis64 = s / norm(s)
    a = axis64 if axis is None else np.asarray(axis, dtype=np.float64)
    ang = angle(a[None, :], u)
    return dict(axis64=axis64, sumlen=norm(s) / len(P), maxang=ang.max(), maxdist=d.max(), ang=ang, dist=d)


def cone_degenerate64(L, P):
    """Must the cone of open points P keep everything?  True / False, or None within a band of one of the header's thresholds."""
    if len(P) == 0:
        return None
    if not np.isfinite(P).all():
        return True
    d = norm(P - L)
    scale = np.abs(P).sum(-1) + np.abs(L).sum()
    # (d is the root of a float32 sum of squares: past 1.8e19 the sum is inf, which the header's d < 3e38 turns away)
    if (d < 0.5e-6 * scale).any() or (d * d > 3.5e38).any():
        return True
    if (d < 2.0e-6 * scale).any() or (d * d > 1.0e38).any():
        return None
    c = cone64(L, P)
    slack = 1.0e-5 * (np.abs(L).sum() + c["maxdist"])
    if c["sumlen"] < 0.09 or c["maxang"] + K_ANG > HALF_PI + 5.0e-4 or slack > 3.3e37:
        return True
    if c["sumlen"] < 0.11 or c["maxang"] + K_ANG > HALF_PI - 5.0e-4 or slack > 2.7e37:
        return None
    return False


def keep_cone64(L, P, axis, sph):
    """rtx_shadow.hpp's keep condition in float64 with every margin doubled (module docstring); a non-finite sphere is kept."""
    c = cone64(L, P, axis)
    dmax = c["maxdist"] * (1.0 + 2.0 * K_REL) + 1.0e-30
    theta = c["maxang"] + 2.0 * K_ANG
    slack = 2.0e-5 * (np.abs(L).sum() + dmax)
    v = sph[:, :3] - L
    with np.errstate(all="ignore"):
        D = norm(v)
        R = np.abs(sph[:, 3]) * (1.0 + 2.0 * K_REL) + 2.0 * K_REL * D + slack  # (the exact test squares r: a negative radius is |r|)
        phi = angle(np.asarray(axis, dtype=np.float64)[None, :], v)
        beta = np.arcsin(np.clip(R / D, -1.0, 1.0))
        keep = ~(D > R) | ((D - R <= dmax) & (phi <= theta + beta + 2.0 * K_ANG))
    return keep | ~np.isfinite(sph).all(-1)


def segment_distance(P, L, C):
    """(m, n): float64 distance of centre C[j] from the segment (P[i], L)."""
    toL = L - P
    len2 = (toL * toL).sum(-1)
    w = C[:, None, :] - P[None, :, :]
    with np.errstate(all="ignore"):
        s = np.clip((w * toL[None]).sum(-1) / np.maximum(len2, 1e-300)[None], 0.0, 1.0)
        return norm(w - toL[None] * s[..., None])


# ---------------------------------------------------------------------------------------------- float64 rules: mirrors

def ray_degenerate(O, D):
    """rtx_reflect.hpp, unit_direction: zero, infinite or NaN direction, or an origin that is not finite (float32 inputs)."""
    with np.errstate(all="ignore"):
        ln = norm(D)
        scale = np.abs(O).sum(-1)
        return ~(ln > 1.0e-30) | ~(ln < 3.0e38) | ~(scale < 3.0e37)


def unit_rays(O, D):
    deg = ray_degenerate(O, D)
    with np.errstate(all="ignore"):
        u = D / norm(D)[:, None]
    u[deg] = 0.0
    return u, deg


def groups64(open_, O, D, brute=False):
    """build_bundles' grouping in float64: the leader is the lowest open thread, members are within 60 degrees of it (u . lu >=
    0.5; a degenerate ray has u = 0), the fourth group takes the rest, brute gives one group.  Returns the groups' thread lists and
    the smallest |u . lu - 0.5| any decision had."""
    u, _ = unit_rays(O, D)
    left = np.asarray(open_).copy()
    groups, closest = [], np.inf
    for g in range(4):
        if not left.any():
            break
        lead = int(np.flatnonzero(left)[0])
        dots = u @ u[lead]
        if brute or g == 3:
            member = left.copy()
        else:
            member = left & ((dots >= 0.5) | (np.arange(256) == lead))
            others = left & (np.arange(256) != lead)
            if others.any():
                closest = min(closest, np.abs(dots[others] - 0.5).min())
        groups.append(np.flatnonzero(member))
        left &= ~member
    return groups, closest


def group64(O, D, centre=None, axis=None):
    """Float64 maxima of one group's rays about a centre and an axis (None: their float64 mean and normalised direction sum)."""
    u, deg = unit_rays(O, D)
    s = u.sum(0)
    with np.errstate(all="ignore"):
        axis64 = s / norm(s)
    c = O.mean(0) if centre is None else np.asarray(centre, dtype=np.float64)
    a = axis64 if axis is None else np.asarray(axis, dtype=np.float64)
    ang = angle(a[None, :], u)
    dist = norm(O - c)
    return dict(axis64=axis64, sumlen=norm(s) / len(O), maxang=ang.max(), maxdist=dist.max(), ang=ang, dist=dist, degenerate=bool(deg.any()))


def group_degenerate64(O, D):
    if ray_degenerate(O, D).any():
        return True
    g = group64(O, D)
    theta = g["maxang"] * (1.0 + K_REL) + K_ANG
    if g["sumlen"] < 0.09 or theta > HALF_PI + 5.0e-4:
        return True
    if g["sumlen"] < 0.11 or theta > HALF_PI - 5.0e-4:
        return None
    return False


def keep_bundle64(O, D, centre, axis, sph):
    """rtx_reflect.hpp's keep condition in float64 with every margin doubled (module docstring); a non-finite sphere is kept."""
    g = group64(O, D, centre, axis)
    c = np.asarray(centre, dtype=np.float64)
    rho = g["maxdist"] * (1.0 + 2.0 * K_REL)
    theta = g["maxang"] * (1.0 + 2.0 * K_REL) + 2.0 * K_ANG
    slack = 2.0e-5 * (np.abs(c).sum() + rho)
    v = sph[:, :3] - c
    with np.errstate(all="ignore"):
        Dd = norm(v)
        far = Dd + rho
        re = np.sqrt(sph[:, 3] ** 2 * (1.0 + 2.0 * KAPPA) + 2.0 * KAPPA * far * far)
        R = re * (1.0 + 2.0 * K_REL) + 2.0 * K_REL * Dd + rho + slack
        phi = angle(np.asarray(axis, dtype=np.float64)[None, :], v)
        beta = np.arcsin(np.clip(R / Dd, -1.0, 1.0))
        keep = ~(Dd > R) | (phi <= theta + beta + 2.0 * K_ANG)
    return keep | ~np.isfinite(sph).all(-1)


def ray_distance(O, D, C):
    """(m, n): float64 distance of centre C[j] from the half-line O[i] + s D[i], s >= 0."""
    dd = (D * D).sum(-1)
    w = C[:, None, :] - O[None, :, :]
    with np.errstate(all="ignore"):
        s = np.maximum((w * D[None]).sum(-1) / np.maximum(dd, 1e-300)[None], 0.0)
        return norm(w - D[None] * s[..., None])


def closest64(O, D, ids, sph, creation, planes, rel=1e-5):
    """The float64 closest hit of each ray with the production tests' rules (a sphere is hit from outside, both roots >= 0; a plane
    as Plane::Trace has it; the ray's own object `ids` excluded; ties in t go to the lower creation index): (winner, t, decided).
    winner: sphere position, plane index | bit 31, or 0xffffffff.  decided is False where some test lies within the band the shadow
    rule uses (|distance - r| < rel scale + 1e-4 r, scale the distance of the centre from the origin), or where the two best t
    are closer than 1e-4 of the larger and are not an exact tie."""
    n, m = len(O), len(sph)
    a = (D * D).sum(-1)
    T = np.full((m + len(planes), n), np.inf)
    ci = np.concatenate([np.asarray(creation, dtype=np.int64), (1 << 30) + np.arange(len(planes), dtype=np.int64)])
    obj = np.concatenate([np.arange(m, dtype=np.uint32), np.uint32(0x80000000) | np.arange(len(planes), dtype=np.uint32)])
    amb = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if m:
            C, r = sph[:, None, :3], sph[:, None, 3]
            oc = O[None] - C
            b = 2.0 * (oc * D[None]).sum(-1)
            c = (oc * oc).sum(-1) - r * r
            disc = b * b - 4.0 * a[None] * c
            t2 = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a[None])
            own = ids[None, :] == np.arange(m)[:, None]
            finite = np.isfinite(sph).all(-1)[:, None]  # (a non-finite sphere is hit by nothing: its NaN terms fail every comparison)
            hit = (disc >= 0) & (t2 >= 0) & ~own & finite
            scale = norm(oc)
            band = rel * scale + 1e-4 * np.abs(r)
            s = np.maximum(-(oc * D[None]).sum(-1) / a[None], 0.0)
            line = norm(oc + D[None] * s[..., None])
            amb |= (~own & finite & ((np.abs(line - np.abs(r)) < band) | (np.abs(scale - np.abs(r)) < band))).any(0)
            T[:m] = np.where(hit, t2, np.inf)
        for q, pl in enumerate(planes):
            pp, pn, w_, h_ = pl[:3], pl[3:6], pl[9], pl[10]
            dn = D @ pn
            t1 = ((pp - O) @ pn) / dn
            X = O + D * t1[:, None]
            inside = (X[:, 0] > pp[0] - w_ / 2) & (X[:, 0] < pp[0] + w_ / 2) & (X[:, 2] > pp[2] - h_ / 2) & (X[:, 2] < pp[2] + h_ / 2)
            own = ids == (0x80000000 | q)
            hit = (dn < -1.2e-7) & (t1 > 0) & inside & ~own
            edge = np.minimum.reduce([np.abs(X[:, 0] - (pp[0] - w_ / 2)), np.abs(X[:, 0] - (pp[0] + w_ / 2)), np.abs(X[:, 2] - (pp[2] - h_ / 2)),
                                      np.abs(X[:, 2] - (pp[2] + h_ / 2))])
            amb |= ~own & ((np.abs(dn) < 1e-5 * norm(D)) | ((dn < 0) & (t1 > 0) & (edge < rel * (norm(X - O) + 1e-9))) | (np.abs(t1) < rel * norm(pp - O)))
            T[m + q] = np.where(hit, t1, np.inf)
        if len(T) == 0:
            return np.full(n, 0xffffffff, np.uint32), np.full(n, np.inf), ~amb
        best_t = T.min(0)
        tie = T == best_t[None]
        win = np.where(tie, ci[:, None], np.int64(1) << 40).argmin(0)
        second = np.where(tie, np.inf, T).min(0)
        amb |= np.isfinite(second) & (second - best_t < 1e-4 * second)
        # a hit at or beyond the distance a ray starts from is not taken
        amb |= np.isfinite(best_t) & (best_t > 0.5 * NO_HIT)
    best = np.where(np.isfinite(best_t), obj[win], np.uint32(0xffffffff)).astype(np.uint32)
    return best, best_t, ~amb


# ---------------------------------------------------------------------------------------------- generators: points and lights

def patch(rng, scale, centre=(1.0, 2.0, -3.0)):
    """256 hit points on a wavy 16 x 16 patch of side 4 (times scale) about centre (times scale), facing +z."""
    i = np.arange(256)
    x, y = (i % 16 - 7.5) * 0.25, (i // 16 - 7.5) * 0.25
    z = 0.1 * np.sin(2.0 * x) * np.cos(1.5 * y) + 0.01 * rng.standard_normal(256)
    return (np.stack([x, y, z], axis=1) + np.asarray(centre)) * scale


def fan(rng, n, axis, half, psi0=0.0):
    """n unit directions within `half` radians of axis."""
    axis = np.asarray(axis, dtype=np.float64) / norm(np.asarray(axis, dtype=np.float64))
    e1 = any_perp(rng, axis)
    phi = half * np.sqrt(rng.uniform(0, 1, n))
    psi = rng.uniform(0, 2 * np.pi, n) + psi0
    return np.stack([unit_at(axis, e1, p, q) for p, q in zip(phi, psi)])


def wide_points(rng, open_, scale, target):
    """Points whose open ones, seen from the light returned with them, span a half-angle of `target` about their own float64 axis:
    a narrow fan and one outlier (the last open thread), found by bisection on the rounded values."""
    L = np.array([0.5, -1.0, 2.0]) * scale
    z = np.array([0.0, 0.0, -1.0])
    e1 = np.array([1.0, 0.0, 0.0])
    u = fan(rng, 256, z, 0.2)
    d = rng.uniform(2.0, 5.0, 256) * scale
    last = int(np.flatnonzero(open_)[-1])

    def build(phi):
        uu = u.copy()
        uu[last] = unit_at(z, e1, phi, 0.3)
        P = f64(f32(L + uu * d[:, None]))
        return P, cone64(f64(f32(L)), P[open_])["maxang"]

    lo, hi = 0.3, 3.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if build(mid)[1] < target:
            lo = mid
        else:
            hi = mid
    return build(lo if build(lo)[1] <= target else hi)[0], L


PLACEMENTS = ("far", "near", "under90", "over90", "hull", "at_point")


def shadow_tile(rng, pattern, scale, placement):
    """(open, P, L): the points and the light of one cone case, unrounded."""
    open_ = open_mask(rng, pattern)
    P = patch(rng, scale)
    c = np.array([1.0, 2.0, -3.0]) * scale
    if placement == "far":
        L = c + np.array([3.0, 4.0, 40.0]) * scale
    elif placement == "near":
        L = c + np.array([0.3, 0.2, 1.5]) * scale
    elif placement in ("under90", "over90"):
        if open_.sum() < 2:
            L = c + np.array([0.3, 0.2, 1.5]) * scale
        else:
            P, L = wide_points(rng, open_, scale, HALF_PI - K_ANG + (-2.0e-3 if placement == "under90" else 2.0e-3))
    elif placement == "hull":
        L = c + np.array([0.05, -0.03, 0.0]) * scale
    elif placement == "at_point":
        L = P[int(np.flatnonzero(open_)[0])] if open_.any() else c
    return open_, P, L


# ---------------------------------------------------------------------------------------------- generators: spheres

NON_FINITE = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [0, 0, 0, np.nan], [1, 1, 1, np.inf], [1, 1, 1, -np.inf]])


def random_spheres(rng, n, centre, spread, rmax):
    C = np.asarray(centre) + rng.uniform(-1, 1, (n, 3)) * spread
    r = rmax * rng.uniform(0.02, 1.0, n) ** 2
    return np.concatenate([C, r[:, None]], axis=1)


def spheres_for_cone(rng, open_, P, L, scale, n_random=300):
    """Spheres against one shadow tile (P, L already rounded, float64): grazing the nearest segment, at the cone's rim, beyond dmax,
    around, behind and enclosing the light, non-finite ones, and n_random random ones."""
    out = [NON_FINITE * np.array([scale, scale, scale, scale])]
    Po = P[open_]
    mid = 0.5 * (Po.mean(0) + L)
    reach = norm(Po - L).max()
    out.append(random_spheres(rng, n_random, mid, 0.8 * reach + scale, 0.3 * reach + 0.2 * scale))
    finite = np.isfinite(Po).all(-1)
    if finite.any() and np.isfinite(reach) and reach > 0:
        Pf = Po[finite]
        # grazing a segment: the closest point at s (also before P and past L, where an end point is the nearest), gap +-g r
        for g in GAPS:
            for sign in (-1.0, 1.0):
                for s in (0.3, 0.7, -0.2, 1.2):
                    p = Pf[rng.integers(len(Pf))]
                    d = L - p
                    if not norm(d) > 0:
                        continue
                    r = rng.uniform(0.05, 0.5) * scale
                    foot = p + d * min(max(s, 0.0), 1.0)
                    dirn = any_perp(rng, d) if 0.0 <= s <= 1.0 else (-d / norm(d) if s < 0 else d / norm(d))
                    out.append(np.concatenate([foot + dirn * r * (1.0 + sign * g), [r]])[None])
        # a negative radius: the exact tests square it, so it is the sphere of radius |r|; across a segment, and clear of the cone
        for k in range(4):
            p = Pf[rng.integers(len(Pf))]
            r = rng.uniform(0.05, 0.5) * scale
            out.append(np.concatenate([p + (L - p) * rng.uniform(0.2, 0.8) + any_perp(rng, L - p) * r * (0.5 if k < 2 else 400.0), [-r]])[None])
        c = cone64(L, Pf)
        axis = c["axis64"]
        if np.isfinite(axis).all():
            e1 = any_perp(rng, axis)
            for m in MARGIN_STEPS + (100.0, 3000.0):
                # the rim: the centre at theta + asin(r / D) + m A from the axis
                D = rng.uniform(0.2, 0.9) * c["maxdist"]
                r = rng.uniform(0.02, 0.2) * D
                phi = c["maxang"] + np.arcsin(r / D) + m * K_ANG
                if phi < np.pi:
                    out.append(np.concatenate([L + unit_at(axis, e1, phi, rng.uniform(0, 6.28)) * D, [r]])[None])
                # beyond dmax: the near surface m K dmax past it, on the axis and off it
                r = rng.uniform(0.05, 0.5) * scale
                D = c["maxdist"] * (1.0 + m * K_REL) + r
                out.append(np.concatenate([L + unit_at(axis, e1, 0.5 * c["maxang"], rng.uniform(0, 6.28)) * D, [r]])[None])
            # around and behind the light, and enclosing it
            for k in range(6):
                r = rng.uniform(0.05, 0.3) * scale
                out.append(np.concatenate([L + fan(rng, 1, -axis, 1.5)[0] * r * rng.uniform(1.01, 4.0), [r]])[None])
            out.append(np.concatenate([L + axis * 0.1 * scale, [0.5 * scale]])[None])
            out.append(np.concatenate([L - axis * 0.2 * scale, [0.21 * scale]])[None])
    sph = np.concatenate(out)
    return sph[rng.permutation(len(sph))]


def spheres_for_rays(rng, open_, O, D, scale, n_random=300):
    """Spheres against one mirror tile (O, D rounded, float64): grazing the nearest ray, at each group's rim and ball, around, behind
    and enclosing the origins, non-finite ones, and n_random random ones."""
    out = [NON_FINITE * np.array([scale, scale, scale, scale])]
    ok = open_ & ~ray_degenerate(O, D) & np.isfinite(O).all(-1)
    if not ok.any():
        out.append(random_spheres(rng, n_random, np.zeros(3), 10 * scale, 2 * scale))
        sph = np.concatenate(out)
        return sph[rng.permutation(len(sph))]
    Oo, Do = O[ok], D[ok]
    u = Do / norm(Do)[:, None]
    out.append(random_spheres(rng, n_random, Oo.mean(0), 12 * scale, 2 * scale))
    for g in GAPS:
        for sign in (-1.0, 1.0):
            for s in (2.0, 9.0, -0.5):
                k = rng.integers(len(Oo))
                r = rng.uniform(0.05, 0.5) * scale
                foot = Oo[k] + u[k] * max(s, 0.0) * scale
                dirn = any_perp(rng, u[k]) if s >= 0 else -u[k]
                out.append(np.concatenate([foot + dirn * r * (1.0 + sign * g), [r]])[None])
    for k in range(4):  # a negative radius, across a ray and clear of the bundles
        j = rng.integers(len(Oo))
        r = rng.uniform(0.05, 0.5) * scale
        out.append(np.concatenate([Oo[j] + u[j] * rng.uniform(2.0, 9.0) * scale + any_perp(rng, u[j]) * r * (0.5 if k < 2 else 400.0), [-r]])[None])
    groups, _ = groups64(ok, O, D)
    for members in groups:
        gm = group64(O[members], D[members])
        axis, centre = gm["axis64"], O[members].mean(0)
        if not np.isfinite(axis).all():
            continue
        e1 = any_perp(rng, axis)
        for m in MARGIN_STEPS + (100.0, 3000.0):
            # the rim: the sphere's distance from the cone about (centre, axis) is r + rho + m (K D + A D)
            Dd = rng.uniform(5.0, 20.0) * scale
            r = rng.uniform(0.05, 0.5) * scale
            phi = gm["maxang"] + np.arcsin(min(1.0, (r + gm["maxdist"]) / Dd)) + m * K_ANG
            if phi < np.pi:
                out.append(np.concatenate([centre + unit_at(axis, e1, phi, rng.uniform(0, 6.28)) * Dd, [r]])[None])
            # the ball: behind the origins, the surface m K (r + rho) outside the ball of radius rho
            r = rng.uniform(0.05, 0.5) * scale
            Dd = (r + gm["maxdist"]) * (1.0 + m * K_REL)
            out.append(np.concatenate([centre - axis * Dd, [r]])[None])
        out.append(np.concatenate([centre, [gm["maxdist"] * 2.0 + scale]])[None])  # encloses the ball
        out.append(np.concatenate([centre - axis * 3.0 * scale, [0.5 * scale]])[None])  # behind it
    sph = np.concatenate(out)
    return sph[rng.permutation(len(sph))]


# ---------------------------------------------------------------------------------------------- generators: rays

RAY_SETS = ("fan", "two_fans", "corner", "five_clusters", "identical", "t255", "zero_dir", "inf_dir", "nan_origin", "none")


def _cluster_axes(k):
    """k unit vectors pairwise more than 60 degrees apart (and more than 1e-3 in the dot product from 0.5)."""
    axes = np.array([[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0], [-1.0, 0, 0]])
    return axes[:k]


def ray_set(rng, name, scale):
    """(open, O, D) of one mirror case, unrounded: origins on a patch, directions by the set's name."""
    open_ = np.ones(256, bool)
    O = patch(rng, scale, centre=(0.5, -1.0, 2.0))
    lens = rng.uniform(0.5, 2.0, 256)[:, None]
    if name in ("fan", "zero_dir", "inf_dir", "nan_origin", "t255", "none", "identical"):
        D = fan(rng, 256, [0.3, 0.2, 1.0], 0.15) * lens
    elif name in ("two_fans", "corner", "five_clusters"):
        k = {"two_fans": 2, "corner": 3, "five_clusters": 5}[name]
        axes = _cluster_axes(k)
        # clusters of equal size: where the last bundle takes two of them its axis is their bisector, so that its half-angle stays
        # below 1 rad, up to which theta's relative margin (1e-4 of it) is within the absolute one C2 allows
        which = rng.permutation(np.arange(256) % k)
        D = np.stack([fan(rng, 1, axes[w], 0.12)[0] for w in which]) * lens
    if name == "identical":
        D[:] = D[0]
        O[:] = O[0]
    elif name == "t255":
        open_[:] = False
        open_[255] = True
    elif name == "zero_dir":
        D[37] = 0.0
    elif name == "inf_dir":
        D[130, 1] = np.inf
    elif name == "nan_origin":
        O[200, 0] = np.nan
    elif name == "none":
        open_[:] = False
    return open_, O, D


# ---------------------------------------------------------------------------------------------- generators: the walk's scenes

def walk_tile(rng, count, mode):
    """A shadow tile for the list accounting: `count` spheres under brute, under a cone that keeps about half of them, or under one
    that keeps fewer than ten.  (open, P, L, spheres, brute)"""
    open_ = np.ones(256, bool)
    P = patch(rng, 1.0)
    L = np.array([1.0, 2.0, -3.0]) + np.array([1.0, -2.0, 12.0])
    c = cone64(L, P)
    axis, e1 = c["axis64"], any_perp(rng, c["axis64"])
    n_in = count if mode == "brute" else ((count + 1) // 2 if mode == "half" else min(count, 7))
    inside = rng.permutation(count) < n_in
    sph = np.zeros((count, 4))
    for j in range(count):
        r = 0.02 + 0.2 * rng.uniform() ** 2
        if inside[j] or mode == "brute":
            # within the cone, between light and points, sized so that together they shadow about a third of the tile
            D = rng.uniform(0.15, 0.9) * c["maxdist"]
            r = D * c["maxang"] * 0.55 / np.sqrt(n_in + 1.0) * rng.uniform(0.5, 1.1)
            sph[j] = np.concatenate([L + unit_at(axis, e1, rng.uniform(0, 0.9) * c["maxang"], rng.uniform(0, 6.28)) * D, [r]])
        else:
            D = rng.uniform(0.3, 3.0) * c["maxdist"]
            phi = c["maxang"] + np.arcsin(min(1.0, r / D)) + rng.uniform(0.05, 2.0)
            sph[j] = np.concatenate([L + unit_at(axis, e1, min(phi, 3.1), rng.uniform(0, 6.28)) * D, [r]])
    return open_, P, L, sph, 1 if mode == "brute" else 0


def mirror_walk_tile(rng, count, mode):
    """The same for the mirror walk: rays of one narrow fan, `count` spheres.  (open, O, D, spheres, brute)"""
    open_, O, D = ray_set(rng, "fan", 1.0)
    g = group64(f64(f32(O)), f64(f32(D)))
    axis, e1, centre = g["axis64"], any_perp(rng, g["axis64"]), O.mean(0)
    n_in = count if mode == "brute" else ((count + 1) // 2 if mode == "half" else min(count, 7))
    inside = rng.permutation(count) < n_in
    sph = np.zeros((count, 4))
    for j in range(count):
        r = 0.05 + 0.4 * rng.uniform() ** 2
        Dd = rng.uniform(6.0, 40.0)
        if inside[j] or mode == "brute":
            r = Dd * g["maxang"] * 0.7 / np.sqrt(n_in + 1.0) * rng.uniform(0.5, 1.2)  # together they stop about a third of the rays
            sph[j] = np.concatenate([centre + unit_at(axis, e1, rng.uniform(0, 1.0) * g["maxang"], rng.uniform(0, 6.28)) * Dd, [r]])
        else:
            phi = g["maxang"] + np.arcsin(min(1.0, (r + g["maxdist"]) / Dd)) + rng.uniform(0.1, 2.0)
            sph[j] = np.concatenate([centre + unit_at(axis, e1, min(phi, 3.1), rng.uniform(0, 6.28)) * Dd, [r]])
    return open_, O, D, sph, 1 if mode == "brute" else 0


# ---------------------------------------------------------------------------------------------- generators: the dark set

DARK_LIGHTS = (1, 2, 3, 8)


def dark_tile(rng, nl, n_planes, n_spheres=180):
    """A tile of the light-set pass: hit points on a sphere's cap (ids: that sphere) and on a floor plane's strip (ids: plane 0 when
    there are planes), nl lights of which two share a position (nl >= 2) and one lies below every point's horizon (nl >= 3: no
    open pixel), spheres between lights and points.  (testable, P, N, ids, spheres, lights)"""
    sph = np.zeros((n_spheres, 4))
    sph[0] = [0.0, 1.0, 0.0, 1.0]  # the sphere half of the points lie on
    testable = np.ones(256, bool)
    testable[rng.choice(256, 9, replace=False)] = False
    P, N, ids = np.zeros((256, 3)), np.zeros((256, 3)), np.zeros(256, np.uint32)
    for t in range(256):
        if t % 2 == 0:
            n = fan(rng, 1, [0.0, 1.0, 0.3], 0.9)[0]
            P[t], N[t], ids[t] = sph[0, :3] + n * sph[0, 3], n, 0
        else:
            P[t] = [rng.uniform(-3, 3), 0.0, rng.uniform(1.2, 4.0)]
            N[t] = [0.0, 1.0, 0.0]
            ids[t] = 0x80000000 if n_planes else 1
    if not n_planes:
        sph[1] = [0.0, -50.0, 2.5, 50.0]  # a big ball for a floor: its points are excluded from it by id
    lights = np.zeros((nl, 3))
    for i in range(nl):
        lights[i] = [rng.uniform(-6, 6), rng.uniform(5, 9), rng.uniform(-2, 6)]
    if nl >= 2:
        lights[1] = lights[0]
    if nl >= 3:
        lights[2] = [0.5, -80.0, 1.0]  # below the floor: every point faces away from it
    for j in range(n_spheres - 30, n_spheres):  # far to the sides: outside every light's cone
        a = rng.uniform(0, 6.28)
        sph[j] = [40.0 * np.cos(a), rng.uniform(0, 4), 40.0 * np.sin(a), rng.uniform(0.1, 1.0)]
    for j in range(2, n_spheres - 30):
        i = rng.integers(nl)
        p = P[rng.integers(256)]
        s = rng.uniform(0.15, 0.85)
        c = p + (lights[i] - p) * s + rng.standard_normal(3) * 0.4
        sph[j] = [c[0], c[1], c[2], 0.03 + 0.15 * rng.uniform() ** 2]
    return testable, P, N, ids, sph, lights


def dark_planes():
    """Two planes in the helper's layout (p, n, colour, w, h): the floor y = 0 the points lie on, and a panel above it that cuts
    some segments."""
    return np.array([[0.0, 0.0, 2.0, 0.0, 1.0, 0.0, 0.5, 0.5, 0.5, 30.0, 30.0],
                     [1.0, 3.5, 2.0, 0.0, -1.0, 0.0, 0.5, 0.5, 0.5, 2.5, 2.0]])


def as_helper_spheres(sph):
    """(n, 4) -> the (n, 7) rows restate_shadows.classify64_points reads."""
    return np.concatenate([np.asarray(sph, dtype=np.float64), np.zeros((len(sph), 3))], axis=1)


# ---------------------------------------------------------------------------------------------- the classes' launches

def _seed(*k):
    return np.random.default_rng([20231, *[int(x) for x in k]])


_FOUR = np.array([[0.0, 0.0, 0.0, 1.0], [5.0, 5.0, 5.0, 0.5], [-3.0, 2.0, 1.0, 0.25], [1.0, 2.0, 0.0, 0.1]])


def cone_cases():
    """Every (placement, scale, pattern) of the cone class and its specials, for one launch of the cone entry point.  index:
    key -> tile; the specials' keys are ("huge", pattern), ("nan", pattern), ("no_spheres", pattern), ("brute", pattern)."""
    ts, index = TileSet(), {}
    for a, placement in enumerate(PLACEMENTS):
        for b, scale in enumerate(SCALES):
            for c, pattern in enumerate(PATTERNS):
                open_, P, L = shadow_tile(_seed(1, a, b, c), pattern, scale, placement)
                index[(placement, scale, pattern)] = ts.add(open_, P=P, lights=L, spheres=_FOUR * scale)
    for c, pattern in enumerate(PATTERNS):
        rng = _seed(2, c)
        open_, P, L = shadow_tile(rng, pattern, 1.0e37, "near")  # slack = 1e-5 (|L|_1 + dmax) passes 3e37
        index[("huge", pattern)] = ts.add(open_, P=P, lights=L, spheres=_FOUR)
        open_, P, L = shadow_tile(rng, pattern, 1.0, "far")
        if open_.any():
            P[int(np.flatnonzero(open_)[-1]), 1] = np.nan
        index[("nan", pattern)] = ts.add(open_, P=P, lights=L, spheres=_FOUR)
        open_, P, L = shadow_tile(rng, pattern, 1.0, "far")
        index[("no_spheres", pattern)] = ts.add(open_, P=P, lights=L)
        index[("brute", pattern)] = ts.add(open_, P=P, lights=L, spheres=_FOUR, brute=1)
    return ts, index


SPHERE_PATTERNS = ("all", "scattered17", "t255")
TIGHT_PLACEMENTS = ("far", "near", "under90")       # a cone that culls: S1, S2, T
KEEP_ALL_PLACEMENTS = ("over90", "hull", "at_point")  # a degenerate one: D


def shadow_sphere_cases():
    """The spheres class of the shadow walk: index[(placement, scale, pattern)] -> tile, each with spheres_for_cone's spheres."""
    ts, index = TileSet(), {}
    for a, placement in enumerate(PLACEMENTS):
        for b, scale in enumerate(SCALES):
            for c, pattern in enumerate(SPHERE_PATTERNS):
                if placement in KEEP_ALL_PLACEMENTS and pattern == "t255":
                    continue  # (one point has neither a hull nor a wide cone)
                rng = _seed(3, a, b, c)
                open_, P, L = shadow_tile(rng, pattern, scale, placement)
                P, L = f64(f32(P)), f64(f32(L))
                sph = spheres_for_cone(rng, open_, P, L, scale)
                ids = rng.integers(0, len(sph), 256)
                with np.errstate(all="ignore"):
                    N = (L - P) / norm(L - P)[:, None]
                index[(placement, scale, pattern)] = ts.add(open_, P=P, N=np.nan_to_num(N), ids=ids, lights=L, spheres=sph)
    for c, pattern in enumerate(SPHERE_PATTERNS):
        rng = _seed(4, c)
        open_, P, L = shadow_tile(rng, pattern, 1.0e37, "near")
        P, L = f64(f32(P)), f64(f32(L))
        sph = np.concatenate([NON_FINITE, random_spheres(rng, 100, P.mean(0), 1e38, 1e36)])
        index[("huge", 1.0e37, pattern)] = ts.add(open_, P=P, ids=rng.integers(0, len(sph), 256), lights=L, spheres=sph)
        open_, P, L = shadow_tile(rng, pattern, 1.0, "far")
        P[int(np.flatnonzero(open_)[-1]), 1] = np.nan
        sph = np.concatenate([NON_FINITE, random_spheres(rng, 100, P[0], 30.0, 2.0)])
        index[("nan", 1.0, pattern)] = ts.add(open_, P=P, ids=rng.integers(0, len(sph), 256), lights=L, spheres=sph)
    return ts, index


def shadow_walk_cases():
    """The walk's counts: index[(count, mode, brute)] -> tile; brute 1 is the same tile with every sphere kept."""
    ts, index = TileSet(), {}
    for a, count in enumerate(WALK_COUNTS):
        for b, mode in enumerate(WALK_MODES):
            rng = _seed(5, a, b)
            open_, P, L, sph, brute = walk_tile(rng, count, mode)
            P, L = f64(f32(P)), f64(f32(L))
            ids = rng.integers(0, count, 256) if count else np.full(256, 0x80000000, np.uint32)
            N = (L - P) / norm(L - P)[:, None]
            for br in sorted({brute, 1}):
                index[(count, mode, br)] = ts.add(open_, P=P, N=N, ids=ids, lights=L, spheres=sph, brute=br)
    return ts, index


def dark_cases():
    """index[(nl, n_planes, brute)] -> tile."""
    ts, index = TileSet(dark_planes()), {}
    for a, nl in enumerate(DARK_LIGHTS):
        for n_planes in (0, 2):
            testable, P, N, ids, sph, lights = dark_tile(_seed(6, a, n_planes), nl, n_planes)
            for br in (0, 1):
                index[(nl, n_planes, br)] = ts.add(testable, P=P, N=N, ids=ids, lights=lights, spheres=sph, brute=br, np_=n_planes)
    return ts, index


def bundle_cases(with_spheres):
    """index[(ray set, scale)] -> tile, and ("brute", scale): the five clusters under brute.  with_spheres: spheres_for_rays'
    spheres and random own objects (the mirror walk's spheres class); else four spheres (the bundles class)."""
    ts, index = TileSet(), {}
    for a, name in enumerate(RAY_SETS):
        for b, scale in enumerate(SCALES):
            rng = _seed(7, a, b)
            open_, O, D = ray_set(rng, name, scale)
            O, D = f64(f32(O)), f64(f32(D))
            sph = spheres_for_rays(rng, open_, O, D, scale) if with_spheres else _FOUR * scale
            index[(name, scale)] = ts.add(open_, O=O, D=D, ids=rng.integers(0, len(sph), 256), spheres=sph)
            if name == "five_clusters":
                index[("brute", scale)] = ts.add(open_, O=O, D=D, ids=rng.integers(0, len(sph), 256), spheres=sph, brute=1)
    return ts, index


def mirror_planes():
    """A ceiling every ray of the fan reaches and a panel below it that stops some of them."""
    return np.array([[0.0, 4.0, 14.0, 0.0, -1.0, 0.0, 0.5, 0.5, 0.5, 60.0, 60.0],
                     [3.0, 1.5, 14.0, 0.0, -1.0, 0.0, 0.5, 0.5, 0.5, 8.0, 8.0]])


def mirror_walk_cases():
    """index[(count, mode, brute)] -> tile, as shadow_walk_cases; two planes; and ("coincident", brute), ("own", brute): pairs of
    coincident spheres of which the later position has the lower creation index, and rays that leave the sphere they would hit."""
    ts, index = TileSet(mirror_planes()), {}
    for a, count in enumerate(WALK_COUNTS):
        for b, mode in enumerate(WALK_MODES):
            rng = _seed(8, a, b)
            open_, O, D, sph, brute = mirror_walk_tile(rng, count, mode)
            O, D = f64(f32(O)), f64(f32(D))
            ids = rng.integers(0, count, 256) if count else np.full(256, 0x80000001, np.uint32)
            ids[::7] = 0x80000000  # some rays leave the ceiling
            for br in sorted({brute, 1}):
                index[(count, mode, br)] = ts.add(open_, O=O, D=D, ids=ids, spheres=sph, brute=br, np_=2)
    rng = _seed(9)
    open_, O, D, sph, _ = mirror_walk_tile(rng, 40, "brute")
    O, D = f64(f32(O)), f64(f32(D))
    sph = f64(f32(sph))
    sph[:, 3] *= 4.0  # big enough that most rays hit something
    two = np.concatenate([sph, sph])
    creation = np.concatenate([np.arange(40) + 100, np.arange(40)])  # the copy at position 40 + j was created first
    ids = np.full(256, 0x80000000, np.uint32)
    for br in (0, 1):
        index[("coincident", br)] = ts.add(open_, O=O, D=D, ids=ids, spheres=two, creation=creation, brute=br)
    first, _, _ = closest64(O, D, ids, sph, np.arange(40), np.zeros((0, 11)))
    for br in (0, 1):
        index[("own", br)] = ts.add(open_, O=O, D=D, ids=first, spheres=sph, brute=br)  # (a ray that hits nothing leaves "no object")
    return ts, index


# ---------------------------------------------------------------------------------------------- what a case must hold (no device)

def shadow_counts(t, axis=None, decide=True):
    """Of one shadow tile: spheres the doubled-margin rule keeps / rejects (about `axis`; None: the float64 axis), spheres within r
    of an open segment, and the float64 decision of every open point by the shared rule (1 shadowed, 0 lit, -1 undecided)."""
    import restate_shadows as RH
    o, L = t["open"], t["lights"][0]
    P = t["P"][o]
    keep = keep_cone64(L, P, cone64(L, P)["axis64"] if axis is None else axis, t["sph"]) if len(P) and len(t["sph"]) else np.ones(len(t["sph"]), bool)
    near = (segment_distance(P, L, t["sph"][:, :3]) < np.abs(t["sph"][:, 3])[:, None]).any(1) if len(P) and len(t["sph"]) else np.zeros(len(t["sph"]), bool)
    k = np.zeros(0, int)
    if decide and len(P):
        with np.errstate(all="ignore"):
            k = RH.classify64_points(P, t["N"][o], t["id"][o].astype(np.int64), as_helper_spheres(t["sph"]), np.zeros((0, 11)), L)
    return dict(keep=keep, near=near, decision=k)


def dark_decisions(t):
    """Of one dark-set tile: (256, nl) decisions of the shared rule; rows of points that are not testable are 0."""
    import restate_shadows as RH
    o = t["open"]
    own = np.where(t["id"] & 0x80000000, len(t["sph"]) + (t["id"] & 0x7fffffff).astype(np.int64), t["id"].astype(np.int64))
    out = np.zeros((256, len(t["lights"])), np.int64)
    for i, L in enumerate(t["lights"]):
        out[o, i] = RH.classify64_points(t["P"][o], t["N"][o], own[o], as_helper_spheres(t["sph"]), t["planes"], L)
    return out


def mirror_counts(t, bundles=None):
    """Of one mirror tile: spheres the doubled-margin rule keeps for some group (about the device's (centre, axis) list `bundles`;
    None: the float64 ones), spheres within r of an open ray, and the groups."""
    o = t["open"]
    groups, closest = groups64(o, t["O"], t["D"], bool(t["brute"]))
    m = len(t["sph"])
    keep = np.zeros(m, bool)
    for g, members in enumerate(groups):
        O, D = t["O"][members], t["D"][members]
        if group_degenerate64(O, D) is not False:
            keep[:] = True
            continue
        ref = group64(O, D)
        centre, axis = (O.mean(0), ref["axis64"]) if bundles is None else bundles[g]
        keep |= keep_bundle64(O, D, centre, axis, t["sph"])
    ok = o & ~ray_degenerate(t["O"], t["D"])
    near = (ray_distance(t["O"][ok], t["D"][ok], t["sph"][:, :3]) < np.abs(t["sph"][:, 3])[:, None]).any(1) if ok.any() and m else np.zeros(m, bool)
    return dict(keep=keep, near=near, groups=groups, closest=closest)
