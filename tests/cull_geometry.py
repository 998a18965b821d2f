"""The float64 yardsticks of the culling geometry, shared by the direct checks that judge it (tests/test_gpu_cull_bound.py,
tests/sched_cases.py): cameras in cull_check.hip's 21-float form, pixel directions as RayTracing.cu:12-23 forms them, a rectangle's
pyramid as cross products of its corner directions, the documented margins of rtx_cull.hpp and rtx_plan.hpp, the pixel half-line
rule, and the later cameras a motion budget admits.  numpy alone: no device code, nothing of the edge basis."""
import functools
import math

import numpy as np


F32 = np.float32
KAPPA = float(F32(2.0e-6))                 # rtx_cull.hpp: kKappa, kDelta, and 1.0f + kKappa as fp32 rounds it
ONE_KAPPA = float(F32(1.0) + F32(2.0e-6))
DELTA = float(F32(5.0e-6))


class Cam:
    def __init__(self, W, H, rot, pos, e1, e2):
        self.W, self.H = int(W), int(H)
        m = np.zeros(16, F32)
        m.reshape(4, 4)[:3, :3] = np.asarray(rot, F32)
        m.reshape(4, 4)[:3, 3] = np.asarray(pos, F32)
        m[15] = 1.0
        self.packed = np.concatenate([m, np.asarray(pos, F32), np.asarray([e1, e2], F32)]).astype(F32)

    @property
    def rot(self):  # float64 view of the float32 matrix
        return self.packed[:16].reshape(4, 4)[:3, :3].astype(np.float64)

    @property
    def pos(self):
        return self.packed[16:19].astype(np.float64)

    @property
    def e(self):
        return float(self.packed[19]), float(self.packed[20])

    def moved(self, rot=None, pos=None):
        e1, e2 = self.packed[19], self.packed[20]
        return Cam(self.W, self.H, self.rot if rot is None else rot, self.pos if pos is None else pos, e1, e2)

    def dirs(self, cx, cy):
        """Unnormalised float64 directions through view-plane points (cx, cy): M (cx e1, cy e2, 1)."""
        R, (e1, e2) = self.rot, self.e
        cx, cy = np.asarray(cx, np.float64), np.asarray(cy, np.float64)
        return (cx * e1)[..., None] * R[:, 0] + (cy * e2)[..., None] * R[:, 1] + R[:, 2]

    def pixel_dirs(self, rect):
        """Directions of the rectangle's pixels as RayTracing.cu:12-23 forms them, evaluated in float64: (w*h, 3)."""
        c0, r0, w, h = (int(v) for v in rect)
        col, row = np.meshgrid(np.arange(c0, c0 + w), np.arange(r0, r0 + h))
        return self.dirs((2.0 * col.ravel() - self.W) / self.W, (self.H - 2.0 * row.ravel()) / self.H)


def rotation(pitch, yaw, roll):
    """tests/host/test_plan.cpp: rotation()."""
    cx, sx, cy, sy, cz, sz = math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll)
    return np.array([[cy * cz + sy * sx * sz, -cy * sz + sy * sx * cz, sy * cx], [cx * sz, cx * cz, -sx],
                     [-sy * cz + cy * sx * sz, sy * sz + cy * sx * cz, cy * cx]])


def axis_rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def camera(W, H, pose):
    import util as U
    p = U.pkg().camera_params(W, H)  # the reference's element1 / element2 and its start pose
    start = np.array(p.inv_v, np.float64).reshape(4, 4)[:3, :3]
    if pose == "default":
        return Cam(W, H, start, (0.0, 0.0, 0.0), p.element1, p.element2)
    if pose == "rolled":
        return Cam(W, H, start @ axis_rotation((0, 0, 1), 0.4), (0.5, 1.0, -2.0), p.element1, p.element2)
    if pose == "general":
        return Cam(W, H, rotation(0.3, 2.0, -0.2), (3.0, -2.0, 5.0), p.element1, p.element2)
    assert pose == "far"
    return Cam(W, H, rotation(-0.25, 0.7, 0.15), (600.0, -500.0, 620.0), p.element1, p.element2)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class Pyramid:
    """A rectangle's pyramid in float64: corner directions half a pixel out, inward unit normals as cross products of the
    corner directions (k = 0 top, 1 right, 2 bottom, 3 left) and the camera plane (k = 4) -- nothing of the edge basis."""

    def __init__(self, cam, rect):
        c0, r0, w, h = (int(v) for v in rect)
        W, H = cam.W, cam.H
        x0, x1 = (2.0 * c0 - 1.0 - W) / W, (2.0 * (c0 + w) - 1.0 - W) / W
        y0, y1 = (H - 2.0 * r0 + 1.0) / H, (H - 2.0 * (r0 + h) + 1.0) / H
        self.cx, self.cy = (x0, x1), (y0, y1)
        self.corners = cam.dirs([x0, x1, x1, x0], [y0, y0, y1, y1])  # TL TR BR BL
        self.axis = unit(cam.dirs(0.5 * (x0 + x1), 0.5 * (y0 + y1)))
        n = []
        for k in range(4):
            v = unit(np.cross(self.corners[k], self.corners[(k + 1) % 4]))
            n.append(v if v @ self.axis > 0 else -v)
        n.append(unit(cam.rot[:, 2]))
        self.n = np.array(n)
        self.cam = cam

    def edge_dir(self, k, f):
        """Unit direction in side plane k, a fraction f along its edge."""
        return unit((1.0 - f) * self.corners[k] + f * self.corners[(k + 1) % 4])


def margin64(r, dist):
    """tile_culls' documented margin for radius r at distance |O| = dist, in float64."""
    return np.sqrt(r * r * ONE_KAPPA + KAPPA * dist * dist) + DELTA * dist


def moving_margin64(r, dist, theta, delta):
    """rtx_plan.hpp ("cell-list reuse"): margin' = m + delta + theta (|O| + delta + m), m = margin(r, |O| + delta)."""
    m = margin64(r, dist + delta)
    return m + delta + theta * (dist + delta + m)


def min_ray_distance(cam, rect, centres, radii, chunk=1 << 22):
    """S2's float64 rule for one rectangle: per sphere, whether some pixel half-line passes within r (1 - 1e-5) of the centre with
    the closest point at t > 0.  Spheres outside the cone around the rectangle's axis that holds all its pixel directions, by
    more than their angular radius, are settled without the walk (no half-line can come that close)."""
    w = cam.pixel_dirs(rect)
    w = w / np.linalg.norm(w, axis=1, keepdims=True)
    axis = unit(w.sum(0))
    cone = np.arccos(np.clip((w @ axis).min(), -1.0, 1.0))
    v = centres - cam.pos
    dist = np.linalg.norm(v, axis=1)
    near = np.zeros(len(v), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        ang = np.arccos(np.clip((v @ axis) / dist, -1.0, 1.0))
        reach = np.where(radii < dist, np.arcsin(np.clip(radii / dist, 0.0, 1.0)), math.pi)
        todo = np.flatnonzero(np.isfinite(dist) & np.isfinite(radii) & ~(ang > cone + reach + 1.0e-9))
    step = max(1, chunk // len(w))
    for a in range(0, len(todo), step):
        i = todo[a:a + step]
        t = v[i] @ w.T                                    # (spheres, pixels): the closest point's parameter
        d2 = (dist[i] ** 2)[:, None] - t * t
        lim = (radii[i] * (1.0 - 1.0e-5)) ** 2
        near[i] = ((t > 0.0) & (d2 < lim[:, None])).any(1)
    return near


def later_cameras(cam, pyr_normals, theta, delta, rng):
    """(class, camera, sphere motion) triples: rotations about three axes by +- the angle whose chord is 0.999 theta (or the
    largest chord cell_motion's own allowances admit), translations by +- 0.999 delta along each inward plane normal, and three
    random mixes with a part of delta left to the spheres."""
    out = []
    chord = max(0.0, min(0.999 * theta, (theta - 1.5e-6) / 1.00011))
    angle = 2.0 * math.asin(0.5 * chord)
    for axis in ((1, 0, 0), (0, 1, 0), (0.3, -0.5, 0.8)):
        for sgn in (1.0, -1.0):
            out.append(("rotation", cam.moved(rot=axis_rotation(axis, sgn * angle) @ cam.rot), 0.0))
    for n in pyr_normals:
        for sgn in (1.0, -1.0):
            out.append(("translation", cam.moved(pos=cam.pos + sgn * 0.999 * delta * n), 0.0))
    for _ in range(3):
        a, b = rng.uniform(0.3, 0.9), rng.uniform(0.2, 0.6)
        R = axis_rotation(rng.normal(size=3), 2.0 * math.asin(0.5 * a * chord))
        out.append(("mix", cam.moved(rot=R @ cam.rot, pos=cam.pos + unit(rng.normal(size=3)) * b * delta), (0.99 - b) * delta))
    return out


def moved_spheres(sph, drift, rng):
    """Every sphere moved by a random vector of length <= 0.999 drift -- where float32 can follow: a sphere whose rounded move
    would exceed drift stays where it is."""
    if drift <= 0.0:
        return sph
    step = unit(rng.normal(size=(len(sph), 3))) * (0.999 * drift * rng.uniform(0.5, 1.0, (len(sph), 1)))
    with np.errstate(invalid="ignore", over="ignore"):
        new = sph.copy()
        new[:, :3] = (sph[:, :3].astype(np.float64) + step).astype(F32)
        moved = np.linalg.norm(new[:, :3].astype(np.float64) - sph[:, :3].astype(np.float64), axis=1)
        keep = ~(moved <= drift)
    new[keep] = sph[keep]
    return new
