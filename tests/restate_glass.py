"""Glass (include/rtx.h at rtx_scene_set_refraction) restated in numpy, one float32 operation per IEEE operation of
csrc/rtx_refract.hpp::through_sphere and of secondary_ray (csrc/rtx_tile_pass.inc), and the scenes tests/test_gpu_glass.py renders.
  * trace_chain_glass: restate.trace_chain with the second way to form the next ray of a chain; it returns trace_chain's dict, so
    restate.shade_chain, values8, encode_records and encode_words serve unchanged;
  * dark_sets: the shadow test of RTX_OPT_SHADOWS / RTX_OPT_REFLECT_SHADOWS in fp32 as the kernels' exact tests state it
    (shadowed_before_spheres and segment_hits_sphere of csrc/rtx_tile_pass.inc), so that shadowed frames compare on every pixel;
  * scene_a, scene_b: the two scenes; scene_c, scene_d: those of tests/test_gpu_glass_edges.py, where glass spheres overlap other
    objects, sink into the floor and hold other spheres, and edge_classes, which counts the rays that start there.
tests/test_host_restate_glass.py states the input conditions of the GPU tests on this file alone."""
import numpy as np

import oracle as O
import restate as RS
import util as U

f32 = np.float32


def refract_sphere(P, N, V, r, ior):
    """through_sphere: the ray (o, d) that leaves the far side.  P, N, V: three float32 arrays each; r, ior: float32 arrays."""
    ci = RS._dot(N, V)
    eta = f32(1.0) / ior
    s2 = (eta * eta) * (f32(1.0) - ci * ci)
    c2 = f32(1.0) - s2
    ct = np.sqrt(np.where(c2 > f32(0.0), c2, f32(0.0)).astype(np.float32))
    g = eta * ci - ct
    T = tuple(N[q] * g - V[q] * eta for q in range(3))
    L = (f32(2.0) * r) * ct
    o = tuple(P[q] + T[q] * L for q in range(3))
    m = f32(2.0) * RS._dot(T, V)
    d = tuple(V[q] - T[q] * m for q in range(3))
    return o, d


def trace_chain_glass(p, sph, pl, ks, iors, pix, max_depth=4, wrong=None):
    """restate.trace_chain with ior per object (a dict {creation index: ior} or an array; 0: a mirror).  Level j + 1's ray is the
    mirror ray of level j where ior(o_j) = 0, the ray through the sphere where o_j is a sphere, and the ray going on from P_j where
    o_j is a plane.  Each level >= 1 also carries `glass`: the ray was refracted, not mirrored.
    `wrong` restates one bug a kernel could have, for tests/test_host_restate_glass.py to show that the scenes would let it be seen:
    "origin" (the ray through a sphere starts at P_j, not at the exit point), "own" (a secondary ray is tested against the object
    it left as well), "radius" (the chord is taken with the radius of the sphere created before)."""
    assert wrong in (None, "origin", "own", "radius")
    sph = np.asarray(sph, dtype=np.float32).reshape(-1, 7)
    pl = RS.host_planes(pl)
    W = int(p.x)
    n = len(pix)
    ns = len(sph)
    kk = RS.k_array(ks, ns + len(pl))
    ii = RS.k_array(iors, ns + len(pl))
    radius = np.concatenate([np.roll(sph[:, 3], 1) if wrong == "radius" else sph[:, 3], np.zeros(len(pl), np.float32)]).astype(np.float32)
    odall = np.concatenate([sph[:, 4:7], pl[:, 6:9]]).astype(np.float32) / f32(255.0)
    with np.errstate(all="ignore"):
        O3, D = RS.primary_rays(p, pix)
        a = RS._dot(D, D)
        t, gid = RS._closest(O3, D, sph, pl, a, f32(4.0) * a, f32(1.0) / (f32(2.0) * a))
        hitm = gid >= 0
        P = tuple(O3[k] + D[k] * t for k in range(3))
        normal = RS._normal(P, sph, pl, gid)
        sv = ((normal[0] * f32(1.0) + normal[1] * f32(0.0)) + normal[2] * f32(0.0)).astype(np.float32)
    od = odall[np.maximum(gid, 0)]
    k0 = np.where(hitm, kk[np.maximum(gid, 0)], f32(0.0)).astype(np.float32)
    chain = hitm & (t <= f32(p.cam_far)) & (pix % W != W - 1) & (k0 > f32(0.0))
    levels = [dict(exists=np.ones(n, dtype=bool), idx=np.arange(n), O=O3, D=D, t=t, gid=gid, normal=normal,
                   od=[od[:, q] for q in range(3)], k=k0)]
    idx = np.nonzero(chain)[0]
    cur = dict(O=tuple(x[idx] for x in O3), D=tuple(x[idx] for x in D), t=t[idx], normal=tuple(x[idx] for x in normal), gid=gid[idx])
    for j in range(max_depth):
        ex = np.zeros(n, dtype=bool)
        ex[idx] = True
        with np.errstate(all="ignore"):
            N = RS._nrm(*cur["normal"])
            V = RS._nrm(*(cur["D"][q] * f32(-1.0) for q in range(3)))
            c = f32(2.0) * RS._dot(N, V)
            Pj = tuple(cur["O"][q] + cur["D"][q] * cur["t"] for q in range(3))
            Rd = tuple(N[q] * c - V[q] for q in range(3))
            Ro = Pj
            ior = ii[cur["gid"]]
            glass = ior > f32(0.0)
            is_sphere = cur["gid"] < ns
            if glass.any():
                go_, gd = refract_sphere(Pj, N, V, radius[cur["gid"]], np.where(glass, ior, f32(1.0)).astype(np.float32))
                through = glass & is_sphere
                sheet = glass & ~is_sphere
                if wrong != "origin":
                    Ro = tuple(np.where(through, go_[q], Pj[q]).astype(np.float32) for q in range(3))
                Rd = tuple(np.where(through, gd[q], np.where(sheet, cur["D"][q], Rd[q])).astype(np.float32) for q in range(3))
            a2 = RS._dot(Rd, Rd)
            t2, g2 = RS._closest(Ro, Rd, sph, pl, a2, f32(4.0) * a2, f32(1.0) / (f32(2.0) * a2), exclude=None if wrong == "own" else cur["gid"])
            P2 = tuple(Ro[q] + Rd[q] * t2 for q in range(3))
            n2 = RS._normal(P2, sph, pl, g2)
        od2 = odall[np.maximum(g2, 0)]
        k2 = np.where(g2 >= 0, kk[np.maximum(g2, 0)], f32(0.0)).astype(np.float32)
        levels.append(dict(exists=ex, idx=idx, O=Ro, D=Rd, P=Ro, Rd=Rd, t=t2, gid=g2, normal=n2, od=[od2[:, q] for q in range(3)],
                           k=k2, left=cur["gid"], glass=glass))
        go = (g2 >= 0) & (k2 > f32(0.0))
        idx = idx[go]
        cur = dict(O=tuple(x[go] for x in Ro), D=tuple(x[go] for x in Rd), t=t2[go], normal=tuple(x[go] for x in n2), gid=g2[go])
    return dict(p=p, W=W, n=n, pix=pix, sph=sph, pl=pl, t=t, gid=gid, sv=sv, normal=normal, hit=hitm, vis=hitm & (pix % W != W - 1),
                levels=levels, rays=[int(l["exists"].sum()) for l in levels[1:]], max_depth=max_depth, _deep={})


# ---------------------------------------------------------------- the shadow test, in fp32

def _dark_points(P, N, owner, sph, pl, light_pos):
    """Is the point P (normal N, on object `owner`) cut off from the light?  The kernels' exact tests, operation for operation:
    facing away (N . toL <= 0), then every plane but its own (the crossing point inside the plane's rectangle, Plane.cu:66-67),
    then every sphere but its own (the closest point of the segment to the centre, closer than r)."""
    ns = len(sph)
    L = tuple(f32(v) for v in light_pos)
    toL = tuple(L[q] - P[q] for q in range(3))
    dark = RS._dot(N, toL) <= f32(0.0)
    for q, pr in enumerate(pl.astype(np.float32)):
        pp, pn = (pr[0], pr[1], pr[2]), (pr[3], pr[4], pr[5])
        sP = RS._dot(tuple(P[k] - pp[k] for k in range(3)), pn)
        sL = RS._dot(tuple(L[k] - pp[k] for k in range(3)), pn)
        cross = ((sP < f32(0.0)) & (sL > f32(0.0))) | ((sP > f32(0.0)) & (sL < f32(0.0)))
        f = sP / (sP - sL)
        x = tuple(P[k] + toL[k] * f for k in range(3))
        hw, hh = pr[9] * f32(0.5), pr[10] * f32(0.5)
        inside = ~(((x[0] <= pp[0] - hw) | (x[0] >= pp[0] + hw)) | ((x[2] <= pp[2] - hh) | (x[2] >= pp[2] + hh)))
        dark |= cross & inside & (owner != ns + q)
    len2 = RS._dot(toL, toL)
    inv = np.where(len2 > f32(0.0), f32(1.0) / len2, f32(0.0)).astype(np.float32)
    for j, s in enumerate(sph.astype(np.float32)):
        w = (s[0] - P[0], s[1] - P[1], s[2] - P[2])
        sc = RS._dot(w, toL) * inv
        k = np.where(sc < f32(0.0), f32(0.0), np.where(sc > f32(1.0), f32(1.0), sc)).astype(np.float32)
        e = tuple(w[q] - toL[q] * k for q in range(3))
        dark |= (RS._dot(e, e) < s[3] * s[3]) & (owner != j)
    return dark


def dark_sets(trace, lights, deep):
    """dark[j], j = 0 .. max_depth, as restate_shadows.shade_chain_dark takes them: per pixel the lights (bit i) level j's hit
    point is shadowed from.  Level 0: the visible pixels within the far distance; levels >= 1 (only when `deep`,
    RTX_OPT_REFLECT_SHADOWS): every level that exists and hit an object, no far limit."""
    out = []
    for j, lev in enumerate(trace["levels"]):
        d = np.zeros(trace["n"], dtype=np.int64)
        if j == 0 or deep:
            ok = lev["gid"] >= 0
            if j == 0:
                ok = ok & trace["vis"] & (lev["t"] <= f32(trace["p"].cam_far))
            with np.errstate(all="ignore"):
                P = tuple((lev["O"][q] + lev["D"][q] * lev["t"])[ok] for q in range(3))
                N = tuple(lev["normal"][q][ok] for q in range(3))
                for i, l in enumerate(lights):
                    dk = _dark_points(P, N, lev["gid"][ok], trace["sph"], trace["pl"], l.pos)
                    d[lev["idx"][ok]] |= dk.astype(np.int64) << i
        out.append(d)
    return out


# ---------------------------------------------------------------- the scenes

GW, GH = 41, 23  # 16 x 16 tiles ragged in both directions

# scene A: three glass spheres (ior 1.0, 1.5, 4.0; k 0.3 or 1.0), a mirror sphere, an opaque sphere, a floor (patterned by the GPU
# tests: restate_pattern.SCENE_A_TABLE's first entry) and a glass plane standing upright between the camera and the spheres
A_SPH = np.array([[-5, 4, 30, 4, 230, 40, 40], [0, 5, 38, 5, 40, 230, 40], [5.5, 4, 30, 4, 40, 40, 230], [2, 3, 22, 2.5, 230, 230, 40],
                  [-3, 2.5, 23, 2, 200, 120, 60]], dtype=np.float32)
A_PL = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80], [4, 4, 15, 0, 0, -1, 90, 140, 160, 5, 12]], dtype=np.float32)
A_KS = {0: 1.0, 1: 0.3, 2: 1.0, 3: 0.6, 5: 0.4, 6: 0.7}  # (sphere 4 opaque; the floor a weak mirror; the sheet)
A_IORS = {0: 1.5, 1: 1.0, 2: 4.0, 6: 1.3}                # (sphere 3 a mirror)
A_FLOOR, A_MIRROR, A_SHEET = 5, 3, 6
A_LIGHTS = [(0.0, 40.0, 50.0), (-30.0, 30.0, 25.0), (30.0, 30.0, 25.0)]


def scene_a_params(W=GW, H=GH):
    return O.camera_params(W, H, pos=(0.0, 12.0, 0.0), rot=(0.3, RS.PI32, 0.0))


def lights_a(n):
    if n == 1:
        return [RS.CUSTOM_LIGHT._replace(pos=A_LIGHTS[0])]
    return RS.light_set(n, positions=A_LIGHTS[:n], scale=0.6)


_cache = {}


def scene_a():
    """(params, spheres, planes, ks, iors, pixels, trace) of scene A at 41 x 23, traced once per process."""
    if "a" not in _cache:
        p = scene_a_params()
        pix = np.arange(GW * GH)
        _cache["a"] = (p, A_SPH, A_PL, A_KS, A_IORS, pix, trace_chain_glass(p, A_SPH, A_PL, A_KS, A_IORS, pix))
    return _cache["a"]


# scene B: 300 small spheres over a floor (the direction-sorted copies exist from 256 spheres on), every fourth one glass
B_NS = 300


def scene_b():
    """(params, spheres, planes, ks, iors, pixels, trace)."""
    if "b" not in _cache:
        p = O.camera_params(GW, GH)
        sph, pl = U.numpy_synth_scene(7, B_NS, 1, p.element1, p.element2)
        ks = np.zeros(B_NS + 1, dtype=np.float32)
        iors = np.zeros(B_NS + 1, dtype=np.float32)
        ks[0:B_NS:4] = 0.85
        iors[0:B_NS:4] = 1.5
        ks[1:B_NS:4] = 0.5  # (mirrors among them)
        ks[B_NS] = 0.4
        pix = np.arange(GW * GH)
        _cache["b"] = (p, sph, pl, ks, iors, pix, trace_chain_glass(p, sph, pl, ks, iors, pix))
    return _cache["b"]


# scene C: glass where objects do not stand clear of each other (scene A's camera).  Sphere 0 (glass) stands in front of and
# overlaps sphere 1 (glass, ior 1.0); sphere 3, a mirror, covers the far side of sphere 2 (glass); sphere 4 (glass) is sunk into the
# floor; sphere 5 (glass), in the free corner of the frame, overlaps sphere 6, a mirror behind it; sphere 7 (glass, ior 4.0) stands
# free.  The floor (patterned by the GPU tests, as scene A's) is a weak mirror, the upright sheet glass.
C_SPH = np.array([[-4, 4, 28, 4, 230, 40, 40], [-3, 4.5, 33, 4, 40, 230, 40], [6, 4, 27, 4, 40, 40, 230], [6.5, 4, 30.5, 3, 230, 230, 40],
                  [0.5, 0, 19, 3, 200, 120, 60], [-3.5, 10, 40, 2.5, 90, 200, 200], [-2, 10, 42, 2.5, 220, 220, 220],
                  [3, 10, 36, 3, 180, 60, 200]], dtype=np.float32)
C_PL = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80], [2, 3, 14, 0, 0, -1, 90, 140, 160, 6, 10]], dtype=np.float32)
C_KS = {0: 1.0, 1: 0.7, 2: 0.9, 3: 0.5, 4: 0.8, 5: 1.0, 6: 0.6, 7: 0.5, 8: 0.4, 9: 0.7}
C_IORS = {0: 1.5, 1: 1.0, 2: 1.3, 4: 2.0, 5: 1.5, 7: 4.0, 9: 1.3}
C_FLOOR, C_SHEET, C_SUNK = 8, 9, 4
C_GLASS = (0, 1, 2, 4, 5, 7, C_SHEET)


def scene_c():
    """(params, spheres, planes, ks, iors, pixels, trace) of scene C at 41 x 23."""
    if "c" not in _cache:
        p = scene_a_params()
        pix = np.arange(GW * GH)
        _cache["c"] = (p, C_SPH, C_PL, C_KS, C_IORS, pix, trace_chain_glass(p, C_SPH, C_PL, C_KS, C_IORS, pix))
    return _cache["c"]


# scene D: 300 spheres over scene C's floor (the direction-sorted copies exist), scene B's pattern of glass and mirrors, and sphere 8
# (glass) so large that it holds dozens of the others and goes to the world grid's large list
D_NS, D_BIG, D_FLOOR = 300, 8, 300


def scene_d_objects():
    """(spheres, planes, ks, iors) of scene D."""
    rng = np.random.default_rng(11)
    sph = np.zeros((D_NS, 7), dtype=np.float32)
    for q, (lo, hi) in enumerate(((-12.0, 12.0), (0.0, 8.0), (20.0, 44.0), (0.8, 2.0))):  # x of every sphere, then y, z and r
        sph[:, q] = rng.uniform(lo, hi, D_NS)
    sph[:, 4:] = rng.integers(40, 231, (D_NS, 3))
    sph[D_BIG] = [0, 5, 34, 9, 200, 200, 230]
    ks = np.zeros(D_NS + 1, dtype=np.float32)
    iors = np.zeros(D_NS + 1, dtype=np.float32)
    ks[0:D_NS:4] = 0.85
    iors[0:D_NS:4] = 1.5
    ks[1:D_NS:4] = 0.5
    ks[D_FLOOR] = 0.4
    return sph, C_PL[:1].copy(), ks, iors


def scene_d():
    """(params, spheres, planes, ks, iors, pixels, trace) of scene D at 41 x 23."""
    if "d" not in _cache:
        p = scene_a_params()
        sph, pl, ks, iors = scene_d_objects()
        pix = np.arange(GW * GH)
        _cache["d"] = (p, sph, pl, ks, iors, pix, trace_chain_glass(p, sph, pl, ks, iors, pix))
    return _cache["d"]


def edge_classes(trace, floor):
    """Per level j >= 1 of a trace (None at 0) the classes of its refracted rays that tests/test_host_restate_glass.py and
    tests/test_gpu_glass_edges.py count, as masks over the level's rays, decided in float64 on the fp32 origins:
      glass   the ray was refracted (it left a glass sphere or went on through a glass plane);
      inside  ... and starts strictly inside a sphere other than the one it left;
      beyond  ... and starts on the far side of the plane `floor` (creation index): below it, where its normal points up;
      hit     the ray hit an object."""
    sph = trace["sph"].astype(np.float64)
    pf = trace["pl"][floor - len(sph)].astype(np.float64)
    out = [None]
    for lev in trace["levels"][1:]:
        o = np.stack([lev["O"][q] for q in range(3)], axis=1).astype(np.float64)
        d2 = ((o[:, None, :] - sph[None, :, :3]) ** 2).sum(-1)
        within = d2 < sph[None, :, 3] ** 2
        within[np.arange(len(o)), np.clip(lev["left"], 0, len(sph) - 1)] &= lev["left"] >= len(sph)
        glass = lev["glass"].copy()
        out.append(dict(glass=glass, inside=glass & within.any(1), beyond=glass & (((o - pf[:3]) * pf[3:6]).sum(1) < 0.0), hit=lev["gid"] >= 0))
    return out
