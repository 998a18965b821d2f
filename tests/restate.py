"""The numpy restatement the GPU tests compare the kernels with: plain numpy, no GPU, no torch.

One numpy float32 operation per IEEE operation of the kernels, in their order (the rule: include/rtx.h at
rtx_scene_set_reflectivity, rtx_scene_set_lights and RTX_OPT_SHADOWS; the header of csrc/rtx_lights_chain_kernels.inc):
  * trace_chain: the geometry of a pixel's mirror chain, once per scene: the primary hit (t, object, shadingValue, normal) and per
    level the ray, its hit, the object it left and k;
  * shade_chain: the colour floats at depths 1 .. 4 under any set of lights, level 0 with a set of dark lights;
  * encode_records / encode_words: the record and the compact pixel word of a pixel from its eight value floats, after
    oracle/rtx_oracle.c (trace_and_encode, ramp_index, u8_sat, digits3) and DESIGN.md section 3;
  * the scenes and light sets tests/test_host_restate.py states its input conditions on and tests/test_gpu_chain_lights.py renders.
tests/test_host_restate.py ties all of it to the CPU oracle where the oracle has a say (no mirrors, the reference's light)."""
import collections

import numpy as np

import oracle as O

f32 = np.float32
NO_HIT = f32(99999999.0)

Light = collections.namedtuple("Light", "pos diffuse_rgb diffuse_power specular_rgb specular_power")


def reference_light():
    """RayTracing.cu:143-157."""
    return Light((1.0, 50.0, 0.0), (1.0, 1.0, 1.0), 2000.0, (1.0, 1.0, 1.0), 3000.0)


def dark(l):
    """The light with both powers 0: what a pixel shadowed from it is shaded with."""
    return Light(tuple(l.pos), tuple(l.diffuse_rgb), 0.0, tuple(l.specular_rgb), 0.0)


def light_tuple(l):
    return (tuple(float(v) for v in l.pos), tuple(float(v) for v in l.diffuse_rgb), float(l.diffuse_power),
            tuple(float(v) for v in l.specular_rgb), float(l.specular_power))


# ---------------------------------------------------------------- the helpers (moved here from tests/test_gpu_reflect.py and
# tests/test_gpu_lights.py, which import them back under their old names)

def _nrm(x, y, z):
    inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
    return x * inv, y * inv, z * inv


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _closest(O3, D, sph, pl, a, fourA, divTwoA, exclude=None):
    """Lexicographic minimum of (t, creation index) over every sphere and plane (spheres first), from kNoHit; `exclude` the
    creation index per ray to skip, or None.  Returns (t, creation index or -1)."""
    n = D[0].shape[0]
    bt = np.full(n, f32(99999999.0), dtype=np.float32)
    bid = np.full(n, -1, dtype=np.int64)
    for j, s in enumerate(sph.astype(np.float32)):
        ox, oy, oz = O3[0] - s[0], O3[1] - s[1], O3[2] - s[2]
        cc = ((ox * ox + oy * oy) + oz * oz) - s[3] * s[3]
        sd = (D[0] * ox + D[1] * oy) + D[2] * oz
        q = sd * sd - a * cc
        b = f32(2.0) * sd
        disc = b * b - fourA * cc
        with np.errstate(invalid="ignore"):
            t2 = (-b - np.sqrt(np.maximum(disc, f32(0.0)))) * divTwoA
        hit = ~(q < f32(-1e-30)) & ~(disc < f32(0.0)) & ~(t2 < f32(0.0)) & ~np.isnan(t2)
        if exclude is not None:
            hit &= exclude != j
        take = hit & ((t2 < bt) | ((t2 == bt) & ((bid < 0) | (j < bid))))
        bt = np.where(take, t2, bt)
        bid = np.where(take, j, bid)
    ns = len(sph)
    for q, P in enumerate(pl.astype(np.float32)):
        gi = ns + q
        nn = (P[3], P[4], P[5])
        dn = _dot(D, nn)
        num = (((P[0] - O3[0]) * nn[0] + (P[1] - O3[1]) * nn[1]) + (P[2] - O3[2]) * nn[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = num / dn
        hx, hz = O3[0] + D[0] * t1, O3[2] + D[2] * t1
        hw, hh = P[9] * f32(0.5), P[10] * f32(0.5)
        hit = ~((dn > f32(0.0)) | (np.abs(dn - f32(0.0)) < f32(1.1920928955078125e-7))) & ~(t1 <= f32(0.0)) & ~np.isnan(t1)
        hit &= ~(((hx <= P[0] - hw) | (hx >= P[0] + hw)) | ((hz <= P[2] - hh) | (hz >= P[2] + hh)))
        if exclude is not None:
            hit &= exclude != gi
        take = hit & ((t1 < bt) | ((t1 == bt) & ((bid < 0) | (gi < bid))))
        bt = np.where(take, t1, bt)
        bid = np.where(take, gi, bid)
    return bt, bid


def _normal(P3, sph, pl, gid):
    """normalize_gpu of the winner's normal (RayTracing.cu:129): sphere normalize(normalize(P - C)), plane normalize(n)."""
    ns = len(sph)
    C = np.concatenate([sph[:, :3], pl[:, :3]]).astype(np.float32)[np.maximum(gid, 0)]
    Np = np.concatenate([np.zeros((ns, 3), np.float32), pl[:, 3:6].astype(np.float32)])[np.maximum(gid, 0)]
    s = _nrm(P3[0] - C[:, 0], P3[1] - C[:, 1], P3[2] - C[:, 2])
    is_pl = gid >= ns
    n0 = tuple(np.where(is_pl, Np[:, k], s[k]) for k in range(3))
    return _nrm(*n0)


def _shade(O3, D, t, normal, od):
    """shade_light with the reference's light and both powers on (RayTracing.cu:41-79)."""
    point = tuple(O3[k] + D[k] * t for k in range(3))
    view = _nrm(*(D[k] * f32(-1.0) for k in range(3)))
    ld = (f32(1.0) - point[0], f32(50.0) - point[1], f32(0.0) - point[2])
    dist = np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])
    dist = dist * dist
    divd = f32(1.0) / dist
    ld = _nrm(*ld)
    nn = _nrm(*normal)
    nv = _nrm(*view)
    di = np.clip(_dot(nn, ld), f32(0.0), f32(1.0))
    h = _nrm(ld[0] + nv[0], ld[1] + nv[1], ld[2] + nv[2])
    si = np.clip(_dot(nn, h), f32(0.0), f32(1.0)).astype(np.float64) ** 32
    si = si.astype(np.float32)
    out = []
    for k in range(3):
        diffuse = ((f32(1.0) * di) * f32(2000.0)) * divd
        spec = ((f32(1.0) * si) * f32(3000.0)) * divd
        r = (f32(0.2) * od[k] + diffuse * od[k]) + spec * f32(1.0)
        r = r * f32(255.0)
        out.append(np.where(f32(255.0) < r, f32(255.0), r).astype(np.float32))
    return out


def _pow32(x):
    d = x.astype(np.float64)
    for _ in range(5):
        d = d * d
    return d.astype(np.float32)


def _shade_lights(O3, D, t, normal, od, lights):
    """The colour of rtx_scene_set_lights: res = 0.2f * od; per light, in order, res = (res + diffuse_i * od) + specular_i * 1.0f;
    res * 255.0f; minf(255.0f, res).  One numpy float32 operation per IEEE operation of the kernel."""
    point = tuple(O3[k] + D[k] * t for k in range(3))
    view = _nrm(*(D[k] * f32(-1.0) for k in range(3)))
    nn = _nrm(*normal)
    nv = _nrm(*view)
    res = [f32(0.2) * od[k] for k in range(3)]
    for l in lights:
        ld = tuple(f32(l.pos[k]) - point[k] for k in range(3))
        dist = np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])
        dist = dist * dist
        divd = f32(1.0) / dist
        ld = _nrm(*ld)
        di = np.clip(_dot(nn, ld), f32(0.0), f32(1.0))
        h = _nrm(ld[0] + nv[0], ld[1] + nv[1], ld[2] + nv[2])
        si = _pow32(np.clip(_dot(nn, h), f32(0.0), f32(1.0)))
        for k in range(3):
            diffuse = ((f32(l.diffuse_rgb[k]) * di) * f32(l.diffuse_power)) * divd
            spec = ((f32(l.specular_rgb[k]) * si) * f32(l.specular_power)) * divd
            res[k] = (res[k] + diffuse * od[k]) + spec * f32(1.0)
    out = []
    for k in range(3):
        r = res[k] * f32(255.0)
        out.append(np.where(f32(255.0) < r, f32(255.0), r).astype(np.float32))
    return out


def _scene_k(name, sph, pl, variant):
    """The reflective objects of the mirror tests' scenes: creation indices (spheres first, then planes) -> k."""
    ns, npl = len(sph), len(pl)
    ks = {}
    if variant in ("floor", "floor+quarter"):
        ks[ns] = 0.5
    if variant == "floor+quarter":
        rng = np.random.default_rng(11)
        for i in rng.choice(ns, size=ns // 4, replace=False):
            ks[int(i)] = float(rng.uniform(0.05, 1.0))
    if variant == "room":
        for q in range(npl):
            ks[ns + q] = 0.7
    if variant == "quarter":
        rng = np.random.default_rng(12)
        for i in rng.choice(ns, size=max(1, ns // 4), replace=False):
            ks[int(i)] = float(rng.uniform(0.05, 1.0))
    return ks


# ---------------------------------------------------------------- the geometry of a chain

def host_planes(pl):
    """The planes as the library and the oracle store them: the normal through the safe host normalise (Plane.cu:6-12,
    MyMath.h:117-123).  Unit axis normals come back unchanged."""
    pl = np.array(pl, dtype=np.float32).reshape(-1, 11)
    n = pl[:, 3:6].copy()
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        div = np.where(length < f32(0.000001), f32(0.0), f32(1.0) / length).astype(np.float32)
        pl[:, 3:6] = n * div[:, None]
    return pl


def k_array(ks, n):
    """ks: {creation index: k} or an array of n floats -> float32 array of n."""
    if isinstance(ks, dict):
        kk = np.zeros(n, dtype=np.float32)
        for i, v in ks.items():
            kk[i] = f32(v)
        return kk
    kk = np.asarray(ks, dtype=np.float32)
    assert kk.shape == (n,)
    return kk


def primary_rays(p, pix):
    """RayTracing.cu:9-24 for the pixels `pix` (flat indices): the origin and the direction, three float32 arrays each.  `p` is
    the product's or the oracle's params struct."""
    W, H = int(p.x), int(p.y)
    col, row = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
    m = np.array(p.inv_v, dtype=np.float32).reshape(16)
    fW, fH = f32(W), f32(H)
    vx = (((f32(2.0) * col) - fW) / fW) * f32(p.element1)
    vy = ((fH - row * f32(2.0)) / fH) * f32(p.element2)
    w = [((m[4 * k] * vx + m[4 * k + 1] * vy) + m[4 * k + 2]) + m[4 * k + 3] * f32(0.0) for k in range(3)]
    D = _nrm(*w)
    O3 = tuple(np.full(len(pix), f32(p.cam_pos[k]), dtype=np.float32) for k in range(3))
    return O3, D


def flat_params(p):
    """The params with inv_v as 16 floats in a row, as the product's struct has them (the oracle's is 4 x 4): what the older
    restatements of tests/test_gpu_reflect.py, test_gpu_lights.py and test_gpu_reflect_depth.py index."""
    import types
    return types.SimpleNamespace(inv_v=[float(v) for v in np.array(p.inv_v, dtype=np.float32).reshape(16)], cam_pos=[float(v) for v in p.cam_pos[:3]],
                                 x=int(p.x), y=int(p.y), element1=float(p.element1), element2=float(p.element2), cam_far=float(p.cam_far))


def trace_chain(p, sph, pl, ks, pix, max_depth=4):
    """The geometry of the rule at rtx_scene_set_reflectivity for the pixels `pix` (flat indices), traced to `max_depth` levels
    once; no light enters.  Returns a dict:
      t, gid, sv, normal: the primary hit (gid -1 and t 99999999 without one), shadingValue = normal . (1, 0, 0), the normal;
      hit, vis: gid >= 0; hit and not in column W-1 (which holds the row's terminator and no values);
      levels[j], j = 0 .. max_depth: exists (bool per pixel), idx (the pixels it exists for), and for those pixels the ray (O, D;
        also P, Rd for j >= 1), its hit (t, gid, normal), the hit object's od and k, and for j >= 1 `left`, the object the ray left;
      rays[j - 1]: how many pixels have a level-j ray."""
    sph = np.asarray(sph, dtype=np.float32).reshape(-1, 7)
    pl = host_planes(pl)
    W = int(p.x)
    n = len(pix)
    kk = k_array(ks, len(sph) + len(pl))
    odall = np.concatenate([sph[:, 4:7], pl[:, 6:9]]).astype(np.float32) / f32(255.0)
    with np.errstate(all="ignore"):
        O3, D = primary_rays(p, pix)
        a = _dot(D, D)
        t, gid = _closest(O3, D, sph, pl, a, f32(4.0) * a, f32(1.0) / (f32(2.0) * a))
        hitm = gid >= 0
        P = tuple(O3[k] + D[k] * t for k in range(3))
        normal = _normal(P, sph, pl, gid)
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
            # mirror_ray: N = normalize(normal_j), V = normalize(-D), c = 2 (N . V), R = N c - V, from P = O + D t
            N = _nrm(*cur["normal"])
            V = _nrm(*(cur["D"][q] * f32(-1.0) for q in range(3)))
            c = f32(2.0) * _dot(N, V)
            Pj = tuple(cur["O"][q] + cur["D"][q] * cur["t"] for q in range(3))
            Rd = tuple(N[q] * c - V[q] for q in range(3))
            a2 = _dot(Rd, Rd)
            t2, g2 = _closest(Pj, Rd, sph, pl, a2, f32(4.0) * a2, f32(1.0) / (f32(2.0) * a2), exclude=cur["gid"])
            P2 = tuple(Pj[q] + Rd[q] * t2 for q in range(3))
            n2 = _normal(P2, sph, pl, g2)
        od2 = odall[np.maximum(g2, 0)]
        k2 = np.where(g2 >= 0, kk[np.maximum(g2, 0)], f32(0.0)).astype(np.float32)
        levels.append(dict(exists=ex, idx=idx, O=Pj, D=Rd, P=Pj, Rd=Rd, t=t2, gid=g2, normal=n2, od=[od2[:, q] for q in range(3)],
                           k=k2, left=cur["gid"]))
        go = (g2 >= 0) & (k2 > f32(0.0))
        idx = idx[go]
        cur = dict(O=tuple(x[go] for x in Pj), D=tuple(x[go] for x in Rd), t=t2[go], normal=tuple(x[go] for x in n2), gid=g2[go])
    return dict(p=p, W=W, n=n, pix=pix, sph=sph, pl=pl, t=t, gid=gid, sv=sv, normal=normal, hit=hitm, vis=hitm & (pix % W != W - 1),
                levels=levels, rays=[int(l["exists"].sum()) for l in levels[1:]], max_depth=max_depth, _deep={})


# ---------------------------------------------------------------- the shading of a chain

def _deep_locals(trace, lights):
    """local_j, k_j per level j >= 1 as full-size arrays: every light at full power, black where level j hit nothing."""
    key = tuple(light_tuple(l) for l in lights)
    if key not in trace["_deep"]:
        out = []
        for lev in trace["levels"][1:]:
            loc = [np.zeros(trace["n"], dtype=np.float32) for _ in range(3)]
            kj = np.zeros(trace["n"], dtype=np.float32)
            with np.errstate(all="ignore"):
                sh = _shade_lights(lev["O"], lev["D"], lev["t"], lev["normal"], lev["od"], lights)
            for q in range(3):
                loc[q][lev["idx"]] = np.where(lev["gid"] >= 0, sh[q], f32(0.0))
            kj[lev["idx"]] = lev["k"]
            out.append((loc, kj))
        trace["_deep"] = {key: out}  # (one set at a time: a frame's worth of floats per level)
    return trace["_deep"][key]


def shade_chain(trace, lights, dark0=0):
    """The colour floats of every pixel of `trace` at depths 1 .. max_depth: {depth: [r, g, b]}.  Level 0 is shaded with the lights
    whose bit is set in `dark0` at both powers 0 (what RTX_OPT_SHADOWS does to a light the pixel is shadowed from); every level
    >= 1 with every light at full power: no shadow test there.  Folded from the deepest level inwards:
    C_j = local_j where level j + 1 does not exist, else minf(255, local_j * (1 - k_j) + C_{j+1} * k_j)."""
    L = trace["levels"]
    l0 = [dark(l) if (dark0 >> i) & 1 else l for i, l in enumerate(lights)]
    with np.errstate(all="ignore"):
        local0 = _shade_lights(L[0]["O"], L[0]["D"], L[0]["t"], L[0]["normal"], L[0]["od"], l0)
    deep = _deep_locals(trace, lights)
    local = [local0] + [d[0] for d in deep]
    k = [L[0]["k"]] + [d[1] for d in deep]
    out = {}
    for depth in range(1, trace["max_depth"] + 1):
        C = [x.copy() for x in local[depth]]
        for j in range(depth - 1, -1, -1):
            kj, wj = k[j], f32(1.0) - k[j]
            nxt = L[j + 1]["exists"]
            folded = []
            for q in range(3):
                with np.errstate(all="ignore"):
                    v = local[j][q] * wj + C[q] * kj
                v = np.where(f32(255.0) < v, f32(255.0), v).astype(np.float32)
                folded.append(np.where(nxt, v, local[j][q]))
            C = folded
        out[depth] = C
    return out


def values8(trace, colour):
    """(n, 8) float32: what RTX_RENDER_VALUES holds for the pixels of `trace` that have a hit (t, shadingValue, normal, colour);
    a pixel without one has t = 99999999 and the rest 0, column W-1 all 0."""
    v = np.zeros((trace["n"], 8), dtype=np.float32)
    v[:, 0] = trace["t"]
    v[:, 1] = trace["sv"]
    for q in range(3):
        v[:, 2 + q] = trace["normal"][q]
        v[:, 5 + q] = colour[q]
    v[~trace["hit"], 1:] = 0.0
    v[trace["pix"] % trace["W"] == trace["W"] - 1] = 0.0
    return v


def same_floats(got, want):
    """Bit for bit; where `want` is a NaN `got` must be one too, the payload is free."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))


# ---------------------------------------------------------------- records and pixel words from the eight values

RAMP = " .`^\",:;Il!i><~+_" "-?*][}{1)(|/tfjrx" "nuvczmwXYUJCLqpdb" "khao#%ZO8B$0QM&W@" "@"  # (RayTracing.h:97-115 and one past it)
assert len(RAMP) == 69
_RAMP = np.frombuffer(RAMP.encode(), dtype=np.uint8)
_ansi = None


def _u8_sat(f):
    """(uint8_t)f as the hardware conversion does it: truncate, negatives and NaN to 0, the low byte of the saturated u32."""
    f = np.asarray(f, dtype=np.float32)
    pos = f > f32(0.0)
    big = f >= f32(4294967296.0)
    v = np.where(pos & ~big, f, f32(0.0)).astype(np.float64)
    return np.where(big, 255, np.floor(v).astype(np.int64) & 255).astype(np.uint8)


def _digits3(v):
    """Three digits, NUL (not '0') for absent leading ones."""
    v = v.astype(np.int32)
    out = np.zeros((v.size, 3), dtype=np.uint8)
    out[:, 0] = np.where(v >= 100, v // 100 + 48, 0)
    out[:, 1] = np.where(v >= 10, (v // 10) % 10 + 48, 0)
    out[:, 2] = v % 10 + 48
    return out


def _pixel_parts(values, mode, cam_far):
    """Per pixel: terminator (column W-1: all eight values 0), visible (distance <= far), the colour bytes and the glyph."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, 8)
    term = (v.view(np.uint32) == 0).all(axis=1)
    visible = (v[:, 0] <= f32(cam_far)) & ~term
    with np.errstate(all="ignore"):
        if mode == O.RGB_NORMALS:
            rgb = np.stack([_u8_sat(v[:, 2 + q] * f32(255.0)) for q in range(3)], axis=1)
        else:
            rgb = np.stack([_u8_sat(v[:, 5 + q]) for q in range(3)], axis=1)
        c = np.ceil(v[:, 1] * f32(67.0))
    ramp = np.where(np.isnan(c), 1, np.clip(np.nan_to_num(c, nan=1.0), 1, 68)).astype(np.int64)
    glyph = _RAMP[ramp] if mode in (O.BIT_ASCII, O.RGB_ASCII) else np.full(len(v), 32, dtype=np.uint8)
    if mode in (O.BIT_ASCII, O.BIT_PIXEL):
        global _ansi
        if _ansi is None:
            _ansi = O.ansi256_table()
        rgb = _ansi[(rgb[:, 0].astype(np.int64) << 16) + (rgb[:, 1].astype(np.int64) << 8) + rgb[:, 2]][:, None]
    return term, visible, rgb, glyph


def encode_records(values8_, mode, cam_far):
    """(n, 8) value floats -> (n, S) record bytes of `mode` (S = 12 for the BIT modes, 20 otherwise): trace_and_encode's rule.  A
    pixel that is not visible gets the miss record, a pixel of column W-1 (all values 0) NULs."""
    term, visible, col, glyph = _pixel_parts(values8_, mode, cam_far)
    bit = mode in (O.BIT_ASCII, O.BIT_PIXEL)
    S = 12 if bit else 20
    miss = np.frombuffer(b"\x1b[48;5;\x0016m " if bit else b"\x1b[48;2;\x00\x000;\x00\x000;\x00\x000m ", dtype=np.uint8)
    rec = np.tile(miss, (len(term), 1))
    hit = np.frombuffer(b"\x1b[38;5;000m " if bit else b"\x1b[38;2;000;000;000m ", dtype=np.uint8).copy()
    hit[2] = ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4")
    rec[visible] = hit
    for q in range(col.shape[1]):
        rec[visible, 7 + 4 * q:10 + 4 * q] = _digits3(col[visible, q])
    rec[visible, S - 1] = glyph[visible]
    rec[term] = 0
    return rec


def encode_words(values8_, mode, cam_far):
    """(n, 8) value floats -> n compact pixel words (RTX_RENDER_COMPACT): bytes 0 .. 2 the record's colour values (the xterm index
    in byte 0 for the BIT modes), byte 3 the glyph; 0 for a pixel that is not visible, 0xffffffff for column W-1."""
    term, visible, col, glyph = _pixel_parts(values8_, mode, cam_far)
    w = glyph.astype(np.uint32) << np.uint32(24)
    for q in range(col.shape[1]):
        w |= col[:, q].astype(np.uint32) << np.uint32(8 * q)
    w[~visible] = 0
    w[term] = 0xFFFFFFFF
    return w


# ---------------------------------------------------------------- the scenes and light sets of the chain tests

DEFAULT_SPH = np.array([[0, 10, 20, 7, 255, 1, 1], [5, 10, 20, 6, 1, 255, 1], [10, 10, 40, 10, 1, 1, 255], [5, 10, 20, 3, 225, 210, 20],
                        [-5, 10, 40, 4, 225, 10, 220]], dtype=np.float32)
DEFAULT_PL = np.array([[0, -3, 30, 0, 1, 0, 100, 100, 100, 10, 20]], dtype=np.float32)
PI32 = float(np.float32(np.pi))
CONFIGS = {"C1": (320, 180, 8, 1, 1), "C2": (1920, 1080, 1024, 1, 2), "C3": (3840, 2160, 4096, 6, 3)}  # 

COLOURS = [(1.0, 0.5, 0.25), (0.25, 1.0, 0.5), (0.5, 0.25, 1.0), (1.0, 1.0, 0.5), (0.75, 0.5, 1.0), (0.5, 1.0, 1.0), (1.0, 0.75, 0.75), (0.3, 0.6, 0.9)]


def light_set(n, positions=None, zero=None, scale=1.0):
    """tests/test_gpu_lights.py::_light_set as plain tuples: n lights with distinct colours and powers around the scene (or at
    `positions`); light `zero` has both powers 0."""
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / 8.0
        pos = positions[i] if positions is not None else (1.0 + 45.0 * np.sin(a), 50.0 + 4.0 * i, 20.0 - 45.0 * np.cos(a))
        dp, sp = scale * (500.0 + 170.0 * i), scale * (1400.0 - 150.0 * i)
        if zero == i:
            dp = sp = 0.0
        out.append(Light(tuple(float(v) for v in pos), COLOURS[i], dp, COLOURS[(i + 3) % 8], sp))
    return out


def config_case(name):
    """(oracle params, spheres, planes) of a BASELINE config, through the numpy scene generator."""
    import util as U
    W, H, ns, npl, seed = CONFIGS[name]
    p = O.camera_params(W, H)
    sph, pl = U.numpy_synth_scene(seed, ns, npl, p.element1, p.element2)
    return p, sph, pl


def chain_scene(name):
    """The scenes of the depth x lights tests: (oracle params, spheres, planes, ks, pixels).  The first two are whole frames."""
    if name == "default":
        return O.camera_params(320, 180), DEFAULT_SPH, DEFAULT_PL, {0: 0.3, 2: 0.8, 4: 1.0, 5: 0.6}, np.arange(320 * 180)
    if name in ("mirror_floor", "mirror_floor_shadows"):
        # (tests/test_gpu_reflect_depth.py::_mirror_floor_scene: a floor under four spheres, the camera looking down)
        p = O.camera_params(320, 180, pos=(0.0, 12.0, 0.0), rot=(0.3, PI32, 0.0))
        sph = np.array([[-7, 4, 30, 4, 230, 40, 40], [0, 5, 36, 5, 40, 230, 40], [8, 4, 30, 4, 40, 40, 230], [2, 3, 22, 2.5, 230, 230, 40]],
                       dtype=np.float32)
        pl = np.array([[0, -1, 30, 0, 1, 0, 120, 120, 120, 80, 80]], dtype=np.float32)
        # (under shadows the floor keeps 0.4 of its own colour: with k = 1 a dark light at level 0 would not show on it)
        return p, sph, pl, {0: .5, 1: .5, 2: .5, 3: .5, 4: 1.0 if name == "mirror_floor" else 0.6}, np.arange(320 * 180)
    if name == "directed":
        # (tests/test_gpu_shadows.py::directed_scene and directed_params, the plane and the sphere reflective)
        p = O.camera_params(320, 180, pos=(0.0, 10.0, 0.0), rot=(0.4, PI32, 0.0))
        sph = np.array([[0.0, 8.0, 40.0, 10.0, 200.0, 40.0, 40.0]], dtype=np.float32)
        pl = np.array([[0.0, -3.0, 30.0, 0.0, 1.0, 0.0, 120.0, 120.0, 120.0, 80.0, 80.0]], dtype=np.float32)
        return p, sph, pl, {0: 0.5, 1: 0.6}, np.arange(320 * 180)
    cfg, variant = {"C2": ("C2", "floor+quarter"), "C3": ("C3", "room")}[name]
    p, sph, pl = config_case(cfg)
    pix = np.sort(np.random.default_rng(3).choice(int(p.x) * int(p.y), size=40000, replace=False))
    return p, sph, pl, _scene_k(cfg, sph, pl, variant), pix


CUSTOM_LIGHT = Light((5.0, 40.0, 10.0), (1.0, 0.5, 0.25), 900.0, (0.2, 1.0, 0.4), 2100.0)
# the light sets of the depth x lights tests: name -> (lights, which one is dark)
LIGHT_SETS = {"1custom": (1, None), "2": (2, None), "3dark1": (3, 1), "8": (8, None)}
# powers scaled as _light_set(scale=...) does until the colour stays below the 255 clamp on >= 5 % of the pixels with a level-2
# ray (tests/test_host_restate.py asserts it for every pair): scene -> light set -> scale
LIGHT_SCALES = {"default": {"1custom": 1.0, "2": 0.6, "3dark1": 0.6, "8": 0.25},
                "mirror_floor": {"1custom": 1.0, "2": 0.6, "3dark1": 0.6, "8": 0.25},
                "C2": {"1custom": 1.0, "2": 0.6, "3dark1": 0.6, "8": 0.25},
                "C3": {"1custom": 1.0, "2": 0.6, "3dark1": 0.6, "8": 0.25}}


def chain_lights(scene, which):
    n, zero = LIGHT_SETS[which]
    s = LIGHT_SCALES[scene][which]
    if which == "1custom":
        return [CUSTOM_LIGHT._replace(diffuse_power=CUSTOM_LIGHT.diffuse_power * s, specular_power=CUSTOM_LIGHT.specular_power * s)]
    return light_set(n, zero=zero, scale=s)


# the shadow tests: scene -> the positions its 1, 2 and 3 lights are the first of (placed so that the conditions of
# tests/test_host_restate.py::test_shadow_inputs hold)
SHADOW_POSITIONS = {"mirror_floor_shadows": [(0.0, 40.0, 50.0), (-30.0, 30.0, 25.0), (30.0, 30.0, 25.0)],
                    "directed": [(0.0, 50.0, 40.0), (-30.0, 40.0, 20.0), (30.0, 40.0, 20.0)]}
SHADOW_SCALE = {"mirror_floor_shadows": 0.6, "directed": 0.6}


def shadow_lights(scene, n):
    pos = SHADOW_POSITIONS[scene]
    if n == 1:
        return [CUSTOM_LIGHT._replace(pos=pos[0])]
    return light_set(n, positions=pos[:n], scale=SHADOW_SCALE[scene])


def record_lights(n):
    """The lights of the record tests on C1 and C2: one custom light, or three around the configs' spheres."""
    if n == 1:
        return [CUSTOM_LIGHT]
    return light_set(n, positions=[(5.0, 40.0, 10.0), (-20.0, 80.0, 10.0), (30.0, 50.0, 60.0)], scale=1.5)


FUZZ_SEEDS = list(range(12))  # (the fixed seeds of the fuzzed GPU test: tests/fuzz_cases.py::chain_case)
