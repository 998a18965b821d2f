"""The cases that pin the oracle and the kernels to the host build of the reference (tests/ref_host.py): one construction
shared by tests/test_ref_host.py (live binary against the oracle), tests/golden/make_ref_golden.py (records a subset into
tests/golden/ref_cases.npz), tests/test_ref_fixtures.py (oracle and live binary against the recording) and
tests/test_gpu_ref_parity.py (the kernels against the recording and the live binary).

A case is a dict: name, objs (ref_host.OBJECT_DTYPE, creation order), w, h, mode, params (f32[22], raw layout), dts.
An expectation (`expect`) is what the reference gave for it, per step: states (y, mover per object), and the frame and the
minimised stream either whole (`frames`, `streams`) or, for frames over STORE_PIXELS pixels in the recording, as FNV-1a
hashes (`frame_hashes`, `stream_hashes`).  Recorded frames come from ref_driver_pinpow (RayTracing.cu:73's pow as five
squarings in double), because the C library's powf may differ from machine to machine and the kernels use the pinned one.
"""
import copy
import os

import numpy as np

import fuzz_cases as FZ
import oracle as O
import ref_host as RH
import util as U

MODES = (O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS)
FIXTURE = os.path.join(U.GOLDEN_DIR, "ref_cases.npz")
STORE_PIXELS = 200          # frames of at most this many pixels are recorded whole, larger ones as hashes
FUZZ_SEEDS = 200            # tests/test_ref_host.py
FUZZ_FIXTURE_SEEDS = 24     # recorded: make_ref_golden.py
PHYSICS_DTS = (0.016, 0.25, 1.7, 0.0333333, 3.0, 0.5, 0.016)   # test_update_objects_matches_oracle_over_many_steps


def case(name, objs, w, h, mode, params, dts=(0.0,)):
    return dict(name=name, objs=np.ascontiguousarray(objs, dtype=RH.OBJECT_DTYPE), w=int(w), h=int(h), mode=int(mode),
                params=np.asarray(params, dtype=np.float32).copy(), dts=tuple(float(d) for d in dts))


# ---------------------------------------------------------------------------------------------------- fuzz

def fuzz_case(seed, max_spheres=700, max_w=120, max_h=41):
    """fuzz_cases.scene under a general matrix, fov x{0.2, 0.5, 1, 2}, mode seed % 5, 1-3 Update calls at dt in
    {0.016, 0.25, 1.7}, random movers and speeds, spheres and planes interleaved in a random creation order."""
    g = np.random.default_rng(7000 + seed)
    w, h = int(g.integers(8, max_w + 1)), int(g.integers(3, max_h + 1))
    pos = [float(v) for v in g.uniform(-30, 30, 3)]
    p = O.camera_params(w, h, pos, O.DEFAULT_ROT)
    M = FZ.general_matrix(g)
    fov = float(g.choice([0.2, 0.5, 1.0, 2.0]))
    p.element1 = float(p.element1) * fov
    p.element2 = float(p.element2) * fov
    for i in range(3):
        for j in range(3):
            p.inv_v[i][j] = float(M[i, j])
    M = np.array([[p.inv_v[i][j] for j in range(3)] for i in range(3)], dtype=np.float64)   # as stored: float32
    kind = int(copy.deepcopy(g).integers(0, 5))     # what scene() is about to draw first
    sph, pl = FZ.scene(g, p, M, pos, w, h, max_spheres=max_spheres)
    movers = g.choice([-1, 1, 1, 3, -2], len(sph))
    speeds = g.uniform(0.5, 4.0, len(sph)).astype(np.float32)
    order = g.permutation(len(sph) + len(pl))
    dts = [float(g.choice([0.016, 0.25, 1.7])) for _ in range(int(g.integers(1, 4)))]
    c = case("fuzz%d" % seed, RH.from_arrays(sph, pl, order, movers, speeds), w, h, seed % 5, RH.raw_of_oracle_params(p), dts)
    c["kind"] = kind
    return c


def fuzz_fixture_case(i):
    """The recorded share: small frames (33 x 17 at most) and at most 30 spheres, so that the inputs fit the fixture."""
    c = fuzz_case(1000 + i, max_spheres=30, max_w=33, max_h=17)
    c["name"] = "fuzzfix%d" % i
    return c


# ---------------------------------------------------------------------------------------------------- directed edges

IDENTITY = np.eye(4, dtype=np.float32)
DW, DH = 8, 4     # pixel (row 2, column 4) of an 8 x 4 frame looks along (0, 0, 1) exactly: 2*4 - 8 = 0 and 4 - 2*2 = 0
CENTRE = (2, 4)
F32 = np.float32


def _up(x, n=1):
    x = F32(x)
    for _ in range(n):
        x = np.nextafter(x, F32(np.inf), dtype=np.float32)
    return x


def _down(x, n=1):
    x = F32(x)
    for _ in range(n):
        x = np.nextafter(x, F32(-np.inf), dtype=np.float32)
    return x


def _axis_params(far=250.0, e1=0.5, e2=0.5, cam=(0.0, 0.0, 0.0)):
    return RH.raw_params(IDENTITY, cam, e1, e2, far)


RED, GREEN, BLUE = (255.0, 1.0, 1.0), (1.0, 255.0, 1.0), (1.0, 1.0, 255.0)


def directed_geometries():
    """(name, objs, w, h, params): one small scene per edge; every one is run in all five modes.  The arithmetic in the comments
    is exact in float32 for the pixel CENTRE, whose ray is (0, 0, 1) from the origin: a = 1, fourA = 4, divTwoA = 0.5."""
    S, P, cat = RH.sphere, RH.plane, np.concatenate
    out = []

    def add(name, objs, params=None, w=DW, h=DH):
        out.append((name, objs, w, h, _axis_params() if params is None else params))

    # RayTracing.cu:123, `distance < closest`: of two hits at the same t the one created first stays
    a, b = S(2.0, (0, 0, 10), RED), S(2.0, (0, 0, 10), GREEN)
    add("coincident_spheres_ab", cat([a, b]))
    add("coincident_spheres_ba", cat([b, a]))
    # sphere (0,0,10) r 2: b = -20, c = 96, discriminant 16, t = (20 - 4) * 0.5 = 8; plane z = 8 facing the camera: t = -8 / -1 = 8
    s, p = S(2.0, (0, 0, 10), RED), P((0, 0, 8), (0, 0, -1), BLUE, 1.0, 1.0)
    add("sphere_plane_equal_t_sp", cat([s, p]))
    add("sphere_plane_equal_t_ps", cat([p, s]))
    # Sphere.cu:39-45.  centre (0.5, 0, 2^-6), r 0.5: dot(oc, oc) = 0.25 + 2^-12, c = 2^-12, b = -2^-5, b*b = 4c = 2^-10:
    # discriminant exactly 0, t1 = t2 = 2^-6, a hit.  r one ulp down: c = 2^-12 + 2^-25, discriminant -2^-23, a miss.
    # r one ulp up: c = 2^-12 - 2^-24, discriminant +2^-22, a hit.
    z = 2.0 ** -6
    add("tangent_discriminant_zero", S(0.5, (0.5, 0, z), RED))
    add("tangent_discriminant_minus", S(_down(0.5), (0.5, 0, z), RED))
    add("tangent_discriminant_plus", S(_up(0.5), (0.5, 0, z), RED))
    # Sphere.cu:57, `t1 < 0 || t2 < 0`: from inside one root is negative and the sphere is not seen at all
    add("camera_inside_sphere", cat([S(5.0, (0, 0, 1), RED), S(1.0, (0, 0, 20), GREEN)]))
    # on the surface, sphere ahead: c = 0, b = -10, roots 10 and 0; 0 is not < 0, so it is a hit at t = 0
    add("camera_on_surface_ahead", S(5.0, (0, 0, 5), RED))
    # on the surface, sphere behind: roots 0 and -10, a miss
    add("camera_on_surface_behind", cat([S(5.0, (0, 0, -5), RED), S(1.0, (0, 0, 20), GREEN)]))
    # RayTracing.cu:207 `distance <= camFarDist` and :30 `distance > farPlane`: the hit at t = 8 exactly
    for nm, far in (("far_equals_hit", F32(8.0)), ("far_ulp_below_hit", _down(8.0)), ("far_ulp_above_hit", _up(8.0))):
        add(nm, S(2.0, (0, 0, 10), RED), _axis_params(far=far))
    # radius 0: discriminant 0 on the axis, the normal is 0 * inf (NaN -> uint8_t)
    add("radius_zero", cat([S(0.0, (0, 0, 10), RED), P((0, -1, 10), (0, 1, 0), BLUE, 40.0, 40.0)]))
    # Plane.cu:47: row 2 runs along the floor (dot = 0), rows below hit it, rows above see its back
    add("plane_parallel_to_ray", P((0, -1, 10), (0, 1, 0), BLUE, 40.0, 40.0))
    # Plane.cu:64-65: hitPoint.x = 0 against planePos.x + halfWidth = 0 exactly (`>=`: a miss), one ulp inside (a hit),
    # and against planePos.x - halfWidth = 0 (`<=`: a miss)
    add("plane_bound_exact_high", P((-1, 0, 8), (0, 0, -1), BLUE, 2.0, 4.0))
    add("plane_bound_inside_high", P((_up(-1.0), 0, 8), (0, 0, -1), BLUE, 2.0, 4.0))
    add("plane_bound_exact_low", P((1, 0, 8), (0, 0, -1), BLUE, 2.0, 4.0))
    add("plane_bound_inside_low", P((_down(1.0), 0, 8), (0, 0, -1), BLUE, 2.0, 4.0))
    add("plane_zero_height", P((0, 0, 8), (0, 0, -1), BLUE, 40.0, 0.0))
    add("plane_from_behind", cat([P((0, 0, 8), (0, 0, 1), BLUE, 40.0, 40.0), S(1.0, (0, 0, 20), GREEN)]))
    add("colour_zero", S(2.0, (0, 0, 10), (0.0, 0.0, 0.0)))
    add("colour_255", S(2.0, (0, 0, 10), (255.0, 255.0, 255.0)))
    # the light is at (1, 50, 0) (RayTracing.cu:146): the top of a white sphere at y = 10 (Sphere::Update keeps y within +-10),
    # seen from straight above, gets 2000 / 37^2 > 1 of diffuse light and saturates Min(255, shading)
    down = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
    add("colour_saturated", S(3.0, (1, 10, 0), (255.0, 255.0, 255.0)), RH.raw_params(down, (1, 20, 0), 0.5, 0.5, 250.0))
    # RayTracing.cu:187: the last column is never traced; W = 1 traces nothing at all
    dflt = RH.DEFAULT_SCENE
    add("width_1", dflt, RH.raw_of_oracle_params(O.camera_params(1, 5)), 1, 5)
    add("width_2", dflt, RH.raw_of_oracle_params(O.camera_params(2, 5)), 2, 5)
    add("height_1", dflt, RH.raw_of_oracle_params(O.camera_params(9, 1)), 9, 1)
    return out


def directed_cases():
    return [case("%s/%s" % (name, O.MODE_NAMES[m]), objs, w, h, m, params) for name, objs, w, h, params in directed_geometries()
            for m in MODES]


def big_scene_case(mode=O.RGB_ASCII):
    """1024 objects, the most RayTracingManager.cu:89-98's launch shape allows: 1000 spheres and 24 planes in
    a random creation order, two Update calls.  Sphere centres are whole numbers, the other lengths multiples of 1/8, colours multiples of 8 and both dt powers of two, so that the
    recorded inputs and sphere states compress."""
    g = np.random.default_rng(1024)
    w, h = 40, 20
    p = O.camera_params(w, h)
    n = 1000
    d = np.stack([g.uniform(-1, 1, n) * p.element1, g.uniform(-1, 1, n) * p.element2, np.ones(n)], axis=1)
    d[:, 0] *= -1.0      # (the default pose looks along +z with x mirrored)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sph = np.zeros((n, 7), dtype=np.float32)
    sph[:, 0:3] = np.round(d * g.uniform(20, 240, n)[:, None])
    sph[:, 3] = np.ceil(g.uniform(0.2, 6.0, n) * 8) / 8
    sph[:, 4:7] = np.floor(g.uniform(0, 32, (n, 3))) * 8
    pl = np.zeros((24, 11), dtype=np.float32)
    for i in range(24):
        nrm = g.normal(0, 1, 3)
        pl[i] = [g.uniform(-20, 20), g.uniform(-20, 20), g.uniform(10, 200), nrm[0], nrm[1], nrm[2]] + \
                list(np.floor(g.uniform(0, 256, 3))) + [g.uniform(1, 100), g.uniform(1, 100)]
    pl = np.round(pl * 8) / 8
    objs = RH.from_arrays(sph, pl, g.permutation(n + 24), g.choice([-1, 1, 3, -2], n), g.integers(2, 17, n) / 4.0)
    return case("objects_1024/%s" % O.MODE_NAMES[mode], objs, w, h, mode, RH.raw_of_oracle_params(p), (0.25, 2.0))


# ---------------------------------------------------------------------------------------------------- physics

def physics_cases():
    """Sphere::Update (Sphere.cu:15-23) alone, on a 2 x 1 frame: y and mover after every step."""
    g = np.random.default_rng(77)
    params = _axis_params()
    out = []
    n = 40
    ys = np.concatenate([g.uniform(-10, 10, n - 8), [-10.0, 10.0, -25.0, 17.5, 10.000001, -10.000001, 0.0, 9.999999]])
    sph = np.zeros((n, 7), dtype=np.float32)
    sph[:, 0], sph[:, 1], sph[:, 2], sph[:, 3] = g.uniform(-5, 5, n), ys, 500.0, 1.0     # (spheres created outside [-10, 10] too)
    speeds = (g.integers(100, 400, n) / 100.0).astype(np.float32)    # Sphere.cu:11-12: (rand() % 300 + 100) / 100
    for movers, nm in ((np.full(n, -1), "movers_default"), (g.choice([-2, -1, 0, 1, 3], n), "movers_mixed")):
        out.append(case("physics/%s" % nm, RH.from_arrays(sph, np.zeros((0, 11)), None, movers, speeds), 2, 1, O.BIT_ASCII, params, PHYSICS_DTS))
        out.append(case("physics/%s_dt0" % nm, RH.from_arrays(sph, np.zeros((0, 11)), None, movers, speeds), 2, 1, O.BIT_ASCII, params, (0.0, 0.25, 0.0)))
    # a dt that lands y exactly on +-10: 10 is not > 10, so no clamp and no flip; the step after overshoots and flips
    s = np.zeros((4, 7), dtype=np.float32)
    s[:, 1], s[:, 2], s[:, 3] = [9.0, -9.0, 8.0, -7.0], 500.0, 1.0
    objs = RH.from_arrays(s, np.zeros((0, 11)), None, [1, -1, 1, -1], [2.0, 2.0, 4.0, 1.5])
    out.append(case("physics/lands_on_bound", objs, 2, 1, O.BIT_ASCII, params, (0.5, 0.5, 0.5, 0.5, 1.0, 0.125, 4.0)))
    return out


# ---------------------------------------------------------------------------------------------------- Minimize alone

MINIMIZE_WIDTHS = (1, 2, 3, 64, 257)


def _nine_bytes_frame(S):
    """Pairs of neighbouring records that differ in exactly one compared colour byte, one pair per byte
    (RayTracingManager.cu:199-201 and :269-271), then a pair that differs only in the glyph."""
    offs = (7, 8, 9) if S == 12 else (7, 8, 9, 11, 12, 13, 15, 16, 17)
    w = 2 * len(offs) + 3
    base = U.words_to_records(np.array([0x41112233], dtype=np.uint32), S, ord("3")).copy()
    recs = []
    for o in offs:
        other = base.copy()
        other[o] = base[o] + 1 if base[o] else ord("1")
        recs += [base, other]
    glyph = base.copy()
    glyph[S - 1] = ord("B")
    recs += [base, glyph, np.zeros(S, dtype=np.uint8)]
    return np.concatenate(recs), w, 1


def minimize_frames(full=True):
    """(name, mode, w, h, 20*w*h host array): frames made up from util.random_words in the 12- and the 20-byte form, runs from 0
    to 0.99, holes from 0 to 0.999 (whole empty rows among them), and the nine-bytes frames.  full=False: the recorded dozen."""
    out = []
    g = np.random.default_rng(4242)
    combos = [(w, runs, holes) for w in MINIMIZE_WIDTHS for runs in (0.0, 0.5, 0.99) for holes in (0.0, 0.3, 0.999)]
    if not full:
        combos = [(1, 0.5, 0.0), (2, 0.0, 0.3), (3, 0.99, 0.0), (3, 0.5, 0.999), (64, 0.5, 0.3)]
    for w, runs, holes in combos:
        h = 5 if w < 64 else 3
        for mode in (O.BIT_ASCII, O.RGB_PIXEL):
            S = 20 if mode >= O.RGB_ASCII else 12
            words = U.random_words(g, w, h, runs, holes).reshape(h, w)
            if h > 2:
                words[1, :] = 0xFFFFFFFF         # a whole empty row
            buf = np.zeros(20 * w * h, dtype=np.uint8)
            buf[:S * w * h] = U.words_to_records(words.reshape(-1), S, ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4"))
            out.append(("minimize/w%d_runs%g_holes%g_%s" % (w, runs, holes, O.MODE_NAMES[mode]), mode, w, h, buf, words.reshape(-1).copy()))
    for mode in (O.BIT_ASCII, O.RGB_ASCII):
        S = 20 if mode >= O.RGB_ASCII else 12
        recs, w, h = _nine_bytes_frame(S)
        buf = np.zeros(20 * w * h, dtype=np.uint8)
        buf[:recs.size] = recs
        out.append(("minimize/every_compared_byte_%s" % O.MODE_NAMES[mode], mode, w, h, buf, U.records_to_words(buf, w, h, S)))
    return out


# ---------------------------------------------------------------------------------------------------- camera

CAMERA_SIZE = (400, 150)


def camera_poses():
    """50 (pos, rot): the default pose first, then random ones; pitch within Camera3D::AddRot's clamp (Camera3D.cpp:178-186)."""
    g = np.random.default_rng(50)
    poses = [((0.0, 0.0, 0.0), tuple(F32(v) for v in O.DEFAULT_ROT))]
    for _ in range(49):
        pos = tuple(F32(v) for v in g.uniform(-60, 60, 3))
        rot = (F32(g.uniform(-np.pi / 2, np.pi / 2)), F32(g.uniform(-2 * np.pi, 2 * np.pi)), F32(g.uniform(-1, 1)))
        poses.append((pos, rot))
    return poses


# ---------------------------------------------------------------------------------------------------- expectations

def oracle_steps(c, flags):
    """What the oracle gives for the case: per step (states, frame, pixel records)."""
    sc = RH.oracle_scene(c["objs"])
    p = RH.oracle_params_of_raw(c["params"], c["w"], c["h"])
    out = []
    for dt in c["dts"]:
        O.lib().orc_update_objects(sc.ptrs(), sc.count, dt)
        st = np.zeros(sc.count, dtype=RH.STATE_DTYPE)
        for i, o in enumerate(sc.objects()):
            st[i] = (o.center.y, o.mover if o.type == O.SPHERE else 0)
        frame, px = O.render(p, sc, c["mode"], flags=flags, want_pixels=True)
        out.append((st, frame, px))
    return out


def ramp68_mask(c, px):
    """Bytes of the frame the host build takes from past the end of ASCII[] (ramp index 68): the glyph of
    such a pixel in the two ASCII modes.  Returns a boolean mask over the 20*W*H frame and the number of pixels."""
    w, h = c["w"], c["h"]
    mask = np.zeros(20 * w * h, dtype=bool)
    if c["mode"] not in (O.BIT_ASCII, O.RGB_ASCII):
        return mask, 0
    S = 20 if c["mode"] >= O.RGB_ASCII else 12
    hit = (px["ramp_index"] == 68)
    hit[:, -1] = False
    idx = np.flatnonzero(hit.reshape(-1))
    mask[idx * S + S - 1] = True
    return mask, idx.size


def run_reference(c, binary):
    return RH.update(c["objs"], c["w"], c["h"], c["mode"], c["params"], c["dts"], binary=binary)


def expect_from_live(c):
    r = run_reference(c, RH.PINPOW)
    return dict(states=r.states, frames=r.frames, streams=r.streams, source="live ref_driver_pinpow")


def hash_of(buf):
    return int(O.fnv1a64(buf), 16)


def frame_matches(expect, k, frame):
    if "frames" in expect:
        return np.array_equal(frame, expect["frames"][k])
    return hash_of(frame) == int(expect["frame_hashes"][k])


def stream_matches(expect, k, stream):
    if "streams" in expect:
        return np.array_equal(stream, expect["streams"][k])
    return hash_of(stream) == int(expect["stream_hashes"][k])


# ---------------------------------------------------------------------------------------------------- the recording

def fixture_update_cases():
    """The Update cases that are recorded: the directed edges, the 1024-object scene, the recorded fuzz share, the physics."""
    return directed_cases() + [big_scene_case()] + [fuzz_fixture_case(i) for i in range(FUZZ_FIXTURE_SEEDS)] + physics_cases()


def load_fixture():
    """-> (update cases with c["expect"], minimize frames with the reference's stream, camera (poses, params))."""
    z = np.load(FIXTURE)
    objs, dts, states = z["objs"].view(RH.OBJECT_DTYPE), z["dts"], z["states"].view(RH.STATE_DTYPE)
    frames, streams, stream_lens, hashes = z["frames"], z["streams"], z["stream_lens"], z["hashes"]
    at = dict(obj=0, dt=0, state=0, frame=0, stream=0, step=0, hash=0)

    def take(arr, key, n):
        at[key] += n
        return arr[at[key] - n:at[key]]

    cases = []
    for name, (w, h, mode, nobj, n, stored), params in zip(z["names"], z["meta"], z["params"]):
        c = case(str(name), take(objs, "obj", nobj), w, h, mode, params, take(dts, "dt", n))
        e = dict(states=list(take(states, "state", n * nobj).reshape(n, nobj)), source="tests/golden/ref_cases.npz")
        if stored:
            e["frames"] = list(take(frames, "frame", n * 20 * w * h).reshape(n, -1))
            e["streams"] = [take(streams, "stream", int(ln)) for ln in take(stream_lens, "step", n)]
        else:
            hh = take(hashes, "hash", n)
            e["frame_hashes"], e["stream_hashes"] = hh[:, 0], hh[:, 1]
        c["expect"] = e
        cases.append(c)
    mins = []
    at.update(word=0, mstream=0)
    for name, (mode, w, h), ln in zip(z["min_names"], z["min_meta"], z["min_stream_lens"]):
        words = take(z["min_words"], "word", w * h)
        S = 20 if mode >= O.RGB_ASCII else 12
        buf = np.zeros(20 * w * h, dtype=np.uint8)
        buf[:S * w * h] = U.words_to_records(words, S, ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4"))
        mins.append((str(name), int(mode), int(w), int(h), buf, words, take(z["min_streams"], "mstream", int(ln))))
    return cases, mins, (z["cam_poses"], z["cam_params"])
