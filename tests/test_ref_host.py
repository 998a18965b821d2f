"""The oracle against the reference's own code: oracle/_ref/ref_driver is the reference's sources (MyMath, Object3D, Sphere,
Plane, RayTracing, RayTracingManager, Scene3D, Camera3D), unedited, compiled for the host with IEEE arithmetic
(oracle/Makefile, oracle/ref_host/).  Every comparison here is bit for bit.  The platform choices of SURVEY App. E remain:
`pow` (stock binary against POW_LIBM, ref_driver_pinpow against the pinned routine), negative floats to uint8_t (the host
build wraps: NORMALS_WRAP), ramp index 68 (the host build reads past ASCII[]: those glyph bytes are left out and counted).

If the binaries are absent and so is the reference's directory, the tests skip and say so; the recording in
tests/golden/ref_cases.npz (tests/test_ref_fixtures.py) then still holds the oracle.  A reference without binaries is a
broken build and fails.
"""
import numpy as np
import pytest

import oracle as O
import ref_cases as RC
import ref_host as RH
import util as U
from test_oracle_pins import SURVEY_8C


@pytest.fixture(scope="module", autouse=True)
def binaries():
    ok, why = RH.availability()
    if ok:
        return
    if RH.have_reference():
        pytest.fail("the reference is at %s but its host build is missing (%s): run make -C oracle" % (RH.ref_dir(), why))
    pytest.skip(why)


def S_of(mode):
    return 20 if mode >= O.RGB_ASCII else 12


def check_case(c, stats=None):
    """One Update case: stock binary == oracle(POW_LIBM | NORMALS_WRAP), pinpow binary == oracle(NORMALS_WRAP), the reference's
    stream == O.minimize of the reference's frame, sphere state after every step.  Returns the oracle's steps (pinned pow)."""
    w, h, mode = c["w"], c["h"], c["mode"]
    stock = RC.run_reference(c, RH.STOCK)
    pin = RC.run_reference(c, RH.PINPOW)
    assert RH.same_bits(stock.params, c["params"]) and RH.same_bits(pin.params, c["params"]), c["name"]
    libm = RC.oracle_steps(c, O.POW_LIBM | O.NORMALS_WRAP)
    pinned = RC.oracle_steps(c, O.NORMALS_WRAP)
    for k in range(len(c["dts"])):
        for ref, orc, what in ((stock, libm, "ref_driver / POW_LIBM"), (pin, pinned, "ref_driver_pinpow / pinned pow")):
            st, frame, px = orc[k]
            assert np.array_equal(ref.states[k]["y"].view(np.uint32), st["y"].view(np.uint32)) and \
                np.array_equal(ref.states[k]["mover"], st["mover"]), "%s step %d (%s): sphere y / mover differ" % (c["name"], k, what)
            mask, n68 = RC.ramp68_mask(c, px)
            same = (ref.frames[k] == frame) | mask
            assert same.all(), "%s step %d (%s): %s (%d pixels left out for ramp index 68)" % (
                c["name"], k, what, U.first_diff(np.where(mask, frame, ref.frames[k]), frame, S_of(mode), w), n68)
            assert np.array_equal(O.minimize(mode, ref.frames[k], w, h), ref.streams[k]), \
                "%s step %d (%s): the reference's minimised stream is not O.minimize of its frame" % (c["name"], k, what)
            if stats is not None and ref is pin:
                traced = np.ones((h, w), dtype=bool)
                traced[:, -1] = False
                stats["pixels"] += int(traced.sum())
                stats["hits"] += int(((px["distance"] <= c["params"][21]) & traced).sum())
                stats["excluded"] += n68
    return pinned


# ---------------------------------------------------------------------------------------------------- ansi256

def test_ansi256_all_inputs():
    got = RH.ansi256_table()
    want = O.ansi256_table()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of 2^24 differ; first 0x%06x: reference %d oracle %d" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------------------------------- default scene

@pytest.mark.parametrize("res", sorted(SURVEY_8C))
@pytest.mark.parametrize("mode", RC.MODES)
def test_default_scene(res, mode):
    """Scene3D::Init and Camera3D's start pose through RayTracingManager::Update: the reference's own frame hashes to SURVEY
    8(c)'s value, and its minimised stream -- the first reference output for Minimize -- is O.minimize of that frame."""
    w, h = res
    for binary in (RH.STOCK, RH.PINPOW):
        r = RH.update(RH.DEFAULT_SCENE, w, h, mode, ((0.0, 0.0, 0.0), O.DEFAULT_ROT), dts=(0.0,), camera=True, init_scene=True, binary=binary)
        assert O.fnv1a64(r.frames[0], O.FNV_OFFSET_SURVEY) == SURVEY_8C[res][mode]
        assert np.array_equal(O.minimize(mode, r.frames[0], w, h), r.streams[0])
        assert RH.same_bits(r.params, RH.raw_of_oracle_params(O.camera_params(w, h)))


# ---------------------------------------------------------------------------------------------------- fuzz

def test_fuzz_scenes():
    stats = dict(pixels=0, hits=0, excluded=0)
    modes, kinds = set(), set()
    for seed in range(RC.FUZZ_SEEDS):
        c = RC.fuzz_case(seed)
        assert len(c["objs"]) <= 720 and c["w"] <= 120 and c["h"] <= 41 and 1 <= len(c["dts"]) <= 3
        check_case(c, stats)
        modes.add(c["mode"])
        kinds.add(c["kind"])
    share = stats["hits"] / stats["pixels"]
    report = "%d seeds, %d pixels, %.1f%% with a hit, %d excluded for ramp index 68" % (RC.FUZZ_SEEDS, stats["pixels"], 100 * share, stats["excluded"])
    print(report)
    assert share >= 0.25, report
    assert modes == set(RC.MODES) and kinds == set(range(5)), report
    assert stats["excluded"] <= 0.001 * stats["pixels"], report


# ---------------------------------------------------------------------------------------------------- directed edges

_DIRECTED = RC.directed_cases()


@pytest.mark.parametrize("c", _DIRECTED, ids=[c["name"] for c in _DIRECTED])
def test_directed_edge(c):
    steps = check_case(c)
    # the case does what its name says (on the oracle's records, which the lines above tied to the reference)
    px = steps[0][2]
    name = c["name"].split("/")[0]
    centre = px[RC.CENTRE] if (c["w"], c["h"]) == (RC.DW, RC.DH) else None
    far = c["params"][21]
    sees = {"coincident_spheres_ab": RC.RED, "coincident_spheres_ba": RC.GREEN}
    if name in ("tangent_discriminant_zero", "tangent_discriminant_plus", "camera_on_surface_ahead", "far_equals_hit", "far_ulp_above_hit",
                "plane_bound_inside_high", "plane_bound_inside_low", "radius_zero"):
        assert centre["hit"] and centre["distance"] <= far
    if name in ("tangent_discriminant_minus", "plane_bound_exact_high", "plane_bound_exact_low", "plane_zero_height"):
        assert not centre["hit"]
    if name in ("camera_inside_sphere", "camera_on_surface_behind", "plane_from_behind"):
        assert centre["hit"] and centre["distance"] == np.float32(19.0)     # only the small sphere behind is seen
    if name == "far_ulp_below_hit":
        assert centre["hit"] and centre["distance"] == np.float32(8.0) and not centre["distance"] <= far
    if name == "far_equals_hit":
        assert centre["distance"] == far and centre["ramp_index"] >= 1
    if name == "camera_on_surface_ahead":
        assert centre["distance"] == 0.0
    if name == "radius_zero":
        assert np.isnan(centre["normal"]).all()
    if name == "plane_parallel_to_ray":
        assert not px["hit"][2, :-1].any() and px["hit"][3, :-1].all() and not px["hit"][:2, :-1].any()
    if name in ("sphere_plane_equal_t_sp", "sphere_plane_equal_t_ps"):
        assert centre["distance"] == np.float32(8.0)
        first_is_sphere = name.endswith("_sp")
        assert (centre["normal"][2] == np.float32(-1.0)) and (np.float32(centre["shading_value"]) == 0.0)
        # same t, same normal (0, 0, -1) at this pixel: only the colour says which object was kept -- the one created first
        lit = steps[0][1].reshape(c["h"], c["w"], 20)[RC.CENTRE] if c["mode"] in (O.RGB_ASCII, O.RGB_PIXEL) else None
        if lit is not None:
            rgb = [int(bytes(lit[o:o + 3]).replace(b"\x00", b"") or b"0") for o in (7, 11, 15)]
            assert (rgb[0] > rgb[2]) == first_is_sphere, rgb
    if name in sees and c["mode"] in (O.RGB_ASCII, O.RGB_PIXEL):
        lit = steps[0][1].reshape(c["h"], c["w"], 20)[RC.CENTRE]
        rgb = [int(bytes(lit[o:o + 3]).replace(b"\x00", b"") or b"0") for o in (7, 11, 15)]
        assert (rgb[0] > rgb[1]) == (sees[name] == RC.RED), rgb
    if name == "colour_saturated" and c["mode"] == O.RGB_PIXEL:
        assert (px["color"][px["hit"] == 1] == 255.0).any()
    if name in ("width_1", "width_2", "height_1"):
        rec = steps[0][1][:S_of(c["mode"]) * c["w"] * c["h"]].reshape(c["h"], c["w"], -1)
        assert not rec[:, -1].any() and (c["w"] == 1 or rec[:, :-1, 0].all())


@pytest.mark.parametrize("mode", RC.MODES)
def test_1024_objects(mode):
    c = RC.big_scene_case(mode)
    assert len(c["objs"]) == 1024
    steps = check_case(c)
    assert steps[0][2]["hit"].mean() > 0.25


# ---------------------------------------------------------------------------------------------------- physics

_PHYSICS = RC.physics_cases()


@pytest.mark.parametrize("c", _PHYSICS, ids=[c["name"] for c in _PHYSICS])
def test_physics(c):
    """Sphere::Update after every step: y and mover against orc_update_objects (inside check_case), and the case's own premise."""
    steps = check_case(c)
    ys = np.array([s[0]["y"] for s in steps])
    movers = np.array([s[0]["mover"] for s in steps])
    assert (np.abs(ys) <= 10.0).all()
    if c["name"] == "physics/lands_on_bound":
        # landing exactly on the bound neither clamps nor flips; the next step does both
        assert ys[0, 0] == 10.0 and movers[0, 0] == 1 and ys[1, 0] == 10.0 and movers[1, 0] == -1
        assert ys[0, 1] == -10.0 and movers[0, 1] == -1 and movers[1, 1] == 1
        assert ys[3, 3] == -10.0 and movers[3, 3] == -1 and movers[4, 3] == 1
    elif c["name"].endswith("_dt0"):
        # dt = 0 moves nothing, yet a sphere created outside [-10, 10] is clamped and flipped by it
        y0 = c["objs"]["center"][:, 1]
        inside = np.abs(y0) <= 10.0
        assert np.array_equal(ys[0][inside], y0[inside]) and (~inside).sum() >= 4
        assert np.array_equal(movers[0][~inside], -c["objs"]["mover"][~inside])
    else:
        assert (movers[-1] != c["objs"]["mover"]).any()


# ---------------------------------------------------------------------------------------------------- Minimize alone

_MINIMIZE = RC.minimize_frames()


@pytest.mark.parametrize("m", _MINIMIZE, ids=[m[0] for m in _MINIMIZE])
def test_minimize_alone(m):
    name, mode, w, h, buf, words = m
    S = S_of(mode)
    got = RH.minimize(mode, buf, w, h)
    want = O.minimize(mode, buf, w, h)
    assert np.array_equal(got, want), "%s: reference %d bytes, oracle %d bytes" % (name, got.size, want.size)
    assert (got == 10).sum() >= h
    # the frame is what its pixel words expand to (tests/test_gpu_ref_parity.py feeds rtx_minimize_words the words)
    kind = ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4")
    assert np.array_equal(U.words_to_records(words, S, kind), buf[:S * w * h])


# ---------------------------------------------------------------------------------------------------- camera

def test_camera_params():
    """Camera3D (SetPos, SetRot, Init, Update, GetInverseVMatrix; Engine3D.cpp:90-97's fill) against orc_camera_params and the
    package's rtx_camera_params: matrix, element1, element2, far, all bits."""
    w, h = RC.CAMERA_SIZE
    poses = RC.camera_poses()
    assert len(poses) == 50
    ref = RH.camera(w, h, poses)
    R = U.pkg()
    for (pos, rot), want in zip(poses, ref):
        orc = RH.raw_of_oracle_params(O.camera_params(w, h, [float(v) for v in pos], [float(v) for v in rot]))
        assert RH.same_bits(orc, want), "oracle: pos %r rot %r: %r != %r" % (pos, rot, orc, want)
        pp = R.camera_params(w, h, [float(v) for v in pos], [float(v) for v in rot])
        got = RH.raw_params(np.array(pp.inv_v[:], dtype=np.float32), pp.cam_pos[:], pp.element1, pp.element2, pp.cam_far)
        assert RH.same_bits(got, want), "package: pos %r rot %r: %r != %r" % (pos, rot, got, want)
