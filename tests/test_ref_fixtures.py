"""tests/golden/ref_cases.npz holds what the host build of the reference's own sources gave (tests/golden/make_ref_golden.py)
for the directed edges, the 1024-object scene, two dozen small fuzz seeds, the physics sequences, a dozen Minimize frames and
fifty camera poses.  Here the oracle has to reproduce every recorded output, bit for bit, on any machine; and where the
binaries are present (tests/ref_host.py) they have to reproduce the recording too, so that it cannot drift from them.
Nothing here skips: without the binaries the second half has nothing to compare and says so in its name only.
"""
import numpy as np
import pytest

import oracle as O
import ref_cases as RC
import ref_host as RH
import util as U

CASES, MINIMIZE, (CAM_POSES, CAM_PARAMS) = RC.load_fixture()
LIVE = RH.have_binaries()


def test_the_recording_is_the_subset_the_generator_names():
    want = RC.fixture_update_cases()
    assert [c["name"] for c in CASES] == [c["name"] for c in want]
    for got, c in zip(CASES, want):
        assert got["objs"].tobytes() == c["objs"].tobytes() and RH.same_bits(got["params"], c["params"]), c["name"]
        assert (got["w"], got["h"], got["mode"], got["dts"]) == (c["w"], c["h"], c["mode"], c["dts"]), c["name"]
    assert [m[0] for m in MINIMIZE] == [m[0] for m in RC.minimize_frames(full=False)]
    assert len(CAM_POSES) == 50 and len(MINIMIZE) == 12
    names = {c["name"].split("/")[0] for c in CASES}
    assert {"coincident_spheres_ab", "tangent_discriminant_zero", "far_equals_hit", "radius_zero", "width_1", "objects_1024", "physics"} <= names
    assert sum(n.startswith("fuzzfix") for n in names) == RC.FUZZ_FIXTURE_SEEDS


def check_against(c, steps_of):
    """steps_of(c) -> per step (states, frame, stream)."""
    e = c["expect"]
    for k, (st, frame, stream) in enumerate(steps_of(c)):
        assert np.array_equal(st["y"].view(np.uint32), e["states"][k]["y"].view(np.uint32)) and \
            np.array_equal(st["mover"], e["states"][k]["mover"]), "%s step %d: sphere y / mover differ from the recording" % (c["name"], k)
        detail = U.first_diff(frame, e["frames"][k], 20 if c["mode"] >= O.RGB_ASCII else 12, c["w"]) if "frames" in e else "recorded as a hash"
        assert RC.frame_matches(e, k, frame), "%s step %d: frame differs from the recording: %s" % (c["name"], k, detail)
        assert RC.stream_matches(e, k, stream), "%s step %d: minimised stream differs from the recording" % (c["name"], k)


def oracle_steps(c):
    out = []
    for st, frame, px in RC.oracle_steps(c, O.NORMALS_WRAP):
        # the host build's glyph for ramp index 68 is whatever lies past ASCII[]: such a pixel is not recorded
        assert RC.ramp68_mask(c, px)[1] == 0, c["name"]
        out.append((st, frame, O.minimize(c["mode"], frame, c["w"], c["h"])))
    return out


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_oracle_reproduces_recorded_update(c):
    check_against(c, oracle_steps)


@pytest.mark.parametrize("m", MINIMIZE, ids=[m[0] for m in MINIMIZE])
def test_oracle_reproduces_recorded_minimize(m):
    name, mode, w, h, buf, words, stream = m
    assert np.array_equal(O.minimize(mode, buf, w, h), stream)


def test_camera_builders_reproduce_recorded_params():
    w, h = RC.CAMERA_SIZE
    R = U.pkg()
    for pose, want in zip(CAM_POSES, CAM_PARAMS):
        pos, rot = [float(v) for v in pose[:3]], [float(v) for v in pose[3:]]
        assert RH.same_bits(RH.raw_of_oracle_params(O.camera_params(w, h, pos, rot)), want), "oracle, pose %r" % (pose,)
        pp = R.camera_params(w, h, pos, rot)
        got = RH.raw_params(np.array(pp.inv_v[:], dtype=np.float32), pp.cam_pos[:], pp.element1, pp.element2, pp.cam_far)
        assert RH.same_bits(got, want), "package, pose %r" % (pose,)


def test_live_binary_reproduces_the_recording():
    """Where oracle/_ref/ holds the binaries: ref_driver_pinpow gives the recorded frames, streams and states, MinimizeResults
    the recorded streams, Camera3D the recorded params.  Elsewhere there is nothing to run, and the oracle tests above stand."""
    if not LIVE:
        return
    for c in CASES:
        check_against(c, lambda c: zip(*(lambda r: (r.states, r.frames, r.streams))(RC.run_reference(c, RH.PINPOW))))
    for name, mode, w, h, buf, words, stream in MINIMIZE:
        for binary in (RH.STOCK, RH.PINPOW):
            assert np.array_equal(RH.minimize(mode, buf, w, h, binary=binary), stream), name
    got = RH.camera(RC.CAMERA_SIZE[0], RC.CAMERA_SIZE[1], [(p[:3], p[3:]) for p in CAM_POSES])
    assert RH.same_bits(got, CAM_PARAMS)
