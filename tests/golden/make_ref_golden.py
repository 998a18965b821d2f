#!/usr/bin/env python3
"""Generates tests/golden/ref_cases.npz from the host build of the reference's own sources (oracle/_ref/, built by
oracle/Makefile where the reference lies on the machine): inputs and the reference's outputs for the subset of
tests/test_ref_host.py that tests/ref_cases.py names -- the directed edges in all five modes, the 1024-object scene, two
dozen small fuzz seeds, the physics sequences, a dozen Minimize frames, the fifty camera poses.

Where the binaries are absent, tests/test_ref_fixtures.py and tests/test_gpu_ref_parity.py hold the oracle and the kernels
to this recording; where they are present, test_ref_fixtures.py also holds the recording to the binaries.

Frames and minimised streams come from ref_driver_pinpow (pow as five squarings in double: the C library's powf is not the
same on every machine).  Frames of at most ref_cases.STORE_PIXELS pixels are stored whole with their streams; larger ones as
standard FNV-1a-64 hashes of the 20*W*H host array and of the stream.  Sphere y and mover are stored for every step.

Usage: python tests/golden/make_ref_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_cases as RC  # noqa: E402
import ref_host as RH  # noqa: E402


def main():
    ok, why = RH.availability()
    if not ok:
        sys.exit("make_ref_golden: " + why)
    out = {}
    cases = RC.fixture_update_cases()
    # one array per field over all cases (an .npz entry per case and field would cost more than the data)
    meta, objs, dts, states, frames, streams, stream_lens, hashes = [], [], [], [], [], [], [], []
    for c in cases:
        e = RC.expect_from_live(c)
        stored = c["w"] * c["h"] <= RC.STORE_PIXELS
        meta.append([c["w"], c["h"], c["mode"], len(c["objs"]), len(c["dts"]), int(stored)])
        objs.append(c["objs"].view(np.uint8))
        dts.append(np.array(c["dts"], dtype=np.float64))
        states.append(np.stack(e["states"]).view(np.uint8).reshape(-1))
        if stored:
            frames += e["frames"]
            streams += e["streams"]
            stream_lens += [s.size for s in e["streams"]]
        else:
            hashes += [[RC.hash_of(f), RC.hash_of(s)] for f, s in zip(e["frames"], e["streams"])]
    out["names"] = np.array([c["name"] for c in cases])
    out["meta"] = np.array(meta, dtype=np.int32)
    out["params"] = np.stack([c["params"] for c in cases])
    out["objs"] = np.concatenate(objs)
    out["dts"] = np.concatenate(dts)
    out["states"] = np.concatenate(states)
    out["frames"] = np.concatenate(frames)
    out["streams"] = np.concatenate(streams)
    out["stream_lens"] = np.array(stream_lens, dtype=np.int64)
    out["hashes"] = np.array(hashes, dtype=np.uint64).reshape(-1, 2)
    mins = RC.minimize_frames(full=False)
    out["min_names"] = np.array([m[0] for m in mins])
    out["min_meta"] = np.array([[mode, w, h] for _, mode, w, h, _, _ in mins], dtype=np.int32)
    out["min_words"] = np.concatenate([words for *_, words in mins])
    ref_streams = [RH.minimize(mode, buf, w, h) for _, mode, w, h, buf, _ in mins]
    out["min_streams"] = np.concatenate(ref_streams)
    out["min_stream_lens"] = np.array([s.size for s in ref_streams], dtype=np.int64)
    poses = RC.camera_poses()
    out["cam_poses"] = np.array([list(p) + list(r) for p, r in poses], dtype=np.float32)
    out["cam_params"] = RH.camera(RC.CAMERA_SIZE[0], RC.CAMERA_SIZE[1], poses)
    np.savez_compressed(RC.FIXTURE, **out)
    print("%s: %d Update cases, %d Minimize frames, %d camera poses, %d bytes" % (
        os.path.relpath(RC.FIXTURE), len(cases), len(mins), len(poses), os.path.getsize(RC.FIXTURE)))


if __name__ == "__main__":
    main()
