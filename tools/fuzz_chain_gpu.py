#!/usr/bin/env python3
"""Randomised check of the deep mirror chains under light sets against the numpy restatement (tests/restate.py): fuzzed scenes
(general camera matrices, cameras inside spheres, tiny radii, planes with arbitrary normals) with random k and 1-3 random lights
at depth 4, the eight value floats of a pixel sample bit for bit.  The long-running front end of
tests/fuzz_cases.py::chain_case (tests/test_gpu_chain_lights.py runs 12 fixed seeds inside `pytest -m gpu`).

  python tools/fuzz_chain_gpu.py [seconds] [first_seed]
"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fuzz_cases as F  # noqa: E402

R = importlib.import_module("raytracing-in-windows-console_amd")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
budget = float(args[0]) if len(args) > 0 else 120.0
seed0 = int(args[1]) if len(args) > 1 else 1

t_end = time.time() + budget
seed, bad = seed0, 0
stats = {}
with R.Context(640, 360) as ctx:
    while time.time() < t_end:
        for line in F.chain_case(R, torch, ctx, seed, stats=stats):
            bad += 1
            print("DIFF " + line, flush=True)
        if seed % 20 == 0:
            print("... seed %d, %d pixels (%d visible), %d findings" % (seed, stats.get("pixels", 0), stats.get("visible", 0), bad), flush=True)
        seed += 1
print("fuzz chain: seeds %d..%d, %d pixels, %d visible, rays per level %s, %d with a NaN, %d findings" % (
    seed0, seed - 1, stats.get("pixels", 0), stats.get("visible", 0), [stats.get("rays%d" % j, 0) for j in (1, 2, 3, 4)], stats.get("nan", 0), bad))
sys.exit(1 if bad else 0)
