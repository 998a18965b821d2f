"""Cost of the mirror path on one GPU (same-box A/B, one JSON line per run).

Scenes (mode RGB_ASCII, whole frames): C2 with the floor at k = 0.5 ("floor"), C2 with the floor and a fixed-seed quarter of the
spheres at random k ("floor+quarter"), C3 with its six planes at k = 0.7 ("room"), C5 with a quarter of the spheres at random k
("quarter").  Per scene: nothing reflective (today's one launch), the mirror path (three launches, culled secondary pass) and
RTX_OPT_REFLECT_CHECK 1 (every sphere tested), each warmed up, then timed two ways: one frame alone (HIP events around `reps`
frames on the context's stream, the median of `batches` batches) and 4 frames in flight (render_rows round robin on 4 streams,
wall time over `reps` frames after a synchronize).  RTX_STAT_REFLECT_LONGEST_LIST is read after each run.  The per-kernel times come
from a separate run under rocprofv3 --kernel-trace --stats, e.g.

    rocprofv3 --kernel-trace --stats -d reflect_prof -o run -- python tools/reflect_gpu.py --reps 5 --batches 2

Usage: python tools/reflect_gpu.py [--scenes floor,floor+quarter,room,quarter] [--reps 20] [--batches 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = importlib.import_module("raytracing-in-windows-console_amd")

SCENES = {"floor": "C2", "floor+quarter": "C2", "room": "C3", "quarter": "C5"}


def reflectivities(variant, ns, npl):
    """creation index -> k (spheres first, then planes), as tests/test_gpu_reflect.py's scenes"""
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


def alone(c, p, reps, batches, buf):
    H = int(p.y)
    for _ in range(5):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr())
    c.synchronize()
    per = []
    for _ in range(batches):
        c.timer_start()
        for _ in range(reps):
            c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr())
        per.append(c.timer_stop() / reps)
    return float(np.median(per))


def in_flight(c, p, reps, bufs, streams):
    H = int(p.y)
    for k in range(8):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=bufs[k % 4].data_ptr(), stream=streams[k % 4].cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(reps):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=bufs[k % 4].data_ptr(), stream=streams[k % 4].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="floor,floor+quarter,room,quarter")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()
    for variant in a.scenes.split(","):
        name = SCENES[variant]
        p, sph, pl = R.config_inputs(name)
        W, H = int(p.x), int(p.y)
        bufs = [torch.empty(20 * W * H, dtype=torch.uint8, device="cuda") for _ in range(4)]
        streams = [torch.cuda.Stream() for _ in range(4)]
        torch.cuda.synchronize()
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            ks = reflectivities(variant, len(sph), len(pl))
            base = None
            for state, check in (("off", 0), ("mirror", 0), ("brute", 1)):
                c.set_reflectivity(0, np.zeros(len(sph) + len(pl), dtype=np.float32))
                if state != "off":
                    for i, k in ks.items():
                        c.set_reflectivity(i, k)
                c.set_option(R.OPT_REFLECT_CHECK, check)
                ms = alone(c, p, a.reps, a.batches, bufs[0])
                kernel = c.last_kernel
                longest = c.get_option(R.STAT_REFLECT_LONGEST_LIST)
                ms4 = in_flight(c, p, a.reps, bufs, streams)
                base = (ms, ms4) if state == "off" else base
                line = {"scene": variant, "config": name, "state": state, "ms_alone": round(ms, 5), "ms_in_flight_4": round(ms4, 5),
                        "vs_off_alone": round(ms / base[0], 3), "vs_off_in_flight": round(ms4 / base[1], 3), "last_kernel": kernel,
                        "reflective": len(ks), "spheres": int(len(sph))}
                if state != "off":
                    line["longest_list"] = longest
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
