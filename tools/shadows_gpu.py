"""Cost of the light / shadow path on one GPU (same-box A/B, one JSON line per run).

For C2, C3, C5 (whole frames) and C4 (as 8 row slabs, a rank's share at N = 8), mode RGB_ASCII: shadows off (today's one
launch), shadows on (two launches, culled occluders) and RTX_OPT_SHADOW_CHECK 1 (two launches, every sphere tested), each warmed
up, then timed with HIP events around `reps` frames on the context's stream; the median of `batches` batches per frame.  The
kernel statistics come from a separate run under rocprofv3 --kernel-trace --stats, e.g.

    rocprofv3 --kernel-trace --stats -d shadow_prof -o run -- python tools/shadows_gpu.py --reps 5 --batches 2

Usage: python tools/shadows_gpu.py [--configs C2,C3,C5,C4] [--reps 20] [--batches 5]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = importlib.import_module("raytracing-in-windows-console_amd")

STATES = [("off", 0, 0), ("on", 1, 0), ("brute", 1, 1)]


def run(c, p, reps, batches, slabs):
    W, H = int(p.x), int(p.y)
    rows = H // slabs
    bufs = [torch.empty(20 * W * rows, dtype=torch.uint8, device="cuda") for _ in range(slabs)]
    torch.cuda.synchronize()

    def frame():
        for k in range(slabs):
            c.render_rows(p, R.RGB_ASCII, k * rows, rows, d_out=bufs[k].data_ptr(), out_row_base=k * rows)

    for _ in range(5):
        frame()
    c.synchronize()
    per = []
    for _ in range(batches):
        c.timer_start()
        for _ in range(reps):
            frame()
        per.append(c.timer_stop() / reps)
    return float(np.median(per)), c.last_kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5,C4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()
    for name in a.configs.split(","):
        p, sph, pl = R.config_inputs(name)
        slabs = 8 if name == "C4" else 1
        with R.Context(int(p.x), int(p.y)) as c:
            c.set_scene(sph, pl)
            base = None
            for state, shadows, check in STATES:
                c.set_option(R.OPT_SHADOWS, shadows)
                c.set_option(R.OPT_SHADOW_CHECK, check)
                ms, kernel = run(c, p, a.reps, a.batches, slabs)
                base = ms if state == "off" else base
                line = {"config": name, "slabs": slabs, "state": state, "ms_per_frame": round(ms, 5), "vs_off": round(ms / base, 3),
                        "last_kernel": kernel, "shadow_frames": c.get_option(R.STAT_SHADOW_FRAMES)}
                if shadows:
                    line["longest_list"] = c.get_option(R.STAT_SHADOW_LONGEST_LIST)
                    line["spheres"] = int(len(sph))
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
