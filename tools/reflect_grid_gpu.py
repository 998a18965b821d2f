"""Cost of the mirror rays through the world grid (RTX_OPT_REFLECT_GRID) on one GPU: one frame alone, the option off against on, in ONE
process.

States: C2floor (C2 with a mirror floor), C2floor+quarter (and a quarter of its spheres reflective), C3room (C3's six planes
mirrors) and C5quarter (a quarter of C5's spheres reflective), each at depth 1 and depth 4.  Mode RGB_ASCII at 1920 x 1080, the
reference's light, no shadow test.  Per state the option's two values alternate round by round, so that drift of the machine hits
both alike; the baseline of every ratio is the option off in the same process -- the existing kernels, not the code under test.  A
round is --frames frames queued back to back on one stream between two device events (the launches of a frame depend on one
another, so back to back is one frame at a time; the events take the enqueue out of the figure); slow states get fewer frames a
round, at least 3.  Per state: median [min-max] over the rounds -- the spread is the state's own run-to-run spread, what a
difference between the two has to be judged against -- then, of the frames with the option on: the rays per level
(RTX_STAT_REFLECT_RAYS), the rays that fell back to testing every sphere (RTX_STAT_REFLECT_GRID_FALLBACK_RAYS) and their share, the
grid's cells and pairs, and what the first frame after a physics step costs on the host's clock -- the rebuild blocks -- beside a
frame on an unchanged scene timed the same way.  Both outputs are compared byte for byte before anything is timed.

Usage: python tools/reflect_grid_gpu.py [--cases C2floor:1,C2floor:4,C2floor+quarter:1,C2floor+quarter:4,C3room:1,C3room:4,C5quarter:1,C5quarter:4]
                                        [--rounds 7] [--frames 40] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM = 3
CASES = "C2floor:1,C2floor:4,C2floor+quarter:1,C2floor+quarter:4,C3room:1,C3room:4,C5quarter:1,C5quarter:4"
W, H = 1920, 1080


def scene_inputs(R, name):
    """(params at 1920 x 1080, spheres, planes, {creation index: k}); `quarter`: a quarter of the spheres, no plane."""
    import numpy as np
    import reflect_shadows_gpu as RSG
    if name.endswith("quarter") and "+" not in name:
        _, sph, pl = R.config_inputs(name[:2])
        rng = np.random.default_rng(11)
        ks = {int(i): float(rng.uniform(0.05, 1.0)) for i in rng.choice(len(sph), size=len(sph) // 4, replace=False)}
    else:
        _, sph, pl, ks = RSG.scene_inputs(R, name)
    return R.camera_params(W, H), sph, pl, ks  # (every configuration is 16 : 9: the projection terms its scene was made with are these)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES, help="scene:depth")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table and the states (JSON lines) to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reflect_grid_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    states = ["off", "on"]
    results, lines = [], []
    lines.append("us per frame (RGB_ASCII %d x %d, one frame alone): median [min-max] over %d rounds of up to %d frames; library %s" % (
        W, H, a.rounds, a.frames, os.path.basename(R.LIB_PATH)))
    buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()  # (the frames and the events that bracket them go to one stream)
    loaded = (None, None)
    for case in a.cases.split(","):
        scene, depth = case.split(":")[0], int(case.split(":")[1])
        if loaded[0] != scene:
            loaded = (scene, scene_inputs(R, scene))
        p, sph, pl, ks = loaded[1]

        def frame(c):
            c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)

        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            k = np.zeros(len(sph) + len(pl), dtype=np.float32)
            for i, v in ks.items():
                k[int(i)] = v
            c.set_reflectivity(0, k)
            c.set_option(R.OPT_REFLECT_DEPTH, depth)
            us = {s: [] for s in states}
            info, outputs, frames = {}, {}, {}
            for s in states:  # warm-up, the counters, the bytes, and how many frames a round of this state gets
                c.set_option(R.OPT_REFLECT_GRID, 1 if s == "on" else 0)
                for _ in range(WARM):
                    frame(c)
                stream.synchronize()
                t0 = time.perf_counter()
                frame(c)
                stream.synchronize()
                wall = time.perf_counter() - t0
                frames[s] = max(3, min(a.frames, int(0.3 / max(wall, 1e-6))))
                outputs[s] = buf.cpu().numpy().copy()
                info[s] = {"last_kernel": c.last_kernel, "frames_per_round": frames[s], "frame_wall_us": round(1e6 * wall, 1),
                           "longest_list": int(c.get_option(R.STAT_REFLECT_LONGEST_LIST))}
                if s == "on":
                    rays = [int(c.get_option(R.STAT_REFLECT_RAYS + l)) for l in range(R.MAX_REFLECT_DEPTH)]
                    fb = int(c.get_option(R.STAT_REFLECT_GRID_FALLBACK_RAYS))
                    info[s].update({"rays": rays, "fallback_rays": fb, "fallback_share": round(fb / max(sum(rays), 1), 4),
                                    "grid_cells": int(c.get_option(R.STAT_QUERY_GRID_CELLS)), "grid_pairs": int(c.get_option(R.STAT_QUERY_GRID_PAIRS)),
                                    "large_spheres": int(c.get_option(R.STAT_QUERY_LARGE_SPHERES)), "grid_frames": int(c.get_option(R.STAT_REFLECT_GRID_FRAMES))})
            if not np.array_equal(outputs["off"], outputs["on"]):
                raise SystemExit("%s: the option changes the frame" % case)
            if info["on"]["grid_frames"] == 0:
                raise SystemExit("%s: the option is not in effect" % case)
            for rnd in range(a.rounds):
                for s in states:
                    c.set_option(R.OPT_REFLECT_GRID, 1 if s == "on" else 0)
                    frame(c)
                    torch.cuda.synchronize()
                    start.record(stream)
                    for _ in range(frames[s]):
                        frame(c)
                    stop.record(stream)
                    torch.cuda.synchronize()
                    us[s].append(1e3 * start.elapsed_time(stop) / frames[s])
            # the first frame after a physics step: the rebuild blocks, so the host's clock sees it
            c.set_option(R.OPT_REFLECT_GRID, 1)
            walls = []
            for _ in range(5):
                c.update_objects(0.01)
                c.synchronize()
                t0 = time.perf_counter()
                frame(c)
                stream.synchronize()
                walls.append(1e6 * (time.perf_counter() - t0))
            info["on"]["frame_after_physics_wall_us"] = round(sorted(walls)[2], 1)
            info["on"]["grid_builds"] = int(c.get_option(R.STAT_QUERY_GRID_BUILDS))
            cells = []
            for s in states:
                d = sorted(us[s])
                row = {"case": case, "scene": scene, "depth": depth, "state": s,
                       "us": {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "rounds": len(d)},
                       "library": os.path.basename(R.LIB_PATH)}
                row.update(info[s])
                results.append(row)
                cells.append("%s %.1f [%.1f-%.1f]" % (s, row["us"]["median"], row["us"]["min"], row["us"]["max"]))
            m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
            i = info["on"]
            cells.append("on/off %.3f | rays %s | fallback %d (%.1f %%) | longest list off %d | cells %d pairs %d large %d | frame after a physics step %.0f us on "
                         "the host's clock, unchanged scene %.0f" % (m["on"] / m["off"], "/".join(str(r) for r in i["rays"]), i["fallback_rays"],
                                                                     100.0 * i["fallback_share"], info["off"]["longest_list"], i["grid_cells"], i["grid_pairs"],
                                                                     i["large_spheres"], i["frame_after_physics_wall_us"], i["frame_wall_us"]))
            line = "%-20s | %s" % (case, " | ".join(cells))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            for row in results:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
