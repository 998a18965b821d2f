"""Cost of the shadow tests through the world grid (RTX_OPT_SHADOW_GRID) on one GPU: one frame alone, the option off against on, in ONE
process.

States: C2, C3 and C5 (no mirror) with one light inside the scene and with three lights around the camera; C2floor+quarter (C2 with a
mirror floor and a quarter of its spheres reflective) at depth 1 and 4 under RTX_OPT_REFLECT_SHADOWS, one light.  Mode RGB_ASCII,
RTX_OPT_SHADOWS 1.  Per state the option's two values alternate round by round, so that drift of the machine hits both alike.  A
round is --frames frames queued back to back on one stream between two device events (the launches of a frame depend on one another,
so back to back is one frame at a time; the events take the enqueue out of the figure); slow states (C5 with the option off) get
fewer frames a round, at least 3.  Per state: median [min-max] over the rounds -- the spread is the state's own run-to-run spread,
what a difference between the two has to be judged against -- then, of the frames with the option on: the segments that fell back
to testing every sphere (RTX_STAT_SHADOW_GRID_FALLBACK_POINTS) and their share of the (point, light) pairs the launch set tested
(level 0's hit points within the far distance, counted from a values frame, plus RTX_STAT_REFLECT_SHADOW_POINTS), the grid's cells
and pairs, and what the first frame after a physics step costs on the host's clock -- the rebuild blocks -- beside a frame on an
unchanged scene timed the same way.  Both outputs are compared byte for byte before anything is timed.

--states off with RTX_LIB naming a build of the parent commit (which has no such option) times that build's frames, for an A/B of
the default path: tools/ab_gpu.sh's interleaving, with this tool in place of bench.py.

Usage: python tools/shadow_grid_gpu.py [--cases C2:1,C2:3,C3:1,C3:3,C5:1,C5:3,C2floor+quarter:1:1,C2floor+quarter:1:4] [--states off,on]
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
WARM = 4
CASES = "C2:1,C2:3,C3:1,C3:3,C5:1,C5:3,C2floor+quarter:1:1,C2floor+quarter:1:4"
INSIDE = (0.0, 5.0, 120.0)  # (the synthetic scenes' spheres lie 40 .. 200 in front of the camera: a light in the middle of the cloud)


def set_state(R, c, on):
    try:
        c.set_option(R.OPT_SHADOW_GRID, 1 if on else 0)
    except (R.RtxError, AttributeError):
        if on:  # (a build of the parent commit has no such option: it can be timed with the option off only)
            raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES, help="scene:lights[:depth], depth given: mirrors with RTX_OPT_REFLECT_SHADOWS")
    ap.add_argument("--states", default="off,on")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table and the states (JSON lines) to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("shadow_grid_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    import reflect_shadows_gpu as RSG
    states = a.states.split(",")
    results, lines = [], []
    lines.append("us per frame (RGB_ASCII, shadows on, one frame alone): median [min-max] over %d rounds of up to %d frames; library %s" % (
        a.rounds, a.frames, os.path.basename(R.LIB_PATH)))
    for case in a.cases.split(","):
        parts = case.split(":")
        scene, nl, depth = parts[0], int(parts[1]), (int(parts[2]) if len(parts) > 2 else 0)
        p, sph, pl, ks = RSG.scene_inputs(R, scene)
        W, H = int(p.x), int(p.y)
        buf = torch.empty(32 * W * H, dtype=torch.uint8, device="cuda")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.Stream()  # (the frames and the events that bracket them go to one stream)

        def frame(c, flags=0):
            c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream, flags=flags)

        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            for i, k in ks.items():
                c.set_reflectivity(int(i), float(k))
            c.set_option(R.OPT_SHADOWS, 1)
            if nl == 1:
                c.set_light(R.make_light(pos=INSIDE))
            else:
                c.set_lights(RSG.light_set(R, p, nl))
            if depth:
                c.set_option(R.OPT_REFLECT_DEPTH, depth)
                c.set_option(R.OPT_REFLECT_SHADOWS, 1)
            us = {s: [] for s in states}
            info, outputs, frames = {}, {}, {}
            for s in states:  # warm-up, the counters, the bytes, and how many frames a round of this state gets
                set_state(R, c, s == "on")
                for _ in range(WARM):
                    frame(c)
                stream.synchronize()
                t0 = time.perf_counter()
                frame(c)
                stream.synchronize()
                wall = time.perf_counter() - t0
                frames[s] = max(3, min(a.frames, int(0.3 / max(wall, 1e-6))))
                outputs[s] = buf[:20 * W * H].cpu().numpy().copy()
                info[s] = {"last_kernel": c.last_kernel, "frames_per_round": frames[s], "frame_wall_us": round(1e6 * wall, 1)}
                if s == "on":
                    fb = int(c.get_option(R.STAT_SHADOW_GRID_FALLBACK_POINTS))
                    pts = sum(int(c.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(R.MAX_REFLECT_DEPTH))
                    frame(c, R.RENDER_VALUES)
                    stream.synchronize()
                    v = buf.cpu().numpy().view(np.float32).reshape(-1, 8)[:, 0]
                    pts += int(((v != np.float32(99999999.0)) & (v <= np.float32(p.cam_far)) & (np.arange(W * H) % W != W - 1)).sum())
                    info[s].update({"fallback_segments": fb, "tested_pairs_at_most": pts * nl, "fallback_share": round(fb / max(pts * nl, 1), 4),
                                    "grid_cells": int(c.get_option(R.STAT_QUERY_GRID_CELLS)), "grid_pairs": int(c.get_option(R.STAT_QUERY_GRID_PAIRS)),
                                    "large_spheres": int(c.get_option(R.STAT_QUERY_LARGE_SPHERES)), "grid_frames": int(c.get_option(R.STAT_SHADOW_GRID_FRAMES))})
            if len(states) == 2 and not np.array_equal(outputs["off"], outputs["on"]):
                raise SystemExit("%s: the option changes the frame" % case)
            for rnd in range(a.rounds):
                for s in states:
                    set_state(R, c, s == "on")
                    frame(c)
                    torch.cuda.synchronize()
                    start.record(stream)
                    for _ in range(frames[s]):
                        frame(c)
                    stop.record(stream)
                    torch.cuda.synchronize()
                    us[s].append(1e3 * start.elapsed_time(stop) / frames[s])
            if "on" in states:  # the first frame after a physics step: the rebuild blocks, so the host's clock sees it
                set_state(R, c, True)
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
                row = {"case": case, "scene": scene, "lights": nl, "depth": depth, "state": s,
                       "us": {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "rounds": len(d)},
                       "library": os.path.basename(R.LIB_PATH)}
                row.update(info[s])
                results.append(row)
                cells.append("%s %.1f [%.1f-%.1f]" % (s, row["us"]["median"], row["us"]["min"], row["us"]["max"]))
            if len(states) == 2:
                m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
                i = info["on"]
                cells.append("on/off %.3f | fallback %d of %d (%.1f %%) | cells %d pairs %d large %d | frame after a physics step %.0f us on the host's clock, "
                             "unchanged scene %.0f" % (m["on"] / m["off"], i["fallback_segments"], i["tested_pairs_at_most"], 100.0 * i["fallback_share"],
                                                       i["grid_cells"], i["grid_pairs"], i["large_spheres"], i["frame_after_physics_wall_us"], i["frame_wall_us"]))
            line = "%-22s | %s | %s" % (case, " | ".join(cells), info[states[-1]]["last_kernel"])
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
