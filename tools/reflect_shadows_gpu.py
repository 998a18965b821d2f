"""Cost of shadows seen in mirrors (RTX_OPT_REFLECT_SHADOWS) on one GPU: one frame alone, the option off against on, in ONE process.

Scenes: C2floor (C2 with a mirror floor), C2floor+quarter, C3room; mode RGB_ASCII, RTX_OPT_SHADOWS 1; depths 1, 2 and 4; 1 and 3
lights.  Per (scene, depth, lights) the two states alternate round by round, so that drift of the machine hits both alike.  A
round of a state is --frames frames queued back to back on one stream between two device events (the launches of a frame depend
on one another, so back to back is one frame at a time; the events take the enqueue out of the figure); its figure is the elapsed
time over the frames.  Per state: median [min-max] over the rounds -- the spread is the state's own run-to-run spread, what a
difference between two states has to be judged against -- the kernel launched last, the longest occluder list any workgroup held
(RTX_STAT_SHADOW_LONGEST_LIST: level 0's with the option off, the maximum over level 0 and the deeper levels with it on) and the
hit points tested per level (RTX_STAT_REFLECT_SHADOW_POINTS).

--states off with RTX_LIB naming a build of the parent commit (which has no such option) times that build's frames, for an A/B of
the default path: tools/ab_gpu.sh's interleaving, with this tool in place of bench.py.

Usage: python tools/reflect_shadows_gpu.py [--scenes C2floor,C2floor+quarter,C3room] [--depths 1,2,4] [--lights 1,3] [--states off,on]
                                          [--rounds 7] [--frames 40] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 6
SCENES = ["C2floor", "C2floor+quarter", "C3room"]
COLOURS = [(1.0, 0.5, 0.25), (0.25, 1.0, 0.5), (0.5, 0.25, 1.0)]


def scene_inputs(R, name):
    """(params, spheres, planes, {creation index: k}) of a scene; the k of tests/restate.py's _scene_k."""
    import numpy as np
    config, variant = name[:2], name[2:]
    p, sph, pl = R.config_inputs(config)
    ns, ks = len(sph), {}
    if variant in ("floor", "floor+quarter"):
        ks[ns] = 0.5
    if variant == "floor+quarter":
        rng = np.random.default_rng(11)
        for i in rng.choice(ns, size=ns // 4, replace=False):
            ks[int(i)] = float(rng.uniform(0.05, 1.0))
    if variant == "room":
        for q in range(len(pl)):
            ks[ns + q] = 0.7
    return p, sph, pl, ks


def light_set(R, p, n):
    """n lights spread around the camera, above it and below C3's ceiling (y = 30: a light above it is cut off from the whole room by
    the plane test alone, and no tile would walk a sphere)."""
    import numpy as np
    cam = np.array(p.cam_pos[:3], dtype=np.float64)
    out = []
    for i in range(n):
        a = 2.0 * np.pi * ((i * 3) % 8) / 8.0
        pos = cam + np.array([60.0 * np.sin(a), 20.0 + 3.0 * i, 60.0 * np.cos(a)])
        out.append(R.make_light(pos=tuple(float(v) for v in pos), diffuse_rgb=COLOURS[i], diffuse_power=600.0 + 100.0 * i,
                                specular_rgb=COLOURS[(i + 1) % 3], specular_power=900.0))
    return out


def set_state(R, c, on):
    try:
        c.set_option(R.OPT_REFLECT_SHADOWS, 1 if on else 0)
    except (R.RtxError, AttributeError):
        if on:  # (a build of the parent commit has no such option: it can be timed with the option off only)
            raise


def read_stats(R, c):
    try:
        pts = [int(c.get_option(R.STAT_REFLECT_SHADOW_POINTS + l)) for l in range(R.MAX_REFLECT_DEPTH)]
    except (R.RtxError, AttributeError):
        pts = [0] * 4
    return pts, int(c.get_option(R.STAT_SHADOW_LONGEST_LIST))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--depths", default="1,2,4")
    ap.add_argument("--lights", default="1,3")
    ap.add_argument("--states", default="off,on")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table and the states (JSON lines) to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reflect_shadows_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    states = a.states.split(",")
    results, lines = [], []
    lines.append("us per frame (RGB_ASCII, shadows on, one frame alone): median [min-max] over %d rounds of %d frames; library %s" % (
        a.rounds, a.frames, os.path.basename(R.LIB_PATH)))
    for scene in a.scenes.split(","):
        p, sph, pl, ks = scene_inputs(R, scene)
        W, H = int(p.x), int(p.y)
        buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.Stream()  # (the frames and the events that bracket them go to one stream)
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            for i, k in ks.items():
                c.set_reflectivity(int(i), float(k))
            c.set_option(R.OPT_SHADOWS, 1)
            for nl in [int(v) for v in a.lights.split(",")]:
                ls = light_set(R, p, nl)
                if nl == 1:
                    c.set_light(ls[0])
                else:
                    c.set_lights(ls)
                for depth in [int(v) for v in a.depths.split(",")]:
                    c.set_option(R.OPT_REFLECT_DEPTH, depth)
                    us = {s: [] for s in states}
                    info = {}
                    for rnd in range(-1, a.rounds):  # (round -1: every state's warm-up and its counters)
                        for s in states:
                            set_state(R, c, s == "on")
                            if rnd < 0:
                                for _ in range(WARM):
                                    c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)
                                stream.synchronize()
                                pts, longest = read_stats(R, c)
                                info[s] = {"last_kernel": c.last_kernel, "points": pts, "longest_list": longest}
                                continue
                            torch.cuda.synchronize()
                            start.record(stream)
                            for _ in range(a.frames):
                                c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)
                            stop.record(stream)
                            torch.cuda.synchronize()
                            us[s].append(1e3 * start.elapsed_time(stop) / a.frames)
                    cells = []
                    for s in states:
                        d = sorted(us[s])
                        row = {"scene": scene, "lights": nl, "depth": depth, "state": s, "us": {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2),
                              "max": round(d[-1], 2), "rounds": len(d)}, "library": os.path.basename(R.LIB_PATH)}
                        row.update(info[s])
                        results.append(row)
                        cells.append("%s %.1f [%.1f-%.1f] longest %d" % (s, row["us"]["median"], row["us"]["min"], row["us"]["max"], row["longest_list"]))
                    if len(states) == 2:
                        m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
                        cells.append("on/off %.2f, points %s" % (m["on"] / m["off"], info["on"]["points"][:depth]))
                    line = "%-16s lights %d depth %d | %s | %s" % (scene, nl, depth, " | ".join(cells), info[states[-1]]["last_kernel"])
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
