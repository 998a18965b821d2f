"""Cost of spot lights (rtx_scene_set_spots) on one GPU: C2 over a floor (1024 spheres over a plane) at 1920 x 1080, mode RGB_ASCII,
one frame alone, in ONE process per library.

(a) No cone set -- every launch is the kernel it was before there were cones.  Cases `light` (a custom light, shadows on: the
closest hits and rtx_shadow_shade), `mirrors1` and `mirrors4` (the floor k = 0.5 and a quarter of the spheres k = 0.85 under the same
light: rtx_reflect_shade at depth 1, rtx_lights_chain_shade at depth 4), state `none`.  A library that lacks the entry points (a
build of the commit before, --tree DIR: a checkout with its library built) is timed in these alone: run in turns with this build's
processes on the same box, three processes per build, its repeats give the run-to-run range this build's frames are judged against.

(b) Cones set -- cases `eight` (restate.light_set(8), no mirrors, shadows off) and `eight_shadows` (shadows on), states `points` (the
set as point lights) and `cones` (every light a 20 / 12 degree cone aimed at the middle of the spheres).  Per state the frame and
RTX_STAT_SHADOW_LONGEST_LIST.

The whole frame: the states alternate round by round, so that drift of the machine hits all alike; a round is --frames frames queued
back to back on one stream between two device events.  Per state: median [min-max] over the rounds.

The shade launch alone: --trace-pass runs --frames frames per (case, state) in a fixed order and writes that order beside --out; run
it under `rocprofv3 --kernel-trace` in a run of its own, then --fold-trace DIR reads the kernel trace back, takes the shade
dispatches in start order, cuts them by the recorded order and prints the median per (case, state).

Usage: python tools/spot_cost_gpu.py [--cases light,mirrors1,mirrors4,eight,eight_shadows] [--rounds 7] [--frames 40] [--tree DIR] [--out FILE]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/spot_cost_gpu.py --trace-pass --out FILE
       python tools/spot_cost_gpu.py --fold-trace DIR --out FILE
"""
import argparse
import csv
import glob
import importlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 3
CASES = "light,mirrors1,mirrors4,eight,eight_shadows"
W, H = 1920, 1080
OUTER, INNER = 20.0, 12.0


def fold_trace(root, order_path, out):
    """The shade dispatches of a --trace-pass run, cut by the order it recorded: median us per (case, state)."""
    order = json.load(open(order_path))
    paths = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no kernel_trace.csv under %s" % root)
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                if "_shade" in name:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    want = sum(o["launches"] for o in order)
    if len(rows) != want:
        raise SystemExit("the trace holds %d shade dispatches, the pass queued %d" % (len(rows), want))
    lines, at = ["shade launch alone, us (rocprofv3 --kernel-trace): median [min-max] of the timed dispatches"], 0
    for o in order:
        mine = rows[at + o["warm"]:at + o["launches"]]
        at += o["launches"]
        d = sorted((e - s) / 1e3 for s, e, _ in mine)
        names = sorted({n.split("(")[0].split("::")[-1] for _, _, n in mine})
        lines.append("%-13s %-7s | %.1f [%.1f-%.1f] over %d dispatches | %s" % (o["case"], o["state"], d[len(d) // 2], d[0], d[-1], len(d), ",".join(names)))
    print("\n".join(lines))
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are timed (default: this one)")
    ap.add_argument("--out", default=None, help="also write the table and the states (JSON lines) to this file")
    ap.add_argument("--trace-pass", action="store_true", help="no timing: the frames of every (case, state) in a fixed order, recorded in OUT.order.json")
    ap.add_argument("--fold-trace", default=None, metavar="DIR", help="fold the kernel trace under DIR by OUT.order.json")
    a = ap.parse_args()
    if a.fold_trace:
        return fold_trace(a.fold_trace, a.out + ".order.json", a.out)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spot_cost_gpu.py needs a GPU: nothing is timed without one")
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    R = importlib.import_module("raytracing-in-windows-console_amd")
    import restate as RS
    has_spots = hasattr(R.Context, "set_spots")
    _, sph, pl = R.config_inputs("C2")
    p = R.camera_params(W, H)
    n_obj = len(sph) + len(pl)
    quarter = sorted(int(i) for i in np.random.default_rng(21).choice(len(sph), size=len(sph) // 4, replace=False))
    k = np.zeros(n_obj, dtype=np.float32)
    k[quarter] = 0.85
    k[len(sph)] = 0.5
    middle = [float(v) for v in np.asarray(sph, dtype=np.float64)[:, :3].mean(axis=0)]
    eight = RS.light_set(8)
    cones = [(tuple(middle[q] - l.pos[q] for q in range(3)), math.cos(math.radians(OUTER)), math.cos(math.radians(INNER))) for l in eight]
    buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()
    results, order = [], []
    lib = R.LIB_PATH if tree != ROOT else os.path.basename(R.LIB_PATH)
    lines = ["us per frame (RGB_ASCII %d x %d, C2 over a floor; light: a custom light, shadows on; mirrors: floor k 0.5, a quarter of the spheres k 0.85; eight: "
             "restate.light_set(8), as points or as %g / %g degree cones aimed at (%.1f, %.1f, %.1f); one frame alone): median [min-max] over %d rounds of %d frames; "
             "library %s%s" % (W, H, OUTER, INNER, middle[0], middle[1], middle[2], a.rounds, a.frames, lib, "" if has_spots else " (no spot entry points: no cones)")]

    def frame(c):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)

    for case in a.cases.split(","):
        depth = int(case[-1]) if case.startswith("mirrors") else 0
        states = ["none"] if not case.startswith("eight") else (["points", "cones"] if has_spots else ["points"])
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            if case.startswith("eight"):
                c.set_lights([R.make_light(*RS.light_tuple(l)) for l in eight])
                c.set_option(R.OPT_SHADOWS, 1 if case == "eight_shadows" else 0)
            else:
                c.set_light(R.make_light(pos=(5.0, 40.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=900.0, specular_rgb=(0.2, 1.0, 0.4), specular_power=2100.0))
                c.set_option(R.OPT_SHADOWS, 1 if case == "light" else 0)
            if depth:
                c.set_reflectivity(0, k)
                c.set_option(R.OPT_REFLECT_DEPTH, depth)

            def set_state(s):
                if has_spots:
                    c.set_spots(cones if s == "cones" else [])

            us, info, outputs = {s: [] for s in states}, {}, {}
            for s in states:  # warm-up, the kernel, the counters, the bytes
                set_state(s)
                for _ in range(WARM + (a.frames if a.trace_pass else 0)):
                    frame(c)
                stream.synchronize()
                c.synchronize()
                outputs[s] = buf.cpu().numpy().copy()
                info[s] = {"last_kernel": c.last_kernel, "shadow_longest_list": int(c.get_option(R.STAT_SHADOW_LONGEST_LIST))}
                if has_spots:
                    info[s]["spot_lights"] = int(c.get_option(R.STAT_SPOT_LIGHTS))
                order.append({"case": case, "state": s, "warm": WARM, "launches": WARM + a.frames})
            if len(states) == 2 and np.array_equal(outputs["points"], outputs["cones"]):
                raise SystemExit("%s: the cones change no byte" % case)
            if a.trace_pass:
                continue
            for rnd in range(a.rounds):
                for s in states:
                    set_state(s)
                    frame(c)
                    torch.cuda.synchronize()
                    start.record(stream)
                    for _ in range(a.frames):
                        frame(c)
                    stop.record(stream)
                    torch.cuda.synchronize()
                    us[s].append(1e3 * start.elapsed_time(stop) / a.frames)
            cells = []
            for s in states:
                d = sorted(us[s])
                row = {"case": case, "state": s, "us": {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "rounds": len(d)}, "library": lib}
                row.update(info[s])
                results.append(row)
                cells.append("%s %.1f [%.1f-%.1f] longest list %d" % (s, row["us"]["median"], row["us"]["min"], row["us"]["max"], info[s]["shadow_longest_list"]))
            if len(states) == 2:
                m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
                cells.append("cones/points %.3f" % (m["cones"] / m["points"]))
            cells.append(info[states[-1]]["last_kernel"])
            line = "%-13s | %s" % (case, " | ".join(cells))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if a.trace_pass:
            with open(a.out + ".order.json", "w") as f:
                json.dump(order, f)
        else:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
                for row in results:
                    f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
