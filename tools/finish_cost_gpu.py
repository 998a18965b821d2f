"""Cost of per-object finishes (rtx_scene_set_finish) on one GPU: C2 over a floor (1024 spheres over a plane) at 1920 x 1080, mode
RGB_ASCII, one frame alone, in ONE process per library.

Cases: `light` (a custom light, no mirrors: the closest hits and rtx_shadow_shade), `mirrors1` and `mirrors4` (the floor k = 0.5 and
a quarter of the spheres k = 0.85 under the same light: rtx_reflect_shade at depth 1, rtx_lights_chain_shade at depth 4).  States:
`none` (every object has the default finish: every launch is what it is without the call), `quarter` (a quarter of the spheres and the
floor finished) and `all` (every object).  A library that lacks the entry points (a build of the commit before, --tree DIR: a
checkout with its library built) is timed in the state `none` alone: run in turns with this build's processes on the same box, its
repeats give the run-to-run range this build's `none` frames are judged against.

The whole frame: the states alternate round by round, so that drift of the machine hits all alike; a round is --frames frames queued
back to back on one stream between two device events.  Per state: median [min-max] over the rounds.

The shade launch alone: --trace-pass runs --frames frames per (case, state) in a fixed order and writes that order beside --out; run
it under `rocprofv3 --kernel-trace` in a run of its own, then --fold-trace DIR reads the kernel trace back, takes the shade
dispatches in start order, cuts them by the recorded order and prints the median per (case, state).

Usage: python tools/finish_cost_gpu.py [--cases light,mirrors1,mirrors4] [--rounds 7] [--frames 40] [--tree DIR] [--out FILE]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/finish_cost_gpu.py --trace-pass --out FILE
       python tools/finish_cost_gpu.py --fold-trace DIR --out FILE
"""
import argparse
import csv
import glob
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 3
CASES = "light,mirrors1,mirrors4"
W, H = 1920, 1080
FINISHES = [(0.2, 1.0, 0.0, 5), (0.1, 0.8, 1.7, 7), (0.8, 0.3, 1.0, 0), (0.3, 1.0, 0.6, 3)]  # dealt round over the finished objects


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
        lines.append("%-8s %-8s | %.1f [%.1f-%.1f] over %d dispatches | %s" % (o["case"], o["state"], d[len(d) // 2], d[0], d[-1], len(d), ",".join(names)))
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
        raise SystemExit("finish_cost_gpu.py needs a GPU: nothing is timed without one")
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    R = importlib.import_module("raytracing-in-windows-console_amd")
    has_finish = hasattr(R.Context, "set_finish")
    states = ["none", "quarter", "all"] if has_finish else ["none"]
    _, sph, pl = R.config_inputs("C2")
    p = R.camera_params(W, H)
    n_obj = len(sph) + len(pl)
    quarter = sorted(int(i) for i in np.random.default_rng(21).choice(len(sph), size=len(sph) // 4, replace=False))
    k = np.zeros(n_obj, dtype=np.float32)
    k[quarter] = 0.85
    k[len(sph)] = 0.5
    finished = {"none": [], "quarter": quarter + [len(sph)], "all": list(range(n_obj))}
    buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()
    results, order = [], []
    lines = ["us per frame (RGB_ASCII %d x %d, C2 over a floor, a custom light; mirrors: floor k 0.5, a quarter of the spheres k 0.85; one frame alone): "
             "median [min-max] over %d rounds of %d frames; library %s%s" % (W, H, a.rounds, a.frames, R.LIB_PATH if tree != ROOT else os.path.basename(R.LIB_PATH),
                                                                              "" if has_finish else " (no finish entry points: state `none` alone)")]

    def frame(c):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)

    def set_state(c, s):
        if has_finish:
            fin = [R.make_finish()] * n_obj
            for j, i in enumerate(finished[s]):
                fin[i] = R.make_finish(*FINISHES[j % len(FINISHES)])
            c.set_finish(0, fin)

    for case in a.cases.split(","):
        depth = int(case[-1]) if case.startswith("mirrors") else 0
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            c.set_light(R.make_light(pos=(5.0, 40.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=900.0, specular_rgb=(0.2, 1.0, 0.4), specular_power=2100.0))
            if depth:
                c.set_reflectivity(0, k)
                c.set_option(R.OPT_REFLECT_DEPTH, depth)
            us, info, outputs = {s: [] for s in states}, {}, {}
            for s in states:  # warm-up, the kernel, the counters, the bytes
                set_state(c, s)
                for _ in range(WARM + (a.frames if a.trace_pass else 0)):
                    frame(c)
                stream.synchronize()
                c.synchronize()
                outputs[s] = buf.cpu().numpy().copy()
                info[s] = {"last_kernel": c.last_kernel}
                if has_finish:
                    info[s]["finished_objects"] = int(c.get_option(R.STAT_FINISHED_OBJECTS))
                order.append({"case": case, "state": s, "warm": WARM, "launches": WARM + a.frames})
            if has_finish and (np.array_equal(outputs["none"], outputs["quarter"]) or np.array_equal(outputs["quarter"], outputs["all"])):
                raise SystemExit("%s: the finishes change no byte" % case)
            if a.trace_pass:
                continue
            for rnd in range(a.rounds):
                for s in states:
                    set_state(c, s)
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
                row = {"case": case, "state": s, "us": {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "rounds": len(d)},
                       "library": R.LIB_PATH if tree != ROOT else os.path.basename(R.LIB_PATH)}
                row.update(info[s])
                results.append(row)
                cells.append("%s %.1f [%.1f-%.1f]" % (s, row["us"]["median"], row["us"]["min"], row["us"]["max"]))
            if has_finish:
                m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
                cells.append("quarter/none %.3f all/none %.3f" % (m["quarter"] / m["none"], m["all"] / m["none"]))
            cells.append(info[states[-1]]["last_kernel"])
            line = "%-8s | %s" % (case, " | ".join(cells))
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
