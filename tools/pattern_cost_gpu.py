"""Cost of checker patterns (rtx_scene_set_patterns) on one GPU: C2 with a floor ("floor+quarter": 1024 spheres over a plane) at
1920 x 1080, mode RGB_ASCII, one frame alone, in ONE process per library.

Cases: `light` (a custom light, no mirrors: closest hit + rtx_shadow_shade), `mirror1` and `mirror4` (the floor and a quarter of the
spheres reflective, the reference's light, depth 1 and depth 4).  States: `none` (a table of two entries, no slot assigned: every
launch is what it is without patterns) and `patterned` (slot 1, a two-axis checker, on the floor; slot 2, a three-axis one, on a
quarter of the spheres).  A library that lacks the entry points (a build of the commit before) is timed in the state `none` alone,
without a table: with --out of both, its repeats give the run-to-run spread the unpatterned frames of this commit are judged against.

The whole frame: the states alternate round by round, so that drift of the machine hits both alike; a round is --frames frames queued
back to back on one stream between two device events (the launches of a frame depend on one another, so back to back is one frame at
a time; the events take the enqueue out of the figure).  Per state: median [min-max] over the rounds.

The shade launch alone: --trace-pass runs --frames frames per (case, state) in a fixed order and writes that order beside --out; run
it under `rocprofv3 --kernel-trace` in a run of its own, then --fold-trace DIR reads the kernel trace back, takes the *_shade
dispatches in start order, cuts them by the recorded order and prints the median per (case, state).

Usage: python tools/pattern_cost_gpu.py [--cases light,mirror1,mirror4] [--rounds 7] [--frames 40] [--out FILE]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pattern_cost_gpu.py --trace-pass --out FILE
       python tools/pattern_cost_gpu.py --fold-trace DIR --out FILE
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
CASES = "light,mirror1,mirror4"
W, H = 1920, 1080
TABLE = [((0.37, 0.0, 0.41), (0.25, 0.0, 0.25), (20.0, 20.0, 20.0)), ((0.13, 0.29, 0.07), (0.5, 0.5, 0.5), (250.0, 250.0, 250.0))]


def fold_trace(root, order_path, out):
    """The *_shade dispatches of a --trace-pass run, cut by the order it recorded: median us per (case, state)."""
    order = json.load(open(order_path))
    paths = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no kernel_trace.csv under %s" % root)
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                if "_shade" in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    want = sum(o["launches"] for o in order)
    if len(rows) != want:
        raise SystemExit("the trace holds %d shade dispatches, the pass queued %d" % (len(rows), want))
    lines, at = ["shade launch alone, us (rocprofv3 --kernel-trace): median [min-max] of the timed dispatches"], 0
    for o in order:
        mine = rows[at + o["warm"]:at + o["launches"]]
        at += o["launches"]
        d = sorted((e - s) / 1e3 for s, e, _ in mine)
        names = sorted({n.split("<")[0].split("(")[0].split("::")[-1] for _, _, n in mine})
        lines.append("%-8s %-10s | %.1f [%.1f-%.1f] over %d dispatches | %s" % (o["case"], o["state"], d[len(d) // 2], d[0], d[-1], len(d), ",".join(names)))
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
    ap.add_argument("--out", default=None, help="also write the table and the states (JSON lines) to this file")
    ap.add_argument("--trace-pass", action="store_true", help="no timing: the frames of every (case, state) in a fixed order, recorded in OUT.order.json")
    ap.add_argument("--fold-trace", default=None, metavar="DIR", help="fold the kernel trace under DIR by OUT.order.json")
    a = ap.parse_args()
    if a.fold_trace:
        return fold_trace(a.fold_trace, a.out + ".order.json", a.out)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pattern_cost_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    R = importlib.import_module("raytracing-in-windows-console_amd")
    import restate as RS
    has_patterns = hasattr(R, "make_pattern")
    states = ["none", "patterned"] if has_patterns else ["none"]
    _, sph, pl = R.config_inputs("C2")
    p = R.camera_params(W, H)
    ks = RS._scene_k("C2", sph, pl, "floor+quarter")
    quarter = sorted(int(i) for i in np.random.default_rng(21).choice(len(sph), size=len(sph) // 4, replace=False))
    buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()
    results, order = [], []
    lines = ["us per frame (RGB_ASCII %d x %d, C2 floor+quarter, one frame alone): median [min-max] over %d rounds of %d frames; library %s%s" % (
        W, H, a.rounds, a.frames, os.path.basename(R.LIB_PATH), "" if has_patterns else " (no pattern entry points: state `none` alone)")]

    def frame(c):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)

    def set_state(c, s):
        if has_patterns:
            c.set_object_pattern(0, 0, n=len(sph) + len(pl))
            if s == "patterned":
                c.set_object_pattern(len(sph), 1)
                for i in quarter:
                    c.set_object_pattern(i, 2)

    for case in a.cases.split(","):
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            if case == "light":
                c.set_light(R.make_light(*RS.light_tuple(RS.CUSTOM_LIGHT)))
            else:
                k = np.zeros(len(sph) + len(pl), dtype=np.float32)
                for i, v in ks.items():
                    k[int(i)] = v
                c.set_reflectivity(0, k)
                c.set_option(R.OPT_REFLECT_DEPTH, int(case[len("mirror"):]))
            if has_patterns:
                c.set_patterns([R.make_pattern(*t) for t in TABLE])
            us, info, outputs = {s: [] for s in states}, {}, {}
            for s in states:  # warm-up, the kernel, the bytes
                set_state(c, s)
                for _ in range(WARM + (a.frames if a.trace_pass else 0)):
                    frame(c)
                stream.synchronize()
                outputs[s] = buf.cpu().numpy().copy()
                info[s] = {"last_kernel": c.last_kernel}
                if has_patterns:
                    info[s]["patterned_objects"] = int(c.get_option(R.STAT_PATTERNED_OBJECTS))
                order.append({"case": case, "state": s, "warm": WARM, "launches": WARM + a.frames})
            if has_patterns and np.array_equal(outputs["none"], outputs["patterned"]):
                raise SystemExit("%s: the patterns change no byte" % case)
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
                       "library": os.path.basename(R.LIB_PATH)}
                row.update(info[s])
                results.append(row)
                cells.append("%s %.1f [%.1f-%.1f]" % (s, row["us"]["median"], row["us"]["min"], row["us"]["max"]))
            if has_patterns:
                m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
                cells.append("patterned/none %.3f" % (m["patterned"] / m["none"]))
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
