"""Cost of the several-lights shading launch on one GPU: a table of shade-kernel durations from rocprofv3 --kernel-trace --stats.

For each configuration (C2, C3, C5), mode RGB_ASCII, shadows off and on, one frame alone and 4 in flight on 4 streams:
  one0 .. one7   each of 8 lights spread around the camera alone through rtx_shadow_shade (the one-light kernel, which the
                 several-lights work leaves unchanged: the baseline)
  L1             light 0 through rtx_lights_shade (RTX_OPT_LIGHTS_CHECK 1): what the generality costs
  L2, L4, L8     the first 2, 4 and 8 of those lights through rtx_lights_shade
What an L-light launch is judged against is the L one-light launches of its lights, summed.

One rocprofv3 run per configuration (kernel trace only, no counters), each a child process under its own time limit; a failed
step ends the run.  The child renders the states in a fixed order, warm-up frames first, and writes how many shade launches each
state made; the parent cuts the trace's shade launches (sorted by start time) into the states by those counts.  Per state: the
median, minimum and maximum duration of the shade launch over the measured frames.  --pmc A,B,... collects counters instead (a run
of its own, shadows on, one frame alone) and reports them per launch.

Usage: python tools/lights_gpu.py [--configs C2,C3,C5] [--reps 24] [--out DIR] [--limit 240] [--pmc SQ_INSTS_VALU,SQ_INSTS_LDS,...]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 4
# (name, first light, lights, RTX_OPT_LIGHTS_CHECK): every light alone through the one-light kernel, then the sets
VARIANTS = [("one%d" % i, i, 1, 0) for i in range(8)] + [("L1", 0, 1, 1), ("L2", 0, 2, 0), ("L4", 0, 4, 0), ("L8", 0, 8, 0)]
SETS = [v for v in VARIANTS if v[0].startswith("L")]
COLOURS = [(1.0, 0.5, 0.25), (0.25, 1.0, 0.5), (0.5, 0.25, 1.0), (1.0, 1.0, 0.5), (0.75, 0.5, 1.0), (0.5, 1.0, 1.0), (1.0, 0.75, 0.75), (0.3, 0.6, 0.9)]


def states(pmc):
    for shadows in ((1,) if pmc else (0, 1)):
        for in_flight in ((1,) if pmc else (1, 4)):
            for variant, first, n, check in VARIANTS:
                yield shadows, in_flight, variant, first, n, check


def child(config, reps, manifest, pmc):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    p, sph, pl = R.config_inputs(config)
    W, H = int(p.x), int(p.y)
    cam = np.array(p.cam_pos[:3], dtype=np.float64)
    lights = []
    for i in range(8):
        # alternating near and far sides of a circle around the camera, so that any prefix of the set is spread out
        a = 2.0 * np.pi * ((i * 3) % 8) / 8.0
        pos = cam + np.array([60.0 * np.sin(a), 50.0 + 3.0 * i, 60.0 * np.cos(a)])
        lights.append(R.make_light(pos=tuple(float(v) for v in pos), diffuse_rgb=COLOURS[i], diffuse_power=600.0 + 100.0 * i,
                                   specular_rgb=COLOURS[(i + 3) % 8], specular_power=900.0))
    cams = [R.camera_params(W, H, pos=(0.4 * i, -0.2 * i, 0.1 * i)) for i in range(4)]  # (the configuration's view, nudged)
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.empty(20 * W * H, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    out = []
    with R.Context(W, H) as c:
        c.set_scene(sph, pl)
        for shadows, in_flight, variant, first, n, check in states(pmc):
            c.set_option(R.OPT_SHADOWS, shadows)
            c.set_option(R.OPT_LIGHTS_CHECK, check)
            c.set_lights(lights[first:first + n])
            launches = 0
            for it in range(WARM + (reps if in_flight == 1 else max(1, reps // 4))):
                if in_flight == 1:
                    c.render_rows(cams[0], R.RGB_ASCII, 0, H, d_out=bufs[0].data_ptr(), out_row_base=0)
                    c.synchronize()
                    launches += 1
                else:
                    c.submit_frames(cams, R.RGB_ASCII, [b.data_ptr() for b in bufs], [s.cuda_stream for s in streams])
                    torch.cuda.synchronize()
                    launches += 4
            out.append({"config": config, "shadows": shadows, "in_flight": in_flight, "variant": variant, "lights": n, "launches": launches,
                        "warm": WARM * in_flight, "last_kernel": c.last_kernel, "spheres": int(len(sph)),
                        "longest_list": c.get_option(R.STAT_SHADOW_LONGEST_LIST) if shadows else 0})
    with open(manifest, "w") as f:
        json.dump(out, f)


def shade_rows(trace_dir, pmc):
    """The shade launches of a run in dispatch order: (start, end, name, {counter: value})."""
    pattern = "*counter_collection.csv" if pmc else "*kernel_trace.csv"
    paths = glob.glob(os.path.join(trace_dir, "**", pattern), recursive=True)
    if not paths:
        raise SystemExit("no %s under %s" % (pattern, trace_dir))
    rows = {}
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "rtx_shadow_shade" not in name and "rtx_lights_shade" not in name:
                continue
            row = rows.setdefault(int(r["Dispatch_Id"]), [int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, {}])
            if pmc:
                row[3][r["Counter_Name"]] = row[3].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    # by start time (under counter collection launches are serialised and dispatch order is start order)
    return sorted(rows.values(), key=lambda r: r[0]) if not pmc else [rows[k] for k in sorted(rows)]


def summarise(config, manifest, trace_dir, pmc):
    rows = shade_rows(trace_dir, pmc)
    with open(manifest) as f:
        sts = json.load(f)
    if sum(s["launches"] for s in sts) != len(rows):
        raise SystemExit("%s: the trace holds %d shade launches, the run made %d" % (config, len(rows), sum(s["launches"] for s in sts)))
    at = 0
    for s in sts:
        chunk = rows[at:at + s["launches"]]
        at += s["launches"]
        want = "rtx_shadow_shade" if s["variant"].startswith("one") else "rtx_lights_shade"
        if not all(want in r[2] for r in chunk):
            raise SystemExit("%s %s: launches of another kernel in the state's share of the trace" % (config, s["variant"]))
        chunk = chunk[s["warm"]:]
        if pmc:
            s["counters_per_launch"] = {k: round(sum(r[3][k] for r in chunk) / len(chunk), 1) for k in sorted(chunk[0][3])}
            continue
        d = sorted((r[1] - r[0]) / 1e3 for r in chunk)
        s["shade_us"] = {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "n": len(d)}
    return sts


def table(all_states, pmc):
    """Per configuration and state one line: the one-light launches (light 0; the sum over the first 2, 4, 8 lights: what a caller
    without the several-lights kernels would have to launch), then each set's launch and its share of that sum."""
    by = {(s["config"], s["shadows"], s["in_flight"], s["variant"]): s for s in all_states}
    keys = sorted(set((s["config"], s["shadows"], s["in_flight"]) for s in all_states))
    lines = []
    if pmc:
        for config, shadows, in_flight in keys:
            for name in sorted(by[(config, shadows, in_flight, "L1")]["counters_per_launch"]):
                one = [by[(config, shadows, in_flight, "one%d" % i)]["counters_per_launch"][name] for i in range(8)]
                cells = ["one0 %.4g" % one[0]]
                for v, _, n, _ in SETS:
                    u = by[(config, shadows, in_flight, v)]["counters_per_launch"][name]
                    cells.append("%s %.4g (%.2f of the %d one-light launches)" % (v, u, u / max(sum(one[:n]), 1e-9), n))
                lines.append("%-3s shadows %-3s %-28s | %s" % (config, "on" if shadows else "off", name, " | ".join(cells)))
        return "\n".join(lines)
    lines.append("shade launch, us: median [min-max] over the measured launches; sets also as a share of the sum of their lights' one-light launches")
    for config, shadows, in_flight in keys:
        one = [by[(config, shadows, in_flight, "one%d" % i)]["shade_us"] for i in range(8)]
        cells = ["one0 %.1f [%.1f-%.1f]" % (one[0]["median"], one[0]["min"], one[0]["max"])]
        cells += ["sum of %d: %.1f" % (n, sum(o["median"] for o in one[:n])) for n in (2, 4, 8)]
        for v, _, n, _ in SETS:
            u = by[(config, shadows, in_flight, v)]["shade_us"]
            cells.append("%s %.1f [%.1f-%.1f] = %.2f" % (v, u["median"], u["min"], u["max"], u["median"] / sum(o["median"] for o in one[:n])))
        lines.append("%-3s shadows %-3s in flight %d | %s" % (config, "on" if shadows else "off", in_flight, " | ".join(cells)))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default="lights_prof")
    ap.add_argument("--limit", type=int, default=240, help="seconds each profiled child may take")
    ap.add_argument("--pmc", default=None, help="counters instead of the kernel trace (a run of its own): shadows on, one frame alone")
    ap.add_argument("--child", default=None)
    ap.add_argument("--manifest", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.manifest, a.pmc is not None)
        return 0
    os.makedirs(a.out, exist_ok=True)
    everything = []
    for config in a.configs.split(","):
        trace_dir = os.path.join(a.out, "trace_" + config)
        manifest = os.path.join(a.out, "states_%s.json" % config)
        how = ["--pmc"] + a.pmc.split(",") if a.pmc else ["--kernel-trace", "--stats"]
        cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3"] + how + ["--output-format", "csv", "-d", trace_dir, "--",
               sys.executable, os.path.abspath(__file__), "--child", config, "--manifest", manifest, "--reps", str(a.reps)] + (["--pmc", a.pmc] if a.pmc else [])
        with open(os.path.join(a.out, "run_%s.log" % config), "w") as log:
            rc = subprocess.call(cmd, stdout=log, stderr=subprocess.STDOUT)
        if rc != 0:
            print("%s: the profiled run ended with status %d; nothing more is started" % (config, rc), flush=True)
            return rc
        sts = summarise(config, manifest, trace_dir, a.pmc is not None)
        everything += sts
        for s in sts:
            print(json.dumps(s), flush=True)
    text = table(everything, a.pmc is not None)
    print(text)
    with open(os.path.join(a.out, "table.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
