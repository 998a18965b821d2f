"""Cost of reflection depth on one GPU: per-kernel durations of the mirror path from rocprofv3 --kernel-trace --stats.

For each scene, mode RGB_ASCII, one frame alone and 4 in flight on 4 streams:
  d1       depth 1, the one-bounce kernels (rtx_reflect_hit, rtx_reflect_shade): the baseline, what the parent commit launches
  d1chain  depth 1 through the chain kernels (RTX_OPT_REFLECT_DEPTH_CHECK 1): what the level loop and the general shade cost
  d2 d3 d4 depths 2, 3 and 4 (rtx_reflect_chain, rtx_lights_chain_shade)
Scenes: C2floor (no pixel reaches level 2), C2floor+quarter, C3room, default (the reference's default scene at console size,
400 x 150, with the reflectivities of the exact test).

One rocprofv3 run per scene (kernel trace only, no counters), each a child process under its own time limit; a failed step ends
the run.  The child renders the states in a fixed order, warm-up frames first, and writes how many frames each state made, the
rays per level (RTX_STAT_REFLECT_RAYS) and the longest list; the parent cuts the trace's launches (sorted by start time) into the
states by those counts.  Per state: median [min-max] of the closest-hit launch, the secondary launch and the shade launch over the
measured frames, their sum, and every rtx_ kernel name launched with its launches per frame.

--variants d1 with RTX_LIB naming a build of the parent commit (which has depth 1 only and neither option) measures that build's
launches for an A/B of the default path.

Usage: python tools/reflect_depth_gpu.py [--scenes C2floor,C2floor+quarter,C3room,default] [--variants d1,d1chain,d2,d3,d4] [--reps 24]
                                        [--out DIR] [--limit 240]
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
# (name, RTX_OPT_REFLECT_DEPTH, RTX_OPT_REFLECT_DEPTH_CHECK)
VARIANTS = [("d1", 1, 0), ("d1chain", 1, 1), ("d2", 2, 0), ("d3", 3, 0), ("d4", 4, 0)]
SCENES = ["C2floor", "C2floor+quarter", "C3room", "default"]
ROLES = (("hits", ("rtx_trace",)), ("secondary", ("rtx_reflect_hit", "rtx_reflect_chain")), ("shade", ("rtx_reflect_shade", "rtx_lights_chain_shade")))


def scene_inputs(R, name):
    """(params, spheres, planes, {creation index: k}) of a scene; the k of tests/test_gpu_reflect.py's _scene_k."""
    import numpy as np
    if name == "default":
        return R.camera_params(400, 150), None, None, {0: 0.3, 2: 0.8, 4: 1.0, 5: 0.6}
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


def set_depth(R, c, depth, check):
    try:
        c.set_option(R.OPT_REFLECT_DEPTH, depth)
        c.set_option(R.OPT_REFLECT_DEPTH_CHECK, check)
    except R.RtxError:
        if (depth, check) != (1, 0):  # (a build of the parent commit has depth 1 and no such option)
            raise


def depth_stats(R, c):
    try:
        return [int(c.get_option(R.STAT_REFLECT_RAYS + l)) for l in range(R.MAX_REFLECT_DEPTH)]
    except R.RtxError:
        return [0] * R.MAX_REFLECT_DEPTH


def child(scene, reps, manifest, variants):
    import torch
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    p, sph, pl, ks = scene_inputs(R, scene)
    W, H = int(p.x), int(p.y)
    cams = [p] + [R.camera_params(W, H, pos=(0.4 * i, -0.2 * i, 0.1 * i)) for i in range(1, 4)] if scene != "default" else [p] * 4
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.empty(20 * W * H, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    out = []
    with R.Context(W, H) as c:
        if sph is None:
            c.set_reference_default_scene()
        else:
            c.set_scene(sph, pl)
        for i, k in ks.items():
            c.set_reflectivity(int(i), float(k))
        for in_flight in (1, 4):
            for variant, depth, check in [v for v in VARIANTS if v[0] in variants]:
                set_depth(R, c, depth, check)
                frames = 0
                for it in range(WARM + (reps if in_flight == 1 else max(1, reps // 4))):
                    if in_flight == 1:
                        c.render_rows(cams[0], R.RGB_ASCII, 0, H, d_out=bufs[0].data_ptr(), out_row_base=0)
                        c.synchronize()
                        frames += 1
                    else:
                        c.submit_frames(cams, R.RGB_ASCII, [b.data_ptr() for b in bufs], [s.cuda_stream for s in streams])
                        torch.cuda.synchronize()
                        frames += 4
                # the counters of one frame alone (with frames in flight the one array holds one of theirs)
                c.render_rows(cams[0], R.RGB_ASCII, 0, H, d_out=bufs[0].data_ptr(), out_row_base=0)
                c.synchronize()
                frames += 1
                out.append({"scene": scene, "in_flight": in_flight, "variant": variant, "depth": depth, "frames": frames, "warm": WARM * in_flight,
                            "last_kernel": c.last_kernel, "pixels": W * H,
                            "rays": depth_stats(R, c),
                            "longest_list": int(c.get_option(R.STAT_REFLECT_LONGEST_LIST))})
    with open(manifest, "w") as f:
        json.dump(out, f)


def kernel_rows(trace_dir):
    """Every rtx_ kernel launch of a run by start time: (start, end, name)."""
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows = []
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "rtx_" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    return sorted(rows)


def short(name):
    """rtx::rtx_lights_chain_shade<2, 0>(KArgs, ...) -> rtx_lights_chain_shade<2, 0>"""
    name = name.split("(")[0]
    return name[name.index("rtx_"):].replace("rtx::", "")


def summarise(scene, manifest, trace_dir):
    rows = kernel_rows(trace_dir)
    with open(manifest) as f:
        sts = json.load(f)
    by_role = {role: [r for r in rows if any(short(r[2]).startswith(n) for n in names)] for role, names in ROLES}
    total = sum(s["frames"] for s in sts)
    for role, rr in by_role.items():
        if len(rr) != total:
            raise SystemExit("%s: the trace holds %d %s launches, the run made %d frames" % (scene, len(rr), role, total))
    at = 0
    for s in sts:
        n = s["frames"]
        first = by_role["hits"][at][0]
        end = by_role["hits"][at + n][0] if at + n < total else rows[-1][1] + 1
        names = {}
        for r in rows:
            if first <= r[0] < end:
                names[short(r[2])] = names.get(short(r[2]), 0) + 1
        s["launches_per_frame"] = {k: round(v / n, 3) for k, v in sorted(names.items())}
        s["us"] = {}
        per_frame = None
        for role, rr in by_role.items():
            chunk = rr[at + s["warm"]:at + n - 1]  # (without the warm-up frames and the last frame, rendered alone for the counters)
            d = [(r[1] - r[0]) / 1e3 for r in chunk]
            per_frame = d if per_frame is None else [x + y for x, y in zip(per_frame, d)]
            d.sort()
            s["us"][role] = {"median": round(d[len(d) // 2], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "n": len(d)}
        per_frame.sort()
        s["us"]["sum"] = {"median": round(per_frame[len(per_frame) // 2], 2), "min": round(per_frame[0], 2), "max": round(per_frame[-1], 2)}
        at += n
    return sts


def table(all_states):
    lines = ["kernel durations, us: median [min-max] over the measured frames; `sum` = the three launches of a frame; rays per level and the longest "
             "list from a frame alone"]
    for s in all_states:
        u = s["us"]
        cells = ["%s %.1f [%.1f-%.1f]" % (role, u[role]["median"], u[role]["min"], u[role]["max"]) for role in ("hits", "secondary", "shade", "sum")]
        lines.append("%-16s in flight %d %-8s | %s | rays %s longest %d | rtx_ launches per frame %.2f" % (
            s["scene"], s["in_flight"], s["variant"], " | ".join(cells), s["rays"], s["longest_list"], sum(s["launches_per_frame"].values())))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--variants", default=",".join(v[0] for v in VARIANTS))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default="reflect_depth_prof")
    ap.add_argument("--limit", type=int, default=240, help="seconds each profiled child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--manifest", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.manifest, a.variants.split(","))
        return 0
    os.makedirs(a.out, exist_ok=True)
    everything = []
    for scene in a.scenes.split(","):
        tag = scene.replace("+", "_")
        trace_dir = os.path.join(a.out, "trace_" + tag)
        manifest = os.path.join(a.out, "states_%s.json" % tag)
        cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--",
               sys.executable, os.path.abspath(__file__), "--child", scene, "--manifest", manifest, "--reps", str(a.reps), "--variants", a.variants]
        with open(os.path.join(a.out, "run_%s.log" % tag), "w") as log:
            rc = subprocess.call(cmd, stdout=log, stderr=subprocess.STDOUT)
        if rc != 0:
            print("%s: the profiled run ended with status %d; nothing more is started" % (scene, rc), flush=True)
            return rc
        sts = summarise(scene, manifest, trace_dir)
        everything += sts
        for s in sts:
            print(json.dumps(s), flush=True)
    text = table(everything)
    print(text)
    with open(os.path.join(a.out, "table.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
