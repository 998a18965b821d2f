"""Cost of objects that cast no shadow (rtx_scene_set_shadow_casting).  Two reports.

(1) Kernel resources against the parent's, no GPU needed: --resources PARENT.txt THIS.txt reads two remark files of
`make asm` (hipcc -Rpass-analysis=kernel-resource-usage over csrc/rtx_kernels.hip: build/rtx_kernels.resources.txt, one of a checkout
of the commit before and one of this), compares every field per kernel and writes the comparison to --out.  Kernels are matched by
their demangled name without the argument list.  The plain forms (no FIN, no SPOT) must be the parent's in every field; the rich
forms (FIN of the shade families, SPOT of the two shadow passes) read the flags and may move; none may use scratch.

(2) Frames on one GPU: C2 over a floor (1024 spheres over a plane) at 1920 x 1080, mode RGB_ASCII, shadows on, one frame alone, in ONE
process per library.  Cases `light` (a custom light: the closest hits and rtx_shadow_shade), `eight` (restate.light_set(8):
rtx_lights_shade), `grid` (`eight` under RTX_OPT_SHADOW_GRID: rtx_grid_shadow and rtx_grid_shade) and `mirrors4` (the floor k = 0.5
and a quarter of the spheres k = 0.85 at depth 4 with RTX_OPT_REFLECT_SHADOWS: rtx_chain_shadow and rtx_lights_chain_shadow_shade).
States: `all` (every object casts: the plain forms), `rich` (every object casts, sphere 0 has a finish of its own: the rich forms with
no flags, which is what a parent build runs in that state too) and `half` (the even-numbered spheres cast no shadow: the rich forms
with flags).  A library that lacks the entry points (a build of the commit before, --tree DIR: a checkout with its library built) is
timed in `all` and `rich` alone: run in turns with this build's processes on the same box, its repeats give the run-to-run range this
build's frames are judged against.

The whole frame: the states alternate round by round, so that drift of the machine hits all alike; a round is --frames frames queued
back to back on one stream between two device events.  Per state: median [min-max] over the rounds, RTX_STAT_SHADOW_LONGEST_LIST
and the last kernel's name.

Usage: python tools/cast_cost_gpu.py --resources PARENT.txt THIS.txt --out profiles/rNN_cast_resource_usage.txt
       python tools/cast_cost_gpu.py [--cases light,eight,grid,mirrors4] [--rounds 7] [--frames 40] [--tree DIR] [--out FILE]
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 3
CASES = "light,eight,grid,mirrors4"
W, H = 1920, 1080
FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def read_resources(path):
    """{demangled name without arguments: {field: value}} of one remark file."""
    remark = re.compile(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis=kernel-resource-usage\]")
    kernels, order, cur = {}, [], None
    for line in open(path, errors="replace"):
        m = remark.search(line)
        if not m:
            continue
        key, value = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = value
            order.append(cur)
            kernels[cur] = {}
        elif cur is not None:
            kernels[cur][key] = value
    demangled = subprocess.run(["c++filt"], input="\n".join(order), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for mangled, name in zip(order, demangled):
        name = re.sub(r"^void ", "", name)
        depth, cut = 0, len(name)
        for i, ch in enumerate(name):  # the argument list: the first '(' outside the template brackets
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        out[name[:cut]] = kernels[mangled]
    return out


def is_rich(name):
    """The FIN form of a shade family, the SPOT form of a shadow pass."""
    base = name.split("<")[0]
    return (base.endswith("_shade") and name.endswith(", true>")) or (base in ("rtx::rtx_chain_shadow", "rtx::rtx_grid_shadow") and name.endswith("<true>"))


def cell(k):
    return "%3s / %3s / %s / %s" % (k["VGPRs"], k["TotalSGPRs"], k["Occupancy [waves/SIMD]"], k["ScratchSize [bytes/lane]"])


def compare_resources(parent_path, this_path, out):
    parent, this = read_resources(parent_path), read_resources(this_path)
    names = sorted(this)
    missing, new = sorted(set(parent) - set(this)), sorted(set(this) - set(parent))
    plain = [n for n in names if not is_rich(n) and n in parent]
    rich = [n for n in names if is_rich(n) and n in parent]
    differs = lambda n: any(parent[n].get(f) != this[n].get(f) for f in FIELDS)
    plain_diff, rich_diff = [n for n in plain if differs(n)], [n for n in rich if differs(n)]
    changed = new + plain_diff + rich_diff
    scratch = [n for n in changed if this[n]["ScratchSize [bytes/lane]"] != "0"]
    spills = [n for n in changed if this[n]["VGPRs Spill"] != "0"]
    steps = [n for n in rich_diff if int(this[n]["Occupancy [waves/SIMD]"]) < int(parent[n]["Occupancy [waves/SIMD]"])]
    lines = ["%d kernels in the parent; %d in this change; %d names only in the parent, %d only in this change." % (len(parent), len(this), len(missing), len(new)),
             "Of the %d names without FIN / SPOT %d are identical in every field; %d differ." % (len(plain), len(plain) - len(plain_diff), len(plain_diff)),
             "Of the %d rich forms (FIN of the shade families, SPOT of the two shadow passes) %d are identical in every field; %d differ (below); %d lose an occupancy step."
             % (len(rich), len(rich) - len(rich_diff), len(rich_diff), len(steps)),
             "Kernels of this change that are new or differ and use scratch: %s" % (", ".join(scratch) or "none"),
             "... that spill VGPRs: %s" % (", ".join(spills) or "none"), ""]
    for n in missing:
        lines.append("only in the parent: %s" % n)
    for n in new:
        lines.append("only in this change: %s  %s" % (n, cell(this[n])))
    if plain_diff:
        lines += ["", "Plain forms that differ, parent | this change:  VGPRs / TotalSGPRs / occupancy [waves/SIMD] / scratch [bytes/lane]"]
        lines += ["  %-52s %s | %s" % (n, cell(parent[n]), cell(this[n])) for n in plain_diff]
    lines += ["", "The rich forms that differ, parent | this change:  VGPRs / TotalSGPRs / occupancy [waves/SIMD] / scratch [bytes/lane]; LDS [bytes/block]"]
    for n in rich_diff:
        mark = "   <- one occupancy step" if n in steps else ""
        lines.append("  %-52s %s; %s | %s; %s%s" % (n, cell(parent[n]), parent[n]["LDS Size [bytes/block]"], cell(this[n]), this[n]["LDS Size [bytes/block]"], mark))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 1 if plain_diff or scratch or spills or missing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", nargs=2, default=None, metavar=("PARENT", "THIS"), help="compare two remark files of `make asm`; no GPU needed")
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are timed (default: this one)")
    ap.add_argument("--out", default=None, help="also write the table (and, for the frames, the states as JSON lines) to this file")
    a = ap.parse_args()
    if a.resources:
        return compare_resources(a.resources[0], a.resources[1], a.out)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cast_cost_gpu.py needs a GPU: nothing is timed without one")
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    R = importlib.import_module("raytracing-in-windows-console_amd")
    import restate as RS
    has_cast = hasattr(R.Context, "set_shadow_casting")
    _, sph, pl = R.config_inputs("C2")
    p = R.camera_params(W, H)
    n_obj = len(sph) + len(pl)
    quarter = sorted(int(i) for i in np.random.default_rng(21).choice(len(sph), size=len(sph) // 4, replace=False))
    k = np.zeros(n_obj, dtype=np.float32)
    k[quarter] = 0.85
    k[len(sph)] = 0.5
    half = np.ones(n_obj, dtype=np.uint8)
    half[0:len(sph):2] = 0
    buf = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()
    results = []
    lib = R.LIB_PATH if tree != ROOT else os.path.basename(R.LIB_PATH)
    lines = ["us per frame (RGB_ASCII %d x %d, C2 over a floor, shadows on; light: a custom light; eight: restate.light_set(8); grid: eight under RTX_OPT_SHADOW_GRID; "
             "mirrors4: floor k 0.5, a quarter of the spheres k 0.85, depth 4, RTX_OPT_REFLECT_SHADOWS; states: all cast | all cast and sphere 0 glossy (the rich forms) | "
             "the even-numbered spheres cast no shadow; one frame alone): median [min-max] over %d rounds of %d frames; library %s%s"
             % (W, H, a.rounds, a.frames, lib, "" if has_cast else " (no shadow-casting entry points: no flags)")]

    def frame(c):
        c.render_rows(p, R.RGB_ASCII, 0, H, d_out=buf.data_ptr(), out_row_base=0, stream=stream.cuda_stream)

    for case in a.cases.split(","):
        states = ["all", "rich", "half"] if has_cast else ["all", "rich"]
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            if case == "light":
                c.set_light(R.make_light(pos=(5.0, 40.0, 10.0), diffuse_rgb=(1.0, 0.5, 0.25), diffuse_power=900.0, specular_rgb=(0.2, 1.0, 0.4), specular_power=2100.0))
            else:
                c.set_lights([R.make_light(*RS.light_tuple(l)) for l in RS.light_set(8)])
            c.set_option(R.OPT_SHADOWS, 1)
            if case == "grid":
                c.set_option(R.OPT_SHADOW_GRID, 1)
            if case == "mirrors4":
                c.set_reflectivity(0, k)
                c.set_option(R.OPT_REFLECT_DEPTH, 4)
                c.set_option(R.OPT_REFLECT_SHADOWS, 1)

            def set_state(s):
                c.set_finish(0, [R.make_finish(0.2, 1.0, 1.5, 7) if s == "rich" else R.make_finish()])
                if has_cast:
                    c.set_shadow_casting(0, half if s == "half" else np.ones(n_obj, dtype=np.uint8))

            us, info, outputs = {s: [] for s in states}, {}, {}
            for s in states:  # warm-up, the kernel, the counters, the bytes
                set_state(s)
                for _ in range(WARM):
                    frame(c)
                stream.synchronize()
                c.synchronize()
                outputs[s] = buf.cpu().numpy().copy()
                info[s] = {"last_kernel": c.last_kernel, "shadow_longest_list": int(c.get_option(R.STAT_SHADOW_LONGEST_LIST))}
                if has_cast:
                    info[s]["shadowless_objects"] = int((half == 0).sum()) if s == "half" else 0
            if has_cast and np.array_equal(outputs["all"], outputs["half"]):
                raise SystemExit("%s: the flags change no byte" % case)
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
            m = {s: sorted(us[s])[len(us[s]) // 2] for s in states}
            if has_cast:
                cells.append("half/all %.3f half/rich %.3f" % (m["half"] / m["all"], m["half"] / m["rich"]))
            cells.append(info[states[-1]]["last_kernel"])
            line = "%-9s | %s" % (case, " | ".join(cells))
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
