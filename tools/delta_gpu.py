"""Cost of delta frames (rtx_update_delta, rtx_delta_words) on one GPU, beside rtx_update on the same frames.

Two frames -- config 2 at 1920 x 1080 (1024 spheres + 1 plane) and the reference's own console frame, 400 x 150 with its start
scene -- in RGB_ASCII under three conditions: at rest, a camera turning 0.003 rad per frame, and a physics step per frame (every
sphere moving, dt = 1/60).

  * default: bytes and milliseconds per call.  Two contexts hold the same scene; per frame one runs rtx_update and the other
    rtx_update_delta with the same camera and the same step, in alternating order (one context cannot do both: an rtx_update in
    between makes the next delta a key frame).  Host clock around the blocking call, rtx_synchronize of both contexts before it;
    median [min-max] over --frames frames after --warm.  --side update times rtx_update alone, and --tree DIR imports the package
    from another checkout: together, in the same job, they give another build's figure for the same frames.
  * --kernels: the launches alone, for a run under `rocprofv3 --kernel-trace`: per condition --frames frames of 1080p words
    (rtx_render_rows), each minimised (rtx_minimize_words: rtx_min_fused<WordSource>) and diffed against the frame before
    (rtx_delta_words: rtx_min_fused<DeltaSource>).
  * --stats DIR: reads the kernel trace rocprofv3 left under DIR and prints the two kernels' times per condition.
No fixed targets: nobody had measured any of this.  The one derivable figure, 0 bytes at rest, is asserted.

Usage: python tools/delta_gpu.py [--frames 60] [--warm 5] [--side both|update] [--tree DIR] [--out FILE]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/delta_gpu.py --kernels
       python tools/delta_gpu.py --stats DIR [--out FILE]
"""
import argparse
import csv
import glob
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONDITIONS = ("rest", "turning 0.003 rad/frame", "physics step/frame")
TURN, DT, YAW0 = 0.003, 1.0 / 60.0, 3.14159274


def med(xs):
    return "%.3f [%.3f-%.3f]" % (statistics.median(xs), min(xs), max(xs))


def build_scene(R, c, name):
    if name == "C2":
        p, sph, pl = R.config_inputs("C2")
        c.set_scene(sph, pl)
        n = len(sph)
    else:
        c.set_reference_default_scene()
        n = 5
    for i in range(n):
        c.set_sphere_motion(i, 1 if i % 2 else -1, 1.0)


def pose(R, W, H, cond, i):
    return R.camera_params(W, H, (0.0, 0.0, 0.0), (0.0, YAW0 + (TURN * i if cond == 1 else 0.0), 0.0))


def timing(R, a, out):
    out("delta frames: ms per blocking call (host clock, both contexts synchronised before it), median [min-max] over %d frames after %d; "
        "bytes per frame: mean [min-max]; RGB_ASCII; library %s" % (a.frames, a.warm, os.path.relpath(R.LIB_PATH, ROOT)))
    for name, W, H in (("C2", 1920, 1080), ("console (reference start scene)", 400, 150)):
        for cond, label in enumerate(CONDITIONS):
            with R.Context(W, H) as cu, R.Context(W, H) as cd:
                build_scene(R, cu, name.split()[0])
                build_scene(R, cd, name.split()[0])
                t_u, t_d, b_u, b_d, kinds = [], [], [], [], []
                cells = runs = 0
                for i in range(a.warm + a.frames):
                    p = pose(R, W, H, cond, i)
                    phys = cond == 2

                    def run_update():
                        cu.synchronize(); cd.synchronize()
                        t0 = time.perf_counter()
                        s = cu.update(p, R.RGB_ASCII, DT, phys)
                        return (time.perf_counter() - t0) * 1e3, len(s)

                    def run_delta():
                        cu.synchronize(); cd.synchronize()
                        t0 = time.perf_counter()
                        s, kind = cd.update_delta(p, R.RGB_ASCII, DT, phys)
                        return (time.perf_counter() - t0) * 1e3, len(s), kind

                    if a.side == "update":
                        u, d = run_update(), (0.0, 0, 1)
                    elif i % 2:
                        u = run_update(); d = run_delta()
                    else:
                        d = run_delta(); u = run_update()
                    if i >= a.warm:
                        t_u.append(u[0]); b_u.append(u[1]); t_d.append(d[0]); b_d.append(d[1]); kinds.append(d[2])
                if a.side != "update":
                    cells, runs = cd.get_option(R.STAT_DELTA_CELLS), cd.get_option(R.STAT_DELTA_RUNS)
                    assert all(k == R.DELTA_DIFF for k in kinds)
                    assert cond != 0 or max(b_d) == 0, "a frame at rest must give 0 bytes"
                out("%-32s %4dx%-4d %-24s rtx_update %s ms, %9.0f [%d-%d] B" %
                    (name, W, H, label, med(t_u), statistics.mean(b_u), min(b_u), max(b_u)))
                if a.side != "update":
                    out("%-32s %4dx%-4d %-24s rtx_update_delta %s ms, %9.0f [%d-%d] B (%.3f of rtx_update's); last frame %d cells in %d runs of %d" %
                        ("", W, H, "", med(t_d), statistics.mean(b_d), min(b_d), max(b_d), statistics.mean(b_d) / max(1.0, statistics.mean(b_u)),
                         cells, runs, (W - 1) * H))


def kernels(R, a):
    import torch
    W, H = 1920, 1080
    n = W * H
    with R.Context(W, H) as c:
        build_scene(R, c, "C2")
        words = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        cap = R.delta_bound(R.RGB_ASCII, W, H)
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for cond in range(3):
            for i in range(a.warm + a.frames + 1):
                if cond == 2:
                    c.update_objects(DT)
                cur, prev = words[i % 2], words[(i + 1) % 2]
                c.render_rows(pose(R, W, H, cond, i), R.RGB_ASCII, 0, H, d_out=cur.data_ptr(), flags=R.RENDER_COMPACT)
                c.synchronize()
                if i == 0:
                    continue  # (the first frame of a condition has no frame before it)
                nk = c.minimize_words(R.RGB_ASCII, W, H, cur.data_ptr(), out.data_ptr())
                nd = c.delta_words(R.RGB_ASCII, W, H, cur.data_ptr(), prev.data_ptr(), out.data_ptr(), cap)
                if i == a.warm + a.frames:
                    print("%s: key frame %d B, delta %d B, %d cells in %d runs" %
                          (CONDITIONS[cond], nk, nd, c.get_option(R.STAT_DELTA_CELLS), c.get_option(R.STAT_DELTA_RUNS)), flush=True)
        assert c.get_option(R.STAT_MINIMIZE_FALLBACKS) == 0


def stats(a, out):
    rows = []
    for path in glob.glob(os.path.join(a.stats, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = a.warm + a.frames
    out("kernel times at 1920x1080 RGB_ASCII, config 2 (rocprofv3 --kernel-trace; us, median [min-max] over %d launches per condition after %d)" %
        (a.frames, a.warm))
    for label, key in (("rtx_min_fused<WordSource> (rtx_minimize_words: the key frame)", "WordSource"),
                       ("rtx_min_fused<DeltaSource> (rtx_delta_words)", "DeltaSource")):
        mine = [(e - s) / 1e3 for s, e, k in rows if "rtx_min_fused" in k and key in k]
        if len(mine) != 3 * per:
            raise SystemExit("%s: %d launches in the trace, expected %d" % (label, len(mine), 3 * per))
        for cond, name in enumerate(CONDITIONS):
            out("%-66s %-24s %s" % (label, name, med(mine[cond * per + a.warm:(cond + 1) * per])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--side", choices=("both", "update"), default="both")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported (default: this one)")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats", default=None, help="directory rocprofv3 wrote the --kernels run's trace under")
    ap.add_argument("--out", default=None, help="also append the table to this file")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.stats:
        stats(a, out)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("delta_gpu.py needs a GPU: nothing is timed without one")
        sys.path.insert(0, os.path.abspath(a.tree))
        R = importlib.import_module("raytracing-in-windows-console_amd")
        if a.kernels:
            kernels(R, a)
        else:
            timing(R, a, out)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
