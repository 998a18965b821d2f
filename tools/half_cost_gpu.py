"""Cost of half-block frames (rtx_update_half, rtx_half_words) on one GPU, beside rtx_update of the same rays.

Config 2's scene (1024 spheres + 1 plane) in RGB_PIXEL with the camera at rest, as a 160 x 50 and as a 1920 x 540 console: the
half-block frame traces W x 2H pixels, so the frame it is set beside is rtx_update of W x 2H.

  * default: milliseconds per blocking call and bytes per frame.  Host clock around the call, the context synchronised before it;
    --rounds rounds, each one batch of --frames calls per side after --warm warm-up calls per shape, the sides alternating within
    a round; per side the median of the batch means, with the lowest and highest batch mean.  Sides: rtx_update_half, this build's
    rtx_update at W x 2H and at W x H, and -- with --parent DIR, a checkout of the parent commit with its library built -- the
    parent's rtx_update at W x 2H, run by a child process (one package per process) that takes its turn in every round.
  * --kernels: the launches alone, for a run under `rocprofv3 --kernel-trace`: per shape the sample frame's words traced once
    (rtx_render_rows), then --frames times rtx_minimize_words of the W x 2H frame (rtx_min_fused<WordSource>) and rtx_half_words of
    the W x H console (rtx_min_fused<HalfSource>) over the same words.
  * --stats DIR: reads the kernel trace rocprofv3 left under DIR and prints the two kernels' times and their ratio.
No threshold is set in advance: nobody had timed the pass.  A fused launch that fell back to the chain would be another workload, so
RTX_STAT_MINIMIZE_FALLBACKS == 0 is asserted.

Usage: python tools/half_cost_gpu.py [--rounds 7] [--frames 40] [--warm 10] [--parent DIR] [--out FILE]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/half_cost_gpu.py --kernels
       python tools/half_cost_gpu.py --stats DIR [--out FILE]
"""
import argparse
import csv
import glob
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((160, 50), (1920, 540))
MODE = 3  # RTX_RGB_PIXEL


def med(xs):
    return "%.4f [%.4f-%.4f]" % (statistics.median(xs), min(xs), max(xs))


def load(tree):
    sys.path.insert(0, os.path.abspath(tree))
    return importlib.import_module("raytracing-in-windows-console_amd")


def scene(R, c):
    _, sph, pl = R.config_inputs("C2")
    c.set_scene(sph, pl)


def batch(c, call, frames):
    """Mean milliseconds per call over one batch, and the last call's bytes.  One call before the clock starts: the side before this
    one may have left the context planned for another frame size."""
    call()
    c.synchronize()
    n = 0
    t0 = time.perf_counter()
    for _ in range(frames):
        n = len(call())
    return (time.perf_counter() - t0) * 1e3 / frames, n


def serve(a):
    """The child of --parent: this checkout's rtx_update at W x 2H, one batch per line read from stdin."""
    R = load(a.tree)
    ctxs = {}
    for W, H in SHAPES:
        c = R.Context(W, 2 * H)
        scene(R, c)
        p = R.camera_params(W, 2 * H)
        for _ in range(a.warm):
            c.update(p, MODE)
        ctxs[(W, H)] = (c, p)
    print("ready", flush=True)
    for line in sys.stdin:
        W, H = (int(v) for v in line.split())
        c, p = ctxs[(W, H)]
        ms, n = batch(c, lambda: c.update(p, MODE), a.frames)
        print("%.6f %d" % (ms, n), flush=True)


def timing(R, a, out):
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", "--tree", a.parent, "--frames", str(a.frames), "--warm", str(a.warm)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        if child.stdout.readline().strip() != "ready":
            raise SystemExit("the parent build's child process did not start")
    out("half-block frames: ms per blocking call (host clock, context synchronised before each batch), median [min-max] of the means of %d batches "
        "of %d calls after %d warm-up calls; RGB_PIXEL, config 2's scene, camera at rest; library %s" %
        (a.rounds, a.frames, a.warm, os.path.relpath(R.LIB_PATH, ROOT)))
    for W, H in SHAPES:
        with R.Context(W, 2 * H) as c:
            scene(R, c)
            p, p2 = R.camera_params(W, H), R.camera_params(W, 2 * H)
            p_half = R.Params.from_buffer_copy(bytes(p2))  # W x 2H's projection, so that the rays are those of rtx_update at W x 2H
            p_half.y = H
            sides = [("rtx_update_half %dx%d cells" % (W, H), lambda: c.update_half(p_half, MODE)),
                     ("rtx_update %dx%d" % (W, 2 * H), lambda: c.update(p2, MODE)),
                     ("rtx_update %dx%d" % (W, H), lambda: c.update(p, MODE))]
            for _, call in sides:
                for _ in range(a.warm):
                    call()
            ms = [[] for _ in sides]
            nbytes = [0] * len(sides)
            parent_ms, parent_bytes = [], 0
            for r in range(a.rounds):
                order = list(range(len(sides)))
                order = order[r % len(order):] + order[:r % len(order)]  # (every side takes every place in turn)
                for k in order:
                    t, nbytes[k] = batch(c, sides[k][1], a.frames)
                    ms[k].append(t)
                if child:
                    child.stdin.write("%d %d\n" % (W, H))
                    child.stdin.flush()
                    t, n = child.stdout.readline().split()
                    parent_ms.append(float(t))
                    parent_bytes = int(n)
            for k, (label, _) in enumerate(sides):
                out("%-34s %s ms, %9d B" % (label, med(ms[k]), nbytes[k]))
            if child:
                out("%-34s %s ms, %9d B   (the parent commit's build, same rounds)" % ("rtx_update %dx%d, parent" % (W, 2 * H), med(parent_ms), parent_bytes))
                assert parent_bytes == nbytes[1], "the parent's stream for the same frame has another length"
            out("%-34s half / update(W x 2H) = %.3f in time, %.3f in bytes; bound %d B" %
                ("", statistics.median(ms[0]) / statistics.median(ms[1]), nbytes[0] / max(1, nbytes[1]), R.half_bound(MODE, W, H)))
            assert c.get_option(R.STAT_MINIMIZE_FALLBACKS) == 0
    if child:
        child.stdin.close()
        child.wait(timeout=60)


def kernels(R, a):
    import torch
    for W, H in SHAPES:
        with R.Context(W, 2 * H) as c:
            scene(R, c)
            words = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
            cap = max(R.half_bound(MODE, W, H), 20 * W * 2 * H)
            out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c.render_rows(R.camera_params(W, 2 * H), MODE, 0, 2 * H, d_out=words.data_ptr(), flags=R.RENDER_COMPACT)
            c.synchronize()
            for _ in range(a.warm + a.frames):
                nk = c.minimize_words(MODE, W, 2 * H, words.data_ptr(), out.data_ptr())
                nh = c.half_words(MODE, W, H, words.data_ptr(), out.data_ptr(), cap)
            print("%dx%d cells: rtx_minimize_words of %dx%d %d B, rtx_half_words %d B" % (W, H, W, 2 * H, nk, nh), flush=True)
            assert c.get_option(R.STAT_MINIMIZE_FALLBACKS) == 0


def stats(a, out):
    rows = []
    for path in glob.glob(os.path.join(a.stats, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = a.warm + a.frames
    out("kernel times, RGB_PIXEL, config 2's scene (rocprofv3 --kernel-trace; us, median [min-max] over %d launches per shape after %d)" % (a.frames, a.warm))
    got = {}
    for label, key in (("rtx_min_fused<WordSource<RGB_PIXEL>> over W x 2H (rtx_minimize_words)", "WordSource"),
                       ("rtx_min_fused<HalfSource<true>> over W x H cells (rtx_half_words)", "HalfSource")):
        mine = [(e - s) / 1e3 for s, e, k in rows if "rtx_min_fused" in k and key in k]
        if len(mine) != len(SHAPES) * per:
            raise SystemExit("%s: %d launches in the trace, expected %d" % (label, len(mine), len(SHAPES) * per))
        for i, (W, H) in enumerate(SHAPES):
            t = mine[i * per + a.warm:(i + 1) * per]
            got[(key, i)] = statistics.median(t)
            out("%-72s %4dx%-3d cells  %s" % (label, W, H, med(t)))
    for i, (W, H) in enumerate(SHAPES):
        out("%4dx%-3d cells: the half pass takes %.2f x the word-form Minimize of the W x 2H frame" % (W, H, got[("HalfSource", i)] / got[("WordSource", i)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its rtx_update is timed in the same rounds")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported (default: this one)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
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
            raise SystemExit("half_cost_gpu.py needs a GPU: nothing is timed without one")
        if a.serve:
            serve(a)
            return
        R = load(a.tree)
        if a.kernels:
            kernels(R, a)
        else:
            timing(R, a, out)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
