"""Cost of delta frames of half-block streams (rtx_update_half_delta) on one GPU, beside rtx_update_half of the same frames.

Config 2's scene (1024 spheres + 1 plane, every sphere moving) in RGB_PIXEL as a 160 x 50 and as a 1920 x 540 console, under three
motions: at rest, a physics step per frame (dt = 1/60), and a camera turning 0.003 rad per frame.

Milliseconds per blocking call and bytes per call.  Every side has a context of its own with the same scene (one context cannot do
both: an rtx_update_half in between makes the next delta a key frame) and walks through the same frames: frame i has pose i and,
under physics, i steps behind it.  Host clock around a batch of --frames calls, the context synchronised before it; --rounds rounds,
the sides alternating within a round and taking every place in turn; per side the median of the batch means with the lowest and the
highest, and the mean bytes per call.  Sides: rtx_update_half_delta, this build's rtx_update_half and rtx_update (W x H), and -- with
--parent DIR, a checkout of the parent commit with its library built -- the parent's rtx_update_half and rtx_update, run by a child
process (one package per process) that takes its turn in every round: that shows whether the existing calls moved.
No threshold is set in advance: nobody had timed this.  The one derivable figure, 0 bytes at rest, is asserted, and so is that no
fused launch fell back to the chain and that every timed delta call returned RTX_DELTA_DIFF.

Usage: python tools/half_delta_cost_gpu.py [--rounds 5] [--frames 30] [--warm 8] [--parent DIR] [--out FILE]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((160, 50), (1920, 540))
MOTIONS = ("rest", "physics step/frame", "turning 0.003 rad/frame")
MODE = 3  # RTX_RGB_PIXEL
TURN, DT, YAW0 = 0.003, 1.0 / 60.0, 3.14159274


def med(xs):
    return "%.4f [%.4f-%.4f]" % (statistics.median(xs), min(xs), max(xs))


def load(tree):
    sys.path.insert(0, os.path.abspath(tree))
    return importlib.import_module("raytracing-in-windows-console_amd")


class Side:
    """One call on a context of its own, walking through the frames of one motion."""

    def __init__(self, R, W, H, motion, what):
        self.R, self.W, self.H, self.motion, self.what = R, W, H, motion, what
        self.c = R.Context(W, 2 * H)
        _, sph, pl = R.config_inputs("C2")
        self.c.set_scene(sph, pl)
        for i in range(len(sph)):
            self.c.set_sphere_motion(i, 1 if i % 2 else -1, 1.0)
        self.i = 0
        self.kinds = set()

    def call(self):
        R, c = self.R, self.c
        p = R.camera_params(self.W, self.H, (0.0, 0.0, 0.0), (0.0, YAW0 + (TURN * self.i if self.motion == 2 else 0.0), 0.0))
        phys = self.motion == 1
        self.i += 1
        if self.what == "half_delta":
            s, kind = c.update_half_delta(p, MODE, DT, phys)
            self.kinds.add(kind)
            return len(s)
        if self.what == "half":
            return len(c.update_half(p, MODE, DT, phys))
        return len(c.update(p, MODE, DT, phys))

    def batch(self, frames):
        """Mean milliseconds and mean bytes per call over one batch."""
        self.c.synchronize()
        total = 0
        t0 = time.perf_counter()
        for _ in range(frames):
            total += self.call()
        return (time.perf_counter() - t0) * 1e3 / frames, total / frames

    def close(self):
        self.c.close()


def serve(a):
    """The child of --parent: this checkout's rtx_update_half and rtx_update, one batch per line read from stdin."""
    R = load(a.tree)
    sides = {}
    print("ready", flush=True)
    for line in sys.stdin:
        W, H, motion, what = line.split()
        key = (int(W), int(H), int(motion), what)
        if what == "close":
            for k in [k for k in sides if k[:3] == key[:3]]:
                sides.pop(k).close()
            print("closed", flush=True)
            continue
        if key not in sides:
            sides[key] = Side(R, key[0], key[1], key[2], what)
            for _ in range(a.warm):
                sides[key].call()
        ms, n = sides[key].batch(a.frames)
        print("%.6f %.1f" % (ms, n), flush=True)


def timing(R, a, out):
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", "--tree", a.parent, "--frames", str(a.frames), "--warm", str(a.warm)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        if child.stdout.readline().strip() != "ready":
            raise SystemExit("the parent build's child process did not start")

    def ask(W, H, motion, what):
        child.stdin.write("%d %d %d %s\n" % (W, H, motion, what))
        child.stdin.flush()
        return child.stdout.readline().split()

    out("delta frames of half-block streams: ms per blocking call (host clock, context synchronised before each batch), median [min-max] of the means "
        "of %d batches of %d calls after %d warm-up calls; bytes: mean per call over all batches; RGB_PIXEL, config 2's scene, every sphere moving under "
        "physics; library %s" % (a.rounds, a.frames, a.warm, os.path.relpath(R.LIB_PATH, ROOT)))
    for W, H in SHAPES:
        for motion, label in enumerate(MOTIONS):
            names = ["half_delta", "half", "update"]
            sides = [Side(R, W, H, motion, n) for n in names]
            for s in sides:
                for _ in range(a.warm):
                    s.call()
            sides[0].kinds.clear()  # (the warm-up's first call was the key frame)
            labels = ["rtx_update_half_delta", "rtx_update_half", "rtx_update %dx%d" % (W, H)]
            if child:
                names += ["parent half", "parent update"]
                labels += ["rtx_update_half, parent", "rtx_update %dx%d, parent" % (W, H)]
            ms = [[] for _ in names]
            nbytes = [[] for _ in names]
            for r in range(a.rounds):
                order = list(range(len(names)))
                order = order[r % len(order):] + order[:r % len(order)]
                for k in order:
                    if k < 3:
                        t, n = sides[k].batch(a.frames)
                    else:
                        t, n = (float(v) for v in ask(W, H, motion, names[k].split()[1]))
                    ms[k].append(t)
                    nbytes[k].append(n)
            out("%4dx%-3d cells, %s" % (W, H, label))
            for k, lab in enumerate(labels):
                out("    %-28s %s ms, %11.0f B" % (lab, med(ms[k]), statistics.mean(nbytes[k])))
            out("    %-28s half_delta / half = %.3f in time, %.3f in bytes; last frame %d cells in %d runs of %d; bound %d B" %
                ("", statistics.median(ms[0]) / statistics.median(ms[1]), statistics.mean(nbytes[0]) / max(1.0, statistics.mean(nbytes[1])),
                 sides[0].c.get_option(R.STAT_DELTA_CELLS), sides[0].c.get_option(R.STAT_DELTA_RUNS), (W - 1) * H, R.half_delta_bound(MODE, W, H)))
            assert sides[0].kinds == {R.DELTA_DIFF}, "a timed call gave a key frame"
            assert motion != 0 or max(nbytes[0]) == 0, "a frame at rest must give 0 bytes"
            for s in sides:
                assert s.c.get_option(R.STAT_MINIMIZE_FALLBACKS) == 0
                s.close()
            if child:
                ask(W, H, motion, "close")
    if child:
        child.stdin.close()
        child.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its rtx_update_half and rtx_update are timed in the same rounds")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported (default: this one)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also append the table to this file")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("half_delta_cost_gpu.py needs a GPU: nothing is timed without one")
    if a.serve:
        serve(a)
        return
    timing(load(a.tree), a, out)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
