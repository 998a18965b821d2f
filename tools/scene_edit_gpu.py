"""Cost of editing scene objects in place (rtx_scene_set_spheres, rtx_scene_set_spheres_device) on one GPU, beside the only route
there was before: rtx_scene_clear + rtx_scene_add_spheres + the first render after them.

  * us per call of the host form and of the device form for n = 1024 spheres (config 2's scene, a whole-scene edit) and n = 100 000
    (a synthetic scene of that size): the median of --calls calls after --warm warm-up calls, rtx_synchronize before each timed
    call, time.perf_counter around it -- the call blocks, so host time is the figure.  Every call moves every centre by up to 0.05.
  * the rebuild route for the same two scenes: scene_clear + add_spheres (+ the plane) + one render + synchronize, timed the same
    way, and the render of an unchanged scene beside it.
  * config 2's frame time over --frames frames one at a time (RGB_ASCII, the context's own buffer, synchronised per frame), without
    and with a whole-scene edit of 0.05 between the frames; the edit's own time is inside the second figure.
No fixed targets: nobody had measured any of this.

Usage: python tools/scene_edit_gpu.py [--calls 50] [--warm 5] [--frames 64] [--out FILE]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(xs):
    return "%.1f [%.1f-%.1f]" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_edit_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    lines = ["editing spheres in place: us, median [min-max] of %d calls after %d warm-up calls, host clock, rtx_synchronize before each; library %s" % (
        a.calls, a.warm, os.path.basename(R.LIB_PATH))]
    p, sph2, pl2 = R.config_inputs("C2")
    W, H = int(p.x), int(p.y)
    big, _ = R.synth_scene(9, 100000, 0, p.element1, p.element2)
    rng = np.random.default_rng(1)

    def jitter(rows):
        out = rows.copy()
        out[:, 0:3] += rng.uniform(-0.05 / 3 ** 0.5, 0.05 / 3 ** 0.5, (len(rows), 3)).astype(np.float32)
        return out

    def timed(fn, c, reps, warm):
        out = []
        for k in range(warm + reps):
            c.synchronize()
            t0 = time.perf_counter()
            fn(k)
            t1 = time.perf_counter()
            if k >= warm:
                out.append((t1 - t0) * 1e6)
        return out

    for name, sph, pl in (("C2, n = 1024", sph2, pl2), ("n = 100000", big, np.zeros((0, 11), dtype=np.float32))):
        n = len(sph)
        with R.Context(W, H) as c:
            c.set_scene(sph, pl)
            c.render(p, R.RGB_ASCII)
            c.synchronize()
            variants = [jitter(sph) for _ in range(4)]
            d_variants = [torch.from_numpy(v).cuda() for v in variants]
            torch.cuda.synchronize()
            host = timed(lambda k: c.set_spheres(0, variants[k % 4]), c, a.calls, a.warm)
            dev = timed(lambda k: c.set_spheres_device(0, n, d_variants[k % 4].data_ptr()), c, a.calls, a.warm)
            move = np.array([c.get_option(R.STAT_SCENE_EDIT_MOVE)], dtype=np.uint32).view(np.float32)[0]

            def rebuild(k):
                c.set_scene(variants[k % 4], pl)
                c.render(p, R.RGB_ASCII)
                c.synchronize()

            def frame(k):
                c.render(p, R.RGB_ASCII)
                c.synchronize()

            reps = a.calls if n <= 4096 else max(3, a.calls // 10)   # (100 000 push_backs a call: fewer of them)
            rb = timed(rebuild, c, reps, 2)
            fr = timed(frame, c, a.calls, a.warm)
            lines.append("%-14s rtx_scene_set_spheres %s   rtx_scene_set_spheres_device %s   (last RTX_STAT_SCENE_EDIT_MOVE %.6f)" % (name, med(host), med(dev), move))
            lines.append("%-14s scene_clear + add_spheres + first render %s (%d calls)   a render of the unchanged scene, same clock %s" % (name, med(rb), reps, med(fr)))
    # config 2 frame by frame, with and without an edit of the whole scene between the frames
    with R.Context(W, H) as c:
        c.set_scene(sph2, pl2)
        for _ in range(96):   # (past the first 64 frames of the tile grid, in which the dispatch order is re-derived every fourth frame)
            c.render(p, R.RGB_ASCII)
            c.synchronize()
        variants = [jitter(sph2) for _ in range(4)]
        for label, edit in (("no edit", False), ("an edit of all 1024 spheres by up to 0.05 before every frame", True), ("no edit, again", False)):
            s0 = {k: c.get_option(v) for k, v in (("builds", R.STAT_CELL_BUILDS), ("hits", R.STAT_CELL_HITS), ("per_frame", R.STAT_CELL_PER_FRAME),
                                                  ("grid", R.STAT_QUERY_GRID_BUILDS), ("order passes", R.STAT_ORDER_PASSES))}
            c.synchronize()
            t0 = time.perf_counter()
            for f in range(a.frames):
                if edit:
                    c.set_spheres(0, variants[f % 4])
                c.render(p, R.RGB_ASCII)
                c.synchronize()
            t1 = time.perf_counter()
            s1 = {k: c.get_option(v) for k, v in (("builds", R.STAT_CELL_BUILDS), ("hits", R.STAT_CELL_HITS), ("per_frame", R.STAT_CELL_PER_FRAME),
                                                  ("grid", R.STAT_QUERY_GRID_BUILDS), ("order passes", R.STAT_ORDER_PASSES))}
            lines.append("C2 over %d frames, one at a time, %s: %.1f us per frame (kernel %s; counters over the run: %s)" % (
                a.frames, label, (t1 - t0) * 1e6 / a.frames, c.last_kernel, ", ".join("%s +%d" % (k, s1[k] - s0[k]) for k in s0)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
