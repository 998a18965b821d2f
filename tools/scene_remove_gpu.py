"""Cost of removing scene objects in place (rtx_scene_remove_objects, rtx_scene_remove_marked_device) on one GPU, beside the only
route there was before: rtx_scene_clear + rtx_scene_add_spheres of the survivors + the first render after them.

  * us per call for n = 1024 spheres (config 2's scene) and n = 100 000 (a synthetic scene of that size), removing one sphere and
    removing every second sphere, host form and device form: the median of --calls calls after --warm warm-up calls.  A removal
    cannot be repeated on the same scene, so every repetition first rebuilds the scene and renders it once (untimed: the sorted
    copy, the cell lists and the dispatch order exist, as in a running application), then rtx_synchronize, then
    time.perf_counter around the call -- it blocks, so host time is the figure -- and around the first render after it.
  * the rebuild route for the same result, timed the same way: scene_clear + add_spheres of the survivors (+ the plane) + the first
    render + synchronize.  It uses only calls that predate the removal, and it is given the survivors' rows for free: an
    application whose spheres had moved on the device would first have to read every one back.
No fixed targets: nobody had measured any of this.

Usage: python tools/scene_remove_gpu.py [--calls 30] [--warm 3] [--out FILE]
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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_remove_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    R = importlib.import_module("raytracing-in-windows-console_amd")
    lines = ["removing objects in place: us, median [min-max] after warm-up calls, host clock, rtx_synchronize before each; the scene is rebuilt and "
             "rendered once (untimed) before every call; library %s" % os.path.basename(R.LIB_PATH)]
    p, sph2, pl2 = R.config_inputs("C2")
    W, H = int(p.x), int(p.y)
    big, _ = R.synth_scene(9, 100000, 0, p.element1, p.element2)

    def clock(fn, c):
        c.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    def frame(c):
        c.render(p, R.RGB_ASCII)
        c.synchronize()

    for name, sph, pl in (("C2, n = 1024", sph2, pl2), ("n = 100000", big, np.zeros((0, 11), dtype=np.float32))):
        n = len(sph)
        reps, warm = (a.calls, a.warm) if n <= 4096 else (max(3, a.calls // 5), 1)   # (100 000 push_backs a rebuild: fewer of them)
        with R.Context(W, H) as c:
            for what, removed in (("1 sphere", np.array([n // 2], dtype=np.uint32)), ("every second sphere", np.arange(1, n, 2, dtype=np.uint32))):
                keep = np.ones(n, dtype=bool)
                keep[removed] = False
                left = np.ascontiguousarray(sph[keep])
                marks = np.zeros(n + len(pl), dtype=np.uint8)
                marks[removed] = 1
                d_marks = torch.from_numpy(marks).cuda()
                torch.cuda.synchronize()
                t = {"host": [], "device": [], "host, first render": [], "device, first render": [], "rebuild": [], "render": []}
                for k in range(warm + reps):
                    row = {}
                    for form in ("host", "device"):
                        c.set_scene(sph, pl)
                        frame(c)
                        if form == "host":
                            row[form] = clock(lambda: c.remove_objects(removed), c)
                        else:
                            row[form] = clock(lambda: c.remove_marked_device(d_marks.data_ptr()), c)
                        assert c.object_count == n + len(pl) - len(removed)
                        row[form + ", first render"] = clock(lambda: frame(c), c)
                        row["render"] = clock(lambda: frame(c), c)
                    c.set_scene(sph, pl)
                    frame(c)

                    def rebuild():
                        c.set_scene(left, pl)
                        frame(c)

                    row["rebuild"] = clock(rebuild, c)
                    if k >= warm:
                        for key, v in row.items():
                            t[key].append(v)
                lines.append("%-14s removing %-20s rtx_scene_remove_objects %s + first render %s   rtx_scene_remove_marked_device %s + first render %s" % (
                    name, what + ":", med(t["host"]), med(t["host, first render"]), med(t["device"]), med(t["device, first render"])))
                lines.append("%-14s          %-20s scene_clear + add_spheres of the survivors + first render %s   (%d calls each; a render of the "
                             "unchanged scene, same clock %s)" % (name, "", med(t["rebuild"]), reps, med(t["render"])))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
