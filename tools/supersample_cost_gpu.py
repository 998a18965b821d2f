"""Cost of supersampling (RTX_OPT_SUPERSAMPLE) on one GPU, in ONE process: for config 2's scene at 1920 x 1080 and at 400 x 150 cells and
S = 2, 3, 4 three things, one frame at a time in RGB_ASCII records:

  whole   the supersampled rtx_render_rows of the W x H frame (the sample frame's launches and the fold);
  plain   the render of the S W x S H frame in values form with S = 1: the part that is not new;
  fold    the fold kernel alone against a device-to-device hipMemcpyAsync of the same number of input bytes, timed together by
          tools/microbench/resolve_vs_copy (built beforehand; its line is copied into the table).

whole and plain alternate round by round, so that drift of the machine hits both alike.  A round is --frames frames queued back to
back on one stream between two device events (a frame's launches depend on one another, so back to back is one frame at a time; the
events take the enqueue out of the figure).  Per state: median [min-max] over the rounds; the spread is the state's own run-to-run
spread.  Before anything is timed the supersampled values are compared bit for bit with the numpy fold of the plain frame
(tests/restate_supersample.py).  No ratio is asserted: the file says what was measured.

Usage: python tools/supersample_cost_gpu.py [--sizes 1920x1080,400x150] [--samples 2,3,4] [--rounds 7] [--frames 40]
                                            [--out profiles/r18_supersample_cost.txt]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICROBENCH = os.path.join(ROOT, "tools", "microbench", "resolve_vs_copy")
WARM = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,400x150")
    ap.add_argument("--samples", default="2,3,4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_supersample_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("supersample_cost_gpu.py needs a GPU: nothing is timed without one")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    R = importlib.import_module("raytracing-in-windows-console_amd")
    import restate_supersample as SS
    import restate as RS
    _, sph, pl = R.config_inputs("C2")
    mode = R.RGB_ASCII
    lines = ["supersampling, config 2's scene, RGB_ASCII records, one frame alone: us per frame, median [min-max] over %d rounds of up to %d frames; "
             "library %s" % (a.rounds, a.frames, os.path.basename(R.LIB_PATH))]
    results = []
    stream = torch.cuda.Stream()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for S in (int(v) for v in a.samples.split(",")):
            p = R.camera_params(W, H)
            ps = SS.sample_params(p, S)
            out = torch.empty(32 * W * H, dtype=torch.uint8, device="cuda")
            big = torch.empty(32 * S * S * W * H, dtype=torch.uint8, device="cuda")
            with R.Context(W, H) as c:
                c.set_scene(sph, pl)

                def frame(state, flags=0):
                    if state == "whole":
                        c.render_rows(p, mode, 0, H, d_out=out.data_ptr(), out_row_base=0, stream=stream.cuda_stream, flags=flags)
                    else:
                        c.render_rows(ps, mode, 0, S * H, d_out=big.data_ptr(), out_row_base=0, stream=stream.cuda_stream, flags=R.RENDER_VALUES)

                def set_state(state):
                    c.set_option(R.OPT_SUPERSAMPLE, S if state == "whole" else 1)

                # the frames agree with the rule before anything is timed
                set_state("plain")
                frame("plain")
                stream.synchronize()
                want = SS.fold(big.cpu().numpy().view(np.float32), W, H, S, float(p.cam_far))
                set_state("whole")
                frame("whole", R.RENDER_VALUES)
                stream.synchronize()
                if not RS.same_floats(out.cpu().numpy().view(np.float32).reshape(-1, 8), want).all():
                    raise SystemExit("%s S = %d: the supersampled values are not the fold of the plain frame" % (size, S))
                kernels, frames, us = {}, {}, {"whole": [], "plain": []}
                for state in ("whole", "plain"):
                    set_state(state)
                    for _ in range(WARM):
                        frame(state)
                    stream.synchronize()
                    kernels[state] = c.last_kernel
                    start.record(stream)
                    frame(state)
                    stop.record(stream)
                    torch.cuda.synchronize()
                    frames[state] = max(3, min(a.frames, int(0.3e3 / max(start.elapsed_time(stop), 1e-3))))
                for _ in range(a.rounds):
                    for state in ("whole", "plain"):
                        set_state(state)
                        frame(state)
                        torch.cuda.synchronize()
                        start.record(stream)
                        for _ in range(frames[state]):
                            frame(state)
                        stop.record(stream)
                        torch.cuda.synchronize()
                        us[state].append(1e3 * start.elapsed_time(stop) / frames[state])
                set_state("plain")
            med = {}
            cells = []
            for state in ("whole", "plain"):
                d = sorted(us[state])
                med[state] = d[len(d) // 2]
                results.append({"size": size, "S": S, "state": state, "us": {"median": round(med[state], 2), "min": round(d[0], 2), "max": round(d[-1], 2), "rounds": len(d)},
                                "frames_per_round": frames[state], "last_kernel": kernels[state], "sample_bytes": 32 * S * S * W * H})
                cells.append("%s %.1f [%.1f-%.1f]" % (state, med[state], d[0], d[-1]))
            cells.append("whole - plain %.1f us, whole / plain %.3f" % (med["whole"] - med["plain"], med["whole"] / med["plain"]))
            line = "%-9s S = %d | %s | %s after %s" % (size, S, " | ".join(cells), kernels["whole"], kernels["plain"])
            print(line, flush=True)
            lines.append(line)
            if os.path.exists(MICROBENCH):
                mb = subprocess.run([MICROBENCH, str(W), str(H), str(S), str(a.rounds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
                text = mb.stdout.strip() if mb.returncode == 0 else "fold alone: tools/microbench/resolve_vs_copy failed (%d): %s" % (mb.returncode, mb.stdout.strip()[-300:])
            else:
                text = "fold alone: not measured (tools/microbench/resolve_vs_copy is not built)"
            print("          " + text, flush=True)
            lines.append("          " + text)
            results.append({"size": size, "S": S, "state": "fold", "text": text})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
        for row in results:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
