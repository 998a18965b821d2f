#!/usr/bin/env python3
"""bench.py -- Mrays/s (primary rays) of the ray-trace hot path on MI355X.

Contract (one JSON line on stdout, printed by rank 0):
  python bench.py --gpus N --steps K --warmup W
  N > 1: one rank per GPU over RCCL.  Started by torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the
         environment) it runs as that rank.  Started plainly -- `python bench.py --gpus N`, no WORLD_SIZE -- the process
         launches `python -m torch.distributed.run --nproc-per-node N bench.py ...` itself as a CHILD process, before it
         has imported torch or made any GPU call (never an exec of a process that touched the GPU), relays rank 0's JSON
         line and exits with the child's exit code.

Workload: BASELINE.json configs[1] -- 1920x1080, 1024 spheres + 1 plane (SURVEY.md App. D scene, LCG seed 2), mode
RGB_ASCII (20-byte records).  A step is one frame: primary-ray generation, closest hit over the scene, shading and the
ANSI record write for every pixel, complete character buffer resident in HBM at the end.  rays per frame = (W-1)*H
(RayTracing.cu:187).

N = 1: each frame is rendered by one launch; by default 4 frames are in flight on 4 HIP streams (frame i in frame buffer
       i % 4), because consecutive frames are independent and the drain of one launch overlaps the ramp of the next.
       --frames-in-flight 1 renders strictly one after the other.
N > 1: every frame is sharded by pixel rows (rank g renders rows [g*H/N, (g+1)*H/N) with the global row index in ray
       generation) and assembled, complete, in the HBM of its root GPU.  The root rotates (frame i on rank i % N), so
       every directed xGMI link carries one slab per N frames.  Default (--exchange compact): frames go in rounds of M*N;
       a rank queues its slab launches of a round on several streams and ONE RCCL all-to-all per round delivers the slabs
       (4-byte pixel words, expanded into records on the root).  --exchange p2p: one point-to-point gather per frame
       (--root fixed pins the root to rank 0).  Total work is fixed as N grows ("strong").  With --full the line also carries
       "cpu_baseline" (rank 0, after the ranks are done) and "configs": {"C4": ...}: BASELINE config 4 (7680x4320, 1024
       spheres: at N = 8 the eight 540-row slabs of SURVEY 8(e)) through the same loop, with its own ms_per_step,
       verified_against_golden and roofline.

A plain run does only what the headline figure needs: it sets up, runs the run-in and the W warm-up steps, times exactly K
steps once, writes the outputs of the last step if --dump-outputs is given and prints the line.  Everything else below
(repeated batches, the golden check, roofline, timing.moving_view, modes, end_to_end, cpu_baseline; for N > 1 the C4
sub-record, the check rounds and native_group) is measured only with --full; --no-cpu-baseline, --no-verify,
--no-moving-view and --no-side-legs leave parts of it out again.

--dump-outputs DIR: after the timed steps, what the timed path computed in its last step goes to DIR/<name>.npy as float32
(N = 1 and --native): the records of the last frame ("frame_records", one row of S bytes per pixel; when the frame is larger
than the budget, a fixed sample of pixels drawn with seed 0, their pixel indices in "frame_records_index" as float64), or for
--what update / update-async the minimised stream of the last Update ("update_stream", sampled the same way).  At most 64 MB
in all.  The inputs are fixed by --config, so two builds run with the same arguments can be compared output for output.

Timing (N = 1): after the run-in and the W warm-up steps, a batch of exactly K steps is timed with HIP events (recorded on
the stream(s) the kernels are launched on: every render stream stamps the start of its first frame of the batch and the
end of its last one; the batch took from the earliest start to the latest end) and bracketed by synchronisation on both
sides.  With --full the batch is repeated until at least --min-timed-ms of GPU time has been measured and the MEDIAN batch is
reported ("timing" says how many repeats, their spread, and the wall-clock figure beside it); the last frame of the last
batch is then compared (SHA-256 of the whole 20*W*H buffer) with the committed golden value, outside the timed region:
"verified_against_golden" (null when nothing was compared).  "timing.moving_view" is the same K-frame batch with a camera
that turns 0.001 rad per frame (no two frames alike), frames in flight and one launch at a time: what the static view's
learned dispatch order is worth.

Also reported with --full (N = 1, outside the graded number): "modes": {"BIT_ASCII": ...} -- the same workload in the reference's start-up
mode (RayTracingManager.h:54; 12-byte records, the integer xterm-256 mapper) with its own ms_per_step, roofline and golden check --
and "end_to_end": the whole RayTracingManager::Update (RayTracingManager.cu:127-150: trace + GPU minimise + copy of the minimised
stream to pinned host memory), ms per Update pipelined and blocking and the bytes that cross PCIe.

Also reported with --full: "roofline" (algorithmic HBM bytes / measured kernel time vs 8 TB/s, plus the executed-VALU utilisation from
the committed rocprofv3 counters -- used only while the library sources still hash to what was profiled -- since this
path is VALU-issue bound, not HBM bound) and "cpu_baseline" (the CPU oracle -- a structure-faithful port of the reference's
loop -- timed on this host's cores on full frames of the same workload).

--native: N GPUs driven by ONE process through a device group behind the C ABI (rtx_group_create, include/rtx.h: row slabs traced on
N devices, gathered on the first by RCCL send/recv or peer copies, compact words expanded there) -- no launcher, no torch.distributed;
--native-devices 0,0,0,0 repeats a device (logical ranks on one GPU: how a single GPU walks N > 1).  With --full the N > 1 line also
carries a "native_group" sub-record: the same measurement made by rank 0 after the torch.distributed ranks are done.

--dry (tests only): the N > 1 loops over gloo with CPU tensors and the CPU oracle standing in for the HIP renderer, so that
the launch, exchange and line-assembly code can be exercised on a machine without a GPU.  Its line says "dry": true and is
not a measurement.
"""
import argparse
import hashlib
import importlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PKG = "raytracing-in-windows-console_amd"
BASELINE_METRIC = "Mrays/s (primary rays) at 1920×1080, 1024 spheres; 1/2/4/8 GPU"   # BASELINE.json "metric", verbatim
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
VALU_PEAK_TFLOPS = 157.3     # fp32 vector peak counts FMA as 2; this path may not contract, so 78.65 Tops/s
VALU_PEAK_TLANEOPS = VALU_PEAK_TFLOPS / 2.0   # lane-operations per second when no instruction is an FMA
MOVING_STEP_RAD = 0.001      # timing.moving_view: the camera's yaw changes by this much from every frame to the next


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def csrc_sha256(root=ROOT):
    """SHA-256 over the product library's sources (csrc/* and include/rtx.h, names and contents, sorted): what a
    rocprofv3 summary was taken of.  tools/summarize_prof.py stores it with the counters; here it decides whether the
    committed counters still describe the kernels that are being timed."""
    h = hashlib.sha256()
    d = os.path.join(root, PKG, "csrc")
    paths = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".cpp", ".h", ".hpp", ".inc")))
    paths.append(os.path.join(root, "include", "rtx.h"))
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()


def committed_counters(config, mode_name, kernel, root=ROOT):
    """(entry, note): per-launch rocprofv3 PMC averages of this kernel from profiles/counters.json (written by
    tools/make_counters.py from the committed *_summary.json of the same bench command).  The entry is used only if it
    carries the hash of the sources it was profiled on and that hash is the current one: a kernel edit that keeps the
    kernel's name must not report stale counters.  (None, why) otherwise."""
    path = os.path.join(root, "profiles", "counters.json")
    try:
        with open(path) as f:
            entry = json.load(f).get("%s_%s_%s" % (config, mode_name, kernel))
    except (OSError, ValueError):
        return None, "profiles/counters.json missing or unreadable"
    if not entry:
        return None, "no committed counters for this config / mode / kernel"
    want = entry.get("csrc_sha256")
    if not want:
        return None, "committed counters carry no source hash (taken before round 3): not used"
    if want != csrc_sha256(root):
        return None, "committed counters were taken on other sources (csrc hash %s..., now %s...): not used" % (want[:12], csrc_sha256(root)[:12])
    return entry, None


def algorithmic_bytes(W, H, S, ns, npl, rows=None):
    """records written + scene payload read once + params payload."""
    rows = H if rows is None else rows
    return (W - 1) * rows * S + 28 * ns + 44 * npl + 88


def algorithmic_flops(W, H, ns, npl, hit_frac):
    """19*Ns + 7*Np + 30 (ray-gen) + 150*[hit] per ray."""
    return (W - 1) * H * (19.0 * ns + 7.0 * npl + 30.0 + 150.0 * hit_frac)


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        try:
            with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
                _GOLDEN = json.load(f)
        except OSError:
            _GOLDEN = {}
    return _GOLDEN


def _frame_matches_golden(frame, config, mode_name):
    """SHA-256 of the whole frame buffer against tests/golden/golden.json (oracle-generated; no oracle needed here)."""
    want = golden().get("%s_%s" % (config, mode_name), {}).get("frame_sha256")
    if not want:
        return None   # no golden frame for this config / mode
    return hashlib.sha256(frame.tobytes()).hexdigest() == want


DUMP_LIMIT_BYTES = 56 << 20     # --dump-outputs: all files together stay under 64 MB


def dump_outputs(dirname, outputs):
    """--dump-outputs: every (n, S) uint8 array of `outputs` to dirname/<name>.npy as float32.  An array that does not fit
    the budget is replaced by a fixed sample of its rows (seed 0, ascending), whose row indices go to <name>_index.npy as
    float64: the same rows from run to run, so that two builds can be compared output for output."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    budget = DUMP_LIMIT_BYTES // max(1, len(outputs))
    for name, a in outputs.items():
        n, S = a.shape
        if n * S * 4 > budget:
            keep = budget // (S * 4 + 8)
            idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
            np.save(os.path.join(dirname, name + "_index.npy"), idx.astype(np.float64))
            a = a[idx]
        np.save(os.path.join(dirname, name + ".npy"), a.astype(np.float32))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", default=None, help="BASELINE config name (C1..C5); the graded line uses C2 (the default; C1 with --dry)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure (repeated batches, golden check, roofline, "
                         "moving view, other modes, end_to_end, cpu_baseline; N>1: C4 sub-record, check rounds, native_group)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="N=1 / --native: write what the last timed step computed to DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--sub-configs", default=None,
                    help="N>1: comma-separated configs that get a sub-record under \"configs\" after the main measurement "
                         "(default: C4 when the main config is C2 and --full is given; none with --dry; 'none' = none)")
    ap.add_argument("--mode", default="RGB_ASCII")
    ap.add_argument("--kernel", default="auto", choices=["auto", "brute", "binned"])
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--subtiles", type=int, default=0)
    ap.add_argument("--two-level", type=int, default=-1, help="-1 auto, 0 off, 1 on, 2 on with block binning")
    ap.add_argument("--refine", type=int, default=-1)
    ap.add_argument("--cell-reuse", type=int, default=-1, help="coarse-cell lists outlive the frame (RTX_OPT_CELL_REUSE): -1 auto (on), 0 off, 1 on")
    ap.add_argument("--sorted-store", type=int, default=-1, help="staging reads a direction-sorted copy of the sphere array (RTX_OPT_SORTED_STORE): -1 auto (on), 0 off")
    ap.add_argument("--xcd-order", type=int, default=-1, help="XCD-aware dispatch order of two-level grids (RTX_OPT_XCD_ORDER): -1 auto, 0 off, 1 on")
    ap.add_argument("--tile-order", type=int, default=-2, help="heaviest-first dispatch of the macro tiles: -2 library default (auto), -1 auto, 0 off, k refresh period")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: leave out cpu_baseline")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--verify", action="store_true", help="check the last frame against the golden hash, outside the timed region (default with --full)")
    ap.add_argument("--no-verify", action="store_true", help="--full: skip the byte check of the last frame")
    ap.add_argument("--no-moving-view", action="store_true", help="N=1: skip the timing.moving_view leg")
    ap.add_argument("--moving-step", type=float, default=MOVING_STEP_RAD, help="N=1: timing.moving_view's yaw step per frame in radians (default 0.001)")
    ap.add_argument("--no-side-legs", action="store_true", help="N=1: skip the secondary figures (modes.BIT_ASCII, end_to_end)")
    ap.add_argument("--min-timed-ms", type=float, default=50.0,
                    help="--full: the K-step batch is repeated until this much GPU time has been measured; the median batch is reported")
    ap.add_argument("--max-repeats", type=int, default=2000)
    ap.add_argument("--root", default="rotate", choices=["rotate", "fixed"],
                    help="N>1: frame i is assembled on rank i %% N (rotate: highest throughput) or always on rank 0, in frame order "
                         "(fixed: north_star's literal gather, in-order delivery to one consumer)")
    ap.add_argument("--exchange", default="compact", choices=["compact", "rounds", "p2p"],
                    help="N>1: compact (default) = frames in rounds of M*N with rotating roots, one RCCL all-to-all per "
                         "round, slabs as 4-byte pixel words expanded into records on the root; rounds = the same with "
                         "the slabs as records (M=1); p2p = one point-to-point gather per frame (see --root)")
    ap.add_argument("--frames-per-root", type=int, default=0, help="N>1, --exchange compact: M (0 = 8/4/4 for 2/4/8 GPUs; 8 with --root fixed)")
    ap.add_argument("--graphs", type=int, default=1, help="N>1, --exchange compact: record a round's slab launches (and its expansions) as HIP graphs (0 = off)")
    ap.add_argument("--latency", action="store_true", help="N>1, --exchange compact: also stamp every frame's completion and report queue-to-complete latency")
    ap.add_argument("--frames-in-flight", type=int, default=0,
                    help="N=1: frames rendered concurrently on separate HIP streams into separate frame buffers (default 4; 6 from 16384 spheres; "
                         "1 = strictly one launch after the other, the form the rocprof summaries are taken in).  "
                         "N>1: render streams the slab launches of a round are spread over (default 1: the loop's own stream, one batched launch per round)")
    ap.add_argument("--prewarm-ms", type=float, default=150.0,
                    help="untimed, uncounted run-in before the warm-up steps so that the GPU is at its running clocks "
                         "(N>1: the equivalent number of frames, fixed so that all ranks agree)")
    ap.add_argument("--what", default="trace", choices=["trace", "update", "update-async"],
                    help="trace: the graded step (frame resident in HBM). update: whole RayTracingManager::Update "
                         "(trace + GPU minimise + copy of the minimised stream to the host), N=1 only")
    ap.add_argument("--update-records", action="store_true",
                    help="--what update: the record form of Update (RTX_OPT_UPDATE_WORDS = 0: records written, then minimised) instead of the default word form")
    ap.add_argument("--update-host-write", type=int, default=-1, choices=[-1, 0, 1],
                    help="--what update / update-async: RTX_OPT_UPDATE_HOST_WRITE (the Minimize launch writes the pinned host buffer itself; auto = small frames only)")
    ap.add_argument("--minimize-chain", action="store_true",
                    help="--what update: Minimize from words as three launches (RTX_OPT_MINIMIZE_FUSED = 0) instead of the default single launch")
    ap.add_argument("--physics", action="store_true", help="--what update: run the UpdateObjects step (dt 0.016) in every Update, as the reference does")
    ap.add_argument("--native", action="store_true",
                    help="N GPUs in ONE process, no torchrun: a device group behind the C ABI (rtx_group_create: row slabs traced on N devices, "
                         "gathered on the first by RCCL send/recv or peer copies); the line's parallelism says so")
    ap.add_argument("--native-devices", default=None,
                    help="--native: the device list, e.g. 0,0,0,0 (an ordinal may repeat: several logical ranks on one GPU, how a one-GPU "
                         "box walks N = 4); default 0 .. N-1")
    ap.add_argument("--native-frames", type=int, default=8,
                    help="--native: frames per rtx_submit_frames call (every rank traces its rows of that many frames with one batched launch, "
                         "the slabs travel together); 1 = rtx_render, a frame per call")
    ap.add_argument("--native-threads", type=int, default=-1, help="--native: RTX_OPT_GROUP_THREADS (-1 auto: a submission thread per rank, 0 off)")
    ap.add_argument("--native-wire", default="compact", choices=["compact", "records"], help="--native: what the slabs travel as")
    ap.add_argument("--no-native-leg", action="store_true", help="N>1: skip the native_group sub-record rank 0 measures after the ranks are done")
    ap.add_argument("--dry", action="store_true",
                    help="tests only: N>1 over gloo with CPU tensors and the CPU oracle as the renderer (no GPU, not a measurement)")
    args = ap.parse_args(argv)
    if args.config is None:
        args.config = "C1" if args.dry else "C2"
    # what a plain run leaves out: only --full (or --verify for the golden check) brings it back
    args.verify = (args.full or args.verify) and not args.no_verify
    args.cpu_baseline = args.full and not args.no_cpu_baseline
    return args


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a child process (torch.distributed.run, one rank
    per GPU, rendezvous on 127.0.0.1), relay rank 0's JSON line and return the child's exit code.  Nothing in this
    process has imported torch or touched the GPU, and nothing will: it only waits."""
    nproc = max(1, args.gpus)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // nproc)))
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    out, _ = proc.communicate()
    line = None
    for ln in out.splitlines():
        s = ln.strip()
        if s.startswith("{") and s.endswith("}"):
            try:
                if "metric" in json.loads(s):
                    line = s
                    continue
            except ValueError:
                pass
        if s:
            sys.stderr.write(ln + "\n")   # anything else the ranks printed
    if line is not None:
        print(line)
        sys.stdout.flush()
    elif proc.returncode == 0:
        sys.stderr.write("bench.py: the ranks exited without printing a result line\n")
        return 1
    return proc.returncode


def host_info():
    """The host the CPU baseline ran on: logical CPUs, the CPUs this process may run on, the CPU's model name."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = None
    return {"logical_cpus": os.cpu_count(), "usable_cpus": usable, "model": model}


def cpu_baseline_leg(config, mode, threads_arg):
    """The CPU oracle (oracle/: a structure-faithful port of the reference's per-pixel loop, gcc -O2 -ffp-contract=off)
    timed on this host's cores on full frames of the same scene and mode: T = all hardware threads (4-row blocks
    drawn from a shared counter) and T = 1 beside it, the host named.  A reported baseline, not the target."""
    import oracle as O
    import util as U
    R = importlib.import_module(PKG)
    W, H, ns, npl, seed = R.CONFIGS[config]
    params, sph, pl = R.config_inputs(config)
    rays_per_frame = (W - 1) * H
    host = host_info()
    sc = O.Scene.from_arrays(sph, pl)
    op = U.oracle_params(params)
    reps = 3 if rays_per_frame <= 4_000_000 else 1   # median of >= 3 frames (1 for the big configs)

    def frame_seconds(threads):
        times = []
        for _ in range(reps):
            t1 = time.perf_counter()
            O.render(op, sc, mode, threads=threads)
            times.append(time.perf_counter() - t1)
        return sorted(times)[len(times) // 2]

    # T = every logical CPU.  A box may grant this process fewer CPUs than the host has (a cgroup quota does not
    # show in the affinity mask; 256 threads on a 16-CPU share run slower than 16), so a few smaller counts are timed beside it
    # and the FASTEST is the baseline's value -- the figure most favourable to the CPU; every count tried is listed.
    t_all = max(1, min(host["logical_cpus"] or 1, 1024))
    counts = [threads_arg] if threads_arg else sorted(set([t_all] + [t for t in (16, 32, 64) if t < t_all]))
    if rays_per_frame > 4_000_000:
        counts = counts[-1:]
    by_threads = {t: frame_seconds(t) for t in counts}
    threads = min(by_threads, key=lambda t: by_threads[t])
    dt = by_threads[threads]
    cpu = {"value": round(rays_per_frame / dt / 1e6, 4), "unit": "Mrays/s", "cores": threads, "kind": "port", "host": host,
           "by_threads": {str(t): round(rays_per_frame / by_threads[t] / 1e6, 4) for t in counts},
           "sample": "%d full %dx%d frame(s) of the same scene and mode (median) per thread count, threads drawing 4-row blocks from a "
                     "shared counter, gcc -O2 -ffp-contract=off; value = the fastest count tried (%d threads, %.2f s wall per frame; "
                     "the host has %s logical CPUs)" % (reps, W, H, threads, dt, host["logical_cpus"])}
    if threads > 1 and rays_per_frame <= 4_000_000:
        # SURVEY 8(d) asks for T=1 beside T=all; the middle quarter of the rows keeps it to ~1 s
        rows1 = max(8, (H // 4) // 8 * 8)
        t1 = time.perf_counter()
        O.render(op, sc, mode, threads=1, row0=(H - rows1) // 2, rows=rows1)
        dt1 = time.perf_counter() - t1
        cpu["single_thread"] = {"value": round((W - 1) * rows1 / dt1 / 1e6, 4), "unit": "Mrays/s", "cores": 1,
                                "sample": "rows %d..%d of the same frame; %.2f s wall" % ((H - rows1) // 2, (H - rows1) // 2 + rows1, dt1)}
    return cpu


def roofline_object(config, mode_name, kernel, W, H, S_written, ns, npl, my_rows, kernel_ms, hit_frac):
    """The "roofline" object of the line for one kernel launch: algorithmic bytes over the live kernel time
    against the HBM peak, PMC traffic and executed-VALU utilisation from the committed counters when they are current."""
    bytes_alg = algorithmic_bytes(W, H, S_written, ns, npl, my_rows)
    achieved_gbs = bytes_alg / (kernel_ms * 1e-3) / 1e9
    # HBM bytes per launch from the PMC counters of the committed profile of this same kernel
    # (profiles/counters.json: WRITE_SIZE + 2*FETCH_SIZE, the gfx950 correction); null when there is none (or stale).
    ctr, why = committed_counters(config, mode_name, kernel) if my_rows == H else (None, "a row slab, not the profiled whole-frame launch")
    traffic = round(ctr["total_bytes"]) if ctr and ctr.get("total_bytes") else None
    flops = algorithmic_flops(W, H, ns, npl, hit_frac) * (my_rows / float(H))
    # second view: this path is bound by VALU issue, not by HBM.  Executed utilisation from the committed
    # rocprofv3 counters of this same kernel and workload: SQ_INSTS_VALU wave-instructions x 64 lanes per
    # launch / kernel time / 78.65 T lane-ops/s (the fp32 vector peak with no FMA: -ffp-contract=off).
    valu = None
    if ctr and ctr.get("SQ_INSTS_VALU"):
        lane_ops = ctr["SQ_INSTS_VALU"] * 64.0
        valu = {"executed_wave_instructions_per_launch": round(ctr["SQ_INSTS_VALU"]), "lane_ops_per_launch": lane_ops,
                "achieved": round(lane_ops / (kernel_ms * 1e-3) / 1e12, 3), "peak": VALU_PEAK_TLANEOPS, "unit": "T lane-ops/s",
                "frac": round(lane_ops / (kernel_ms * 1e-3) / 1e12 / VALU_PEAK_TLANEOPS, 5),
                "source": ctr.get("source"),
                "note": "executed VALU instructions (PMC) x 64 lanes over the live kernel time; the reference's all-pairs loop would "
                        "need %.3g flops per launch (SURVEY 8(d) formula), which the culling kernel provably does not have to do" % flops}
        if ctr.get("SQ_THREAD_CYCLES_VALU") and ctr.get("SQ_ACTIVE_INST_VALU"):
            # active lanes per executed VALU instruction (rocprofv3's AvgNumActiveThreads), measured: the 64 above is an upper bound
            lanes = ctr["SQ_THREAD_CYCLES_VALU"] / ctr["SQ_ACTIVE_INST_VALU"]
            valu["active_lanes_per_instruction"] = round(lanes, 2)
            valu["active_lane_ops_per_launch"] = ctr["SQ_INSTS_VALU"] * lanes
    return {
        "bound": "hbm", "kernel": kernel, "achieved": round(achieved_gbs, 2), "peak": HBM_PEAK_GBS,
        "unit": "GB/s", "frac": round(achieved_gbs / HBM_PEAK_GBS, 5), "traffic": traffic,
        "traffic_unit": "bytes per launch (compare with bytes_per_launch)", "traffic_source": (ctr or {}).get("source"),
        "traffic_note": why,
        "bytes_per_launch": bytes_alg, "kernel_ms": round(kernel_ms, 5),
        "kernel_ms_note": "one launch at a time on one stream (HIP events, median of 5 batches), as in the rocprofv3 summaries under profiles/",
        "valu": valu,
    }


def moving_cameras(R, W, H, n=1000, step=MOVING_STEP_RAD, amplitude=0.25):
    """A ring of n cameras whose yaw follows a triangle wave of +-amplitude around the default pose, `step` radians from
    every camera to the next (also across the wrap-around): no two consecutive frames alike, the scene stays in view."""
    import math
    quarter = n // 4
    assert quarter * 4 == n and abs(quarter * step - amplitude) < 1e-9
    cams = []
    for i in range(n):
        k = i % n
        tri = k if k <= quarter else (2 * quarter - k if k <= 3 * quarter else k - 4 * quarter)
        cams.append(R.camera_params(W, H, pos=(0.0, 0.0, 0.0), rot=(0.0, float(math.pi) + tri * step, 0.0)))
    return cams


def apply_options(R, ctx, args):
    ctx.set_option(R.OPT_KERNEL, {"auto": R.KERNEL_AUTO, "brute": R.KERNEL_BRUTE, "binned": R.KERNEL_BINNED}[args.kernel])
    ctx.set_option(R.OPT_TILE_LOG2_W, args.tile)
    ctx.set_option(R.OPT_SUBTILES, args.subtiles)
    ctx.set_option(R.OPT_TWO_LEVEL, args.two_level)
    ctx.set_option(R.OPT_REFINE, args.refine)
    if args.cell_reuse != -1:
        ctx.set_option(R.OPT_CELL_REUSE, args.cell_reuse)
    if args.xcd_order != -1:
        ctx.set_option(R.OPT_XCD_ORDER, args.xcd_order)
    if args.sorted_store != -1:
        ctx.set_option(R.OPT_SORTED_STORE, args.sorted_store)
    if args.tile_order >= -1:
        ctx.set_option(R.OPT_TILE_ORDER, args.tile_order)


# ---------------------------------------------------------------------------------------------- N = 1

def run_single(args, torch, R):
    """One GPU: returns the result line (a dict)."""
    import numpy as np
    mode = R.MODE_NAMES.index(args.mode)
    S = R.SIZE_RGB if mode >= R.RGB_ASCII else R.SIZE_8BIT
    W, H, ns, npl, seed = R.CONFIGS[args.config]
    params, sph, pl = R.config_inputs(args.config)
    ctx = R.Context(W, H, device=0)
    ctx.set_scene(sph, pl)
    apply_options(R, ctx, args)
    if args.update_records:
        ctx.set_option(R.OPT_UPDATE_WORDS, 0)
    if args.minimize_chain:
        ctx.set_option(R.OPT_MINIMIZE_FUSED, 0)
    if args.update_host_write != -1:
        ctx.set_option(R.OPT_UPDATE_HOST_WRITE, args.update_host_write)
    ctx.render_rows(params, mode, 0, 1)   # uploads the scene
    ctx.synchronize()
    if args.frames_in_flight <= 0:
        # 4 frames in flight; 6 where a frame is two dependent launches (the coarse-cell pre-pass of large scenes, then
        # the trace): config 5 44.7 -> 42.7 us per frame, the other configs the same with 4 and 6
        args.frames_in_flight = 6 if len(sph) >= 16384 else 4
    K, Wm = args.steps, args.warmup
    frame_bytes = 20 * W * H
    F = max(1, args.frames_in_flight)
    streams, fbufs, inflight = None, None, []
    last_update = [None, 0]     # the Update forms: the host buffer of the latest step and its minimised length
    if args.what == "update":
        F = 1

        def step(i):
            last_update[0] = ctx.update(params, mode, dt=0.016, run_physics=args.physics)
            last_update[1] = len(last_update[0])
    elif args.what == "update-async":
        F = 1
        hb = [ctx.host_alloc(frame_bytes) for _ in range(2)]

        def step(i):
            if len(inflight) == 2:
                ctx.update_end(inflight.pop(0))
            inflight.append(ctx.update_begin(params, mode, hb[i % 2][0]))
            last_update[0] = hb[i % 2][1]
    elif F == 1:
        def step(i):
            ctx.render(params, mode)
    else:
        # F frames in flight: frame i goes to stream i % F and frame buffer i % F.  Consecutive frames do
        # not depend on each other, so the tail of one frame's launch (few workgroups left, SIMDs
        # under-occupied) overlaps with the start of the next ones.  Every frame is rendered in full.
        streams = [torch.cuda.Stream() for _ in range(F)]
        fbufs = [torch.zeros(frame_bytes, dtype=torch.uint8, device="cuda") for _ in range(F)]
        torch.cuda.synchronize()
        submit = ctx.make_submitter(params, mode, [b.data_ptr() for b in fbufs], [st.cuda_stream for st in streams])

        def step(i):
            # one frame per step; rtx_submit_frames queues it on stream i % F (one host call per frame)
            submit(1, i % F)

    # Clock ramp: an idle MI355X needs some tens of milliseconds of work to reach its running clocks (measured:
    # 25.3 us per frame when timing starts 5 ms after idle, 20.2 us in steady state).  So the GPU is first kept
    # busy with the same frames for --prewarm-ms; none of this is timed or counted.
    def drain():
        if args.what == "update-async":
            while inflight:
                last_update[1] = ctx.update_end(inflight.pop(0))   # the last one ended is the latest step's
        ctx.synchronize()
        torch.cuda.synchronize()

    n_pre = 0
    t_pre = time.perf_counter()
    while (time.perf_counter() - t_pre) * 1e3 < args.prewarm_ms:
        for _ in range(64):
            step(n_pre)
            n_pre += 1
        drain()
    for i in range(Wm):
        step(i)
    drain()

    # One timed batch = exactly K steps, device-timed with HIP events on the streams the kernels run on and
    # bracketed by synchronisation on both sides.
    def make_timed_batch(step_fn, nstreams):
        if args.what != "trace":
            def timed_batch():       # the Update forms block on the host: wall clock is the measurement
                t0 = time.perf_counter()
                for i in range(K):
                    step_fn(i)
                drain()
                dt = (time.perf_counter() - t0) * 1e3
                return dt, dt
        elif nstreams == 1:
            def timed_batch():
                t0 = time.perf_counter()
                ctx.timer_start()                     # hipEventRecord on the context's stream
                for i in range(K):
                    step_fn(i)
                ev_ms = ctx.timer_stop()              # hipEventRecord + hipEventSynchronize + elapsed
                torch.cuda.synchronize()
                return ev_ms, (time.perf_counter() - t0) * 1e3
        else:
            # Each render stream stamps the start of its first frame of the batch and the end of its last one; the batch
            # took from the earliest start to the latest end (hipEventElapsedTime between events of different streams).
            # No stream waits for another at either end, so the window holds the K frames' launches and nothing else.
            ev_s = [torch.cuda.Event(enable_timing=True) for _ in range(nstreams)]
            ev_e = [torch.cuda.Event(enable_timing=True) for _ in range(nstreams)]

            def timed_batch():
                t0 = time.perf_counter()
                used = min(nstreams, K)
                for i in range(K):
                    if i < nstreams:
                        ev_s[i].record(streams[i])
                    step_fn(i)
                for j in range(used):
                    ev_e[j].record(streams[j])
                for j in range(used):
                    ev_e[j].synchronize()
                torch.cuda.synchronize()
                ev_ms = max(ev_s[a].elapsed_time(ev_e[b]) for a in range(used) for b in range(used))
                return ev_ms, (time.perf_counter() - t0) * 1e3
        return timed_batch

    def repeat(timed_batch, min_ms):
        evs, walls = [], []
        while True:
            e_ms, w_ms = timed_batch()
            evs.append(e_ms)
            walls.append(w_ms)
            if len(evs) >= args.max_repeats or (sum(evs) >= min_ms and len(evs) >= 3):
                break
        return evs, walls

    if args.full:
        ev_batches, wall_batches = repeat(make_timed_batch(step, F), args.min_timed_ms)
    else:
        # a plain run: exactly K timed steps, one batch
        e_ms, w_ms = make_timed_batch(step, F)()
        ev_batches, wall_batches = [e_ms], [w_ms]
    batch_ms = median(ev_batches)
    elapsed = batch_ms * 1e-3                     # seconds per K steps, the median batch
    how = "; median over repeated batches" if args.full else "; one batch"
    timing = {"method": ("HIP events on the render streams around each batch of K steps (earliest first-frame start to latest "
                         "last-frame end), sync on both sides" if args.what == "trace" else "wall clock around each batch of K blocking steps") + how,
              "repeats": len(ev_batches), "timed_ms_total": round(sum(ev_batches), 3),
              "batch_ms": {"median": round(batch_ms, 5), "min": round(min(ev_batches), 5), "max": round(max(ev_batches), 5)},
              "wall_ms_per_step_median": round(median(wall_batches) / K, 5)}
    # what the last timed step computed, read back outside the timed region (before any other leg reuses the buffers)
    final = None
    if args.what == "trace" and (args.verify or args.dump_outputs):
        final = ctx.read_frame(frame_bytes) if F == 1 else fbufs[(K - 1) % F].cpu().numpy()
    if args.dump_outputs:
        if args.what == "trace":
            dump_outputs(args.dump_outputs, {"frame_records": final[:S * W * H].reshape(H * W, S)})
        else:
            dump_outputs(args.dump_outputs, {"update_stream": np.array(last_update[0][:last_update[1]]).reshape(-1, 1)})
    kernel_ms = None
    # The dominant kernel on its own: launches one after the other on the context's stream, timed with
    # HIP events on that stream (this is what a rocprofv3 kernel trace of --frames-in-flight 1 shows).
    if args.what != "trace":
        kernel_ms = elapsed / K * 1e3
    elif args.full:
        Kr = max(10, min(K, 100))
        # (the context's own stream has its own dispatch order: let it settle as the render streams' did --
        # the library balances a tile grid over its first launches on a stream, and keeps refining every 64th)
        for _ in range(5 if F == 1 else 1000):
            ctx.render(params, mode)
        ctx.synchronize()
        singles = []
        for _ in range(5):
            ctx.timer_start()
            for _ in range(Kr):
                ctx.render(params, mode)
            singles.append(ctx.timer_stop() / Kr)
        kernel_ms = median(singles)

    # timing.moving_view: the same K-frame batches with a camera that turns MOVING_STEP_RAD per frame (a ring of 1000
    # views, +-0.25 rad around the default pose), F frames in flight and one launch at a time.  The dispatch order the
    # library learns on a static view (rtx_balance_tiles) has nothing to learn from here; these are the rates a caller
    # whose camera never rests sees.  Outside the graded number, after the verification copy.
    if args.full and args.what == "trace" and not args.no_moving_view:
        NMV = 1000 if 1000 % F == 0 else 1200          # a multiple of the frames in flight (1200: of 1..6, 8, 10, 12)
        MS = args.moving_step
        cams = moving_cameras(R, W, H, NMV, step=MS, amplitude=NMV // 4 * MS)
        counter = [0]
        mv = {"step_rad_per_frame": MS, "views": NMV,
              "what": "batches of the same K frames, yaw on a triangle wave of +-%.2f rad, every frame %g rad from the one before" % (NMV // 4 * MS, MS)}
        if F > 1:
            ring = ctx.make_submitter(cams, mode, [fbufs[i % F].data_ptr() for i in range(NMV)], [streams[i % F].cuda_stream for i in range(NMV)])

            def step_mv(i):
                # frame buffer / stream i % F as in the static batch (NMV is a multiple of F or the ring position decides)
                ring(1, counter[0] % NMV)
                counter[0] += 1
            if NMV % F == 0:
                for i in range(200):
                    step_mv(i)
                drain()
                counter[0] = 0   # batches start on stream 0, as the event bookkeeping assumes
                evs, _ = repeat(make_timed_batch(lambda i: (ring(1, (counter[0] + i) % NMV)), F), min(args.min_timed_ms, 30.0))
                # (every batch replays views counter[0] .. counter[0]+K-1; advancing by K keeps ring position % F == i % F only
                # when K % F == 0, so the batches all start at view 0: K consecutive views, each a step from the last)
                mv["in_flight_ms_per_frame"] = round(median(evs) / K, 5)
                mv["frames_in_flight"] = F

        def step_alone(i):
            ctx.render(cams[counter[0] % NMV], mode)
            counter[0] += 1
        counter[0] = 0
        for i in range(200):
            step_alone(i)
        ctx.synchronize()
        alone = []
        for _ in range(5):
            ctx.timer_start()
            for i in range(max(10, min(K, 200))):
                step_alone(i)
            alone.append(ctx.timer_stop() / max(10, min(K, 200)))
        mv["alone_ms_per_frame"] = round(median(alone), 5)
        try:   # how the coarse-cell lists (two-level culling) were obtained over the whole run: in-line builds, builds ahead of time, launches served from cached lists, launches that binned for themselves
            mv["cell_lists"] = {k: ctx.get_option(v) for k, v in (("builds", R.STAT_CELL_BUILDS), ("prefetches", R.STAT_CELL_PREFETCHES),
                                                                  ("hits", R.STAT_CELL_HITS), ("per_frame", R.STAT_CELL_PER_FRAME),
                                                                  ("capacity_floor", R.STAT_CELL_CAPACITY_FLOOR))}
        except R.RtxError:
            pass
        mv["static_in_flight_ms_per_frame"] = round(elapsed / K * 1e3, 5)
        mv["static_alone_ms_per_frame"] = round(kernel_ms, 5)
        timing["moving_view"] = mv

    rays_per_frame = (W - 1) * H
    kernel = ctx.last_kernel
    # ---- side legs (SURVEY 8(d)'s secondary figures, outside the graded number): the same workload in BIT_ASCII -- the
    # reference's start-up mode (RayTracingManager.h:54), 12-byte records, the integer xterm-256 mapper -- and the whole
    # RayTracingManager::Update (RayTracingManager.cu:127-150: trace + minimise + copy of the minimised stream to the host)
    side_modes, end_to_end = {}, None
    if args.full and args.what == "trace" and not args.no_side_legs:
        for mname in [m for m in ("BIT_ASCII",) if m != args.mode]:
            m2 = R.MODE_NAMES.index(mname)
            S2 = R.SIZE_RGB if m2 >= R.RGB_ASCII else R.SIZE_8BIT
            rec = {"workload": "%s in mode %s (%d-byte records)" % (args.config, mname, S2)}
            if F > 1:
                for b in fbufs:
                    b.zero_()        # the 8-bit modes leave bytes >= 12*W*H of the frame untouched (RayTracing.cu:238): NUL, as after the reference's memset
                torch.cuda.synchronize()
                sub2 = ctx.make_submitter(params, m2, [b.data_ptr() for b in fbufs], [st.cuda_stream for st in streams])

                def step2(i):
                    sub2(1, i % F)
            else:
                def step2(i):
                    ctx.render(params, m2)
            for i in range(max(Wm, 8 * F)):
                step2(i)
            drain()
            evs2, _ = repeat(make_timed_batch(step2, F), min(args.min_timed_ms, 25.0))
            ms2 = median(evs2) / K
            if args.verify:
                fin2 = ctx.read_frame(frame_bytes) if F == 1 else fbufs[(K - 1) % F].cpu().numpy()
                rec["verified_against_golden"] = _frame_matches_golden(fin2, args.config, mname)
            for _ in range(5 if F == 1 else 300):
                ctx.render(params, m2)
            ctx.synchronize()
            singles2 = []
            for _ in range(5):
                ctx.timer_start()
                for _ in range(max(10, min(K, 100))):
                    ctx.render(params, m2)
                singles2.append(ctx.timer_stop() / max(10, min(K, 100)))
            g2 = golden().get("%s_%s" % (args.config, mname), {})
            rec.update({"value": round(rays_per_frame / (ms2 * 1e-3) / 1e6, 3), "unit": "Mrays/s", "ms_per_step": round(ms2, 5),
                        "frames_in_flight": F, "repeats": len(evs2),
                        "roofline": roofline_object(args.config, mname, ctx.last_kernel, W, H, S2, ns, npl, H, median(singles2),
                                                    (g2.get("foreground_pixels") or 0) / float(rays_per_frame))})
            side_modes[mname] = rec
        # the whole Update, pipelined (rtx_update_begin / _end: the copy of frame k beside the trace of frame k+1) and blocking
        # (each form runs untimed for 100 ms first: freshly pinned buffers and an idle PCIe link read 0.376 ms per Update over the
        # first hundred frames where the steady state -- `--what update-async` over thousands -- is 0.326)
        n_up = max(50, min(K, 200))
        hb = [ctx.host_alloc(frame_bytes) for _ in range(2)]
        tick = []
        i, t_warm, t_up = 0, time.perf_counter(), None
        while t_up is None or i < n_up:
            if t_up is None and (time.perf_counter() - t_warm) > 0.1:
                while tick:
                    ctx.update_end(tick.pop(0))
                t_up, i = time.perf_counter(), 0
            if len(tick) == 2:
                ctx.update_end(tick.pop(0))
            tick.append(ctx.update_begin(params, mode, hb[i % 2][0]))
            i += 1
        nbytes = 0
        while tick:
            nbytes = ctx.update_end(tick.pop(0))
        async_ms = (time.perf_counter() - t_up) * 1e3 / n_up
        for p_, _ in hb:
            ctx.host_free(p_)
        t_warm = time.perf_counter()
        while (time.perf_counter() - t_warm) < 0.1:
            ctx.update(params, mode)
        t_up = time.perf_counter()
        for _ in range(n_up):
            ctx.update(params, mode)
        sync_ms = (time.perf_counter() - t_up) * 1e3 / n_up
        gm = golden().get("%s_%s" % (args.config, args.mode), {})
        end_to_end = {"what": "RayTracingManager::Update (RayTracingManager.cu:127-150) per frame, static scene: trace + GPU minimise + copy of the "
                              "minimised stream into pinned host memory; wall clock over %d frames" % n_up,
                      "ms_per_update_pipelined": round(async_ms, 5), "ms_per_update_blocking": round(sync_ms, 5),
                      "pcie_bytes_per_update": int(nbytes), "frame_bytes_not_copied": frame_bytes,
                      "pcie_GBs_pipelined": round(nbytes / (async_ms * 1e-3) / 1e9, 2),
                      "minimized_bytes_match_golden": (nbytes == gm.get("minimized_bytes")) if gm.get("minimized_bytes") else None,
                      "bound": "PCIe (the device side of an Update is a few tens of microseconds; see DESIGN.md)"}
        # ... and the reference's own workload: its default scene on a console-sized frame (400 x 150) in its start-up mode
        # (BIT_ASCII, RayTracingManager.h:54), physics step included -- launches and host waits, nothing else, at this size
        try:
            cw, chh = 400, 150
            with R.Context(cw, chh) as small:
                small.set_reference_default_scene()
                sp = R.camera_params(cw, chh)
                for _ in range(200):
                    got_small = small.update(sp, R.BIT_ASCII, dt=0.016, run_physics=True)
                n_small = 2000
                t_up = time.perf_counter()
                for _ in range(n_small):
                    got_small = small.update(sp, R.BIT_ASCII, dt=0.016, run_physics=True)
                small_sync = (time.perf_counter() - t_up) * 1e6 / n_small
                hb2 = [small.host_alloc(20 * cw * chh) for _ in range(2)]
                tick = []
                for i in range(n_small + 200):
                    if i == 200:
                        while tick:
                            small.update_end(tick.pop(0))
                        t_up = time.perf_counter()
                    if len(tick) == 2:
                        small.update_end(tick.pop(0))
                    tick.append(small.update_begin(sp, R.BIT_ASCII, hb2[i % 2][0], dt=0.016, run_physics=True))
                while tick:
                    small.update_end(tick.pop(0))
                small_async = (time.perf_counter() - t_up) * 1e6 / n_small
                for p_, _ in hb2:
                    small.host_free(p_)
                end_to_end["console_frame"] = {"what": "the reference's default scene (Scene3D.cpp:28-33), 400 x 150, BIT_ASCII, UpdateObjects step included: "
                                                       "whole Update per frame, wall clock over %d frames" % n_small,
                                               "us_per_update_blocking": round(small_sync, 2), "us_per_update_pipelined": round(small_async, 2),
                                               "bytes_per_update": int(len(got_small))}
        except Exception as exc:   # (a side figure must not lose the line)
            end_to_end["console_frame"] = {"error": repr(exc)}
    mrays = rays_per_frame * K / elapsed / 1e6
    g = golden().get("%s_%s" % (args.config, args.mode), {})
    hit_frac = (g.get("foreground_pixels") or 0) / float(rays_per_frame)
    verified = _frame_matches_golden(final, args.config, args.mode) if (args.verify and final is not None) else None
    roofline = roofline_object(args.config, args.mode, kernel, W, H, S, ns, npl, H, kernel_ms, hit_frac) if (args.full and args.what == "trace") else None
    ctx.close()

    cpu = None
    if args.cpu_baseline:
        cpu = cpu_baseline_leg(args.config, mode, args.cpu_threads)
    out = {
        "metric": BASELINE_METRIC,
        "value": round(mrays, 3), "unit": "Mrays/s", "n_gpus": 1, "steps": K, "warmup": Wm,
        "ms_per_step": round(elapsed / K * 1e3, 5), "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s: %dx%d, %d spheres + %d planes, mode %s, SURVEY App. D scene seed %d"
                               % (args.config, W, H, ns, npl, args.mode, seed),
                   "rays_per_frame": rays_per_frame, "kernel": kernel, "prewarm_ms": args.prewarm_ms,
                   "parallelism": "1 GPU"},
        "timing": timing, "roofline": roofline, "cpu_baseline": cpu,
    }
    if args.what != "trace":
        out["metric"] = "Mrays/s through the whole Update (trace + minimise + D2H of the minimised stream); not the graded metric"
        out["roofline"] = None
    else:
        eff_ms = elapsed / K * 1e3
        out["config"]["frames_in_flight"] = F
        if roofline is not None:
            roofline["pipelined"] = {
                "frames_in_flight": F, "effective_ms_per_frame": round(eff_ms, 5),
                "achieved": round(roofline["bytes_per_launch"] / (eff_ms * 1e-3) / 1e9, 2), "unit": "GB/s",
                "frac": round(roofline["bytes_per_launch"] / (eff_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                "note": "whole-job rate with overlapping launches; 'achieved'/'frac' above are for one launch alone"}
    if side_modes:
        out["modes"] = side_modes
    if end_to_end:
        out["end_to_end"] = end_to_end
    # true / false = the last frame was compared with the committed golden SHA-256; null = nothing was compared
    out["verified_against_golden"] = verified
    if cpu:
        out["speedup_vs_cpu_baseline"] = round(mrays / cpu["value"], 1)
    return out


# ---------------------------------------------------------------------------------------------- N GPUs, one process (device group)

def run_native(args, torch, R, devices, config, K, Wm, prewarm_ms, update_leg=True):
    """The row-sharded frame behind the C ABI: ONE process, a device group over `devices` (rtx_group_create), K frames through
    rtx_render -- every rank traces its row slab on its device, the slabs are gathered on devices[0] (RCCL send/recv between
    distinct devices, peer copies otherwise), compact words expanded there -- timed with HIP events on the root's stream
    (the frame is complete in stream order there), median over repeated batches.  Returns the record (a dict)."""
    mode = R.MODE_NAMES.index(args.mode)
    S = R.SIZE_RGB if mode >= R.RGB_ASCII else R.SIZE_8BIT
    W, H, ns, npl, seed = R.CONFIGS[config]
    params, sph, pl = R.config_inputs(config)
    n = len(devices)
    ctx = R.Context(W, H, devices=devices)
    try:
        ctx.set_scene(sph, pl)
        apply_options(R, ctx, args)
        ctx.set_option(R.OPT_GROUP_WIRE, R.WIRE_RECORDS if args.native_wire == "records" else R.WIRE_COMPACT)
        if n > 1:
            ctx.set_option(R.OPT_GROUP_THREADS, args.native_threads)
        ctx.render(params, mode)
        ctx.synchronize()
        M = max(1, min(args.native_frames, 16, K))
        fbufs = None
        if M > 1:
            # M frames per call into M frame buffers on the root's device (rtx_submit_frames on the group)
            fbufs = [torch.zeros(20 * W * H, dtype=torch.uint8, device="cuda:%d" % devices[0]) for _ in range(M)]
            torch.cuda.synchronize()
            sub = ctx.make_submitter(params, mode, [b.data_ptr() for b in fbufs], [None] * M)

        def frames(count):
            if M == 1:
                for _ in range(count):
                    ctx.render(params, mode)
            else:
                done = 0
                while done < count:
                    sub(min(M, count - done), 0)
                    done += min(M, count - done)

        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < prewarm_ms:
            frames(32)
            ctx.synchronize()
        frames(Wm)
        ctx.synchronize()
        evs, walls = [], []
        while True:
            tw = time.perf_counter()
            ctx.timer_start()
            frames(K)
            evs.append(ctx.timer_stop())
            walls.append((time.perf_counter() - tw) * 1e3)
            if not args.full or len(evs) >= min(args.max_repeats, 200) or (sum(evs) >= args.min_timed_ms and len(evs) >= 3):
                break     # (a plain run: exactly K timed frames, one batch)
        batch_ms = median(evs)
        frame = None
        if args.verify or args.dump_outputs:
            frame = ctx.read_frame(20 * W * H) if M == 1 else fbufs[(K - 1) % M if K % M else M - 1].cpu().numpy()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"frame_records": frame[:S * W * H].reshape(H * W, S)})
        verified = _frame_matches_golden(frame, config, args.mode) if args.verify else None
        rays = (W - 1) * H
        rec = {"value": round(rays * K / (batch_ms * 1e-3) / 1e6, 3), "unit": "Mrays/s", "n_gpus": len(set(devices)), "logical_ranks": n,
               "steps": K, "warmup": Wm, "ms_per_step": round(batch_ms / K, 5),
               "config": {"workload": "%s: %dx%d, %d spheres + %d planes, mode %s, SURVEY App. D scene seed %d" % (config, W, H, ns, npl, args.mode, seed),
                          "rays_per_frame": rays, "devices": list(devices), "frames_per_call": M,
                          "rows_per_rank": [ctx.group_rows(H, r)[1] for r in range(n)],
                          "parallelism": "device group behind the C ABI (rtx_group_create): one process, %d logical rank(s) on %d device(s), rows "
                                         "sharded, slabs gathered on device %d as %s; exchange: %s"
                                         % (n, len(set(devices)), devices[0], "4-byte pixel words expanded there" if args.native_wire == "compact" else "records",
                                            ctx.exchange_note)},
               "timing": {"method": "HIP events on the root's stream around each batch of K rtx_render calls (a frame is complete there in stream order); " +
                                    ("median over repeated batches" if args.full else "one batch"), "repeats": len(evs),
                          "batch_ms": {"median": round(batch_ms, 5), "min": round(min(evs), 5), "max": round(max(evs), 5)},
                          "wall_ms_per_step_median": round(median(walls) / K, 5)},
               "gather_bytes_per_frame": ctx.get_option(R.STAT_GROUP_BYTES),
               "verified_against_golden": verified}
        if update_leg:
            gm = golden().get("%s_%s" % (config, args.mode), {})
            n_up = max(10, min(K, 50))

            def time_updates():
                for _ in range(5):
                    ctx.update(params, mode)
                tw = time.perf_counter()
                for _ in range(n_up):
                    got = ctx.update(params, mode)
                return (time.perf_counter() - tw) * 1e3 / n_up, got

            # both forms of the hand-off (RTX_OPT_GROUP_UPDATE): gathered on the root and copied over its link; every rank its own rows
            # over its own link.  The group's default (auto: direct where the list names two or more distinct devices) is named.
            default_direct = len(set(devices)) >= 2
            forms = {}
            streams = {}
            for name, val in (("gathered", 0), ("direct", 1)):
                if n < 2 and val == 1:
                    continue
                ctx.set_option(R.OPT_GROUP_UPDATE, val)
                up_ms, got = time_updates()
                streams[name] = bytes(got)     # (a view of the pinned buffer: valid until the next update)
                forms[name] = {"ms_per_update_blocking": round(up_ms, 5), "pcie_bytes_per_update": int(len(got)),
                               "minimized_bytes_match_golden": (int(len(got)) == gm.get("minimized_bytes")) if gm.get("minimized_bytes") else None}
            if "direct" in streams:
                forms["direct"]["same_bytes_as_gathered"] = streams["direct"] == streams["gathered"]
            ctx.set_option(R.OPT_GROUP_UPDATE, -1)
            used = "direct" if (default_direct and "direct" in forms) else "gathered"
            rec["end_to_end"] = {"what": "rtx_update through the group (RayTracingManager::Update's seam, RayTracingManager.cu:76-154), blocking, wall clock over %d "
                                         "frames.  gathered: sharded trace, gather of the pixel words, minimise on the root, copy of the minimised stream over the "
                                         "root's PCIe link.  direct (RTX_OPT_GROUP_UPDATE): every rank traces, minimises and copies its own rows over its own link" % n_up,
                                 "default_form": used, "direct_updates_counted": ctx.get_option(R.STAT_GROUP_DIRECT_UPDATES)}
            rec["end_to_end"].update(forms[used])
            rec["end_to_end"]["forms"] = forms
        return rec
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- N > 1 (GPUs over RCCL)

def run_sharded(args, torch, dist, R, sharding, rank, world, local_rank, config, K, Wm, prewarm_frames):
    """One configuration through the N > 1 loop on this rank's GPU.  Returns (on every rank) a dict with the elapsed
    seconds per K frames (MAX over ranks, median window), the timing object, the verification verdicts, this rank's
    slab-kernel time and the strings the line needs."""
    import numpy as np
    mode = R.MODE_NAMES.index(args.mode)
    S = R.SIZE_RGB if mode >= R.RGB_ASCII else R.SIZE_8BIT
    W, H, ns, npl, seed = R.CONFIGS[config]
    params, sph, pl = R.config_inputs(config)
    ctx = R.Context(W, H, device=local_rank)
    ctx.set_scene(sph, pl)
    apply_options(R, ctx, args)
    ctx.render_rows(params, mode, 0, 1)   # uploads the scene (a HIP graph capture later on must not have to)
    ctx.synchronize()
    # render streams of a rank's slab launches.  Default 1: every slab of a round on the loop's own stream, where the library
    # traces them with ONE batched launch per <= 16 frames (RTX_OPT_BATCH, rtx_trace_batch: eight 135-row slab-frames of 1080p in
    # 26 us against 88-113 us as eight launches over 2-4 streams, tools/batch_slabs_gpu.py) and no fork / join is needed; F > 1
    # spreads the slabs over F streams of their own, a launch each, as rounds 1-3 did.
    F = args.frames_in_flight if args.frames_in_flight > 0 else 1
    bounds = sharding.row_bounds(H, world)
    row0, rows = bounds[rank], bounds[rank + 1] - bounds[rank]
    # The loop runs on a stream of its own, made torch's current stream: the collectives are ordered after it, and
    # its handle is not 0.  (torch's default stream has handle 0, which the C ABI reads as "the context's own
    # stream" / "no stream to join": with it neither rtx_submit_slabs' fork/join nor a graph capture would touch
    # the stream the exchange is queued on.  Round 1's loop did exactly that; its frames only looked right because
    # every frame of a bench run is the same frame.  The check rounds below would now catch it.)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    latency = None
    n_rounds = q0 = RF = None
    rstreams = None
    compact = args.exchange == "compact"
    if args.exchange in ("compact", "rounds"):
        # Frames in rounds of M*N, frame m*N+j of a round assembled on rank j, ONE all-to-all per round.  The
        # slab launches of a round go to F streams forked from / joined into torch's current stream (inside
        # rtx_submit_slabs), which the RCCL call is ordered after.  "compact": the slabs travel as 4-byte
        # pixel words and the root expands them into records on a side stream once the exchange is done.
        fixed_root = args.root == "fixed"      # in-order delivery: every frame assembled on rank 0, in frame order
        roots = [0] if fixed_root else None
        M = 1 if not compact else (args.frames_per_root or ({2: 8, 4: 8, 8: 8} if fixed_root else {2: 8, 4: 4, 8: 4}).get(world, max(1, 16 // world)))
        # at most 512 MB per destination and round: a single transfer past 1 GiB arrived truncated in the world-size-1 walk of
        # config 4 (16 units of 133 MB to one destination: frames 8..15 of every full round were stale), and rounds that large
        # buy nothing anyway
        M = max(1, min(M, (1 << 29) // max(1, 4 * W * max(1, rows))))
        post = torch.cuda.Stream()
        expanders = {}
        use_graphs = [compact and args.graphs != 0]
        slab_graphs, expand_graphs = {}, {}
        full_mine = [None]
        # per-frame latency: an event when a round's slab launches are queued, one when each of its frames is
        # complete on its root (pools of timing events, reused round-robin; read after the timed region)
        POOL = 64
        ev_submit = [torch.cuda.Event(enable_timing=True) for _ in range(POOL)]
        ev_done = [[torch.cuda.Event(enable_timing=True) for _ in range(max(1, M))] for _ in range(POOL)]
        done_count = {}

        class _After:
            def __init__(self, ev):
                self.ev = ev

            def wait(self):
                torch.cuda.current_stream().wait_event(self.ev)

        def graph_or_none(build, on_stream, what):
            """Records what build() queues on `on_stream` as a HIP graph; None (and no more attempts) if that fails."""
            if not use_graphs[0]:
                return None
            try:
                ctx.graph_begin(on_stream)
                try:
                    build()
                finally:
                    g = ctx.graph_end(on_stream)
                return ctx.graph_launcher(g, on_stream)
            except R.RtxError as exc:
                sys.stderr.write("bench.py: HIP graph capture of the %s failed (%s); queueing launch by launch\n" % (what, exc))
                use_graphs[0] = False
                return None

        def finish(q, b, work, mine):
            with torch.cuda.stream(post):
                work.wait()   # orders `post` (only) after the exchange
                key = (b, len(mine))
                for m, segs in mine:
                    ek = (b, m, len(mine))
                    if ek not in expanders:
                        expanders[ek] = ctx.make_expander(mode, pipe.recv[b].data_ptr(), pipe.frames[b][m].data_ptr(), segs, post.cuda_stream)
                if args.latency:
                    # frame by frame, so that every frame's completion can be stamped (frames leave in frame order)
                    for m, _ in mine:
                        expanders[(b, m, len(mine))]()
                        ev_done[q % POOL][m].record(post)
                    done_count[q % POOL] = (q, len(mine))
                else:
                    # a graph only for full rounds (the first round, untimed, is one: it fixes how many frames of a
                    # full round are this rank's); a partial round -- K is not a multiple of the round -- is queued
                    # launch by launch, so that nothing is recorded inside the timed region
                    if full_mine[0] is None:
                        full_mine[0] = len(mine)
                    if mine and len(mine) == full_mine[0] and key not in expand_graphs:
                        expand_graphs[key] = graph_or_none(lambda: [expanders[(b, m, len(mine))]() for m, _ in mine], post.cuda_stream, "expansions")
                    if mine and expand_graphs.get(key) is not None:
                        expand_graphs[key]()
                    else:
                        for m, _ in mine:
                            expanders[(b, m, len(mine))]()
                ev = torch.cuda.Event()
                ev.record(post)
            return _After(ev)

        pipe = sharding.RowShardedRounds(dist, torch, rank, world, W, H, S, "cuda", nbuf=2, frames_per_root=M,
                                         pixel_bytes=4 if compact else None, finish=finish if compact else None, roots=roots)
        rstreams = [torch.cuda.Stream() for _ in range(F)] if F > 1 else [stream]
        torch.cuda.synchronize()
        RF = pipe.round_frames
        submitters = [ctx.make_slab_submitter(params, mode, row0, rows, row0,
                                              [pipe.unit(b, f).data_ptr() if rows else pipe.send[b].data_ptr() for f in range(RF)],
                                              [rstreams[f % F].cuda_stream for f in range(RF)], stream.cuda_stream,
                                              flags=R.RENDER_COMPACT if compact else 0)
                      for b in range(pipe.nbuf)]

        # A recorded launch runs under the dispatch order its tile grid has converged to on its stream, and freezes it (rtx.h):
        # so the first rounds are queued launch by launch until every render stream has been through the library's settling
        # passes (about 70 launches of the slab's grid per stream), as far as the run-in allows; then the rounds are recorded.
        settle_rounds = min(-(-72 * F // RF), max(0, prewarm_frames // RF - 2))
        rounds_queued = [0]

        def render_round(q, b, nframes):
            if args.latency:
                ev_submit[q % POOL].record(stream)
            if not rows:
                return
            rounds_queued[0] += 1
            if nframes == RF and use_graphs[0] and rounds_queued[0] > settle_rounds:
                # a full round's slab launches (forked over the render streams, joined back) as one graph replay
                if b not in slab_graphs:
                    slab_graphs[b] = graph_or_none(lambda: submitters[b](RF), stream.cuda_stream, "slab launches")
                if slab_graphs.get(b) is not None:
                    slab_graphs[b]()
                    return
            submitters[b](nframes)

        elapsed, q0 = sharding.timed_rounds(dist, torch, pipe, render_round, K, Wm, "cuda", torch.cuda.synchronize,
                                            prewarm=prewarm_frames,
                                            min_total=args.min_timed_ms * 1e-3, max_repeats=min(args.max_repeats, 200) if args.full else 1)
        n_rounds = -(-K // RF)
        last_frame = (q0 + n_rounds - 1) * RF + (K - 1 - (n_rounds - 1) * RF)
        slab0 = pipe.unit(0, 0)
        if args.latency and compact:
            # queued -> complete on the root, for the frames of the last rounds still in the event pools
            lat = []
            for slot, (q, n) in done_count.items():
                if q0 <= q < q0 + n_rounds:
                    for m in range(n):
                        lat.append(ev_submit[slot].elapsed_time(ev_done[slot][m]))
            t = torch.tensor([median(lat) if lat else -1.0, max(lat) if lat else -1.0], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            latency = {"median_ms": round(float(t[0].item()), 4), "max_ms": round(float(t[1].item()), 4),
                       "of": "a frame, from the queueing of its round's slab launches to the complete frame on its root (HIP events; "
                             "worst rank); a round is %d frames" % RF}
        exchange_note = ("frames in rounds of %d (M=%d per root), %s by one RCCL all-to-all per round; "
                         % (RF, M, "every frame assembled on rank 0 in frame order (in-order delivery)" if fixed_root
                            else "frame i of a round assembled on rank i %% N")) + \
                        ("slabs travel as 4-byte pixel words, the root expands them into records (rtx_expand)" if compact
                         else "slabs travel as records") + ("; HIP graph per round" if use_graphs[0] and slab_graphs else "")
    else:
        pipe = sharding.RowShardedFrames(dist, torch, rank, world, W, H, S, "cuda", nbuf=2, rotate_root=(args.root == "rotate"))

        def render(buf, r0, nrows, base):
            # root traces its own rows straight into the frame; peers into their slab.  Same stream as the
            # RCCL transfers are ordered after.
            ctx.render_rows(params, mode, r0, nrows, d_out=buf.data_ptr(), out_row_base=base, stream=stream.cuda_stream)

        elapsed = sharding.timed_frames(dist, torch, pipe, render, K, Wm, "cuda", torch.cuda.synchronize,
                                        prewarm=prewarm_frames,
                                        min_total=args.min_timed_ms * 1e-3, max_repeats=min(args.max_repeats, 200) if args.full else 1)
        last_frame = K - 1
        slab0 = pipe.slabs[0] if pipe.slabs is not None else None
        exchange_note = "RCCL p2p gather per frame; frame i assembled on rank %s" % ("i % N" if args.root == "rotate" else "0")
    wins = getattr(pipe, "timed_windows", [elapsed])
    timing = {"method": "wall clock around exactly K frames, barrier + synchronize on both sides, MAX over ranks" +
                        ("; the window is repeated (each time from a drained pipeline) and the median window reported" if args.full else "; one window"),
              "repeats": len(wins), "timed_ms_total": round(sum(wins) * 1e3, 3),
              "batch_ms": {"median": round(elapsed * 1e3, 5), "min": round(min(wins) * 1e3, 5), "max": round(max(wins) * 1e3, 5)}}
    dist_verified = None
    if args.verify:
        # byte check of the last assembled frame, outside the timed region: its root hashes it (SHA-256 of the
        # whole 20*W*H buffer against the committed golden value); the verdict is reduced to rank 0 as a
        # tri-state: 1 = compared and equal, 0 = compared and different (or the check itself failed),
        # 2 = no golden value for this config / mode, nothing compared
        code = 2
        try:
            if rank == pipe.root_of(last_frame):
                m = _frame_matches_golden(pipe.frame(last_frame).cpu().numpy(), config, args.mode)
                code = 2 if m is None else int(bool(m))
        except Exception as exc:   # a failed check must not lose the measurement, but it must be seen
            sys.stderr.write("bench.py: golden check of frame %d failed on rank %d: %r\n" % (last_frame, rank, exc))
            code = 0
        flag = torch.tensor([code], dtype=torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        dist_verified = {0: False, 1: True}.get(int(flag.item()))   # None: no rank compared anything
    # ---- check rounds, outside the timed region: is every frame that arrives on a root the frame its camera
    # renders?  (a) the send buffers are poisoned and one more round goes through the very path that was timed
    # (graph replays included): a slab that was not rendered again, or exchanged before it was rendered, shows as
    # poison; (b) a round in which every frame has its own camera, queued launch by launch: a slab that lands in the
    # wrong frame or on the wrong root shows.  Each root compares its frames on the GPU with the whole frame it
    # renders itself for the same camera.
    if args.exchange in ("compact", "rounds") and args.verify:
        code = 1
        try:
            qn = q0 + n_rounds
            tmp = torch.empty(20 * W * H, dtype=torch.uint8, device="cuda")

            def frame_is(i, p_i):
                ctx.render_rows(p_i, mode, 0, H, d_out=tmp.data_ptr(), out_row_base=0, stream=stream.cuda_stream,
                                flags=0 if mode >= R.RGB_ASCII else R.RENDER_ZERO_TAIL)
                torch.cuda.synchronize()
                return bool(torch.equal(pipe.frame(i)[:S * W * H], tmp[:S * W * H]))

            for b in range(pipe.nbuf):
                pipe.send[b].fill_(0xEE)
            for r in range(pipe.nbuf):
                pipe.round(qn + r, RF, render_round)
            pipe.drain()
            torch.cuda.synchronize()
            for r in range(pipe.nbuf):
                for f in range(RF):
                    i = (qn + r) * RF + f
                    if pipe.root_of(i) == rank and not frame_is(i, params):
                        sys.stderr.write("bench.py: rank %d: frame %d of a poisoned round differs from the frame rendered in one piece\n" % (rank, i))
                        code = 0
            qn += pipe.nbuf
            cams = [R.camera_params(W, H, pos=(0.03 * f, 0.01 * f, 0.0), rot=(0.0, float(np.float32(np.pi)) + 0.002 * f, 0.0)) for f in range(RF)]

            def render_round_cams(q, b, nframes):
                if rows:
                    ctx.submit_slabs(cams[:nframes], mode, row0, rows, [pipe.unit(b, f).data_ptr() for f in range(nframes)], row0,
                                     [rstreams[f % F].cuda_stream for f in range(nframes)], after=stream.cuda_stream,
                                     flags=R.RENDER_COMPACT if compact else 0)

            pipe.round(qn, RF, render_round_cams)
            pipe.drain()
            torch.cuda.synchronize()
            for f in range(RF):
                i = qn * RF + f
                if pipe.root_of(i) == rank and not frame_is(i, cams[f]):
                    sys.stderr.write("bench.py: rank %d: frame %d (own camera) differs from the frame rendered in one piece\n" % (rank, i))
                    code = 0
            del tmp
        except Exception as exc:
            sys.stderr.write("bench.py: check rounds failed on rank %d: %r\n" % (rank, exc))
            code = 0
        flag = torch.tensor([code], dtype=torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        rounds_ok = bool(flag.item())
        if rounds_ok is False:
            dist_verified = False
        timing["check_rounds"] = {"passed": rounds_ok,
                                  "what": "after the timed region: %d round(s) through the timed path with poisoned send buffers, one round with a camera "
                                          "per frame; every root compares its frames with the same frames rendered in one piece" % pipe.nbuf}
    if latency is not None:
        timing["frame_latency"] = latency
    # per-rank kernel time, measured apart from the pipeline, for the roofline object (--full)
    ctx.synchronize()
    torch.cuda.synchronize()
    kernel_ms = None
    if args.full:
        n_k = max(10, min(K, 50))
        tgt = slab0 if slab0 is not None else pipe.frames[0]
        if isinstance(tgt, list):
            tgt = tgt[0]
        for _ in range(3):
            ctx.render_rows(params, mode, row0, rows, d_out=tgt.data_ptr(), out_row_base=row0 if slab0 is not None else 0,
                            flags=R.RENDER_COMPACT if compact else 0)
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(n_k):
            ctx.render_rows(params, mode, row0, rows, d_out=tgt.data_ptr(), out_row_base=row0 if slab0 is not None else 0,
                            flags=R.RENDER_COMPACT if compact else 0)
        kernel_ms = ctx.timer_stop() / n_k
    kernel = ctx.last_kernel
    torch.cuda.synchronize()
    del pipe
    ctx.close()
    torch.cuda.empty_cache()
    return {"config": config, "elapsed": elapsed, "timing": timing, "verified": dist_verified, "kernel_ms": kernel_ms, "kernel": kernel,
            "exchange_note": exchange_note, "rows": rows, "S_written": 4 if compact else S,
            "W": W, "H": H, "ns": ns, "npl": npl, "seed": seed}


# ---------------------------------------------------------------------------------------------- N > 1, dry (tests)

def run_sharded_dry(args, torch, dist, R, sharding, rank, world, config, K, Wm):
    """The N > 1 loops over gloo with CPU tensors; the CPU oracle renders (there is no GPU): same sharding classes, same
    timing functions, same verification as run_sharded, so that launch, exchange and line assembly can be tested on CPU."""
    import numpy as np
    import oracle as O
    import util as U
    mode = R.MODE_NAMES.index(args.mode)
    S = R.SIZE_RGB if mode >= R.RGB_ASCII else R.SIZE_8BIT
    W, H, ns, npl, seed = R.CONFIGS[config]
    params, sph, pl = R.config_inputs(config)
    sc = O.Scene.from_arrays(sph, pl)
    op = U.oracle_params(params)
    compact = args.exchange == "compact"
    hit_kind = ord("3") if args.mode.endswith("ASCII") else ord("4")
    bounds = sharding.row_bounds(H, world)
    row0, rows = bounds[rank], bounds[rank + 1] - bounds[rank]
    my_slab = O.render(op, sc, mode, row0=row0, rows=rows)[row0 * W * S:(row0 + rows) * W * S]   # every frame is this frame
    my_words = U.records_to_words(my_slab, W, rows, S) if compact and rows else None
    q0 = n_rounds = RF = None
    if args.exchange in ("compact", "rounds"):
        fixed_root = args.root == "fixed"
        roots = [0] if fixed_root else None
        M = 1 if not compact else (args.frames_per_root or 2)

        def finish(q, b, work, mine):
            # stands in for "wait on a side stream, then rtx_expand": words -> records, segment by segment
            work.wait()
            for m, segs in mine:
                words = pipe.recv[b].numpy().view(np.uint32)
                dst = pipe.frames[b][m].numpy()
                for src_px, dst_px, n in segs:
                    dst[dst_px * S:(dst_px + n) * S] = U.words_to_records(words[src_px:src_px + n], S, hit_kind)
            return None

        pipe = sharding.RowShardedRounds(dist, torch, rank, world, W, H, S, "cpu", nbuf=2, frames_per_root=M,
                                         pixel_bytes=4 if compact else None, finish=finish if compact else None, roots=roots)
        RF = pipe.round_frames

        def render_round(q, b, nframes):
            for f in range(nframes):
                if rows:
                    if compact:
                        pipe.unit(b, f).numpy().view(np.uint32)[:] = my_words
                    else:
                        pipe.unit(b, f).numpy()[:] = my_slab

        elapsed, q0 = sharding.timed_rounds(dist, torch, pipe, render_round, K, Wm, "cpu", lambda: None, prewarm=0,
                                            min_total=0.0, max_repeats=1)
        n_rounds = -(-K // RF)
        last_frame = (q0 + n_rounds - 1) * RF + (K - 1 - (n_rounds - 1) * RF)
        exchange_note = "dry: rounds of %d frames over gloo, %s" % (RF, "compact words" if compact else "records")
    else:
        pipe = sharding.RowShardedFrames(dist, torch, rank, world, W, H, S, "cpu", nbuf=2, rotate_root=(args.root == "rotate"))

        def render(buf, r0, nrows, base):
            buf.numpy()[(r0 - base) * W * S:(r0 - base + nrows) * W * S] = my_slab

        elapsed = sharding.timed_frames(dist, torch, pipe, render, K, Wm, "cpu", lambda: None, prewarm=0, min_total=0.0, max_repeats=1)
        last_frame = K - 1
        exchange_note = "dry: p2p gather per frame over gloo"
    wins = getattr(pipe, "timed_windows", [elapsed])
    timing = {"method": "dry run: wall clock around K frames of CPU copies over gloo; not a measurement", "repeats": len(wins),
              "timed_ms_total": round(sum(wins) * 1e3, 3),
              "batch_ms": {"median": round(elapsed * 1e3, 5), "min": round(min(wins) * 1e3, 5), "max": round(max(wins) * 1e3, 5)}}
    code = 2
    if args.verify:
        if rank == pipe.root_of(last_frame):
            m = _frame_matches_golden(pipe.frame(last_frame).numpy(), config, args.mode)
            code = 2 if m is None else int(bool(m))
    flag = torch.tensor([code], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    verified = {0: False, 1: True}.get(int(flag.item()))
    return {"config": config, "elapsed": elapsed, "timing": timing, "verified": verified, "kernel_ms": None, "kernel": "oracle (dry run)",
            "exchange_note": exchange_note, "rows": rows, "S_written": 4 if compact else S,
            "W": W, "H": H, "ns": ns, "npl": npl, "seed": seed}


def sharded_record(args, r, n_gpus, K, Wm):
    """The line (or sub-record) of one configuration from run_sharded's result."""
    W, H, ns, npl = r["W"], r["H"], r["ns"], r["npl"]
    rays_per_frame = (W - 1) * H
    mrays = rays_per_frame * K / r["elapsed"] / 1e6
    g = golden().get("%s_%s" % (r["config"], args.mode), {})
    hit_frac = (g.get("foreground_pixels") or 0) / float(rays_per_frame)
    roofline = None
    if r["kernel_ms"]:
        # rank 0's slab launch: the trace kernel of a rank writes S bytes per pixel, or 4 when the slabs travel as pixel words
        roofline = roofline_object(r["config"], args.mode, r["kernel"], W, H, r["S_written"], ns, npl, r["rows"], r["kernel_ms"], hit_frac)
        roofline["kernel_ms_note"] = "rank 0's slab launch (%d rows) alone on one stream, HIP events" % r["rows"]
    return {
        "value": round(mrays, 3), "unit": "Mrays/s", "n_gpus": n_gpus, "steps": K, "warmup": Wm,
        "ms_per_step": round(r["elapsed"] / K * 1e3, 5),
        "config": {"workload": "%s: %dx%d, %d spheres + %d planes, mode %s, SURVEY App. D scene seed %d"
                               % (r["config"], W, H, ns, npl, args.mode, r["seed"]),
                   "rays_per_frame": rays_per_frame, "kernel": r["kernel"], "prewarm_ms": args.prewarm_ms,
                   "rows_per_rank": r["rows"],
                   "parallelism": "rows sharded over %d GPUs; %s" % (n_gpus, r["exchange_note"])},
        "timing": r["timing"], "roofline": roofline, "verified_against_golden": r["verified"],
    }


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    force_dist = os.environ.get("RTX_BENCH_FORCE_DIST") == "1"
    if args.dump_outputs and not args.native and (args.gpus > 1 or force_dist):
        raise SystemExit("--dump-outputs: N = 1 and --native only")
    if args.native:
        # one process drives every GPU through a device group: no launcher, no torch.distributed
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the ray-trace path has no CPU fallback")
        R = importlib.import_module(PKG)
        devices = [int(v) for v in args.native_devices.split(",")] if args.native_devices else list(range(max(1, args.gpus)))
        rec = run_native(args, torch, R, devices, args.config, args.steps, args.warmup, args.prewarm_ms, update_leg=args.full)
        out = {"metric": BASELINE_METRIC}
        out.update(rec)
        out.update({"higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic"})
        if args.cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_leg(args.config, R.MODE_NAMES.index(args.mode), args.cpu_threads)
            out["speedup_vs_cpu_baseline"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
        print(json.dumps(out))
        return 0
    if (args.gpus > 1 or force_dist) and "WORLD_SIZE" not in os.environ:
        # no launcher around us: be the launcher (a parent that never touches the GPU)
        return self_launch(args, argv)

    # dmabuf IPC (RCCL across processes needs it on this driver); before anything initialises HIP
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = args.gpus
    # RTX_BENCH_FORCE_DIST=1 with one rank walks the N>1 code (RCCL init, rings, all-reduce of the time) on a one-GPU
    # box; the numbers it prints are not a bench line
    distributed = world > 1 or force_dist
    if distributed and world != n_gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (n_gpus, world))
    if args.dry and not distributed:
        raise SystemExit("--dry is the N>1 loop over gloo: use --gpus 2 or more")
    if not args.dry and not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the ray-trace path has no CPU fallback")
    if distributed and args.what != "trace":
        raise SystemExit("--what %s is N=1 only" % args.what)

    R = importlib.import_module(PKG)
    K, Wm = args.steps, args.warmup
    if not distributed:
        torch.cuda.set_device(0)
        out = run_single(args, torch, R)
        print(json.dumps(out))
        return 0

    import torch.distributed as dist
    sharding = importlib.import_module(PKG + ".sharding")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if args.dry:
        dist.init_process_group(backend="gloo")
    else:
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    subs = args.sub_configs
    if subs is None:
        subs = "C4" if (args.full and args.config == "C2" and not args.dry and args.exchange != "p2p") else ""
    subs = [s for s in subs.split(",") if s and s.lower() != "none"]
    for s in subs:
        if s not in R.CONFIGS:
            raise SystemExit("--sub-configs: unknown config %r" % s)
    results = []
    for i, cfg in enumerate([args.config] + subs):
        if args.dry:
            results.append(run_sharded_dry(args, torch, dist, R, sharding, rank, world, cfg, K, Wm))
        else:
            W, H = R.CONFIGS[cfg][0], R.CONFIGS[cfg][1]
            # the run-in that brings an idle GPU to its clocks: --prewarm-ms of frames at ~25 us per 1080p frame on one GPU;
            # sub-records run on a warm GPU and take a tenth of it
            frames = int(args.prewarm_ms * 40 * (1920.0 * 1080.0) / (W * H)) if i == 0 else int(args.prewarm_ms * 4 * (1920.0 * 1080.0) / (W * H))
            results.append(run_sharded(args, torch, dist, R, sharding, rank, world, local_rank, cfg, K, Wm, max(0, frames)))
    dist.barrier()
    dist.destroy_process_group()
    if rank != 0:
        return 0
    main_rec = sharded_record(args, results[0], n_gpus, K, Wm)
    out = {"metric": BASELINE_METRIC}
    out.update(main_rec)
    out.update({"higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic"})
    if args.dry:
        out["dry"] = True
        out["data"] = "synthetic (dry run: CPU oracle as the renderer over gloo; not a measurement)"
    # the CPU baseline of the main workload: rank 0, now that the ranks are done (it must not sit inside anyone's timed region)
    cpu = None
    if args.cpu_baseline:
        cpu = cpu_baseline_leg(args.config, R.MODE_NAMES.index(args.mode), args.cpu_threads)
        out["speedup_vs_cpu_baseline"] = round(out["value"] / cpu["value"], 1)
    out["cpu_baseline"] = cpu
    if args.full and not args.dry and not args.no_native_leg:
        # the same sharded frame behind the C ABI: ONE process (this one) drives all N GPUs through a device group, now that
        # the other ranks have let go of theirs.  A sub-record beside the torch.distributed line, never the line's value.
        # In a child process with a time limit: the RCCL form of the gather between distinct GPUs has only ever run at one device
        # on the boxes this was built on, and a sub-record must lose neither the line nor the driver's patience.
        try:
            devs = list(range(n_gpus)) if torch.cuda.device_count() >= n_gpus else [0] * n_gpus
            cmd = [sys.executable, os.path.abspath(__file__), "--native", "--gpus", str(n_gpus), "--native-devices", ",".join(str(d) for d in devs),
                   "--config", args.config, "--mode", args.mode, "--steps", str(K), "--warmup", str(Wm), "--prewarm-ms", str(min(args.prewarm_ms, 50.0)),
                   "--full", "--no-cpu-baseline", "--min-timed-ms", str(args.min_timed_ms)] + (["--no-verify"] if args.no_verify else [])
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK")}
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=env)
            line = next((ln for ln in proc.stdout.splitlines()[::-1] if ln.strip().startswith("{")), None)
            if proc.returncode == 0 and line:
                rec = json.loads(line)
                rec.pop("metric", None)
                out["native_group"] = rec
            else:
                out["native_group"] = {"error": "exit code %d: %s" % (proc.returncode, (proc.stderr or "").strip()[-400:])}
        except Exception as exc:   # (a sub-record must not lose the line)
            sys.stderr.write("bench.py: native_group leg failed: %r\n" % (exc,))
            out["native_group"] = {"error": repr(exc)}
    if subs:
        out["configs"] = {}
        for r in results[1:]:
            rec = sharded_record(args, r, n_gpus, K, Wm)
            rec["metric"] = "Mrays/s (primary rays), same loop, BASELINE config %s" % r["config"]
            out["configs"][r["config"]] = rec
    # key order of the contract first (readability only)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
