"""Rates of the ray queries on one GPU (one JSON line per figure).

Scenes C2, C3 and C5; ray sets as tests/test_gpu_query.py draws them: (a) the camera's primary rays of a 1080p frame, (b) random
origins in twice the scene box with random directions, (c) origins on sphere surfaces with mirrored directions and the sphere
skipped.  2^21 rays per set (a 1080p frame has 2.07 M pixels).  Per scene and set: the grid kernel and the brute kernel
(RTX_OPT_QUERY_CHECK 1) through the device-pointer form on a stream of the caller, warmed up, then timed with device events around
`reps` launches (the median of `batches` batches; the brute kernel on C5 takes one launch per batch); the grid's build apart, as
the host time of a query that rebuilds (the grid load set to another value and back before it) less that of one that does not.  --loads repeats the
grid figures of sets (b) and (c) for other grid loads (RTX_OPT_QUERY_LOAD, sixteenths of a sphere per cell).  Counters come from
separate runs, e.g.

    rocprofv3 --kernel-trace --stats -d query_prof -o run -- python tools/query_gpu.py --configs C5 --sets c --no-brute --reps 5 --batches 2
    rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY -d query_pmc -o run -- python tools/query_gpu.py ...

Usage: python tools/query_gpu.py [--configs C2,C3,C5] [--sets a,b,c] [--reps 20] [--batches 5] [--loads 8,16,32,64,128] [--no-brute] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = importlib.import_module("raytracing-in-windows-console_amd")

N = 1 << 21


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def primary(p, pix):
    f32 = np.float32
    W, H = int(p.x), int(p.y)
    col, row = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
    m = np.array(p.inv_v[:], dtype=np.float32)
    vx = (((f32(2.0) * col) - f32(W)) / f32(W)) * f32(p.element1)
    vy = ((f32(H) - row * f32(2.0)) / f32(H)) * f32(p.element2)
    w = [((m[4 * k] * vx + m[4 * k + 1] * vy) + m[4 * k + 2]) + m[4 * k + 3] * f32(0.0) for k in range(3)]
    inv = f32(1.0) / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    o = np.tile(np.array(p.cam_pos[:], dtype=np.float32), (len(pix), 1))
    return R.make_rays(o, np.stack([w[k] * inv for k in range(3)], -1), tmax=f32(p.cam_far))


def ray_set(which, sph, rng, n):
    lo = (sph[:, :3] - sph[:, 3:4]).min(0).astype(np.float64)
    hi = (sph[:, :3] + sph[:, 3:4]).max(0).astype(np.float64)
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    if which == "a":  # in frame order: neighbouring lanes hold neighbouring pixels
        p = R.camera_params(1920, 1080)
        return primary(p, np.arange(n) % (1920 * 1080))
    if which == "b":
        return R.make_rays(ctr + rng.uniform(-2, 2, (n, 3)) * half, unit(rng, n) * rng.uniform(0.2, 5.0, (n, 1)))
    if which == "c":
        j = rng.integers(0, len(sph), n)
        nrm = unit(rng, n)
        o = sph[j, :3].astype(np.float64) + nrm * sph[j, 3:4]
        v = unit(rng, n)
        v = np.where((np.einsum("nk,nk->n", v, nrm) > 0)[:, None], -v, v)
        return R.make_rays(o, v - 2 * np.einsum("nk,nk->n", v, nrm)[:, None] * nrm, skip=j.astype(np.uint32))
    raise ValueError(which)


def timed(c, n, d_rays, d_hits, stream, reps, batches):
    for _ in range(2):
        c.query_rays_device(n, d_rays.data_ptr(), d_hits.data_ptr(), R.QUERY_CLOSEST, stream.cuda_stream)
    stream.synchronize()
    per = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            c.query_rays_device(n, d_rays.data_ptr(), d_hits.data_ptr(), R.QUERY_CLOSEST, stream.cuda_stream)
        e1.record(stream)
        stream.synchronize()
        per.append(e0.elapsed_time(e1) / reps)
    return float(np.median(per)), float(min(per)), float(max(per))


def build_ms(c, rays, batches):
    """host time of a small query that rebuilds less that of one that does not (both end in a wait for the device)"""
    small = rays[:1024]
    with_build, without = [], []
    load = c.get_option(R.OPT_QUERY_LOAD)
    for _ in range(batches):
        c.set_option(R.OPT_QUERY_LOAD, 4000)  # (a change of the load marks the grid for a rebuild; back to the load in force: the same grid again)
        c.set_option(R.OPT_QUERY_LOAD, load)
        c.synchronize()
        t0 = time.perf_counter()
        c.query_rays(small)
        with_build.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        c.query_rays(small)
        without.append(time.perf_counter() - t0)
    return 1e3 * (float(np.median(with_build)) - float(np.median(without)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--sets", default="a,b,c")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--loads", default="")
    ap.add_argument("--no-brute", action="store_true")
    ap.add_argument("--rays", type=int, default=N)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on a CPU")
    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    stream = torch.cuda.Stream()
    with R.Context(1920, 1080) as c:
        for name in a.configs.split(","):
            p, sph, pl = R.config_inputs(name)
            c.set_scene(sph, pl)
            rng = np.random.default_rng(21)
            for which in a.sets.split(","):
                rays = ray_set(which, sph, rng, a.rays)
                n = len(rays)
                d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
                d_hits = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                loads = [0] + [int(x) for x in a.loads.split(",") if x and which in "bc"]
                for load in loads:
                    c.set_option(R.OPT_QUERY_CHECK, 0)
                    c.set_option(R.OPT_QUERY_LOAD, load)
                    med, lo, hi = timed(c, n, d_rays, d_hits, stream, a.reps, a.batches)
                    hits = d_hits.cpu().numpy().view(R.RAY_HIT_DTYPE)
                    emit({"config": name, "set": which, "kernel": "grid", "load_16ths": load, "rays": n, "ms": round(med, 4), "ms_min": round(lo, 4),
                          "ms_max": round(hi, 4), "mrays_per_s": round(n / med / 1e3, 1), "hit_share": round(float((hits["index"] != R.NO_OBJECT).mean()), 4),
                          "fallback_rays": c.get_option(R.STAT_QUERY_FALLBACK_RAYS), "cells": c.get_option(R.STAT_QUERY_GRID_CELLS),
                          "pairs": c.get_option(R.STAT_QUERY_GRID_PAIRS), "large": c.get_option(R.STAT_QUERY_LARGE_SPHERES), "spheres": len(sph),
                          "build_ms": round(build_ms(c, rays, a.batches), 3)})
                c.set_option(R.OPT_QUERY_LOAD, 0)
                if not a.no_brute:
                    c.set_option(R.OPT_QUERY_CHECK, 1)
                    heavy = len(sph) > 8192
                    med, lo, hi = timed(c, n, d_rays, d_hits, stream, 1 if heavy else max(1, a.reps // 4), 3 if heavy else a.batches)
                    c.set_option(R.OPT_QUERY_CHECK, 0)
                    emit({"config": name, "set": which, "kernel": "brute", "rays": n, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "mrays_per_s": round(n / med / 1e3, 1), "sphere_tests_per_s": round(n * len(sph) / med * 1e3, 0), "spheres": len(sph)})
    if out:
        out.close()


if __name__ == "__main__":
    main()
