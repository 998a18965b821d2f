"""A context's whole life, twelve times over in one process: create, touch every owner that is created on first use, destroy.

Everything a context allocates on the device -- memory, pinned words, events, streams -- belongs to an owning type of csrc/rtx_mem.hpp
and goes when rtx_destroy deletes the context.  A leak, or a free that a queued launch still reads, renders a correct frame, so no
other test sees either; this one checks that
  * every call of every iteration succeeds and every frame, stream and query answer of iteration k equals iteration 1's byte for byte,
  * the direct path's frames and rtx_update's streams equal tests/oracle.py's (the modes the oracle covers),
  * the device's free memory (torch.cuda.mem_get_info, the device-wide figure) after the last rtx_destroy is not below what it was
    after the first by more than MARGIN.

The frames are 48 x 24 and then 96 x 40, so that every per-size buffer is outgrown once; the scene has 300 spheres and 2 planes, above
the 256 at which the sorted store and a dense view's two-level culling engage.  A dispatch-order set needs a grid of at least two
workgroups per compute unit (rtx_render.cpp, dispatch_order_args: 512 tiles of 256 pixels on this device), which neither size has:
that one step renders a 640 x 256 frame.

MARGIN.  Twice the largest drift (free memory after the first rtx_destroy minus free memory after the last) that the same loop
shows on the commit before the owning types, whose rtx_destroy freed everything by hand, field by field.  Three runs of it on one MI355X:
    drift 0, 0 and 0 bytes (308 356 841 472 bytes free after the first destroy and after the twelfth, in each run),
so the margin is 0: the runtime gives a context's memory back in full, and nothing else moved the device-wide figure during the 3 s
of a run.  One context's footprint (free memory before rtx_create minus free memory at the end of its life) was 27 262 976 bytes
(205 520 896 in the first life of a process, which brings up the runtime's own pools and code objects): the check sees a leak of a
frame-sized buffer many times over; what it cannot see is a leak smaller than the granularity the runtime takes device memory in.
This build: drift 0.  (profiles/r19_ownership_ab.txt)
"""
import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

SIZES = [(48, 24), (96, 40)]
ORDER_SIZE = (640, 256)
N_SPHERES, N_PLANES, SEED = 300, 2, 19
ITERATIONS = 12
MARGIN = 0


def _scene(R):
    p = R.camera_params(*SIZES[1])
    return R.synth_scene(SEED, N_SPHERES, N_PLANES, p.element1, p.element2)


def _lights(R):
    return [R.make_light(pos=(1.0, 50.0, 0.0)), R.make_light(pos=(-30.0, 40.0, 60.0), diffuse_power=1500.0, specular_power=2000.0)]


def _life(R, torch, sph, pl, dev, streams, out):
    """One context's life; out[name] = bytes of every result.  Returns the context's footprint in bytes of device memory."""
    free_before = torch.cuda.mem_get_info()[0]
    c = R.Context(*ORDER_SIZE)
    try:
        c.set_scene(sph, pl)
        s0, s1 = streams

        def frame(tag, p, mode, stream=None, flags=0):
            W, H = int(p.x), int(p.y)
            n = (4 if flags & R.RENDER_COMPACT else 20) * W * H
            dev[:n].fill_(0xEE)
            torch.cuda.synchronize()
            c.render_rows(p, mode, 0, H, d_out=dev.data_ptr(), out_row_base=0, stream=stream, flags=flags)
            torch.cuda.synchronize()
            out[tag] = dev[:n].cpu().numpy().tobytes()

        for W, H in SIZES:
            p = R.camera_params(W, H)
            t = "%dx%d " % (W, H)
            # the direct path: the context's own frame, then a recorded graph of it into the caller's buffer, replayed once
            c.set_option(R.OPT_TWO_LEVEL, 0)
            out[t + "direct"] = c.render_to_host(p, R.RGB_ASCII).tobytes()
            frame(t + "direct 8-bit", p, R.BIT_ASCII, s0.cuda_stream, R.RENDER_ZERO_TAIL)
            c.render_rows(p, R.RGB_ASCII, 0, H, d_out=dev.data_ptr(), out_row_base=0, stream=s0.cuda_stream)
            torch.cuda.synchronize()
            c.graph_begin(s0.cuda_stream)
            c.render_rows(p, R.RGB_ASCII, 0, H, d_out=dev.data_ptr(), out_row_base=0, stream=s0.cuda_stream)
            g = c.graph_end(s0.cuda_stream)
            dev[:20 * W * H].fill_(0xEE)
            torch.cuda.synchronize()
            c.graph_launch(g, s0.cuda_stream)
            torch.cuda.synchronize()
            out[t + "graph"] = dev[:20 * W * H].cpu().numpy().tobytes()
            c.graph_destroy(g)
            # shadows from two lights; mirrors two bounces deep with shadows at every reflected hit; shadow tests through the world grid
            c.set_option(R.OPT_SHADOWS, 1)
            c.set_lights(_lights(R))
            frame(t + "shadows", p, R.RGB_ASCII, s0.cuda_stream)
            c.set_reflectivity(0, [0.5 if i % 3 == 0 else 0.0 for i in range(N_SPHERES)] + [0.4, 0.0])
            c.set_option(R.OPT_REFLECT_DEPTH, 2)
            c.set_option(R.OPT_REFLECT_SHADOWS, 1)
            frame(t + "mirrors", p, R.RGB_ASCII, s1.cuda_stream)
            out[t + "mirror stats"] = repr([c.get_option(R.STAT_REFLECT_RAYS + k) for k in range(2)] +
                                           [c.get_option(R.STAT_REFLECT_SHADOW_POINTS + k) for k in range(2)]).encode()
            c.set_option(R.OPT_SHADOW_GRID, 1)
            frame(t + "mirrors grid", p, R.RGB_ASCII, s0.cuda_stream)
            c.set_reflectivity(0, [0.0] * (N_SPHERES + N_PLANES))
            frame(t + "shadows grid", p, R.BIT_PIXEL, s1.cuda_stream, R.RENDER_ZERO_TAIL)
            assert c.get_option(R.STAT_SHADOW_GRID_FRAMES) > 0
            c.set_option(R.OPT_SHADOW_GRID, 0)
            c.set_option(R.OPT_REFLECT_SHADOWS, 0)
            c.set_option(R.OPT_REFLECT_DEPTH, 1)
            c.set_option(R.OPT_SHADOWS, 0)
            c.set_light(None)
            # ray queries: from host memory (a temporary device buffer), from device memory on a render stream, and rtx_pick
            rays = R.make_rays([[0.0, 0.0, 0.0]] * 64, [[0.02 * (i % 8) - 0.07, 0.02 * (i // 8) - 0.07, 1.0] for i in range(64)])
            out[t + "query"] = c.query_rays(rays).tobytes()
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
            d_hits = torch.zeros(64 * 8, dtype=torch.uint8, device="cuda")
            c.query_rays_device(64, d_rays.data_ptr(), d_hits.data_ptr(), R.QUERY_ANY, s1.cuda_stream)
            torch.cuda.synchronize()
            out[t + "query any"] = d_hits.cpu().numpy().tobytes()
            out[t + "pick"] = repr(c.pick(p, W // 2, H // 2)).encode()
            # two-level culling on two render streams: lists that outlive a frame (built, prefetched, reused), then binned per frame
            c.set_option(R.OPT_TWO_LEVEL, 1)
            for reuse in (1, 0):
                c.set_option(R.OPT_CELL_REUSE, reuse)
                for k in range(4):
                    frame(t + "two-level reuse %d frame %d" % (reuse, k), p, R.RGB_ASCII, (s0, s1)[k & 1].cuda_stream)
            c.set_option(R.OPT_CELL_REUSE, -1)
            c.set_option(R.OPT_TWO_LEVEL, 0)
            # Update: blocking and pipelined, from pixel words and from records; then delta frames
            for words in (1, 0):
                c.set_option(R.OPT_UPDATE_WORDS, words)
                out[t + "update words %d" % words] = c.update(p, R.RGB_ASCII).tobytes()
                host = [c.host_alloc(20 * W * H) for _ in range(2)]
                try:
                    tickets = [c.update_begin(p, (R.RGB_ASCII, R.BIT_ASCII)[k], host[k][0]) for k in range(2)]
                    for k in range(2):
                        n = c.update_end(tickets[k])
                        out[t + "pipelined words %d slot %d" % (words, k)] = host[k][1][:n].tobytes()
                finally:
                    for ptr, _ in host:
                        c.host_free(ptr)
            c.set_option(R.OPT_UPDATE_WORDS, -1)
            for k in range(3):
                s, kind = c.update_delta(R.camera_params(W, H, pos=(0.25 * k, 0.0, 0.0)), R.RGB_ASCII)  # (the scene stays: the oracle has no physics here)
                assert kind == (R.DELTA_KEY if k == 0 else R.DELTA_DIFF)
                out[t + "delta %d" % k] = s.tobytes()
            out[t + "delta stats"] = repr([c.get_option(o) for o in (R.STAT_DELTA_FRAMES, R.STAT_DELTA_KEYFRAMES, R.STAT_DELTA_CELLS, R.STAT_DELTA_RUNS)]).encode()
        # a dispatch-order set and its pass: a grid of two workgroups per compute unit or more
        p = R.camera_params(*ORDER_SIZE)
        c.set_option(R.OPT_KERNEL, R.KERNEL_BINNED)
        c.set_option(R.OPT_TILE_ORDER, 1)
        for k in range(3):
            frame("order frame %d" % k, p, R.RGB_ASCII, s0.cuda_stream)
        assert c.get_option(R.STAT_ORDER_PASSES) > 0
        c.set_option(R.OPT_TILE_ORDER, -1)
        c.set_option(R.OPT_KERNEL, R.KERNEL_AUTO)
        # an edit in place from host rows, a removal (spheres and a plane: the second set of arrays, the lists), and the frame after each
        p = R.camera_params(*SIZES[1])
        rows = sph[10:20].copy()
        rows[:, 0] += 1.5
        rows[:, 4:7] = 200.0
        c.set_spheres(10, rows)
        out["edited"] = c.render_to_host(p, R.RGB_ASCII).tobytes()
        c.remove_objects([3, 7, 150, N_SPHERES + 1])
        assert c.object_count == N_SPHERES + N_PLANES - 4
        out["removed"] = c.render_to_host(p, R.RGB_ASCII).tobytes()
        marks = torch.zeros(c.object_count, dtype=torch.uint8, device="cuda")
        marks[5] = 1
        torch.cuda.synchronize()
        assert c.remove_marked_device(marks.data_ptr()) == 1
        out["removed marked"] = c.update(p, R.BIT_ASCII).tobytes()
        torch.cuda.synchronize()
        return free_before - torch.cuda.mem_get_info()[0]
    finally:
        c.close()


def test_twelve_lives_of_a_context_leave_the_same_bytes_and_the_same_free_memory():
    import torch
    R = U.pkg()
    sph, pl = _scene(R)
    dev = torch.empty(20 * ORDER_SIZE[0] * ORDER_SIZE[1], dtype=torch.uint8, device="cuda")
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    first, free_after, footprints = None, [], []
    for k in range(ITERATIONS):
        out = {}
        footprints.append(_life(R, torch, sph, pl, dev, streams, out))
        torch.cuda.synchronize()
        free_after.append(torch.cuda.mem_get_info()[0])
        if first is None:
            first = out
            continue
        assert sorted(out) == sorted(first)
        for name in first:
            assert out[name] == first[name], "iteration %d: %s differs from iteration 1: %s" % (
                k + 1, name, U.first_diff(np.frombuffer(out[name], np.uint8), np.frombuffer(first[name], np.uint8), 20, 1))
    # against the oracle, where it covers the mode: the direct path and Update
    sc = O.Scene.from_arrays(sph, pl)
    for W, H in SIZES:
        p = R.camera_params(W, H)
        t = "%dx%d " % (W, H)
        want = O.render(U.oracle_params(p), sc, O.RGB_ASCII)
        for name in ("direct", "graph"):
            got = np.frombuffer(first[t + name], np.uint8)
            assert np.array_equal(got, want), "%s%s: %s" % (t, name, U.first_diff(got, want, 20, W))
        want8 = O.render(U.oracle_params(p), sc, O.BIT_ASCII)
        got = np.frombuffer(first[t + "direct 8-bit"], np.uint8)
        assert np.array_equal(got, want8), "%sdirect 8-bit: %s" % (t, U.first_diff(got, want8, 12, W))
        mini = O.minimize(O.RGB_ASCII, want, W, H).tobytes()
        for name in ("update words 1", "update words 0", "pipelined words 1 slot 0", "pipelined words 0 slot 0", "delta 0"):
            assert first[t + name] == mini, t + name
        mini8 = O.minimize(O.BIT_ASCII, want8, W, H).tobytes()
        for name in ("pipelined words 1 slot 1", "pipelined words 0 slot 1"):
            assert first[t + name] == mini8, t + name
        # two-level culling, the tile passes and the recorded graph change how a frame is computed, never the frame
        for name in first:
            if name.startswith(t + "two-level"):
                assert first[name] == first[t + "direct"], name
    drift = free_after[0] - free_after[-1]
    print("lifecycle: free after destroy 1 / %d: %d / %d bytes, drift %d, footprint of a context %d .. %d, margin %d" % (
        ITERATIONS, free_after[0], free_after[-1], drift, min(footprints), max(footprints), MARGIN))
    assert drift <= MARGIN, "device memory free after the last rtx_destroy is %d bytes below what it was after the first (margin %d)" % (drift, MARGIN)
