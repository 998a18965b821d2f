"""bench.py on the GPU, as the driver runs it: a plain run times exactly the K steps it is given, and --dump-outputs writes
what the last timed step computed -- here checked against the committed golden hashes of config 1."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_line(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RTX_BENCH_FORCE_DIST")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(argv), cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_frame(tmp_path):
    d = _bench_line("--config", "C1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["timing"]["repeats"] == 1
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["verified_against_golden"] is None
    assert "modes" not in d and "end_to_end" not in d and "moving_view" not in d["timing"]
    W, H, S = 320, 180, 20
    recs = np.load(tmp_path / "frame_records.npy")
    assert recs.dtype == np.float32 and recs.shape == (W * H, S)      # small enough to be written whole
    frame = recs.astype(np.uint8).reshape(-1)
    assert hashlib.sha256(frame.tobytes()).hexdigest() == U.load_golden()["C1_RGB_ASCII"]["frame_sha256"]


def test_update_run_dumps_the_minimised_stream(tmp_path):
    _bench_line("--config", "C1", "--what", "update", "--steps", "5", "--warmup", "1", "--dump-outputs", str(tmp_path))
    stream = np.load(tmp_path / "update_stream.npy")
    gold = U.load_golden()["C1_RGB_ASCII"]
    assert stream.dtype == np.float32 and stream.shape == (gold["minimized_bytes"], 1)
    assert O.fnv1a64(stream.astype(np.uint8).reshape(-1)) == gold["minimized_fnv1a64"]
