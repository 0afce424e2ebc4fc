"""`bench.py` on the MI355X: a plain run (no `--full`) prints the headline line only, dumps the last timed step's
trajectory and gradients, and spends little time outside its warm-up and timed steps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from test_bench_dist import HEADLINE_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, D = 10000, 100, 12
OVERHEAD_LIMIT_S = 30.0   # a plain run: set-up, pre-conditioning, dump and exit together


@pytest.mark.gpu
def test_a_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    steps, warmup = 20, 5
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(dump)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert list(out) == HEADLINE_KEYS
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert out["value"] == pytest.approx(N * 1e3 / out["ms_per_step"], rel=1e-9)
    shapes = {"h": (T, N, D), "grad_y0": (N, D), "grad_w": (D - 4, D), "grad_b": (D - 4,), "grad_theta": (16,)}
    assert sorted(os.listdir(dump)) == sorted(k + ".npy" for k in shapes)
    for k, shape in shapes.items():
        a = np.load(dump / (k + ".npy"))
        assert a.shape == shape and a.dtype == np.float32 and np.isfinite(a).all(), k
    outside = wall - (steps + warmup) * out["ms_per_step"] * 1e-3
    assert outside < OVERHEAD_LIMIT_S, "plain run spent %.1f s outside its steps" % outside
