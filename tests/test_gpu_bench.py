"""bench.py as a pull request's checks run it: the plain command does what its headline figure needs and nothing beside it, `--full`
is where every figure with a run of its own lives."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("configs", "gpu_inlined", "cpu_baseline")     # blocks of the line that only a --full run measures


def test_a_plain_run_is_lean_and_keeps_the_headline_keys():
    """`bench.py --gpus 1 --steps N --warmup W` at the BASELINE size, in a new process: the whole run, start to exit, less (N + W) x
    ms_per_step stays within 30 s (set-up, the first step's compiling or tuning and the result line included), the line keeps the
    headline keys with today's meaning and carries none of the figures that moved behind --full."""
    N, W = 20, 5
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(N), "--warmup", str(W)],
                         capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    outside = wall - (N + W) * d["ms_per_step"] / 1e3
    print("plain run: %.1f s in all, %.3f ms per step, %.1f s outside its %d steps" % (wall, d["ms_per_step"], outside, N + W))
    assert d["metric"] == "leapfrog steps/sec (all chains)" and d["unit"] == "leapfrog steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == N and d["warmup"] == W and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 32 * 1024) <= 1e-6 * 32 * 1024      # one step = L x chains leapfrog steps
    assert not any(k in d for k in MOVED) and d["ess_per_s"] is None and d["ess_leg"] is None and d["ess_leg_identity_mass"] is None
    assert not str(d["roofline"].get("traffic_source", "")).startswith("measured in this run")
    assert d["roofline"]["launches"] > 0 and 0 < d["roofline"]["frac"] < 1            # (from the timed steps' own events)
    assert outside <= 30.0, (wall, d["ms_per_step"], outside)
