"""bench.py without --full: the headline line alone (no extra legs, roofline steps or CPU baseline), the number of timed steps
--steps asks for, and --dump-outputs: the loss, parameters and gradients of the last timed step as float .npy files under 64 MB,
the same from run to run on the same arguments (seeded inputs and weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--config", "A",
           "--batch-per-gpu", "2", "--mask-ratio", "0.5", "--dump-outputs", str(out_dir)]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GDMAE_BENCH_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = _plain_run(a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["optimizer_steps_timed"] == 3                              # counted by the optimizer, not echoed
    assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) <= 0.01 * out["value"]       # frames/s and ms per step of the same steps
    for k in ("also", "roofline", "cpu_baseline", "kernel_time_shares_profiling_box"):
        assert k not in out, k                                                        # --full only
    assert out["host_issue_ms_idle_device"] is None

    files = sorted(os.listdir(a))
    assert files == ["grads.npy", "loss.npy", "params.npy"]
    arrs = {f[:-4]: np.load(a / f) for f in files}
    assert sum(os.path.getsize(a / f) for f in files) <= 64e6
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in arrs.values())
    assert arrs["loss"].shape == (1,) and abs(float(arrs["loss"][0]) - out["config"]["loss_last"]) <= 1e-4 * abs(out["config"]["loss_last"]) + 1e-5
    assert arrs["params"].shape == arrs["grads"].shape and float(np.abs(arrs["grads"]).sum()) > 0

    _plain_run(b)                                            # same arguments: same inputs, so the same outputs up to fp32 round-off
    for k, v in arrs.items():
        w = np.load(b / f"{k}.npy")
        assert w.shape == v.shape and w.dtype == v.dtype, k
        assert np.allclose(w, v, rtol=1e-3, atol=1e-3 * float(np.abs(v).max()) + 1e-12), k
