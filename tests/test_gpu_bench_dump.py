"""A plain bench.py run (no --full) with --dump-outputs: one JSON line with the headline fields
and none of the --full legs, and the last timed step's outputs as .npy files (f32 / f64, under
64 MB).  C2 (GridWorld, 20,000 particles) is the smallest workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_last_step_outputs(cuda, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--workload", "C2", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True,
                         text=True, timeout=280, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["unit"] == "s/epoch"
    assert rec["dtype"] == "f64" and rec["higher_is_better"] is False
    assert rec["ms_per_step"] == pytest.approx(rec["value"] * 1e3, abs=1e-3) and rec["value"] > 0
    assert "cpu_baseline" not in rec and "roofline_iteration" not in rec
    assert "traffic_per_kernel" not in rec["roofline"]

    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    N, k = 20 * 1000, 4
    assert got["knn_distances"].shape == got["knn_indices"].shape == (N, k + 1)
    assert got["knn_indices"].min() >= 0 and got["knn_indices"].max() < N
    assert np.all(got["knn_distances"][:, 0] == 0) and np.all(np.diff(got["knn_distances"]) >= 0)
    assert got["rollout_states"].shape == (20, 1001, 2)
    assert got["rollout_actions"].shape == (20, 1000, 2)
    # H is -inf where the walls pile particles onto one point (d_k = 0), as in the reference
    assert got["final_entropy"].shape == () and not np.isnan(got["final_entropy"])
    assert 0 <= got["off_policy_iters"] <= 30
    params = [n for n in got if n.startswith("policy.")]
    assert params and all(np.isfinite(got[n]).all() for n in params)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
