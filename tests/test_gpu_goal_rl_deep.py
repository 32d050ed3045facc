"""TRPO's goal sampler for policies with 3 to 6 hidden layers, from the gate
(kernel_path.goal_sampler) through collect_sample_batch and trpo() to the goal_rl command line.
The sampled arrays are checked against the un-terminated ops.rollout_deep rollout cut by
goal_rl_cases (first_hit, truncate, budget), as test_gpu_goal_rl.py checks the two-layer sampler
against the oracle's."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_gpu_goal_rl import BATCH, ROUND, T, _expected_sample, _goal_env, _sample_with_pool
from test_gpu_rollout_deep_goal import NT, _case

pytestmark = pytest.mark.gpu


# ---- 7. the gate -----------------------------------------------------------------------------
def test_goal_sampler_takes_deep_policies(cuda, monkeypatch):
    from mepol_amd import kernel_path
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.envs import CustomRewardEnv, GridGoal, GridWorldContinuous
    from mepol_amd.policy import GaussianPolicy

    for var in ("MEPOL_TRPO_SAMPLER", "MEPOL_ROLLOUT_FUSED", "MEPOL_ROLLOUT_DEEP_MAX_WORDS"):
        monkeypatch.delenv(var, raising=False)
    torch.manual_seed(0)
    env = CustomRewardEnv(GridWorldContinuous(), GridGoal((5, 5)))
    pol = GaussianPolicy([64, 64, 64], 2, 2).cuda()
    goal, layers = kernel_path.goal_sampler(env, pol)
    assert goal is env.get_reward and [tuple(W.shape) for W, _ in layers] == [(64, 2), (64, 64),
                                                                             (64, 64)]
    # no word cap here; MEPOL's own dispatch keeps its own
    wide = GaussianPolicy([512] * 6, 2, 2).cuda()
    assert len(kernel_path.goal_sampler(env, wide)[1]) == 6
    assert M._rollout_deep_layers(wide, 2, 2) is None
    assert M._rollout_deep_layers(pol, 2, 2) is not None
    # the two-layer return value is what it was: a pair of (W, b) pairs
    two = kernel_path.goal_sampler(env, GaussianPolicy([64, 48], 2, 2).cuda())[1]
    assert isinstance(two, tuple) and len(two) == 2

    assert kernel_path.goal_sampler(env, GaussianPolicy([8] * 7, 2, 2).cuda()) is None
    assert kernel_path.goal_sampler(
        env, GaussianPolicy([64, 64, 64], 2, 2, activation=nn.Tanh).cuda()) is None
    other = CustomRewardEnv(GridWorldContinuous(dim=5), GridGoal((4, 4)))
    assert kernel_path.goal_sampler(other, pol) is None
    monkeypatch.setenv("MEPOL_TRPO_SAMPLER", "host")
    assert kernel_path.goal_sampler(env, pol) is None


# ---- 8. collect_sample_batch -----------------------------------------------------------------
def test_collect_sample_batch_deep_policy(cuda, monkeypatch):
    """[64, 48, 64], 8 trajectories a round from a scripted pool, 700 steps: a second round runs,
    and its last trajectory is cut by the budget."""
    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    pol, init, noise, S, A = _case((64, 48, 64), NT, T)
    goal = S[0, 30]
    (st, ac, rw, ln, dn), taken, stats = _sample_with_pool(pol, init, noise, goal)
    exp, rounds = _expected_sample(S, A, goal)
    assert rounds == 2 and taken == [ROUND, ROUND]
    assert stats["path"] == "kernel" and stats["rounds"] == 2
    assert st.is_cuda and st.dtype == torch.float32 and ac.dtype == torch.float32
    assert rw.dtype == torch.float32 and ln.dtype == torch.int32 and dn.dtype == torch.bool
    assert int(ln.sum()) == BATCH
    for got, want in zip((st, ac, rw, ln, dn), exp):
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert 0 < int(ln[-1]) < T and not bool(dn[-1])  # the cut one
    assert bool(dn.any()) and float(rw.sum()) == int(dn.sum())


# ---- 9. trpo() -------------------------------------------------------------------------------
def test_trpo_deep_policy_two_epochs(cuda, tmp_path, monkeypatch):
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments.goal_rl import create_critic
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    assert 600 >= TR.fvp_min_rows()
    fisher_kernels = []
    real_init = TR.PolicyFisher.__init__

    def init(self, *a, **k):
        real_init(self, *a, **k)
        fisher_kernels.append(self.kernels)

    monkeypatch.setattr(TR.PolicyFisher, "__init__", init)
    torch.manual_seed(2)
    policy = GaussianPolicy([64, 64, 64], 2, 2, -1.5).cuda()
    vfunc = create_critic(2)
    before = dict(TR.SAMPLER_STATS)
    TR.trpo(lambda: _goal_env((-5, -5)), "GridGoalTest", 2, 600, 60, vfunc=vfunc, policy=policy,
            optimizer="lbfgs", cg_iters=10, kl_thresh=0.01, out_path=str(tmp_path), seed=3)
    assert TR.SAMPLER_STATS["kernel_batches"] == before["kernel_batches"] + 2
    assert TR.SAMPLER_STATS["host_batches"] == before["host_batches"]
    assert TR.SAMPLER_STATS["path"] == "kernel"
    assert fisher_kernels == [True, True]
    lines = (tmp_path / "GridGoalTest.csv").read_text().splitlines()
    assert lines[0] == "Epoch,NumSamples,ExecutionTime,AverageReturn,BacktrackSuccess,BacktrackIters"
    rows = [r.split(",") for r in lines[1:]]
    assert [r[:2] for r in rows] == [["0", "600"], ["1", "1200"]]
    assert all(math.isfinite(float(r[2])) and math.isfinite(float(r[3])) for r in rows)
    assert all(torch.isfinite(p).all() for p in policy.parameters())
    assert all(p.is_cuda and torch.isfinite(p).all() for p in vfunc.parameters())
    # the files of a two-layer run (test_gpu_goal_rl.test_trpo_gpu_two_epochs)
    assert {"GridGoalTest.csv", "log_file.txt", "policy_weights"} <= set(os.listdir(tmp_path))
    sd = torch.load(tmp_path / "policy_weights")
    assert all(torch.equal(v, policy.state_dict()[k].cpu()) for k, v in sd.items())


# ---- 10. the command line --------------------------------------------------------------------
def test_goal_rl_cli_round_trip(cuda, tmp_path, capsys, monkeypatch):
    """A three-layer checkpoint through goal_rl.main: with --hidden_sizes it trains an epoch on
    the kernel sampler, without it the run ends with a line that names the checkpoint's widths."""
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments import goal_rl
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    torch.manual_seed(4)
    ckpt = tmp_path / "3-policy"
    torch.save(GaussianPolicy([64, 64, 64], 2, 2).state_dict(), ckpt)
    args = ["--env", "GridGoal1", "--policy_init", str(ckpt), "--num_epochs", "1", "--batch_size",
            "600", "--traj_len", "60", "--kl_thresh", "0.01", "--seed", "1", "--results_dir",
            str(tmp_path / "results")]
    default = torch.get_default_dtype()
    try:  # main() makes f64 the process's default dtype
        assert goal_rl.main(args + ["--hidden_sizes", "64", "64", "64"]) == 0
        assert TR.SAMPLER_STATS["path"] == "kernel"
        capsys.readouterr()
        assert goal_rl.main(args) == 4
    finally:
        torch.set_default_dtype(default)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and "64 64 64" in out[0] and "--hidden_sizes 64 64 64" in out[0]
    runs = os.listdir(tmp_path / "results" / "goal_rl")
    assert len(runs) == 1 and "init=MEPOLInit,hidden=64x64x64__" in runs[0]
    info = (tmp_path / "results" / "goal_rl" / runs[0] / "log_info.txt").read_text()
    assert "hidden_sizes=[64, 64, 64]\n" in info
