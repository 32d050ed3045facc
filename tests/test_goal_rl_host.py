"""TRPO's sampling, batch processing, driver and command line on the host (no GPU): against the
reference's recorded outputs (tests/golden/goal_rl_*.npz, made by make_golden_goal_rl.py) and the
sequential restatements of goal_rl_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import goal_rl_cases as C


@pytest.fixture(scope="module")
def traj_golden():
    return load_golden("goal_rl_process_traj")


@pytest.fixture(scope="module")
def budget_golden():
    return load_golden("goal_rl_budget")


def _traj_cases(z):
    for c in range(int(z["num_cases"])):
        yield {k: z[f"c{c}_{k}"] for k in ("rewards", "vfuncs", "boot", "done", "targets",
                                           "advantages")}


def test_process_traj_matches_reference(traj_golden):
    """Host process_traj against the reference's: bit-equal to the helper's f64 loop, and within
    the reference's own per-step f32 rounding of its recorded (f32) results: each of a
    trajectory's len steps rounds a value of magnitude <= max|value| to f32 (relative 2^-24,
    bounded here by 2^-23), and the recurrences' factors are below 1, so the errors add up to at
    most 2^-23 * len * max|value|."""
    from mepol_amd.algorithms.trpo import process_traj

    gamma, lambd = float(traj_golden["gamma"]), float(traj_golden["lambd"])
    for case in _traj_cases(traj_golden):
        n = len(case["rewards"])
        z = np.zeros((n, 2), dtype=np.float32)
        t, a = process_traj(gamma, lambd, case["vfuncs"], z, z, case["rewards"], case["boot"])
        th, ah = C.gae_traj(case["rewards"], case["vfuncs"], case["boot"], gamma, lambd)
        assert t.dtype == np.float64 and a.dtype == np.float64
        assert np.array_equal(t, th) and np.array_equal(a, ah)
        for got, ref in ((t, case["targets"]), (a, case["advantages"])):
            tol = 2.0 ** -23 * n * max(np.abs(got).max(), np.abs(ref).max())
            assert np.abs(got - ref).max() <= tol, (n, np.abs(got - ref).max(), tol)


def test_process_traj_takes_tensors(traj_golden):
    """The reference passes the critic's output and boot value as tensors."""
    from mepol_amd.algorithms.trpo import process_traj

    case = list(_traj_cases(traj_golden))[3]
    n = len(case["rewards"])
    z = np.zeros((n, 2), dtype=np.float32)
    t0, a0 = process_traj(C.GAMMA, C.LAMBD, case["vfuncs"], z, z, case["rewards"], case["boot"])
    t1, a1 = process_traj(C.GAMMA, C.LAMBD, torch.as_tensor(case["vfuncs"]).unsqueeze(1), z, z,
                          case["rewards"], torch.as_tensor(case["boot"]).reshape(1))
    assert np.array_equal(t0, t1) and np.array_equal(a0, a1)


def _batch_from_golden(z):
    """The golden's trajectories as one padded batch (T = the longest), lengths / dones as a
    sampler returns them."""
    cases = list(_traj_cases(z))
    m, T = len(cases), max(len(c["rewards"]) for c in cases)
    rng = np.random.default_rng(4)
    S = rng.standard_normal((m, T + 1, 2)).astype(np.float32)
    A = rng.standard_normal((m, T, 2)).astype(np.float32)
    R = np.zeros((m, T), dtype=np.float32)
    V = rng.standard_normal((m, T + 1))
    lens = np.zeros((m, 1), dtype=np.int32)
    dones = np.zeros((m, 1), dtype=bool)
    for i, c in enumerate(cases):
        n = len(c["rewards"])
        R[i, :n], V[i, :n], V[i, n] = c["rewards"], c["vfuncs"], float(c["boot"])
        lens[i], dones[i] = n, bool(c["done"])
    return cases, S, A, R, V, lens, dones


def test_process_batch_cpu_matches_reference_and_helper(traj_golden):
    from mepol_amd.algorithms.trpo import process_batch

    cases, S, A, R, V, lens, dones = _batch_from_golden(traj_golden)
    es, ea, et, eadv = process_batch(*(torch.as_tensor(x) for x in (S, A, R, lens, dones, V)),
                                     C.GAMMA, C.LAMBD)
    t, adv, st, ac = C.gae_batch(R, V, lens.ravel(), dones.ravel(), S, A)
    N = int(lens.sum())
    assert es.shape == (N, 2) and ea.shape == (N, 2) and et.shape == (N, 1) and eadv.shape == (N,)
    assert all(x.dtype == torch.float64 for x in (es, ea, et, eadv))
    assert np.array_equal(es.numpy(), st) and np.array_equal(ea.numpy(), ac)
    assert np.array_equal(et.numpy()[:, 0], t)
    assert np.array_equal(eadv.numpy(), (adv - adv.mean()) / adv.std())
    # targets against the reference's recorded ones, trajectory by trajectory
    o = 0
    for c in cases:
        n = len(c["rewards"])
        tol = 2.0 ** -23 * n * max(np.abs(t[o:o + n]).max(), np.abs(c["targets"]).max())
        assert np.abs(t[o:o + n] - c["targets"]).max() <= tol
        o += n


def test_budget_rule_matches_reference_sampler(budget_golden):
    """The helper's budget rule over the scripted episodes rolled out in parallel gives exactly
    the lengths, dones and step count of the reference's sequential collect_sample_batch."""
    z = budget_golden
    seen = set()
    for name in z["names"]:
        T, B = int(z[f"{name}_traj_len"]), int(z[f"{name}_batch_size"])
        lens, dones = C.scripted_parallel(z[f"{name}_ep_lens"], T)
        lo, do, off, (m, kept) = C.budget(lens, dones, B)
        ref_l, ref_d = z[f"{name}_real_traj_lens"].ravel(), z[f"{name}_dones"].ravel()
        assert m == len(ref_l) and kept == int(z[f"{name}_steps"]) == B
        assert np.array_equal(lo[:m], ref_l) and np.array_equal(do[:m], ref_d)
        assert not lo[m:].any() and not do[m:].any() and off[-1] == B
        last = m - 1
        if lo[last] < lens[last]:
            seen.add("cut")
        elif dones[last]:
            seen.add("on_termination")
        else:
            seen.add("at_traj_len")
    assert seen == {"cut", "on_termination", "at_traj_len"}


class _ScriptedEnv:
    def __init__(self, ep_lens):
        from mepol_amd.envs import Box

        # Python ints: the sampler tests `done is True`, as the reference does
        self.ep_lens, self.episode, self.num_features = [int(x) for x in ep_lens], -1, 2
        self.action_space = Box(-np.ones(2, dtype=np.float32), np.ones(2, dtype=np.float32))

    def reset(self):
        self.episode += 1
        self.t = 0
        return np.zeros(2, dtype=np.float32)

    def step(self, a):
        self.t += 1
        done = self.t >= self.ep_lens[self.episode]
        return np.full(2, self.t, dtype=np.float32), (1 if done else 0), done, {}


class _ZeroPolicy:
    device = torch.device("cpu")

    def predict(self, s):
        return torch.zeros(2)


def test_collect_sample_batch_host_matches_reference(budget_golden):
    """The sequential path of collect_sample_batch on the golden's scripted env."""
    from mepol_amd.algorithms import trpo as T

    z = budget_golden
    for name in z["names"]:
        L, B = int(z[f"{name}_traj_len"]), int(z[f"{name}_batch_size"])
        st, ac, rw, lens, dones = T.collect_sample_batch(_ScriptedEnv(z[f"{name}_ep_lens"]),
                                                        _ZeroPolicy(), B, L)
        assert T.SAMPLER_STATS["path"] == "host"
        assert st.dtype == torch.float32 and lens.dtype == torch.int32 and dones.dtype == torch.bool
        assert np.array_equal(lens.numpy(), z[f"{name}_real_traj_lens"])
        assert np.array_equal(dones.numpy(), z[f"{name}_dones"])
        assert float(rw.sum()) == float(z[f"{name}_reward_sum"])
        for i, n in enumerate(lens.ravel().tolist()):  # the state reached is kept, zeros behind
            assert st[i, n, 0] == n and not st[i, n + 1:].any() and not rw[i, n:].any()


def test_grid_goal_matches_numpy_norm_at_the_radius():
    """GridGoal against np.linalg.norm(s - g).astype(np.float64) <= 0.1 on 100,000 f32 points
    within 2e-7 of the radius (both sides of it, and exactly on the f32 0.1)."""
    from mepol_amd.envs import GridGoal

    rng = np.random.default_rng(8)
    n = 100_000
    for g in ((5, 5), (2, 5), (5, 2), (-5, -5)):
        goal = GridGoal(g)
        assert goal.goal.dtype == np.float32 and goal.radius == 0.1
        th = rng.uniform(0, 2 * np.pi, n)
        rad = 0.1 + rng.uniform(-2e-7, 2e-7, n)
        s = (np.asarray(g, dtype=np.float64) + rad[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
             ).astype(np.float32)
        ref = np.linalg.norm(s - goal.goal, axis=1).astype(np.float64) <= 0.1
        got = goal.hit(s)
        assert np.array_equal(got, ref)
        assert np.array_equal(got, C.goal_hit(s, goal.goal))
        assert 0.2 < ref.mean() < 0.8  # the points do straddle the radius
        for i in range(0, n, 997):  # the scalar form CustomRewardEnv calls
            r, d = goal(s[i], 0, False, {})
            want = bool(np.linalg.norm(s[i] - goal.goal).astype(np.float64) <= 0.1)
            assert (r, d) == ((1, True) if want else (0, False))


def test_custom_reward_env_semantics():
    from mepol_amd.envs import (CustomRewardEnv, ErgodicEnv, GridGoal, GridWorldContinuous,
                                unwrap)

    base = GridWorldContinuous()
    env = CustomRewardEnv(base, GridGoal((-5, -5), radius=3.0))
    assert env.unwrapped is base and unwrap(env) is base and env.num_features == 2
    assert not isinstance(env, ErgodicEnv)  # its episodes end
    both = ErgodicEnv(env)
    assert both.unwrapped is base and unwrap(both) is base
    env.seed(3)
    env.reset()
    s, r, d, _ = env.step(np.zeros(2))
    assert (r, d) == (1, True)  # the whole start box is within 3 of (-5, -5)
    far = CustomRewardEnv(base, lambda s, r, d, i: (7, "x"))
    assert far.step(np.zeros(2))[1:3] == (7, "x")


def _critic():
    from mepol_amd.experiments.goal_rl import create_critic

    return create_critic(2)


@pytest.mark.parametrize("optimizer", ["lbfgs", "adam"])
def test_trpo_cpu_two_epochs(tmp_path, optimizer):
    """trpo() on the host path: the reference's CSV, log and weights files."""
    from mepol_amd.algorithms import trpo as T
    from mepol_amd.envs import CustomRewardEnv, GridGoal, GridWorldContinuous
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(0)
    policy = GaussianPolicy([32, 32], 2, 2, -1.5)
    vfunc = _critic()
    before = T.SAMPLER_STATS["host_batches"]
    T.trpo(lambda: CustomRewardEnv(GridWorldContinuous(), GridGoal((-5, -5))), "GridGoalTest", 2,
           200, 20, vfunc=vfunc, policy=policy, optimizer=optimizer, critic_iters=2,
           out_path=str(tmp_path), seed=5)
    assert T.SAMPLER_STATS["host_batches"] == before + 2
    lines = (tmp_path / "GridGoalTest.csv").read_text().splitlines()
    assert lines[0] == "Epoch,NumSamples,ExecutionTime,AverageReturn,BacktrackSuccess,BacktrackIters"
    assert len(lines) == 3
    for e, row in enumerate(lines[1:]):
        f = row.split(",")
        assert len(f) == 6 and int(f[0]) == e and int(f[1]) == 200 * (e + 1)
        assert float(f[2]) > 0 and 0 <= float(f[3]) <= 1 and f[4] in ("True", "False")
        assert 0 <= int(f[5]) <= 9
    assert (tmp_path / "log_file.txt").stat().st_size > 0
    fresh = GaussianPolicy([32, 32], 2, 2, -1.5)
    fresh.load_state_dict(torch.load(tmp_path / "policy_weights"))
    for p, q in zip(fresh.parameters(), policy.parameters()):
        assert torch.equal(p, q) and torch.isfinite(p).all()
    assert all(torch.isfinite(p).all() for p in vfunc.parameters())


def test_trpo_rejects_discrete_actions(tmp_path):
    from mepol_amd.algorithms import trpo as T

    class _Discrete:
        n = 3

    class _Env:
        action_space = _Discrete()
        num_features = 2

    with pytest.raises(NotImplementedError):
        T.trpo(_Env, "x", 1, 10, 5, vfunc=_critic(), policy=None, out_path=str(tmp_path))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "mepol_amd.experiments.goal_rl", *args],
                          capture_output=True, text=True, cwd=ROOT, env=env, timeout=120)


def test_cli_help_lists_reference_flags():
    out = _cli("--help")
    assert out.returncode == 0
    for flag in ("--num_workers", "--env", "--policy_init", "--num_epochs", "--batch_size",
                 "--traj_len", "--gamma", "--lambd", "--optimizer", "--critic_lr", "--critic_reg",
                 "--critic_iters", "--critic_batch_size", "--cg_iters", "--cg_damping",
                 "--kl_thresh", "--seed", "--tb_dir_name"):
        assert flag in out.stdout, flag


def test_cli_defaults_and_specs():
    from mepol_amd.experiments.goal_rl import build_parser, exp_specs

    a = build_parser().parse_args(["--env", "GridGoal1", "--num_epochs", "1", "--batch_size", "10",
                                   "--traj_len", "5", "--kl_thresh", "0.001"])
    assert (a.gamma, a.lambd, a.optimizer, a.critic_lr, a.critic_reg, a.critic_iters) == (
        0.995, 0.98, "adam", 1e-2, 1e-3, 5)
    assert (a.critic_batch_size, a.cg_iters, a.cg_damping, a.num_workers, a.tb_dir_name) == (
        64, 10, 0.1, 1, "goal_rl")
    specs = exp_specs()
    for name, goal in (("GridGoal1", (5, 5)), ("GridGoal2", (2, 5)), ("GridGoal3", (5, 2))):
        env = specs[name]["env_create"]()
        assert tuple(env.get_reward.goal) == goal and env.get_reward.radius == 0.1
        assert specs[name]["hidden_sizes"] == [300, 300] and specs[name]["log_std_init"] == -1.5
    for name in ("AntEscape", "AntNavigate", "AntJump", "HumanoidUp"):
        assert specs[name]["hidden_sizes"] == [400, 300] and specs[name]["log_std_init"] == -0.5


def test_cli_mujoco_env_exits_with_message():
    out = _cli("--env", "AntJump", "--num_epochs", "1", "--batch_size", "10", "--traj_len", "5",
               "--kl_thresh", "0.001")
    assert out.returncode == 2
    assert "AntJump needs MuJoCo" in out.stdout
