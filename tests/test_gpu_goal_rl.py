"""TRPO's sampling and batch processing on the HIP kernels (mepol_rollout_goal, mepol_traj_budget,
mepol_gae, mepol_standardize) and the layers above them, against the sequential restatements of
goal_rl_cases.py and the oracle's k-ordered rollout."""
import functools

import numpy as np
import pytest
import torch

import goal_rl_cases as C
from oracle import mepol_oracle as O

pytestmark = pytest.mark.gpu

NT, T = 20, 60
U = 2.0 ** -53


def _scaled_policy(hidden):
    """The rollout tests' policy with a small mean (the untouched random policy parks 93 % of its
    steps against the outer wall)."""
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(11)
    pol = GaussianPolicy(hidden, 2, 2, -1.5).cuda()
    with torch.no_grad():
        pol.mean.weight.mul_(0.02)
        pol.mean.bias.fill_(0.05)
    return pol


@functools.lru_cache(maxsize=None)
def _rollout_case(h0, h1):
    """(policy, init, noise, S, A): the un-terminated oracle rollout every goal test truncates;
    computed once per policy shape and left unchanged."""
    from mepol_amd import ops

    pol = _scaled_policy([h0, h1])
    rng = np.random.default_rng(3)
    init = rng.uniform(-6, -4, (NT, 2)).astype(np.float32)
    noise = rng.standard_normal((T, NT, 2))
    sd = {k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()}
    std_dev = torch.exp(pol.log_std.detach()).cpu().numpy()  # as the device computes it
    plan = ops.rollout_mlp_plan(NT, h0, h1, 2)
    S, A = O.rollout_kordered("gridworld", sd, std_dev, init, noise, T, plan["k_chunks"])
    for x in (init, noise, S, A):
        x.setflags(write=False)
    return pol, init, noise, S, A


def _ff(shape, dtype):
    """A device buffer whose every byte is 0xff (NaN as f32, -1 as int32)."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _run_goal(pol, init, noise, goal, radius=0.1, env_id=1):
    from mepol_amd import ops

    Tn, n, a = noise.shape
    out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32),
           _ff((n, Tn), torch.float32), _ff((n,), torch.int32), _ff((n,), torch.int32))
    l1, l2 = pol.net[0], pol.net[2]
    ops.rollout_goal(l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach(),
                     pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
                     torch.tensor(init, device="cuda"),
                     torch.tensor(noise, dtype=torch.float64, device="cuda"), goal, radius,
                     *out, env_id=env_id)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("mw", ["1", "0"], ids=["multi-wg", "one-wg"])
@pytest.mark.parametrize("hidden", [(300, 300), (64, 48)])
def test_rollout_goal_bitexact_vs_truncated_oracle(cuda, monkeypatch, hidden, mw):
    """mepol_rollout_goal equals the un-terminated k-ordered oracle rollout cut at each
    trajectory's first hit, bit for bit, in both kernel forms: states and actions up to len,
    zeros behind, reward 1 on a terminated episode's last step, every output defined by the call
    (the buffers start as 0xff)."""
    from mepol_amd import ops

    monkeypatch.setenv("MEPOL_ROLLOUT_MW", mw)
    pol, init, noise, S, A = _rollout_case(*hidden)
    plan = ops.rollout_mlp_plan(NT, hidden[0], hidden[1], 2)
    assert plan["k_chunks"] == 4
    assert plan["workgroups_per_traj"] == (1 if mw == "0" else (hidden[1] + 63) // 64)
    kinds = set()
    for t_star in (1, 30, 60):
        goal = S[0, t_star]
        lens, dones = C.first_hit(S, goal)
        St, At, Rt = C.truncate(S, A, lens, dones)
        s, a, r, ln, dn = _run_goal(pol, init, noise, goal)
        assert np.array_equal(ln, lens) and np.array_equal(dn, dones.astype(np.int32))
        assert np.array_equal(s, St) and np.array_equal(a, At) and np.array_equal(r, Rt)
        assert not np.signbit(s[St == 0]).any() and not np.signbit(a[At == 0]).any()
        for L, d in zip(lens.tolist(), dones.tolist()):
            kinds.add("len1" if L == 1 else "mid_done" if 1 < L < T and d else
                      "T_done" if L == T and d else "T_not_done" if L == T else "other")
        assert (lens == T).sum() >= 16
    assert {"len1", "mid_done", "T_done", "T_not_done"} <= kinds, kinds


def test_rollout_goal_arguments(cuda):
    """env_id 0 is MEPOL_ERR_UNSUPPORTED, from the workspace query (the wrapper's first call) and
    from the launcher itself (called with a workspace of the caller's); n = 0 launches nothing
    (the outputs keep their bytes)."""
    from mepol_amd._lib import MepolError, call, ptr

    pol, init, noise, S, _ = _rollout_case(64, 48)
    with pytest.raises(MepolError, match="rc=1003"):
        _run_goal(pol, init, noise, S[0, 1], env_id=0)
    l1, l2 = pol.net[0], pol.net[2]
    w = [t.detach().contiguous() for t in (l1.weight, l1.bias, l2.weight.t(), l2.bias,
                                           pol.mean.weight, pol.mean.bias, pol.log_std)]
    d_init = torch.tensor(init, device="cuda")
    d_noise = torch.tensor(noise, dtype=torch.float64, device="cuda")
    out = (_ff((NT, T + 1, 2), torch.float32), _ff((NT, T, 2), torch.float32),
           _ff((NT, T), torch.float32), _ff((NT,), torch.int32), _ff((NT,), torch.int32))
    ws = _ff((256,), torch.uint8)
    gx, gy = (float(v) for v in S[0, 1])
    with pytest.raises(MepolError, match="rc=1003"):
        call("mepol_rollout_goal", 0, ptr(w[0]), ptr(w[1]), 64, ptr(w[2]), ptr(w[3]), 48,
             ptr(w[4]), ptr(w[5]), ptr(w[6]), 2, ptr(d_init), ptr(d_noise), NT, T, gx, gy, 0.1,
             *(ptr(x) for x in out), ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert all(bool((x.view(torch.uint8) == 0xFF).all()) for x in (*out, ws))  # nothing ran
    out = _run_goal(pol, init[:0], noise[:, :0], S[0, 1])
    assert all(x.size == 0 for x in out)
    with pytest.raises(MepolError, match="rc=1001"):
        _run_goal(pol, init, noise, S[0, 1], radius=-1.0)


def _budget_inputs(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 40, n).astype(np.int32)
    dones = rng.integers(0, 2, n).astype(bool)
    return lens, dones


@pytest.mark.parametrize("n", [1, 3, 70, 1000])
def test_traj_budget_exact(cuda, n):
    from mepol_amd import ops

    lens, dones = _budget_inputs(n, n)
    total = int(lens.sum())
    mid = int(lens[:(n + 1) // 2].sum())
    budgets = {max(int(lens[0]) - 1, 0), int(lens[0]), mid, max(mid - 1, 1), total - 1, total,
               total + 7}
    dl = torch.as_tensor(lens, device="cuda")
    dd = torch.as_tensor(dones.astype(np.int32), device="cuda")
    for b in sorted(budgets):
        lo, do, off, (m, kept) = C.budget(lens, dones, b)
        g_lo, g_do, g_off, g_meta = (x.cpu().numpy() for x in ops.traj_budget(dl, dd, b))
        assert g_meta.tolist() == [m, kept] and kept == min(b, total)
        assert np.array_equal(g_lo, lo) and np.array_equal(g_do, do.astype(np.int32))
        assert np.array_equal(g_off, off) and g_off.dtype == np.int64
        assert not g_lo[m:].any() and not g_do[m:].any()


def test_traj_budget_arguments(cuda):
    from mepol_amd import ops
    from mepol_amd._lib import MepolError

    z = torch.ones(65537, dtype=torch.int32, device="cuda")
    with pytest.raises(MepolError, match="rc=1003"):
        ops.traj_budget(z, z, 10)
    with pytest.raises(MepolError, match="rc=1001"):
        ops.traj_budget(z[:4], z[:4], -1)


def _gae_inputs(n, Tn):
    """Ragged lengths that include 1, T with done, T not done, a budget-cut last trajectory and
    unused trajectories of length 0 (where n allows), as traj_budget hands them on."""
    rng = np.random.default_rng(100 * n + Tn)
    lens = rng.integers(1, Tn + 1, n).astype(np.int32)
    dones = lens < Tn  # an episode shorter than T ended at the goal
    b = int(lens.sum())
    if n >= 3:
        lens[0], dones[0] = 1, True
        lens[1], dones[1] = Tn, True
        lens[2], dones[2] = Tn, False
        b = int(lens.sum())
    if n > 8:  # trajectory n - 5 ends at the goal but is cut 3 steps short; 4 stay unused
        lens[n - 5], dones[n - 5] = Tn // 2, True
        b = int(lens[:n - 4].sum()) - 3
    if n < 3:
        dones[:] = False
    R = np.where(rng.random((n, Tn)) < 0.3, rng.standard_normal((n, Tn)), 0).astype(np.float32)
    V = rng.standard_normal((n, Tn + 1))
    S = rng.standard_normal((n, Tn + 1, 2)).astype(np.float32)
    A = rng.standard_normal((n, Tn, 2)).astype(np.float32)
    return lens, dones, b, R, V, S, A


@pytest.mark.parametrize("n,Tn", [(1, 1), (3, 5), (70, 130)])
def test_gae_bit_equal_to_sequential_f64(cuda, n, Tn):
    """mepol_gae against the numpy f64 loop: targets, advantages and the packed states / actions
    are the same bits.  70 trajectories are more than a wave of them and several workgroups; 130
    steps cross the 64-step staging chunk twice."""
    from mepol_amd import ops

    lens, dones, b, R, V, S, A = _gae_inputs(n, Tn)
    lo, do, off, (m, kept) = C.budget(lens, dones, b)
    if n == 70:
        assert m < n and lo[m - 1] < lens[m - 1] and not do[m - 1]  # cut, and unused behind it
        assert {1, Tn} <= set(lo.tolist())
    dev = lambda x: torch.as_tensor(x, device="cuda")  # noqa: E731
    t, a, st, ac = ops.gae(dev(R), dev(V), dev(lo), dev(do.astype(np.int32)), dev(off), kept,
                           C.GAMMA, C.LAMBD, dev(S), dev(A))
    et, ea, es, eac = C.gae_batch(R, V, lo, do, S, A)
    assert t.shape == (kept,) and st.shape == (kept, 2) and ac.shape == (kept, 2)
    assert np.array_equal(t.cpu().numpy(), et) and np.array_equal(a.cpu().numpy(), ea)
    assert np.array_equal(st.cpu().numpy(), es) and np.array_equal(ac.cpu().numpy(), eac)


def _std_bound(z, N):
    """|computed - exact| per element of (x - mean) / std for fixed-order f64 sums, u = 2^-53.
    With a = sum|x| / (N std):
      mean   a fixed-order sum errs by (N-1) u sum|x|, the division by u |mean| <= u sum|x| / N,
             so |d mean| / std <= N u a;
      std    sum d_i = 0, so the mean's error enters the variance only in second order; each
             (x_i - mean)^2 is off by 3 u relatively, their fixed-order sum by (N-1) u, the
             division and the root by u each and the root halves the rest: |d std| / std <=
             (N / 2 + 3) u;
      z_i    the subtraction and the division add 2 u |z_i|.
    Together |d z_i| <= N u a + (N / 2 + 5) u |z_i| <= 16 N u (1 + |z_i|) whenever a <= 16, which
    the test asserts of its inputs; the issue's constant stands.  The longdouble reference's own
    error is 2^-11 of that."""
    return 16 * N * U * (1 + np.abs(z))


@pytest.mark.parametrize("N", [1, 2, 257, 24000])
def test_standardize(cuda, N):
    from mepol_amd import ops

    rng = np.random.default_rng(N)
    x = 0.3 + 2.0 * rng.standard_normal(N)
    dx = torch.as_tensor(x, device="cuda")
    got = ops.standardize(dx)
    again = ops.standardize(dx)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))  # same bits, NaN included
    g = got.cpu().numpy()
    with np.errstate(all="ignore"):
        ref_np = (x - x.mean()) / x.std()
    if N == 1:
        assert not np.isfinite(g).any() and not np.isfinite(ref_np).any()
        return
    z = C.standardize_ld(x)
    assert np.abs(x).sum() / (N * x.std()) <= 16
    err = np.abs(g.astype(np.longdouble) - z)
    assert (err <= _std_bound(z, N)).all(), float((err / _std_bound(z, N)).max())
    # a constant vector (1.5 N is exact, so the mean is): 0 / 0, as numpy
    const = torch.full((N,), 1.5, dtype=torch.float64, device="cuda")
    with np.errstate(all="ignore"):
        c_np = (const.cpu().numpy() - 1.5) / const.cpu().numpy().std()
    assert not np.isfinite(c_np).any()
    assert not torch.isfinite(ops.standardize(const)).any()


def _goal_env(goal):
    from mepol_amd.envs import CustomRewardEnv, GridGoal, GridWorldContinuous

    return CustomRewardEnv(GridWorldContinuous(), GridGoal(goal))


ROUND, BATCH = 8, 700


def _sample_with_pool(pol, init, noise, goal, batch=BATCH, round_traj=ROUND):
    """collect_sample_batch on the kernel path, its rounds drawing round_traj trajectories at a
    time from the pool (init, noise) in order."""
    from mepol_amd.algorithms import trpo as TR

    taken = []

    def draw(R, Tn, a, device):
        k = len(taken)
        taken.append(R)
        sl = slice(k * R, (k + 1) * R)
        return (torch.tensor(init[sl], device=device),
                torch.tensor(noise[:, sl], dtype=torch.float64, device=device))

    out = TR.collect_sample_batch(_goal_env(goal), pol, batch, T, draw=draw,
                                  round_traj=round_traj)
    return out, taken, dict(TR.SAMPLER_STATS)


def _expected_sample(S, A, goal, batch=BATCH, round_traj=ROUND):
    remaining, parts, k = batch, [], 0
    while remaining > 0:
        sl = slice(k * round_traj, (k + 1) * round_traj)
        lens, dones = C.first_hit(S[sl], goal)
        lo, do, _, (m, kept) = C.budget(lens, dones, remaining)
        St, At, Rt = C.truncate(S[sl], A[sl], lo, do)
        parts.append((St[:m], At[:m], Rt[:m], lo[:m, None], do[:m, None]))
        remaining -= kept
        k += 1
    return [np.concatenate(x) for x in zip(*parts)], k


def test_collect_sample_batch_kernel_path(cuda):
    """The sampler's rounds (rollout_goal, traj_budget, concatenation) equal the helper's:
    truncate the oracle rollout, apply the budget to each round in turn.  8 trajectories a round
    and 700 steps need a second round, whose fifth trajectory is cut."""
    pol, init, noise, S, A = _rollout_case(300, 300)
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


def test_collect_sample_batch_cuts_before_a_goal(cuda):
    """A last trajectory that is cut BEFORE the step at which it reaches the goal: the kernel
    wrote reward 1 at that later step, and the batch must not keep it (rows behind a
    trajectory's end are zero; the rewards sum to the number of done trajectories).  10
    trajectories a round: the second round's trajectory 17 of the pool reaches the goal at step
    8 and is cut at 5."""
    pol, init, noise, S, A = _rollout_case(300, 300)
    goal = S[0, 30]
    lens, dones = C.first_hit(S, goal)
    assert dones[17] and lens[17] > 5  # the test's premise, from the un-cut rollout
    batch = int(lens[:17].sum()) + 5
    (st, ac, rw, ln, dn), taken, stats = _sample_with_pool(pol, init, noise, goal, batch, 10)
    exp, rounds = _expected_sample(S, A, goal, batch, 10)
    assert rounds == 2 and taken == [10, 10] and stats["rounds"] == 2
    assert ln.shape == (18, 1) and int(ln[-1]) == 5 and not bool(dn[-1])
    assert int(ln.sum()) == batch
    for got, want in zip((st, ac, rw, ln, dn), exp):
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert float(rw[-1].sum()) == 0 and float(rw.sum()) == int(dn.sum()) > 0


def test_goal_sampler_gate_takes_the_default_gridworld_only(cuda):
    """The kernels' GridWorld has the default size, step and walls: another one takes the host
    loop."""
    from mepol_amd import kernel_path
    from mepol_amd.envs import CustomRewardEnv, GridGoal, GridWorldContinuous

    pol = _rollout_case(64, 48)[0]
    goal = GridGoal((5, 5))
    assert kernel_path.goal_sampler(CustomRewardEnv(GridWorldContinuous(), goal), pol) is not None
    for kw in (dict(dim=5), dict(max_delta=0.1), dict(wall_width=2.0)):
        env = CustomRewardEnv(GridWorldContinuous(**kw), goal)
        assert kernel_path.goal_sampler(env, pol) is None, kw


def test_round_capacity_follows_the_goal_kernels_plan(cuda, monkeypatch):
    """A round of _round_capacity trajectories is the largest that still takes the goal kernel's
    multi-workgroup form, and the cached value follows MEPOL_ROLLOUT_MW."""
    from mepol_amd import ops
    from mepol_amd.algorithms import trpo as TR

    dev = torch.device("cuda", torch.cuda.current_device())
    monkeypatch.delenv("MEPOL_ROLLOUT_MW", raising=False)
    cap = TR._round_capacity(300, 300, 2, dev)
    assert ops.rollout_goal_plan(cap, 300, 300)["workgroups_per_traj"] == 5
    assert ops.rollout_goal_plan(cap + 1, 300, 300)["workgroups_per_traj"] == 1
    assert ops.rollout_goal_plan(cap, 300, 300)["k_chunks"] == 4
    monkeypatch.setenv("MEPOL_ROLLOUT_MW", "0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert TR._round_capacity(300, 300, 2, dev) == cus


def test_process_batch_cuda_matches_cpu(cuda):
    from mepol_amd.algorithms import trpo as TR

    pol, init, noise, S, A = _rollout_case(300, 300)
    batch, _, _ = _sample_with_pool(pol, init, noise, S[0, 30])
    m = batch[0].shape[0]
    values = torch.as_tensor(np.random.default_rng(1).standard_normal((m, T + 1)), device="cuda")
    gpu = TR.process_batch(*batch, values, C.GAMMA, C.LAMBD)
    cpu = TR.process_batch(*(x.cpu() for x in batch), values.cpu(), C.GAMMA, C.LAMBD)
    for g, c in zip(gpu[:3], cpu[:3]):
        assert g.is_cuda and g.dtype == torch.float64 and g.shape == c.shape
        assert torch.equal(g.cpu(), c)
    # the standardised advantages: both within the fixed-order bound of the extended-precision
    # standardisation of the raw advantages (the helper's, bit-equal to both paths')
    st, ac, rw, ln, dn = (x.cpu().numpy() for x in batch)
    _, adv, _, _ = C.gae_batch(rw, values.cpu().numpy(), ln.ravel(), dn.ravel(), st, ac)
    z = C.standardize_ld(adv)
    assert np.abs(adv).sum() / (len(adv) * adv.std()) <= 16
    for got in (gpu[3].cpu().numpy(), cpu[3].numpy()):
        assert got.shape == (BATCH,)
        assert (np.abs(got.astype(np.longdouble) - z) <= _std_bound(z, BATCH)).all()


def test_trpo_gpu_two_epochs(cuda, tmp_path):
    """trpo() end to end on the GPU: the sampler on the kernel path (600 rows >= FVP_MIN_ROWS, so
    trpo_step takes its kernels too), CSV rows written, policy and critic finite."""
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments.goal_rl import create_critic
    from mepol_amd.policy import GaussianPolicy

    assert 600 >= TR.fvp_min_rows()
    torch.manual_seed(2)
    policy = GaussianPolicy([300, 300], 2, 2, -1.5).cuda()
    vfunc = create_critic(2)
    before = dict(TR.SAMPLER_STATS)
    TR.trpo(lambda: _goal_env((-5, -5)), "GridGoalTest", 2, 600, 60, vfunc=vfunc, policy=policy,
            optimizer="lbfgs", cg_iters=10, kl_thresh=0.01, out_path=str(tmp_path), seed=3)
    assert TR.SAMPLER_STATS["kernel_batches"] == before["kernel_batches"] + 2
    assert TR.SAMPLER_STATS["host_batches"] == before["host_batches"]
    assert TR.SAMPLER_STATS["path"] == "kernel"
    lines = (tmp_path / "GridGoalTest.csv").read_text().splitlines()
    assert lines[0] == "Epoch,NumSamples,ExecutionTime,AverageReturn,BacktrackSuccess,BacktrackIters"
    assert [r.split(",")[:2] for r in lines[1:]] == [["0", "600"], ["1", "1200"]]
    assert all(torch.isfinite(p).all() for p in policy.parameters())
    assert all(p.is_cuda and torch.isfinite(p).all() for p in vfunc.parameters())
    sd = torch.load(tmp_path / "policy_weights")
    assert all(torch.equal(v, policy.state_dict()[k].cpu()) for k, v in sd.items())
