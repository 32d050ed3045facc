"""TRPO's "roll out, then cut" sampler on the GPU (kernel_path.cut_sampler, trpo._cut_round,
ops.traj_cut): any envs.BatchReward samples on the un-terminated one-launch rollouts.

  route equivalence   a goal the kernels have a kind for gives, wrapped in a one-member AnyGoal,
                      the same five tensors bit for bit on the cut route as on the in-kernel route;
  other rewards       BoxGoal and a three-member AnyGoal equal traj_cut_cases.cut_reference applied
                      to the un-terminated kernel's own records with the numpy predicate;
  budget and rounds   goal_rl_cases.budget over the same records, round by round;
  gates, bad results and two epochs through trpo() on the new goal_rl specs.

8 trajectories of T = 12 or 40 steps; init and noise from rollout_cases through `draw`."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import goal_rl_cases as G
import rollout_cases as R
import threshold_goal_cases as TC
import traj_cut_cases as CC

pytestmark = pytest.mark.gpu

N = 8
T_VALUES = (12, 40)
HIDDEN = ((36, 64), (5, 65), (64, 48, 64))
INF = float("inf")
BALL_MARGIN = 1e-5
RADIUS = 0.1


def _id(hidden):
    return "x".join(map(str, hidden))


_CASES, _GPU, _FREE = {}, {}, {}


def _case(env, hidden, T):
    key = (env, hidden, T)
    if key not in _CASES:
        rng = np.random.default_rng(77)
        init = np.concatenate([R._init(env, 3, rng) for _ in range(3)])[:N]
        _CASES[key] = R.make_case(f"cut-{env[:2]}-{_id(hidden)}-T{T}", env, hidden, n=N, steps=T,
                                  seed=60 + T, init=init)
    return _CASES[key]


def _policy(case):
    pol = R.case_policy(case)
    if id(pol) not in _GPU:
        _GPU[id(pol)] = (pol, copy.deepcopy(pol).cuda())
    return _GPU[id(pol)][1]


def _unterminated(case):
    """(S f32 [n, T+1, 2], A f32 [n, T, a], V f64 [n, T, 2]) of the un-terminated one-launch
    rollout of the case: once per case, shared and read-only."""
    from mepol_amd import ops

    if case["name"] not in _FREE:
        pol = _policy(case)
        Tn, n, a = case["noise"].shape
        out = (torch.empty((n, Tn + 1, 2), dtype=torch.float32, device="cuda"),
               torch.empty((n, Tn, a), dtype=torch.float32, device="cuda"),
               torch.empty((n, Tn, 2), dtype=torch.float64, device="cuda"))
        head = (pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
                torch.tensor(case["init"], device="cuda"),
                torch.tensor(case["noise"], dtype=torch.float64, device="cuda"))
        layers = [(m.weight.detach(), m.bias.detach()) for m in pol.net if isinstance(m, nn.Linear)]
        env_id = 0 if case["env"] == "mountaincar" else 1
        if len(layers) == 2:
            ops.rollout_mlp(env_id, *layers[0], *layers[1], *head, out[0], out[1], visited=out[2])
        else:
            ops.rollout_deep(env_id, layers, *head, out[0], out[1], visited=out[2])
        res = tuple(x.cpu().numpy() for x in out)
        for x in res:
            x.setflags(write=False)
        S, _, V = res
        assert np.array_equal(V.astype(np.float32), S[:, 1:])
        if env_id == 1:
            assert np.array_equal(V, S[:, 1:].astype(np.float64))
        _FREE[case["name"]] = res
    return _FREE[case["name"]]


def _draw(case, taken=None):
    """The same round every time: the case's init (in the env's own dtype) and noise."""
    def draw(Rn, Tn, a, device):
        assert (Rn, Tn, a) == (case["n"], case["T"], case["a_dim"])
        if taken is not None:
            taken.append(Rn)
        return (torch.tensor(case["init"], device=device),
                torch.tensor(case["noise"], dtype=torch.float64, device=device))
    return draw


def _env(case, reward):
    from mepol_amd.envs import CustomRewardEnv, GridWorldContinuous, MountainCarContinuous

    base = MountainCarContinuous() if case["env"] == "mountaincar" else GridWorldContinuous()
    return CustomRewardEnv(base, reward)


def _sample(case, reward, batch, path):
    from mepol_amd.algorithms import trpo as TR

    taken = []
    before = dict(TR.SAMPLER_STATS)
    out = TR.collect_sample_batch(_env(case, reward), _policy(case), batch, case["T"],
                                  draw=_draw(case, taken), round_traj=N)
    assert TR.SAMPLER_STATS["path"] == path and TR.SAMPLER_STATS["rounds"] == len(taken)
    for key in ("kernel_batches", "cut_batches", "host_batches"):
        assert TR.SAMPLER_STATS[key] == before[key] + (key == path + "_batches"), key
    st, ac, rw, ln, dn = out
    assert st.dtype == ac.dtype == rw.dtype == torch.float32
    assert ln.dtype == torch.int32 and dn.dtype == torch.bool
    return [x.cpu().numpy() for x in out], taken


def _expected(S, A, hit, reward, batch):
    """The sampler's result from the un-terminated records: per round cut_reference with the
    predicate's hits, then the step budget and the masking of the budget-cut last trajectory."""
    n, Tn = hit.shape
    Rc, Sc, Ac, lens, dones = CC.cut_reference(hit, reward, S, A)
    remaining, parts, rounds = batch, [], 0
    while remaining > 0:
        lo, do, _, (m, kept) = G.budget(lens, dones, remaining)
        st, ac, rw = Sc[:m].copy(), Ac[:m].copy(), Rc[:m].copy()
        last = int(lo[m - 1])
        st[m - 1, last + 1:] = 0
        ac[m - 1, last:] = 0
        rw[m - 1, last:] = 0
        parts.append((st, ac, rw, lo[:m, None], do[:m, None]))
        remaining -= kept
        rounds += 1
    return [np.concatenate(x) for x in zip(*parts)], rounds


def _assert_same(got, want, what):
    for key, g, w in zip(("states", "actions", "rewards", "lens", "dones"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, w.shape)
        assert np.array_equal(CC.bits(g), CC.bits(w)), (what, key)


def _ball_goal(case):
    """A ball goal that trajectory 0 reaches by step GOAL_T, with the margin condition: no tested
    state lies within BALL_MARGIN of the radius, so neither sqrt's last bit nor the predicate's
    decides a hit."""
    S, _, _ = _unterminated(case)
    g = (S[0, R.GOAL_T] + R.GOAL_OFF).astype(np.float32)
    d = np.sqrt(((S[:, 1:].astype(np.float64) - g.astype(np.float64)) ** 2).sum(axis=-1))
    assert (np.abs(d - RADIUS) > BALL_MARGIN).all(), float(np.abs(d - RADIUS).min())
    assert (d[0, :R.GOAL_T] <= RADIUS).any()
    return g


# ---- 1. route equivalence ----------------------------------------------------------------------
def _pairs(case):
    """[(label, reward of the in-kernel route, the same goal as a BatchReward)]."""
    from mepol_amd.envs import AnyGoal, GridGoal, ThresholdGoal

    _, _, V = _unterminated(case)
    coord = 0
    thr = float(V[0, R.GOAL_T - 1, coord])                 # a value the rollout reaches exactly
    out = [("threshold", ThresholdGoal(coord, thr), AnyGoal(ThresholdGoal(coord, thr)))]
    if case["env"] == "gridworld":
        g = _ball_goal(case)
        out.append(("ball", GridGoal(g, RADIUS), AnyGoal(GridGoal(g, RADIUS))))
    return out


@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("hidden", HIDDEN, ids=_id)
@pytest.mark.parametrize("env", R.ENVS)
def test_cut_route_equals_the_in_kernel_route(cuda, monkeypatch, env, hidden, T):
    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    case = _case(env, hidden, T)
    for label, in_kernel, batched in _pairs(case):
        batch = N * T + 5                                  # more than a round holds
        want, rounds_k = _sample(case, in_kernel, batch, "kernel")
        got, rounds_c = _sample(case, batched, batch, "cut")
        assert rounds_k == rounds_c and len(rounds_c) >= 2, label
        _assert_same(got, want, (case["name"], label))
        assert int(got[3].sum()) == batch and got[4].any(), label


# ---- 2. BoxGoal and a three-member AnyGoal against the restatement --------------------------------
def _np_box(X, low, high):
    with np.errstate(invalid="ignore"):
        return ((np.asarray(low) <= X) & (X <= np.asarray(high))).all(axis=-1)


def _other_rewards(case):
    """[(label, reward, hits bool [n, T] by the numpy predicate on the env's own states)]."""
    from mepol_amd.envs import AnyGoal, BoxGoal, GridGoal, ThresholdGoal

    _, _, V = _unterminated(case)
    t = R.GOAL_T - 1
    p, q = float(V[0, t, 0]), float(V[0, t, 1])
    # a half-space `<=` (what ThresholdGoal cannot say) whose face is a value the rollout reaches
    low, high = (-INF, -INF), (p, INF)
    out = [("box<=", BoxGoal(low, high), _np_box(V, low, high))]
    # a closed box with trajectory 0's state at step GOAL_T on its corner
    span = 0.05 if case["env"] == "mountaincar" else 0.5
    low, high = (p, q - span), (p + span, q)
    out.append(("box-corner", BoxGoal(low, high), _np_box(V, low, high)))
    thr = float(V[1, t, 1])
    members = [BoxGoal(low, high), ThresholdGoal(1, thr)]
    hits = [_np_box(V, low, high), ThresholdGoal(1, thr).hit(V)]
    if case["env"] == "gridworld":
        g = _ball_goal(case)
        members.append(GridGoal(g, RADIUS))
        hits.append(GridGoal(g, RADIUS).hit(V.astype(np.float32)))
    else:
        members.append(ThresholdGoal(0, float(V[2, t, 0])))
        hits.append(members[-1].hit(V))
    out.append(("any3", AnyGoal(*members), hits[0] | hits[1] | hits[2]))
    return out


@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("hidden", HIDDEN, ids=_id)
@pytest.mark.parametrize("env", R.ENVS)
def test_box_and_any_goals_equal_the_cut_restatement(cuda, monkeypatch, env, hidden, T):
    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    case = _case(env, hidden, T)
    S, A, V = _unterminated(case)
    some_done = False
    for label, reward, hit in _other_rewards(case):
        assert hit.shape == (N, T) and hit[0, R.GOAL_T - 1], label
        batch = int(CC.cut_reference(hit, hit.astype(np.float32), S, A)[3].sum())  # one round
        want, rounds = _expected(S, A, hit, hit.astype(np.float32), batch)
        assert rounds == 1
        got, taken = _sample(case, reward, batch, "cut")
        assert taken == [N]
        _assert_same(got, want, (case["name"], label))
        assert got[2].sum() == got[4].sum() > 0            # reward 1 exactly where done
        some_done |= bool(0 < got[4].sum() < N)
    assert some_done


# ---- 3. budget and rounds ----------------------------------------------------------------------
@pytest.mark.parametrize("hidden", HIDDEN[1:], ids=_id)
@pytest.mark.parametrize("env", R.ENVS)
def test_second_round_and_the_budget_cut(cuda, monkeypatch, env, hidden):
    """A batch that needs a second round whose last trajectory the budget cuts one step before
    its hit: it is not done and loses that reward, as on the goal route."""
    from mepol_amd.envs import BoxGoal

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    case = _case(env, hidden, 40)
    S, A, V = _unterminated(case)
    # the half-space x >= p with p a value the rollout reaches, the first such that some
    # trajectory ends done after two steps or more (so that a cut can fall in front of its hit)
    for p in V[:, R.GOAL_T - 1:, 0].T.reshape(-1).tolist():
        low, high = (p, -INF), (INF, INF)
        hit = _np_box(V, low, high)
        _, _, _, lens, dones = CC.cut_reference(hit, hit.astype(np.float32), S, A)
        late = np.flatnonzero((dones == 1) & (lens >= 2))
        if len(late):
            break
    j = int(late[0])
    batch = int(lens.sum()) + int(lens[:j].sum()) + int(lens[j]) - 1
    want, rounds = _expected(S, A, hit, hit.astype(np.float32), batch)
    assert rounds == 2
    got, taken = _sample(case, BoxGoal(low, high), batch, "cut")
    assert taken == [N, N]
    _assert_same(got, want, case["name"])
    st, ac, rw, ln, dn = got
    assert ln.shape == (N + j + 1, 1) and int(ln.sum()) == batch
    assert int(ln[-1, 0]) == lens[j] - 1 and not dn[-1, 0]  # cut by the budget: not done ...
    assert rw[-1].sum() == 0 and rw[j].sum() == 1          # ... and the hit behind the cut is lost
    for i in range(len(ln)):                               # rows behind every end are zero
        L = int(ln[i, 0])
        assert not st[i, L + 1:].any() and not ac[i, L:].any() and not rw[i, L:].any()
        assert not np.signbit(st[i, L + 1:]).any() and not np.signbit(ac[i, L:]).any()


# ---- 4. gates ----------------------------------------------------------------------------------
def test_cut_sampler_gate(cuda, monkeypatch):
    from mepol_amd import kernel_path
    from mepol_amd.envs import (AnyGoal, BoxGoal, CustomRewardEnv, ErgodicEnv, GridGoal,
                                GridWorldContinuous, MountainCarContinuous, ThresholdGoal)
    from mepol_amd.experiments.goal_rl import exp_specs
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    monkeypatch.delenv("MEPOL_ROLLOUT_FUSED", raising=False)
    torch.manual_seed(0)
    cut, gate = kernel_path.cut_sampler, kernel_path.goal_sampler
    specs = exp_specs()
    for name, a_dim, env_id in (("GridGoalAny", 2, 1), ("MountainCarLeft", 1, 0)):
        spec = specs[name]
        env = spec["env_create"]()
        pol = GaussianPolicy(spec["hidden_sizes"], 2, a_dim, spec["log_std_init"]).cuda()
        reward, layers, eid = cut(env, pol)
        assert reward is env.get_reward and eid == env_id
        assert isinstance(layers, tuple) and len(layers) == 2
        assert gate(env, pol) is None                      # no in-kernel kind for it
        deep = GaussianPolicy([64, 48, 64], 2, a_dim, spec["log_std_init"]).cuda()
        assert len(cut(env, deep)[1]) == 3
    two = GaussianPolicy([36, 64], 2, 2, -1.5).cuda()
    one = GaussianPolicy([36, 64], 2, 1, -0.5).cuda()
    box = BoxGoal((-INF, -INF), (0.0, INF))
    gw, mc = GridWorldContinuous, MountainCarContinuous
    assert cut(CustomRewardEnv(gw(), box), two) is not None
    assert cut(CustomRewardEnv(mc(), box), one) is not None
    # declined: a plain function reward, a goal of the in-kernel kinds (no BatchReward) ...
    assert cut(CustomRewardEnv(gw(), lambda s, r, d, i: (0, False)), two) is None
    assert cut(CustomRewardEnv(gw(), GridGoal((5, 5))), two) is None
    assert cut(CustomRewardEnv(mc(), ThresholdGoal(0, 0.45)), one) is None
    # ... a Tanh policy, seven layers, the other env's action count, a CPU policy ...
    assert cut(CustomRewardEnv(gw(), box), GaussianPolicy([36, 64], 2, 2, activation=nn.Tanh).cuda()) is None
    assert cut(CustomRewardEnv(gw(), box), GaussianPolicy([8] * 7, 2, 2).cuda()) is None
    assert cut(CustomRewardEnv(gw(), box), one) is None
    assert cut(CustomRewardEnv(mc(), box), two) is None
    assert cut(CustomRewardEnv(gw(), box), GaussianPolicy([36, 64], 2, 2)) is None
    # ... a non-default env, a subclass, another wrapper in between ...
    for kw in (dict(dim=8), dict(max_delta=0.1), dict(wall_width=2.0)):
        assert cut(CustomRewardEnv(gw(**kw), box), two) is None, kw
    steep = mc()
    steep.power = 0.002
    assert cut(CustomRewardEnv(steep, box), one) is None
    assert cut(CustomRewardEnv(ErgodicEnv(gw()), box), two) is None
    assert cut(ErgodicEnv(gw()), two) is None
    # ... and the switch
    env = CustomRewardEnv(gw(), AnyGoal(GridGoal((5, 5))))
    assert cut(env, two) is not None
    monkeypatch.setenv("MEPOL_TRPO_SAMPLER", "host")
    assert cut(env, two) is None
    monkeypatch.delenv("MEPOL_TRPO_SAMPLER")
    # goal_sampler answers what it did: one accepted input, one declined
    ball = CustomRewardEnv(gw(), GridGoal((5, 5)))
    goal, layers = gate(ball, two)
    assert goal is ball.get_reward and isinstance(layers, tuple) and len(layers) == 2
    assert gate(CustomRewardEnv(gw(dim=5), GridGoal((4, 4))), two) is None
    assert gate(CustomRewardEnv(mc(), GridGoal((0.45, 0.0))), one) is None


def test_host_switch_takes_the_host_loop(cuda, monkeypatch):
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import BoxGoal, CustomRewardEnv, GridWorldContinuous

    case = _case("gridworld", (36, 64), 12)
    env = CustomRewardEnv(GridWorldContinuous(), BoxGoal((-INF, -INF), (INF, INF)))
    env.seed(0)
    monkeypatch.setenv("MEPOL_TRPO_SAMPLER", "host")
    out = TR.collect_sample_batch(env, _policy(case), 9, 12)
    assert TR.SAMPLER_STATS["path"] == "host" and out[3].reshape(-1).tolist() == [1] * 9
    monkeypatch.delenv("MEPOL_TRPO_SAMPLER")
    out = TR.collect_sample_batch(env, _policy(case), 9, 12)
    assert TR.SAMPLER_STATS["path"] == "cut" and out[3].reshape(-1).tolist() == [1] * 9
    assert out[4].all() and float(out[2].sum()) == 9


# ---- 5. a bad batch() ----------------------------------------------------------------------------
def test_bad_batch_results_raise(cuda, monkeypatch):
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import BatchReward

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    case = _case("gridworld", (36, 64), 12)

    def reward_class(fn):
        return type("OddReward", (BatchReward,), {"batch": lambda self, s: fn(s)})()

    ok = lambda s: (torch.zeros(s.shape[:2], device=s.device), s[..., 0] > 1e9)  # noqa: E731
    bad = {
        "done of the wrong shape": lambda s: (ok(s)[0], ok(s)[1][:, :-1]),
        "reward of the wrong shape": lambda s: (ok(s)[0][..., None], ok(s)[1]),
        "done that is not bool": lambda s: (ok(s)[0], ok(s)[1].to(torch.int32)),
        "done as floats": lambda s: (ok(s)[0], ok(s)[0]),
        "an integer reward": lambda s: (ok(s)[1].to(torch.int64), ok(s)[1]),
        "one tensor": lambda s: ok(s)[1],
    }
    for what, fn in bad.items():
        with pytest.raises(ValueError, match="OddReward"):
            TR.collect_sample_batch(_env(case, reward_class(fn)), _policy(case), 20, 12,
                                    draw=_draw(case), round_traj=N)
    out = TR.collect_sample_batch(_env(case, reward_class(ok)), _policy(case), 20, 12,
                                  draw=_draw(case), round_traj=N)
    assert TR.SAMPLER_STATS["path"] == "cut" and out[3].reshape(-1).tolist() == [12, 8]
    # an f64 reward is rounded to f32, kept in front of the end
    shaped = reward_class(lambda s: (s[..., 0] * (1.0 / 3.0), s[..., 0] > 1e9))
    out = TR.collect_sample_batch(_env(case, shaped), _policy(case), 12, 12, draw=_draw(case),
                                  round_traj=N)
    S, _, V = _unterminated(case)
    want = torch.tensor(V[:1, :, 0]).mul(1.0 / 3.0).to(torch.float32).numpy()
    assert np.array_equal(out[2].cpu().numpy(), want)


# ---- 6. through trpo() -----------------------------------------------------------------------
@pytest.mark.parametrize("name,a_dim", [("GridGoalAny", 2), ("MountainCarLeft", 1)])
def test_trpo_two_epochs_on_the_new_specs(cuda, tmp_path, monkeypatch, name, a_dim):
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments.goal_rl import create_critic, exp_specs
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    spec = exp_specs()[name]
    torch.manual_seed(2)
    policy = GaussianPolicy(spec["hidden_sizes"], 2, a_dim, spec["log_std_init"]).cuda()
    vfunc = create_critic(2)
    before = dict(TR.SAMPLER_STATS)
    TR.trpo(spec["env_create"], name, 2, 600, 40, vfunc=vfunc, policy=policy, optimizer="lbfgs",
            cg_iters=10, kl_thresh=0.01, out_path=str(tmp_path), seed=3)
    assert TR.SAMPLER_STATS["path"] == "cut"
    assert TR.SAMPLER_STATS["cut_batches"] == before["cut_batches"] + 2
    assert TR.SAMPLER_STATS["kernel_batches"] == before["kernel_batches"]
    assert TR.SAMPLER_STATS["host_batches"] == before["host_batches"]
    lines = (tmp_path / f"{name}.csv").read_text().splitlines()
    assert lines[0] == "Epoch,NumSamples,ExecutionTime,AverageReturn,BacktrackSuccess,BacktrackIters"
    rows = [r.split(",") for r in lines[1:]]
    assert len(rows) == 2 and all(len(r) == 6 for r in rows)
    assert [r[:2] for r in rows] == [["0", "600"], ["1", "1200"]]
    sd = torch.load(tmp_path / "policy_weights")
    fresh = GaussianPolicy(spec["hidden_sizes"], 2, a_dim, spec["log_std_init"])
    fresh.load_state_dict(sd)
    assert all(torch.equal(v, policy.state_dict()[k].cpu()) for k, v in sd.items())
    assert all(torch.isfinite(p).all() for p in policy.parameters())
