"""The threshold goals of the one-launch rollouts on the GPU (mepol_rollout_goal_threshold in both
forms, mepol_rollout_deep_goal_threshold; MountainCar and GridWorld) and the layers above them:
the sampler's gate and rounds and trpo() on the MountainCar goal.

References, never the goal kernels themselves:
  states / actions   the un-terminated rollout of the same inputs cut at each episode's end.  For
                     two hidden layers that is O.rollout_kordered (GridWorld bit for bit;
                     MountainCar's first step bit for bit and the rest to the 1e-12 of
                     test_gpu_rollout_ops.py, since cos() may differ from glibc in the last ulp)
                     AND the records of ops.rollout_mlp, bit for bit on both envs, as the header
                     promises.  For 3 to 6 layers it is ops.rollout_deep, which
                     test_gpu_rollout_deep.py pins (the k-ordered oracle has two layers).
  len / done         the first hit computed on the host: for the MountainCar climb case from the
                     independent f64 rollout (threshold_goal_cases.climb_f64: every comparison
                     keeps its margin), for thresholds taken from a rollout's own values from the
                     `visited` f64 output of the un-terminated kernel.
Every output buffer starts as 0xff bytes, so an element the call left alone is NaN or -1."""
import copy

import numpy as np
import pytest
import torch

import goal_rl_cases as G
import rollout_cases as R
import threshold_goal_cases as TC

pytestmark = pytest.mark.gpu

FORMS = ["one-wg", "multi-wg"]
INF = float("inf")


def _ids(hs):
    return ["x".join(map(str, h)) for h in hs]


def _ff(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _dev(x, dtype=None):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


_GPU = {}


def _policy(case):
    """The case's policy on the GPU and exp(log_std) as the device computes it."""
    pol = R.case_policy(case)
    if id(pol) not in _GPU:
        dev = copy.deepcopy(pol).cuda()
        _GPU[id(pol)] = (pol, dev, torch.exp(dev.log_std.detach()).cpu().numpy())
    return _GPU[id(pol)][1:]


def _layers(pol):
    import torch.nn as nn

    return [(m.weight.detach(), m.bias.detach()) for m in pol.net if isinstance(m, nn.Linear)]


def _env_id(case):
    return 0 if case["env"] == "mountaincar" else 1


_FREE = {}


def _unterminated(case, noise=None):
    """(S f32 [n, T+1, 2], A f32 [n, T, a], V f64 [n, T, 2]) of ops.rollout_mlp / ops.rollout_deep
    on the case: computed once per (case, noise), shared and left unchanged."""
    from mepol_amd import ops

    key = (case["name"], None if noise is None else noise.tobytes())
    if key not in _FREE:
        pol, _ = _policy(case)
        noise_ = case["noise"] if noise is None else noise
        Tn, n, a = noise_.shape
        out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32),
               _ff((n, Tn, 2), torch.float64))
        head = (pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
                _dev(case["init"]), _dev(noise_, torch.float64))
        layers = _layers(pol)
        if len(layers) == 2:
            ops.rollout_mlp(_env_id(case), *layers[0], *layers[1], *head, out[0], out[1],
                            visited=out[2])
        else:
            ops.rollout_deep(_env_id(case), layers, *head, out[0], out[1], visited=out[2])
        res = tuple(x.cpu().numpy() for x in out)
        for x in res:
            x.setflags(write=False)
        _FREE[key] = res
    return _FREE[key]


_ORACLE = {}


def _check_against_oracle(case):
    """The un-terminated kernel's records against O.rollout_kordered (two layers), once per case."""
    if case["name"] in _ORACLE or len(case["hidden"]) != 2:
        return
    S, A, V = _unterminated(case)
    S_ref, A_ref = R.oracle(case, std=_policy(case)[1])
    if case["env"] == "gridworld":
        assert np.array_equal(S, S_ref) and np.array_equal(A, A_ref)
    else:
        assert np.array_equal(A[:, 0], A_ref[:, 0]) and np.array_equal(S[:, 0], S_ref[:, 0])
        np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(S, S_ref, rtol=0, atol=1e-12)
    assert np.array_equal(V.astype(np.float32), S[:, 1:])
    _ORACLE[case["name"]] = True


def _run(case, coord, threshold, noise=None):
    from mepol_amd import ops

    pol, _ = _policy(case)
    noise = case["noise"] if noise is None else noise
    Tn, n, a = noise.shape
    out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32),
           _ff((n, Tn), torch.float32), _ff((n,), torch.int32), _ff((n,), torch.int32))
    head = (pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
            _dev(case["init"]), _dev(noise, torch.float64), coord, threshold)
    layers = _layers(pol)
    if len(layers) == 2:
        ops.rollout_goal_threshold(_env_id(case), *layers[0], *layers[1], *head, *out)
    else:
        ops.rollout_deep_goal_threshold(_env_id(case), layers, *head, *out)
    return [x.cpu().numpy() for x in out]


def _assert_cut(got, S, A, lens, dones):
    """The outputs equal the un-terminated records cut at these episodes, bit for bit, with
    positive zeros behind each episode, reward 1 only on a terminated episode's last step, and
    no byte left as the caller's 0xff."""
    St, At, Rt = G.truncate(S, A, lens, dones)
    s, a, r, ln, dn = got
    assert np.array_equal(ln, lens), (ln, lens)
    assert np.array_equal(dn, np.asarray(dones).astype(np.int32)), (dn, dones)
    assert np.array_equal(s, St, equal_nan=True) and np.array_equal(a, At, equal_nan=True)
    assert np.array_equal(r, Rt)
    assert not np.signbit(s[St == 0]).any() and not np.signbit(a[At == 0]).any()
    assert not np.signbit(r).any()


def _set_form(monkeypatch, case, form):
    """Select the two-layer form and assert which one the threshold instance's plan reports."""
    from mepol_amd import ops

    h0, h1 = case["hidden"]
    monkeypatch.setenv("MEPOL_ROLLOUT_MW", "1" if form == "multi-wg" else "0")
    plan = ops.rollout_goal_threshold_plan(_env_id(case), case["n"], h0, h1, case["a_dim"])
    m = R.mw_model(h0, h1, case["a_dim"])
    assert plan["k_chunks"] == R.K_CHUNKS
    assert plan["workgroups_per_traj"] == (m["np"] if form == "multi-wg" and m["accepted"] else 1)


def _two_layer_params():
    return [pytest.param(h, f, id=f"{'x'.join(map(str, h))}-{f}")
            for h in TC.TWO_LAYER + (TC.WIDE,) for f in FORMS]


# ---- 1. MountainCar: the climb to the hilltop --------------------------------------------------
def _climb(hidden):
    """The hilltop goal on the climb case: the four kinds of episode, the ends from the host's
    independent f64 rollout; the threshold 0.45 is reached only through the wall's clip."""
    case = TC.climb_case(hidden)
    V64, _, _, _ = TC.climb_f64(hidden)
    lens, dones = TC.first_hit(V64, *TC.HILLTOP)
    assert TC.kinds(lens, dones, case["T"]) == TC.KINDS
    _check_against_oracle(case)
    S, A, V = _unterminated(case)
    lk, dk = TC.first_hit(V, *TC.HILLTOP)  # the kernel's own f64 states say the same
    assert np.array_equal(lk, lens) and np.array_equal(dk, dones)
    got = _run(case, *TC.HILLTOP)
    _assert_cut(got, S, A, lens, dones)
    for i in np.flatnonzero(dones):
        assert got[0][i, lens[i], 0] == np.float32(0.45) and got[0][i, lens[i], 1] == 0
    if len(hidden) == 2:  # and against the oracle's records, cut the same way
        S_ref, A_ref = R.oracle(case, std=_policy(case)[1])
        St, At, _ = G.truncate(S_ref, A_ref, lens, dones)
        np.testing.assert_allclose(got[0], St, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got[1], At, rtol=0, atol=1e-12)
        assert np.array_equal(got[1][:, 0], At[:, 0])


@pytest.mark.parametrize("hidden,form", _two_layer_params())
def test_mountaincar_climb_two_layers(cuda, monkeypatch, hidden, form):
    _set_form(monkeypatch, TC.climb_case(hidden), form)
    _climb(hidden)


@pytest.mark.parametrize("hidden", TC.DEEP, ids=_ids(TC.DEEP))
def test_mountaincar_climb_deep(cuda, hidden):
    _climb(hidden)


# ---- 2. the edges of the comparison -----------------------------------------------------------
def _edges(case):
    """Thresholds at the comparison's edges; every first hit comes from the un-terminated
    kernel's `visited` f64 states, which existing tests pin to the oracle."""
    _check_against_oracle(case)
    S, A, V = _unterminated(case)
    n, Tn = case["n"], case["T"]
    t = R.GOAL_T - 1                      # the step after which trajectory 0 is at S[0, GOAL_T]
    seen = set()
    for coord in (0, 1):
        at = float(V[0, t, coord])        # exactly the f64 value reached (f32-exact on GridWorld)
        up = float(np.nextafter(at, INF))
        assert np.isfinite(at) and up > at
        if case["env"] == "gridworld":    # less than an f32 ulp away: an f32 compare would hit
            assert np.float32(up) == S[0, R.GOAL_T, coord] == np.float32(at)
        for thr, hits in ((at, True), (up, False)):
            lens, dones = TC.first_hit(V, coord, thr)
            assert (V[0, t, coord] >= thr) == hits and (lens[0] <= R.GOAL_T) >= hits
            _assert_cut(_run(case, coord, thr), S, A, lens, dones)
            seen |= TC.kinds(lens, dones, Tn)
    settings = [(0, -INF), (1, -INF), (0, INF), (1, INF)]
    if case["env"] == "mountaincar":
        settings += [(0, 0.45), (1, 0.07), (1, -0.07), (0, -1.2)]
    for coord, thr in settings:
        lens, dones = TC.first_hit(V, coord, thr)
        if thr == -INF:
            assert (lens == 1).all() and dones.all()
        if thr == INF:
            assert (lens == Tn).all() and not dones.any()
        _assert_cut(_run(case, coord, thr), S, A, lens, dones)
    return seen


def _edge_case(env, hidden):
    return TC.mc_case(hidden) if env == "mountaincar" else TC.gw_case(hidden)


@pytest.mark.parametrize("env", R.ENVS)
@pytest.mark.parametrize("hidden,form", _two_layer_params())
def test_threshold_edges_two_layers(cuda, monkeypatch, env, hidden, form):
    case = _edge_case(env, hidden)
    _set_form(monkeypatch, case, form)
    _edges(case)


@pytest.mark.parametrize("env", R.ENVS)
@pytest.mark.parametrize("hidden", TC.DEEP, ids=_ids(TC.DEEP))
def test_threshold_edges_deep(cuda, env, hidden):
    _edges(_edge_case(env, hidden))


@pytest.mark.parametrize("hidden,form", _two_layer_params()[:2] + [pytest.param((70, 9, 66), None,
                                                                                id="70x9x66")])
def test_velocity_clamp_value_on_the_climb(cuda, monkeypatch, hidden, form):
    """coord = 1 with threshold 0.07, the velocity clamp's value, on the climb case, whose
    velocities sit on the clamp: `>=` takes the clamped 0.07 itself."""
    case = TC.climb_case(hidden)
    if form:
        _set_form(monkeypatch, case, form)
    S, A, V = _unterminated(case)
    lens, dones = TC.first_hit(V, 1, 0.07)
    assert dones.any() and (V[:, :, 1] <= 0.07).all()
    assert (V[dones, lens[dones] - 1, 1] == 0.07).all()
    _assert_cut(_run(case, 1, 0.07), S, A, lens, dones)
    up = float(np.nextafter(0.07, 1.0))
    _assert_cut(_run(case, 1, up), S, A, np.full(case["n"], case["T"], np.int32),
                np.zeros(case["n"], bool))


@pytest.mark.parametrize("form", FORMS + ["deep"])
def test_nan_state_is_no_hit(cuda, monkeypatch, form):
    """A NaN action makes the MountainCar state NaN: no hit from there on, done = 0.  With the
    NaN on the first step and a threshold below every position, the other trajectories end at
    step 1 and the NaN one runs to T; with rollout_cases' NaN at step NAN_STEP and the hilltop as
    the goal, it is cut exactly as the un-terminated NaN rollout's own states say."""
    (base,) = [c for c in R.nan_cases() if c["env"] == "mountaincar"]
    if form == "deep":
        case = R.make_case("nan_action-mc-deep", "mountaincar", (70, 9, 66), seed=90)
        assert np.array_equal(case["noise"], base["noise"])
    else:
        case = base
        _set_form(monkeypatch, case, form)
    first = case["noise"].copy()
    first[0, R.NAN_TRAJ, 0] = np.nan
    S, A, V = _unterminated(case, noise=first)
    assert np.isnan(V[R.NAN_TRAJ]).all() and np.isfinite(np.delete(V, R.NAN_TRAJ, 0)).all()
    got = _run(case, 0, -1.3, noise=first)
    want_len = np.ones(case["n"], np.int32)
    want_len[R.NAN_TRAJ] = case["T"]
    want_done = np.ones(case["n"], bool)
    want_done[R.NAN_TRAJ] = False
    _assert_cut(got, S, A, want_len, want_done)
    late = base["noise_nan"]
    S, A, V = _unterminated(case, noise=late)
    assert np.isnan(V[R.NAN_TRAJ, R.NAN_STEP:]).all()
    for coord, thr in (TC.HILLTOP, (1, -0.07), (0, float(V[R.NAN_TRAJ, R.NAN_STEP - 1, 0]))):
        lens, dones = TC.first_hit(V, coord, thr)
        _assert_cut(_run(case, coord, thr, noise=late), S, A, lens, dones)


# ---- 3. arguments on the device ---------------------------------------------------------------
def test_threshold_arguments_on_the_device(cuda):
    from mepol_amd import ops
    from mepol_amd._lib import MepolError

    case = TC.climb_case((64, 48))
    with pytest.raises(MepolError, match="rc=1001"):
        _run(case, 2, 0.45)
    with pytest.raises(MepolError, match="rc=1001"):
        _run(case, 0, float("nan"))
    pol, _ = _policy(case)
    (W1, b1), (W2, b2) = _layers(pol)
    head = (pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach())
    n, Tn = case["n"], case["T"]
    out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, 1), torch.float32),
           _ff((n, Tn), torch.float32), _ff((n,), torch.int32), _ff((n,), torch.int32))
    noise = _dev(case["noise"], torch.float64)
    with pytest.raises(ValueError, match="f64 for MountainCar"):
        ops.rollout_goal_threshold(0, W1, b1, W2, b2, *head, _dev(case["init"], torch.float32),
                                   noise, 0, 0.45, *out)
    with pytest.raises(MepolError, match="rc=1001"):  # GridWorld has two actions
        ops.rollout_goal_threshold(1, W1, b1, W2, b2, *head, _dev(case["init"], torch.float32),
                                   noise, 0, 0.45, *out)
    ops.rollout_goal_threshold(0, W1, b1, W2, b2, *head, _dev(case["init"])[:0], noise[:, :0], 0,
                               0.45, *(x[:0] for x in out))
    torch.cuda.synchronize()
    assert all(bool((x.view(torch.uint8) == 0xFF).all()) for x in out)  # nothing ran


# ---- 4. the sampler ---------------------------------------------------------------------------
ROUND = 8


def _pool_case(hidden):
    """16 trajectories: the climb case's four starts four times over, so that a round of 8 holds
    60 steps and every kind of episode."""
    init = np.array([[p, TC.CLIMB_V0] for p in TC.CLIMB_P0 * 4], dtype=np.float64)
    noise = np.full((R.T, 16, 1), R.BIG)
    return R.make_case("pool-" + "x".join(map(str, hidden)), "mountaincar", hidden, n=16, init=init,
                       noise=noise)


def _mc_env(index=0, threshold=0.45):
    from mepol_amd.envs import CustomRewardEnv, MountainCarContinuous, ThresholdGoal

    return CustomRewardEnv(MountainCarContinuous(), ThresholdGoal(index, threshold))


@pytest.mark.parametrize("hidden", [TC.WIDE, (70, 9, 66)], ids=_ids([TC.WIDE, (70, 9, 66)]))
def test_collect_sample_batch_on_the_mountaincar_goal(cuda, hidden):
    """The sampler's rounds on a MountainCarGoal-shaped env equal "truncate, then budget per
    round" over the un-terminated rollout of the pool: 8 trajectories a round and 73 steps need a
    second round, whose third trajectory is cut at 7 of its 12 steps."""
    from mepol_amd.algorithms import trpo as TR

    case = _pool_case(hidden)
    pol, _ = _policy(case)
    S, A, V = _unterminated(case)
    lens, dones = TC.first_hit(V, *TC.HILLTOP)
    assert tuple(lens.tolist()) == TC.CLIMB_LENS * 4 and tuple(dones.tolist()) == TC.CLIMB_DONE * 4
    batch = int(lens[:ROUND].sum()) + 1 + 5 + 7
    taken = []

    def draw(Rn, Tn, a, device):
        assert (Tn, a) == (case["T"], 1)
        k = len(taken)
        taken.append(Rn)
        sl = slice(k * Rn, (k + 1) * Rn)
        return (torch.tensor(case["init"][sl], device=device),  # f64: the env's own dtype
                torch.tensor(case["noise"][:, sl], dtype=torch.float64, device=device))

    st, ac, rw, ln, dn = TR.collect_sample_batch(_mc_env(), pol, batch, case["T"], draw=draw,
                                                 round_traj=ROUND)
    assert TR.SAMPLER_STATS["path"] == "kernel" and TR.SAMPLER_STATS["rounds"] == 2
    assert taken == [ROUND, ROUND]
    remaining, parts = batch, []
    for k in range(2):
        sl = slice(k * ROUND, (k + 1) * ROUND)
        lo, do, _, (m, kept) = G.budget(lens[sl], dones[sl], remaining)
        St, At, Rt = G.truncate(S[sl], A[sl], lo, do)
        parts.append((St[:m], At[:m], Rt[:m], lo[:m, None], do[:m, None]))
        remaining -= kept
    assert remaining == 0
    exp = [np.concatenate(x) for x in zip(*parts)]
    assert st.dtype == torch.float32 and ln.dtype == torch.int32 and dn.dtype == torch.bool
    for got, want in zip((st, ac, rw, ln, dn), exp):
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert ln.shape == (11, 1) and int(ln[-1]) == 7 and not bool(dn[-1]) and int(ln.sum()) == batch
    assert float(rw.sum()) == int(dn.sum()) == 8


def test_goal_sampler_gate_threshold_goals(cuda, monkeypatch):
    from mepol_amd import kernel_path
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import (CustomRewardEnv, GridGoal, GridWorldContinuous,
                                MountainCarContinuous, ThresholdGoal)
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    torch.manual_seed(0)
    one = GaussianPolicy([64, 48], 2, 1, -0.5).cuda()
    two = GaussianPolicy([64, 48], 2, 2, -1.5).cuda()
    deep1 = GaussianPolicy([70, 9, 66], 2, 1, -0.5).cuda()
    east = ThresholdGoal(0, 3.5)
    gate = kernel_path.goal_sampler
    # GridWorld with a threshold goal: the default one, two actions
    goal, layers = gate(CustomRewardEnv(GridWorldContinuous(), east), two)
    assert goal is east and len(layers) == 2
    assert gate(CustomRewardEnv(GridWorldContinuous(), east), one) is None
    for kw in (dict(dim=5), dict(max_delta=0.1), dict(wall_width=2.0)):
        assert gate(CustomRewardEnv(GridWorldContinuous(**kw), east), two) is None, kw
    # MountainCar with a threshold goal: exactly that type, the kernel's constants, one action
    env = _mc_env()
    goal, layers = gate(env, one)
    assert goal is env.get_reward and len(layers) == 2
    assert len(gate(_mc_env(1, 0.07), deep1)[1]) == 3
    assert gate(env, two) is None

    class Steeper(MountainCarContinuous):
        pass

    assert gate(CustomRewardEnv(Steeper(), ThresholdGoal(0, 0.45)), one) is None
    for field in kernel_path.MOUNTAINCAR_FIELDS:
        other = _mc_env()
        setattr(other.env, field, getattr(other.env, field) * 1.5)
        assert gate(other, one) is None, field
    # the None cases of the goal itself
    assert gate(CustomRewardEnv(MountainCarContinuous(), GridGoal((0.45, 0.0))), one) is None
    for index in (2, -1):
        assert gate(_mc_env(index, 0.45), one) is None
        assert gate(CustomRewardEnv(GridWorldContinuous(), ThresholdGoal(index, 3.5)), two) is None
    assert gate(_mc_env(0, float("nan")), one) is None
    # the switch: the gate closes and the sampler takes the host loop
    monkeypatch.setenv("MEPOL_TRPO_SAMPLER", "host")
    assert gate(env, one) is None
    env.seed(0)
    out = TR.collect_sample_batch(env, one, 30, 12)
    assert TR.SAMPLER_STATS["path"] == "host" and int(out[3].sum()) == 30
    monkeypatch.setenv("MEPOL_TRPO_SAMPLER", "kernel")
    out = TR.collect_sample_batch(env, one, 30, 12)
    assert TR.SAMPLER_STATS["path"] == "kernel" and int(out[3].sum()) == 30
    assert out[0].dtype == torch.float32 and out[1].shape[2] == 1


def test_gridworld_threshold_sampler_round(cuda):
    """A GridWorld threshold goal through the sampler: one round equals the truncated rollout."""
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import CustomRewardEnv, GridWorldContinuous, ThresholdGoal

    case = TC.gw_case((64, 48))
    pol, _ = _policy(case)
    S, A, V = _unterminated(case)
    thr = float(V[0, R.GOAL_T - 1, 0])
    lens, dones = TC.first_hit(V, 0, thr)
    batch = int(lens.sum())

    def draw(Rn, Tn, a, device):
        return (torch.tensor(case["init"], device=device),
                torch.tensor(case["noise"], dtype=torch.float64, device=device))

    env = CustomRewardEnv(GridWorldContinuous(), ThresholdGoal(0, thr))
    st, ac, rw, ln, dn = TR.collect_sample_batch(env, pol, batch, case["T"], draw=draw,
                                                 round_traj=case["n"])
    assert TR.SAMPLER_STATS["path"] == "kernel" and TR.SAMPLER_STATS["rounds"] == 1
    St, At, Rt = G.truncate(S, A, lens, dones)
    for got, want in zip((st, ac, rw, ln, dn), (St, At, Rt, lens[:, None], dones[:, None])):
        assert np.array_equal(got.cpu().numpy(), want)


def test_round_capacities_follow_their_own_plans(cuda, monkeypatch):
    """Each (env, goal kind) asks the plan of the instance that runs; the positional call keeps
    its meaning, GridWorld's ball goal."""
    from mepol_amd import ops
    from mepol_amd.algorithms import trpo as TR

    dev = torch.device("cuda", torch.cuda.current_device())
    monkeypatch.delenv("MEPOL_ROLLOUT_MW", raising=False)
    monkeypatch.delenv("MEPOL_ROLLOUT_KL", raising=False)
    for env_id, a in ((TR.MOUNTAINCAR, 1), (TR.GRIDWORLD, 2)):
        cap = TR._round_capacity(300, 300, a, dev, env_id, TR.THRESHOLD)
        plan = ops.rollout_goal_threshold_plan
        assert plan(env_id, cap, 300, 300, a)["workgroups_per_traj"] == 5
        assert plan(env_id, cap + 1, 300, 300, a)["workgroups_per_traj"] == 1
        assert plan(env_id, cap, 300, 300)["k_chunks"] == 4
        widths = (300, 300, 300)
        assert TR._round_capacity_deep(widths, a, dev, env_id, TR.THRESHOLD) == \
            ops.rollout_deep_goal_threshold_plan(env_id, widths)["resident_workgroups"] > 0
    ball = TR._round_capacity(300, 300, 2, dev)
    assert ops.rollout_goal_plan(ball, 300, 300)["workgroups_per_traj"] == 5
    assert ops.rollout_goal_plan(ball + 1, 300, 300)["workgroups_per_traj"] == 1
    assert TR._round_capacity_deep((300, 300, 300), 2, dev) == \
        ops.rollout_deep_goal_plan((300, 300, 300))["resident_workgroups"]
    monkeypatch.setenv("MEPOL_ROLLOUT_MW", "0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert TR._round_capacity(300, 300, 1, dev, TR.MOUNTAINCAR, TR.THRESHOLD) == cus


# ---- 5. end to end ----------------------------------------------------------------------------
def test_trpo_two_epochs_on_the_mountaincar_goal(cuda, tmp_path):
    """trpo() on the MountainCar goal, as test_trpo_gpu_two_epochs on GridWorld: the sampler on
    the kernel path, CSV rows written, policy and critic finite."""
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments.goal_rl import create_critic, exp_specs
    from mepol_amd.policy import GaussianPolicy

    spec = exp_specs()["MountainCarGoal"]
    torch.manual_seed(2)
    policy = GaussianPolicy(spec["hidden_sizes"], 2, 1, spec["log_std_init"]).cuda()
    vfunc = create_critic(2)
    before = dict(TR.SAMPLER_STATS)
    TR.trpo(spec["env_create"], "MountainCarGoal", 2, 600, 60, vfunc=vfunc, policy=policy,
            optimizer="lbfgs", cg_iters=10, kl_thresh=0.01, out_path=str(tmp_path), seed=3)
    assert TR.SAMPLER_STATS["kernel_batches"] == before["kernel_batches"] + 2
    assert TR.SAMPLER_STATS["host_batches"] == before["host_batches"]
    assert TR.SAMPLER_STATS["path"] == "kernel"
    lines = (tmp_path / "MountainCarGoal.csv").read_text().splitlines()
    assert lines[0] == "Epoch,NumSamples,ExecutionTime,AverageReturn,BacktrackSuccess,BacktrackIters"
    assert [r.split(",")[:2] for r in lines[1:]] == [["0", "600"], ["1", "1200"]]
    assert all(torch.isfinite(p).all() for p in policy.parameters())
    assert all(p.is_cuda and torch.isfinite(p).all() for p in vfunc.parameters())
