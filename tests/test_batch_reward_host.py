"""The batched reward protocol (envs.BatchReward) on the CPU: BoxGoal and AnyGoal against
hand-placed rows, GridGoal.batch / ThresholdGoal.batch against their own hit() on the rows of the
existing goal case families, the derived __call__, the gates on a CPU policy and the new goal_rl
specs."""
import numpy as np
import pytest
import torch

import rollout_cases as R
import threshold_goal_cases as TC

INF = float("inf")


def _up(x):
    return float(np.nextafter(np.float64(x), INF))


def _down(x):
    return float(np.nextafter(np.float64(x), -INF))


def _batch(goal, rows):
    """(reward [k], done [k]) of goal.batch over rows [k, nf], laid out as [1, k, nf]."""
    x = torch.tensor(np.asarray(rows, dtype=np.float64)).reshape(1, len(rows), -1)
    reward, done = goal.batch(x)
    assert tuple(reward.shape) == tuple(done.shape) == (1, len(rows))
    assert done.dtype == torch.bool and reward.is_floating_point()
    assert torch.equal(reward.to(torch.float64), done.to(torch.float64))  # reward = done as 0/1
    return reward[0].numpy(), done[0].numpy()


# ---- BoxGoal ---------------------------------------------------------------------------------
LOW, HIGH = (-0.25, 0.1), (0.5, 0.3)
BOX_ROWS = [
    # (state, inside?)
    ((0.0, 0.2), True),                                    # the interior
    ((-0.25, 0.2), True), ((0.5, 0.2), True),              # on each face: the box is closed
    ((0.0, 0.1), True), ((0.0, 0.3), True),
    ((-0.25, 0.1), True), ((0.5, 0.3), True),              # corners
    ((_down(-0.25), 0.2), False), ((_up(0.5), 0.2), False),  # one f64 ulp outside each face
    ((0.0, _down(0.1)), False), ((0.0, _up(0.3)), False),
    ((_up(-0.25), 0.2), True), ((_down(0.5), 0.2), True),  # and one inside
    ((0.0, _up(0.1)), True), ((0.0, _down(0.3)), True),
    ((np.nan, 0.2), False), ((0.0, np.nan), False), ((np.nan, np.nan), False),  # NaN is no hit
    ((INF, 0.2), False), ((0.0, -INF), False),
]


def test_box_goal_faces_ulps_and_nan():
    from mepol_amd.envs import BatchReward, BoxGoal

    goal = BoxGoal(LOW, HIGH)
    assert isinstance(goal, BatchReward)
    _, done = _batch(goal, [s for s, _ in BOX_ROWS])
    assert done.tolist() == [inside for _, inside in BOX_ROWS]
    for s, inside in BOX_ROWS:                             # the derived __call__, row by row
        out = goal(np.array(s), -3.0, False, {})
        assert out == ((1.0, True) if inside else (0.0, False))
        assert type(out[0]) is float and type(out[1]) is bool


def test_box_goal_infinite_bounds():
    from mepol_amd.envs import BoxGoal

    left = BoxGoal((-INF, -INF), (-1.1, INF))              # goal_rl's MountainCarLeft
    rows = [((-1.1, 0.0), True), ((_up(-1.1), 0.0), False), ((_down(-1.1), 0.07), True),
            ((-1.2, -0.07), True), ((-INF, INF), True), ((0.45, 0.0), False),
            ((np.nan, 0.0), False), ((-1.15, np.nan), False)]
    assert _batch(left, [s for s, _ in rows])[1].tolist() == [hit for _, hit in rows]
    everything = BoxGoal((-INF, -INF), (INF, INF))
    assert _batch(everything, [(0.0, 0.0), (INF, -INF), (np.nan, 0.0)])[1].tolist() == [
        True, True, False]
    with pytest.raises(ValueError):
        BoxGoal((0.0, np.nan), (1.0, 1.0))
    with pytest.raises(ValueError):
        BoxGoal((0.0,), (1.0, 1.0))


# ---- AnyGoal ---------------------------------------------------------------------------------
def test_any_goal_is_the_or_of_its_members():
    from mepol_amd.envs import AnyGoal, BatchReward, BoxGoal, GridGoal, ThresholdGoal

    box, east, ball = BoxGoal(LOW, HIGH), ThresholdGoal(0, 3.5), GridGoal((2, 5))
    goal = AnyGoal(box, east, ball)
    assert isinstance(goal, BatchReward)
    rows = [s for s, _ in BOX_ROWS] + [(3.5, -4.0), (_down(3.5), -4.0), (2.0, 4.9375),
                                       (-5.0, -5.0), (np.nan, 5.0)]
    members = [_batch(g, rows)[1] for g in (box, east, ball)]
    reward, done = _batch(goal, rows)
    assert np.array_equal(done, members[0] | members[1] | members[2])
    assert [m.any() and not m.all() for m in members] == [True] * 3
    for k, m in enumerate(members):                        # each member alone decides some row
        others = members[(k + 1) % 3] | members[(k + 2) % 3]
        assert (m & ~others).any(), k
    assert np.array_equal(_batch(AnyGoal(box), rows)[1], members[0])   # one member
    out = goal(np.array([3.5, -4.0], dtype=np.float32), 0, False, {})
    assert out == (1.0, True) and type(out[0]) is float and type(out[1]) is bool
    assert goal(np.array([0.0, 0.0], dtype=np.float32), 0, False, {}) == (0.0, False)
    with pytest.raises(ValueError):
        AnyGoal()
    with pytest.raises(ValueError):
        AnyGoal(box, lambda s, r, d, i: (0, False))


# ---- GridGoal.batch / ThresholdGoal.batch: hit() restated ---------------------------------------
@pytest.mark.parametrize("case", R.goal_cases(), ids=lambda c: c["name"])
def test_grid_goal_batch_equals_hit_on_the_goal_cases(case):
    from mepol_amd.envs import BatchReward, GridGoal

    S, _ = R.oracle(case)                                  # f32 [n, T+1, 2]
    reached = S[:, 1:]
    x = torch.tensor(reached.astype(np.float64))
    hits = 0
    for label, g, radius, ends in R.goal_settings(S):
        goal = GridGoal(g, radius)
        assert not isinstance(goal, BatchReward)
        reward, done = goal.batch(x)
        want = goal.hit(reached)
        assert done.dtype == torch.bool and np.array_equal(done.numpy(), want), label
        assert np.array_equal(reward.numpy(), want.astype(np.float32)), label
        assert bool(want[0, R.GOAL_T - 1]) == ends, label
        hits += int(want.sum())
        for i, t in ((0, R.GOAL_T - 1), (1, 0)):           # __call__ is the reference's, unchanged
            assert goal(reached[i, t], 0, False, {}) == ((1, True) if want[i, t] else (0, False))
    assert hits > 0


def _threshold_rows():
    """(name, V f64 [n, T, 2], [(coord, threshold)]) from threshold_goal_cases: the climb to the
    hilltop, and rollouts with thresholds at their own values and one ulp above."""
    out = []
    for hidden in TC.TWO_LAYER:
        V, _, _, _ = TC.climb_f64(hidden)
        out.append((f"climb-{hidden}", V, [TC.HILLTOP, (1, 0.07), (0, -INF), (1, INF)]))
        for case in (TC.mc_case(hidden), TC.gw_case(hidden)):
            S, _ = R.oracle(case)
            V = S[:, 1:].astype(np.float64)
            at = [float(V[0, R.GOAL_T - 1, c]) for c in (0, 1)]
            out.append((case["name"], V, [(0, at[0]), (0, _up(at[0])), (1, at[1]),
                                          (1, _up(at[1]))]))
    return out


def test_threshold_goal_batch_equals_hit_on_the_threshold_cases():
    from mepol_amd.envs import BatchReward, ThresholdGoal

    hits = misses = 0
    for name, V, settings in _threshold_rows():
        withnan = V.copy()
        withnan[-1, -1, :] = np.nan                        # a NaN state is no hit
        for coord, thr in settings:
            goal = ThresholdGoal(coord, thr)
            assert not isinstance(goal, BatchReward)
            for rows in (V, withnan):
                with np.errstate(invalid="ignore"):
                    want = goal.hit(rows)
                reward, done = goal.batch(torch.tensor(rows))
                assert done.dtype == torch.bool and np.array_equal(done.numpy(), want), name
                assert np.array_equal(reward.numpy(), want.astype(np.float32)), name
                lens, dones = TC.first_hit(rows, coord, thr)
                assert np.array_equal(dones, want.any(axis=1))
            hits += int(want.sum())
            misses += int((~want).sum())
    assert hits > 0 and misses > 0


# ---- the derived __call__ --------------------------------------------------------------------
def test_derived_call_agrees_with_batch_and_returns_python_scalars():
    from mepol_amd.envs import BatchReward, CustomRewardEnv, MountainCarContinuous

    class Shaped(BatchReward):
        """A shaped reward of the state alone: -|p - 0.45| every step, done at the hilltop."""

        def batch(self, states):
            p = states[..., 0]
            return -(p - 0.45).abs(), p >= 0.45

    goal = Shaped()
    rows = np.array([[0.45, 0.0], [0.2, 0.01], [-1.2, -0.07], [np.nan, 0.0]])
    reward, done = goal.batch(torch.tensor(rows).reshape(1, 4, 2))
    for k, row in enumerate(rows):
        for s in (row, row.astype(np.float32), list(row)):
            r, d = goal(s, 123.0, True, {"x": 1})
            assert type(r) is float and type(d) is bool
            want = goal.batch(torch.tensor(np.asarray(s, dtype=np.float64)).reshape(1, 1, 2))
            assert (r == float(want[0])) or (r != r and float(want[0]) != float(want[0]))
            assert d == bool(want[1])
        r, d = goal(row, 0, False, {})
        assert d == bool(done[0, k]) and (r == float(reward[0, k]) or r != r)
    # through CustomRewardEnv: the host loop tests `done is True`
    env = CustomRewardEnv(MountainCarContinuous(), goal)
    env.seed(0)
    s = env.reset()
    s, r, d, _ = env.step(np.array([1.0]))
    assert d is False and type(r) is float and r == -abs(float(s[0]) - 0.45)
    with pytest.raises(NotImplementedError):
        BatchReward()(rows[0], 0, False, {})


# ---- gates without a GPU ---------------------------------------------------------------------
def test_gates_decline_a_cpu_policy(monkeypatch):
    from mepol_amd import kernel_path
    from mepol_amd.envs import (AnyGoal, BoxGoal, CustomRewardEnv, GridGoal, GridWorldContinuous,
                                MountainCarContinuous)
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    torch.manual_seed(0)
    two, one = GaussianPolicy([36, 64], 2, 2, -1.5), GaussianPolicy([36, 64], 2, 1, -0.5)
    gw = CustomRewardEnv(GridWorldContinuous(), AnyGoal(GridGoal((5, 5))))
    mc = CustomRewardEnv(MountainCarContinuous(), BoxGoal((-INF, -INF), (-1.1, INF)))
    for env, pol in ((gw, two), (mc, one)):
        assert kernel_path.cut_sampler(env, pol) is None
        assert kernel_path.goal_sampler(env, pol) is None
    # kernel_env itself needs no device: the env id, or None for anything but the default envs
    assert kernel_path.kernel_env(GridWorldContinuous()) == 1
    assert kernel_path.kernel_env(MountainCarContinuous()) == 0
    assert kernel_path.kernel_env(GridWorldContinuous(dim=8)) is None
    assert kernel_path.kernel_env(gw) is None              # a wrapper is not the env

    class Steeper(MountainCarContinuous):
        pass

    assert kernel_path.kernel_env(Steeper()) is None
    other = MountainCarContinuous()
    other.power = 0.002
    assert kernel_path.kernel_env(other) is None


def test_cpu_sampler_takes_the_host_loop_with_a_batch_reward(monkeypatch):
    """On a CPU policy a BatchReward env samples through the reference's loop, which sees real
    Python bools: every trajectory but the budget-cut last one ends done or at traj_len."""
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import BoxGoal, CustomRewardEnv, GridWorldContinuous
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    torch.manual_seed(1)
    pol = GaussianPolicy([36, 64], 2, 2, -1.5)
    env = CustomRewardEnv(GridWorldContinuous(), BoxGoal((-INF, -INF), (INF, INF)))  # always done
    env.seed(0)
    st, ac, rw, ln, dn = TR.collect_sample_batch(env, pol, 7, 5)
    assert TR.SAMPLER_STATS["path"] == "host"
    assert ln.reshape(-1).tolist() == [1] * 7 and dn.reshape(-1).tolist() == [True] * 7
    assert rw[:, 0].tolist() == [1.0] * 7 and float(rw.sum()) == 7.0


# ---- the goal_rl specs -----------------------------------------------------------------------
def test_new_goal_rl_specs():
    from mepol_amd.envs import (AnyGoal, BoxGoal, CustomRewardEnv, GridGoal, GridWorldContinuous,
                                MountainCarContinuous)
    from mepol_amd.experiments.goal_rl import build_parser, exp_specs

    specs = exp_specs()
    env = specs["GridGoalAny"]["env_create"]()
    assert type(env) is CustomRewardEnv and type(env.env) is GridWorldContinuous
    goal = env.get_reward
    assert type(goal) is AnyGoal and [type(g) for g in goal.goals] == [GridGoal] * 3
    assert [tuple(g.goal) for g in goal.goals] == [(5, 5), (2, 5), (5, 2)]
    assert all(g.radius == 0.1 for g in goal.goals)
    for key in ("hidden_sizes", "activation", "log_std_init"):   # the GridGoal policy spec
        assert specs["GridGoalAny"][key] == specs["GridGoal1"][key]
    for k, name in enumerate(("GridGoal1", "GridGoal2", "GridGoal3")):
        assert tuple(specs[name]["env_create"]().get_reward.goal) == tuple(goal.goals[k].goal)

    env = specs["MountainCarLeft"]["env_create"]()
    assert type(env) is CustomRewardEnv and type(env.env) is MountainCarContinuous
    goal = env.get_reward
    assert type(goal) is BoxGoal
    assert goal.low.tolist() == [-INF, -INF] and goal.high.tolist() == [-1.1, INF]
    for key in ("hidden_sizes", "activation", "log_std_init"):   # MountainCarGoal's policy spec
        assert specs["MountainCarLeft"][key] == specs["MountainCarGoal"][key]
    # each call builds a fresh env with a fresh reward object
    assert specs["GridGoalAny"]["env_create"]().get_reward is not specs["GridGoalAny"][
        "env_create"]().get_reward
    help_text = build_parser().format_help()
    assert "GridGoalAny" in help_text and "MountainCarLeft" in help_text
