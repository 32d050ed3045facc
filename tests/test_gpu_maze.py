"""The box maze (the kernels' env 2) on the GPU: the step kernel, every one-launch rollout route
with its goal kinds, MEPOL's particle collection and TRPO's samplers.  All comparisons are bit
for bit: the GridWorld family has no cos().

References, never the maze kernels themselves:
  default maze     the GridWorld (env 1) kernels on the same inputs, with real random policies;
  custom mazes     the numpy class under policies whose action is computable exactly on the host
                   (mean.weight = 0, log_std = 0: action = bias + noise, one rounded f64 add), and
                   for real policies the GridWorld kernel asked for the action at every state the
                   maze run visited (the policy arithmetic does not depend on the env);
  goal modes       the un-terminated records cut where the HOST goal test fires.
Every output buffer starts as 0xff bytes, so an element a call left alone is NaN or -1.
maze_cases.py holds the cases; test_maze_cases_host.py proves they meet every wall and bound."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import goal_rl_cases as G
import maze_cases as MC
import rollout_cases as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

CUSTOM = ("four_rooms", "sixteen")
ROUTES = [("step", None), ("one-wg", None), ("multi-wg", None), ("deep", None)] + [
    (form, goal) for form in ("one-wg", "multi-wg", "deep") for goal in ("ball", "thr0", "thr1")]
ROUTE_IDS = [f if g is None else f"{f}-{g}" for f, g in ROUTES]


def _ff(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _dev(x, dtype=None):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(a, b):
    """Equal bit for bit; a NaN equals a NaN whatever its payload."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    eq = _bits(a) == _bits(b)
    if a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


_GPU = {}


def _gpu(pol):
    if id(pol) not in _GPU:
        _GPU[id(pol)] = (pol, copy.deepcopy(pol).cuda())
    return _GPU[id(pol)][1]


def _layers(pol):
    return [(m.weight.detach(), m.bias.detach()) for m in pol.net if isinstance(m, nn.Linear)]


def _set_form(monkeypatch, env_id, hidden, form, goal):
    """Select the two-layer form and assert that the plan of the instance that runs (env x goal
    kind) reports it."""
    from mepol_amd import ops

    h0, h1 = hidden
    monkeypatch.setenv("MEPOL_ROLLOUT_MW", "1" if form == "multi-wg" else "0")
    if goal is None:
        plan = ops.rollout_mlp_plan(MC.N, h0, h1, 2, env_id=env_id)
    elif goal == "ball":
        plan = ops.rollout_goal_plan(MC.N, h0, h1, 2, env_id=env_id)
    else:
        plan = ops.rollout_goal_threshold_plan(env_id, MC.N, h0, h1, 2)
    m = R.mw_model(h0, h1, 2)
    assert plan["k_chunks"] == R.K_CHUNKS
    assert plan["workgroups_per_traj"] == (m["np"] if form == "multi-wg" and m["accepted"] else 1)


def _roll(env_id, mz, pol, init, noise, goal=None):
    """One launch of the route the policy's depth and `goal` name, on GridWorld (env_id 1) or a
    maze (2): numpy (S, A, V) without a goal, (S, A, rewards, len, done) with (kind, ...)."""
    from mepol_amd import ops

    dev = _gpu(pol)
    layers = _layers(dev)
    Tn, n, a = noise.shape
    head = (dev.mean.weight.detach(), dev.mean.bias.detach(), dev.log_std.detach(),
            _dev(init), _dev(noise, torch.float64))
    kw = dict(maze=mz) if env_id == 2 else {}
    S, A = _ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32)
    if goal is None:
        V = _ff((n, Tn, 2), torch.float64)
        if len(layers) == 2:
            ops.rollout_mlp(env_id, *layers[0], *layers[1], *head, S, A, visited=V, **kw)
        else:
            ops.rollout_deep(env_id, layers, *head, S, A, visited=V, **kw)
        return [x.cpu().numpy() for x in (S, A, V)]
    out = (S, A, _ff((n, Tn), torch.float32), _ff((n,), torch.int32), _ff((n,), torch.int32))
    if goal[0] == "ball":
        if len(layers) == 2:
            ops.rollout_goal(*layers[0], *layers[1], *head, goal[1], goal[2], *out, env_id=env_id,
                             **kw)
        else:
            ops.rollout_deep_goal(layers, *head, goal[1], goal[2], *out, env_id=env_id, **kw)
    elif len(layers) == 2:
        ops.rollout_goal_threshold(env_id, *layers[0], *layers[1], *head, goal[1], goal[2], *out,
                                   **kw)
    else:
        ops.rollout_deep_goal_threshold(env_id, layers, *head, goal[1], goal[2], *out, **kw)
    return [x.cpu().numpy() for x in out]


def _stepped(env_id, mz, pol, init, noise):
    """The per-step route: T launches of ops.rollout_step, the mean from the policy's own layers
    as algorithms/mepol.py computes it.  (S, A, V)."""
    from mepol_amd import ops

    dev = _gpu(pol)
    Tn, n, a = noise.shape
    env = _dev(init)
    pin = env.to(torch.float64).contiguous()
    nz = _dev(noise, torch.float64)
    S, A = _ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32)
    V = _ff((n, Tn, 2), torch.float64)
    S[:, 0] = env
    log_std = dev.log_std.detach().contiguous()
    kw = dict(maze=mz) if env_id == 2 else {}
    with torch.no_grad():
        for t in range(Tn):
            mean = dev.mean_action(pin).contiguous()
            ops.rollout_step(env_id, None, env, mean, nz[t], log_std, t, Tn, S, A, pin, **kw)
            V[:, t].copy_(pin)
    assert torch.equal(env.to(torch.float64), pin)
    return [x.cpu().numpy() for x in (S, A, V)]


def _run(monkeypatch, env_id, mz, case, form, goal_name, policy_of, goal_of=None):
    """The case on one route.  goal_of(S, V) -> the goal's arguments, from the un-terminated
    records of the SAME env and route (a second launch)."""
    hidden = case["deep"] if form == "deep" else case["hidden"]
    pol = policy_of(hidden)
    if form == "step":
        return _stepped(env_id, mz, pol, case["init"], case["noise"]), None
    if form != "deep":
        _set_form(monkeypatch, env_id, hidden, form, None if goal_name is None else
                  "ball" if goal_name == "ball" else "thr")
    free = _roll(env_id, mz, pol, case["init"], case["noise"])
    if goal_name is None:
        return free, None
    goal = goal_of(free[0], free[2])
    return _roll(env_id, mz, pol, case["init"], case["noise"], goal), goal


def _goal_from(goal_name):
    def make(S, V):
        if goal_name == "ball":
            return ("ball", *MC.ball_goal(S))
        coord = int(goal_name[-1])
        return ("thr", coord, float(V[1, MC.GOAL_T - 1, coord]))

    return make


def _host_episodes(goal, S, V):
    hit = (MC.ball_hits(S, goal[1], goal[2]) if goal[0] == "ball"
           else MC.threshold_hits(V, goal[1], goal[2]))
    return MC.first_hit(hit)


def _assert_cut(got, S, A, lens, dones):
    """The outputs equal the un-terminated records cut at these episodes, bit for bit, with
    positive zeros behind each episode, reward 1 only on a terminated episode's last step, and no
    byte left as the caller's 0xff."""
    St, At, Rt = G.truncate(S, A, lens, dones)
    s, a, r, ln, dn = got
    assert np.array_equal(ln, lens), (ln, lens)
    assert np.array_equal(dn, np.asarray(dones).astype(np.int32)), (dn, dones)
    assert np.array_equal(s, St, equal_nan=True) and np.array_equal(a, At, equal_nan=True)
    assert np.array_equal(r, Rt)
    assert not np.signbit(s[St == 0]).any() and not np.signbit(a[At == 0]).any()
    assert not np.signbit(r).any()


# ---- 1. the step kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.NAMES)
def test_step_kernel_on_the_edge_set(cuda, name):
    from mepol_amd import ops

    mz, e = MC.maze(name), MC.edge_steps(name)
    want = MC.class_steps(mz, e["S"], e["A"])
    s = _dev(e["S"])
    ops.step_maze(s, _dev(e["A"]), mz)
    got = s.cpu().numpy()
    bad = [nm for nm, g, w in zip(e["name"], got, want) if not _same(g, w)]
    assert not bad, bad
    # the same rows through the fused per-step kernel: mean 0, noise = A, log_std 0
    n = len(e["S"])
    st = _dev(e["S"])
    states, actions = _ff((n, 2, 2), torch.float32), _ff((n, 1, 2), torch.float32)
    pin = _ff((n, 2), torch.float64)
    zeros = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    ops.rollout_step(2, None, st, zeros, _dev(e["A"]), zeros[0].clone(), 0, 1, states, actions, pin,
                     maze=mz)
    assert _same(st.cpu().numpy(), want) and _same(states.cpu().numpy()[:, 1], want)
    assert _same(pin.cpu().numpy(), want.astype(np.float64))
    with np.errstate(over="ignore"):
        assert _same(actions.cpu().numpy()[:, 0], e["A"].astype(np.float32))


@pytest.mark.parametrize("golden", ["env_gw", "env_gw_edges"])
def test_default_maze_step_reproduces_the_golden_vectors(cuda, golden):
    from mepol_amd import ops

    z = load_golden(golden)
    s = _dev(np.ascontiguousarray(z["S"]))
    ops.step_maze(s, _dev(z["A"], torch.float64), MC.maze("gridworld"))
    assert _same(s.cpu().numpy(), np.ascontiguousarray(z["NS"]))


# ---- 2. the default maze against the GridWorld kernels, real policies ----------------------------
@pytest.mark.parametrize("form,goal_name", ROUTES, ids=ROUTE_IDS)
def test_default_maze_equals_the_gridworld_kernels(cuda, monkeypatch, form, goal_name):
    mz = MC.maze("gridworld")
    ended = 0
    for case in MC.rollout_cases("gridworld"):
        want, goal = _run(monkeypatch, 1, None, case, form, goal_name, MC.real_policy,
                          None if goal_name is None else _goal_from(goal_name))
        fixed = None if goal is None else (lambda S, V, g=goal: g)
        got, _ = _run(monkeypatch, 2, mz, case, form, goal_name, MC.real_policy, fixed)
        assert len(got) == len(want) == (3 if goal is None else 5)
        for g, w in zip(got, want):
            assert _same(g, w), (case["name"], form, goal_name)
        if goal is not None:
            ended += int(got[4].sum())
    assert goal_name is None or ended > 0


# ---- 3. custom mazes against the numpy class, exactly computable actions -------------------------
@pytest.mark.parametrize("form,goal_name", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("name", CUSTOM)
def test_custom_maze_equals_the_numpy_class(cuda, monkeypatch, name, form, goal_name):
    mz = MC.maze(name)
    ended = 0
    for c, case in enumerate(MC.rollout_cases(name)):
        S, A, V, _ = MC.class_rollout(name, c)
        goal = None if goal_name is None else _goal_from(goal_name)(S, V)
        got, _ = _run(monkeypatch, 2, mz, case, form, goal_name, MC.exact_policy,
                      None if goal is None else (lambda S_, V_, g=goal: g))
        if goal is None:
            assert _same(got[0], S) and _same(got[1], A) and _same(got[2], V), (case["name"], form)
        else:
            lens, dones = _host_episodes(goal, S, V)
            _assert_cut(got, S, A, lens, dones)
            ended += int(dones.sum())
    assert goal_name is None or ended > 0


# ---- 4. custom mazes with real policies: the action at every visited state -----------------------
@pytest.mark.parametrize("kind", ["two-layer", "deep"])
@pytest.mark.parametrize("name", CUSTOM)
def test_custom_maze_actions_along_the_trajectory(cuda, monkeypatch, name, kind):
    monkeypatch.setenv("MEPOL_ROLLOUT_MW", "0")
    mz = MC.maze(name)
    moved = 0
    for case in MC.rollout_cases(name)[:2]:
        pol = MC.real_policy(case["deep"] if kind == "deep" else case["hidden"])
        S, A, V = _roll(2, mz, pol, case["init"], case["noise"])
        assert _same(V.astype(np.float32), S[:, 1:]) and _same(S[:, 0], case["init"])
        for t in range(MC.T):
            # GridWorld's kernel for one step from the state the maze run was in
            _, A1, _ = _roll(1, None, pol, S[:, t], case["noise"][t:t + 1])
            assert _same(A1[:, 0], A[:, t]), (case["name"], kind, t)
        moved += int((_bits(S[:, 1:]) != _bits(S[:, :-1])).any(axis=2).sum())
        # and the states are the class's under those recorded f64 actions' clipped moves: every
        # state lies in no wall's interior and inside the bounds
        for p in S.reshape(-1, 2):
            walls, bounds = MC.blockers(mz, float(p[0]), float(p[1]))
            assert not bounds and all(
                p[0] in (mz.walls[w][0], mz.walls[w][1]) or p[1] in (mz.walls[w][2], mz.walls[w][3])
                for w in walls), (case["name"], p)
    assert moved > 0


# ---- 5. MEPOL's particle collection ---------------------------------------------------------------
def _spy(monkeypatch, names):
    from mepol_amd import ops

    calls = []
    for nm in names:
        real = getattr(ops, nm)

        def wrapped(*a, _real=real, _nm=nm, **kw):
            calls.append((_nm, a[0], kw.get("maze")))
            return _real(*a, **kw)

        monkeypatch.setattr(ops, nm, wrapped)
    return calls


def _collect(env, pol, seed=5, nt=4, T=6, **kw):
    from mepol_amd.algorithms import mepol as M

    g = torch.Generator(device="cuda").manual_seed(seed)
    st, ac, rtl, nxt = M.collect_particles_device(env, pol, nt, T, None, generator=g, **kw)
    return st.cpu().numpy(), ac.cpu().numpy()


def test_mepol_collects_particles_on_a_maze(cuda, monkeypatch):
    from mepol_amd import _lib
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.envs import ErgodicEnv
    from mepol_amd.policy import GaussianPolicy

    for k in ("MEPOL_ROLLOUT_FUSED", "MEPOL_ROLLOUT_GRAPH", "MEPOL_ROLLOUT_MW"):
        monkeypatch.delenv(k, raising=False)
    fr, six = MC.maze("four_rooms"), MC.maze("sixteen")
    env = ErgodicEnv(fr)
    torch.manual_seed(4)
    two = GaussianPolicy([300, 300], 2, 2, -1.5).cuda()
    deep = GaussianPolicy([64, 64, 64], 2, 2, -1.5).cuda()
    calls = _spy(monkeypatch, ["rollout_mlp", "rollout_deep", "rollout_step"])
    # the one-launch kernels, with `visited`
    vis = _ff((4, 6, 2), torch.float64)
    s2, a2 = _collect(env, two, visited=vis)
    assert [c[0] for c in calls] == ["rollout_mlp"] and calls[0][1:] == (2, fr)
    assert _same(vis.cpu().numpy().astype(np.float32), s2[:, 1:])
    del calls[:]
    sd, ad = _collect(env, deep)
    assert [c[0] for c in calls] == ["rollout_deep"] and calls[0][1:] == (2, fr)
    assert np.isfinite(s2).all() and np.isfinite(sd).all() and np.isfinite(ad).all()
    # a 2-way shard concatenates to the unsharded rollout
    parts = [_collect(env, two, shard=(r, 2)) for r in range(2)]
    assert _same(np.concatenate([p[0] for p in parts]), s2)
    assert _same(np.concatenate([p[1] for p in parts]), a2)
    # MEPOL_ROLLOUT_FUSED=0: the replayed per-step graph, equal to the eager loop bit for bit
    monkeypatch.setenv("MEPOL_ROLLOUT_FUSED", "0")
    del calls[:]
    sg, ag = _collect(env, two)
    assert {c[0] for c in calls} == {"rollout_step"} and len(calls) == 1 + 6
    assert all(c[1] == 2 and isinstance(c[2], _lib.Maze) for c in calls)
    graphs = M._ROLLOUT_GRAPHS[two]
    assert len(graphs) == 1
    monkeypatch.setenv("MEPOL_ROLLOUT_GRAPH", "0")
    se, ae = _collect(env, two)
    assert _same(sg, se) and _same(ag, ae)
    vis = _ff((4, 6, 2), torch.float64)
    sv, av = _collect(env, two, visited=vis)       # eager, with `visited`
    assert _same(sv, se) and _same(vis.cpu().numpy().astype(np.float32), se[:, 1:])
    # two mazes with the same shapes do not share a captured graph
    env6 = ErgodicEnv(six)
    s6e, a6e = _collect(env6, two)
    monkeypatch.delenv("MEPOL_ROLLOUT_GRAPH")
    s6g, a6g = _collect(env6, two)
    assert len(M._ROLLOUT_GRAPHS[two]) == 2
    assert _same(s6g, s6e) and _same(a6g, a6e)
    sg2, ag2 = _collect(env, two)                   # the first maze's graph again
    assert len(M._ROLLOUT_GRAPHS[two]) == 2 and _same(sg2, sg) and _same(ag2, ag)
    # the per-step records obey the walls the one-launch run obeyed: same start states
    assert _same(sg[:, 0], s2[:, 0])


# ---- 6. TRPO's samplers ---------------------------------------------------------------------------
def _check_batch(mz, out, batch, T):
    """The invariants of a sampled batch: lengths, dones, budget, zero tails; and the maze's: no
    state in a wall's interior or on / outside a bound, no move longer than max_delta."""
    st, ac, rw, ln, dn = [x.cpu().numpy() for x in out]
    lens, dones = ln[:, 0], dn[:, 0]
    m = len(lens)
    assert st.shape == (m, T + 1, 2) and ac.shape == (m, T, 2) and rw.shape == (m, T)
    assert int(lens.sum()) == batch and (lens >= 1).all() and (lens <= T).all()
    for i in range(m):
        L = int(lens[i])
        assert not st[i, L + 1:].any() and not ac[i, L:].any() and not rw[i, L:].any()
        if dones[i]:
            assert rw[i, L - 1] == 1 and not rw[i, :L - 1].any()
        else:
            assert not rw[i].any() and (L == T or i == m - 1)
        assert (np.abs(np.diff(st[i, :L + 1].astype(np.float64), axis=0))
                <= mz.max_delta + 1e-5).all()
        for p in st[i, :L + 1]:
            walls, bounds = MC.blockers(mz, float(p[0]), float(p[1]))
            assert not bounds and all(
                p[0] in (mz.walls[w][0], mz.walls[w][1]) or p[1] in (mz.walls[w][2], mz.walls[w][3])
                for w in walls), p
    return lens, dones


@pytest.mark.parametrize("hidden", [(36, 64), (70, 9, 66)], ids=["two-layer", "deep"])
def test_trpo_samplers_take_the_maze(cuda, monkeypatch, hidden):
    from mepol_amd import kernel_path
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import BoxGoal, CustomRewardEnv, ThresholdGoal
    from mepol_amd.experiments.goal_rl import exp_specs

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    pol = _gpu(MC.real_policy(hidden))
    inf = float("inf")
    rooms = exp_specs()["FourRoomsGoal"]["env_create"]()
    six = MC.maze("sixteen")
    boxed = CustomRewardEnv(six, BoxGoal((-2.4, -inf), (inf, inf)))
    over = CustomRewardEnv(six, ThresholdGoal(1, -1.4))
    spec = kernel_path.goal_sampler(rooms, pol)
    assert spec is not None and spec[0] is rooms.get_reward and len(spec[1]) == len(hidden)
    assert kernel_path.goal_sampler(over, pol) is not None
    assert kernel_path.goal_sampler(boxed, pol) is None
    cut = kernel_path.cut_sampler(boxed, pol)
    assert cut is not None and cut[0] is boxed.get_reward and cut[2] == 2
    T = 12
    for env, batch, path in ((rooms, 50, "kernel"), (over, 100, "kernel"), (boxed, 100, "cut")):
        env.seed(1)
        before = dict(TR.SAMPLER_STATS)
        g = torch.Generator(device="cuda").manual_seed(9)
        out = TR.collect_sample_batch(env, pol, batch, T, generator=g)
        assert TR.SAMPLER_STATS["path"] == path and TR.SAMPLER_STATS["rounds"] >= 1
        assert TR.SAMPLER_STATS[path + "_batches"] == before[path + "_batches"] + 1
        assert TR.SAMPLER_STATS["host_batches"] == before["host_batches"]
        lens, dones = _check_batch(env.env, out, batch, T)
        if env is not rooms:
            # the goal lies a few steps from the start box: some episodes end there
            assert dones.any() and (lens[dones] < T).any()
            st = out[0].cpu().numpy()
            for i in np.flatnonzero(dones):
                end, before_end = st[i, lens[i]], st[i, 1:lens[i]]
                if env is boxed:
                    assert end[0] >= -2.4 and (before_end[:, 0] < -2.4).all()
                else:
                    assert end[1] >= -1.4 and (before_end[:, 1] < -1.4).all()


def test_trpo_two_epochs_on_four_rooms(cuda, tmp_path, monkeypatch):
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments.goal_rl import create_critic, exp_specs
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_TRPO_SAMPLER", raising=False)
    name = "FourRoomsGoal"
    spec = exp_specs()[name]
    torch.manual_seed(2)
    policy = GaussianPolicy(spec["hidden_sizes"], 2, 2, spec["log_std_init"]).cuda()
    vfunc = create_critic(2)
    before = dict(TR.SAMPLER_STATS)
    TR.trpo(spec["env_create"], name, 2, 600, 40, vfunc=vfunc, policy=policy, optimizer="lbfgs",
            cg_iters=10, kl_thresh=0.01, out_path=str(tmp_path), seed=3)
    assert TR.SAMPLER_STATS["path"] == "kernel"
    assert TR.SAMPLER_STATS["kernel_batches"] == before["kernel_batches"] + 2
    assert TR.SAMPLER_STATS["cut_batches"] == before["cut_batches"]
    assert TR.SAMPLER_STATS["host_batches"] == before["host_batches"]
    rows = [r.split(",") for r in (tmp_path / f"{name}.csv").read_text().splitlines()[1:]]
    assert len(rows) == 2 and [r[:2] for r in rows] == [["0", "600"], ["1", "1200"]]
    assert all(torch.isfinite(p).all() for p in policy.parameters())


# ---- 7. argument errors on the device path ----------------------------------------------------------
def test_maze_argument_errors(cuda):
    from mepol_amd import _lib, ops

    mz = MC.maze("four_rooms")
    case = MC.rollout_cases("four_rooms")[0]
    for hidden in (case["hidden"], case["deep"]):
        pol = _gpu(MC.exact_policy(hidden))
        layers = _layers(pol)
        head = (pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
                _dev(case["init"]), _dev(case["noise"], torch.float64))
        S, A = _ff((MC.N, MC.T + 1, 2), torch.float32), _ff((MC.N, MC.T, 2), torch.float32)
        extra = (_ff((MC.N, MC.T), torch.float32), _ff((MC.N,), torch.int32),
                 _ff((MC.N,), torch.int32))
        if len(layers) == 2:
            free = lambda e, **kw: ops.rollout_mlp(e, *layers[0], *layers[1], *head, S, A, **kw)
            ball = lambda e, **kw: ops.rollout_goal(*layers[0], *layers[1], *head, (5.0, 5.0), 0.1,
                                                    S, A, *extra, env_id=e, **kw)
            thr = lambda e, **kw: ops.rollout_goal_threshold(e, *layers[0], *layers[1], *head, 0,
                                                             5.0, S, A, *extra, **kw)
        else:
            free = lambda e, **kw: ops.rollout_deep(e, layers, *head, S, A, **kw)
            ball = lambda e, **kw: ops.rollout_deep_goal(layers, *head, (5.0, 5.0), 0.1, S, A,
                                                         *extra, env_id=e, **kw)
            thr = lambda e, **kw: ops.rollout_deep_goal_threshold(e, layers, *head, 0, 5.0, S, A,
                                                                  *extra, **kw)
        for call in (free, ball, thr):
            with pytest.raises(ValueError, match="env_id 2"):
                call(1, maze=mz)
            with pytest.raises(ValueError, match="needs maze"):
                call(2)
            bad = ops.maze_struct(mz)
            bad.n_walls = 17
            with pytest.raises(_lib.MepolInputError, match="n_walls"):
                call(2, maze=bad)
        # nothing above launched: the records are still the caller's bytes
        assert (S.view(torch.uint8) == 0xFF).all() and (A.view(torch.uint8) == 0xFF).all()
