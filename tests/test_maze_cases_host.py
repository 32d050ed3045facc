"""Host side of the box maze (mepol_amd/envs/maze.py, the kernels' env 2): the numpy class against
GridWorld and the reference's golden step vectors, the cases of maze_cases.py are what they claim
(so that no GPU test passes vacuously), the constructor's refusals, the gates, and the C ABI's
argument checks.  Nothing here launches a kernel or needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import maze_cases as MC
from conftest import load_golden

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "mepol_amd.h")
NEW = ["mepol_step_maze", "mepol_rollout_step_maze", "mepol_rollout_maze",
       "mepol_rollout_maze_workspace_size", "mepol_rollout_maze_plan_info",
       "mepol_rollout_deep_maze", "mepol_rollout_deep_maze_workspace_size",
       "mepol_rollout_deep_maze_plan_info"]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the class against GridWorld and the golden vectors --------------------------------------
def test_gridworld_maze_equals_gridworld_on_the_edge_set():
    from mepol_amd.envs import BoxMazeContinuous, GridWorldContinuous

    gw, mz = GridWorldContinuous(), BoxMazeContinuous.gridworld()
    assert mz.walls == [tuple(w) for w in gw.walls] and mz.max_delta == gw.max_delta
    assert mz.bounds == (-gw.dim, gw.dim, -gw.dim, gw.dim)
    assert np.array_equal(mz.init_states.low, gw.init_states.low)
    assert np.array_equal(mz.init_states.high, gw.init_states.high)
    e = MC.edge_steps("gridworld")
    assert np.array_equal(_bits(MC.class_steps(mz, e["S"], e["A"])),
                          _bits(MC.class_steps(gw, e["S"], e["A"])))
    for kw in (dict(dim=8), dict(max_delta=0.5), dict(wall_width=1.0)):
        other = BoxMazeContinuous.gridworld(**kw)
        assert other.walls == [tuple(w) for w in GridWorldContinuous(**kw).walls]


@pytest.mark.parametrize("golden", ["env_gw", "env_gw_edges"])
def test_gridworld_maze_reproduces_the_golden_step_vectors(golden):
    z = load_golden(golden)
    got = MC.class_steps(MC.maze("gridworld"), z["S"], z["A"])
    assert np.array_equal(_bits(got), _bits(z["NS"]))


@pytest.mark.parametrize("name", MC.NAMES)
def test_edge_steps_are_what_they_claim(name):
    mz, e = MC.maze(name), MC.edge_steps(name)
    NS = MC.class_steps(mz, e["S"], e["A"])
    moved = (_bits(NS) != _bits(e["S"])).any(axis=1)
    labels = list(e["name"])
    for label, exp, m in zip(labels, e["expect"], moved):
        if exp != "class":
            assert m == (exp == "free"), label
        if label.endswith("/on"):
            assert exp == "blocked", label
        if label.endswith("/ulp_in"):
            assert exp == "free", label
    # every wall has a free landing one ulp outside some side, and the last wall blocks alone
    for w in range(len(mz.walls)):
        assert any(lb.startswith(f"wall{w}/side") and lb.endswith("ulp_out") and exp == "free"
                   for lb, exp in zip(labels, e["expect"])), w
    assert e["expect"][labels.index("last_wall_only")] == "blocked"
    assert len([lb for lb in labels if lb.startswith("bound/")]) == 8
    # NaN stays NaN in its own coordinate only; +-inf and +-max_delta move by max_delta
    row = {lb: ns for lb, ns in zip(labels, NS)}
    s0 = e["S"][labels.index("nan/x")]
    assert np.isnan(row["nan/x"][0]) and not np.isnan(row["nan/x"][1])
    assert np.isnan(row["nan/y"][1]) and not np.isnan(row["nan/y"][0])
    md = mz.max_delta
    want = np.array([float(s0[0]) + md, float(s0[1]) - md], dtype=np.float32)
    for lb in ("inf/+-", "clip/at+-", "clip/past"):
        assert np.array_equal(row[lb], want), lb


# ---- 2. coverage of the rollout cases -----------------------------------------------------------
@pytest.mark.parametrize("name", MC.NAMES)
def test_rollout_cases_cover_every_wall_and_bound(name):
    mz = MC.maze(name)
    cases = MC.rollout_cases(name)
    walls_hit, bounds_hit = set(), set()
    for c, case in enumerate(cases):
        assert case["init"].shape == (MC.N, 2) and case["noise"].shape == (MC.T, MC.N, 2)
        assert case["init"].dtype == np.float32 and case["hidden"] in MC.TWO_LAYER
        S, A, V, events = MC.class_rollout(name, c)
        free = {j: 0 for j in range(MC.N)}
        for j, t, walls, bounds, moved in events:
            # the class and the restated geometry agree on every step
            assert moved == (not walls and not bounds), (case["name"], j, t)
            if moved:
                free[j] += 1
            elif walls:
                walls_hit.update(walls)
            else:
                bounds_hit.update(bounds)
        assert all(free[j] >= 1 for j in free), (case["name"], free)
        assert np.array_equal(V.astype(np.float32), S[:, 1:])
    assert walls_hit == set(range(len(mz.walls))), sorted(walls_hit)
    assert bounds_hit == {"xlo", "xhi", "ylo", "yhi"}, bounds_hit
    assert {case["hidden"] for case in cases} == set(MC.TWO_LAYER)


def test_case_shapes_reach_both_two_layer_forms():
    import rollout_cases as R

    assert set(MC.TWO_LAYER) <= set(R.SHAPES)
    models = [R.mw_model(*h) for h in MC.TWO_LAYER]
    assert [m["accepted"] for m in models] == [True, True, False]
    assert [m["np"] for m in models] == [2, 3, 1]
    assert len(MC.DEEP) == 3 and max(MC.DEEP) <= 512
    assert len(MC.maze("sixteen").walls) == 16
    xlo, xhi, ylo, yhi = MC.maze("sixteen").bounds
    assert xhi - xlo != yhi - ylo and xlo != ylo and xhi != yhi


def test_goals_taken_from_the_class_rollouts_end_episodes():
    for name in MC.NAMES:
        S, _, V, _ = MC.class_rollout(name, 0)
        goal, radius = MC.ball_goal(S)
        lens, dones = MC.first_hit(MC.ball_hits(S, goal, radius))
        assert dones[0] and lens[0] <= MC.GOAL_T and radius > 0
        for coord in (0, 1):
            thr = float(V[1, MC.GOAL_T - 1, coord])
            lens, dones = MC.first_hit(MC.threshold_hits(V, coord, thr))
            assert dones[1] and lens[1] <= MC.GOAL_T


# ---- 3. constructor refusals ---------------------------------------------------------------------
def test_constructor_refusals():
    from mepol_amd.envs import MAZE_MAX_WALLS, BoxMazeContinuous

    B = (-1.0, 1.0, -1.0, 1.0)
    wall = (0.0, 0.5, 0.0, 0.5)
    assert MAZE_MAX_WALLS == 16
    assert BoxMazeContinuous(B).walls == []                       # zero walls is legal
    assert len(BoxMazeContinuous(B, [wall] * 16).walls) == 16
    assert BoxMazeContinuous(B, [(0.2, 0.2, 0.3, 0.3)]).walls     # a degenerate box is not inverted
    inf, nan = float("inf"), float("nan")
    bad = [dict(walls=[wall] * 17),
           dict(bounds=(-1.0, inf, -1.0, 1.0)), dict(bounds=(nan, 1.0, -1.0, 1.0)),
           dict(walls=[(0.0, nan, 0.0, 0.5)]), dict(walls=[(0.0, 0.5, -inf, 0.5)]),
           dict(max_delta=inf), dict(max_delta=nan),
           dict(init_box=((-1.0, -1.0), (nan, 0.0))),
           dict(walls=[(0.5, 0.0, 0.0, 0.5)]), dict(walls=[(0.0, 0.5, 0.5, 0.0)]),
           dict(bounds=(1.0, -1.0, -1.0, 1.0)), dict(bounds=(-1.0, 1.0, 1.0, 1.0)),
           dict(init_box=((-1.5, -1.0), (0.0, 0.0))), dict(init_box=((-1.0, -1.0), (0.0, 1.5))),
           dict(init_box=((0.5, 0.0), (0.0, 0.5)))]
    for kw in bad:
        args = dict(bounds=B, walls=[wall], max_delta=0.2, init_box=((-1.0, -1.0), (0.0, 0.0)))
        args.update(kw)
        with pytest.raises(ValueError):
            BoxMazeContinuous(**args)


def test_api_and_named_mazes():
    from mepol_amd.envs import BoxMazeContinuous

    fr = BoxMazeContinuous.four_rooms()
    assert fr.batched_kind == "maze" and fr.num_features == 2 and fr.action_space.shape == (2,)
    assert fr.bounds == (-6.0, 6.0, -6.0, 6.0) and fr.max_delta == 0.2 and len(fr.walls) == 6
    assert all(min(x1 - x0, y1 - y0) == 0.5 for x0, x1, y0, y1 in fr.walls)
    # one door, 1.0 wide, in each arm of the cross
    for door in ((0.0, 3.0), (0.0, -3.0), (3.0, 0.0), (-3.0, 0.0)):
        assert MC.is_free(fr, *door)
        assert not MC.is_free(fr, door[0] * 0.5, door[1] * 0.5)
        assert not MC.is_free(fr, door[0] * 1.5, door[1] * 1.5)
    assert np.array_equal(fr.init_states.low, [-6, -6]) and np.array_equal(fr.init_states.high,
                                                                           [-4, -4])
    fr.seed(3)
    s = fr.reset()
    assert s.dtype == np.float32 and s.shape == (2,) and fr.init_states.contains(s)
    ns, r, done, info = fr.step(np.array([0.1, 0.1]))
    assert ns.dtype == np.float32 and r == 0 and done is False and info == {}
    assert "stepped over" in BoxMazeContinuous.__doc__
    assert fr.kernel_key() != BoxMazeContinuous.gridworld().kernel_key()
    assert fr.kernel_key() == BoxMazeContinuous.four_rooms().kernel_key()


# ---- 4. gates --------------------------------------------------------------------------------------
def test_gates():
    from mepol_amd import kernel_path
    from mepol_amd.envs import (BoxMazeContinuous, CustomRewardEnv, ErgodicEnv, GridGoal,
                                GridWorldContinuous, MountainCarContinuous)

    assert (kernel_path.MOUNTAINCAR, kernel_path.GRIDWORLD, kernel_path.MAZE) == (0, 1, 2)
    assert kernel_path.ENV_ACTIONS == (1, 2, 2)
    for name in MC.NAMES:
        assert kernel_path.kernel_env(MC.maze(name)) == 2
    assert kernel_path.kernel_env(BoxMazeContinuous((-1.0, 1.0, -1.0, 1.0))) == 2

    class Mine(BoxMazeContinuous):
        pass

    assert kernel_path.kernel_env(Mine((-1.0, 1.0, -1.0, 1.0))) is None
    assert kernel_path.kernel_env(ErgodicEnv(MC.maze("four_rooms"))) is None  # a wrapper
    # what the existing gate tests assert of GridWorld and MountainCar objects still holds
    assert kernel_path.kernel_env(GridWorldContinuous()) == 1
    assert kernel_path.kernel_env(MountainCarContinuous()) == 0
    assert kernel_path.kernel_env(GridWorldContinuous(dim=8)) is None
    assert kernel_path.kernel_env(CustomRewardEnv(GridWorldContinuous(), GridGoal((5, 5)))) is None

    class Steeper(MountainCarContinuous):
        pass

    class Wider(GridWorldContinuous):
        pass

    assert kernel_path.kernel_env(Steeper()) is None and kernel_path.kernel_env(Wider()) is None
    other = MountainCarContinuous()
    other.power = 0.002
    assert kernel_path.kernel_env(other) is None
    assert kernel_path.maze_of(MC.maze("sixteen"), 2) is MC.maze("sixteen")
    assert kernel_path.maze_of(GridWorldContinuous(), 1) is None
    # a CPU policy takes the host loop on a maze as on GridWorld
    from mepol_amd.policy import GaussianPolicy

    env = CustomRewardEnv(MC.maze("four_rooms"), GridGoal((5, 5)))
    assert kernel_path.goal_sampler(env, GaussianPolicy([8, 8], 2, 2)) is None
    assert kernel_path.cut_sampler(env, GaussianPolicy([8, 8], 2, 2)) is None


def test_cli_specs_and_help():
    from mepol_amd.envs import BoxMazeContinuous, CustomRewardEnv, ErgodicEnv, GridGoal, unwrap
    from mepol_amd.experiments import goal_rl, mepol

    spec = mepol.exp_specs()["FourRooms"]
    env = spec["env_create"]()
    assert type(env) is ErgodicEnv and type(unwrap(env)) is BoxMazeContinuous
    assert unwrap(env).kernel_key() == BoxMazeContinuous.four_rooms().kernel_key()
    gw = mepol.exp_specs()["GridWorld"]
    assert all(spec[k] == gw[k] for k in ("hidden_sizes", "activation", "log_std_init", "eps"))
    disc = spec["discretizer_create"](env)
    assert list(disc.bins_sizes) == [20, 20]
    assert "FourRooms" in mepol.build_parser().format_help()
    spec = goal_rl.exp_specs()["FourRoomsGoal"]
    env = spec["env_create"]()
    assert type(env) is CustomRewardEnv and type(env.env) is BoxMazeContinuous
    assert isinstance(env.get_reward, GridGoal)
    assert np.array_equal(env.get_reward.goal, np.array([5, 5], dtype=np.float32))
    assert spec["hidden_sizes"] == [300, 300] and spec["log_std_init"] == -1.5
    assert "FourRoomsGoal" in goal_rl.build_parser().format_help()


# ---- 5. the C ABI without a device ------------------------------------------------------------------
def test_header_and_library_declare_the_maze_entry_points():
    from mepol_amd import _lib

    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert set(NEW) <= set(re.findall(r"\b(mepol_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"#define\s+MEPOL_MAZE_MAX_WALLS\s+16\b", text)
    assert re.search(r"#define\s+MEPOL_ABI_VERSION\s+4\b", text)
    assert "typedef struct mepol_maze" in text
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.mepol_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert ctypes.sizeof(_lib.Maze) == 6 * 8 + 16 * 4 * 8 and _lib.MAZE_MAX_WALLS == 16


def _maze_struct(**kw):
    from mepol_amd import ops

    m = ops.maze_struct(MC.maze("four_rooms"))
    for k, v in kw.items():
        if k == "wall":
            w, j, val = v
            m.walls[w][j] = val
        else:
            setattr(m, k, v)
    return m


INF, NAN = float("inf"), float("nan")
BAD_MAZES = {"null": None, "n_walls=-1": dict(n_walls=-1), "n_walls=17": dict(n_walls=17),
             "xhi=inf": dict(xhi=INF), "ylo=nan": dict(ylo=NAN), "max_delta=nan": dict(max_delta=NAN),
             "wall=nan": dict(wall=(5, 2, NAN)), "wall=-inf": dict(wall=(0, 0, -INF)),
             "wall-x-inverted": dict(wall=(1, 0, 5.0)), "wall-y-inverted": dict(wall=(2, 3, -5.0)),
             "bounds-x-inverted": dict(xlo=6.0, xhi=-6.0), "bounds-y-equal": dict(ylo=6.0)}


def _calls(lib, mz, a_dim=2, kind=0):
    """name -> thunk of every new entry point that takes a maze, on host memory: a call that
    passed validation would launch, so each one here must be rejected before that."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    w3 = (ctypes.c_int * 3)(8, 8, 8)
    mp = None if mz is None else ctypes.byref(mz)
    calls = {
        "mepol_rollout_step_maze": lambda: lib.mepol_rollout_step_maze(
            mp, p, p, p, p, 4, a_dim, 0, 3, p, p, p, None),
        "mepol_rollout_maze": lambda: lib.mepol_rollout_maze(
            mp, kind, p, p, 8, p, p, 8, p, p, p, a_dim, p, p, 4, 3, 0.0, 0.0, 0, 0.5, p, p, None,
            None, p, p, p, None, 0, None),
        "mepol_rollout_deep_maze": lambda: lib.mepol_rollout_deep_maze(
            mp, kind, 3, w3, p, p, p, p, p, p, p, a_dim, p, p, 4, 3, 0.0, 0.0, 0, 0.5, p, p, None,
            None, p, p, p, None, 0, None)}
    if a_dim == 2:
        calls["mepol_step_maze"] = lambda: lib.mepol_step_maze(mp, p, p, 4, None)
    return calls


@pytest.mark.parametrize("what", list(BAD_MAZES))
def test_bad_mazes_fail_without_gpu(what):
    from mepol_amd import _lib

    lib = _lib.load()
    mz = None if BAD_MAZES[what] is None else _maze_struct(**BAD_MAZES[what])
    for name, thunk in _calls(lib, mz).items():
        assert thunk() == 1001, (what, name)
        msg = lib.mepol_last_error_string()
        assert name.encode() in msg and b"maze" in msg, (what, name, msg)


def test_maze_entry_points_reject_other_bad_arguments_without_gpu():
    from mepol_amd import _lib

    lib = _lib.load()
    good = _maze_struct()
    for a_dim in (1, 3):
        for name, thunk in _calls(lib, good, a_dim=a_dim).items():
            assert thunk() == 1001, (a_dim, name)
            assert b"a_dim" in lib.mepol_last_error_string(), name
    for kind in (-1, 3):
        for name in ("mepol_rollout_maze", "mepol_rollout_deep_maze"):
            assert _calls(lib, good, kind=kind)[name]() == 1001, (kind, name)
    wg, kc, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    w3 = (ctypes.c_int * 3)(8, 8, 8)
    assert lib.mepol_rollout_maze_plan_info(0, 4, 8, 8, 1, ctypes.byref(wg), ctypes.byref(kc)) == 1001
    assert lib.mepol_rollout_maze_plan_info(3, 4, 8, 8, 2, ctypes.byref(wg), ctypes.byref(kc)) == 1001
    assert lib.mepol_rollout_maze_plan_info(0, 4, 8, 513, 2, ctypes.byref(wg),
                                            ctypes.byref(kc)) == 1001
    assert lib.mepol_rollout_maze_workspace_size(0, 4, 3, 8, 8, 3, ctypes.byref(nbytes)) == 1001
    assert lib.mepol_rollout_maze_workspace_size(0, 4, 3, 8, 8, 2, None) == 1001
    assert lib.mepol_rollout_deep_maze_plan_info(0, 3, w3, 1, ctypes.byref(wg)) == 1001
    assert lib.mepol_rollout_deep_maze_plan_info(0, 2, w3, 2, ctypes.byref(wg)) == 1001
    assert lib.mepol_rollout_deep_maze_workspace_size(4, 3, 3, w3, 2, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 256
    assert lib.mepol_rollout_deep_maze_workspace_size(4, 3, 3, w3, 1, ctypes.byref(nbytes)) == 1001
    # goal arguments: a negative radius, a NaN threshold, a coord outside 0 / 1, missing outputs
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    mp = ctypes.byref(good)

    def two(kind, gx=0.0, value=0.5, coord=0, rewards=p):
        return lib.mepol_rollout_maze(mp, kind, p, p, 8, p, p, 8, p, p, p, 2, p, p, 4, 3, gx, 0.0,
                                      coord, value, p, p, None, None, rewards, p, p, None, 0, None)

    assert two(1, value=-1.0) == 1001 and two(1, gx=NAN) == 1001 and two(1, rewards=None) == 1001
    assert two(2, value=NAN) == 1001 and two(2, coord=2) == 1001 and two(2, rewards=None) == 1001
    # an empty batch of a valid maze returns before any launch; a NULL maze does not
    assert lib.mepol_step_maze(mp, p, p, 0, None) == 0
    assert lib.mepol_step_maze(None, p, p, 0, None) == 1001
    rc = lib.mepol_rollout_deep_maze(mp, 0, 3, w3, p, p, p, p, p, p, p, 2, p, p, 4, 3, 0.0, 0.0, 0,
                                     0.0, p, p, None, None, None, None, None, p, 255, None)
    assert rc == 1002 and b"workspace" in lib.mepol_last_error_string()


def test_existing_entry_points_still_reject_env_2():
    from mepol_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    w3 = (ctypes.c_int * 3)(8, 8, 8)
    wg, kc, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.mepol_rollout_step(2, p, p, p, p, p, 4, 2, 0, 3, p, p, p, None) == 1001
    assert lib.mepol_rollout_mlp(2, p, p, 8, p, p, 8, p, p, p, 2, p, p, p, 4, 3, p, p, None, None,
                                 None, 0, None) == 1001
    assert lib.mepol_rollout_goal(2, p, p, 8, p, p, 8, p, p, p, 2, p, p, 4, 3, 0.0, 0.0, 0.5, p, p,
                                  p, p, p, None, 0, None) == 1001
    assert lib.mepol_rollout_goal_threshold(2, p, p, 8, p, p, 8, p, p, p, 2, p, p, p, 4, 3, 0, 0.5,
                                            p, p, p, p, p, None, 0, None) == 1001
    assert lib.mepol_rollout_goal_workspace_size(2, 4, 3, 8, 8, 2, ctypes.byref(nbytes)) == 1001
    assert lib.mepol_rollout_goal_threshold_plan_info(2, 4, 8, 8, 2, ctypes.byref(wg),
                                                      ctypes.byref(kc)) == 1001
    assert lib.mepol_rollout_goal_threshold_workspace_size(2, 4, 3, 8, 8, 2,
                                                           ctypes.byref(nbytes)) == 1001
    assert lib.mepol_rollout_deep(2, 3, w3, p, p, p, p, p, p, p, 2, p, p, p, 4, 3, p, p, None, None,
                                  None, 0, None) == 1001
    assert lib.mepol_rollout_deep_plan_info(2, 3, w3, 2, ctypes.byref(wg)) == 1001
    assert lib.mepol_rollout_deep_goal(2, 3, w3, p, p, p, p, p, p, p, 2, p, p, 4, 3, 0.0, 0.0, 0.5,
                                       p, p, p, p, p, None, 0, None) == 1001
    assert lib.mepol_rollout_deep_goal_threshold(2, 3, w3, p, p, p, p, p, p, p, 2, p, p, p, 4, 3, 0,
                                                 0.5, p, p, p, p, p, None, 0, None) == 1001
    assert lib.mepol_rollout_deep_goal_threshold_plan_info(2, 3, w3, 2, ctypes.byref(wg)) == 1001
    assert lib.mepol_abi_version() == 4


def test_ops_maze_argument_rules_need_no_device():
    """maze= belongs to env_id 2 and only there: both mistakes raise before any tensor is read."""
    from mepol_amd import ops

    mz = MC.maze("four_rooms")
    t = torch.zeros((2, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="env_id 2"):
        ops.rollout_step(1, None, t, t, t, t, 0, 1, t, t, t, maze=mz)
    with pytest.raises(ValueError, match="needs maze"):
        ops.rollout_step(2, None, t, t, t, t, 0, 1, t, t, t)
    m = ops.maze_struct(mz)
    assert m.n_walls == 6 and m.max_delta == 0.2 and (m.xlo, m.xhi, m.ylo, m.yhi) == (-6, 6, -6, 6)
    assert [list(m.walls[w]) for w in range(6)] == [list(w) for w in mz.walls]
    assert all(v == 0.0 for w in range(6, 16) for v in m.walls[w])
