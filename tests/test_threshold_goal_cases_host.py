"""Host side of the threshold goals: the premises of threshold_goal_cases.py, ThresholdGoal, the
host sampler on the MountainCar goal, the goal_rl spec, and the argument checks of
mepol_rollout_goal_threshold / mepol_rollout_deep_goal_threshold and their queries, which run
before any launch.  Nothing here launches a kernel or needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import rollout_cases as R
import threshold_goal_cases as TC

ALL_SHAPES = TC.TWO_LAYER + (TC.WIDE,) + TC.DEEP


# ---- the cases are what they claim -------------------------------------------------------------
@pytest.mark.parametrize("hidden", ALL_SHAPES, ids=lambda h: "x".join(map(str, h)))
def test_climb_case_premises(hidden):
    """From the independent f64 rollout on the host: the force is saturated on every step, the
    four trajectories end as CLIMB_LENS / CLIMB_DONE say (so the four kinds of episode occur),
    every comparison of the env step keeps MARGIN on every step, and within each episode the
    threshold comparison keeps CLIMB_GAP."""
    V, pre, margin, A = TC.climb_f64(hidden)
    assert A.min() > 1.0 + 1.0                      # far beyond the clip at 1
    lens, dones = TC.first_hit(V, *TC.HILLTOP)
    assert tuple(lens.tolist()) == TC.CLIMB_LENS and tuple(dones.tolist()) == TC.CLIMB_DONE
    assert TC.kinds(lens, dones, R.T) == TC.KINDS
    assert margin.min() >= R.MARGIN
    for i, L in enumerate(lens.tolist()):
        assert np.abs(pre[:L, i] - TC.HILLTOP[1]).min() >= TC.CLIMB_GAP, i
        crossed = pre[:L, i] > TC.HILLTOP[1]
        assert crossed[:-1].sum() == 0 and bool(crossed[-1]) == TC.CLIMB_DONE[i]
        # the hilltop is reached only through the wall's clip: exactly 0.45 with v = 0
        if TC.CLIMB_DONE[i]:
            assert V[i, L - 1, 0] == 0.45 and V[i, L - 1, 1] == 0.0
    assert (V[:, :, 0] <= 0.45).all()


def test_gridworld_cases_share_goal_cases_starts():
    for (h0, h1), ref in zip(TC.TWO_LAYER, R.goal_cases()):
        c = TC.gw_case((h0, h1))
        assert c["hidden"] == ref["hidden"] and np.array_equal(c["init"], ref["init"])
        assert np.array_equal(c["noise"], ref["noise"])


def test_first_hit_helper():
    V = np.array([[[0.0, 0.0], [0.5, 0.0], [0.7, 0.0]],
                  [[0.0, 0.0], [np.nan, 0.0], [np.nan, 0.0]],
                  [[0.6, 1.0], [0.0, 0.0], [0.9, 0.0]]])
    lens, dones = TC.first_hit(V, 0, 0.5)
    assert lens.tolist() == [2, 3, 1] and dones.tolist() == [True, False, True]
    lens, dones = TC.first_hit(V, 0, -np.inf)
    assert lens.tolist() == [1, 1, 1] and dones.all()     # NaN comes later in trajectory 1
    lens, dones = TC.first_hit(V, 0, np.inf)
    assert lens.tolist() == [3, 3, 3] and not dones.any()
    assert TC.first_hit(V, 1, 1.0)[0].tolist() == [3, 3, 1]


# ---- ThresholdGoal ----------------------------------------------------------------------------
def test_threshold_goal_scalar_and_vectorised_agree():
    from mepol_amd.envs import ThresholdGoal

    rng = np.random.default_rng(5)
    for dtype in (np.float64, np.float32):
        S = rng.uniform(-1, 1, (50, 2)).astype(dtype)
        S[3, 0], S[4, 1] = np.nan, np.nan
        for index in (0, 1):
            thr = float(S[7, index])  # an exact value: >= is closed
            g = ThresholdGoal(index, thr)
            with np.errstate(invalid="ignore"):
                vec = g.hit(S)
                assert vec.shape == (50,) and vec.dtype == bool and vec[7]
                assert not g.hit(S[7:8] * 0 + np.nextafter(dtype(thr), dtype(-2)))[0]
                for s, v in zip(S, vec):
                    r, d = g(s, -1.0, False, {})
                    assert (r, d) == ((1, True) if v else (0, False))
                    assert v == (float(s[index]) >= thr)
            assert not vec[3 + index]  # a NaN coordinate is no hit
    # an f32 state is widened, not the threshold narrowed
    x = np.float32(0.1)
    up = float(np.nextafter(np.float64(x), 1.0))
    assert ThresholdGoal(0, float(x)).hit(np.array([x, 0], np.float32))
    assert not ThresholdGoal(0, up).hit(np.array([x, 0], np.float32))
    assert np.float32(up) == x
    assert ThresholdGoal(0, -np.inf).hit(np.zeros(2))
    assert not ThresholdGoal(0, np.inf).hit(np.zeros(2))


# ---- the host loop on the MountainCar goal ----------------------------------------------------
class _Pump:
    """Pushes along the velocity (uphill from rest): reaches the hilltop in a few swings."""

    def predict(self, s):
        return torch.tensor([1.0 if s[1] >= 0 else -1.0])


def test_collect_host_ends_at_the_first_clipped_step():
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import CustomRewardEnv, MountainCarContinuous, ThresholdGoal

    env = CustomRewardEnv(MountainCarContinuous(), ThresholdGoal(0, 0.45))
    env.seed(4)
    Tn, batch = 400, 900
    st, ac, rw, ln, dn = (x.numpy() for x in TR.collect_sample_batch(env, _Pump(), batch, Tn))
    assert TR.SAMPLER_STATS["path"] == "host"
    assert int(ln.sum()) == batch and dn[:-1].all() and len(ln) >= 3
    top = np.float32(0.45)
    for i in range(len(ln)):
        L = int(ln[i, 0])
        assert (st[i, :L, 0] < top).all()
        if dn[i, 0]:
            assert 1 < L < Tn and st[i, L, 0] == top and st[i, L, 1] == 0
            assert rw[i, L - 1] == 1 and rw[i].sum() == 1
        else:
            assert rw[i].sum() == 0
        assert not st[i, L + 1:].any() and not ac[i, L:].any()


# ---- the command line's spec ------------------------------------------------------------------
def test_goal_rl_spec_mountaincar_goal():
    import torch.nn as nn

    from mepol_amd.envs import CustomRewardEnv, MountainCarContinuous, ThresholdGoal
    from mepol_amd.experiments import mepol as mepol_cli
    from mepol_amd.experiments.goal_rl import exp_specs

    spec = exp_specs()["MountainCarGoal"]
    env = spec["env_create"]()
    assert type(env) is CustomRewardEnv and type(env.env) is MountainCarContinuous
    assert type(env.get_reward) is ThresholdGoal
    assert (env.get_reward.index, env.get_reward.threshold) == (0, 0.45)
    assert spec["hidden_sizes"] == [300, 300] and spec["activation"] is nn.ReLU
    assert spec["log_std_init"] == -0.5
    assert env.num_features == 2 and env.action_space.shape == (1,)
    # the MEPOL command line's MountainCar policy: its checkpoints load
    pre = mepol_cli.exp_specs()["MountainCar"]
    assert pre["hidden_sizes"] == spec["hidden_sizes"] and pre["activation"] is spec["activation"]
    assert pre["log_std_init"] == spec["log_std_init"]


def test_goal_sampler_gate_without_gpu():
    """A CPU policy never takes the kernel path, whatever the env."""
    from mepol_amd import kernel_path
    from mepol_amd.envs import CustomRewardEnv, MountainCarContinuous, ThresholdGoal
    from mepol_amd.policy import GaussianPolicy

    env = CustomRewardEnv(MountainCarContinuous(), ThresholdGoal(0, 0.45))
    assert kernel_path.goal_sampler(env, GaussianPolicy([8, 8], 2, 1, -0.5)) is None
    assert tuple(getattr(env.env, k) for k in kernel_path.MOUNTAINCAR_FIELDS) == \
        kernel_path.MOUNTAINCAR_DEFAULTS


# ---- argument checks of the C ABI, before any launch ------------------------------------------
NAN = float("nan")


def _widths(ws):
    return (ctypes.c_int * len(ws))(*ws)


def _run(lib, deep, env_id=0, a_dim=None, n=4, T=3, coord=0, threshold=0.45, null=None,
         widths=None, ws_bytes=None):
    """The two launchers on host memory: every call here must be rejected, or return, before a
    launch."""
    a_dim = (1 if env_id == 0 else 2) if a_dim is None else a_dim
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    names = ["W1", "b1", "W2t", "b2", "Wm", "bm", "log_std", "init64", "init32", "noise",
             "states_rec", "actions_rec", "rewards_rec", "len_out", "done_out"]
    a = {k: (None if k == null else p) for k in names}
    ws = (p, ws_bytes) if ws_bytes is not None else (None, 0)
    tail = (a_dim, a["init64"], a["init32"], a["noise"], n, T, coord, threshold, a["states_rec"],
            a["actions_rec"], a["rewards_rec"], a["len_out"], a["done_out"], *ws, None)
    if deep:
        widths = (8, 8, 8) if widths is None else widths
        return lib.mepol_rollout_deep_goal_threshold(
            env_id, len(widths), _widths(widths), a["W1"], a["b1"], a["W2t"], a["b2"], a["Wm"],
            a["bm"], a["log_std"], *tail)
    h0, h1 = (8, 8) if widths is None else widths
    return lib.mepol_rollout_goal_threshold(env_id, a["W1"], a["b1"], h0, a["W2t"], a["b2"], h1,
                                            a["Wm"], a["bm"], a["log_std"], *tail)


BAD = [dict(coord=2), dict(coord=-1), dict(threshold=NAN),
       dict(env_id=0, a_dim=2), dict(env_id=1, a_dim=1), dict(env_id=1, a_dim=3),
       dict(env_id=0, null="init64"), dict(env_id=1, null="init32"), dict(env_id=2),
       dict(env_id=-1, a_dim=1), dict(null="W1"), dict(null="noise"), dict(null="states_rec"),
       dict(null="rewards_rec"), dict(null="len_out"), dict(null="done_out")]


@pytest.mark.parametrize("deep", [False, True], ids=["two-layer", "deep"])
@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in BAD])
def test_threshold_bad_arguments_fail_without_gpu(kw, deep):
    from mepol_amd import _lib

    lib = _lib.load()
    assert _run(lib, deep, **kw) == 1001, kw
    msg = lib.mepol_last_error_string()
    name = b"mepol_rollout_deep_goal_threshold" if deep else b"mepol_rollout_goal_threshold"
    for part in (name, b"coord 0 or 1", b"threshold not NaN"):
        assert part in msg, (part, msg)


@pytest.mark.parametrize("deep", [False, True], ids=["two-layer", "deep"])
def test_threshold_shapes_empty_batches_and_the_other_init(deep):
    from mepol_amd import _lib

    lib = _lib.load()
    for env_id in (0, 1):
        assert _run(lib, deep, env_id=env_id, n=0) == 0 and _run(lib, deep, env_id=env_id, T=0) == 0
    assert _run(lib, deep, n=0, coord=7, threshold=NAN) == 0  # nothing to launch comes first
    # shape limits are the non-goal entry points'
    wide = (8, 513, 8) if deep else (8, 513)
    assert _run(lib, deep, widths=wide) == 1001
    assert _run(lib, deep, widths=(8, 0, 8) if deep else (0, 8)) == 1001
    if deep:
        assert _run(lib, deep, widths=(8, 8)) == 1001 and _run(lib, deep, widths=(8,) * 7) == 1001
        assert _run(lib, deep, ws_bytes=255) == 1002
        assert b"workspace" in lib.mepol_last_error_string()


def test_threshold_queries_bad_arguments():
    from mepol_amd import _lib

    lib = _lib.load()
    wg, kc, nb = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_size_t(77)
    plan = lib.mepol_rollout_goal_threshold_plan_info
    ref = (ctypes.byref(wg), ctypes.byref(kc))
    assert plan(0, 4, 8, 8, 2, *ref) == 1001 and plan(1, 4, 8, 8, 1, *ref) == 1001
    assert plan(2, 4, 8, 8, 1, *ref) == 1001 and plan(0, 0, 8, 8, 1, *ref) == 1001
    assert plan(0, 4, 513, 8, 1, *ref) == 1001 and plan(0, 4, 8, 8, 1, None, None) == 1001
    assert b"mepol_rollout_goal_threshold_plan_info" in lib.mepol_last_error_string()
    size = lib.mepol_rollout_goal_threshold_workspace_size
    assert size(0, 4, 3, 8, 8, 2, ctypes.byref(nb)) == 1001
    assert size(1, 4, 3, 8, 8, 1, ctypes.byref(nb)) == 1001
    assert size(0, 4, 3, 8, 8, 1, None) == 1001
    assert size(0, -1, 3, 8, 8, 1, ctypes.byref(nb)) == 1001
    assert size(0, 0, 3, 8, 8, 1, ctypes.byref(nb)) == 0 and nb.value == 256
    deep = lib.mepol_rollout_deep_goal_threshold_plan_info
    out = ctypes.c_int(-7)
    assert deep(0, 3, _widths((8, 8, 8)), 2, ctypes.byref(out)) == 1001
    assert deep(1, 3, _widths((8, 8, 8)), 1, ctypes.byref(out)) == 1001
    assert deep(2, 3, _widths((8, 8, 8)), 1, ctypes.byref(out)) == 1001
    assert deep(0, 2, _widths((8, 8)), 1, ctypes.byref(out)) == 1001
    assert deep(0, 3, _widths((8, 8, 8)), 1, None) == 1001
    assert b"mepol_rollout_deep_goal_threshold_plan_info" in lib.mepol_last_error_string()
    assert (wg.value, kc.value, out.value) == (-7, -7, -7)
    assert lib.mepol_abi_version() == 4
