"""Host side of the deep rollout's goal mode: the argument checks of mepol_rollout_deep_goal and
mepol_rollout_deep_goal_plan_info, which run before any launch, and the goal sampler's layer gate.
Nothing here launches a kernel or needs a GPU."""
import ctypes

import pytest


def _widths(ws):
    return (ctypes.c_int * len(ws))(*ws)


def _run(lib, env_id=1, widths=(8, 8, 8), a_dim=2, n=4, T=3, goal=(1.0, 1.0), radius=0.1,
         null=None, ws_bytes=None):
    """mepol_rollout_deep_goal on host memory: every call here must be rejected, or return,
    before a launch."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    names = ["W1", "b1", "Wt", "bt", "Wm", "bm", "log_std", "init32", "noise", "states_rec",
             "actions_rec", "rewards_rec", "len_out", "done_out"]
    a = {k: (None if k == null else p) for k in names}
    ws = (p, ws_bytes) if ws_bytes is not None else (None, 0)
    return lib.mepol_rollout_deep_goal(
        env_id, len(widths), _widths(widths), a["W1"], a["b1"], a["Wt"], a["bt"], a["Wm"], a["bm"],
        a["log_std"], a_dim, a["init32"], a["noise"], n, T, goal[0], goal[1], radius,
        a["states_rec"], a["actions_rec"], a["rewards_rec"], a["len_out"], a["done_out"], *ws, None)


NAN = float("nan")
BAD = [dict(a_dim=1), dict(a_dim=3), dict(goal=(NAN, 0.0)), dict(goal=(0.0, NAN)),
       dict(radius=-1.0), dict(radius=NAN), dict(widths=(8, 8)), dict(widths=(8,) * 7),
       dict(widths=(8, 513, 8)), dict(widths=(8, 0, 8)), dict(env_id=2), dict(env_id=-1),
       dict(null="W1"), dict(null="Wt"), dict(null="init32"), dict(null="noise"),
       dict(null="rewards_rec"), dict(null="len_out"), dict(null="done_out")]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in BAD])
def test_deep_goal_bad_arguments_fail_without_gpu(kw):
    from mepol_amd import _lib

    lib = _lib.load()
    assert _run(lib, **kw) == 1001, kw
    msg = lib.mepol_last_error_string()
    for part in (b"mepol_rollout_deep_goal", b"3 <= n_hidden <= 6", b"width <= 512", b"a_dim = 2",
                 b"radius >= 0"):
        assert part in msg, (part, msg)


def test_deep_goal_unsupported_env_empty_batch_and_short_workspace():
    from mepol_amd import _lib

    lib = _lib.load()
    assert _run(lib, env_id=0) == 1003
    assert b"only GridWorld (env_id 1) has a goal mode" in lib.mepol_last_error_string()
    assert _run(lib, n=0) == 0 and _run(lib, T=0) == 0
    assert _run(lib, env_id=0, n=0) == 0  # nothing to launch comes first, as mepol_rollout_goal
    assert _run(lib, ws_bytes=255) == 1002 and b"workspace" in lib.mepol_last_error_string()


def test_deep_goal_plan_info_arguments():
    from mepol_amd import _lib

    lib = _lib.load()
    out = ctypes.c_int(-7)
    plan = lib.mepol_rollout_deep_goal_plan_info
    assert plan(2, _widths((64, 64)), 2, ctypes.byref(out)) == 1001
    assert plan(7, _widths((8,) * 7), 2, ctypes.byref(out)) == 1001
    assert plan(3, _widths((64, 513, 64)), 2, ctypes.byref(out)) == 1001
    assert plan(3, _widths((64, 64, 64)), 1, ctypes.byref(out)) == 1001
    assert plan(3, _widths((64, 64, 64)), 2, None) == 1001
    assert b"mepol_rollout_deep_goal_plan_info" in lib.mepol_last_error_string()
    assert out.value == -7


def test_goal_sampler_layer_gate_has_no_word_cap(monkeypatch):
    """_rollout_layers(word_cap=False) takes [512] x 6, which MEPOL's own dispatch
    (_rollout_deep_layers, ROLLOUT_DEEP_MAX_WORDS) refuses; the other conditions stay."""
    import torch.nn as nn

    from mepol_amd.algorithms import mepol as M
    from mepol_amd.policy import GaussianPolicy

    for var in ("MEPOL_ROLLOUT_FUSED", "MEPOL_ROLLOUT_DEEP_MAX_WORDS"):
        monkeypatch.delenv(var, raising=False)
    wide = GaussianPolicy([512] * 6, 2, 2)
    assert M._rollout_deep_layers(wide, 2, 2) is None
    assert len(M._rollout_layers(wide, 2, 2, deep=True, word_cap=False)) == 6
    assert M._rollout_layers(GaussianPolicy([8] * 7, 2, 2), 2, 2, deep=True, word_cap=False) is None
    assert M._rollout_layers(GaussianPolicy([8, 513, 8], 2, 2), 2, 2, deep=True,
                             word_cap=False) is None
    assert M._rollout_layers(GaussianPolicy([8, 8, 8], 2, 2, activation=nn.Tanh), 2, 2, deep=True,
                             word_cap=False) is None
