"""The goal mode of the one-launch rollout for 3 to 6 hidden layers (mepol_rollout_deep_goal,
csrc/rollout_deep.hip with GOAL = true).  The reference throughout is the non-goal path that
test_gpu_rollout_deep.py pins, ops.rollout_deep on the same policy, initial states and noise, cut
at each trajectory's first hit by goal_rl_cases.first_hit / truncate; never the goal kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import goal_rl_cases as C

pytestmark = pytest.mark.gpu

NT, T = 20, 60


def _layers(pol):
    import torch.nn as nn

    return [(m.weight.detach(), m.bias.detach()) for m in pol.net if isinstance(m, nn.Linear)]


def _unterminated(pol, init, noise):
    """ops.rollout_deep on GridWorld: (S [n, T+1, 2], A [n, T, 2]) as read-only numpy arrays."""
    from mepol_amd import ops

    Tn, n, a = noise.shape
    states = torch.zeros((n, Tn + 1, 2), dtype=torch.float32, device="cuda")
    actions = torch.zeros((n, Tn, a), dtype=torch.float32, device="cuda")
    ops.rollout_deep(1, _layers(pol), pol.mean.weight.detach(), pol.mean.bias.detach(),
                     pol.log_std.detach(), torch.tensor(init, device="cuda"),
                     torch.tensor(noise, dtype=torch.float64, device="cuda"), states, actions)
    S, A = states.cpu().numpy(), actions.cpu().numpy()
    S.setflags(write=False)
    A.setflags(write=False)
    return S, A


@functools.lru_cache(maxsize=None)
def _case(hidden, nt, Tn):
    """(policy, init, noise, S, A): test_gpu_goal_rl's scaled policy (seed 11, mean weights x 0.02,
    mean bias 0.05) and inputs (rng 3) for these hidden widths, and the un-terminated
    ops.rollout_deep rollout every test here truncates; computed once and left unchanged."""
    from test_gpu_goal_rl import _scaled_policy

    pol = _scaled_policy(list(hidden))
    rng = np.random.default_rng(3)
    init = rng.uniform(-6, -4, (nt, 2)).astype(np.float32)
    noise = rng.standard_normal((Tn, nt, 2))
    for x in (init, noise):
        x.setflags(write=False)
    return (pol, init, noise, *_unterminated(pol, init, noise))


def _ff(shape, dtype):
    """A device buffer whose every byte is 0xff (NaN as f32, -1 as int32)."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _outputs(n, Tn):
    return (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, 2), torch.float32),
            _ff((n, Tn), torch.float32), _ff((n,), torch.int32), _ff((n,), torch.int32))


def _run_goal(pol, init, noise, goal, radius=0.1, env_id=1):
    from mepol_amd import ops

    Tn, n, _ = noise.shape
    out = _outputs(n, Tn)
    ops.rollout_deep_goal(_layers(pol), pol.mean.weight.detach(), pol.mean.bias.detach(),
                          pol.log_std.detach(), torch.tensor(init, device="cuda"),
                          torch.tensor(noise, dtype=torch.float64, device="cuda"), goal, radius,
                          *out, env_id=env_id)
    return [x.cpu().numpy() for x in out]


def _assert_cut(got, S, A, goal):
    """The goal kernel's outputs equal the un-terminated rollout cut at this goal, bit for bit,
    with positive zeros behind each episode.  Returns (lens, dones) of the cut."""
    lens, dones = C.first_hit(S, goal)
    St, At, Rt = C.truncate(S, A, lens, dones)
    s, a, r, ln, dn = got
    assert np.array_equal(ln, lens) and np.array_equal(dn, dones.astype(np.int32))
    assert np.array_equal(s, St) and np.array_equal(a, At) and np.array_equal(r, Rt)
    assert not np.signbit(s[St == 0]).any() and not np.signbit(a[At == 0]).any()
    assert not np.signbit(r[Rt == 0]).any()
    return lens, dones


# ---- 1. bit-exact against the truncated un-terminated rollout --------------------------------
@pytest.mark.parametrize("hidden", [(70, 9, 66), (64, 130, 6, 33, 10, 65)],
                         ids=["70-9-66", "six-layers"])
def test_deep_goal_bitexact_vs_truncated_rollout(cuda, hidden):
    """The restatement test's edge shapes (an empty fourth chunk, one-row tails, two- and
    three-wave workgroups), 20 trajectories of 60 steps, goals at steps 1, 30 and 60 of trajectory
    0; the outputs start as 0xff bytes, so every word is the call's.  Every ending occurs: len 1, a
    mid-episode hit, a hit on step T, T without a hit.  That is a condition on the inputs: with
    test_gpu_goal_rl's scaling and seeds unchanged, the oracle's un-terminated rollout
    (oracle.rollout) of both policies yields all four kinds on the CPU."""
    pol, init, noise, S, A = _case(hidden, NT, T)
    assert np.isfinite(A).all() and np.abs(np.diff(S, axis=1)).max() > 0  # the point moves
    kinds = set()
    for t_star in (1, 30, 60):
        goal = S[0, t_star]
        lens, dones = _assert_cut(_run_goal(pol, init, noise, goal), S, A, goal)
        for L, d in zip(lens.tolist(), dones.tolist()):
            kinds.add("len1" if L == 1 else "mid_done" if 1 < L < T and d else
                      "T_done" if L == T and d else "T_not_done" if L == T else "other")
    assert {"len1", "mid_done", "T_done", "T_not_done"} <= kinds, kinds


# ---- 2. against the exact restatement --------------------------------------------------------
def test_deep_goal_vs_restatement(cuda):
    """test_gpu_rollout_deep's plain-Python restatement of the summation order, cut at a goal
    taken from step 5 of trajectory 1."""
    from test_gpu_rollout_deep import _case as deep_case
    from test_gpu_rollout_deep import _restated_rollout

    nt, Tn = 3, 12
    pol, sd, init, noise = deep_case("gridworld", (70, 9, 66), nt, Tn)
    std = torch.exp(pol.log_std.detach()).cpu().numpy()  # as the device computes it
    S_ref, A_ref, _ = _restated_rollout("gridworld", sd, std, init, noise, Tn)
    goal = S_ref[1, 5]
    lens, dones = _assert_cut(_run_goal(pol, init, noise, goal), S_ref, A_ref, goal)
    assert dones[1] and 1 <= lens[1] <= 5


# ---- 3. wide shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(300, 300, 300), (512,) * 6], ids=["300x3", "512x6"])
def test_deep_goal_wide_shapes(cuda, hidden):
    """[512] x 6 holds 5 * 512^2 weight words behind layer 1, more than MEPOL's dispatch sends to
    the deep kernel (ROLLOUT_DEEP_MAX_WORDS): the entry point itself has no such cap."""
    from mepol_amd.algorithms import mepol as M

    if len(hidden) == 6:
        assert sum(a * b for a, b in zip(hidden, hidden[1:])) > M.ROLLOUT_DEEP_MAX_WORDS
    nt, Tn = 4, 30
    pol, init, noise, S, A = _case(hidden, nt, Tn)
    ended = set()
    for t_star in (1, 15, 30):
        goal = S[0, t_star]
        lens, dones = _assert_cut(_run_goal(pol, init, noise, goal), S, A, goal)
        ended.update(zip(lens.tolist(), dones.tolist()))
    assert (1, True) in ended and (Tn, False) in ended
    assert any(1 < L < Tn and d for L, d in ended)


# ---- 4. LDS residency does not change bits ---------------------------------------------------
def test_deep_goal_lds_rows_do_not_change_bits(cuda, monkeypatch):
    pol, init, noise, S, _ = _case((300, 300, 300), 4, 30)
    outs = []
    for kl in ("0", None):
        if kl is None:
            monkeypatch.delenv("MEPOL_ROLLOUT_KL", raising=False)
        else:
            monkeypatch.setenv("MEPOL_ROLLOUT_KL", kl)
        outs.append(_run_goal(pol, init, noise, S[0, 15]))
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()


# ---- 5. arguments ----------------------------------------------------------------------------
def test_deep_goal_arguments(cuda):
    from mepol_amd._lib import MepolError, call, ptr
    from mepol_amd.policy import GaussianPolicy

    hidden = (70, 9, 66)
    pol, init, noise, S, _ = _case(hidden, NT, T)
    goal = S[0, 30]
    with pytest.raises(MepolError, match="rc=1003"):
        _run_goal(pol, init, noise, goal, env_id=0)
    with pytest.raises(MepolError, match="rc=1001"):
        _run_goal(pol, init, noise, goal, radius=-1.0)
    with pytest.raises(MepolError, match="rc=1001"):
        _run_goal(pol, init, noise, (float("nan"), 0.0))
    torch.manual_seed(0)
    with pytest.raises(MepolError, match="rc=1001"):
        _run_goal(GaussianPolicy([8] * 7, 2, 2, -1.5).cuda(), init, noise, goal)

    # the entry point itself, with the caller's own workspace
    layers = _layers(pol)
    widths = (ctypes.c_int * 3)(*hidden)
    Wt = torch.cat([W.t().reshape(-1) for W, _ in layers[1:]])
    bt = torch.cat([b.reshape(-1) for _, b in layers[1:]])
    w = [t.detach().contiguous() for t in (layers[0][0], layers[0][1], Wt, bt, pol.mean.weight,
                                           pol.mean.bias, pol.log_std)]
    d_init = torch.tensor(init, device="cuda")
    d_noise = torch.tensor(noise, dtype=torch.float64, device="cuda")
    out = _outputs(NT, T)
    ws = _ff((256,), torch.uint8)
    gx, gy = (float(v) for v in goal)

    def entry(env_id=1, a_dim=2, n=NT, ws_bytes=256):
        call("mepol_rollout_deep_goal", env_id, 3, widths, *(ptr(t) for t in w), a_dim,
             ptr(d_init), ptr(d_noise), n, T, gx, gy, 0.1, *(ptr(x) for x in out), ptr(ws),
             ws_bytes, None)

    with pytest.raises(MepolError, match="rc=1003"):
        entry(env_id=0)
    with pytest.raises(MepolError, match="rc=1001"):
        entry(a_dim=1)
    with pytest.raises(MepolError, match="rc=1002"):
        entry(ws_bytes=255)  # a stale workspace, sized for something else
    entry(n=0)
    torch.cuda.synchronize()
    assert all(bool((x.view(torch.uint8) == 0xFF).all()) for x in (*out, ws))  # nothing ran


# ---- 6. plan ---------------------------------------------------------------------------------
def test_deep_goal_plan(cuda):
    from mepol_amd import ops
    from mepol_amd._lib import MepolError

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ops.rollout_deep_goal_plan((64, 64, 64))["resident_workgroups"] >= cus
    wide = ops.rollout_deep_goal_plan((512,) * 6)["resident_workgroups"]
    assert wide > 0 and wide % cus == 0
    with pytest.raises(MepolError, match="rc=1001"):
        ops.rollout_deep_goal_plan((64, 64))
