"""The rollout kernels and env steps case by case at their edges (rollout_cases.py): the env steps
on the reference's boundary fixtures, and mepol_rollout_mlp / _goal / _deep / _step against the
oracle's k-ordered rollout at the shapes where the K loops, the mail and the noise lookahead
change path.  GridWorld is compared bit for bit; MountainCar's step 0 actions bit for bit and the
rest to the 1e-12 the rollout tests use (cos() may differ from glibc in the last ulp); a single
MountainCar step to the 1e-15 of test_gpu_envs.py, and exactly where the result is a clamp's
constant.  Every output buffer starts as 0xff bytes, so an element the call left alone is NaN."""
import copy

import numpy as np
import pytest
import torch

import goal_rl_cases as G
import rollout_cases as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

FORMS = ["one-wg", "multi-wg"]


def _ff(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _dev(x, dtype=None):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- A: the env steps on the boundary fixtures -----------------------------------------------
def test_step_gridworld_on_the_boundary_rows(cuda):
    from mepol_amd import ops

    z = load_golden("env_gw_edges")
    s = _dev(z["S"])
    ops.step_gridworld(s, _dev(z["A"]))
    got = s.cpu().numpy()
    bad = [nm for nm, g, w in zip(z["name"], got, z["NS"]) if not _same(g, w)]
    assert not bad, bad


MC_CONSTANTS = (-1.2, 0.45, 0.07, -0.07, 0.0)


def _check_mc_step(got, z):
    NS = z["NS"]
    nan = np.isnan(NS)
    assert np.array_equal(np.isnan(got), nan), z["name"][np.isnan(got).any(1) != nan.any(1)]
    const = np.isin(NS, MC_CONSTANTS)
    assert const.sum() >= 20
    bad = [nm for nm, g, w, c in zip(z["name"], got, NS, const) if not (g[c] == w[c]).all()]
    assert not bad, bad
    rest = ~const & ~nan
    print("max |got - NS| off the constants:", np.abs(got[rest] - NS[rest]).max())
    np.testing.assert_allclose(got[rest], NS[rest], rtol=0, atol=1e-15)


def test_step_mountaincar_on_the_boundary_rows(cuda):
    from mepol_amd import ops

    z = load_golden("env_mc_edges")
    s = _dev(z["S"])
    ops.step_mountaincar(s, _dev(z["A"]))
    _check_mc_step(s.cpu().numpy(), z)


@pytest.mark.parametrize("env", R.ENVS)
def test_rollout_step_on_the_boundary_rows(cuda, env):
    """rollout_step_kernel over the same rows: mean 0, noise = A and log_std 0 make the action A."""
    from mepol_amd import ops

    mc = env == "mountaincar"
    z = load_golden("env_mc_edges" if mc else "env_gw_edges")
    n, a_dim = z["A"].shape
    st = _dev(z["S"])
    states, actions, pin = _ff((n, 2, 2), torch.float32), _ff((n, 1, a_dim), torch.float32), \
        _ff((n, 2), torch.float64)
    ops.rollout_step(0 if mc else 1, st if mc else None, None if mc else st,
                     torch.zeros((n, a_dim), dtype=torch.float64, device="cuda"), _dev(z["A"]),
                     torch.zeros(a_dim, dtype=torch.float64, device="cuda"), 0, 1, states, actions,
                     pin)
    got = st.cpu().numpy()
    with np.errstate(over="ignore"):
        assert _same(actions.cpu().numpy()[:, 0], z["A"].astype(np.float32))
    if mc:
        _check_mc_step(got, z)
    else:
        bad = [nm for nm, g, w in zip(z["name"], got, z["NS"]) if not _same(g, w)]
        assert not bad, bad
    assert _same(pin.cpu().numpy(), got.astype(np.float64))
    assert _same(states.cpu().numpy()[:, 1], got.astype(np.float32))
    assert (states.cpu().numpy()[:, 0].view(np.uint32) == 0xFFFFFFFF).all()  # row 0 is the caller's


# ---- C: the one-launch rollouts --------------------------------------------------------------
_GPU = {}


def _policy(case):
    """The case's policy on the GPU and exp(log_std) as the device computes it (it agrees with
    numpy's to an ulp)."""
    pol = R.case_policy(case)
    if id(pol) not in _GPU:
        dev = copy.deepcopy(pol).cuda()
        std = torch.exp(dev.log_std.detach()).cpu().numpy()
        np.testing.assert_allclose(std, np.exp(pol.log_std.detach().numpy()), rtol=2.3e-16, atol=0)
        _GPU[id(pol)] = (pol, dev, std)
    return _GPU[id(pol)][1:]


_ORACLE = {}


def _oracle(case, std, noise=None):
    """O.rollout_kordered once per (case, noise), shared and left unchanged."""
    key = (case["name"], case["hidden"], None if noise is None else noise.tobytes())
    if key not in _ORACLE:
        S, A = R.oracle(case, std=std, noise=noise)
        S.setflags(write=False)
        A.setflags(write=False)
        _ORACLE[key] = (S, A)
    return _ORACLE[key]


def _set_form(monkeypatch, case, form, a_dim=None, goal=False):
    """Select the form and assert, as the existing rollout tests do, which one the plan reports."""
    from mepol_amd import ops

    h0, h1 = case["hidden"]
    a_dim = case["a_dim"] if a_dim is None else a_dim
    monkeypatch.setenv("MEPOL_ROLLOUT_MW", "1" if form == "multi-wg" else "0")
    plan = (ops.rollout_goal_plan if goal else ops.rollout_mlp_plan)(case["n"], h0, h1, a_dim)
    assert plan["k_chunks"] == R.K_CHUNKS
    m = R.mw_model(h0, h1, a_dim)
    assert plan["workgroups_per_traj"] == (m["np"] if form == "multi-wg" and m["accepted"] else 1)
    return m


def _run_mlp(case, noise=None):
    """mepol_rollout_mlp through its C entry point (ops.rollout_mlp passes no final_state), all
    five outputs pre-filled with 0xff."""
    from mepol_amd import ops
    from mepol_amd._lib import call, ptr

    pol, _ = _policy(case)
    noise = case["noise"] if noise is None else noise
    Tn, n, a = noise.shape
    h0, h1 = case["hidden"]
    mc = case["env"] == "mountaincar"
    l1, l2 = pol.net[0], pol.net[2]
    w = [t.detach().contiguous() for t in (l1.weight, l1.bias, l2.weight.t(), l2.bias,
                                           pol.mean.weight, pol.mean.bias, pol.log_std)]
    init, nz = _dev(case["init"]), _dev(noise, torch.float64)
    out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32),
           _ff((n, Tn, 2), torch.float64), _ff((n, 2), torch.float64))
    ws = ops._ws_or_cached(None, init.device, "rollout", "rollout_mlp", n, Tn, h0, h1, a)
    call("mepol_rollout_mlp", 0 if mc else 1, ptr(w[0]), ptr(w[1]), h0, ptr(w[2]), ptr(w[3]), h1,
         ptr(w[4]), ptr(w[5]), ptr(w[6]), a, ptr(init if mc else None), ptr(None if mc else init),
         ptr(nz), n, Tn, *(ptr(x) for x in out), ptr(ws), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32)[0].item()) == 0  # no part gave up waiting
    return [x.cpu().numpy() for x in out]


def _check(case, got, ref):
    """States / actions against the oracle, visited and final_state against the states."""
    S, A, visited, final = got
    S_ref, A_ref = ref
    if case["env"] == "gridworld":
        assert np.array_equal(A, A_ref)
        assert np.array_equal(S, S_ref)
    else:
        assert np.array_equal(A[:, 0], A_ref[:, 0])  # first step: no cos() involved yet
        assert np.array_equal(S[:, 0], S_ref[:, 0])
        assert np.isfinite(A).all() and np.isfinite(S).all()
        np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(S, S_ref, rtol=0, atol=1e-12)
    assert np.array_equal(visited.astype(np.float32), S[:, 1:])
    assert np.array_equal(final.astype(np.float32), S[:, -1])
    assert np.array_equal(final, visited[:, -1])


def _forms_of(cases):
    return [pytest.param(c, f, id=f"{c['name']}-{f}") for c in cases for f in FORMS]


@pytest.mark.parametrize("case,form", _forms_of(R.shapes_cases()))
def test_shapes(cuda, monkeypatch, case, form):
    m = _set_form(monkeypatch, case, form)
    if form == "multi-wg" and not m["accepted"]:
        assert case["hidden"][0] > R.MW_MAX_H0  # refused: the one-workgroup form ran (again)
    _check(case, _run_mlp(case), _oracle(case, _policy(case)[1]))


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c in R.kl_cases()])
def test_kl_split(cuda, monkeypatch, case):
    """However many W2^T rows sit in LDS, the one-workgroup form gives the oracle's bits."""
    monkeypatch.setenv("MEPOL_ROLLOUT_KL", str(case["kl"]))
    _set_form(monkeypatch, case, "one-wg")
    _check(case, _run_mlp(case), _oracle(case, _policy(case)[1]))


@pytest.mark.parametrize("case,form", _forms_of(R.adim_cases()))
def test_action_widths(cuda, monkeypatch, case, form):
    """a_dim 1, 3 and 8 on MountainCar (only action 0 drives the env): every action column
    against the oracle; np * a_dim reaches 64 mail words at [64, 512] x 8."""
    m = _set_form(monkeypatch, case, form)
    assert m["accepted"]
    got = _run_mlp(case)
    ref = _oracle(case, _policy(case)[1])
    assert got[1].shape == (case["n"], case["T"], case["a_dim"])
    if case["T"] == 1:
        assert np.array_equal(got[1], ref[1])  # one step: every action is bit-exact
    _check(case, got, ref)


@pytest.mark.parametrize("case,form", _forms_of(R.short_cases()))
def test_short_rollouts(cuda, monkeypatch, case, form):
    """T = 1 and 2 (the noise lookahead's `t + 1 < T`) with one and three trajectories."""
    _set_form(monkeypatch, case, form)
    _check(case, _run_mlp(case), _oracle(case, _policy(case)[1]))


@pytest.mark.parametrize("case,form", _forms_of(R.env_edges_cases()))
def test_env_edges_in_the_fused_kernels(cuda, monkeypatch, case, form):
    _set_form(monkeypatch, case, form)
    _check(case, _run_mlp(case), _oracle(case, _policy(case)[1]))


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"])
                                  for c in R.env_edges_cases((70, 9, 66))])
def test_env_edges_in_the_deep_rollout(cuda, case):
    from mepol_amd import ops
    from test_gpu_rollout_deep import _layers, _restated_rollout

    pol, std = _policy(case)
    sd = R.state_dict(R.case_policy(case))
    S_ref, A_ref, V_ref = _restated_rollout(case["env"], sd, std, case["init"], case["noise"],
                                            case["T"])
    n, Tn, a = case["n"], case["T"], case["a_dim"]
    out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32),
           _ff((n, Tn, 2), torch.float64))
    ops.rollout_deep(0 if case["env"] == "mountaincar" else 1, _layers(pol),
                     pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
                     _dev(case["init"]), _dev(case["noise"], torch.float64), *out)
    S, A, V = (x.cpu().numpy() for x in out)
    if case["env"] == "gridworld":
        assert np.array_equal(A, A_ref) and np.array_equal(S, S_ref) and np.array_equal(V, V_ref)
    else:
        assert np.array_equal(A[:, 0], A_ref[:, 0]) and np.isfinite(S).all()
        np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(S, S_ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(V, V_ref, rtol=0, atol=1e-12)
    assert np.array_equal(V.astype(np.float32), S[:, 1:])


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c in R.env_edges_cases()])
def test_env_edges_in_the_per_step_loop(cuda, case):
    """rollout_step_kernel T times.  The mean comes from the host (the numpy MLP on the state the
    kernel handed back), so the comparison is of the kernel alone: the reference is the same loop
    with the numpy oracle's env step."""
    from mepol_amd import ops
    from oracle import mepol_oracle as O

    _, std = _policy(case)
    sd = R.state_dict(R.case_policy(case))
    mc = case["env"] == "mountaincar"
    n, Tn, a = case["n"], case["T"], case["a_dim"]
    env_state = _dev(case["init"])
    pin = _dev(case["init"], torch.float64)
    states, actions = _ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32)
    zero = torch.zeros(a, dtype=torch.float64, device="cuda")
    s = case["init"].copy()
    S_ref, A_ref = np.zeros((n, Tn + 1, 2), np.float32), np.zeros((n, Tn, a), np.float32)
    S_ref[:, 0] = s
    for t in range(Tn):
        x = pin.cpu().numpy()
        mean, scaled = O.mlp_mean(sd, x), case["noise"][t] * std
        ops.rollout_step(0 if mc else 1, env_state if mc else None, None if mc else env_state,
                         _dev(mean), _dev(scaled), zero, t, Tn, states, actions, pin)
        act = O.mlp_mean(sd, s.astype(np.float64)) + scaled
        A_ref[:, t] = act
        s = O.mountaincar_step(s, act) if mc else O.gridworld_step(s, act)
        S_ref[:, t + 1] = s
    S, A = states.cpu().numpy(), actions.cpu().numpy()
    if mc:
        assert np.array_equal(A[:, 0], A_ref[:, 0])
        np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(S[:, 1:], S_ref[:, 1:], rtol=0, atol=1e-12)
    else:
        assert np.array_equal(A, A_ref) and np.array_equal(S[:, 1:], S_ref[:, 1:])


# ---- a NaN action ----------------------------------------------------------------------------
def _check_nan(case, clean, dirty):
    S0, A0 = clean[:2]
    S1, A1 = dirty[:2]
    i, t = R.NAN_TRAJ, R.NAN_STEP
    others = [k for k in range(case["n"]) if k != i]
    assert np.array_equal(S1[others], S0[others]) and np.array_equal(A1[others], A0[others])
    assert np.array_equal(S1[i, :t + 1], S0[i, :t + 1]) and np.array_equal(A1[i, :t], A0[i, :t])
    assert np.isnan(A1[i, t, 0])
    for c in (0, 1):
        if c in case["nan_coords"]:
            assert np.isnan(S1[i, t + 1:, c]).all()  # NaN at step 5 and to the end
        else:
            assert np.isfinite(S1[i, :, c]).all()


@pytest.mark.parametrize("case,form", _forms_of(R.nan_cases()))
def test_nan_action_in_rollout_mlp(cuda, monkeypatch, case, form):
    """One NaN noise value: the reference's clip keeps it, the state turns NaN where the fixture's
    does and stays so (the k-NN then refuses the batch, as sklearn does in the reference); the
    other trajectories do not notice.  Nothing is asserted about the trajectory's later actions."""
    _set_form(monkeypatch, case, form)
    clean = _run_mlp(case)
    _check(case, clean, _oracle(case, _policy(case)[1]))
    dirty = _run_mlp(case, noise=case["noise_nan"])
    _check_nan(case, clean, dirty)
    S, _, visited, final = dirty
    assert _same(visited.astype(np.float32), S[:, 1:]) and _same(final.astype(np.float32), S[:, -1])


def _run_goal(case, noise, goal, radius):
    from mepol_amd import ops

    pol, _ = _policy(case)
    Tn, n, a = noise.shape
    out = (_ff((n, Tn + 1, 2), torch.float32), _ff((n, Tn, a), torch.float32),
           _ff((n, Tn), torch.float32), _ff((n,), torch.int32), _ff((n,), torch.int32))
    l1, l2 = pol.net[0], pol.net[2]
    ops.rollout_goal(l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach(),
                     pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(),
                     _dev(case["init"]), _dev(noise, torch.float64), goal, radius, *out)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("form", FORMS)
def test_nan_action_in_rollout_goal(cuda, monkeypatch, form):
    """A NaN state is never a hit: the episode runs to T with done = 0."""
    (case,) = [c for c in R.nan_cases() if c["env"] == "gridworld"]
    _set_form(monkeypatch, case, form, goal=True)
    goal = np.array([0.0, 0.0], np.float32)  # inside the central wall: out of reach
    clean = _run_goal(case, case["noise"], goal, 0.1)
    S_ref, A_ref = _oracle(case, _policy(case)[1])
    assert np.array_equal(clean[0], S_ref) and np.array_equal(clean[1], A_ref)
    dirty = _run_goal(case, case["noise_nan"], goal, 0.1)
    _check_nan(case, clean, dirty)
    for out in (clean, dirty):
        assert (out[2] == 0).all() and (out[3] == case["T"]).all() and (out[4] == 0).all()


# ---- goal mode on the radius -----------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c in R.goal_cases()])
def test_goal_radius_is_closed(cuda, monkeypatch, case, form):
    """goal_hit's `<=`: a radius equal to the f32 distance hits, the f64 below it does not, and
    radius 0 hits the goal state itself; against goal_rl_cases.first_hit / truncate."""
    _set_form(monkeypatch, case, form, goal=True)
    S, A = _oracle(case, _policy(case)[1])
    for label, goal, radius, ends in R.goal_settings(S):
        lens, dones = G.first_hit(S, goal, radius)
        assert (int(lens[0]) == R.GOAL_T and bool(dones[0])) == ends, label
        St, At, Rt = G.truncate(S, A, lens, dones)
        s, a, r, ln, dn = _run_goal(case, case["noise"], goal, radius)
        assert np.array_equal(ln, lens) and np.array_equal(dn, dones.astype(np.int32)), label
        assert np.array_equal(s, St) and np.array_equal(a, At) and np.array_equal(r, Rt), label
