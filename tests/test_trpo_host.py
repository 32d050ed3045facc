"""TRPO policy step, host side (no GPU): the closed form of the Fisher-vector product against the
reference's double backward, PolicyFisher's fallback, conj_gradient, backtracking and
assign_flat_params.  The reference is tests/trpo_reference.py (torch f64 on the CPU)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import trpo_reference as R

TOL = 1e-12  # per tensor, max |diff| <= TOL * max |ref| (measured: <= 1e-15)
SHAPES = [(2, [300, 300], 2, 517), (29, [400, 300], 8, 700), (5, [34, 18, 22], 3, 501)]


def _states(n, nf, seed):
    return torch.randn(n, nf, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _policy(hidden, nf, a, ref, activation=nn.ReLU):
    from mepol_amd.policy import GaussianPolicy

    p = GaussianPolicy(hidden, nf, a, activation=activation)
    ref.load_into(p)
    return p


def test_parameter_order_is_the_reference_layout():
    from mepol_amd.policy import GaussianPolicy

    names = [n for n, _ in GaussianPolicy([6, 4], 3, 2).named_parameters()]
    assert names == ["log_std", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias",
                     "mean.weight", "mean.bias"]


@pytest.mark.parametrize("nf,hidden,a,n", SHAPES)
def test_closed_form_matches_double_backward(nf, hidden, a, n):
    ref = R.RefPolicy.random(nf, hidden, a, seed=1)
    x = _states(n, nf, 2)
    v = torch.randn(ref.flat().numel(), generator=torch.Generator().manual_seed(3),
                    dtype=torch.float64)
    want = R.make_hvp(ref, x, 0.1)(v)
    got = R.closed_form_hvp(ref, x, v, 0.1)
    err = R.per_tensor_rel(ref.params(), got, want)
    print(f"closed form vs double backward {nf}->{hidden}->{a}, n={n}: {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("nf,hidden,a,n,activation,act", [
    (2, [64, 48], 2, 203, nn.ReLU, torch.relu),
    (3, [20, 12], 2, 150, nn.Tanh, torch.tanh),
    (5, [33, 17], 3, 131, nn.ReLU, torch.relu),
    (4, [24], 2, 97, nn.ReLU, torch.relu),
])
def test_fallback_hvp_matches_reference(nf, hidden, a, n, activation, act):
    from mepol_amd.algorithms import trpo

    ref = R.RefPolicy.random(nf, hidden, a, seed=4, act=act)
    policy = _policy(hidden, nf, a, ref, activation)
    x = _states(n, nf, 5)
    fisher = trpo.PolicyFisher(policy, x, 0.1)
    assert not fisher.kernels
    v = torch.randn(fisher.numel, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    want = R.make_hvp(ref, x, 0.1)(v)
    got = fisher.hvp(v)
    err = R.per_tensor_rel(ref.params(), got, want)
    print(f"fallback hvp {activation.__name__} {hidden}: {err:.2e}")
    assert err <= TOL
    assert all(p.grad is None for p in policy.parameters())


def test_conj_gradient_solves_spd_system():
    from mepol_amd.algorithms import trpo

    rng = np.random.default_rng(0)
    M = rng.standard_normal((40, 40))
    A = M @ M.T + 40 * np.eye(40)
    b = rng.standard_normal(40)
    At, bt = torch.as_tensor(A), torch.as_tensor(b)
    x = trpo.conj_gradient(lambda p: At @ p, bt, 40)
    want = np.linalg.solve(A, b)
    assert np.abs(x.numpy() - want).max() <= 1e-10 * np.abs(want).max()
    x1 = trpo.conj_gradient(lambda p: At @ p, bt, 1)
    torch.testing.assert_close(x1, bt * (bt @ bt) / (bt @ (At @ bt)), rtol=1e-15, atol=0)
    # the same iterates as the reference's loop
    torch.testing.assert_close(trpo.conj_gradient(lambda p: At @ p, bt, 10),
                               R.conj_gradient(lambda p: At @ p, bt, 10), rtol=1e-13, atol=0)


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(3, dtype=torch.float64))
        self.b = nn.Parameter(torch.ones(2, 2, dtype=torch.float64))

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.parameters()])


def _scripted(values):
    it = iter(values)
    return lambda: next(it)


def test_backtracking_accepts_first_valid_trial():
    from mepol_amd.algorithms import trpo

    m = _Model()
    old = m.flat()
    d = torch.arange(7, dtype=torch.float64)
    # trial 0: no improvement; trial 1: improves, constraint over; trial 2: valid
    obj = _scripted([1.0, 0.5, 2.0, torch.tensor(1.5)])
    con = _scripted([0.0, 0.5, torch.tensor(0.05)])
    ok, new, i = trpo.backtracking(m, obj, con, 0.1, d, 2.0)
    assert ok is True and i == 2
    torch.testing.assert_close(new, old + 0.25 * 2.0 * d, rtol=0, atol=0)
    assert torch.equal(m.flat(), new)


def test_backtracking_restores_parameters_when_exhausted():
    from mepol_amd.algorithms import trpo

    m = _Model()
    old = m.flat()
    d = torch.ones(7, dtype=torch.float64)
    ok, params, i = trpo.backtracking(m, lambda: 1.0, lambda: 0.0, 0.1, d, 1.0, max_iters=10)
    assert (ok, i) == (False, 9)
    assert torch.equal(params, old) and torch.equal(m.flat(), old)


def test_backtracking_just_check_constraint_and_nan():
    from mepol_amd.algorithms import trpo

    d = torch.ones(7, dtype=torch.float64)
    # no improvement, but only the constraint is asked for
    ok, _, i = trpo.backtracking(_Model(), lambda: 1.0, lambda: 0.05, 0.1, d, 1.0,
                                 just_check_constraint=True)
    assert ok and i == 0
    # NaN objective rejects trial 0, NaN constraint rejects trial 1, trial 2 is valid
    obj = _scripted([1.0, float("nan"), 2.0, 2.0])
    con = _scripted([0.0, float("nan"), 0.0])
    ok, _, i = trpo.backtracking(_Model(), obj, con, 0.1, d, 1.0)
    assert ok and i == 2
    # a NaN constraint rejects under just_check_constraint as well
    ok, _, i = trpo.backtracking(_Model(), lambda: 1.0, lambda: float("nan"), 0.1, d, 1.0,
                                 max_iters=3, just_check_constraint=True)
    assert (ok, i) == (False, 2)


def test_assign_flat_params_round_trips():
    from mepol_amd.algorithms import trpo
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(0)
    p = GaussianPolicy([6, 5], 3, 2)
    flat = torch.cat([t.detach().reshape(-1) for t in p.parameters()])
    new = torch.randn_like(flat)
    trpo.assign_flat_params(p, new)
    assert torch.equal(torch.cat([t.detach().reshape(-1) for t in p.parameters()]), new)
    trpo.assign_flat_params(p, flat)
    assert torch.equal(torch.cat([t.detach().reshape(-1) for t in p.parameters()]), flat)
    with pytest.raises(ValueError):
        trpo.assign_flat_params(p, flat[:-1].clone())


def test_trpo_step_on_the_cpu_matches_reference():
    """The whole step on the fallback path: the same decision and parameters as the reference."""
    from mepol_amd.algorithms import trpo

    nf, hidden, a, n = 2, [16, 12], 2, 120
    ref = R.RefPolicy.random(nf, hidden, a, seed=7)
    policy = _policy(hidden, nf, a, ref)
    x = _states(n, nf, 8)
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(n, a, generator=g, dtype=torch.float64)
    actions = (ref.mean(x) + noise * torch.exp(ref.log_std)).detach()
    adv = noise[:, 0] + 0.5 * noise[:, 1] ** 2
    ok_ref, it_ref, _, _ = R.trpo_step(ref, x, actions, adv, 0.01)
    ok, it = trpo.trpo_step(policy, x, actions, adv, 0.01)
    assert (ok, it) == (ok_ref, it_ref)
    got = torch.cat([t.detach().reshape(-1) for t in policy.parameters()])
    # on the CPU the fallback runs the reference's own torch operations: measured 0.0
    assert R.per_tensor_rel(ref.params(), got, ref.flat()) <= TOL
