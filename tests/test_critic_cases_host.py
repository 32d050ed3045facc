"""CPU checks of the critic fit's yardstick and host side: the numpy stand-in of critic_cases.py
against a torch autograd loop, that the stand-in with one planted mistake is caught at the GPU
test's tolerance, the mini-batch indices against the DataLoader they replace, and the gate."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import critic_cases as C

# The stand-in and torch differ in summation order and in where a product is rounded, a few ulp
# per step on values of order 1 (measured: 6e-16 over 40 steps); 1e-13 leaves two decimal orders
# and is a tenth of the GPU tolerance.
TORCH_ATOL = 1e-13


def _torch_fit(case):
    """The case's steps through nn.Sequential, autograd and torch.optim.Adam, in f64 on the CPU."""
    nf, h0, h1, B = case["nf"], case["h0"], case["h1"], case["B"]
    net = nn.Sequential(nn.Linear(nf, h0), nn.ReLU(), nn.Linear(h0, h1), nn.ReLU(),
                        nn.Linear(h1, 1)).double()
    params = list(net.parameters())
    with torch.no_grad():
        for p, a in zip(params, case["params"]):
            p.copy_(torch.from_numpy(a.copy()))
    opt = torch.optim.Adam(params, lr=C.LR)
    if case["first_step"] > 1 or any(a.any() for a in case["m"] + case["v"]):
        for p, m, v in zip(params, case["m"], case["v"]):
            opt.state[p] = {"step": torch.tensor(float(case["first_step"] - 1)),
                            "exp_avg": torch.from_numpy(m.copy()),
                            "exp_avg_sq": torch.from_numpy(v.copy())}
    states, targets = torch.from_numpy(case["states"].copy()), torch.from_numpy(
        case["targets"].copy()).unsqueeze(1)
    index = torch.from_numpy(case["index"].astype(np.int64))
    loss_out = []
    for s in range(index.numel() // B):
        rows = index[s * B:(s + 1) * B]
        opt.zero_grad()
        loss = torch.mean((net(states[rows]) - targets[rows]) ** 2)
        loss.backward()
        opt.step()
        loss_out.append(float(loss.detach()))
    return {"params": [p.detach().numpy() for p in params],
            "m": [opt.state[p]["exp_avg"].numpy() for p in params],
            "v": [opt.state[p]["exp_avg_sq"].numpy() for p in params],
            "loss": np.array(loss_out)}


@pytest.mark.parametrize("name", C.NAMES)
def test_stand_in_agrees_with_torch_autograd(name):
    dev, rel = C.max_deviation(_torch_fit(C.case(name)), C.reference(name))
    print(f"{name}: stand-in vs torch: max abs {dev:.3e}, loss rel {rel:.3e}")
    assert dev <= TORCH_ATOL and rel <= TORCH_ATOL


def test_nan_target_in_an_unread_row_changes_nothing():
    a, b = C.reference("ragged"), C.reference("ragged_nan")
    assert np.isnan(C.case("ragged_nan")["targets"][C.RAGGED_NAN_ROW])
    assert C.RAGGED_NAN_ROW not in C.case("ragged_nan")["index"]
    assert C.case("ragged")["index"].size == 2 * 4 * 5
    for k in ("params", "m", "v"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
    assert np.array_equal(a["loss"], b["loss"])


def test_dead_units_stay_exactly_where_they_were():
    case, ref = C.case("dead_unit"), C.reference("dead_unit")
    assert np.array_equal(C.dead_elements(ref, "params"), C.dead_elements(case, "params"))
    assert not C.dead_elements(ref, "m").any() and not C.dead_elements(ref, "v").any()
    # and the other units did move
    assert C.max_deviation({**ref, "loss": ref["loss"]},
                           {**case, "loss": ref["loss"]})[0] > 1e-3


# the case on which each planted mistake shows
MISTAKE_CASE = {"mask_ge": "dead_unit", "dv_no_mean": "full_1step", "stale_w2": "full_2step",
                "bc2_wrong_step": "full_2step"}


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_one_mistake_is_caught_at_the_gpu_tolerance(mistake):
    name = MISTAKE_CASE[mistake]
    dev, rel = C.max_deviation(C.fit_reference(C.case(name), mistake=mistake), C.reference(name))
    print(f"{mistake} on {name}: max abs {dev:.3e}, loss rel {rel:.3e}")
    # not merely above the tolerance: orders above it, so the check cannot pass by a hair
    assert dev > 1e3 * C.GPU_ATOL


def _loader_batches(n, batch, passes):
    ds = torch.utils.data.TensorDataset(torch.arange(n))
    dl = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True)
    out = []
    for _ in range(passes):
        for (rows,) in dl:
            out.append(rows)
    return torch.cat(out)


def test_index_reproduces_the_dataloader_and_its_generator_draws():
    from mepol_amd.algorithms.trpo import critic_fit_index

    n, batch, passes = 341, 48, 3
    torch.manual_seed(1234)
    want = _loader_batches(n, batch, passes)
    state_want = torch.get_rng_state()
    torch.manual_seed(1234)
    got = critic_fit_index(n, passes, batch)
    state_got = torch.get_rng_state()
    assert got.dtype == torch.int32 and got.numel() == passes * (n // batch) * batch
    assert torch.equal(got.to(torch.int64), want)
    assert torch.equal(state_got, state_want)


def _critic(layers=None):
    torch.manual_seed(0)
    layers = layers or [nn.Linear(2, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(),
                        nn.Linear(64, 1)]
    return nn.Sequential(*layers).double()


def _reason(vfunc, opt, states=None, batch=64):
    from mepol_amd import kernel_path

    states = torch.zeros(128, 2, dtype=torch.float64) if states is None else states
    reason, params = kernel_path.critic_fit_refusal(vfunc, opt, states, batch)
    assert (reason is None) == (params is not None)
    assert kernel_path.critic_fit_ok(vfunc, opt, states, batch) is params
    return reason


def test_gate_refuses_what_the_kernel_does_not_fit(monkeypatch):
    """Each refusal for its own reason.  Without a GPU the accepted critic is refused last, for
    its device alone, so a reason other than the device's shows the check that fired."""
    monkeypatch.delenv("MEPOL_CRITIC_FIT", raising=False)
    good = _critic()
    adam = torch.optim.Adam(good.parameters(), lr=1e-2)
    assert "GPU" in _reason(good, adam)  # a CPU critic: everything else about it is accepted

    tanh = _critic([nn.Linear(2, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)])
    assert "layer types" in _reason(tanh, torch.optim.Adam(tanh.parameters(), lr=1e-2))
    deep = _critic([nn.Linear(2, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64),
                    nn.ReLU(), nn.Linear(64, 1)])
    assert "layer count" in _reason(deep, torch.optim.Adam(deep.parameters(), lr=1e-2))
    wide = _critic([nn.Linear(2, 65), nn.ReLU(), nn.Linear(65, 64), nn.ReLU(), nn.Linear(64, 1)])
    assert "limits" in _reason(wide, torch.optim.Adam(wide.parameters(), lr=1e-2))
    assert "limits" in _reason(good, adam, batch=65)
    f32 = _critic().float()
    assert "float64" in _reason(f32, torch.optim.Adam(f32.parameters(), lr=1e-2),
                                states=torch.zeros(128, 2))
    assert "weight decay" in _reason(good, torch.optim.Adam(good.parameters(), lr=1e-2,
                                                            weight_decay=1e-3))
    assert "amsgrad" in _reason(good, torch.optim.Adam(good.parameters(), lr=1e-2, amsgrad=True))
    assert "Adam" in _reason(good, torch.optim.LBFGS(good.parameters(), lr=1e-2, max_iter=25))
    assert "exactly" in _reason(good, torch.optim.Adam(list(good.parameters())[:4], lr=1e-2))
    monkeypatch.setenv("MEPOL_CRITIC_FIT", "host")
    assert _reason(good, adam) == "MEPOL_CRITIC_FIT=host"


def test_host_loop_runs_when_the_gate_refuses(monkeypatch):
    """A CPU critic takes the reference's loop, as before: _fit_critic says so and never reaches
    ops.critic_fit."""
    from mepol_amd import ops
    from mepol_amd.algorithms import trpo as TR

    def boom(*a, **k):
        raise AssertionError("ops.critic_fit must not be called for a CPU critic")

    monkeypatch.setattr(ops, "critic_fit", boom)
    vfunc = _critic()
    opt = torch.optim.Adam(vfunc.parameters(), lr=1e-2)
    before = [p.detach().clone() for p in vfunc.parameters()]
    torch.manual_seed(3)
    st, tg = torch.rand(130, 2, dtype=torch.float64), torch.randn(130, 1, dtype=torch.float64)
    TR._fit_critic(vfunc, opt, "adam", st, tg, 1e-3, 2, 64)
    assert TR.CRITIC_FIT_STATS["path"] == "host"
    assert float(opt.state[next(vfunc.parameters())]["step"]) == 4.0
    assert any(not torch.equal(a, b) for a, b in zip(before, vfunc.parameters()))


def test_adam_step_scalars_are_torchs():
    from mepol_amd import ops

    got = ops.adam_step_scalars(C.LR, C.BETAS, 11, 3)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 2)
    assert got.tolist() == [list(x) for x in C.adam_scalars(11, 3)]
