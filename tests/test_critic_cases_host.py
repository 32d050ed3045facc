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


# ---------------------------------------------------------------------------------------------
# The op-level cases (second half of critic_cases.py): the GPU test's runner on the CPU
# ---------------------------------------------------------------------------------------------
def test_op_level_bounds_hold_for_an_honest_f64_implementation():
    """Every case of tests/test_gpu_critic_ops.py through cpu_ops.critic_fit (plain f64 numpy in
    its own summation order) and through the long-double stand-in: no bound is too tight for an
    honest implementation.  Prints the largest error / bound per output."""
    import cpu_ops

    for label, ops in (("cpu_ops", cpu_ops), ("stand-in", C.stand_in_ops())):
        for k in [k for k in C.RATIOS if k.startswith("critic_fit.")]:
            del C.RATIOS[k]
        C.run_all(ops, "cpu")
        ratios = {k: v for k, v in C.RATIOS.items() if k.startswith("critic_fit.")}
        assert len(ratios) >= 20 and max(ratios.values()) <= 1.0
        for k in sorted(ratios):
            print(f"{label}: {k:40s} {ratios[k]:.3f}")
        for name in C.CHAIN_NAMES:
            d, rel, atol, rtol = C.CHAIN_DEVIATIONS[name]
            print(f"{label}: {name}: spread {C.chain_spread(name)[0]:.3e} / "
                  f"{C.chain_spread(name)[1]:.3e}, deviation {d:.3e} / {rel:.3e}")


def test_chain_spreads_are_measured_not_assumed():
    """The recorded spreads between the two references are what this machine measures (not
    grown), and 100 x each stays far inside the old 1e-12."""
    assert set(C.CHAIN_SPREADS) == set(C.CHAIN_NAMES)
    for name in C.CHAIN_NAMES:
        dev, rel = C.chain_spread(name)
        rec = C.CHAIN_SPREADS[name]
        print(f"{name}: stand-in vs torch: max abs {dev:.3e}, loss rel {rel:.3e}")
        # torch's CPU products may sum in another order on another processor: a factor of 4
        assert dev <= 4 * rec[0] and rel <= 4 * rec[1], (name, dev, rel)
        assert 0 < rec[0] < 1e-14 and 0 < rec[1] < 1e-14
        atol, rtol = C.chain_tolerance(name)
        assert atol == C.SPREAD_FACTOR * rec[0] and rtol == C.SPREAD_FACTOR * rec[1]


# Where each planted mistake must show: (runner, its arguments).  "step" is a one-step case,
# the others are the multi-step families by name.
_STEP = lambda shape, variant: ("step", shape, variant)
MORE_MISTAKE_CASES = {
    "mean_64": [_STEP((2, 64, 64, 63), "s0"), _STEP((2, 64, 64, 1), "g")],
    "rows_ge_48": [_STEP((2, 64, 64, 49), "g"), _STEP((2, 64, 64, 63), "s0")],
    "db1_wave": [_STEP((2, 64, 64, 17), "g")],
    "db2_wave": [_STEP((2, 64, 64, 17), "g")],
    "dW3_wave": [_STEP((2, 64, 64, 17), "g")],
    "db3_wave": [_STEP((2, 64, 64, 17), "g")],
    "next_rows": [("prefetch", "split_ragged"), ("chain", "chain8_nf5_h7x50_B9")],
    "step_size_wrong_step": [_STEP((5, 7, 50, 9), "s0"), ("chain", "chain8_nf5_h50x7_B9")],
    "betas_default": [_STEP((5, 7, 50, 9), "s1")],
    "eps_default": [_STEP((5, 7, 50, 9), "s2"), _STEP((5, 7, 50, 9), "s1")],
    "w2_transposed": [_STEP((5, 7, 50, 9), "s0"), _STEP((5, 50, 7, 9), "g")],
    "w1_last_col_moments": [_STEP((1, 1, 1, 1), "s0"), _STEP((16, 16, 64, 64), "s0")],
    "kdrop_z1": [_STEP((5, 7, 50, 9), "g"), _STEP((2, 64, 64, 64), "s0")],
    "kdrop_z2": [_STEP((5, 7, 50, 9), "g"), _STEP((2, 63, 64, 64), "s0")],
    "kdrop_dW2": [_STEP((5, 7, 50, 9), "g"), _STEP((2, 64, 64, 63), "s0")],
    "kdrop_dh1": [_STEP((5, 50, 7, 9), "g"), _STEP((2, 64, 63, 64), "s0")],
    "kdrop_dW1": [_STEP((5, 7, 50, 9), "g"), _STEP((2, 64, 64, 1), "s0")],
    "index_clamp": [_STEP((2, 64, 64, 3), "s0"), _STEP((2, 64, 64, 64), "g")],
    "dz1_mask_z2": [_STEP((2, 64, 64, 16), "g"), _STEP((2, 64, 64, 64), "s0")],
}
# the four mistakes of the multi-step tests must show on the op-level cases too
MORE_MISTAKE_CASES.update({
    "mask_ge": [("exact",)],
    "dv_no_mean": [_STEP((2, 64, 64, 3), "g")],
    "stale_w2": [("split", "split_ragged"), ("chain", "chain8_nf3_h24x40_B5")],
    "bc2_wrong_step": [_STEP((2, 64, 64, 3), "s1")],
})


def _run_one(ops, what):
    kind, args = what[0], what[1:]
    if kind == "step":
        return C.run_one_step(ops, "cpu", *args)
    if kind == "exact":
        return C.run_exact(ops, "cpu")
    return {"prefetch": C.run_prefetch, "chain": C.run_chain, "split": C.run_split}[kind](
        ops, "cpu", *args)


@pytest.mark.parametrize("mistake", sorted(MORE_MISTAKE_CASES))
def test_planted_mistake_fails_its_op_level_cases(mistake):
    """The stand-in with ONE wrong step through the GPU test's runner: every listed case must
    fail (and passes without the mistake: the test above).  On a chain the deviation exceeds the
    tolerance 1000-fold, not by a hair."""
    assert mistake in C.MISTAKES + C.MORE_MISTAKES
    ops = C.stand_in_ops(mistake)
    for what in MORE_MISTAKE_CASES[mistake]:
        assert what[0] != "step" or what[1] in C.SHAPES
        honest = dict(C.RATIOS)   # the mistake's error / bound must not stay in the record
        try:
            with pytest.raises(AssertionError):
                _run_one(ops, what)
        finally:
            C.RATIOS.clear()
            C.RATIOS.update(honest)
        if what[0] == "chain":
            d, rel, atol, rtol = C.CHAIN_DEVIATIONS[what[1]]
            print(f"{mistake} on {what[1]}: {d:.3e} vs {atol:.3e}, loss {rel:.3e} vs {rtol:.3e}")
            assert d >= 1e3 * atol or rel >= 1e3 * rtol
    assert set(MORE_MISTAKE_CASES) == set(C.MISTAKES + C.MORE_MISTAKES)


def test_one_step_cases_cover_the_launch_arithmetic():
    """The shapes the issue names are there, and between them they reach every value of the
    kernel's selection lines (critic_cases.plan)."""
    S = set(C.SHAPES)
    want = ({(1, 1, 1, 1), (5, 7, 50, 9), (5, 50, 7, 9)}
            | {(2, 64, 64, B) for B in (1, 3, 15, 16, 17, 33, 47, 48, 49, 63)}
            | {(2, h, 64, 64) for h in (1, 3, 17, 33, 47, 49, 63)}
            | {(2, 64, h, 64) for h in (1, 3, 17, 33, 47, 49, 63)}
            | {(nf, 16, 64, 64) for nf in (3, 4, 5, 8, 9, 12, 13, 15, 16)})
    assert want <= S and len(S) == len(C.SHAPES)
    assert all(1 <= nf <= 16 and max(h0, h1, B) <= 64 for nf, h0, h1, B in S)
    plans = [C.plan(*s) for s in C.SHAPES]
    for key in ("nfB", "nfH0", "nfH1", "ksF", "slots"):
        assert {p[key] for p in plans} == {1, 2, 3, 4}, key
    for i in range(4):
        assert {s[i] % 4 for s in S} == {0, 1, 2, 3}, i
    for a, b in (("nfB", "nfH0"), ("nfB", "nfH1"), ("nfH0", "nfH1")):
        assert any(p[a] < p[b] for p in plans) and any(p[a] > p[b] for p in plans), (a, b)
    for a, b in (("dW2", "forward"), ("dW1", "dW2")):   # a wave in one phase and not the other
        assert any(p[a] - p[b] for p in plans) and any(p[b] - p[a] for p in plans), (a, b)
    assert {p["ksB"] for p in plans} >= {1, 4, 5, 12, 13, 16}
    # the vector owners: a width of 1, a ragged one and the full 64 lanes, for h0 and for h1
    for i in (1, 2):
        assert {1, 64} <= {s[i] for s in S} and any(s[i] % 16 for s in S)
    # the index of every case: 0, N - 1 and a duplicate as far as B entries can hold them
    for s in C.SHAPES:
        c = C.one_step_case(s, "s0")
        idx, B, N = c["index"], c["B"], c["N"]
        assert idx.size == B and (N - 1 in idx) and (B == 1 or 0 in idx)
        assert B < 3 or len(set(idx.tolist())) < B
        assert all(np.any(a) for a in c["m"] + c["v"]) and c["first_step"] > 1
        g = C.one_step_case(s, "g")
        assert not any(np.any(a) for a in g["m"] + g["v"]) and g["first_step"] == 1
    assert any(C.one_step_case(s, "s0")["N"] == 1 and s[3] > 1 for s in C.SHAPES)
    assert [C.one_step_case(C.SHAPES[0], v_).get("eps", C.EPS) for v_ in C.VARIANTS] == [
        1e-8, 1e-6, 0.0, 1e-8]
    assert C.one_step_case(C.SHAPES[0], "s1")["betas"] == (0.8, 0.99)
    assert C.one_step_case(C.SHAPES[0], "s2")["lr"] != C.LR


def test_multi_step_cases_are_what_they_claim():
    for name, n in (("split_ragged", 5), ("split_full", 4)):
        c = C.steps_case(name)
        B = c["B"]
        assert c["index"].size == n * B
        batches = [tuple(c["index"][s * B:(s + 1) * B]) for s in range(n)]
        assert len(set(batches)) == n          # a different batch in every step
    assert C.steps_case("split_ragged")["B"] % 16 and C.steps_case("split_full")["B"] == 64
    a, b = C.steps_case("unread_clean"), C.steps_case("unread_nonfinite")
    assert C.UNREAD_ROW not in a["index"] and np.array_equal(a["index"], b["index"])
    assert not np.isfinite(b["states"][C.UNREAD_ROW]).any() and np.isfinite(a["states"]).all()
    for name, (kind, value) in C.NONFINITE.items():
        c = C.steps_case(name)
        B = c["B"]
        assert c["index"].size == 3 * B
        arr = c["states"] if kind == "state" else c["targets"]
        bad = np.argwhere(~np.isfinite(arr))
        assert len(bad) == 1 and 0 <= bad[0][0] < c["N"]
        assert list(np.where(c["index"] == bad[0][0])[0]) == [B + C.NONFINITE_AT]
    for name in C.CHAIN_NAMES:
        c = C.steps_case(name)
        assert c["index"].size // c["B"] in (8, 40) and c["B"] % 16


@pytest.mark.parametrize("name", list(C.NONFINITE))
def test_non_finite_row_that_is_read(name):
    """What the select-ReLU restatement returns is the pinned pattern; torch's loop reports a
    non-finite loss from that step on and returns every tensor NaN.  For a non-finite STATE the
    two differ in what a caller can see: the restatement's (the kernel's) losses stay finite."""
    c = C.steps_case(name)
    assert C.finite_pattern(C.steps_reference(name)) == C.NONFINITE_PIN[name]
    assert C.finite_pattern(C.torch_fit(c)) == C.TORCH_PIN
    if C.NONFINITE[name][0] == "state":
        assert all(C.NONFINITE_PIN[name]["loss"])
        assert C.NONFINITE_PIN[name]["params.W1"] == ("cols", C.NONFINITE_F)
        assert "params.b3" not in C.NONFINITE_PIN[name]


def test_driver_spreads_a_non_finite_result_and_leaves_a_finite_one_alone():
    """_fit_critic's kernel path multiplies every tensor by 1.0 or by NaN on the device: the
    restatement's NaN-state result (finite losses, one NaN column) comes out all NaN, as the host
    loop's does; a finite result keeps its bits, -0.0 and denormals included."""
    from mepol_amd.algorithms.trpo import _spread_non_finite

    ref = C.steps_reference("nan_state")
    tensors = [torch.from_numpy(a.copy()) for k in ("params", "m", "v") for a in ref[k]]
    loss = torch.from_numpy(ref["loss"].copy())
    assert torch.isfinite(loss).all() and torch.isfinite(tensors[5]).all()
    _spread_non_finite(tensors, loss)
    assert all(torch.isnan(t).all() for t in tensors)
    good = C.reference("ragged")
    tensors = [torch.from_numpy(a.copy()) for k in ("params", "m", "v") for a in good[k]]
    tensors[0][0, 0], tensors[1][0] = -0.0, 5e-324
    before = [t.clone() for t in tensors]
    _spread_non_finite(tensors, torch.from_numpy(good["loss"].copy()))
    assert all(C.bits_equal(a, b) for a, b in zip(before, tensors))
    tensors = [t.clone() for t in before]
    _spread_non_finite(tensors, torch.tensor([1.0, float("inf")], dtype=torch.float64))
    assert all(torch.isnan(t).all() for t in tensors)   # a non-finite loss alone is enough


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
