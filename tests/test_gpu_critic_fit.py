"""TRPO's critic fit in one launch (ops.critic_fit, csrc/critic_fit.hip) against the long-double
stand-in of critic_cases.py, and the driver above it (_fit_critic, trpo()).

Tolerance (critic_cases.GPU_ATOL = 1e-12 absolute on parameters and moments, 1e-12 relative on
the loss): about 1000 x the spread between the stand-in and a torch autograd loop
(test_critic_cases_host.py), and ten orders below one wrong step at lr = 1e-2.  Largest observed
deviations per case: profiles/r17/critic_fit/README.md (at most 4.4e-16 on parameters and
moments, 8.2e-16 on the loss).
"""
import functools

import numpy as np
import pytest
import torch

import critic_cases as C

pytestmark = pytest.mark.gpu


def _dev(arrays):
    return [torch.from_numpy(a.copy()).cuda() for a in arrays]


def _run(name):
    """One launch of the case; (result in fit_reference's form, states, targets as they came
    back).  loss_out is pre-filled with 0xff bytes."""
    from mepol_amd import ops

    c = C.case(name)
    states, targets = _dev([c["states"], c["targets"]])
    index = torch.from_numpy(c["index"].copy()).cuda()
    p, m, v = _dev(c["params"]), _dev(c["m"]), _dev(c["v"])
    n_steps = c["index"].size // c["B"]
    loss = torch.empty(n_steps, dtype=torch.float64, device="cuda")
    loss.view(torch.uint8).fill_(0xFF)
    out = ops.critic_fit(states, targets, index, c["B"], p, m, v, C.LR, betas=C.BETAS, eps=C.EPS,
                         first_step=c["first_step"], loss_out=loss)
    assert out is loss
    res = {"params": [t.cpu().numpy() for t in p], "m": [t.cpu().numpy() for t in m],
           "v": [t.cpu().numpy() for t in v], "loss": loss.cpu().numpy()}
    return res, states.cpu().numpy(), targets.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gpu(name):
    return _run(name)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64))
               for k in ("params", "m", "v") for x, y in zip(a[k], b[k])) and np.array_equal(
                   a["loss"].view(np.uint64), b["loss"].view(np.uint64))


@pytest.mark.parametrize("name", C.NAMES)
def test_case_against_the_stand_in(cuda, name):
    got, states, targets = _gpu(name)
    c = C.case(name)
    assert np.array_equal(states, c["states"])
    assert np.array_equal(targets, c["targets"], equal_nan=True)
    assert np.isfinite(got["loss"]).all()  # every 0xff byte overwritten
    dev, rel = C.max_deviation(got, C.reference(name))
    print(f"{name}: GPU vs stand-in: max abs {dev:.3e}, loss rel {rel:.3e}")
    assert dev <= C.GPU_ATOL and rel <= C.GPU_LOSS_RTOL


@pytest.mark.parametrize("name", C.NAMES)
def test_two_calls_give_the_same_bits(cuda, name):
    again, _, _ = _run(name)
    assert _same_bits(again, _gpu(name)[0])


def test_nan_target_in_an_unread_row_changes_nothing(cuda):
    assert _same_bits(_gpu("ragged")[0], _gpu("ragged_nan")[0])


def test_dead_units_stay_exactly_where_they_were(cuda):
    got, c = _gpu("dead_unit")[0], C.case("dead_unit")
    assert np.array_equal(C.dead_elements(got, "params"), C.dead_elements(c, "params"))
    assert not C.dead_elements(got, "m").any() and not C.dead_elements(got, "v").any()


@pytest.mark.parametrize("shape,limit", C.REFUSED)
def test_shapes_outside_the_limits_are_refused(cuda, shape, limit):
    from mepol_amd import _lib, ops

    nf, h0, h1, B = shape
    f64 = dict(dtype=torch.float64, device="cuda")
    shapes = [(h0, nf), (h0,), (h1, h0), (h1,), (1, h1), (1,)]
    p, m, v = ([torch.zeros(s, **f64) for s in shapes] for _ in range(3))
    states, targets = torch.zeros((100, nf), **f64), torch.zeros(100, **f64)
    index = torch.zeros(max(B, 1), dtype=torch.int32, device="cuda")
    plan = ops.critic_fit_plan(nf, h0, h1, B)
    assert not plan["accepted"]
    with pytest.raises(_lib.MepolInputError) as e:
        ops.critic_fit(states, targets, index, B, p, m, v, C.LR)
    assert "rc=1001" in str(e.value) and limit in str(e.value)
    torch.cuda.synchronize()
    assert all(not t.any() for t in p + m + v)  # nothing ran


def test_plan_info(cuda):
    from mepol_amd import ops

    plan = ops.critic_fit_plan(2, 64, 64, 64)
    assert plan["accepted"] and plan["threads"] == 256
    assert 0 < plan["lds_bytes"] <= 160 * 1024
    assert ops.critic_fit_plan(1, 1, 1, 1)["accepted"]
    assert ops.critic_fit_plan(16, 64, 64, 64)["accepted"]


def test_argument_checks(cuda):
    from mepol_amd import ops

    c = C.case("full_1step")
    states, targets = _dev([c["states"], c["targets"]])
    index = torch.from_numpy(c["index"].copy()).cuda()
    p, m, v = _dev(c["params"]), _dev(c["m"]), _dev(c["v"])
    with pytest.raises(ValueError, match="int32"):
        ops.critic_fit(states, targets, index.long(), 64, p, m, v, C.LR)
    with pytest.raises(ValueError, match="f64"):
        ops.critic_fit(states.float(), targets, index, 64, p, m, v, C.LR)
    with pytest.raises(ValueError, match="CPU"):
        ops.critic_fit(states.cpu(), targets, index, 64, p, m, v, C.LR)
    with pytest.raises(ValueError, match="contiguous"):
        ops.critic_fit(states, targets, index, 64, [p[0].t().contiguous().t()] + p[1:], m, v, C.LR)
    with pytest.raises(ValueError, match="whole number"):
        ops.critic_fit(states, targets, index[:63], 64, p, m, v, C.LR)
    with pytest.raises(ValueError, match="shapes"):
        ops.critic_fit(states, targets, index, 64, p, m[:2] + m[:4], v, C.LR)
    for t, a in zip(p, c["params"]):
        assert np.array_equal(t.cpu().numpy(), a)


def test_index_outside_the_rows_reads_nothing_and_shows(cuda):
    """An index outside [0, N) must not be followed: the step's loss comes back NaN."""
    from mepol_amd import ops

    c = C.case("ragged")
    states, targets = _dev([c["states"], c["targets"]])
    index = torch.from_numpy(c["index"][:5].copy()).cuda()
    index[2] = c["N"]
    p, m, v = _dev(c["params"]), _dev(c["m"]), _dev(c["v"])
    loss = ops.critic_fit(states, targets, index, 5, p, m, v, C.LR)
    assert torch.isnan(loss).all()


def _critic_and_batch(seed):
    from mepol_amd.experiments.goal_rl import create_critic

    torch.manual_seed(seed)
    vfunc = create_critic(2).to(device="cuda", dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 1)
    states = torch.rand(341, 2, generator=g, dtype=torch.float64).cuda()
    targets = torch.randn(341, 1, generator=g, dtype=torch.float64).cuda()
    return vfunc, torch.optim.Adam(vfunc.parameters(), lr=1e-2), states, targets


def _fit_then_one_torch_step(path, monkeypatch):
    """_fit_critic (2 passes of 7 mini-batches of 48 over 341 rows) on `path`, then one torch
    optimizer.step() on a further batch: the optimizer must be able to go on from the state the
    fit leaves."""
    from mepol_amd.algorithms import trpo as TR

    monkeypatch.setenv("MEPOL_CRITIC_FIT", path)
    vfunc, opt, states, targets = _critic_and_batch(21)
    torch.manual_seed(77)
    TR._fit_critic(vfunc, opt, "adam", states, targets, 1e-3, 2, 48)
    assert TR.CRITIC_FIT_STATS["path"] == path
    rng_after = torch.get_rng_state()
    opt.zero_grad()
    torch.mean((vfunc(states[:50]) - targets[:50]) ** 2).backward()
    opt.step()
    params = list(vfunc.parameters())
    return {"params": [p.detach().cpu().numpy() for p in params],
            "m": [opt.state[p]["exp_avg"].cpu().numpy() for p in params],
            "v": [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in params],
            "loss": np.ones(1), "step": [float(opt.state[p]["step"]) for p in params],
            "rng": rng_after}


def test_driver_leaves_the_optimizer_where_the_host_loop_would(cuda, monkeypatch):
    k = _fit_then_one_torch_step("kernel", monkeypatch)
    h = _fit_then_one_torch_step("host", monkeypatch)
    dev, _ = C.max_deviation(k, h)
    print(f"driver: kernel path vs host path after 14 + 1 steps: max abs {dev:.3e}")
    assert dev <= C.GPU_ATOL
    assert k["step"] == h["step"] == [15.0] * 6
    assert torch.equal(k["rng"], h["rng"])  # the global CPU generator did not move


def test_driver_continues_a_used_optimizer(cuda, monkeypatch):
    """Two fits in a row (epochs): the second starts from the first's moments and step number."""
    from mepol_amd.algorithms import trpo as TR

    res = {}
    for path in ("kernel", "host"):
        monkeypatch.setenv("MEPOL_CRITIC_FIT", path)
        vfunc, opt, states, targets = _critic_and_batch(22)
        torch.manual_seed(78)
        for _ in range(2):
            TR._fit_critic(vfunc, opt, "adam", states, targets, 1e-3, 1, 64)
            assert TR.CRITIC_FIT_STATS["path"] == path
        params = list(vfunc.parameters())
        res[path] = {"params": [p.detach().cpu().numpy() for p in params],
                     "m": [opt.state[p]["exp_avg"].cpu().numpy() for p in params],
                     "v": [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in params],
                     "loss": np.ones(1)}
        assert [float(opt.state[p]["step"]) for p in params] == [10.0] * 6
    dev, _ = C.max_deviation(res["kernel"], res["host"])
    print(f"driver, two fits: kernel path vs host path: max abs {dev:.3e}")
    assert dev <= C.GPU_ATOL


def test_gate_on_the_gpu(cuda, monkeypatch):
    from mepol_amd import kernel_path

    monkeypatch.delenv("MEPOL_CRITIC_FIT", raising=False)
    vfunc, opt, states, _ = _critic_and_batch(23)
    reason, params = kernel_path.critic_fit_refusal(vfunc, opt, states, 64)
    assert reason is None and all(a is b for a, b in zip(params, vfunc.parameters()))
    assert kernel_path.critic_fit_ok(vfunc, opt, states.cpu(), 64) is None
    assert kernel_path.critic_fit_ok(vfunc, opt, states.float(), 64) is None
    assert kernel_path.critic_fit_ok(vfunc, opt, states[:10], 64) is None
    assert kernel_path.critic_fit_ok(vfunc, opt, states, 65) is None
    monkeypatch.setenv("MEPOL_CRITIC_FIT", "host")
    assert kernel_path.critic_fit_ok(vfunc, opt, states, 64) is None


def test_trpo_two_epochs_fit_the_critic_on_the_kernel_path(cuda, tmp_path, monkeypatch):
    """trpo() with the Adam critic at the smoke shape: both epochs' fits go through
    ops.critic_fit, CSV rows are written, the critic is finite and has moved."""
    from mepol_amd import ops
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.envs import CustomRewardEnv, GridGoal, GridWorldContinuous
    from mepol_amd.experiments.goal_rl import create_critic
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_CRITIC_FIT", raising=False)
    calls = []
    real = ops.critic_fit

    def counted(*a, **k):
        out = real(*a, **k)
        calls.append(out.numel())
        return out

    monkeypatch.setattr(ops, "critic_fit", counted)
    torch.manual_seed(2)
    policy = GaussianPolicy([300, 300], 2, 2, -1.5).cuda()
    vfunc = create_critic(2)
    start = [p.detach().clone().double() for p in vfunc.parameters()]
    TR.trpo(lambda: CustomRewardEnv(GridWorldContinuous(), GridGoal((-5, -5))), "GridGoalTest", 2,
            600, 60, vfunc=vfunc, policy=policy, optimizer="adam", critic_iters=2,
            critic_batch_size=64, cg_iters=10, kl_thresh=0.01, out_path=str(tmp_path), seed=3)
    assert calls == [2 * (600 // 64)] * 2  # one launch per epoch, 2 passes of 9 steps
    assert TR.CRITIC_FIT_STATS["path"] == "kernel"
    lines = (tmp_path / "GridGoalTest.csv").read_text().splitlines()
    assert [r.split(",")[:2] for r in lines[1:]] == [["0", "600"], ["1", "1200"]]
    now = list(vfunc.parameters())
    assert all(p.is_cuda and torch.isfinite(p).all() for p in now)
    assert all(not torch.equal(a.cuda(), b) for a, b in zip(start, now))
