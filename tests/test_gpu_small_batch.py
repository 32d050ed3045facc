"""Batches under 16384 rows on the HIP kernels and the graph loop: the three row tiles of the
split policy forward give the same bits, get_log_p and its gradients below the old floor equal
the nn.Linear path, the graph-replayed iteration at the MountainCar script's batch (20 x 400
particles, 2 -> [300, 300] -> 1, k = 4) and at a small deep policy equals the eager path and the
oracle's torch CPU loop, and one CLI epoch of the script builds the loop.

Tolerances are the ones the same quantities have in tests/test_gpu_policy.py,
tests/test_gpu_multilayer_policy.py and tests/test_gpu_device_loop.py."""
import copy

import numpy as np
import pytest
import scipy.special
import torch

from loop_runs import _assert_same_run, _run

pytestmark = pytest.mark.gpu

TILES = (64, 32, 16)
TILE_NS = (1, 15, 16, 17, 31, 33, 63, 65, 257, 1000)
TILE_SHAPES = [(2, 48, 40, 1), (2, 300, 300, 1), (29, 64, 48, 5), (29, 400, 300, 8)]


# ---- 1. tile identity ------------------------------------------------------------------------
def _forward_operands(nf, h0, h1, a, n_max):
    from mepol_amd import policy as P

    torch.manual_seed(3)
    pol = P.GaussianPolicy([h0, h1], nf, a, -0.4).cuda()
    with torch.no_grad():  # biases off zero
        for p in pol.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    s = torch.randn(n_max, nf, dtype=torch.float64, device="cuda")
    act = 0.5 * torch.randn(n_max, a, dtype=torch.float64, device="cuda")
    params = (pol.net[0].weight.detach(), pol.net[0].bias.detach(), pol.net[2].weight.detach(),
              pol.net[2].bias.detach(), pol.mean.weight.detach(), pol.mean.bias.detach(),
              pol.log_std.detach())
    return s, act, params


@pytest.mark.parametrize("nf,h0,h1,a", TILE_SHAPES)
def test_row_tiles_give_the_same_bits(cuda, nf, h0, h1, a):
    from mepol_amd import ops
    from mepol_amd import policy as P

    s_all, act_all, (W1, b1, W2, b2, Wm, bm, ls) = _forward_operands(nf, h0, h1, a, max(TILE_NS))
    for n in TILE_NS:
        s, act = s_all[:n].contiguous(), act_all[:n].contiguous()
        outs = {}
        for t in TILES + (0,):
            mask = ops.h1_mask_buffer(n, h0, s.device)
            mask.fill_(-1)
            o = ops.policy_forward(s, W1, b1, W2, b2, Wm, bm, ls, act, mask_out=mask, row_tile=t)
            outs[t] = o + (mask,)
        for t in (32, 16, 0):
            for name, x, y in zip(("h1", "z2", "mu", "logp", "mask"), outs[64], outs[t]):
                assert torch.equal(x, y), (n, t, name)
        h1o, z2, mu, logp, mask = outs[64]
        h1_ref = torch.relu(s @ W1.t() + b1)
        z2_ref = h1_ref @ W2.t()
        mu_ref = torch.relu(z2_ref + b2) @ Wm.t() + bm
        std = torch.exp(ls) + 1e-7
        lp_ref = torch.sum(-0.5 * (P.LOG_2PI + 2 * ls + (act - mu_ref) ** 2 / std ** 2), dim=1)
        torch.testing.assert_close(h1o, h1_ref, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(z2, z2_ref, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(mu, mu_ref, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(logp, lp_ref, rtol=1e-12, atol=1e-11)
        # bit b of word w of row r = (h1[r][16 w + b] > 0)
        bits = (h1o > 0).to(torch.int32)
        pad = (-h0) % 16
        bits = torch.nn.functional.pad(bits, (0, pad)).view(n, -1, 16)
        words = (bits << torch.arange(16, device=bits.device, dtype=torch.int32)).sum(-1)
        assert torch.equal(words, mask.to(torch.int32) & 0xFFFF), n


def test_bad_row_tile_raises(cuda):
    from mepol_amd import _lib, ops

    s, act, (W1, b1, W2, b2, Wm, bm, ls) = _forward_operands(2, 48, 40, 1, 100)
    with pytest.raises(_lib.MepolInputError):
        ops.policy_forward(s, W1, b1, W2, b2, Wm, bm, ls, act, row_tile=48)
    # the one-kernel form (odd hidden0) has 64-row blocks only
    s, act, (W1, b1, W2, b2, Wm, bm, ls) = _forward_operands(2, 37, 40, 1, 100)
    ref = ops.policy_forward(s, W1, b1, W2, b2, Wm, bm, ls, act)
    got = ops.policy_forward(s, W1, b1, W2, b2, Wm, bm, ls, act, row_tile=64)
    assert all(torch.equal(x, y) for x, y in zip(ref, got))
    with pytest.raises(_lib.MepolError, match="rc=1003"):
        ops.policy_forward(s, W1, b1, W2, b2, Wm, bm, ls, act, row_tile=32)


# ---- 2. get_log_p and its gradients below the old floor --------------------------------------
@pytest.mark.parametrize("n,nf,hidden,a,fn", [(8000, 2, [300, 300], 1, "TwoLayer"),
                                              (1000, 29, [64, 48], 8, "TwoLayer"),
                                              (2000, 2, [64, 48, 32], 2, "MultiLayer")],
                         ids=["mountaincar", "few-row-blocks", "deep"])
def test_logp_and_gradients_below_the_old_floor(cuda, monkeypatch, n, nf, hidden, a, fn):
    from mepol_amd import policy as P

    monkeypatch.delenv("MEPOL_FUSED_MIN_ROWS", raising=False)
    assert P.FUSED_MIN_ROWS <= n < P.SPLITK_MIN_ROWS
    torch.manual_seed(1)
    pol = P.GaussianPolicy(hidden, nf, a, -0.3).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    s = torch.randn(n, nf, dtype=torch.float64, device="cuda")
    act = 0.5 * torch.randn(n, a, dtype=torch.float64, device="cuda")
    coef = torch.randn(n, dtype=torch.float64, device="cuda")
    lp = pol.get_log_p(s, act)
    assert lp.grad_fn is not None and fn in type(lp.grad_fn).__name__
    (coef * lp).sum().backward()
    got = {k: v.grad.clone() for k, v in pol.named_parameters()}
    pol.zero_grad()
    monkeypatch.setenv("MEPOL_FUSED_MIN_ROWS", str(n + 1))  # the plain nn.Linear path
    ref = pol.get_log_p(s, act)
    assert "Logp" not in type(ref.grad_fn).__name__
    (coef * ref).sum().backward()
    if fn == "TwoLayer":  # tests/test_gpu_policy.py
        assert torch.allclose(lp, ref, rtol=1e-12, atol=1e-12)
        for k, v in pol.named_parameters():
            err = (got[k] - v.grad).abs().max().item()
            print(f"{k}: max |err| {err:.3e} of max |grad| {v.grad.abs().max().item():.3e}")
            assert torch.allclose(got[k], v.grad, rtol=1e-10, atol=1e-12 * v.grad.abs().max()), k
    else:                 # tests/test_gpu_multilayer_policy.py
        np.testing.assert_allclose(lp.detach().cpu().numpy(), ref.detach().cpu().numpy(),
                                   rtol=1e-10)
        for k, v in pol.named_parameters():
            g, w = got[k].cpu().numpy(), v.grad.cpu().numpy()
            print(f"{k}: max |err| {np.abs(g - w).max():.3e} of max |grad| {np.abs(w).max():.3e}")
            np.testing.assert_allclose(g, w, rtol=1e-8, atol=1e-11, err_msg=k)


# ---- 3. graph loop == eager == oracle --------------------------------------------------------
MC = dict(NT=20, T=400, NF=2, A=1, K=4, HID=[300, 300])   # scripts/tae/mountain_car.sh's batch
DEEP = dict(NT=10, T=200, NF=2, A=2, K=4, HID=[64, 48, 32])
MAX_BT = 4  # the backtracking tries loop_runs._run passes to the loop


def _oracle_loop(g, c, opt_name, lr, kl_threshold, max_off_iters):
    """The off-policy loop of mepol.py:416-483 (KL acceptance, backtracking with coefficient 2
    and MAX_BT tries) on the oracle's torch CPU policy_update / compute_kl / compute_entropy,
    from _setup's initial weights, the same particles and the GPU's D / I."""
    import oracle.mepol_oracle as O
    from mepol_amd.policy import GaussianPolicy

    NT, T, NF, A, K, HID = c["NT"], c["T"], c["NF"], c["A"], c["K"], c["HID"]
    states, actions = g["raw"]
    torch.manual_seed(5)
    sd = GaussianPolicy(HID, NF, A).state_dict()  # the initial weights _setup drew
    beh = O.TorchPolicy(HID, NF, A)
    beh.load_state_dict(sd)
    tgt, last = copy.deepcopy(beh), copy.deepcopy(beh)
    opt_cls = torch.optim.Adam if opt_name == "adam" else torch.optim.RMSprop
    opt = opt_cls(tgt.parameters(), lr=lr)
    S = torch.as_tensor(states, dtype=torch.float64)
    Ac = torch.as_tensor(actions, dtype=torch.float64)
    lengths = torch.full((NT, 1), T, dtype=torch.int64)
    D, I = g["D"].cpu(), g["I"].cpu()
    G = float(scipy.special.gamma(NF / 2 + 1))
    B = float(np.log(K) - scipy.special.digamma(K))
    trace, n, bt, cur_lr = [], 0, 1, lr
    while True:
        loss, err = O.torch_policy_update(opt, beh, tgt, S, Ac, NT, lengths, D, I, K, G, B, NF,
                                          0.0)
        kl, kl_err = O.torch_kl(beh, tgt, S, Ac, NT, lengths, I, K, 0.0)
        if not err and not kl_err and float(kl) <= kl_threshold:
            last.load_state_dict(tgt.state_dict())
            n += 1
            trace.append((n, -float(loss.detach()), float(kl), cur_lr))
        elif bt != MAX_BT:
            tgt.load_state_dict(last.state_dict())
            cur_lr = lr / 2 ** bt
            for group in opt.param_groups:
                group["lr"] = cur_lr
            bt += 1
            continue
        else:
            break
        if bt > 1 or n == max_off_iters:
            break
    with torch.no_grad():
        H = float(O.torch_entropy(last, last, S, Ac, NT, lengths, D, I, K, G, B, NF, 0.0))
    params = torch.cat([q.detach().reshape(-1) for q in last.parameters()]).numpy()
    return dict(trace=trace, n=n, bt=bt, lr=cur_lr, H=H, params=params)


def _assert_matches_oracle(g, o):
    """The tolerances of tests/test_gpu_device_loop.py::_oracle_steps."""
    assert (g["n"], g["bt"], g["lr"]) == (o["n"], o["bt"], o["lr"])
    assert len(g["trace"]) == len(o["trace"])
    for a, b in zip(g["trace"], o["trace"]):
        assert a[0] == b[0] and a[3] == b[3]
        np.testing.assert_allclose(a[1], b[1], rtol=1e-9)
        np.testing.assert_allclose(a[2], b[2], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(g["H"], o["H"], rtol=1e-9)
    np.testing.assert_allclose(g["params"], o["params"], rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("case", ["accepted", "rejected"])
@pytest.mark.parametrize("opt_name", ["adam", "rmsprop"])
@pytest.mark.parametrize("shape", ["mountaincar", "deep"])
def test_small_batch_graph_loop(cuda, monkeypatch, shape, opt_name, case):
    """accepted: every step passes the KL test until max_off_iters (the importance weights are
    products over 200 to 400 steps of a trajectory, so the learning rates are a hundredth of
    the ones tests/test_gpu_device_loop.py uses at 1250 steps and 29 features: Adam at 1e-3
    has its first step rejected here).  rejected: a high learning rate against a small
    threshold, so the first step is rejected and the loop backtracks."""
    monkeypatch.delenv("MEPOL_FUSED_MIN_ROWS", raising=False)
    c = MC if shape == "mountaincar" else DEEP
    if case == "accepted":
        lr, thr = (1e-5 if opt_name == "adam" else 1e-6), 10.0
    else:
        lr, thr = 5e-2, 1e-3
    g = _run(monkeypatch, True, opt_name, lr, thr, cfg=c)
    e = _run(monkeypatch, False, opt_name, lr, thr, cfg=c)
    print("graph", g["n"], g["bt"], g["lr"], g["trace"])
    # the graph run is the iteration object of device_loop._CACHE
    assert g["it_type"].__name__ == ("DeviceIteration" if shape == "mountaincar" else
                            "MultiLayerIteration")
    if case == "accepted":
        assert g["n"] == 6 and g["bt"] == 1
    else:
        assert g["bt"] > 1
    _assert_same_run(g, e)
    _assert_matches_oracle(g, _oracle_loop(g, c, opt_name, lr, thr, 6))


def test_small_batch_graph_loop_backtracked_step_accepted(cuda, monkeypatch):
    """Adam at 1e-3 on the MountainCar-script shape: the first tries exceed KL 10, a halved
    learning rate passes, and the loop ends on that accepted backtracked step."""
    monkeypatch.delenv("MEPOL_FUSED_MIN_ROWS", raising=False)
    g = _run(monkeypatch, True, "adam", 1e-3, 10.0, cfg=MC)
    e = _run(monkeypatch, False, "adam", 1e-3, 10.0, cfg=MC)
    print("graph", g["n"], g["bt"], g["lr"], g["trace"])
    assert g["it_type"].__name__ == "DeviceIteration" and g["bt"] > 1 and g["n"] == 1
    _assert_same_run(g, e)
    _assert_matches_oracle(g, _oracle_loop(g, MC, "adam", 1e-3, 10.0, 6))


# ---- 4. one CLI-level epoch of the MountainCar script ----------------------------------------
def test_cli_mountaincar_script_batch_builds_the_loop(cuda, monkeypatch, tmp_path):
    from mepol_amd.algorithms import device_loop
    from mepol_amd.experiments.mepol import main

    monkeypatch.delenv("MEPOL_FUSED_MIN_ROWS", raising=False)
    monkeypatch.setenv("MEPOL_DEVICE_LOOP", "1")
    built = []
    orig = device_loop.get

    def counting(*args, **kw):
        it = orig(*args, **kw)
        built.append((type(it).__name__, it.N))
        return it

    monkeypatch.setattr(device_loop, "get", counting)
    rc = main(["--env", "MountainCar", "--k", "4", "--kl_threshold", "15", "--max_off_iters", "30",
               "--learning_rate", "0.0001", "--num_trajectories", "20", "--trajectory_length",
               "400", "--num_epochs", "2", "--heatmap_every", "1000", "--heatmap_episodes", "1",
               "--heatmap_num_steps", "10", "--use_backtracking", "1", "--zero_mean_start", "1",
               "--full_entropy_traj_scale", "5", "--full_entropy_k", "4", "--seed", "3",
               "--results_dir", str(tmp_path)])
    assert rc == 0
    assert built == [("DeviceIteration", 8000)] * 2  # one loop per epoch, at the script's batch
