"""Policies with three or more hidden layers on the f64 MFMA path: _MultiLayerLogp (policy.py)
against the oracle's torch CPU policy, and the graph-replayed MultiLayerIteration
(algorithms/device_loop.py) == the eager path == the oracle's torch CPU loop.  The particle
set-up is tests/test_gpu_device_loop.py's SMALL one."""
import copy
import glob
import os

import numpy as np
import pytest
import scipy.special
import torch
import torch.nn as nn

from loop_runs import _assert_same_run, _run

pytestmark = pytest.mark.gpu

NT, T, NF, A, K = 16, 1250, 29, 8, 10  # N = 20000 >= the fused-path minimum
HID3 = [64, 48, 32]
HID4 = [72, 200, 50, 34]


def _cfg(HID, NF=NF, A=A, activation=nn.ReLU):
    return dict(NT=NT, T=T, NF=NF, A=A, K=K, HID=HID, activation=activation)


# ---- 1. get_log_p and its gradients ----------------------------------------------------------
def _oracle_policy(HID, nf, a, sd, activation=nn.ReLU):
    import oracle.mepol_oracle as O

    ref = O.TorchPolicy(HID, nf, a)
    if activation is not nn.ReLU:
        for i in range(1, len(ref.net), 2):
            ref.net[i] = activation()
    ref.load_state_dict(sd)
    return ref


def _logp_case(HID, nf, a, activation=nn.ReLU, seed=7):
    """(policy on the GPU, its logp, the oracle's policy and logp on the CPU) for N = 20000
    random state / action rows and the same state dict."""
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(seed)
    pol = GaussianPolicy(HID, nf, a, activation=activation)
    with torch.no_grad():  # biases off zero, so every bias gradient path carries a signal
        for p in pol.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    sd = {k: v.clone() for k, v in pol.state_dict().items()}
    N = NT * T
    s = torch.randn(N, nf, dtype=torch.float64)
    ac = 0.5 * torch.randn(N, a, dtype=torch.float64)
    ref = _oracle_policy(HID, nf, a, sd, activation)
    ref_logp = ref.get_log_p(s, ac)
    pol = pol.cuda()
    logp = pol.get_log_p(s.cuda(), ac.cuda())
    return pol, logp, ref, ref_logp


def _assert_logp_and_grads(pol, logp, ref, ref_logp):
    np.testing.assert_allclose(logp.detach().cpu().numpy(), ref_logp.detach().numpy(), rtol=1e-10)
    logp.sum().backward()
    ref_logp.sum().backward()
    got, want = dict(pol.named_parameters()), dict(ref.named_parameters())
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].grad is not None, name
        g, w = got[name].grad.cpu().numpy(), want[name].grad.numpy()
        print(f"{name}: max |err| {np.abs(g - w).max():.3e} of max |grad| {np.abs(w).max():.3e}")
        np.testing.assert_allclose(g, w, rtol=1e-8, atol=1e-11, err_msg=name)


@pytest.mark.parametrize("HID,nf,a", [(HID3, NF, A), (HID4, NF, A), (HID3, 63, 20)],
                         ids=["hid3", "hid4", "hid3-nf63-a20"])
def test_multilayer_logp_and_gradients_match_oracle(cuda, monkeypatch, HID, nf, a):
    from mepol_amd import policy as P

    used = []
    orig = P._MultiLayerLogp.forward

    def spy(ctx, *args):
        used.append(len(args))
        return orig(ctx, *args)

    monkeypatch.setattr(P._MultiLayerLogp, "forward", staticmethod(spy))
    pol, logp, ref, ref_logp = _logp_case(HID, nf, a)
    assert used == [2 + 2 * len(HID) + 3]  # the native path ran, with all 2 L + 3 parameters
    assert len(list(pol.parameters())) == 2 * len(HID) + 3
    _assert_logp_and_grads(pol, logp, ref, ref_logp)


# ---- 2. graph loop == eager ------------------------------------------------------------------
@pytest.mark.parametrize("opt_name,lr,kl_threshold,HID", [
    ("adam", 1e-3, 10.0, HID3),
    ("rmsprop", 1e-4, 10.0, HID3),
    ("adam", 1e-3, 10.0, HID4),
], ids=["adam-hid3", "rmsprop-hid3", "adam-hid4"])
def test_multilayer_graph_loop_matches_eager(cuda, monkeypatch, opt_name, lr, kl_threshold, HID):
    from mepol_amd.algorithms import device_loop

    g = _run(monkeypatch, True, opt_name, lr, kl_threshold, cfg=_cfg(HID))
    e = _run(monkeypatch, False, opt_name, lr, kl_threshold, cfg=_cfg(HID))
    assert g["it_type"] is device_loop.MultiLayerIteration
    _assert_same_run(g, e)


# ---- 3. graph loop == oracle -----------------------------------------------------------------
def _oracle_steps(g, cfg, lr, steps):
    """Replay `steps` accepted Adam steps of the oracle's torch-CPU policy_update/compute_kl
    (oracle/mepol_oracle.py, mepol.py:268-281, 157-174) from _setup's initial weights on the
    same particles and the GPU's D/I; compare H, KL per step and the final parameters."""
    import oracle.mepol_oracle as O
    from mepol_amd.policy import GaussianPolicy

    NT, T, NF, A, K, HID = cfg["NT"], cfg["T"], cfg["NF"], cfg["A"], cfg["K"], cfg["HID"]
    states, actions = g["raw"]
    torch.manual_seed(5)
    sd = GaussianPolicy(HID, NF, A).state_dict()  # the initial weights _setup drew
    beh = O.TorchPolicy(HID, NF, A)
    beh.load_state_dict(sd)
    tgt = copy.deepcopy(beh)
    opt = torch.optim.Adam(tgt.parameters(), lr=lr)
    S = torch.as_tensor(states, dtype=torch.float64)
    Ac = torch.as_tensor(actions, dtype=torch.float64)
    lengths = torch.full((NT, 1), T, dtype=torch.int64)
    D, I = g["D"].cpu(), g["I"].cpu()
    G = float(scipy.special.gamma(NF / 2 + 1))
    B = float(np.log(K) - scipy.special.digamma(K))
    for it in range(steps):
        loss, _ = O.torch_policy_update(opt, beh, tgt, S, Ac, NT, lengths, D, I, K, G, B, NF, 0.0)
        kl, _ = O.torch_kl(beh, tgt, S, Ac, NT, lengths, I, K, 0.0)
        np.testing.assert_allclose(g["trace"][it][1], -float(loss.detach()), rtol=1e-9)
        np.testing.assert_allclose(g["trace"][it][2], float(kl), rtol=1e-9, atol=1e-13)
    p = torch.cat([q.detach().reshape(-1) for q in tgt.parameters()]).numpy()
    np.testing.assert_allclose(g["params"], p, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("HID", [HID3, HID4], ids=["hid3", "hid4"])
def test_multilayer_graph_loop_matches_oracle(cuda, monkeypatch, HID):
    cfg = _cfg(HID)
    g = _run(monkeypatch, True, "adam", 1e-3, 1e9, max_off_iters=3, cfg=cfg)
    assert g["used"] and g["n"] == 3
    _oracle_steps(g, cfg, 1e-3, 3)


# ---- 4. rejection mid-loop -------------------------------------------------------------------
_PROBE = {}


def _probe_kls(monkeypatch):
    """KL of six eager steps accepted at any threshold (computed once for both cases)."""
    if "kls" not in _PROBE:
        probe = _run(monkeypatch, False, "adam", 1e-3, 1e9, max_off_iters=6, cfg=_cfg(HID3))
        _PROBE["kls"] = [t[2] for t in probe["trace"]]
    return _PROBE["kls"]


@pytest.mark.parametrize("speculate", ["1", "0"])
def test_multilayer_graph_loop_mid_loop_rejection(cuda, monkeypatch, speculate):
    """A step rejected after accepted ones, while the next replay is already in flight
    (speculative launch): the cancelled replay leaves theta, the moments and the step count
    as the eager loop does."""
    monkeypatch.setenv("MEPOL_SPECULATE", speculate)
    kls = _probe_kls(monkeypatch)
    # the last step whose KL exceeds every earlier one: a threshold between them accepts the
    # steps before it and rejects it (KL is not monotone in the step count)
    cut = [i for i in range(1, len(kls)) if kls[i] > max(kls[:i])]
    assert len(kls) == 6 and cut, kls
    i = cut[-1]
    thr = 0.5 * (max(kls[:i]) + kls[i])
    g = _run(monkeypatch, True, "adam", 1e-3, thr, max_off_iters=6, cfg=_cfg(HID3))
    e = _run(monkeypatch, False, "adam", 1e-3, thr, max_off_iters=6, cfg=_cfg(HID3))
    assert 1 <= i <= e["n"] <= i + 1  # accepted steps, the rejection, the backtracked step
    assert e["bt"] > 1                # a step was rejected
    _assert_same_run(g, e)


# ---- 5. gates --------------------------------------------------------------------------------
@pytest.mark.parametrize("HID,activation", [([64, 47, 32], nn.ReLU), (HID3, nn.Tanh)],
                         ids=["odd-width", "tanh"])
def test_other_shapes_keep_their_path(cuda, monkeypatch, HID, activation):
    from mepol_amd import policy as P

    def never(*a, **k):
        raise AssertionError("_MultiLayerLogp ran for a shape it does not cover")

    monkeypatch.setattr(P._MultiLayerLogp, "forward", staticmethod(never))
    g = _run(monkeypatch, True, "adam", 1e-3, 10.0, max_off_iters=1,
             cfg=_cfg(HID, activation=activation))
    assert not g["used"] and g["n"] == 1
    pol, logp, ref, ref_logp = _logp_case(HID, NF, A, activation=activation)
    np.testing.assert_allclose(logp.detach().cpu().numpy(), ref_logp.detach().numpy(), rtol=1e-10)


def test_two_layer_policy_keeps_its_iteration(cuda, monkeypatch):
    from mepol_amd.algorithms import device_loop

    g = _run(monkeypatch, True, "adam", 1e-3, 10.0, max_off_iters=1, cfg=_cfg([64, 48]))
    assert g["used"] and g["fused"] == (True, True)
    assert g["it_type"] is device_loop.DeviceIteration


# ---- 6. CLI ----------------------------------------------------------------------------------
def test_cli_hidden_sizes_epoch(cuda, tmp_path):
    from mepol_amd.experiments.mepol import main
    from mepol_amd.policy import GaussianPolicy

    env = "GridWorld"
    rc = main(["--env", env, "--k", "50", "--kl_threshold", "15", "--max_off_iters", "5",
               "--learning_rate", "0.0001", "--num_trajectories", "8", "--trajectory_length", "300",
               "--num_epochs", "1", "--heatmap_every", "1", "--heatmap_episodes", "1",
               "--heatmap_num_steps", "10", "--full_entropy_traj_scale", "2", "--full_entropy_k",
               "4", "--seed", "3", "--results_dir", str(tmp_path),
               "--hidden_sizes", "32", "32", "32"])
    assert rc == 0
    (run,) = glob.glob(os.path.join(tmp_path, "mepol", "*"))
    assert ",hidden=32x32x32__" in os.path.basename(run)
    csv1 = open(os.path.join(run, f"{env}.csv")).read().strip().splitlines()
    assert csv1[0] == "epoch,loss,entropy,full_entropy,num_off_iters,execution_time"
    assert len(csv1) == 1 + 2  # epoch 0 + 1 epoch
    csv3 = open(os.path.join(run, f"{env}_off_policy_iter.csv")).read().strip().splitlines()
    assert csv3[0] == "epoch,off_policy_iter,entropy,kl,learning_rate"
    csv2 = open(os.path.join(run, f"{env}-heatmap.csv")).read().strip().splitlines()
    assert csv2[0] == "epoch,average_entropy"
    assert "hidden_sizes=[32, 32, 32]" in open(os.path.join(run, "log_info.txt")).read()
    sd = torch.load(os.path.join(run, "1-policy"), weights_only=True)
    assert sorted(sd) == ["log_std", "mean.bias", "mean.weight", "net.0.bias", "net.0.weight",
                          "net.2.bias", "net.2.weight", "net.4.bias", "net.4.weight"]
    pol = GaussianPolicy([32, 32, 32], 2, 2)
    pol.load_state_dict(sd)
    assert pol.net[4].weight.shape == (32, 32)
