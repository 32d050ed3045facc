"""One off-policy loop on random particles, as a graph-replayed or an eager run, and the
comparison of two such runs: shared by tests/test_gpu_device_loop.py,
tests/test_gpu_multilayer_policy.py, tests/test_gpu_small_batch.py and
tests/test_gpu_loop_launch_order.py, which keep their own shapes.

cfg: dict(NT, T, NF, A, K, HID) and, optionally, activation (default nn.ReLU)."""
import numpy as np
import scipy.special
import torch
import torch.nn as nn


def _setup(opt_name, lr, seed=5, *, cfg):
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.policy import GaussianPolicy

    NT, T, NF, A, K, HID = (cfg[n] for n in ("NT", "T", "NF", "A", "K", "HID"))
    act = cfg.get("activation", nn.ReLU)
    rng = np.random.default_rng(seed)
    states = rng.standard_normal((NT, T + 1, NF)).astype(np.float32)
    actions = (0.5 * rng.standard_normal((NT, T, A))).astype(np.float32)
    dev = torch.device("cuda")
    st = torch.as_tensor(states, dtype=torch.float64, device=dev)
    ac = torch.as_tensor(actions, dtype=torch.float64, device=dev)
    rtl = torch.full((NT, 1), T, dtype=torch.int64, device=dev)
    nxt = torch.as_tensor(states[:, 1:].reshape(-1, NF), device=dev)
    torch.manual_seed(seed)
    beh = GaussianPolicy(HID, NF, A, activation=act).to(dev)
    tgt = GaussianPolicy(HID, NF, A, activation=act).to(dev)
    last = GaussianPolicy(HID, NF, A, activation=act).to(dev)
    tgt.load_state_dict(beh.state_dict())
    last.load_state_dict(beh.state_dict())
    opt_cls = torch.optim.Adam if opt_name == "adam" else torch.optim.RMSprop
    opt = opt_cls(tgt.parameters(), lr=lr)
    batch = M.make_particle_batch(st, ac, rtl, nxt, K)
    return M, (states, actions), beh, tgt, last, opt, batch


def _run(monkeypatch, graph, opt_name, lr, kl_threshold, max_off_iters=6, *, cfg,
         backtracking=True):
    from mepol_amd.algorithms import device_loop

    NT, NF, K = cfg["NT"], cfg["NF"], cfg["K"]
    monkeypatch.setenv("MEPOL_DEVICE_LOOP", "1" if graph else "0")
    M, raw, beh, tgt, last, opt, (st, ac, rl, _, D, I) = _setup(opt_name, lr, cfg=cfg)
    G = float(scipy.special.gamma(NF / 2 + 1))
    B = float(np.log(K) - scipy.special.digamma(K))
    trace = []
    res = M.off_policy_optimization(
        opt, beh, tgt, last, st, ac, NT, rl, D, I, K, G, B, NF, 0.0, kl_threshold, max_off_iters,
        backtracking, 2, 4, lr,
        on_accept=lambda n, e, kl, l: trace.append((n, float(e), float(kl), l)))
    used = tgt in device_loop._CACHE
    it = device_loop._CACHE.get(tgt)
    fused = (it.fused_fwd, it.fused_dh1) if it is not None else None
    params = torch.cat([p.detach().reshape(-1) for p in last.parameters()]).cpu().numpy()
    state = opt.state_dict()["state"]
    steps = [float(state[i]["step"]) for i in sorted(state)]
    moments = np.concatenate([state[i][key].detach().reshape(-1).cpu().numpy()
                              for i in sorted(state) for key in sorted(state[i])
                              if key != "step"])
    tparams = torch.cat([p.detach().reshape(-1) for p in tgt.parameters()]).cpu().numpy()
    return dict(H=float(res[0]), n=res[1], bt=res[2], lr=res[3], trace=trace, params=params,
                steps=steps, used=used, raw=raw, D=D, I=I, moments=moments, tparams=tparams,
                fused=fused, it_type=type(it) if it is not None else None)


def _assert_same_run(g, e):
    assert g["used"] and not e["used"]
    assert (g["n"], g["bt"], g["lr"]) == (e["n"], e["bt"], e["lr"])
    assert g["steps"] == e["steps"]
    assert len(g["trace"]) == len(e["trace"])
    for a, b in zip(g["trace"], e["trace"]):
        assert a[0] == b[0] and a[3] == b[3]
        np.testing.assert_allclose(a[1:3], b[1:3], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(g["H"], e["H"], rtol=1e-9)
    np.testing.assert_allclose(g["params"], e["params"], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(g["tparams"], e["tparams"], rtol=1e-8, atol=1e-11)
    # the optimizer moments carry into the next epoch: a cancelled speculative replay must
    # leave them exactly as the rejected step did
    np.testing.assert_allclose(g["moments"], e["moments"], rtol=1e-8, atol=1e-14)
