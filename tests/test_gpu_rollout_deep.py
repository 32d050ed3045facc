"""The one-launch rollout for ReLU policies with 3 to 6 hidden layers (mepol_rollout_deep,
csrc/rollout_deep.hip) against a plain-Python restatement of the summation order it commits to,
against the oracle's per-step rollout, and through collect_particles_device / get_heatmap."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import mepol_oracle as O

pytestmark = pytest.mark.gpu

ENVS = ["mountaincar", "gridworld"]


# ---- the kernel's order, restated ------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once (int / int true division is correctly rounded in CPython)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _deep_mean(layers, Wm, bm, x0, x1):
    """The policy mean for one state in the order of csrc/rollout_deep.hip; all Python floats."""
    W1, b1 = layers[0]
    h = [max((x0 * w[0] + x1 * w[1]) + b, 0.0) for w, b in zip(W1, b1)]
    for W, bias in layers[1:]:
        hp = len(h)
        Lc = -(-hp // 4)
        out = []
        for row, b in zip(W, bias):
            c = []
            for r in range(4):
                ka = min(r * Lc, hp)
                s = 0.0
                for k in range(ka, min(ka + Lc, hp)):
                    s = _fma(row[k], h[k], s)
                c.append(s)
            out.append(max((((c[0] + c[1]) + c[2]) + c[3]) + b, 0.0))
        h = out
    mu = []
    for wm, b in zip(Wm, bm):
        total = None
        for w0 in range(0, len(h), 64):
            v = [wm[j] * h[j] if j < len(h) else 0.0 for j in range(w0, w0 + 64)]
            for m in (32, 16, 8, 4, 2, 1):
                v = [v[i] + v[i ^ m] for i in range(64)]
            total = v[0] if total is None else total + v[0]
        mu.append(total + b)
    return mu


def _restated_rollout(env, sd, std, init, noise, T):
    """collect_particles with the mean from _deep_mean: states f32 [nt, T+1, 2], actions f32
    [nt, T, a], visited f64 [nt, T, 2] (the env's own state after each step)."""
    layers, i = [], 0
    while f"net.{i}.weight" in sd:
        layers.append((sd[f"net.{i}.weight"].tolist(), sd[f"net.{i}.bias"].tolist()))
        i += 2
    Wm, bm = sd["mean.weight"].tolist(), sd["mean.bias"].tolist()
    nt, a_dim = init.shape[0], noise.shape[2]
    states = np.zeros((nt, T + 1, 2), np.float32)
    actions = np.zeros((nt, T, a_dim), np.float32)
    visited = np.zeros((nt, T, 2), np.float64)
    s = init.astype(np.float64) if env == "mountaincar" else init.astype(np.float32)
    states[:, 0] = s
    sdv = [float(v) for v in std]
    for t in range(T):
        a = np.array([[m + float(noise[t, n, k]) * sdv[k] for k, m in enumerate(
            _deep_mean(layers, Wm, bm, float(s[n, 0]), float(s[n, 1])))] for n in range(nt)])
        actions[:, t] = a
        s = O.mountaincar_step(s, a) if env == "mountaincar" else O.gridworld_step(s, a)
        states[:, t + 1] = s
        visited[:, t] = s
    return states, actions, visited


# ---- shared inputs ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(env, hidden, nt, T):
    """(policy on the GPU, numpy state dict, init, noise): seeded as
    test_rollout_mlp_bitexact_vs_kordered_oracle seeds its own."""
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(11)
    a_dim = 1 if env == "mountaincar" else 2
    pol = GaussianPolicy(list(hidden), 2, a_dim, -0.5 if env == "mountaincar" else -1.5).cuda()
    rng = np.random.default_rng(3)
    if env == "mountaincar":
        init = np.stack([rng.uniform(-0.6, -0.4, nt), np.zeros(nt)], 1)
    else:
        init = rng.uniform(-6, -4, (nt, 2)).astype(np.float32)
    noise = rng.standard_normal((T, nt, a_dim))
    sd = {k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()}
    return pol, sd, init, noise


def _layers(pol):
    import torch.nn as nn

    return [(m.weight.detach(), m.bias.detach()) for m in pol.net if isinstance(m, nn.Linear)]


def _run(env, pol, init, noise, with_visited=True):
    from mepol_amd import ops

    T, nt, a_dim = noise.shape
    dev = "cuda"
    states = torch.zeros((nt, T + 1, 2), dtype=torch.float32, device=dev)
    actions = torch.zeros((nt, T, a_dim), dtype=torch.float32, device=dev)
    visited = torch.zeros((nt, T, 2), dtype=torch.float64, device=dev) if with_visited else None
    ops.rollout_deep(0 if env == "mountaincar" else 1, _layers(pol), pol.mean.weight.detach(),
                     pol.mean.bias.detach(), pol.log_std.detach(), torch.as_tensor(init, device=dev),
                     torch.as_tensor(noise, dtype=torch.float64, device=dev), states, actions,
                     visited)
    return states, actions, visited


# ---- 1. bit-exact against the restatement ----------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("hidden,nt,T", [((70, 9, 66), 3, 12), ((64, 130, 6, 33, 10, 65), 2, 6)],
                         ids=["70-9-66", "six-layers"])
def test_rollout_deep_bitexact_vs_restatement(cuda, env, hidden, nt, T):
    """[70, 9, 66]: chunks of 18 / 18 / 18 / 16 and 3 / 3 / 3 / empty rows, a last layer of two
    waves, one partial.  Six layers: widths rising and falling, a three-wave workgroup, chunks
    with empty and one-row tails.  GridWorld has no transcendental: bit-identical.  MountainCar's
    device cos() may differ from glibc's in the last ulp: step 0 exact, the rest to 1e-12."""
    pol, sd, init, noise = _case(env, hidden, nt, T)
    # exp(log_std) as the device computes it (ocml); it agrees with numpy's to an ulp
    std = torch.exp(pol.log_std.detach()).cpu().numpy()
    np.testing.assert_allclose(std, np.exp(sd["log_std"]), rtol=2.3e-16, atol=0)
    S_ref, A_ref, _ = _restated_rollout(env, sd, std, init, noise, T)
    states, actions, visited = _run(env, pol, init, noise)
    S, A = states.cpu().numpy(), actions.cpu().numpy()
    assert np.abs(A).max() > 0 and np.isfinite(A).all()
    if env == "gridworld":
        assert np.array_equal(A, A_ref)
        assert np.array_equal(S, S_ref)
    else:
        assert np.array_equal(A[:, 0], A_ref[:, 0])  # first step: no cos() involved yet
        np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(S, S_ref, rtol=0, atol=1e-12)
    assert np.array_equal(visited.cpu().numpy().astype(np.float32), S[:, 1:])


# ---- 2. wide shapes against the oracle's per-step rollout ------------------------------------
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("hidden", [(300, 300, 300), (512,) * 6], ids=["300x3", "512x6"])
def test_rollout_deep_wide_matches_oracle(cuda, env, hidden):
    nt, T = 4, 30
    pol, sd, init, noise = _case(env, hidden, nt, T)
    S_ref, A_ref = O.rollout(env, sd, sd["log_std"], init, noise, T)
    states, actions, visited = _run(env, pol, init, noise)
    S, A = states.cpu().numpy(), actions.cpu().numpy()
    assert np.abs(A - A_ref).max() < 1e-5
    assert np.abs(S - S_ref).max() < 1e-3
    assert np.array_equal(visited.cpu().numpy().astype(np.float32), S[:, 1:])


# ---- 3. LDS residency does not change bits ---------------------------------------------------
def test_rollout_deep_lds_rows_do_not_change_bits(cuda, monkeypatch):
    """The kernel keeps leading rows of the packed W^T buffer in LDS (64 of layer 2's 300 at this
    shape); MEPOL_ROLLOUT_KL = 0 streams everything, 37 ends the resident rows inside chunk 0."""
    pol, _, init, noise = _case("gridworld", (300, 300, 300), 4, 30)
    outs = []
    for kl in ("0", "37", None):
        if kl is None:
            monkeypatch.delenv("MEPOL_ROLLOUT_KL", raising=False)
        else:
            monkeypatch.setenv("MEPOL_ROLLOUT_KL", kl)
        outs.append(_run("gridworld", pol, init, noise))
    for out in outs[1:]:
        for x, y in zip(out, outs[0]):
            assert torch.equal(x, y)


# ---- 4 / 5. dispatch and shards --------------------------------------------------------------
def _gw_policy():
    from mepol_amd.envs import ErgodicEnv, GridWorldContinuous
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(11)
    return ErgodicEnv(GridWorldContinuous()), GaussianPolicy([48, 40, 56], 2, 2, -1.5).cuda()


def _direct(env, pol, nt, T, seed):
    """ops.rollout_deep on the init / noise collect_particles_device draws from this seed."""
    from mepol_amd import ops
    from mepol_amd.envs.wrappers import unwrap

    g = torch.Generator(device="cuda").manual_seed(seed)
    init = unwrap(env).reset_batch_torch(nt, pol.device, g)
    noise = torch.randn((T, nt, 2), dtype=torch.float64, device="cuda", generator=g)
    states = torch.zeros((nt, T + 1, 2), dtype=torch.float32, device="cuda")
    actions = torch.zeros((nt, T, 2), dtype=torch.float32, device="cuda")
    ops.rollout_deep(1, _layers(pol), pol.mean.weight.detach(), pol.mean.bias.detach(),
                     pol.log_std.detach(), init, noise, states, actions)
    return states, actions


def test_collect_particles_dispatches_deep_policy(cuda, monkeypatch):
    from mepol_amd.algorithms import mepol as M

    monkeypatch.delenv("MEPOL_ROLLOUT_FUSED", raising=False)
    env, pol = _gw_policy()
    nt, T = 6, 20
    S, A = _direct(env, pol, nt, T, 7)

    def collect():
        g = torch.Generator(device="cuda").manual_seed(7)
        return M.collect_particles_device(env, pol, nt, T, None, generator=g)

    st, ac, rtl, ns = collect()
    assert torch.equal(st, S) and torch.equal(ac, A)
    assert torch.equal(ns, S[:, 1:].reshape(-1, 2)) and bool((rtl == T).all())
    assert len(M._ROLLOUT_GRAPHS.get(pol, {})) == 0  # no graph was captured for it
    monkeypatch.setenv("MEPOL_ROLLOUT_FUSED", "0")
    st0, ac0, _, _ = collect()
    assert (ac0 - A).abs().max().item() < 1e-5
    assert (st0 - S).abs().max().item() < 1e-3


def test_deep_rollout_shards_concatenate(cuda, monkeypatch):
    from mepol_amd.algorithms import mepol as M

    monkeypatch.delenv("MEPOL_ROLLOUT_FUSED", raising=False)
    env, pol = _gw_policy()
    nt, T = 6, 20

    def collect(shard):
        g = torch.Generator(device="cuda").manual_seed(7)
        return M.collect_particles_device(env, pol, nt, T, None, generator=g, shard=shard)

    whole = collect(None)
    S, A = _direct(env, pol, nt, T, 7)
    assert torch.equal(whole[0], S) and torch.equal(whole[1], A)
    parts = [collect((r, 2)) for r in range(2)]
    for q in (0, 1, 3):
        assert torch.equal(torch.cat([p[q] for p in parts]), whole[q])


# ---- 6. get_heatmap --------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["MountainCar", "GridWorld"])
def test_get_heatmap_deep_policy(cuda, monkeypatch, env_name):
    """The heatmap of a deep policy (a rollout with `visited`) is served by the kernel and has
    the statistics of the per-step path (MEPOL_ROLLOUT_FUSED=0) on the same random stream."""
    from mepol_amd import ops
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.experiments.mepol import exp_specs
    from mepol_amd.policy import GaussianPolicy

    spec = exp_specs()[env_name]
    env = spec["env_create"]()
    disc = spec["discretizer_create"](env)
    torch.manual_seed(1)
    pol = GaussianPolicy([48, 40, 56], 2, env.action_space.shape[0], spec["log_std_init"]).cuda()
    calls = []
    real = ops.rollout_deep
    monkeypatch.setattr(ops, "rollout_deep", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def heatmap(fused):
        monkeypatch.setenv("MEPOL_ROLLOUT_FUSED", fused)
        torch.manual_seed(5)
        return M.get_heatmap(env, pol, disc, 6, 40, spec["heatmap_cmap"], spec["heatmap_interp"],
                             spec["heatmap_labels"])

    d1, h1, _ = heatmap("1")
    assert len(calls) == 1
    d0, h0, _ = heatmap("0")
    assert len(calls) == 1
    assert d1.shape == tuple(disc.bins_sizes) and abs(d1.sum() - 1.0) < 1e-12
    np.testing.assert_allclose(d1, d0, rtol=1e-14, atol=0)
    assert abs(h1 - h0) <= 1e-13 * max(abs(h0), 1.0)


# ---- 7. stale workspace ----------------------------------------------------------------------
def test_rollout_deep_stale_workspace(cuda):
    """The error-word header of the cached workspace is zeroed by every call: a workspace full
    of 0xff neither raises nor changes bits."""
    from mepol_amd import ops

    pol, _, init, noise = _case("gridworld", (70, 9, 66), 3, 12)
    ref = _run("gridworld", pol, init, noise)
    ws = ops._workspace(torch.device("cuda", 0), 1 << 20, tag="rollout")
    ws.fill_(0xFF)
    out = _run("gridworld", pol, init, noise)
    for x, y in zip(out, ref):
        assert torch.equal(x, y)
    assert int(ws[:256].max().item()) == 0 and int(ws[256:512].min().item()) == 0xFF
