"""Truth table of the gates that decide whether a policy and a batch take the HIP kernels:

    head    GaussianPolicy._fused_head_ok(states, actions)
    multi   policy.multilayer_ok(hidden widths, features)
    fvp     trpo.fvp_kernels_ok(policy, states)
    sup     device_loop.supported(batch, behavioral, target, optimizer)
    supm    device_loop.supported_multilayer(batch, behavioral, target, optimizer)
    rmlp    mepol._rollout_mlp_layers(policy, features, actions) is not None
    rdeep   mepol._rollout_deep_layers(policy, features, actions) is not None

and the two row floors, policy.fused_min_rows() and trpo.fvp_min_rows().  No kernel under test
is launched: the gates only look at shapes, dtypes, devices and the environment.

Every answer is written out below, not computed from the package's constants; they are the
answers the gates gave before they shared one module.  Rows are one-factor variations around
the base (f64 ReLU [64, 48], 3 features, 2 actions, 512 rows on the device); the rollout gates
want 2 features, so their rows vary around the same base with 2 features.  The batch of sup /
supm is loop_runs._setup's at NT = 4, T = 128 (512 rows, as tests/test_gpu_loop_launch_order.py
builds it), so rows with another row count or dtype leave those two columns out ("-")."""
import numpy as np
import pytest
import scipy.special
import torch
import torch.nn as nn

from loop_runs import _setup

pytestmark = pytest.mark.gpu

COLUMNS = ("head", "multi", "fvp", "sup", "supm", "rmlp", "rdeep")
ENV = ("MEPOL_FUSED_MIN_ROWS", "MEPOL_FVP_MIN_ROWS", "MEPOL_ROLLOUT_FUSED",
       "MEPOL_ROLLOUT_DEEP_MAX_WORDS", "MEPOL_DEVICE_LOOP")
BASE = dict(hidden=[64, 48], nf=3, a=2, act=nn.ReLU, dtype=torch.float64, rows=512, env={},
            opt="adam", same=False, floors=(500, 500))
WIDE = [512, 512, 512, 8]  # 512 * 512 + 512 * 512 + 512 * 8 = 528384 weight words behind layer 1


def _row(answers, **changes):
    assert len(answers) == len(COLUMNS) and set(changes) <= set(BASE)
    return dict(BASE, **changes), answers


# id: (changes to BASE, answers in COLUMNS' order: T, F or - (not asked))
TABLE = {
    "base": _row("TFTTFFF"),
    # hidden widths
    "hidden-64": _row("TFFFFFF", hidden=[64]),
    "hidden-64-47": _row("TFFTFFF", hidden=[64, 47]),
    "hidden-63-48": _row("TFFTFFF", hidden=[63, 48]),
    "hidden-64-514": _row("FFFFFFF", hidden=[64, 514]),
    "hidden-514-64": _row("TFFTFFF", hidden=[514, 64]),
    "hidden-64-48-32": _row("TTTFTFF", hidden=[64, 48, 32]),
    "hidden-64-47-32": _row("TFFFFFF", hidden=[64, 47, 32]),
    "hidden-2x6": _row("TTTFTFF", hidden=[2] * 6),
    "hidden-2x7": _row("TFFFFFF", hidden=[2] * 7),
    # input features
    "nf-2": _row("TFTTFTF", nf=2),
    "nf-64": _row("TFTTFFF", nf=64),
    "nf-65": _row("TFFFFFF", nf=65),
    # actions
    "a-8": _row("TFTTFFF", a=8),
    "a-9": _row("TFTTFFF", a=9),
    "a-32": _row("TFTTFFF", a=32),
    "a-33": _row("FFFFFFF", a=33),
    # activation, dtype of the states
    "tanh": _row("FFFFFFF", act=nn.Tanh),
    "states-f32": _row("FFF--FF", dtype=torch.float32),
    # rows against the two floors
    "rows-499": _row("FFF--FF", rows=499),
    "rows-500": _row("TFT--FF", rows=500),
    "fused-floor-600": _row("FFTFFFF", env={"MEPOL_FUSED_MIN_ROWS": "600"}, floors=(600, 500)),
    "fvp-floor-600": _row("TFFTFFF", env={"MEPOL_FVP_MIN_ROWS": "600"}, floors=(500, 600)),
    # the graph loop's own conditions
    "sgd": _row("TFTFFFF", opt="sgd"),
    "sgd-deep": _row("TTTFFFF", hidden=[64, 48, 32], opt="sgd"),
    "target-is-behavioral": _row("TFTFFFF", same=True),
    "target-is-behavioral-deep": _row("TTTFFFF", hidden=[64, 48, 32], same=True),
    "device-loop-off": _row("TFTFFFF", env={"MEPOL_DEVICE_LOOP": "0"}),
    "device-loop-off-deep": _row("TTTFFFF", hidden=[64, 48, 32], env={"MEPOL_DEVICE_LOOP": "0"}),
    # the rollout gates: 2 features
    "rollout-deep": _row("TTTFTFT", nf=2, hidden=[64, 48, 32]),
    "rollout-odd-deep": _row("TFFFFFT", nf=2, hidden=[64, 47, 32]),
    "rollout-514-64": _row("TFFTFFF", nf=2, hidden=[514, 64]),
    "rollout-a-8": _row("TFTTFTF", nf=2, a=8),
    "rollout-a-9": _row("TFTTFFF", nf=2, a=9),
    "rollout-deep-a-9": _row("TTTFTFF", nf=2, a=9, hidden=[64, 48, 32]),
    "rollout-off": _row("TFTTFFF", nf=2, env={"MEPOL_ROLLOUT_FUSED": "0"}),
    "rollout-off-deep": _row("TTTFTFF", nf=2, hidden=[64, 48, 32],
                             env={"MEPOL_ROLLOUT_FUSED": "0"}),
    "rollout-wide-default-cap": _row("TTTFTFF", nf=2, hidden=WIDE),  # 528384 > 2 * 512 * 512
    "rollout-wide-cap-below": _row("TTTFTFF", nf=2, hidden=WIDE,
                                   env={"MEPOL_ROLLOUT_DEEP_MAX_WORDS": "528383"}),
    "rollout-wide-cap-equal": _row("TTTFTFT", nf=2, hidden=WIDE,
                                   env={"MEPOL_ROLLOUT_DEEP_MAX_WORDS": "528384"}),
}


def test_every_gate_answers_both_ways():
    for c, name in enumerate(COLUMNS):
        seen = {answers[c] for _, answers in TABLE.values()}
        assert {"T", "F"} <= seen, name
    assert {spec["floors"] for spec, _ in TABLE.values()} == {(500, 500), (600, 500), (500, 600)}


def _answers(spec, with_loop):
    """The gates' answers for one row, in COLUMNS' order ("-" where the row leaves one out)."""
    from mepol_amd import policy as P
    from mepol_amd.algorithms import device_loop, trpo
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.policy import GaussianPolicy

    hidden, nf, a = spec["hidden"], spec["nf"], spec["a"]
    dev = torch.device("cuda")
    if with_loop:
        cfg = dict(NT=4, T=128, NF=nf, A=a, K=4, HID=hidden, activation=spec["act"])
        _, _, beh, tgt, _, opt, (st, ac, rl, _, D, I) = _setup("adam", 1e-3, cfg=cfg)
        batch = M.P.lookup(st, ac, rl, D, I)
        assert batch.N == 512
        if spec["opt"] == "sgd":
            opt = torch.optim.SGD(tgt.parameters(), lr=1e-3)
        if spec["same"]:
            beh = tgt
        loop = [device_loop.supported(batch, beh, tgt, opt),
                device_loop.supported_multilayer(batch, beh, tgt, opt)]
    else:
        torch.manual_seed(5)
        tgt = GaussianPolicy(hidden, nf, a, activation=spec["act"]).to(dev)
        loop = ["-", "-"]
    states = torch.zeros((spec["rows"], nf), dtype=spec["dtype"], device=dev)
    actions = torch.zeros((spec["rows"], a), dtype=torch.float64, device=dev)
    got = ([tgt._fused_head_ok(states, actions), P.multilayer_ok(hidden, nf),
            trpo.fvp_kernels_ok(tgt, states)] + loop
           + [M._rollout_mlp_layers(tgt, nf, a) is not None,
              M._rollout_deep_layers(tgt, nf, a) is not None])
    assert all(g == "-" or isinstance(g, bool) for g in got), got
    return "".join(g if g == "-" else "FT"[g] for g in got), (P.fused_min_rows(),
                                                               trpo.fvp_min_rows())


@pytest.mark.parametrize("name", list(TABLE))
def test_gate_truth_table(cuda, monkeypatch, name):
    spec, expected = TABLE[name]
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    for var, value in spec["env"].items():
        monkeypatch.setenv(var, value)
    got, floors = _answers(spec, with_loop=expected[3] != "-")
    print(name, dict(zip(COLUMNS, got)), floors)
    assert got == expected
    assert floors == spec["floors"]


@pytest.mark.parametrize("hidden,cls", [([64, 48], "DeviceIteration"),
                                        ([64, 48, 32], "MultiLayerIteration")],
                         ids=["two-layer", "deep3"])
def test_iteration_class(cuda, monkeypatch, hidden, cls):
    from mepol_amd.algorithms import device_loop

    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    cfg = dict(NT=4, T=128, NF=3, A=2, K=4, HID=hidden)
    M, _, _, tgt, _, opt, (st, ac, rl, _, D, I) = _setup("adam", 1e-3, cfg=cfg)
    batch = M.P.lookup(st, ac, rl, D, I)
    G = float(scipy.special.gamma(3 / 2 + 1))
    B = float(np.log(4) - scipy.special.digamma(4))
    it = device_loop.get(tgt, opt, batch, 4, G, B, 3, 0.0)
    assert type(it).__name__ == cls
