"""The launch list of one body of the graph-replayed iteration (algorithms/device_loop.py):
which mepol_amd.ops calls it makes, in which order and on which of its streams.  The other loop
tests compare results, which stay the same when a kernel moves to another stream or two launches
swap; the iteration's time does not.

The lists are written out here, not derived from the code under test: a change that needs one
of them edited changes the iteration's schedule and wants a timing of the loop beside it.  The
deep forward asks ops.gemm_nt_variant for its tiling before each ops.gemm_nt: a host-side helper,
recorded like every other ops call."""
import numpy as np
import pytest
import scipy.special
import torch

from loop_runs import _setup

pytestmark = pytest.mark.gpu

# N = 512 rows, just over policy.FUSED_MIN_ROWS
SHAPE = dict(NT=4, T=128, NF=3, A=2, K=4)


def _main(*names):
    return [(n, "main") for n in names]


HEAD = _main("memcpy_async", "entropy_gamma", "entropy_reverse_scan", "head_backward")
TAIL = _main("iw_forward", "entropy_forward", "memcpy_async")

FUSED = (HEAD + [("weight_grad", "fork"), ("dh1_layer1_backward", "gemm")]
         + _main("optim_step", "policy_forward") + TAIL)
# the two torch.mm calls (dh1 and z2) are not ops calls
UNFUSED = (HEAD + [("weight_grad", "fork"), ("layer_backward", "gemm")]
           + _main("optim_step", "layer_forward", "head_forward") + TAIL)
# L = 4: the smallest depth at which a dz_buf slot is reused and the read_done wait runs
DEEP4 = (HEAD + 3 * [("weight_grad", "fork"), ("hidden_backward", "main")]
         + _main("layer_backward", "optim_step", "layer_forward")
         + 3 * _main("gemm_nt_variant", "gemm_nt") + _main("head_forward") + TAIL)


class _Recorder:
    """Stands in for the name `ops` of the device_loop and kernel_path modules: calls made
    through it are noted with the stream they were issued on; calls ops functions make to each
    other are not."""

    def __init__(self, ops, it, calls):
        self._ops, self._it, self._calls = ops, it, calls

    def __getattr__(self, name):
        real = getattr(self._ops, name)
        if not callable(real):
            return real

        def wrapper(*args, **kw):
            s = torch.cuda.current_stream()
            role = ("fork" if s == self._it.fork else
                    "gemm" if s == getattr(self._it, "s_gemm", None) else "main")
            self._calls.append((name, role))
            return real(*args, **kw)

        return wrapper


@pytest.mark.parametrize("hid,fused,cls,expected", [
    ([64, 48], "1", "DeviceIteration", FUSED),
    ([64, 48], "0", "DeviceIteration", UNFUSED),
    ([64, 48, 32, 16], "1", "MultiLayerIteration", DEEP4),
], ids=["two-layer-fused", "two-layer-unfused", "deep4"])
def test_body_launch_list(cuda, monkeypatch, hid, fused, cls, expected):
    from mepol_amd import kernel_path, ops
    from mepol_amd.algorithms import device_loop

    monkeypatch.delenv("MEPOL_FUSED_MIN_ROWS", raising=False)
    monkeypatch.setenv("MEPOL_DEVICE_LOOP", "1")
    monkeypatch.setenv("MEPOL_FUSED_FWD", fused)
    monkeypatch.setenv("MEPOL_FUSED_DH1", fused)
    cfg = dict(SHAPE, HID=hid)
    NF, K = cfg["NF"], cfg["K"]
    M, _, beh, tgt, _, opt, (st, ac, rl, _, D, I) = _setup("adam", 1e-3, cfg=cfg)
    batch = M.P.lookup(st, ac, rl, D, I)
    gate = device_loop.supported if len(hid) == 2 else device_loop.supported_multilayer
    assert batch.N == 512 and gate(batch, beh, tgt, opt)
    G = float(scipy.special.gamma(NF / 2 + 1))
    B = float(np.log(K) - scipy.special.digamma(K))
    it = device_loop.get(tgt, opt, batch, K, G, B, NF, 0.0)
    assert type(it).__name__ == cls
    if len(hid) == 2:
        assert (it.fused_fwd, it.fused_dh1) == (fused == "1", fused == "1")
    it.load(batch)
    it.start_from_behavioral()
    theta = [p.detach().clone() for p in tgt.parameters()]

    calls = []
    recorder = _Recorder(ops, it, calls)
    monkeypatch.setattr(device_loop, "ops", recorder)
    monkeypatch.setattr(kernel_path, "ops", recorder)  # the deep forward's chain is made there
    it._warmup()  # one eager body on the side stream, enable flag 0
    torch.cuda.synchronize()

    print(calls)
    assert calls == expected
    assert all(torch.equal(p, q) for p, q in zip(tgt.parameters(), theta))
