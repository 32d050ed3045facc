"""Host side of the one-launch rollout for 3 to 6 hidden layers: the C ABI of mepol_rollout_deep
and the rule that sends a policy to it.  Nothing here launches a kernel or needs a GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "mepol_amd.h")
NEW = ["mepol_rollout_deep", "mepol_rollout_deep_workspace_size"]


def test_header_declares_rollout_deep():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert set(NEW) <= set(re.findall(r"\b(mepol_[a-z0-9_]+)\s*\(", text))


def test_library_exports_rollout_deep():
    from mepol_amd import _lib

    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.mepol_abi_version() == 4


def _widths(ws):
    return (ctypes.c_int * len(ws))(*ws)


def _run(lib, env_id=0, widths=(8, 8, 8), a_dim=1, n=4, T=3, null=None):
    """mepol_rollout_deep on host memory: a call that passes validation would launch, so every
    call here is one that must be rejected (or returns before the launch)."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    names = ["W1", "b1", "Wt", "bt", "Wm", "bm", "log_std", "init64", "init32", "noise",
             "states_rec", "actions_rec"]
    a = {k: (None if k == null else p) for k in names}
    return lib.mepol_rollout_deep(env_id, len(widths), _widths(widths), a["W1"], a["b1"], a["Wt"],
                                  a["bt"], a["Wm"], a["bm"], a["log_std"], a_dim, a["init64"],
                                  a["init32"], a["noise"], n, T, a["states_rec"],
                                  a["actions_rec"], None, None, None, 0, None)


BAD = [dict(widths=(8, 8)), dict(widths=(8,) * 7), dict(widths=(8, 0, 8)), dict(widths=(8, 513, 8)),
       dict(widths=(513, 8, 8)), dict(a_dim=9), dict(a_dim=0), dict(env_id=1, a_dim=1),
       dict(env_id=2), dict(null="W1"), dict(null="Wt"), dict(null="bt"), dict(null="noise"),
       dict(null="init64"), dict(env_id=1, a_dim=2, null="init32"), dict(null="actions_rec")]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in BAD])
def test_rollout_deep_bad_arguments_fail_without_gpu(kw):
    """Validation happens on the host before any launch: the pointers are host memory and are
    never dereferenced, and no device is needed.  The text names the limits."""
    from mepol_amd import _lib

    lib = _lib.load()
    assert _run(lib, **kw) == 1001, kw
    msg = lib.mepol_last_error_string()
    assert b"mepol_rollout_deep" in msg, msg
    for limit in (b"3 <= n_hidden <= 6", b"width <= 512", b"a_dim <= 8", b"GridWorld a_dim = 2"):
        assert limit in msg, (limit, msg)


def test_rollout_deep_empty_batch_returns_before_launch():
    from mepol_amd import _lib

    lib = _lib.load()
    assert _run(lib, n=0) == 0
    assert _run(lib, T=0) == 0


def test_rollout_deep_workspace_size():
    from mepol_amd import _lib

    lib = _lib.load()
    nbytes = ctypes.c_size_t()
    size = lib.mepol_rollout_deep_workspace_size
    assert size(20, 1200, 3, _widths((300, 300, 300)), 2, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 256
    assert size(0, 0, 6, _widths((512,) * 6), 8, ctypes.byref(nbytes)) == 0 and nbytes.value == 256
    assert size(20, 1200, 3, _widths((300, 300, 300)), 2, None) == 1001
    assert size(20, 1200, 2, _widths((300, 300)), 2, ctypes.byref(nbytes)) == 1001
    assert size(20, 1200, 3, _widths((300, 513, 300)), 2, ctypes.byref(nbytes)) == 1001
    assert b"width <= 512" in lib.mepol_last_error_string()
    # a short workspace is its own error, also before any launch
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    rc = lib.mepol_rollout_deep(0, 3, _widths((8, 8, 8)), p, p, p, p, p, p, p, 1, p, None, p, 4, 3,
                                p, p, None, None, p, 255, None)
    assert rc == 1002 and b"workspace" in lib.mepol_last_error_string()


def test_deep_rollout_eligibility(monkeypatch):
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.delenv("MEPOL_ROLLOUT_FUSED", raising=False)

    def deep(hidden, nf=2, a=2, **kw):
        return M._rollout_deep_layers(GaussianPolicy(hidden, nf, a, **kw), nf, a)

    monkeypatch.delenv("MEPOL_ROLLOUT_DEEP_MAX_WORDS", raising=False)
    for hidden in ([300, 300, 300], [71, 9, 65], [512] * 3, [400, 300, 300], [300] * 6):
        lin = deep(hidden)
        assert lin is not None and [W.shape[0] for W, _ in lin] == hidden
        assert all(b.shape == (W.shape[0],) for W, b in lin) and lin[0][0].shape[1] == 2
    assert deep([300, 300]) is None          # two layers: the two-layer kernel's
    assert M._rollout_mlp_layers(GaussianPolicy([300, 300], 2, 2), 2, 2) is not None
    assert M._rollout_mlp_layers(GaussianPolicy([64, 48, 32], 2, 2), 2, 2) is None
    assert deep([8] * 7) is None
    assert deep([64, 513, 64]) is None
    assert deep([64, 48, 32], activation=nn.Tanh) is None
    assert deep([64, 48, 32], dtype=torch.float32) is None
    assert deep([64, 48, 32], nf=3) is None
    assert deep([64, 48, 32], a=9) is None
    # the measured cap on the weight words streamed per step: sum h_{l-1} h_l <= 2 * 512^2
    assert M.ROLLOUT_DEEP_MAX_WORDS == 2 * 512 * 512
    assert deep([512] * 4) is None and deep([384] * 6) is None and deep([512, 512, 513]) is None
    monkeypatch.setenv("MEPOL_ROLLOUT_DEEP_MAX_WORDS", str(1 << 30))
    assert deep([512] * 6) is not None
    monkeypatch.delenv("MEPOL_ROLLOUT_DEEP_MAX_WORDS")
    monkeypatch.setenv("MEPOL_ROLLOUT_FUSED", "0")
    for hidden in ([300, 300, 300], [71, 9, 65]):
        assert deep(hidden) is None
