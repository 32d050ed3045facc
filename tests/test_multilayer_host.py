"""Host side of the three-or-more-hidden-layer path: the C ABI of mepol_hidden_backward, the
optimizer's tensor limit and the CLI flag.  Nothing here launches a kernel."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "mepol_amd.h")
NEW = ["mepol_hidden_backward", "mepol_hidden_backward_workspace_size"]


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(mepol_[a-z0-9_]+)\s*\(", text))


def test_header_declares_hidden_backward():
    assert set(NEW) <= _declared()


def test_library_exports_hidden_backward():
    from mepol_amd import _lib

    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.mepol_abi_version() == 4


def test_workspace_size():
    from mepol_amd import _lib

    lib = _lib.load()
    small, big = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.mepol_hidden_backward_workspace_size(1, 2, ctypes.byref(small)) == 0
    assert small.value > 0
    assert lib.mepol_hidden_backward_workspace_size(200000, 400, ctypes.byref(big)) == 0
    assert big.value > small.value
    assert lib.mepol_hidden_backward_workspace_size(10, 4, None) == 1001


def test_hidden_backward_bad_arguments_fail_without_gpu():
    """Argument validation happens on the host before any launch: the pointers below are never
    dereferenced (they are not device memory)."""
    from mepol_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)  # 16-byte aligned
    nbytes = ctypes.c_size_t()
    assert lib.mepol_hidden_backward_workspace_size(4, 6, ctypes.byref(nbytes)) == 0
    ws = nbytes.value

    def run(n=4, out=4, inn=6, dz=p, W=p, h=p, dzin=p, db=p, wsp=p, wsb=ws):
        return lib.mepol_hidden_backward(dz, n, out, W, h, inn, dzin, db, wsp, wsb, None)

    for kw in (dict(inn=5), dict(out=3), dict(dz=None), dict(W=None), dict(h=None),
               dict(dzin=None), dict(wsp=None), dict(n=0), dict(inn=0), dict(out=0),
               dict(dz=ctypes.c_void_p(p.value + 8)), dict(W=ctypes.c_void_p(p.value + 8))):
        assert run(**kw) == 1001, kw
        msg = lib.mepol_last_error_string()
        assert b"mepol_hidden_backward" in msg and b"even" in msg, (kw, msg)
        assert b"16-B aligned" in msg
    # a short workspace is its own error, also before any launch
    assert run(wsb=ws - 1) == 1002
    assert b"workspace" in lib.mepol_last_error_string()


def test_optim_step_tensor_limit():
    """Up to 16 tensors (six hidden layers: 2 * 6 + 3 = 15); 17 is still a bad argument."""
    from mepol_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    a = ctypes.addressof(buf)
    for n, name in ((17, "mepol_optim_step"), (0, "mepol_optim_step")):
        arr = (ctypes.c_void_p * max(n, 1))(*([a] * max(n, 1)))
        sizes = (ctypes.c_int64 * max(n, 1))(*([1] * max(n, 1)))
        rc = getattr(lib, name)(0, n, arr, arr, arr, arr, sizes, ctypes.c_void_p(a), None)
        assert rc == 1001
        assert b"16 tensors" in lib.mepol_last_error_string()
    text = open(HEADER).read()
    assert "n_tensors (<= 16)" in text and "(<= 8)" not in text


def test_cli_hidden_sizes_flag():
    from mepol_amd.experiments.mepol import build_parser

    base = ["--env", "GridWorld", "--k", "4", "--kl_threshold", "15", "--learning_rate", "1e-4",
            "--num_trajectories", "2", "--trajectory_length", "10", "--num_epochs", "1",
            "--heatmap_episodes", "1", "--heatmap_num_steps", "5"]
    p = build_parser()
    assert p.parse_args(base).hidden_sizes is None
    assert p.parse_args(base + ["--hidden_sizes", "64", "48", "32"]).hidden_sizes == [64, 48, 32]


def test_multilayer_gate():
    from mepol_amd.policy import multilayer_ok

    assert multilayer_ok([64, 48, 32], 29) and multilayer_ok([72, 200, 50, 34, 2, 2], 64)
    assert not multilayer_ok([64, 48], 29)            # two layers: _TwoLayerLogp
    assert not multilayer_ok([64, 47, 32], 29)        # odd width
    assert not multilayer_ok([64, 48, 32], 65)        # input layer kernel: <= 64 features
    assert not multilayer_ok([2] * 7, 29)             # 2 * 7 + 3 > 16 optimizer tensors
