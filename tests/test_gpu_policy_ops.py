"""The Gaussian head, input layer and optimizer kernels op by op against 80-bit references.

Every case of tests/policy_cases.py goes through mepol_amd.ops (csrc/head.hip, csrc/mlp.hip,
csrc/optim.hip) with the same checkers that tests/test_policy_cases_host.py applies to the CPU
stand-ins: each output within m u0 A of the np.longdouble reference (the derivations are in
policy_cases.py).  The shapes are the smallest that reach each branch: every template
instantiation of the head's forward (49) and backward (32 narrow, 5 wide) at 37 rows, row counts
from 1 to 4100 (last groups of 1 to 3 rows, 1 to 33 partial records with empty record groups, odd
counts for the wide kernel's row pairs), both ends of the input layer's six feature bands with
last chunks of 1 to 63 rows and one batch in which a block stages two chunks, optimizer tensors
of 0 to 1024 x 256 + 1 elements in 1, 8, 9 and 16 tensors.  Every op runs twice, same bits.
"""
import pytest
import torch

import policy_cases as P

BZ = [True, False]
FWD_GROUPS, BWD_GROUPS = P.head_fwd_groups(), P.head_bwd_groups()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    return gpu_ops


def _same(a, b):
    for key in a:
        assert P.bits_equal(a[key], b[key]), key


@pytest.mark.parametrize("group", list(FWD_GROUPS))
def test_head_forward(cuda, ops, group):
    for name in FWD_GROUPS[group]:
        c = P.head_fwd_cases()[name]
        for with_bz in BZ:
            _same(P.run_head_forward(ops, cuda, c, with_bz),
                  P.run_head_forward(ops, cuda, c, with_bz))


@pytest.mark.parametrize("group", list(BWD_GROUPS))
def test_head_backward(cuda, ops, group):
    """One call, checked; need_dz=False, nan-filled outs= and ws=, reduce_stream= and
    defer_reduce=True with the one call's bits; the whole of it twice."""
    for name in BWD_GROUPS[group]:
        c = P.head_bwd_cases()[name]
        for with_bz in BZ:
            _same(P.run_head_backward(ops, cuda, c, with_bz, streams=True),
                  P.run_head_backward(ops, cuda, c, with_bz, streams=True))


@pytest.mark.parametrize("with_bz", BZ)
@pytest.mark.parametrize("name", P.HEAD_CHAIN)
def test_head_forward_then_backward(cuda, ops, name, with_bz):
    c = P.head_bwd_cases()[name]
    a, b = P.run_head_chain(ops, cuda, c, with_bz), P.run_head_chain(ops, cuda, c, with_bz)
    assert all(P.bits_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(P.layer_cases()))
def test_layer(cuda, ops, name):
    from mepol_amd._lib import call, ptr

    c = P.layer_cases()[name]
    a = P.run_layer(ops, cuda, c)
    _same(a, P.run_layer(ops, cuda, c))
    # db = NULL through the C entry point: the same dW, nothing else asked for
    ref = P.layer_reference(name)
    dh, h, x = (P._t(v, cuda) for v in (c.dh, ref.h, c.x))
    dW = torch.full((c.H, c.F), float("nan"), dtype=torch.float64, device=cuda)
    ws = ops.layer_workspace(c.n, c.F, c.H, cuda)
    call("mepol_layer_backward", ptr(dh), ptr(h), ptr(x), c.n, c.F, c.H, ptr(dW), None, ptr(ws),
         ws.numel(), ops._stream())
    assert P.bits_equal(dW, a["dW"])


@pytest.mark.parametrize("name", list(P.optim_cases()))
def test_optim_step(cuda, ops, name):
    """Bounds, snapshots and the scal[0] == 0 switch as P.run_optim states them; the kernel's
    bits also equal the one-rounding-per-op numpy restatement's (cpu_ops.optim_step), as
    measured on the MI355X (profiles/r13/policy_ops/README.md)."""
    c = P.optim_cases()[name]
    a = P.run_optim(ops, cuda, c)
    differ, compared = P.OPTIM_BITS[name]
    b = P.run_optim(ops, cuda, c)
    for la, lb in zip(a, b):
        assert all(P.bits_equal(x, y) for x, y in zip(la, lb))
    print(f"{name}: {differ} of {compared} elements differ in bits from the numpy restatement")
    assert differ == 0, "the kernel's bits differ from the numpy restatement of its op sequence"


# ---------------------------------------------------------------------------------------------
# host-side refusals: nothing is launched, nothing is written
# ---------------------------------------------------------------------------------------------
N, H, A, F = 8, 64, 2, 4
SENTINEL = -7.25


@pytest.fixture()
def bufs(cuda, ops):
    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float64, device=cuda)

    t = dict(z=full(N, H), bz=full(H), Wm=full(A, H), bm=full(A), ls=full(A), act=full(N, A),
             mu=full(N, A), logp=full(N), g=full(N), dz=full(N, H), dWm=full(A, H), dbm=full(A),
             dls=full(A), dbz=full(H), x=full(N, F), W=full(H, F), b=full(H), h=full(N, H),
             dh=full(N, H), dW=full(H, F), db=full(H))
    t["head_ws"] = ops.head_workspace(N, H, A, cuda)
    t["layer_ws"] = ops.layer_workspace(N, F, H, cuda)
    yield t
    torch.cuda.synchronize()
    for key, v in t.items():
        if v.dtype == torch.float64:
            assert bool((v == SENTINEL).all()), f"{key} was written"


def _head_fwd(t, n, hidden, a_dim, st):
    from mepol_amd._lib import call, ptr

    call("mepol_head_forward", ptr(t["z"]), n, hidden, ptr(t["bz"]), ptr(t["Wm"]), ptr(t["bm"]),
         ptr(t["ls"]), ptr(t["act"]), a_dim, ptr(t["mu"]), ptr(t["logp"]), st)


def _head_bwd(t, n, hidden, a_dim, st, phase=None, ws_bytes=None):
    from mepol_amd._lib import call, ptr

    ws = t["head_ws"]
    args = (ptr(t["g"]), ptr(t["z"]), n, hidden, ptr(t["bz"]), ptr(t["Wm"]), ptr(t["ls"]),
            ptr(t["act"]), ptr(t["mu"]), a_dim, ptr(t["dz"]), ptr(t["dWm"]), ptr(t["dbm"]),
            ptr(t["dls"]), ptr(t["dbz"]), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes)
    if phase is None:
        call("mepol_head_backward", *args, st)
    else:
        call("mepol_head_backward_phase", *args, phase, st)


def _layer_fwd(t, n, f, st):
    from mepol_amd._lib import call, ptr

    call("mepol_layer_forward", ptr(t["x"]), n, f, ptr(t["W"]), ptr(t["b"]), H, ptr(t["h"]), st)


def _layer_bwd(t, n, f, st, ws_bytes=None):
    from mepol_amd._lib import call, ptr

    ws = t["layer_ws"]
    call("mepol_layer_backward", ptr(t["dh"]), ptr(t["h"]), ptr(t["x"]), n, f, H, ptr(t["dW"]),
         ptr(t["db"]), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, st)


def test_sizes_past_the_kernels_limits_are_refused(cuda, ops, bufs):
    from mepol_amd._lib import MepolInputError

    st = ops._stream()
    for hidden, a_dim in ((513, A), (H, 33)):
        with pytest.raises(MepolInputError):
            _head_fwd(bufs, N, hidden, a_dim, st)
        with pytest.raises(MepolInputError):
            _head_bwd(bufs, N, hidden, a_dim, st)
        with pytest.raises(MepolInputError):
            _head_bwd(bufs, N, hidden, a_dim, st, phase=1)
    with pytest.raises(MepolInputError):
        _layer_fwd(bufs, N, 65, st)
    with pytest.raises(MepolInputError):
        _layer_bwd(bufs, N, 65, st)


def test_head_backward_phase_takes_1_or_2_only(cuda, ops, bufs):
    from mepol_amd._lib import MepolInputError

    for phase in (0, 3):
        with pytest.raises(MepolInputError):
            _head_bwd(bufs, N, H, A, ops._stream(), phase=phase)


def test_a_workspace_one_byte_short_is_refused(cuda, ops, bufs):
    from mepol_amd._lib import MepolError, MepolInputError

    st = ops._stream()
    for fn, args, key in ((_head_bwd, (N, H, A), "head_ws"), (_layer_bwd, (N, F), "layer_ws")):
        need = bufs[key].numel()
        assert need == ops._ws_bytes(key[:-3], N, *((H, A) if key == "head_ws" else (F, H)))
        with pytest.raises(MepolError, match="rc=1002") as err:
            fn(bufs, *args, st, ws_bytes=need - 1)
        assert not isinstance(err.value, MepolInputError)


def test_zero_rows(cuda, ops, bufs):
    """n = 0: the forwards succeed and write nothing; the backwards refuse it (bad argument), as
    they do today: their outputs are sums over rows, and they write none."""
    from mepol_amd._lib import MepolInputError

    st = ops._stream()
    _head_fwd(bufs, 0, H, A, st)
    _layer_fwd(bufs, 0, F, st)
    with pytest.raises(MepolInputError):
        _head_bwd(bufs, 0, H, A, st)
    with pytest.raises(MepolInputError):
        _layer_bwd(bufs, 0, F, st)
