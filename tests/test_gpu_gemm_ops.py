"""The f64 matrix-core GEMM kernels op by op against 80-bit references.

Every case of tests/gemm_cases.py goes through mepol_amd.ops (csrc/gemm.hip, csrc/wgrad.hip,
csrc/policy_fwd.hip) with the same checkers that tests/test_gemm_cases_host.py applies to the CPU
stand-ins: each output within m u0 A of the np.longdouble reference (the derivations are in
gemm_cases.py), non-finite values exactly where the reference has them.  The shapes are the
smallest that reach each path: all ten gemm_nt tilings at 257 x 18 x 401 (two row blocks, a ragged
last column block, a k tail of 2) with the bias / ReLU epilogue and with strided operands and
output; every FP band of policy_forward in its five forms, the one-kernel form with a misaligned
h1_out among them; NH 1 to 4, 1 to 4 k-tiles, 1 to 17 row blocks of the two DEEP-loop kernels in
their three forms; fol 1 to 4 of the weight gradient with empty K-slices and an uneven plan.  Every
case runs twice, same bits.
"""
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    return gpu_ops


@pytest.mark.parametrize("family,group", G.family_groups())
def test_cases(cuda, ops, family, group):
    G.run_group(ops, cuda, family, group, twice=True)


def _hb_raw(ops, cuda, dz_out, W, h_in, dz, db, ws, ws_bytes=None):
    from mepol_amd._lib import call, ptr

    n, k = dz_out.shape
    call("mepol_hidden_backward", ptr(dz_out), n, k, ptr(W), ptr(h_in), W.shape[1], ptr(dz),
         ptr(db), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, ops._stream())


@pytest.mark.parametrize("name", [f"n{n}_unit" for n in G.DEEP_N] + ["M2_work", "K50_unit"])
def test_hidden_backward_without_db(cuda, ops, name):
    """db_in = NULL through the C entry point: the same dz_in, no record is written."""
    c = G.hb_cases()[name]
    want = G.run_hidden_backward(ops, cuda, c)
    dz_out, W, h_in = (G._t(v, cuda) for v in (c.dz_out, c.W, c.h_in))
    ws = ops.hidden_backward_workspace(c.n, c.M, cuda)
    ws.fill_(0x7F)
    dz = G._nan((c.n, c.M), cuda)
    _hb_raw(ops, cuda, dz_out, W, h_in, dz, None, ws)
    assert G.bits_equal(dz, want["dz"])
    assert bool((ws == 0x7F).all()), "the workspace was written without a db_in"


# ---------------------------------------------------------------------------------------------
# host-side refusals: nothing is launched, nothing is written
# ---------------------------------------------------------------------------------------------
N, K, M, F, A = 8, 6, 10, 4, 2


@pytest.fixture()
def bufs(cuda, ops):
    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float64, device=cuda)

    t = dict(a=full(N, K + 2), b=full(M, K + 2), c=full(N, M), bias=full(M), dz2=full(N, K),
             W2t=full(M, K), h1=full(N, M), x=full(N, 64), dW1=full(M, 64), db1=full(M),
             dy=full(N, M), dW=full(M, F), W=full(K, M), dz=full(N, M), db=full(M),
             x11=full(N, F), W1=full(11, F), b1=full(11), W2=full(M, 11), b2=full(M),
             Wm=full(A, M), bm=full(A), ls=full(A), act=full(N, A), h1o=full(N, 11),
             z2=full(N, M), mu=full(N, A), logp=full(N))
    yield t
    torch.cuda.synchronize()
    for key, v in t.items():
        assert bool((v == SENTINEL).all()), f"{key} was written"


def _gemm(ops, t, A_, k, lda, ldb=K + 2, ldc=M):
    from mepol_amd._lib import call, ptr

    call("mepol_gemm_nt", A_, N, k, lda, ptr(t["b"]), M, ldb, ptr(t["bias"]), 1, ptr(t["c"]),
         ldc, 0, ops._stream())


def test_gemm_nt_refuses_odd_k_short_strides_and_a_misaligned_operand(cuda, ops, bufs):
    import ctypes

    from mepol_amd._lib import MepolInputError, ptr

    a = ptr(bufs["a"])
    _gemm_ok = (a, K, K + 2)
    for args in ((a, K - 1, K + 2),                  # odd k
                 (a, K, K - 2),                      # lda < k
                 (a, K, K + 1),                      # odd lda
                 (ctypes.c_void_p(bufs["a"].data_ptr() + 8), K, K + 2)):  # A not 16-B aligned
        assert args != _gemm_ok
        with pytest.raises(MepolInputError):
            _gemm(ops, bufs, *args)
    with pytest.raises(MepolInputError):
        _gemm(ops, bufs, a, K, K + 2, ldb=K - 2)
    with pytest.raises(MepolInputError):
        _gemm(ops, bufs, a, K, K + 2, ldc=M - 1)
    with pytest.raises(MepolInputError):
        ops.hidden_tangent(bufs["dz2"], bufs["dz2"], bufs["W2t"], bufs["W2t"], bufs["bias"],
                           bufs["c"], out=bufs["dz"], variant=4)


def test_dh1_refuses_64_input_features(cuda, ops, bufs):
    from mepol_amd._lib import MepolInputError

    t = bufs
    ws = ops.dh1_layer1_workspace(N, M, 64, cuda)
    mask = ops.h1_mask_buffer(N, M, cuda)
    for kw in (dict(), dict(mask=mask), dict(mask=mask, w2=t["W2t"].t().contiguous())):
        with pytest.raises(MepolInputError):
            ops.dh1_layer1_backward(t["dz2"], t["W2t"], t["h1"], t["x"], ws=ws, dW_out=t["dW1"],
                                    db_out=t["db1"], **kw)


def test_policy_forward_refuses_a_short_tile_with_an_odd_hidden0(cuda, ops, bufs):
    from mepol_amd._lib import MepolError

    t = bufs
    for tile in (32, 16, 8):
        with pytest.raises(MepolError):
            ops.policy_forward(t["x11"], t["W1"], t["b1"], t["W2"], t["b2"], t["Wm"], t["bm"],
                               t["ls"], t["act"], h1_out=t["h1o"], z2_out=t["z2"], mu_out=t["mu"],
                               logp_out=t["logp"], row_tile=tile)


def test_a_workspace_one_byte_short_is_refused(cuda, ops, bufs):
    from mepol_amd._lib import MepolError, MepolInputError, call, ptr

    t, st = bufs, ops._stream()
    big = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)

    def wgrad(nbytes):
        call("mepol_weight_grad", ptr(t["dy"]), N, M, ptr(t["x11"]), F, ptr(t["dW"]), ptr(big),
             nbytes, st)

    def dh1(nbytes):
        call("mepol_dh1_layer1_backward", ptr(t["dz2"]), N, K, ptr(t["W2t"]), M, ptr(t["h1"]),
             ptr(t["x11"]), F, ptr(t["dW"]), ptr(t["db1"]), ptr(big), nbytes, st)

    def hbw(nbytes):
        _hb_raw(ops, cuda, t["dz2"], t["W"], t["h1"], t["dz"], t["db"], big, ws_bytes=nbytes)

    for fn, op, sizes in ((wgrad, "weight_grad", (N, M, F)), (dh1, "dh1_layer1", (N, M, F)),
                          (hbw, "hidden_backward", (N, M))):
        need = ops._ws_bytes(op, *sizes)
        assert 0 < need <= big.numel()
        with pytest.raises(MepolError, match="rc=1002") as err:
            fn(need - 1)
        assert not isinstance(err.value, MepolInputError)
