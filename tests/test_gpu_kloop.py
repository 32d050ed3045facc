"""The f64 MFMA K loops (csrc/mfma_f64.hpp ring_k_loop with its pinned issue order, csrc/gemm.hip
gemm_mainloop): every branch of the loops -- no steady-state round, one round, ragged last
k-step / k-tile, empty K-slices -- against torch f64 on the device, and the same bits on every
call."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


# ---- ring_k_loop through wgrad_kernel -------------------------------------------------------
# (n, out, in); slices_for gives 8 K-slices at all of them:
#   (2048, 300, 400)  256 rows per slice, whole k-steps only
#   (2051, 300, 400)  a ragged last k-step in every slice
#   (31, 17, 33)      slices of 4 rows: one k-step each (less than one steady-state round),
#                     clamped columns, a last slice of 3 rows
#   (5, 16, 16)       two k-steps in all; the slices past the data are empty and write zeros
WGRAD_SHAPES = [(2048, 300, 400), (2051, 300, 400), (31, 17, 33), (5, 16, 16)]


@pytest.mark.parametrize("n,o,i", WGRAD_SHAPES)
def test_weight_grad_ring_branches(cuda, n, o, i):
    from mepol_amd import ops

    g = torch.Generator(device="cuda").manual_seed(n + o + i)
    dy = torch.randn((n, o), dtype=torch.float64, device="cuda", generator=g)
    x = torch.randn((n, i), dtype=torch.float64, device="cuda", generator=g)
    ws_probe = ops.weight_grad_workspace(n, o, i, dy.device)
    assert ws_probe.numel() == 8 * o * i * 8, "the shapes are chosen for 8 K-slices"
    ref = dy.t() @ x
    out = ops.weight_grad(dy, x)
    err = (out - ref).abs().max().item()
    bound = 1e-10 * ref.abs().max().item()
    print(f"weight_grad {(n, o, i)}: max err {err:.3e} (bound {bound:.3e})")
    assert out.shape == (o, i)
    assert err <= bound
    assert torch.equal(ops.weight_grad(dy, x), out)
    ws = ops.weight_grad_workspace(n, o, i, dy.device)
    ws.fill_(0x7F)  # stale scratch must not show in the result
    assert torch.equal(ops.weight_grad(dy, x, ws=ws), out)


# ---- gemm_mainloop --------------------------------------------------------------------------
# K = 16: one k-tile; 32: two (DEEP: one double phase, no steady-state round); 34: an even
# ragged tail (three tiles: a double phase and the odd last tile); 300: many rounds and a
# ragged tail.  300 rows: two 256-row blocks of the DEEP kernels, the second ragged; 77: one.
KS = [16, 32, 34, 300]
ROWS = [300, 77]
H0, NF = 96, 5  # dh1: two 80-column tiles (the second ragged); hidden: M = 96 likewise


@functools.lru_cache(maxsize=None)
def _case(n, k):
    g = torch.Generator(device="cuda").manual_seed(1000 * n + k)
    kw = dict(dtype=torch.float64, device="cuda", generator=g)
    dz = torch.randn(n, k, **kw)
    W = torch.randn(k, H0, **kw) * 0.1          # the Linear weight as stored: [out = k][in = H0]
    h = torch.relu(torch.randn(n, H0, **kw))    # about half of the mask is off
    x = torch.randn(n, NF, **kw)
    dzin = (dz @ W) * (h > 0)
    return dz, W, h, x, dzin, dzin.t() @ x, dzin.sum(0)


def _mask_words(h):
    n, h0 = h.shape
    words = (h0 + 15) // 16
    pos = torch.nn.functional.pad(h > 0, (0, words * 16 - h0)).view(n, words, 16)
    v = (pos.to(torch.int32) << torch.arange(16, device=h.device, dtype=torch.int32)).sum(-1)
    return ((v + 32768) % 65536 - 32768).to(torch.int16).contiguous()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ROWS)
def test_dh1_layer1_backward_k_tiles(cuda, n, k):
    from mepol_amd import ops

    dz, W, h, x, _, ref_dW, ref_db = _case(n, k)
    Wt = W.t().contiguous()
    dW, db = ops.dh1_layer1_backward(dz, Wt, h, x)
    print(f"dh1 n={n} K={k}: dW err {(dW - ref_dW).abs().max().item():.3e}, "
          f"db err {(db - ref_db).abs().max().item():.3e}")
    torch.testing.assert_close(dW, ref_dW, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(db, ref_db, rtol=1e-11, atol=1e-11)
    # the masked form and the form that reads W2 as stored: the same bits, on every call
    mask = ops.h1_mask_buffer(n, H0, x.device)
    mask.copy_(_mask_words(h))
    ws = ops.dh1_layer1_workspace(n, H0, NF, x.device)
    for _ in range(2):
        dWm, dbm = ops.dh1_layer1_backward(dz, Wt, h, x, mask=mask)
        dWw, dbw = ops.dh1_layer1_backward(dz, None, h, x, mask=mask, w2=W, ws=ws)
        assert torch.equal(dW, dWm) and torch.equal(db, dbm)
        assert torch.equal(dW, dWw) and torch.equal(db, dbw)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ROWS)
def test_hidden_backward_k_tiles(cuda, n, k):
    from mepol_amd import ops

    dz, W, h, _, ref_dz, _, ref_db = _case(n, k)
    dz_in, db_in = ops.hidden_backward(dz, W, h)
    err = (db_in - ref_db).abs().max().item()
    bound = 1e-10 * max(ref_db.abs().max().item(), 1.0)
    print(f"hidden_backward n={n} K={k}: dz err {(dz_in - ref_dz).abs().max().item():.3e}, "
          f"db err {err:.3e} (bound {bound:.3e})")
    torch.testing.assert_close(dz_in, ref_dz, rtol=1e-12, atol=1e-12)
    assert err <= bound
    ws = ops.hidden_backward_workspace(n, H0, dz.device)
    b_dz, b_db = ops.hidden_backward(dz, W, h, ws=ws)
    assert torch.equal(dz_in, b_dz) and torch.equal(db_in, b_db)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("variant", [0, 9])
def test_gemm_nt_k_tiles(cuda, n, k, variant):
    from mepol_amd import ops

    dz, W, _, _, _, _, _ = _case(n, k)
    B = W.t().contiguous()  # [H0, k]
    ref = dz @ B.t()
    out = ops.gemm_nt(dz, B, variant=variant)
    print(f"gemm_nt v{variant} n={n} K={k}: err {(out - ref).abs().max().item():.3e}")
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)
    assert torch.equal(ops.gemm_nt(dz, B, variant=variant), out)
