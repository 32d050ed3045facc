"""The tile layouts of the f64 MFMA kernels of the off-policy iteration against torch f64 on the
device, at the tolerances of tests/test_gpu_policy.py and tests/test_gpu_gemm.py, and the same
bits on every call: z2_head_kernel's column fragments at narrow, exact and full hidden1 for its
three row tiles (csrc/policy_fwd.hip), wgrad_kernel's o-blocks without fragment rows past O, with
a K-slice count per kind of o-block (csrc/wgrad.hip), and dh1_layer1_bwd_kernel at more tiles
than the chip has CUs (csrc/gemm.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---- policy_forward: z2 and the head over hidden1's column fragments --------------------------
# hidden1: 300 (19 fragments, the last of 12 columns), 272 (17 whole fragments), 256 (16: every
# wave's columns whole), 320 (all 20), 34 (3 fragments, the third of 2 columns: three waves of
# four own no column).  hidden0 = 10: a K loop of one full stage and a ragged tail.
# n = 83 and n = 5: a ragged last block for every row tile (64, 32 and 16 rows per workgroup).
@pytest.mark.parametrize("n", [83, 5])
@pytest.mark.parametrize("a", [1, 8])
@pytest.mark.parametrize("hidden1", [300, 272, 256, 320, 34])
def test_policy_forward_column_fragments(cuda, hidden1, a, n):
    from mepol_amd import ops
    from mepol_amd import policy as P

    nf, hidden0 = 7, 10
    torch.manual_seed(hidden1 + a + n)
    pol = P.GaussianPolicy([hidden0, hidden1], nf, a, -0.4).cuda()
    s = torch.randn(n, nf, dtype=torch.float64, device="cuda")
    act = 0.5 * torch.randn(n, a, dtype=torch.float64, device="cuda")
    W1, b1 = pol.net[0].weight.detach(), pol.net[0].bias.detach()
    W2, b2 = pol.net[2].weight.detach(), pol.net[2].bias.detach()
    Wm, bm = pol.mean.weight.detach(), pol.mean.bias.detach()
    ls = pol.log_std.detach()
    h1_ref = torch.relu(s @ W1.t() + b1)
    z2_ref = h1_ref @ W2.t()
    mu_ref = torch.relu(z2_ref + b2) @ Wm.t() + bm
    std = torch.exp(ls) + 1e-7
    lp_ref = torch.sum(-0.5 * (P.LOG_2PI + 2 * ls + (act - mu_ref) ** 2 / std ** 2), dim=1)
    z2_tiles = []
    for tile in (64, 32, 16):
        h1, z2, mu, logp = ops.policy_forward(s, W1, b1, W2, b2, Wm, bm, ls, act, row_tile=tile)
        torch.testing.assert_close(h1, h1_ref, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(z2, z2_ref, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(mu, mu_ref, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(logp, lp_ref, rtol=1e-12, atol=1e-11)
        z2_tiles.append(z2)
    assert torch.equal(z2_tiles[0], z2_tiles[1]) and torch.equal(z2_tiles[0], z2_tiles[2])


# ---- weight_grad ----------------------------------------------------------------------------
# (O, I): (300, 400) four full o-blocks and one of 3 fragments, 5 i-blocks; (44, 30) one o-block
# of 3 fragments, clamped columns on both sides; (64, 80) one o-block of 4 fragments, nothing
# ragged; (17, 400) one o-block of 2 fragments, the second holding one row.
# n: 2051 and 300 give 8 K-slices to both kinds of o-block (slices of 260 rows with a ragged last
# k-step in the last one; slices of 40 rows, the last one of 20).  8000 gives (300, 400) 31 slices
# for the full o-blocks and 24 for the last: slice counts that differ, one of them no multiple of
# 8 (the reduce's short last batch), and XCDs with unequal lists.
@pytest.mark.parametrize("n", [2051, 300, 8000])
@pytest.mark.parametrize("o, i", [(300, 400), (44, 30), (64, 80), (17, 400)])
def test_weight_grad_o_blocks(cuda, n, o, i):
    from mepol_amd import ops

    g = torch.Generator(device="cuda").manual_seed(n + o + i)
    dy = torch.randn((n, o), dtype=torch.float64, device="cuda", generator=g)
    x = torch.randn((n, i), dtype=torch.float64, device="cuda", generator=g)
    ref = dy.t() @ x
    ws = ops.weight_grad_workspace(n, o, i, dy.device)
    ws.fill_(0x7F)  # stale scratch must not show in the result
    out = ops.weight_grad(dy, x, ws=ws)
    assert out.shape == (o, i)
    err = (out - ref).abs().max().item()
    bound = 1e-10 * max(ref.abs().max().item(), 1.0)
    print(f"weight_grad {(n, o, i)}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert torch.equal(ops.weight_grad(dy, x), out)


# ---- dh1_layer1_backward ---------------------------------------------------------------------
# M = 400 (5 column tiles), K = 20 (two k-tiles, the second ragged), F = 3.
# n = 13319: 53 row blocks x 5 = 265 tiles, more than the chip has CUs (one workgroup fits a CU),
# so some CUs run two; the last row block holds 7 rows.
# n = 300: 10 tiles, two row blocks, the second of 44 rows.
@pytest.mark.parametrize("n", [13319, 300])
def test_dh1_layer1_backward_many_tiles(cuda, n):
    from mepol_amd import ops

    M, K, F = 400, 20, 3
    torch.manual_seed(n + M)
    f64 = dict(dtype=torch.float64, device="cuda")
    x = torch.randn(n, F, **f64)
    W1, b1 = torch.randn(M, F, **f64) * 0.3, torch.randn(M, **f64) * 0.1
    W2 = torch.randn(K, M, **f64) * 0.1
    h1 = torch.relu(x @ W1.t() + b1)
    dz2 = torch.randn(n, K, **f64)
    pos = (h1 > 0).view(n, M // 16, 16).to(torch.int32)
    bits = (pos << torch.arange(16, device="cuda", dtype=torch.int32)).sum(-1)
    mask = (bits - ((bits & 0x8000) << 1)).to(torch.int16).contiguous()
    assert mask.shape == ops.h1_mask_buffer(n, M, x.device).shape

    dz1 = (dz2 @ W2) * (h1 > 0)
    W2t = W2.t().contiguous()
    dW, db = ops.dh1_layer1_backward(dz2, W2t, h1, x)
    torch.testing.assert_close(dW, dz1.t() @ x, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(db, dz1.sum(0), rtol=1e-11, atol=1e-11)
    dWm, dbm = ops.dh1_layer1_backward(dz2, W2t, h1, x, mask=mask)
    assert torch.equal(dW, dWm) and torch.equal(db, dbm)
    dWw, dbw = ops.dh1_layer1_backward(dz2, None, h1, x, mask=mask, w2=W2)
    assert torch.equal(dW, dWw) and torch.equal(db, dbw)
    # the same bits on a second call
    dWw2, dbw2 = ops.dh1_layer1_backward(dz2, None, h1, x, mask=mask, w2=W2)
    assert torch.equal(dWw, dWw2) and torch.equal(dbw, dbw2)
