"""mepol_hidden_backward (csrc/gemm.hip) against torch f64 on the device, and the optimizer step
over more than 8 tensors against torch.optim."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, out, in): a single element pair; everything ragged in one tile; three column tiles
# (80 wide) with a k tail of 2; the C3 layer with a row tail of 1 past two 256-row blocks;
# many row blocks (more records than sum_records' 16 groups) with ragged columns
SHAPES = [(1, 2, 2), (77, 46, 38), (300, 50, 200), (513, 300, 400), (4097, 34, 72)]


def _inputs(n, o, i, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    kw = dict(dtype=torch.float64, device="cuda", generator=g)
    dz = torch.randn(n, o, **kw)
    W = torch.randn(o, i, **kw)
    h = torch.relu(torch.randn(n, i, **kw))  # about half of the mask is off
    return dz, W, h


def _check(dz_in, db_in, dz, W, h):
    ref_dz = (dz @ W) * (h > 0)
    ref_db = ref_dz.sum(0)
    err = (db_in - ref_db).abs().max().item()
    bound = 1e-10 * max(ref_db.abs().max().item(), 1.0)
    print(f"hidden_backward {tuple(dz.shape)} x {tuple(W.shape)}: dz max err "
          f"{(dz_in - ref_dz).abs().max().item():.3e}, db max err {err:.3e} (bound {bound:.3e})")
    torch.testing.assert_close(dz_in, ref_dz, rtol=1e-12, atol=1e-12)
    assert err <= bound


@pytest.mark.parametrize("n,o,i", SHAPES)
def test_hidden_backward_matches_torch(cuda, n, o, i):
    from mepol_amd import ops

    dz, W, h = _inputs(n, o, i)
    dz_in, db_in = ops.hidden_backward(dz, W, h)
    assert dz_in.shape == (n, i) and db_in.shape == (i,)
    _check(dz_in, db_in, dz, W, h)


@pytest.mark.parametrize("n,o,i", [(77, 46, 38), (4097, 34, 72)])
def test_hidden_backward_is_deterministic(cuda, n, o, i):
    """The same inputs give the same bits on every call, with the eager scratch cache and with
    a caller-owned workspace and output buffers."""
    from mepol_amd import ops

    dz, W, h = _inputs(n, o, i, seed=1)
    a_dz, a_db = ops.hidden_backward(dz, W, h)
    b_dz, b_db = ops.hidden_backward(dz, W, h)
    ws = ops.hidden_backward_workspace(n, i, dz.device)
    out = torch.full((n, i), float("nan"), dtype=torch.float64, device="cuda")
    db = torch.full((i,), float("nan"), dtype=torch.float64, device="cuda")
    c_dz, c_db = ops.hidden_backward(dz, W, h, ws=ws, dz_out_buf=out, db_out=db)
    assert c_dz is out and c_db is db
    d_dz, d_db = ops.hidden_backward(dz, W, h, ws=ws)
    for x_dz, x_db in ((b_dz, b_db), (c_dz, c_db), (d_dz, d_db)):
        assert torch.equal(a_dz, x_dz) and torch.equal(a_db, x_db)


def test_hidden_backward_null_db_and_short_workspace(cuda):
    from mepol_amd import _lib, ops
    from mepol_amd._lib import ptr

    n, o, i = 300, 50, 200
    dz, W, h = _inputs(n, o, i, seed=2)
    ref_dz, _ = ops.hidden_backward(dz, W, h)
    ws = ops.hidden_backward_workspace(n, i, dz.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((n, i), float("nan"), dtype=torch.float64, device="cuda")
    # db_in = NULL: dz_in alone
    _lib.call("mepol_hidden_backward", ptr(dz), n, o, ptr(W), ptr(h), i, ptr(out), None, ptr(ws),
              ws.numel(), st)
    assert torch.equal(out, ref_dz)
    # one byte short: MEPOL_ERR_WORKSPACE, nothing launched
    out.fill_(7.0)
    db = torch.full((i,), 7.0, dtype=torch.float64, device="cuda")
    lib = _lib.load()
    rc = lib.mepol_hidden_backward(ptr(dz), n, o, ptr(W), ptr(h), i, ptr(out), ptr(db), ptr(ws),
                                   ws.numel() - 1, st)
    assert rc == 1002
    assert b"workspace" in lib.mepol_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((db == 7.0).all())


# ---- optimizer over more than 8 tensors -----------------------------------------------------
SIZES = [1, 7, 64 * 29, 64, 48 * 64, 48, 32 * 48, 33, 8 * 32, 8, 1025]  # 11 tensors


def _adam_scalars(lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    return [1.0, lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5, beta1, beta2, eps, 0, 0]


def _optim_run(kind, count, steps=3, lr=1e-3):
    """`steps` optimizer steps over the first `count` tensors through ops.optim_step and through
    torch.optim (foreach=False) on the same gradients; returns (ours, torch's) parameters."""
    from mepol_amd import ops

    g = torch.Generator(device="cuda").manual_seed(3)
    kw = dict(dtype=torch.float64, device="cuda", generator=g)
    init = [torch.randn(s, **kw) for s in SIZES]
    grads = [[torch.randn(s, **kw) for s in SIZES] for _ in range(steps)]
    p = [t.clone() for t in init[:count]]
    m = [torch.zeros_like(t) for t in p] if kind == 0 else None
    v = [torch.zeros_like(t) for t in p]
    q = [torch.nn.Parameter(t.clone()) for t in init[:count]]
    if kind == 0:
        opt = torch.optim.Adam(q, lr=lr, foreach=False)
    else:
        opt = torch.optim.RMSprop(q, lr=lr, foreach=False)
    for s in range(steps):
        if kind == 0:
            scal = _adam_scalars(lr, s + 1)
        else:
            scal = [1.0, lr, 0.99, 1e-8, 0, 0, 0, 0]
        sc = torch.tensor(scal, dtype=torch.float64, device="cuda")
        ops.optim_step(kind, p, grads[s][:count], m, v, sc)
        for t, gr in zip(q, grads[s]):
            t.grad = gr.clone()
        opt.step()
    return p, [t.detach() for t in q]


@pytest.mark.parametrize("kind", [0, 1], ids=["adam", "rmsprop"])
def test_optim_step_eleven_tensors(cuda, kind):
    p11, ref11 = _optim_run(kind, 11)
    for a, b in zip(p11, ref11):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=0)
    # at most 8 tensors: what the kernel did before the limit was raised, the same values as
    # torch's, and the same bits as those tensors get in the 11-tensor call
    p7, ref7 = _optim_run(kind, 7)
    for a, b, c in zip(p7, ref7, p11):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=0)
        assert torch.equal(a, c)
