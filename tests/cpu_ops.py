"""CPU stand-ins for mepol_amd.ops (TEST INFRASTRUCTURE ONLY).

Same function signatures as the HIP-backed ops, implemented with the numpy oracle, so the
multi-rank collective algebra of mepol_amd/parallel.py can be exercised with the gloo backend
on CPU-only machines.  Never used by the product.
"""
import numpy as np
import torch

from oracle import mepol_oracle as O


class _NoCheck:
    def raise_if_invalid(self):
        pass


def knn(cand, kp1, query=None, defer_check=False):
    q = cand if query is None else query
    D, I = O.knn_exact(cand.float().numpy(), kp1, Q=q.float().numpy())
    out = (torch.as_tensor(D), torch.as_tensor(I),
           torch.as_tensor(I.T.astype(np.int32)).contiguous())
    return out + ((_NoCheck(),) if defer_check else ())


def iw_forward(logp_t, logp_b, offsets, n_particles, normalize=True):
    lt, lb = logp_t.numpy(), logp_b.numpy()
    off = offsets.numpy()
    u = np.zeros(n_particles)
    ts = np.zeros(lt.shape[0])
    for n in range(lt.shape[0]):
        L = off[n + 1] - off[n]
        x = np.exp(np.cumsum(lt[n, :L] - lb[n, :L]))
        u[off[n]:off[n + 1]] = x
        ts[n] = x.sum()
    u, ts = torch.as_tensor(u), torch.as_tensor(ts)
    if not normalize:
        return u, ts, None, None
    U = ts.sum()
    return u, ts, u / U, U


def iw_normalize(u, U):
    return u / U


def entropy_forward(w, idxT, D, k, ns, G, B, eps, n_w=None, g_out=None, out4=None, vals=None):
    """ops.entropy_forward, its emit form included: with `vals` (and `out4`) given, vals =
    {out4[0] on entry, new KL} and out4 is then overwritten in place."""
    w = w.numpy()
    I = idxT.numpy().T
    Dn = D.numpy()
    n_w = w.shape[0] if n_w is None else n_w
    W = w[I[:, :k]].sum(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        V = (Dn[:, k] ** ns * np.pi ** (ns / 2)) / G
        r = W / (V + eps)
        term = (W / k) * np.log(r + eps)
        klt = np.log(k / (n_w * W) + eps)
        g = -(1.0 / k) * (np.log(r + eps) + r / (r + eps))
        new4 = np.array([-term.sum() + B, klt.sum() / n_w, term.sum(), klt.sum()])
    g = torch.as_tensor(g)
    if g_out is not None:
        g = g_out.copy_(g)
    if vals is not None:
        assert out4 is not None
        vals[0] = out4[0]
        vals[1] = float(new4[1])
    new4 = torch.as_tensor(new4)
    out4 = out4.copy_(new4) if out4 is not None else new4
    return out4, torch.as_tensor(W), g


def iw_normalize_gathered(xu_all, world, n, nt, w_out):
    """ops.iw_normalize_gathered: w_out [world n] from the [u | trajectory sums] blocks."""
    x = xu_all.numpy().reshape(world, n + nt)
    U = x[:, n:].sum()
    w_out.copy_(torch.as_tensor((x[:, :n] / U).reshape(-1)))
    return w_out


def sharded_emit(x_all, world, stride, off, B, n_global, sums_cur, vals):
    """ops.sharded_emit: vals <- (B - sums_cur[0], rank-order sum of x[r, off + 1] / n_global),
    sums_cur <- the rank-order sums of x[r, off], x[r, off + 1]."""
    x = x_all.numpy().reshape(world, stride)
    s0, s1 = 0.0, 0.0
    for r in range(world):
        s0 += float(x[r, off])
        s1 += float(x[r, off + 1])
    vals[0] = B - float(sums_cur[0])
    vals[1] = s1 / n_global
    sums_cur[0] = s0
    sums_cur[1] = s1


def csr_build(idxT, k, n_own, col_offset=0, row_offset=0, nq=None):
    I = idxT.numpy()[:k]
    nq = I.shape[1] if nq is None else nq
    lists = [[] for _ in range(n_own)]
    for c in range(k):
        for i in range(nq):
            j = int(I[c, i]) - col_offset
            if 0 <= j < n_own:
                lists[j].append(row_offset + i)
    off = np.zeros(n_own + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    rows = np.array([r for x in lists for r in x] or [0], np.int32)
    return torch.as_tensor(off), torch.as_tensor(rows)


def entropy_gamma(g, w_own, csr_off, csr_rows):
    g, w = g.numpy(), w_own.numpy()
    off, rows = csr_off.numpy(), csr_rows.numpy()
    gamma = np.array([g[rows[off[j]:off[j + 1]]].sum() for j in range(w.shape[0])])
    partials = np.array([(gamma * w).sum()])
    return torch.as_tensor(gamma), torch.as_tensor(partials), 1


def entropy_reverse_scan(gamma, w, partials, nparts, offsets, nt, T_stride, grad_H, S_ext=None):
    S = float(S_ext) if S_ext is not None else float(partials[:nparts].sum())
    c = (gamma.numpy() - S) * w.numpy()
    off = offsets.numpy()
    out = np.zeros((nt, T_stride))
    for n in range(nt):
        seg = c[off[n]:off[n + 1]]
        out[n, :len(seg)] = np.cumsum(seg[::-1])[::-1]
    return torch.as_tensor(out * float(grad_H))


# ---------------------------------------------------------------------------------------------
# The Gaussian head, the input layer and the optimizer (csrc/head.hip, mlp.hip, optim.hip) in
# plain f64 numpy, from the formulas in those files' header comments.
# ---------------------------------------------------------------------------------------------
_LOG2PI = float(np.log(2.0 * np.pi))
_STD_EPS = 1e-7


def _np(t):
    return None if t is None else t.numpy()


def _into(out, value):
    value = torch.as_tensor(np.ascontiguousarray(value))
    return value if out is None else out.copy_(value.reshape(out.shape))


def _relu_in(z, bz):
    pre = _np(z) + _np(bz) if bz is not None else _np(z)
    return pre, np.maximum(pre, 0.0)


def head_forward(z, Wm, bm, log_std, act, bz=None, mu_out=None, logp_out=None):
    _, x = _relu_in(z, bz)
    mu = x @ _np(Wm).T + _np(bm)
    ls = _np(log_std)
    sigma = np.exp(ls) + _STD_EPS
    d = _np(act) - mu
    logp = (-0.5 * (_LOG2PI + 2.0 * ls + d * d / (sigma * sigma))).sum(axis=1)
    return _into(mu_out, mu), _into(logp_out, logp)


def head_backward(grad_logp, z, Wm, log_std, act, mu, bz=None, need_dz=True, ws=None,
                  outs=None, reduce_stream=None, defer_reduce=False):
    pre, x = _relu_in(z, bz)
    W, ls, g = _np(Wm), _np(log_std), _np(grad_logp).reshape(-1, 1)
    e = np.exp(ls)
    sigma = e + _STD_EPS
    d = _np(act) - _np(mu)
    dmu = g * d / (sigma * sigma)
    dls = (g * (-1.0 + d * d * (e / (sigma * sigma * sigma)))).sum(axis=0)
    dz = np.where(pre > 0.0, dmu @ W, 0.0)
    o = outs if outs is not None else (None, None, None, None)
    res = (torch.as_tensor(dz) if need_dz else None, _into(o[0], dmu.T @ x),
           _into(o[1], dmu.sum(axis=0)), _into(o[2], dls),
           _into(o[3], dz.sum(axis=0)) if bz is not None else None)
    return res + ((lambda: None),) if defer_reduce else res


def layer_forward(x, W, b, out=None):
    return _into(out, np.maximum(_np(x) @ _np(W).T + _np(b), 0.0))


def layer_backward(dh, h, x, ws=None, dW_out=None, db_out=None):
    dz = np.where(_np(h) > 0.0, _np(dh), 0.0)
    return _into(dW_out, dz.T @ _np(x)), _into(db_out, dz.sum(axis=0))


def layer_tangent(x, dW, db, h, out=None):
    return _into(out, np.where(_np(h) > 0.0, _np(x) @ _np(dW).T + _np(db), 0.0))


def mean_tangent(t, z, Wm, dWm, dbm, scale, bz=None, out=None):
    """ops.mean_tangent: scale (t Wm^T + relu(z + bz) dWm^T + dbm); t is not masked."""
    _, x = _relu_in(z, bz)
    return _into(out, _np(scale) * (_np(t) @ _np(Wm).T + x @ _np(dWm).T + _np(dbm)))


def mean_backward(c, z, Wm, bz=None, need_dz=True, ws=None, dz_out=None, outs=None):
    """ops.mean_backward: (dz or None, dWm, dbm, dbz or None) from the cotangent c on mu."""
    pre, x = _relu_in(z, bz)
    cn = _np(c)
    if cn.shape[0] == 0:
        raise ValueError("mean_backward: no rows")
    dz = np.where(pre > 0.0, cn @ _np(Wm), 0.0)
    o = outs if outs is not None else (None, None, None)
    return (_into(dz_out, dz) if need_dz else None, _into(o[0], cn.T @ x),
            _into(o[1], cn.sum(axis=0)), _into(o[2], dz.sum(axis=0)) if bz is not None else None)


# ---------------------------------------------------------------------------------------------
# TRPO's batch kernels (csrc/trpo_batch.hip) through the sequential restatements of
# tests/goal_rl_cases.py.
# ---------------------------------------------------------------------------------------------
def traj_budget(lens, dones, budget):
    import goal_rl_cases as C

    lo, do, off, meta = C.budget(_np(lens), _np(dones), int(budget))
    return (torch.as_tensor(lo), torch.as_tensor(do.astype(np.int32)), torch.as_tensor(off),
            torch.as_tensor(np.array(meta, dtype=np.int64)))


def gae(rewards, values, lens, dones, offsets, n_out, gamma, lambd, states_rec, actions_rec):
    import goal_rl_cases as C

    nf, a = states_rec.shape[2], actions_rec.shape[2]
    if int(n_out) == 0:
        out = (np.zeros(0), np.zeros(0), np.zeros((0, nf)), np.zeros((0, a)))
    else:
        out = C.gae_batch(_np(rewards), _np(values), _np(lens), _np(dones), _np(states_rec),
                          _np(actions_rec), gamma, lambd)
    return tuple(torch.as_tensor(np.ascontiguousarray(v)) for v in out)


def standardize(x, out=None):
    xn = _np(x).copy()
    with np.errstate(all="ignore"):
        return _into(out, (xn - xn.mean()) / xn.std())


def optim_step(kind, params, grads, exp_avg, exp_avg_sq, scalars, snapshot=None):
    """csrc/optim.hip's op sequence, one f64 rounding per op, in place; scalars[0] == 0: nothing
    is written.  Snapshots (lists or None) receive the values from before the update."""
    sc = [float(s) for s in _np(scalars)]
    if sc[0] == 0.0:
        return
    ps, ms, vs = snapshot if snapshot is not None else (None, None, None)
    with np.errstate(all="ignore"):
        for i, (p, g, v) in enumerate(zip(params, grads, exp_avg_sq)):
            p, g, v = p.numpy(), g.numpy(), v.numpy()
            if ps is not None:
                ps[i].copy_(torch.as_tensor(p.copy()))
            if vs is not None:
                vs[i].copy_(torch.as_tensor(v.copy()))
            if kind == 0:
                step_size, bc2_sqrt, b1, b2, eps = sc[1:6]
                m = exp_avg[i].numpy()
                if ms is not None:
                    ms[i].copy_(torch.as_tensor(m.copy()))
                w1, w2 = 1.0 - b1, 1.0 - b2
                m[...] = m + w1 * (g - m)
                v[...] = v * b2 + w2 * (g * g)
                p[...] = p + (-step_size) * (m / (np.sqrt(v) / bc2_sqrt + eps))
            else:
                lr, alpha, eps = sc[1:4]
                v[...] = v * alpha + (1.0 - alpha) * (g * g)
                p[...] = p + (-lr) * (g / (np.sqrt(v) + eps))


def critic_fit(states, targets, index, batch, params, exp_avg, exp_avg_sq, lr, betas=(0.9, 0.999),
               eps=1e-8, first_step=1, loss_out=None):
    """csrc/critic_fit.hip in plain f64 numpy, in place: numpy's own summation orders (BLAS
    products, pairwise sums), 2 err / B as the kernel writes it, every ReLU and mask a select,
    Adam in adam_math.hpp's op order."""
    x_all, t_all, idx = _np(states), _np(targets), _np(index).astype(np.int64)
    p, m, v = ([t.numpy() for t in lst] for lst in (params, exp_avg, exp_avg_sq))
    W1, b1, W2, b2, W3, b3 = p
    n_steps = idx.size // batch
    loss = np.empty(n_steps)
    w1, w2 = 1.0 - betas[0], 1.0 - betas[1]
    with np.errstate(all="ignore"):
        for s in range(n_steps):
            rows = idx[s * batch:(s + 1) * batch]
            x, t = x_all[rows], t_all[rows]
            z1 = x @ W1.T + b1
            h1 = _sel(z1 > 0, z1)
            z2 = h1 @ W2.T + b2
            h2 = _sel(z2 > 0, z2)
            err = (h2 @ W3[0] + b3[0]) - t
            loss[s] = np.sum(err * err) / batch
            dv = 2.0 * err / batch
            dz2 = _sel(z2 > 0, dv[:, None] * W3[0][None, :])
            dz1 = _sel(z1 > 0, dz2 @ W2)
            grads = (dz1.T @ x, dz1.sum(axis=0), dz2.T @ h1, dz2.sum(axis=0), (dv @ h2)[None, :],
                     dv.sum()[None])
            step = float(first_step + s)
            step_size, bc2_sqrt = lr / (1 - betas[0] ** step), (1 - betas[1] ** step) ** 0.5
            for pi, g, mi, vi in zip(p, grads, m, v):
                mi[...] = mi + w1 * (g - mi)
                vi[...] = vi * betas[1] + w2 * (g * g)
                pi[...] = pi + (-step_size) * (mi / (np.sqrt(vi) / bc2_sqrt + eps))
    return _into(loss_out, loss)


# ---------------------------------------------------------------------------------------------
# The f64 matrix-core kernels (csrc/gemm.hip, wgrad.hip, policy_fwd.hip) in plain f64 numpy.
# Every ReLU and mask is a select, as in the kernels: a nan that is masked off (or a nan
# pre-activation) gives 0.
# ---------------------------------------------------------------------------------------------
def _sel(mask, v):
    return np.where(mask, v, 0.0)


def _gt0(v):
    with np.errstate(invalid="ignore"):
        return v > 0.0


def _pack_mask(on):
    """[n, h0] bools -> [n, ceil(h0 / 16)] int16 words, bit b of word w = on[:, 16 w + b]."""
    n, h0 = on.shape
    mw = (h0 + 15) // 16
    bits = np.zeros((n, mw * 16), np.uint16)
    bits[:, :h0] = on
    words = (bits.reshape(n, mw, 16) << np.arange(16, dtype=np.uint16)).sum(axis=2)
    return words.astype(np.uint16).view(np.int16)


def _unpack_mask(words, h0):
    w = words.numpy().view(np.uint16)
    bits = (w[:, :, None] >> np.arange(16, dtype=np.uint16)) & 1
    return bits.reshape(w.shape[0], -1)[:, :h0].astype(bool)


def _scratch(*_):
    return torch.empty(1, dtype=torch.uint8)


dh1_layer1_workspace = weight_grad_workspace = hidden_backward_workspace = _scratch


def h1_mask_buffer(n, hidden0, device):
    return torch.empty((n, (hidden0 + 15) // 16), dtype=torch.int16)


def gemm_nt(A, B, bias=None, relu=False, out=None, variant=0):
    with np.errstate(invalid="ignore"):
        v = _np(A) @ _np(B).T
        if bias is not None:
            v = v + _np(bias)
    if relu:
        v = _sel(_gt0(v), v)
    return _into(out, v)


def policy_forward(x, W1, b1, W2, b2, Wm, bm, log_std, act, h1_out=None, z2_out=None,
                   mu_out=None, logp_out=None, mask_out=None, row_tile=0):
    with np.errstate(invalid="ignore", over="ignore"):
        pre = _np(x) @ _np(W1).T + _np(b1)
        h1 = _sel(_gt0(pre), pre)
        z2 = h1 @ _np(W2).T
        pre2 = z2 + _np(b2)
        mu = _sel(_gt0(pre2), pre2) @ _np(Wm).T + _np(bm)
        ls = _np(log_std)
        sigma = np.exp(ls) + _STD_EPS
        d = _np(act) - mu
        logp = (-0.5 * (_LOG2PI + 2.0 * ls + d * d / (sigma * sigma))).sum(axis=1)
    if mask_out is not None:
        mask_out.copy_(torch.as_tensor(_pack_mask(h1 > 0.0)))
    return _into(h1_out, h1), _into(z2_out, z2), _into(mu_out, mu), _into(logp_out, logp)


def dh1_layer1_backward(dz2, W2t, h1, x, ws=None, dW_out=None, db_out=None, mask=None, w2=None):
    # (a copy in W2t's layout: BLAS sums a transposed view in another order)
    Wt = np.ascontiguousarray(_np(w2).T) if w2 is not None else _np(W2t)
    on = _unpack_mask(mask, Wt.shape[0]) if mask is not None else _gt0(_np(h1))
    with np.errstate(invalid="ignore", over="ignore"):
        dz1 = _sel(on, _np(dz2) @ Wt.T)
        return _into(dW_out, dz1.T @ _np(x)), _into(db_out, dz1.sum(axis=0))


def weight_grad(dy, x, out=None, ws=None):
    with np.errstate(invalid="ignore", over="ignore"):
        return _into(out, _np(dy).T @ _np(x))


def hidden_backward(dz_out, W, h_in, ws=None, dz_out_buf=None, db_out=None):
    with np.errstate(invalid="ignore", over="ignore"):
        dz = _sel(_gt0(_np(h_in)), _np(dz_out) @ _np(W))
        return _into(dz_out_buf, dz), _into(db_out, dz.sum(axis=0))


def hidden_tangent(t_in, h_in, W, dW, db, mask_src, mask_bias=None, out=None, variant=0):
    with np.errstate(invalid="ignore", over="ignore"):
        pre = _np(mask_src) + (_np(mask_bias) if mask_bias is not None else 0.0)
        v = _np(t_in) @ _np(W).T + _np(h_in) @ _np(dW).T + _np(db)
    return _into(out, _sel(_gt0(pre), v))
