"""Seeded cases of TRPO's critic fit (ops.critic_fit, csrc/critic_fit.hip) and a CPU stand-in.

The stand-in, fit_reference, restates the fit in numpy: n_steps Adam steps of loss =
mean((v(x_b) - t_b)^2) on the critic Linear(nf, h0) -> ReLU -> Linear(h0, h1) -> ReLU ->
Linear(h1, 1).  Every matrix product runs in np.longdouble (x87 80-bit here) and is rounded to
f64 once per result; the elementwise steps and Adam's arithmetic run in f64, Adam's in the op
order of csrc/adam_math.hpp (torch's foreach step).  `mistake` plants ONE wrong step, for the
host test that shows each of them is caught at the GPU test's tolerance.

A case is a dict: nf, h0, h1, B, N, states [N, nf], targets [N], index [n_steps * B] int32,
params / m / v (six arrays each, torch's order W1, b1, W2, b2, W3, b3), first_step.  Cases are
built once and are read-only.
"""
import functools

import numpy as np

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
LD = np.longdouble
MISTAKES = ("mask_ge", "dv_no_mean", "stale_w2", "bc2_wrong_step")
NAMES = ("full_1step", "full_2step", "ragged", "ragged_nan", "nf1", "nf16", "chain_dense",
         "chain_sparse", "dead_unit")
# tolerance of the GPU test: parameters and moments absolute, loss relative
GPU_ATOL, GPU_LOSS_RTOL = 1e-12, 1e-12


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _mm(a, b):
    """a @ b in long double, rounded to f64 once."""
    return _f64(a.astype(LD) @ b.astype(LD))


def adam_scalars(first_step, n_steps):
    """(lr / bias_correction1, sqrt(bias_correction2)) per step, as torch.optim.Adam's Python."""
    out = []
    for k in range(n_steps):
        step = float(first_step + k)
        out.append((LR / (1 - BETAS[0] ** step), (1 - BETAS[1] ** step) ** 0.5))
    return out


def adam_update(p, g, m, v, step_size, bc2_sqrt):
    """In place, csrc/adam_math.hpp's op order, one f64 rounding per op."""
    b1, b2 = BETAS
    w1, w2 = 1.0 - b1, 1.0 - b2
    m += w1 * (g - m)
    v *= b2
    v += w2 * (g * g)
    d = np.sqrt(v) / bc2_sqrt + EPS
    p += (-step_size) * (m / d)


def fit_reference(case, mistake=None):
    """{'params', 'm', 'v': six arrays each, 'loss': [n_steps]} after the case's steps."""
    assert mistake is None or mistake in MISTAKES
    B = case["B"]
    index = case["index"]
    n_steps = index.size // B
    p = [a.copy() for a in case["params"]]
    m = [a.copy() for a in case["m"]]
    v = [a.copy() for a in case["v"]]
    W1, b1, W2, b2, W3, b3 = p
    scal = adam_scalars(case["first_step"], n_steps + 1)
    loss = np.zeros(n_steps)
    W2_before_last_step = None
    for s in range(n_steps):
        rows = index[s * B:(s + 1) * B]
        x, t = case["states"][rows], case["targets"][rows]
        W2_read = W2_before_last_step if (mistake == "stale_w2" and s > 0) else W2
        z1 = _f64(x.astype(LD) @ W1.astype(LD).T + b1.astype(LD))
        h1 = np.where(z1 > 0, z1, 0.0)
        z2 = _f64(h1.astype(LD) @ W2_read.astype(LD).T + b2.astype(LD))
        h2 = np.where(z2 > 0, z2, 0.0)
        val = _f64(h2.astype(LD) @ W3[0].astype(LD) + b3.astype(LD)[0])
        err = val - t
        loss[s] = float(np.sum(err.astype(LD) ** 2) / B)
        dv = 2.0 * err if mistake == "dv_no_mean" else 2.0 * err / B
        mask2 = z2 >= 0 if mistake == "mask_ge" else z2 > 0
        mask1 = z1 >= 0 if mistake == "mask_ge" else z1 > 0
        dW3 = _mm(dv[None, :], h2)
        db3 = _f64([np.sum(dv.astype(LD))])
        dz2 = np.where(mask2, dv[:, None] * W3[0][None, :], 0.0)
        dW2 = _mm(dz2.T, h1)
        db2 = _f64(np.sum(dz2.astype(LD), axis=0))
        dz1 = np.where(mask1, _mm(dz2, W2_read), 0.0)
        dW1 = _mm(dz1.T, x)
        db1 = _f64(np.sum(dz1.astype(LD), axis=0))
        step_size, bc2_sqrt = scal[s]
        if mistake == "bc2_wrong_step":
            bc2_sqrt = scal[s + 1][1]
        W2_before_last_step = W2.copy()
        for pi, gi, mi, vi in zip(p, (dW1, db1, dW2, db2, dW3, db3), m, v):
            adam_update(pi, gi, mi, vi, step_size, bc2_sqrt)
    return {"params": p, "m": m, "v": v, "loss": loss}


@functools.lru_cache(maxsize=None)
def reference(name):
    """fit_reference of a case, computed once and read-only."""
    out = fit_reference(case(name))
    for k in ("params", "m", "v"):
        for a in out[k]:
            a.setflags(write=False)
    out["loss"].setflags(write=False)
    return out


def max_deviation(got, ref):
    """(largest absolute difference over parameters and moments, largest relative loss
    difference) of two results in fit_reference's form."""
    dev = 0.0
    for k in ("params", "m", "v"):
        for a, b in zip(got[k], ref[k]):
            assert a.shape == b.shape
            d = np.abs(np.asarray(a) - np.asarray(b))
            dev = max(dev, float(d.max()) if np.isfinite(d).all() else np.inf)
    la, lb = np.asarray(got["loss"]), np.asarray(ref["loss"])
    rel = np.abs(la - lb) / np.abs(lb)
    return dev, (float(rel.max()) if np.isfinite(rel).all() else np.inf)


def _net(rng, nf, h0, h1):
    def lin(o, i):
        return rng.standard_normal((o, i)) / np.sqrt(i), rng.uniform(-0.3, 0.3, o)

    W1, b1 = lin(h0, nf)
    W2, b2 = lin(h1, h0)
    W3, b3 = lin(1, h1)
    return [W1, b1, W2, b2, W3, b3]


def _build(seed, nf, h0, h1, B, N, n_steps=None, index=None, first_step=1, moments=False,
           sparse=False):
    rng = np.random.default_rng(seed)
    params = _net(rng, nf, h0, h1)
    states = rng.uniform(-1.0, 1.0, (N, nf))
    targets = rng.standard_normal(N)
    if sparse:  # GridGoal-like: a reward of 1 on 3 % of the rows, discounted sums elsewhere 0
        targets = np.where(rng.uniform(size=N) < 0.03, 1.0, 0.0)
    if index is None:
        index = rng.integers(0, N, n_steps * B)
    if moments:
        m = [1e-3 * rng.standard_normal(p.shape) for p in params]
        v = [(1e-3 * rng.standard_normal(p.shape)) ** 2 + 1e-8 for p in params]
    else:
        m = [np.zeros_like(p) for p in params]
        v = [np.zeros_like(p) for p in params]
    return dict(nf=nf, h0=h0, h1=h1, B=B, N=N, states=states, targets=targets,
                index=np.asarray(index, dtype=np.int32), params=params, m=m, v=v,
                first_step=first_step)


RAGGED_NAN_ROW = 7


def _ragged_index():
    """Two passes of 4 mini-batches of 5 over 23 rows: each pass a permutation whose last 3 rows
    drop_last leaves unread; row RAGGED_NAN_ROW is among them in both passes."""
    rng = np.random.default_rng(41)
    passes = []
    for _ in range(2):
        perm = [int(r) for r in rng.permutation(23) if r != RAGGED_NAN_ROW]
        passes.append(perm[:20])
    return np.concatenate(passes)


def _make(name):
    if name == "full_1step":
        return _build(1, 2, 64, 64, 64, 200, n_steps=1, first_step=11, moments=True)
    if name == "full_2step":
        return _build(1, 2, 64, 64, 64, 200, n_steps=2, first_step=11, moments=True)
    if name in ("ragged", "ragged_nan"):
        c = _build(3, 3, 24, 40, 5, 23, index=_ragged_index())
        if name == "ragged_nan":
            c["targets"][RAGGED_NAN_ROW] = np.nan
        return c
    if name == "nf1":
        return _build(5, 1, 16, 64, 17, 50, n_steps=3)
    if name == "nf16":
        return _build(6, 16, 16, 64, 17, 50, n_steps=3)
    if name == "chain_dense":
        return _build(7, 2, 64, 64, 64, 512, n_steps=40)
    if name == "chain_sparse":
        return _build(8, 2, 64, 64, 64, 512, n_steps=40, sparse=True)
    if name == "dead_unit":
        c = _build(9, 2, 64, 64, 64, 256, n_steps=3)
        W1, b1, W2, b2, W3, b3 = c["params"]
        b1[DEAD1] = -1e3          # never active: z1 < 0 on every row
        b2[DEAD2] = -1e3
        W2[ZERO2, :] = 0.0        # z2 == 0 exactly on every row: the mask is z > 0, not z >= 0
        b2[ZERO2] = 0.0
        return c
    raise KeyError(name)


DEAD1, DEAD2, ZERO2 = 5, 17, 33


@functools.lru_cache(maxsize=None)
def case(name):
    c = _make(name)
    for k in ("states", "targets", "index"):
        c[k].setflags(write=False)
    for k in ("params", "m", "v"):
        for a in c[k]:
            a.setflags(write=False)
    return c


def dead_elements(result_or_case, key):
    """The arrays' elements that belong to the dead_unit case's three silent units, as one flat
    array: W1 / b1 of DEAD1 and W2's column DEAD1; W2's rows / b2 / W3 of DEAD2 and ZERO2."""
    W1, b1, W2, b2, W3, b3 = result_or_case[key]
    parts = [W1[DEAD1], b1[DEAD1:DEAD1 + 1], W2[:, DEAD1]]
    for k in (DEAD2, ZERO2):
        parts += [W2[k], b2[k:k + 1], W3[0, k:k + 1]]
    return np.concatenate([np.ravel(x) for x in parts])


# shapes the entry point refuses (nf, h0, h1, B) and the limit its message names
REFUSED = (((17, 64, 64, 64), "nf <= 16"), ((2, 65, 64, 64), "h0, h1 <= 64"),
           ((2, 64, 65, 64), "h0, h1 <= 64"), ((2, 64, 64, 65), "batch <= 64"),
           ((2, 64, 64, 0), "1 <= batch"))
