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
# the mistakes that the op-level cases (second half of this file) must catch as well
MORE_MISTAKES = ("mean_64", "rows_ge_48", "db1_wave", "db2_wave", "dW3_wave", "db3_wave",
                 "next_rows", "step_size_wrong_step", "betas_default", "eps_default",
                 "w2_transposed", "w1_last_col_moments", "kdrop_z1", "kdrop_z2", "kdrop_dW2",
                 "kdrop_dh1", "kdrop_dW1", "index_clamp", "dz1_mask_z2")
NAMES = ("full_1step", "full_2step", "ragged", "ragged_nan", "nf1", "nf16", "chain_dense",
         "chain_sparse", "dead_unit")
# tolerance of the GPU test: parameters and moments absolute, loss relative
GPU_ATOL, GPU_LOSS_RTOL = 1e-12, 1e-12


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _mm(a, b):
    """a @ b in long double, rounded to f64 once."""
    return _f64(a.astype(LD) @ b.astype(LD))


def scalars(case):
    """(lr, betas, eps) of a case: Adam's defaults at lr = 1e-2 unless the case names others."""
    return case.get("lr", LR), case.get("betas", BETAS), case.get("eps", EPS)


def adam_scalars(first_step, n_steps, lr=LR, betas=BETAS):
    """(lr / bias_correction1, sqrt(bias_correction2)) per step, as torch.optim.Adam's Python."""
    out = []
    for k in range(n_steps):
        step = float(first_step + k)
        out.append((lr / (1 - betas[0] ** step), (1 - betas[1] ** step) ** 0.5))
    return out


def adam_update(p, g, m, v, step_size, bc2_sqrt, betas=BETAS, eps=EPS):
    """In place, csrc/adam_math.hpp's op order, one f64 rounding per op."""
    b1, b2 = betas
    w1, w2 = 1.0 - b1, 1.0 - b2
    with np.errstate(all="ignore"):
        m += w1 * (g - m)
        v *= b2
        v += w2 * (g * g)
        d = np.sqrt(v) / bc2_sqrt + eps
        p += (-step_size) * (m / d)


def fit_reference(case, mistake=None):
    """{'params', 'm', 'v': six arrays each, 'loss': [n_steps]} after the case's steps."""
    assert mistake is None or mistake in MISTAKES + MORE_MISTAKES
    B, N, nf, h0, h1n = case["B"], case["N"], case["nf"], case["h0"], case["h1"]
    index = case["index"]
    n_steps = index.size // B
    p = [a.copy() for a in case["params"]]
    m = [a.copy() for a in case["m"]]
    v = [a.copy() for a in case["v"]]
    W1, b1, W2, b2, W3, b3 = p
    lr, betas, eps = scalars(case)
    if mistake == "betas_default":
        betas = BETAS
    if mistake == "eps_default":
        eps = EPS
    scal = adam_scalars(case["first_step"], n_steps + 1, lr, betas)
    loss = np.zeros(n_steps)
    W2_before_last_step = None

    def kdrop(which, K):  # the K that a product with its last ragged k-step dropped sums over
        return 4 * (K // 4) if mistake == "kdrop_" + which and K % 4 else K

    def wave_sum(which, a):  # the column sums of a [B, ...] array, wave 1's rows missing
        if mistake == which + "_wave":
            a = np.concatenate([a[:16], a[32:]])
        return _f64(np.sum(a.astype(LD), axis=0))

    with np.errstate(all="ignore"):
        for s in range(n_steps):
            sr = s + 1 if (mistake == "next_rows" and s + 1 < n_steps) else s
            rows = index[sr * B:(sr + 1) * B]
            if mistake == "index_clamp" and N >= 2:
                rows = np.minimum(rows, N - 2)
            x, t = case["states"][rows], case["targets"][rows]
            W2_read = W2_before_last_step if (mistake == "stale_w2" and s > 0) else W2
            if mistake == "w2_transposed" and h0 != h1n:
                W2_read = W2.reshape(h0, h1n).T
            k = kdrop("z1", nf)
            z1 = _f64(x[:, :k].astype(LD) @ W1[:, :k].astype(LD).T + b1.astype(LD))
            h1 = np.where(z1 > 0, z1, 0.0)
            k = kdrop("z2", h0)
            z2 = _f64(h1[:, :k].astype(LD) @ W2_read[:, :k].astype(LD).T + b2.astype(LD))
            h2 = np.where(z2 > 0, z2, 0.0)
            val = _f64(h2.astype(LD) @ W3[0].astype(LD) + b3.astype(LD)[0])
            err = val - t
            mean = 64 if mistake == "mean_64" else B
            loss[s] = float(np.sum(err.astype(LD) ** 2) / mean)
            dv = 2.0 * err if mistake == "dv_no_mean" else 2.0 * err / mean
            mask2 = z2 >= 0 if mistake == "mask_ge" else z2 > 0
            mask1 = z1 >= 0 if mistake == "mask_ge" else z1 > 0
            if mistake == "dz1_mask_z2" and h0 == h1n:
                mask1 = z2 > 0
            dW3 = _mm(dv[None, :], h2)
            if mistake == "dW3_wave":
                dW3 = wave_sum("dW3", dv[:, None] * h2.astype(LD))[None, :]
            db3 = wave_sum("db3", dv)[None]
            dz2 = np.where(mask2, dv[:, None] * W3[0][None, :], 0.0)
            k = kdrop("dW2", B)
            dW2 = _mm(dz2[:k].T, h1[:k])
            db2 = wave_sum("db2", dz2)
            k = kdrop("dh1", h1n)
            dz1 = np.where(mask1, _mm(dz2[:, :k], W2_read[:k]), 0.0)
            k = min(kdrop("dW1", B), 48 if mistake == "rows_ge_48" else B)
            dW1 = _mm(dz1[:k].T, x[:k])
            db1 = wave_sum("db1", dz1)
            step_size, bc2_sqrt = scal[s]
            if mistake == "bc2_wrong_step":
                bc2_sqrt = scal[s + 1][1]
            if mistake == "step_size_wrong_step":
                step_size = scal[s + 1][0]
            W2_before_last_step = W2.copy()
            keep = (m[0][:, nf - 1:].copy(), v[0][:, nf - 1:].copy())
            for pi, gi, mi, vi in zip(p, (dW1, db1, dW2, db2, dW3, db3), m, v):
                adam_update(pi, gi, mi, vi, step_size, bc2_sqrt, betas, eps)
            if mistake == "w1_last_col_moments":
                m[0][:, nf - 1:], v[0][:, nf - 1:] = keep
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


# =============================================================================================
# Op-level cases: one launch, shape by shape, against np.longdouble with derived bounds.
#
# The bounds have the shape of entropy_cases.py's (see its docstring for u0 and SLACK): m u0 A,
# A the sum of the absolute values of the terms and m the number of roundings a term can pass
# through in ANY summation order, plus the bound of every computed input times the absolute
# value of what multiplies it.  None uses what an implementation returned.
# =============================================================================================
from entropy_cases import RATIOS, SLACK, U0, bits_equal, check, ld  # noqa: E402
from policy_cases import optim_ref  # noqa: E402

TENSORS = ("W1", "b1", "W2", "b2", "W3", "b3")


def plan(nf, h0, h1, B):
    """critic_fit_kernel's selection lines, restated: fragment counts, k-steps, gather slots,
    the waves at work in each phase and the lanes that own the vectors."""
    up = lambda a, b: -(-a // b)
    nfB, nfH0, nfH1 = up(B, 16), up(h0, 16), up(h1, 16)
    waves = lambda n: frozenset(w for w in range(4) if w < n)
    return dict(nfB=nfB, nfH0=nfH0, nfH1=nfH1, ksB=up(B, 4), ksH0=up(h0, 4), ksH1=up(h1, 4),
                ksF=up(nf, 4), slots=up(B * nf, 256),
                forward=waves(nfB),             # phases B and C, and dh1 of phase D
                dW2=waves(nfH1),                # phase D's dW2 and its Adam, phase E's store
                dW1=waves(nfH0),                # phase E
                owners=dict(b2=(0, h1), W3=(1, h1), b1=(2, h0), b3=(3, 1)))  # wave, lanes


def _ab(a, b):
    """sum |a| |b| of a matrix product, in long double."""
    return np.abs(ld(a)) @ np.abs(ld(b))


def grads_ref(c, step=0):
    """Loss and the six gradients of one mini-batch in long double from the case's f64 inputs,
    each with its bound.  K is a product's inner size, `b*` the bound of `*`:
      z1  = x W1^T + b1              (nf + 1) u0 (|x| |W1|^T + |b1|)
      h1  = z1 [z1 > 0]              bz1 where on (a select: no rounding)
      z2  = h1 W2^T + b2             (h0 + 1) u0 (|h1| |W2|^T + |b2|) + bh1 |W2|^T
      v   = h2 W3^T + b3             (h1 + 1) u0 (|h2| |W3| + |b3|) + bh2 |W3|
      err = v - t                    bv + u0 |err|
      loss = sum err^2 / B           (sum 2 |err| berr + (B + 1) u0 sum err^2) / B: the square,
                                     B - 1 additions and the division
      dv  = 2 err / B                2 berr / B + 2 u0 |dv| (the division; one more for an
                                     implementation that multiplies by a rounded 2 / B)
      dW3 = dv^T h2                  B u0 |dv|^T |h2| + bdv^T |h2| + |dv|^T bh2
      db3 = sum dv                   (B - 1) u0 sum |dv| + sum bdv
      dz2 = dv W3 [z2 > 0]           bdv |W3| + u0 |dz2| where on
      dW2 = dz2^T h1                 B u0 |dz2|^T |h1| + bdz2^T |h1| + |dz2|^T bh1
      db2 = sum_b dz2                (B - 1) u0 sum |dz2| + sum bdz2
      dh1 = dz2 W2                   h1 u0 |dz2| |W2| + bdz2 |W2|;  dz1 = dh1 [z1 > 0]
      dW1 = dz1^T x                  B u0 |dz1|^T |x| + bdz1^T |x|
      db1 = sum_b dz1                (B - 1) u0 sum |dz1| + sum bdz1
    A fused multiply-add chain (the MFMA) rounds less often than the product-then-sum these count,
    and the zeros that pad a fragment add no rounding.  Every finite pre-activation must lie
    further from 0 than its bound unless it is exactly 0 (asserted): then the masks are the same
    in every implementation that meets the bounds."""
    B, nf, h0, h1n = c["B"], c["nf"], c["h0"], c["h1"]
    rows = c["index"][step * B:(step + 1) * B]
    x, t = ld(c["states"][rows]), ld(c["targets"][rows])
    W1, b1, W2, b2, W3, b3 = (ld(a) for a in c["params"])
    w3 = W3[0]
    with np.errstate(all="ignore"):
        z1 = x @ W1.T + b1
        bz1 = (nf + 1) * U0 * (_ab(x, W1.T) + np.abs(b1))
        on1 = z1 > 0
        a1, ba1 = np.where(on1, z1, 0), np.where(on1, bz1, 0)
        z2 = a1 @ W2.T + b2
        bz2 = (h0 + 1) * U0 * (_ab(a1, W2.T) + np.abs(b2)) + ba1 @ np.abs(W2.T)
        on2 = z2 > 0
        a2, ba2 = np.where(on2, z2, 0), np.where(on2, bz2, 0)
        val = a2 @ w3 + b3[0]
        bval = (h1n + 1) * U0 * (_ab(a2, w3) + np.abs(b3[0])) + ba2 @ np.abs(w3)
        err = val - t
        berr = bval + U0 * np.abs(err)
        loss = np.sum(err * err) / B
        bloss = (np.sum(2 * np.abs(err) * berr) + (B + 1) * U0 * np.sum(err * err)) / B
        dv = 2 * err / B
        bdv = 2 * berr / B + 2 * U0 * np.abs(dv)
        dW3 = (dv @ a2)[None, :]
        bdW3 = (B * U0 * _ab(dv, a2) + bdv @ np.abs(a2) + np.abs(dv) @ ba2)[None, :]
        db3 = np.sum(dv)[None]
        bdb3 = ((B - 1) * U0 * np.sum(np.abs(dv)) + np.sum(bdv))[None]
        dz2 = np.where(on2, dv[:, None] * w3[None, :], 0)
        bdz2 = np.where(on2, bdv[:, None] * np.abs(w3)[None, :] + U0 * np.abs(dz2), 0)
        dW2 = dz2.T @ a1
        bdW2 = B * U0 * _ab(dz2.T, a1) + bdz2.T @ np.abs(a1) + np.abs(dz2.T) @ ba1
        db2 = np.sum(dz2, axis=0)
        bdb2 = (B - 1) * U0 * np.sum(np.abs(dz2), axis=0) + np.sum(bdz2, axis=0)
        dh1 = dz2 @ W2
        bdh1 = h1n * U0 * _ab(dz2, W2) + bdz2 @ np.abs(W2)
        dz1, bdz1 = np.where(on1, dh1, 0), np.where(on1, bdh1, 0)
        dW1 = dz1.T @ x
        bdW1 = B * U0 * _ab(dz1.T, x) + bdz1.T @ np.abs(x)
        db1 = np.sum(dz1, axis=0)
        bdb1 = (B - 1) * U0 * np.sum(np.abs(dz1), axis=0) + np.sum(bdz1, axis=0)
    for z, bz in ((z1, bz1), (z2, bz2)):
        near = np.isfinite(z) & (z != 0) & (np.abs(z) <= bz)
        assert not near.any(), "a pre-activation within its bound of 0: reseed the case"
    return dict(loss=loss, bloss=bloss * SLACK, z1=z1, z2=z2,
                g=[dW1, db1, dW2, db2, dW3, db3],
                bg=[b * SLACK for b in (bdW1, bdb1, bdW2, bdb2, bdW3, bdb3)])


def step_ref(c, grads=None):
    """One step's reference: grads_ref, then Adam through policy_cases.optim_ref (its own bounds
    are those of adam_math.hpp's op order from an exact gradient).  The gradient's bound bg is
    added through the update's Lipschitz constants, with w1 = 1 - beta1, w2 = 1 - beta2:
      m' = m + w1 (g - m)                    |dm'/dg| = w1
      v' = b2 v + w2 g^2                     |dv'/dg| = 2 w2 |g|  (+ w2 bg^2, the exact rest)
      sqrt(v')                               |d/dg| = w2 |g| / sqrt(v') <= sqrt(w2), everywhere
      den = sqrt(v') / bc2 + eps             bden = sqrt(w2) bg / bc2
      p' = p - step m' / den                 step (w1 bg / den_lo + |m'| bden / (den den_lo)),
    den_lo = den - bden the smallest denominator a gradient within bg can give (asserted above
    den / 2: otherwise the case must be reseeded)."""
    g = grads or grads_ref(c)
    lr, betas, eps = scalars(c)
    step_size, bc2 = adam_scalars(c["first_step"], 1, lr, betas)[0]
    scal = [1.0, step_size, bc2, betas[0], betas[1], eps]
    w1, w2 = 1 - ld(betas[0]), 1 - ld(betas[1])
    out = dict(loss=g["loss"], bloss=g["bloss"], p=[], bp=[], m=[], bm=[], v=[], bv=[])
    for p, gi, bg, m, v in zip(c["params"], g["g"], g["bg"], c["m"], c["v"]):
        r = optim_ref(0, p, gi, m, v, scal)
        with np.errstate(all="ignore"):
            den = np.sqrt(r.v) / ld(bc2) + ld(eps)
            bden = np.sqrt(w2) * bg / ld(bc2)
            den_lo = den - bden
            assert np.all((bg == 0) | (den_lo > den / 2)), "gradient bound against den: reseed"
            dq = np.where(bg > 0, w1 * bg / den_lo + np.abs(r.m) * bden / (den * den_lo), 0)
        out["p"].append(r.p)
        out["bp"].append(r.bp + ld(step_size) * dq * SLACK)
        out["m"].append(r.m)
        out["bm"].append(r.bm + w1 * bg * SLACK)
        out["v"].append(r.v)
        out["bv"].append(r.bv + (2 * w2 * np.abs(gi) * bg + w2 * bg * bg) * SLACK)
    return out


# ---------------------------------------------------------------------------------------------
# the one-step cases
# ---------------------------------------------------------------------------------------------
SCALAR_SETS = ((LR, BETAS, EPS), (LR, (0.8, 0.99), 1e-6), (3e-3, BETAS, 0.0))
# variant: the three scalar sets on random non-zero moments at step 11, and "g": zero moments
# at step 1, where the returned exp_avg is fl(w1 g): the gradient itself to one more rounding
VARIANTS = ("s0", "s1", "s2", "g")
SHAPE_GROUPS = {
    "batch": [(2, 64, 64, B) for B in (1, 3, 15, 16, 17, 33, 47, 48, 49, 63)],
    "h0": [(2, h, 64, 64) for h in (1, 3, 17, 33, 47, 49, 63)],
    "h1": [(2, 64, h, 64) for h in (1, 3, 17, 33, 47, 49, 63)],
    "features": [(nf, 16, 64, 64) for nf in (3, 4, 5, 8, 9, 12, 13, 15, 16)],
    # 1 x 1 x 1 x 1; the asymmetric pair; every size = 2 mod 4; N = 1 with three rows
    "odd": [(1, 1, 1, 1), (5, 7, 50, 9), (5, 50, 7, 9), (7, 30, 22, 34), (6, 2, 2, 3),
            (2, 64, 64, 64)],
}
SHAPES = tuple(s for grp in SHAPE_GROUPS.values() for s in grp)
N1_SHAPES = ((1, 1, 1, 1), (6, 2, 2, 3))   # N = 1: every index is 0 = N - 1, all duplicates


def _edge_index(rng, B, N):
    """B rows of [0, N) that hold 0, N - 1 and a duplicate, as far as B entries can: B = 1 holds
    N - 1 alone, B = 2 holds 0 and N - 1."""
    idx = rng.integers(0, N, B)
    if B == 1:
        idx[0] = N - 1
    elif B == 2:
        idx[:] = (0, N - 1)
    elif B == 3:
        idx[:] = (0, N - 1, 0)
    else:
        idx[:4] = (0, N - 1, idx[3], idx[3])
        rng.shuffle(idx)
    return idx


def shape_name(shape):
    return "nf%d_h%dx%d_B%d" % shape


@functools.lru_cache(maxsize=None)
def _shape_base(shape):
    """The network, rows and index that the four variants of a shape share."""
    nf, h0, h1, B = shape
    N = 1 if shape in N1_SHAPES else B + 5
    rng = np.random.default_rng([11, nf, h0, h1, B])
    seed = int(rng.integers(1 << 30))
    return _frozen(_build(seed, nf, h0, h1, B, N, index=_edge_index(rng, B, N), first_step=11,
                          moments=True))


def _frozen(c):
    for k in ("states", "targets", "index"):
        c[k].setflags(write=False)
    for k in ("params", "m", "v"):
        for a in c[k]:
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _shape_grads(shape):
    return grads_ref(_shape_base(shape))


@functools.lru_cache(maxsize=None)
def one_step_case(shape, variant):
    c = dict(_shape_base(shape))
    if variant == "g":
        c["m"] = [np.zeros_like(p) for p in c["params"]]
        c["v"] = [np.zeros_like(p) for p in c["params"]]
        c["first_step"] = 1
    else:
        c["lr"], c["betas"], c["eps"] = SCALAR_SETS[VARIANTS.index(variant)]
    c["name"] = shape_name(shape) + ":" + variant
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def one_step_reference(shape, variant):
    return step_ref(one_step_case(shape, variant), _shape_grads(shape))


def launch(ops, dev, c, index=None, state=None, first_step=None, carve=None):
    """One call of ops.critic_fit on `dev`: the case's rows and scalars, `index` (default: the
    case's), parameters and moments from `state` (default: the case's).  loss_out is pre-filled
    with 0xff bytes; states, targets and index must come back as they went.  `carve` (see
    carved()) places the tensors.  Returns fit_reference's form."""
    import torch

    lr, betas, eps = scalars(c)
    index = c["index"] if index is None else np.asarray(index, dtype=np.int32)
    src = c if state is None else state
    n_steps = index.size // c["B"]
    arrays = ([c["states"], c["targets"], index] + list(src["params"]) + list(src["m"])
              + list(src["v"]) + [np.full(n_steps, np.nan)])
    if carve is None:
        t = [torch.from_numpy(np.array(a, copy=True)).to(dev) for a in arrays]
    else:
        t = carve(arrays, dev)
    states, targets, idx, loss = t[0], t[1], t[2], t[21]
    p, m, v = t[3:9], t[9:15], t[15:21]
    loss.view(torch.uint8).fill_(0xFF)
    out = ops.critic_fit(states, targets, idx, c["B"], p, m, v, lr, betas=betas, eps=eps,
                         first_step=c["first_step"] if first_step is None else first_step,
                         loss_out=loss)
    assert out is loss
    for got, want in zip(t[:3], arrays[:3]):
        got, want = got.cpu().numpy(), np.asarray(want)
        assert got.tobytes() == want.tobytes(), "the launch wrote to states, targets or index"
    res = {"params": [x.cpu().numpy() for x in p], "m": [x.cpu().numpy() for x in m],
           "v": [x.cpu().numpy() for x in v], "loss": loss.cpu().numpy()}
    unwritten = res["loss"].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert not unwritten.any(), "a loss_out entry was not written"
    return res


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes()
               for k in ("params", "m", "v") for x, y in zip(a[k], b[k])) and (
                   a["loss"].tobytes() == b["loss"].tobytes())


def check_step(name, got, ref):
    """One launch of one step against step_ref's values, each within its bound."""
    assert got["loss"].shape == (1,)
    check("critic_fit.loss", got["loss"], ref["loss"], ref["bloss"])
    for i, tn in enumerate(TENSORS):
        for key, bkey, label in (("m", "bm", "exp_avg"), ("v", "bv", "exp_avg_sq"),
                                 ("params", "bp", "param")):
            rk = "p" if key == "params" else key
            assert got[key][i].shape == np.shape(ref[rk][i]), (name, tn, key)
            check(f"critic_fit.{label}.{tn}", got[key][i], ref[rk][i], ref[bkey][i])


def run_one_step(ops, dev, shape, variant):
    c = one_step_case(shape, variant)
    got = launch(ops, dev, c)
    check_step(c["name"], got, one_step_reference(shape, variant))
    return got


# ---------------------------------------------------------------------------------------------
# exact case: small integers, planted zeros.  Every product and partial sum is an integer
# multiple of 1 / 16 far below 2^53, so every summation order gives the same gradients exactly;
# Adam's element arithmetic has one op order (adam_math.hpp): all outputs must match bit for bit.
# ---------------------------------------------------------------------------------------------
EXACT_SHAPE = (3, 24, 40, 32)
EXACT_ZERO1, EXACT_ZERO2 = 5, 17   # a unit of each hidden layer whose pre-activation is 0.0


@functools.lru_cache(maxsize=None)
def exact_case():
    nf, h0, h1, B = EXACT_SHAPE
    N = B + 5
    rng = np.random.default_rng(77)
    c = _build(77, nf, h0, h1, B, N, index=_edge_index(rng, B, N), first_step=4, moments=True)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    c["params"] = [ints(-2, 2, (h0, nf)), ints(-1, 2, h0), ints(-1, 1, (h1, h0)),
                   ints(-2, 3, h1), ints(-1, 1, (1, h1)), ints(-1, 1, 1)]
    W1, b1, W2, b2, W3, b3 = c["params"]
    W1[EXACT_ZERO1], b1[EXACT_ZERO1] = 0.0, 0.0
    W2[EXACT_ZERO2], b2[EXACT_ZERO2] = 0.0, 0.0
    W3[0, EXACT_ZERO2] = 1.0
    c["states"] = ints(-2, 2, (N, nf))
    c["targets"] = ints(-3, 3, N)
    c["name"] = "exact_int"
    return _frozen(c)


def run_exact(ops, dev):
    c = exact_case()
    g = grads_ref(c)
    assert (g["z1"][:, EXACT_ZERO1] == 0).all() and (g["z2"][:, EXACT_ZERO2] == 0).all()
    assert (g["z1"] > 0).any() and (g["z2"] > 0).any() and g["g"][0].any()
    for a in g["g"] + [g["loss"] * c["B"]]:  # multiples of 1 / 16 below 2^40: exact in f64
        assert np.all(a * 16 == np.round(a * 16)) and np.all(np.abs(a) < 2.0 ** 40)
    got, ref = launch(ops, dev, c), fit_reference(c)
    assert same_bits(got, ref), "exact_int: bits differ from the exact reference"
    return got


# ---------------------------------------------------------------------------------------------
# multi-step cases: chains, split launches, prefetch boundaries, non-finite data
# ---------------------------------------------------------------------------------------------
def _steps_case(name, seed, shape, n_steps, N, sset=0, replace=True):
    nf, h0, h1, B = shape
    rng = np.random.default_rng(seed)
    index = (rng.integers(0, N, n_steps * B) if replace
             else rng.permutation(N)[:n_steps * B])
    c = _build(seed, nf, h0, h1, B, N, index=index, first_step=7, moments=True)
    c["lr"], c["betas"], c["eps"] = SCALAR_SETS[sset]
    c["name"] = name
    return _frozen(c)


CHAIN_SHAPES = ((3, 24, 40, 5), (5, 7, 50, 9), (5, 50, 7, 9))
CHAIN_NAMES = tuple(f"chain{n}_{shape_name(s)}" for s in CHAIN_SHAPES for n in (8, 40))
SPLIT_NAMES = ("split_ragged", "split_full")
# (kind, value): what the second of three steps reads; NONFINITE_AT is the place in the batch
NONFINITE = {"nan_state": ("state", np.nan), "inf_state": ("state", np.inf),
             "inf_target": ("target", np.inf)}
NONFINITE_AT, NONFINITE_F = 2, 1
UNREAD_ROW = 7


@functools.lru_cache(maxsize=None)
def steps_case(name):
    if name in CHAIN_NAMES:
        i = CHAIN_NAMES.index(name)
        shape, n = CHAIN_SHAPES[i // 2], (8, 40)[i % 2]
        # 8 steps with eps = 0 (set 2), 40 with the other betas (set 1): between them and the
        # existing chain_dense / chain_sparse every scalar set runs for more than one step
        return _steps_case(name, 100 + i, shape, n, 4 * shape[3] + 3, sset=2 - i % 2)
    if name == "split_ragged":   # 5 steps, a different batch in each
        return _steps_case(name, 120, (3, 24, 40, 5), 5, 23, sset=1)
    if name == "split_full":
        return _steps_case(name, 121, (2, 64, 64, 64), 4, 300)
    if name in ("unread_clean", "unread_nonfinite"):
        c = dict(_steps_case(name, 122, (3, 24, 40, 5), 3, 23, replace=False))
        c["index"] = np.array([r if r != UNREAD_ROW else 22 for r in
                               np.random.default_rng(5).permutation(22)[:15]], dtype=np.int32)
        assert UNREAD_ROW not in c["index"]
        if name == "unread_nonfinite":
            c["states"] = c["states"].copy()
            c["states"][UNREAD_ROW] = (np.nan, np.inf, -np.inf)
        return _frozen(c)
    if name in NONFINITE:
        c = dict(_steps_case(name, 123, (3, 24, 40, 5), 3, 23, replace=False))
        row = int(c["index"][c["B"] + NONFINITE_AT])   # read once, in the second step
        assert (c["index"] == row).sum() == 1
        kind, value = NONFINITE[name]
        key = "states" if kind == "state" else "targets"
        c[key] = c[key].copy()
        if kind == "state":
            c[key][row, NONFINITE_F] = value
        else:
            c[key][row] = value
        return _frozen(c)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def steps_reference(name):
    return fit_reference(steps_case(name))


def torch_fit(case):
    """The case's steps through nn.Sequential, autograd and torch.optim.Adam, in f64 on the CPU:
    the loop that the kernel replaces."""
    import torch
    import torch.nn as nn

    nf, h0, h1, B = case["nf"], case["h0"], case["h1"], case["B"]
    lr, betas, eps = scalars(case)
    net = nn.Sequential(nn.Linear(nf, h0), nn.ReLU(), nn.Linear(h0, h1), nn.ReLU(),
                        nn.Linear(h1, 1)).double()
    params = list(net.parameters())
    with torch.no_grad():
        for p, a in zip(params, case["params"]):
            p.copy_(torch.from_numpy(a.copy()))
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
    if case["first_step"] > 1 or any(a.any() for a in case["m"] + case["v"]):
        for p, m, v in zip(params, case["m"], case["v"]):
            opt.state[p] = {"step": torch.tensor(float(case["first_step"] - 1)),
                            "exp_avg": torch.from_numpy(m.copy()),
                            "exp_avg_sq": torch.from_numpy(v.copy())}
    states, targets = torch.from_numpy(case["states"].copy()), torch.from_numpy(
        case["targets"].copy()).unsqueeze(1)
    index = torch.from_numpy(case["index"].astype(np.int64))
    loss_out = []
    for s in range(index.numel() // B):
        rows = index[s * B:(s + 1) * B]
        opt.zero_grad()
        loss = torch.mean((net(states[rows]) - targets[rows]) ** 2)
        loss.backward()
        opt.step()
        loss_out.append(float(loss.detach()))
    return {"params": [p.detach().numpy() for p in params],
            "m": [opt.state[p]["exp_avg"].numpy() for p in params],
            "v": [opt.state[p]["exp_avg_sq"].numpy() for p in params],
            "loss": np.array(loss_out)}


SPREAD_FACTOR = 100.0
# (absolute on parameters and moments, relative on the loss): how far two honest references of
# each chain lie apart, the long-double stand-in and torch's f64 autograd loop on the CPU, as
# measured by chain_spread() when the cases were written (test_critic_cases_host.py measures
# them again and fails if one has grown past these figures).
CHAIN_SPREADS = {
    "chain8_nf3_h24x40_B5": (1.111e-16, 3.628e-16), "chain40_nf3_h24x40_B5": (3.331e-16, 6.333e-16),
    "chain8_nf5_h7x50_B9": (1.111e-16, 1.559e-16), "chain40_nf5_h7x50_B9": (6.662e-16, 3.660e-16),
    "chain8_nf5_h50x7_B9": (1.111e-16, 2.048e-16), "chain40_nf5_h50x7_B9": (4.441e-16, 3.016e-16),
}


@functools.lru_cache(maxsize=None)
def chain_spread(name):
    """The spread of CHAIN_SPREADS, measured now."""
    return max_deviation(torch_fit(steps_case(name)), steps_reference(name))


def chain_tolerance(name):
    """What an implementation may deviate from the stand-in over a chain: SPREAD_FACTOR x the
    spread between the two references (another summation order, not another algorithm; the
    margin of test_gpu_trpo.py's CG floors), and never more than the old flat 1e-12."""
    dev, rel = CHAIN_SPREADS[name]
    return min(SPREAD_FACTOR * dev, GPU_ATOL), min(SPREAD_FACTOR * rel, GPU_LOSS_RTOL)


CHAIN_DEVIATIONS = {}   # name -> (abs, loss rel) of the last run_chain


def run_chain(ops, dev, name):
    got = launch(ops, dev, steps_case(name))
    d, rel = max_deviation(got, steps_reference(name))
    atol, rtol = chain_tolerance(name)
    CHAIN_DEVIATIONS[name] = (d, rel, atol, rtol)
    print(f"{name}: max abs {d:.3e} (allowed {atol:.3e}), loss rel {rel:.3e} ({rtol:.3e})")
    assert d <= atol and rel <= rtol, (name, d, atol, rel, rtol)
    return got


def sub_state(res):
    return {k: res[k] for k in ("params", "m", "v")}


def run_split(ops, dev, name):
    """A launch of s steps and one of n - s from where it stopped equal the launch of n steps,
    bit for bit, for every s."""
    c = steps_case(name)
    B, n = c["B"], c["index"].size // c["B"]
    whole = launch(ops, dev, c)
    for s in range(1, n):
        a = launch(ops, dev, c, index=c["index"][:s * B])
        b = launch(ops, dev, c, index=c["index"][s * B:], state=sub_state(a),
                   first_step=c["first_step"] + s)
        b["loss"] = np.concatenate([a["loss"], b["loss"]])
        assert same_bits(b, whole), f"{name}: split after step {s} differs from one launch"
    return whole


@functools.lru_cache(maxsize=None)
def step_references(name):
    """Per step s: grads_ref's loss and bound of batch s at the stand-in's state before it."""
    c = steps_case(name)
    B, n = c["B"], c["index"].size // c["B"]
    out, state = [], sub_state(c)
    for s in range(n):
        one = dict(c, index=c["index"][s * B:(s + 1) * B], first_step=c["first_step"] + s,
                   **state)
        g = grads_ref(one)
        out.append((g["loss"], g["bloss"]))
        state = sub_state(fit_reference(one))
    return out


def run_prefetch(ops, dev, name):
    """Launches of 1, 2, 3 and 4 steps (the first launch's load_idx(1) and each load_idx(s + 2)
    present or not): every step's loss is its own batch's."""
    c = steps_case(name)
    B = c["B"]
    refs = step_references(name)
    for n in range(1, 5):
        got = launch(ops, dev, c, index=c["index"][:n * B])
        assert got["loss"].shape == (n,)
        for s in range(n):
            check("critic_fit.loss.step", got["loss"][s:s + 1], refs[s][0], refs[s][1])


def carved(guard_words=3):
    """A `carve` for launch(): every tensor a contiguous view into ONE flat allocation filled
    with 0xff bytes, `guard_words` or one more 8-byte guard words before, between and after them,
    so that some views start at 16-byte aligned offsets and some at 8-byte-only ones.  Returns
    (carve, verify); verify() asserts every guard byte is still 0xff and that both alignments
    occurred."""
    import torch

    box = {}

    def carve(arrays, dev):
        arrays = [np.ascontiguousarray(a) for a in arrays]
        offs, off = [], 8 * guard_words
        for i, a in enumerate(arrays):
            offs.append(off)
            off += -(-a.nbytes // 8) * 8 + 8 * (guard_words + i % 2)
        flat = torch.full((off,), 0xFF, dtype=torch.uint8, device=dev)
        views = []
        for a, o in zip(arrays, offs):
            tt = torch.from_numpy(a.copy())
            view = flat[o:o + a.nbytes].view(tt.dtype).view(tt.shape)
            view.copy_(tt)
            assert view.data_ptr() == flat.data_ptr() + o and view.is_contiguous()
            views.append(view)
        assert flat.data_ptr() % 16 == 0
        box.update(flat=flat, spans=[(o, o + a.nbytes) for a, o in zip(arrays, offs)])
        return views

    def verify():
        host = box["flat"].cpu().numpy()
        keep = np.ones(host.size, dtype=bool)
        for lo, hi in box["spans"]:
            keep[lo:hi] = False
        assert (host[keep] == 0xFF).all(), "a guard byte next to a tensor was written"
        assert {lo % 16 for lo, _ in box["spans"]} == {0, 8}

    return carve, verify


CANARY_CASES = (((1, 1, 1, 1), "s0"), ((5, 7, 50, 9), "s1"), ((5, 50, 7, 9), "s2"),
                ((2, 64, 64, 17), "g"), ((16, 16, 64, 64), "s0"), ((2, 64, 1, 64), "s1"))


def run_canary(ops, dev, c):
    carve, verify = carved()
    got = launch(ops, dev, c, carve=carve)
    verify()
    assert same_bits(got, launch(ops, dev, c)), "carved tensors gave other bits"
    return got


def finite_pattern(res):
    """{'loss': tuple of bools, tensor key: 'finite' | 'all' | ('cols', ...) | ('mixed', n)}:
    where a result is non-finite, tensor by tensor."""
    out = {"loss": tuple(bool(x) for x in np.isfinite(res["loss"]))}
    for key in ("params", "m", "v"):
        for tn, a in zip(TENSORS, res[key]):
            bad = ~np.isfinite(a)
            if not bad.any():
                continue
            if bad.all():
                out[f"{key}.{tn}"] = "all"
            elif a.ndim == 2 and all(col.all() or not col.any() for col in bad.T):
                out[f"{key}.{tn}"] = ("cols",) + tuple(int(i) for i in np.where(bad[0])[0])
            else:
                out[f"{key}.{tn}"] = ("mixed", int(bad.sum()))
    return out


def run_nonfinite(ops, dev, name):
    """A non-finite value in a row that the second of three steps reads: the result's nan and
    inf positions are the select-ReLU restatement's (check() compares them exactly), the finite
    rest meets the old flat tolerance, and the pattern is the pinned one."""
    c, ref = steps_case(name), steps_reference(name)
    got = launch(ops, dev, c)
    check(f"critic_fit.{name}", got["loss"], ref["loss"], GPU_LOSS_RTOL * np.abs(ref["loss"]))
    for key in ("params", "m", "v"):
        for a, b in zip(got[key], ref[key]):
            check(f"critic_fit.{name}", a, b, GPU_ATOL)
    assert finite_pattern(got) == NONFINITE_PIN[name], (name, finite_pattern(got))
    return got


def _pin(loss, **tensors):
    out = {"loss": loss}
    for tn, what in tensors.items():
        out.update({f"{key}.{tn}": what for key in ("params", "m", "v")})
    return out


# What comes back non-finite (finite_pattern's form; a tensor not named is finite), the same for
# the parameter and both of its moments.  The kernel's ReLU is a select, (z > 0) ? z : 0, so a
# NaN pre-activation is an inactive unit:
#   nan_state   the row's h1 is 0, its value and the loss stay finite; dW1 = dz1^T x puts 0 * NaN
#               into W1's column of that feature; from then on every z1 is NaN, the first layer is
#               off and every loss is finite again.  Nothing but that column shows it.
#   inf_state   the same, and W2's columns of the units that the row drove to +inf (dW2 = dz2^T h1
#               with dz2 = 0 there: 0 * inf).
#   inf_target  the step's loss is inf and the next one's NaN; what a dead unit's zero gradient
#               shields stays finite: W2's rows and b2 of the units that were off in that row.
# torch's loop (relu(NaN) = NaN) reports a non-finite loss from the second step on and returns
# every tensor NaN throughout in all three: TORCH_PIN.
_INF_COLS = ("cols", 1, 2, 3, 5, 6, 7, 9, 12, 13, 17, 19)
NONFINITE_PIN = {
    "nan_state": _pin((True, True, True), W1=("cols", NONFINITE_F)),
    "inf_state": _pin((True, True, True), W1=("cols", NONFINITE_F), W2=_INF_COLS),
    "inf_target": _pin((True, False, False), W1="all", b1="all", W2=("mixed", 864),
                       b2=("mixed", 36), W3="all", b3="all"),
}
TORCH_PIN = _pin((True, False, False), **{tn: "all" for tn in TENSORS})


def run_all(ops, dev):
    """Every op-level case through `ops` on `dev` (the host test's runner; the GPU test calls
    the same run_* functions one group at a time)."""
    for shape in SHAPES:
        for variant in VARIANTS:
            run_one_step(ops, dev, shape, variant)
    run_exact(ops, dev)
    for shape, variant in CANARY_CASES:
        run_canary(ops, dev, one_step_case(shape, variant))
    run_canary(ops, dev, steps_case("split_ragged"))
    for name in SPLIT_NAMES:
        run_split(ops, dev, name)
        run_prefetch(ops, dev, name)
    assert same_bits(launch(ops, dev, steps_case("unread_clean")),
                     launch(ops, dev, steps_case("unread_nonfinite")))
    for name in NONFINITE:
        run_nonfinite(ops, dev, name)
    for name in CHAIN_NAMES:
        run_chain(ops, dev, name)


def stand_in_ops(mistake=None):
    """An `ops` whose critic_fit is fit_reference, with one planted mistake or none."""
    import types

    import torch

    def critic_fit(states, targets, index, batch, params, exp_avg, exp_avg_sq, lr,
                   betas=BETAS, eps=EPS, first_step=1, loss_out=None):
        n = lambda t: t.detach().cpu().numpy()
        W1, W2 = params[0], params[2]
        c = dict(nf=W1.shape[1], h0=W1.shape[0], h1=W2.shape[0], B=batch, N=states.shape[0],
                 states=n(states), targets=n(targets), index=n(index),
                 params=[n(t) for t in params], m=[n(t) for t in exp_avg],
                 v=[n(t) for t in exp_avg_sq], first_step=first_step, lr=lr, betas=betas, eps=eps)
        out = fit_reference(c, mistake=mistake)
        for key, lst in (("params", params), ("m", exp_avg), ("v", exp_avg_sq)):
            for t, a in zip(lst, out[key]):
                t.copy_(torch.from_numpy(a))
        if loss_out is None:
            return torch.from_numpy(out["loss"])
        loss_out.copy_(torch.from_numpy(out["loss"]))
        return loss_out

    return types.SimpleNamespace(critic_fit=critic_fit)
