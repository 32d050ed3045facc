"""Cases, 80-bit references and error bounds for the Gaussian head, input layer and optimizer ops.

TEST INFRASTRUCTURE ONLY (host code; torch is imported lazily and nothing here needs a GPU).

The kernels of csrc/head.hip (head_forward, head_backward), csrc/mlp.hip (layer_forward,
layer_backward, layer_tangent) and csrc/optim.hip (optim_step) are tested op by op, the way
tests/entropy_cases.py tests the entropy kernels: every case goes through an `ops`-shaped module
(tests/cpu_ops.py on the CPU, mepol_amd.ops on the GPU) and every output is compared with a
reference computed here in np.longdouble from the formulas in the kernels' header comments and in
oracle/mepol_oracle.py (gaussian_logp).

The bounds have the shape of entropy_cases.py's (see its docstring for u0, LIBM and SLACK): m u0 A
with A the sum of the absolute values of the terms on the output's path and m the number of
roundings on it for ANY summation order, LIBM per exp call, the product with SLACK, plus the
propagated bound of an input that was itself computed.  A sum of n terms whose accumulator starts
at an exact 0, or that also adds exact zeros (padded lanes, padded actions, empty waves, empty
record groups), has the same bound: adding 0 does not round.  Every derivation stands next to its
bound; none uses what an implementation returned.

The ReLU masks are exact: fl(a + b) is 0 only when a + b is, and has its sign otherwise, so
[z + bz > 0] is the same in f64 and in 80-bit; h of layer_backward / layer_tangent is an input.
The generators still assert that no pre-activation lies within its own bound of 0, except where a
case puts it at exactly 0.0.
"""
import functools
import math
import types

import numpy as np

from entropy_cases import LD, LIBM, RATIOS, SLACK, U0, _n, _t, bits_equal, check, ld

STD_EPS = 1e-7                       # kStdEps of csrc/mfma_f64.hpp
LOG2PI = np.log(2 * ld(np.pi))       # 80-bit; the kernels hold its f64 rounding (see blogp)
F64_MAX = ld(np.finfo(np.float64).max)

# name -> (elements whose bits differ from the numpy restatement's, elements compared); run_optim
# records it.  Two nans count as equal: which nan an invalid operation returns is the machine's
# choice (x86 sets the sign bit of inf - inf, other hardware does not).
OPTIM_BITS = {}


def _mm(a, b):
    """80-bit matrix product (numpy's own loops: there is no BLAS for longdouble)."""
    return np.matmul(np.ascontiguousarray(ld(a)), np.ascontiguousarray(ld(b)))


def _mmb(a, b):
    """The same product in f64, for the sums of absolute values inside the bounds only: all terms
    are >= 0, so its relative error (a few hundred u0) is far inside SLACK."""
    return ld(np.matmul(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))


# =============================================================================================
# The launchers' selection lines, restated (csrc/head.hip, csrc/mlp.hip): what the coverage
# assertions of tests/test_policy_cases_host.py count.
# =============================================================================================
def head_fwd_instance(H, A):
    """(AP, NCL, NCH) of head_fwd16_kernel that mepol_head_forward launches."""
    ap = 1 if A <= 1 else 2 if A <= 2 else 4 if A <= 4 else 8
    nch = (A + 7) // 8
    ncl16 = (H + 15) // 16
    ncl = next(v for v in (4, 8, 12, 16, 20, 24, 32) if ncl16 <= v)
    return ap, ncl, nch


def head_bwd_instance(H, A):
    """("narrow", AP, NC) of head_bwd_kernel or ("wide", AP, block width) of the wide kernel."""
    if A > 8:
        return "wide", next(v for v in (12, 16, 20, 24, 32) if A <= v), (H + 63) // 64 * 64
    return "narrow", 1 if A <= 1 else 2 if A <= 2 else 4 if A <= 4 else 8, (H + 63) // 64


def head_bwd_records(n):
    """Partial records (blocks) of the head backward: 128 rows per block at least, 512 at most."""
    return max(1, min(512, ((n + 31) // 32 + 3) // 4))


def layer_fp(F):
    """FP of MEPOL_FP_SWITCH: the padded feature count the layer kernels are compiled for."""
    return next(v for v in (2, 4, 8, 16, 32, 64) if F <= v)


# =============================================================================================
# References with their bounds (SimpleNamespaces of longdouble arrays: value x, bound bx)
# =============================================================================================
def _sigma_terms(log_std):
    """sigma = exp(ls) + 1e-7 and what the kernels derive from it, with relative bounds.
    e = exp(ls): LIBM.  sigma = e + 1e-7: one rounding, and e <= sigma, so LIBM + u0.
    inv = 1 / (sigma sigma): twice sigma's error, a product, a division: 2 LIBM + 4 u0 (d d /
    (sigma sigma) has the same count).  es3 = e / (sigma sigma sigma): LIBM for e, three times
    sigma's error, two products, a division: 4 LIBM + 6 u0."""
    ls = ld(log_std)
    e = np.exp(ls)
    sigma = e + ld(STD_EPS)
    return types.SimpleNamespace(ls=ls, inv=1 / (sigma * sigma), rinv=2 * LIBM + 4 * U0,
                                 es3=e / (sigma * sigma * sigma), res3=4 * LIBM + 6 * U0)


def _relu_in(z, bz):
    """x = relu(z + bz) with its bound: one rounding of the sum when there is a bz, none else.
    The relu is the select [pre > 0] ? pre : 0, as the kernels' fmax(pre, 0.0) and their masks
    are: a nan pre-activation gives 0 (tests/gemm_cases.py has such inputs; no case here does)."""
    pre = ld(z) + ld(bz) if bz is not None else ld(z)
    with np.errstate(invalid="ignore"):
        x = np.where(pre > 0, pre, 0)
    return pre, x, (U0 if bz is not None else 0 * U0)


def head_fwd_ref(z, bz, Wm, bm, log_std, act, dz_in=None):
    """mu_ia = sum_c x_ic Wm_ac + bm_a, x = relu(z + bz): H + 1 terms.  Each product carries x's
    rounding (with a bz) and its own (none under fma: looser, never tighter), then at most H adds
    whatever the order (16 lanes of strided columns, a 4-step exchange, the bias last): m = H + 2,
    A = sum_c |x Wm| + |bm|.
    logp_i = sum_a -0.5 t_a, t_a = K_a + q_a, K_a = log 2pi + 2 ls_a (the product by 2 is exact;
    one add; the f64 constant is within u0 log 2pi of log 2pi), q_a = d^2 inv_a, d = act - mu^:
    |d^ - d| <= bmu + u0 |d|, the square doubles it and rounds once, the product with inv adds
    inv's relative bound and one rounding; t_a rounds once; the product by -0.5 is exact; the A
    terms are summed in any order (A - 1 adds; A = 1: the sum is the term).
    dz_in [n, H]: the bound of a z that was itself computed (tests/gemm_cases.py: the z2 of
    policy_forward).  The sum with bz and the relu move a value by no more than their input
    moved, so mu's bound grows by sum_c dz_in_ic |Wm_ac|, and logp's follows through bmu."""
    n, H = z.shape
    A = Wm.shape[0]
    pre, x, ux = _relu_in(z, bz)
    W = ld(Wm)
    mu = _mm(x, W.T) + ld(bm)
    Amu = _mmb(x, np.abs(W).T) + np.abs(ld(bm))
    bmu = (H + 2) * U0 * Amu * SLACK if bz is not None else (H + 1) * U0 * Amu * SLACK
    if dz_in is not None:
        bmu = bmu + _mmb(dz_in, np.abs(W).T) * SLACK
    s = _sigma_terms(log_std)
    K = LOG2PI + 2 * s.ls
    bK = U0 * (np.abs(K) + LOG2PI)
    d = ld(act) - mu
    bd = bmu + U0 * np.abs(d)
    q = d * d * s.inv
    bq = s.inv * (2 * np.abs(d) * bd + U0 * d * d) + q * (s.rinv + U0)
    t = K + q
    bt = bK + bq + U0 * np.abs(t)
    logp = np.sum(-0.5 * t, axis=1)
    blogp = (np.sum(0.5 * bt, axis=1) + (A - 1) * U0 * np.sum(0.5 * np.abs(t), axis=1)) * SLACK
    return types.SimpleNamespace(mu=mu, bmu=bmu, logp=logp, blogp=blogp, pre=pre)


def head_bwd_ref(g, z, bz, Wm, log_std, act, mu, dmu_in=None):
    """The head's backward from grad_logp g [n] and the forward's mu (an input; dmu_in bounds its
    error in the chained case, where the reference holds the exact mu).

    d = act - mu: one rounding (+ dmu_in).  dmu_ia = g d inv_a: two products and inv's relative
    bound: |dmu| (rinv + 3 u0) + |g| inv dmu_in.
    dbm_a = sum_i dmu_ia: n - 1 adds in any order (rows strided over waves, waves in order,
    block records in strided groups, the groups in order), A = sum_i |dmu_ia|: cancellation is
    paid for by the absolute sum, not by the result.
    dlog_std_a = sum_i g_i s_i, s = -1 + q, q = d^2 es3_a: d's rounding twice, the square, the
    product with es3 and es3's relative bound (res3 + 4 u0, + dmu_in through 2 |d| es3); s and
    g s round once each; n - 1 adds, A = sum_i |g s|.
    dWm_ac = sum_i dmu_ia x_ic: x's rounding (with a bz) and the product's on top of dmu's; n - 1
    adds, A = sum_i |dmu x|.
    dz_ic = [z + bz > 0] sum_a dmu_ia Wm_ac: a_dim terms, each with dmu's bound and one product
    rounding, a_dim - 1 adds (the fma chain starts at an exact 0): a few u0.
    dbz_c = sum_i dz_ic: the dz bounds and n - 1 adds, A = sum_i |dz_ic|."""
    n, H = z.shape
    A = Wm.shape[0]
    pre, x, ux = _relu_in(z, bz)
    W, g = ld(Wm), ld(g).reshape(n, 1)
    s = _sigma_terms(log_std)
    din = np.zeros((n, A), LD) if dmu_in is None else ld(dmu_in)
    d = ld(act) - ld(mu)
    dmu = g * d * s.inv
    bdm = np.abs(dmu) * (s.rinv + 3 * U0) + np.abs(g) * s.inv * din
    dbm = np.sum(dmu, axis=0)
    bdbm = (np.sum(bdm, axis=0) + (n - 1) * U0 * np.sum(np.abs(dmu), axis=0)) * SLACK
    q = d * d * s.es3
    sq = -1 + q
    t = g * sq
    bt = (np.abs(g) * (q * (s.res3 + 4 * U0) + 2 * np.abs(d) * din * s.es3 + U0 * np.abs(sq))
          + U0 * np.abs(t))
    dls = np.sum(t, axis=0)
    bdls = (np.sum(bt, axis=0) + (n - 1) * U0 * np.sum(np.abs(t), axis=0)) * SLACK
    dWm = _mm(dmu.T, x)
    AW = _mmb(np.abs(dmu).T, x)
    bdWm = (_mmb(bdm.T, x) + (ux + U0) * AW + (n - 1) * U0 * AW) * SLACK
    mask = pre > 0
    dz = np.where(mask, _mm(dmu, W), 0)
    Az = _mmb(np.abs(dmu), np.abs(W))
    bdz = np.where(mask, _mmb(bdm, np.abs(W)) + U0 * Az + (A - 1) * U0 * Az, 0) * SLACK
    dbz = np.sum(dz, axis=0)
    bdbz = (np.sum(bdz, axis=0) + (n - 1) * U0 * np.sum(np.abs(dz), axis=0)) * SLACK
    return types.SimpleNamespace(dz=dz, bdz=bdz, dWm=dWm, bdWm=bdWm, dbm=dbm, bdbm=bdbm, dls=dls,
                                 bdls=bdls, dbz=dbz, bdbz=bdbz, pre=pre)


def layer_fwd_ref(x, W, b):
    """pre_ic = b_c + sum_f x_if W_cf: F + 1 terms, a rounding per product and F adds: m = F + 1,
    A = |b| + sum_f |x W|.  h = relu(pre): the maximum does not round."""
    F = x.shape[1]
    pre = _mm(x, ld(W).T) + ld(b)
    A = _mmb(np.abs(x), np.abs(W).T) + np.abs(ld(b))
    return types.SimpleNamespace(pre=pre, h=np.maximum(pre, 0), bh=(F + 1) * U0 * A * SLACK)


def layer_tangent_ref(x, dW, db, h):
    """t = [h > 0] (db + x dW^T): layer_fwd_ref's sum with the mask read from the input h."""
    r = layer_fwd_ref(x, dW, db)
    m = np.asarray(h) > 0
    return types.SimpleNamespace(t=np.where(m, r.pre, 0), bt=np.where(m, r.bh, 0))


def layer_bwd_ref(dh, h, x):
    """dzz = dh [h > 0] (exact: a select).  dW_cf = sum_i dzz_ic x_if: a rounding per product and
    n - 1 adds in any order (rows over 4 waves, chunks, row blocks, the blocks in order): m = n,
    A = sum_i |dzz x|.  db_c = sum_i dzz_ic: n - 1 adds, A = sum_i |dzz|."""
    n = x.shape[0]
    dzz = np.where(np.asarray(h) > 0, ld(dh), 0)
    dW = _mm(dzz.T, x)
    bdW = n * U0 * _mmb(np.abs(dzz).T, np.abs(x)) * SLACK
    db = np.sum(dzz, axis=0)
    bdb = (n - 1) * U0 * np.sum(np.abs(dzz), axis=0) * SLACK
    return types.SimpleNamespace(dW=dW, bdW=bdW, db=db, bdb=bdb)


def _f64_range(x):
    """An 80-bit value beyond the f64 range is the infinity that f64 arithmetic gives there."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > F64_MAX, np.sign(x) * ld(np.inf), x)


def optim_ref(kind, p, g, m, v, scal):
    """One step of csrc/optim.hip's op sequence in 80-bit from f64 inputs, one rounding per op:
    Adam   m' = m + w1 (g - m), w1 = 1 - b1: the roundings of w1, of g - m and of the product
              (3 u0 |w1 (g - m)|) and of the sum (u0 |m'|).
           v' = v b2 + w2 (g g): u0 |v b2|, 3 u0 w2 g g (w2, the square, the product), u0 v'.
           den = sqrt(v') / bc2 + eps: half of v''s relative bound through the square root, the
              root's and the division's roundings, then the sum's.
           p' = p + (-step) (m' / den): m''s and den's relative bounds, the division, the
              product, the sum.
    RMSprop v' the same with alpha; den = sqrt(v') + eps; p' = p + (-lr) (g / den).
    A few u0 per output.  Values past the f64 range are the infinities f64 gives (g g of 1e200),
    and what follows from them (den = inf, p' = p; g = inf: p' = nan) must be met exactly."""
    p, g, v, sc = ld(p), ld(g), ld(v), ld(scal)
    with np.errstate(all="ignore"):
        if kind == 0:
            step, bc2, b1, b2, eps = sc[1], sc[2], sc[3], sc[4], sc[5]
            m = ld(m)
            w1 = 1 - b1
            dm = w1 * (g - m)
            m1 = _f64_range(m + dm)
            bm = 3 * U0 * np.abs(dm) + U0 * np.abs(m1)
            num = m1
        else:
            step, b2, eps = sc[1], sc[2], sc[3]
            bc2 = ld(1)
            m1, bm, num = None, 0 * U0, g
        w2 = 1 - b2
        gg = _f64_range(g * g)
        v1 = _f64_range(v * b2 + w2 * gg)
        bv = U0 * np.abs(v * b2) + 3 * U0 * w2 * gg + U0 * v1
        ok = np.isfinite(v1) & (v1 > 0)
        relv = np.where(ok, bv / np.where(ok, v1, 1), 0)
        root = np.sqrt(v1) / bc2
        den = root + eps
        fin = np.isfinite(den)
        bden = np.where(fin, root * (relv / 2 + (2 if kind == 0 else 1) * U0) + U0 * den, 0)
        rden = np.where(fin, 1 / np.where(fin, den, 1), 0)
        q = num / den
        bq = bm * rden + np.abs(q) * (bden * rden + U0)
        p1 = p + (-step) * q
        bp = np.abs(step) * (bq + U0 * np.abs(q)) + U0 * np.abs(p1)
    return types.SimpleNamespace(p=p1, bp=bp * SLACK, m=m1, bm=bm * SLACK, v=v1, bv=bv * SLACK)


# =============================================================================================
# Case generators (seeded; plain numpy arrays)
# =============================================================================================
HEAD_FWD_A = (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32)
HEAD_FWD_H = (1, 15, 16, 17, 64, 65, 128, 129, 192, 193, 256, 257, 300, 320, 321, 384, 385, 511,
              512)
HEAD_BWD_NARROW_A = (1, 2, 3, 4, 5, 7, 8)
HEAD_BWD_NARROW_H = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300, 320, 321, 384, 385, 448,
                     449, 512)
HEAD_BWD_WIDE_A = (9, 12, 13, 16, 17, 20, 21, 24, 25, 32)
HEAD_BWD_WIDE_H = (1, 64, 65, 300, 512)
HEAD_CROSS_N = 37
HEAD_SWEEP_SHAPES = ((300, 2), (33, 3), (300, 17), (512, 32))   # (H, A)
HEAD_FWD_SWEEP_N = (1, 2, 3, 4, 5, 63, 64, 65, 517, 4100)
HEAD_BWD_SWEEP_N = (1, 2, 3, 31, 32, 33, 128, 129, 517, 1025, 4100)


def head_case(name, n, H, A, seed, spread=False, zero_pos=False, zero_row=None):
    """z [n, H], bz [H], Wm [A, H] of order 1 / sqrt(H), bm, log_std in [-1, 0.5] (spread: over
    [-16, 1], where the 1e-7 of sigma is up to 47% of it), act, and grad_logp g with mixed signs
    and exact zeros in every fifth row (n > 1).  zero_pos: z[r, c] = -bz[c] exactly at a few
    (r, c), the first and the last column among them, so relu(0) = 0 with a bz; without a bz the
    same positions hold z = 0.0.  zero_row: that row of z is all zeros."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, H))
    bz = 0.5 * rng.standard_normal(H)
    Wm = rng.standard_normal((A, H)) / math.sqrt(H)
    bm = 0.1 * rng.standard_normal(A)
    if spread:
        log_std = rng.permutation(np.linspace(-16.0, 1.0, A)) if A > 1 else np.array([-16.0])
    else:
        log_std = rng.uniform(-1.0, 0.5, A)
    act = rng.standard_normal((n, A))
    g = rng.standard_normal(n)
    if n > 1:
        g[::5] = 0.0  # (a one-row batch keeps its one non-zero g)
    pos = ()
    if zero_pos:
        pos = tuple(sorted({(0, 0), (n - 1, H - 1), (n // 2, H // 2), (n - 1, 0), (1 % n, H - 1)}))
    if zero_row is not None:
        z[zero_row] = 0.0
    return types.SimpleNamespace(name=name, n=n, H=H, A=A, z=z, bz=bz, Wm=Wm, bm=bm,
                                 log_std=log_std, act=act, g=g, zero_pos=pos, zero_row=zero_row)


def head_inputs(c, with_bz):
    """(z, bz or None) of the case: the exact-zero positions follow the variant."""
    z = c.z.copy()
    for r, col in c.zero_pos:
        z[r, col] = -c.bz[col] if with_bz else 0.0
    return z, (c.bz if with_bz else None)


def _assert_masks_decided(c, pre, with_bz):
    """No pre-activation within its bound (u0 (|z| + |bz|), one rounding) of 0 but the exact
    zeros that the case sets; those are there, and the mask is false on them."""
    z, bz = head_inputs(c, with_bz)
    mag = np.abs(z) + (np.abs(bz) if with_bz else 0)
    zero = np.zeros(pre.shape, bool)
    for r, col in c.zero_pos:
        zero[r, col] = True
    if c.zero_row is not None and not with_bz:
        zero[c.zero_row] = True
    assert np.all(pre[zero] == 0), c.name
    assert np.all(np.abs(pre[~zero]) > 4 * U0 * ld(mag[~zero])), c.name


@functools.lru_cache(maxsize=None)
def head_fwd_cases():
    out, i = [], 0
    for A in HEAD_FWD_A:
        for H in HEAD_FWD_H:
            out.append(head_case(f"x_A{A}_H{H}", HEAD_CROSS_N, H, A, 1000 + i))
            i += 1
    for H, A in HEAD_SWEEP_SHAPES:
        for n in HEAD_FWD_SWEEP_N:
            out.append(head_case(f"n{n}_H{H}_A{A}", n, H, A, 2000 + i))
            i += 1
    out.append(head_case("spread_A8", HEAD_CROSS_N, 300, 8, 2900, spread=True))
    out.append(head_case("spread_A17", HEAD_CROSS_N, 300, 17, 2901, spread=True))
    out.append(head_case("zero_pos_A3", HEAD_CROSS_N, 65, 3, 2902, zero_pos=True))
    out.append(head_case("zero_pos_A17", HEAD_CROSS_N, 300, 17, 2903, zero_pos=True))
    out.append(head_case("zero_row_A2", 9, 33, 2, 2904, zero_row=6))
    out.append(head_case("zero_row_A17", 9, 300, 17, 2905, zero_row=8))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def head_bwd_cases():
    out, i = [], 0
    for A in HEAD_BWD_NARROW_A:
        for H in HEAD_BWD_NARROW_H:
            out.append(head_case(f"x_A{A}_H{H}", HEAD_CROSS_N, H, A, 3000 + i))
            i += 1
    for A in HEAD_BWD_WIDE_A:
        for H in HEAD_BWD_WIDE_H:
            out.append(head_case(f"x_A{A}_H{H}", HEAD_CROSS_N, H, A, 3000 + i))
            i += 1
    for H, A in HEAD_SWEEP_SHAPES:
        for n in HEAD_BWD_SWEEP_N:
            out.append(head_case(f"n{n}_H{H}_A{A}", n, H, A, 4000 + i))
            i += 1
    out.append(head_case("spread_A8", HEAD_CROSS_N, 300, 8, 4900, spread=True))
    out.append(head_case("spread_A17", HEAD_CROSS_N, 300, 17, 4901, spread=True))
    out.append(head_case("zero_pos_A3", HEAD_CROSS_N, 65, 3, 4902, zero_pos=True))
    out.append(head_case("zero_pos_A17", HEAD_CROSS_N, 300, 17, 4903, zero_pos=True))
    out.append(head_case("zero_row_A2", 9, 33, 2, 4904, zero_row=6))
    out.append(head_case("zero_row_A17", 9, 300, 17, 4905, zero_row=8))
    return {c.name: c for c in out}


def _groups(cases, actions, sweep_n):
    """Test-sized groups of head cases: one per action count of the cross products, one per
    shape of the row sweeps, one of the special cases."""
    groups = {f"cross_A{A}": [k for k in cases if k.startswith(f"x_A{A}_")] for A in actions}
    for H, A in HEAD_SWEEP_SHAPES:
        groups[f"rows_H{H}_A{A}"] = [f"n{n}_H{H}_A{A}" for n in sweep_n]
    groups["special"] = [k for k in cases if k.startswith(("spread", "zero"))]
    assert sorted(sum(groups.values(), [])) == sorted(cases)
    return groups


def head_fwd_groups():
    return _groups(head_fwd_cases(), HEAD_FWD_A, HEAD_FWD_SWEEP_N)


def head_bwd_groups():
    return _groups(head_bwd_cases(), HEAD_BWD_NARROW_A + HEAD_BWD_WIDE_A, HEAD_BWD_SWEEP_N)


HEAD_CHAIN = ("n517_H300_A2", "n517_H300_A17", "spread_A8", "spread_A17")


@functools.lru_cache(maxsize=None)
def head_fwd_reference(name, with_bz):
    c = head_fwd_cases()[name]
    z, bz = head_inputs(c, with_bz)
    ref = head_fwd_ref(z, bz, c.Wm, c.bm, c.log_std, c.act)
    _assert_masks_decided(c, ref.pre, with_bz)
    return ref


@functools.lru_cache(maxsize=None)
def _head_bwd_mu(name, with_bz):
    c = head_bwd_cases()[name]
    z, bz = head_inputs(c, with_bz)
    pre = ld(z) + ld(bz) if with_bz else ld(z)
    return np.asarray(_mm(np.maximum(pre, 0), ld(c.Wm).T) + ld(c.bm), dtype=np.float64)


def head_bwd_mu(c, with_bz):
    """The mu handed to the backward as an input: the forward's 80-bit mu rounded to f64."""
    return _head_bwd_mu(c.name, with_bz)


@functools.lru_cache(maxsize=None)
def head_bwd_reference(name, with_bz):
    c = head_bwd_cases()[name]
    z, bz = head_inputs(c, with_bz)
    ref = head_bwd_ref(c.g, z, bz, c.Wm, c.log_std, c.act, head_bwd_mu(c, with_bz))
    _assert_masks_decided(c, ref.pre, with_bz)
    for r, col in c.zero_pos:
        assert ref.dz[r, col] == 0
    return ref


@functools.lru_cache(maxsize=None)
def head_chain_reference(name, with_bz):
    """head_forward then head_backward on its mu: the backward reference from the exact mu, the
    forward's bound carried into it."""
    c = head_bwd_cases()[name]
    z, bz = head_inputs(c, with_bz)
    f = head_fwd_ref(z, bz, c.Wm, c.bm, c.log_std, c.act)
    return f, head_bwd_ref(c.g, z, bz, c.Wm, c.log_std, c.act, f.mu, dmu_in=f.bmu)


LAYER_F = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
LAYER_H = (1, 63, 64, 65, 300)
LAYER_N = (1, 3, 5, 17, 63, 64, 65, 517)
LAYER_TWO_CHUNKS = (16449, 2, 64)   # (n, F, H): 256 row blocks x 64 rows + 65


def layer_shapes():
    """(n, F, H): F_i with n_(i + j), j = 0, 1, 2, and H_(i + j): every F and every H with at
    least three n, every n with at least two F (asserted in the host test)."""
    out = []
    for i, F in enumerate(LAYER_F):
        for j in range(3):
            n, H = LAYER_N[(i + 3 * j) % len(LAYER_N)], LAYER_H[(i + 2 * j) % len(LAYER_H)]
            out.append((n, F, H))
    return out + [LAYER_TWO_CHUNKS]


def layer_case(n, F, H, seed):
    """x [n, F], W [H, F], b, and for the backward h (the forward reference rounded to f64: an
    exact input) and dh, non-zero everywhere, so h == 0 meets dh != 0 in about half the entries;
    the tangent's direction (dW, db).  layer_reference asserts that no pre-activation lies within
    its bound of 0."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, F))
    W = rng.standard_normal((H, F)) / math.sqrt(F)
    b = 0.3 * rng.standard_normal(H)
    dh = rng.standard_normal((n, H))
    dh[dh == 0] = 1.0
    dW = rng.standard_normal((H, F))
    db = rng.standard_normal(H)
    return types.SimpleNamespace(name=f"n{n}_F{F}_H{H}", n=n, F=F, H=H, x=x, W=W, b=b, dh=dh,
                                 dW=dW, db=db)


@functools.lru_cache(maxsize=None)
def layer_cases():
    return {c.name: c for c in (layer_case(n, F, H, 5000 + i)
                                for i, (n, F, H) in enumerate(layer_shapes()))}


@functools.lru_cache(maxsize=None)
def layer_reference(name):
    c = layer_cases()[name]
    f = layer_fwd_ref(c.x, c.W, c.b)
    assert np.all(np.abs(f.pre) > f.bh), name  # no pre-activation within its bound of 0
    h = np.asarray(f.h, dtype=np.float64)
    assert np.any((h == 0) & (c.dh != 0)) or c.n * c.H < 4
    return types.SimpleNamespace(fwd=f, h=h, bwd=layer_bwd_ref(c.dh, h, c.x),
                                 tan=layer_tangent_ref(c.x, c.dW, c.db, h))


OPTIM_SIZES = {
    1: [262145],
    8: [0, 1, 255, 256, 257, 262145, 7, 64],
    9: [257, 0, 1, 255, 256, 3, 5, 9, 262145],
    16: [1, 0, 255, 256, 257, 3, 5, 9, 64, 0, 2, 100, 262145, 31, 257, 0],
}
# per step: Adam (step_size, bc2_sqrt, beta1, beta2, eps); RMSprop (lr, alpha, eps)
OPTIM_SCALARS = {0: [(3.1e-3, 0.0316, 0.9, 0.999, 1e-8), (1.6e-3, 0.0447, 0.8, 0.99, 1e-6),
                     (-2.0e-3, 0.0547, 0.95, 0.9999, 1e-10)],
                 1: [(1e-2, 0.99, 1e-8), (3e-3, 0.9, 1e-6), (-1e-3, 0.999, 1e-10)]}
OPTIM_SNAPS = ("pmv", "p-v", "-m-", None)   # which snapshot lists are given ("-": None)
# every pattern under both kinds, every tensor count with a snapshot
OPTIM_CASE_SNAPS = {1: ("pmv", "p-v"), 8: ("p-v", None), 9: ("-m-", "pmv"), 16: ("pmv", None)}


def optim_case(kind, count, snaps, seed):
    """`count` tensors of OPTIM_SIZES, three steps of gradients.  The first tensor of >= 255
    elements holds the special entries in every step: [0] g = 0 with v = 0 (and m = 0), [1] g =
    1e200 (g g overflows: v' = inf, den = inf, p' = p), [2] g = inf (m' = v' = inf, p' = nan)."""
    rng = np.random.default_rng(seed)
    sizes = OPTIM_SIZES[count]
    p = [rng.standard_normal(s) for s in sizes]
    m = [0.1 * rng.standard_normal(s) for s in sizes]
    v = [0.01 * rng.random(s) for s in sizes]
    gs = [[rng.standard_normal(s) * 10.0 ** rng.integers(-3, 2) for s in sizes] for _ in range(3)]
    sp = next(i for i, s in enumerate(sizes) if s >= 255)
    m[sp][0] = v[sp][0] = 0.0
    for g in gs:
        g[sp][0], g[sp][1], g[sp][2] = 0.0, 1e200, np.inf
    return types.SimpleNamespace(name=f"{'adam' if kind == 0 else 'rmsprop'}_{count}_{snaps}",
                                 kind=kind, count=count, sizes=sizes, p=p, m=m, v=v, gs=gs,
                                 snaps=snaps, special=sp)


@functools.lru_cache(maxsize=None)
def optim_cases():
    out, i = [], 0
    for kind in (0, 1):
        for count, patterns in OPTIM_CASE_SNAPS.items():
            for snaps in patterns:
                out.append(optim_case(kind, count, snaps, 6000 + i))
                i += 1
    return {c.name: c for c in out}


# =============================================================================================
# Runners: one case through an `ops`-shaped module, every output checked
# =============================================================================================
def _nan(shape, dev):
    import torch

    return torch.full(shape, float("nan"), dtype=torch.float64, device=dev)


def run_head_forward(ops, dev, c, with_bz, ref=None):
    """head_forward into nan-filled outputs (every element is written) and into fresh ones."""
    ref = ref if ref is not None else head_fwd_reference(c.name, with_bz)
    z, bz = head_inputs(c, with_bz)
    args = [_t(x, dev) for x in (z, c.Wm, c.bm, c.log_std, c.act)]
    bzt = _t(bz, dev) if with_bz else None
    mu_out, logp_out = _nan((c.n, c.A), dev), _nan((c.n,), dev)
    mu, logp = ops.head_forward(*args, bz=bzt, mu_out=mu_out, logp_out=logp_out)
    assert mu.data_ptr() == mu_out.data_ptr() and logp.data_ptr() == logp_out.data_ptr()
    check("mu", _n(mu), ref.mu, ref.bmu)
    check("logp", _n(logp), ref.logp, ref.blogp)
    mu2, logp2 = ops.head_forward(*args, bz=bzt)
    assert bits_equal(mu, mu2) and bits_equal(logp, logp2), "outputs depend on the buffers"
    return dict(mu=mu, logp=logp)


def check_head_backward(got, ref, with_bz, need_dz=True, sfx=""):
    dz, dWm, dbm, dls, dbz = got[:5]
    if need_dz:
        check("dz" + sfx, _n(dz), ref.dz, ref.bdz)
        assert np.all(_n(dz)[np.asarray(ref.pre <= 0)] == 0), "dz is not 0 where z + bz <= 0"
    else:
        assert dz is None
    check("dWm" + sfx, _n(dWm), ref.dWm, ref.bdWm)
    check("dbm" + sfx, _n(dbm), ref.dbm, ref.bdbm)
    check("dlog_std" + sfx, _n(dls), ref.dls, ref.bdls)
    if with_bz:
        check("dbz" + sfx, _n(dbz), ref.dbz, ref.bdbz)
    else:
        assert dbz is None


def run_head_backward(ops, dev, c, with_bz, ref=None, streams=False):
    """head_backward as one call, checked; then its variants, each with the one call's bits:
    need_dz=False, nan-filled outs= with a nan-filled caller-owned ws, and (streams: the GPU
    only) reduce_stream= and defer_reduce=True."""
    import torch

    ref = ref if ref is not None else head_bwd_reference(c.name, with_bz)
    z, bz = head_inputs(c, with_bz)
    g, zt, Wm, ls, act, mu = [_t(x, dev) for x in (c.g, z, c.Wm, c.log_std, c.act,
                                                    head_bwd_mu(c, with_bz))]
    bzt = _t(bz, dev) if with_bz else None
    one = ops.head_backward(g, zt, Wm, ls, act, mu, bz=bzt)
    assert len(one) == 5
    check_head_backward(one, ref, with_bz)
    names = ("dz", "dWm", "dbm", "dlog_std", "dbz")

    def same(other, what, dz=True):
        for k, a, b in zip(names, one, other):
            if k == "dz" and not dz:
                assert b is None, what
            else:
                assert bits_equal(a, b), (what, k)

    same(ops.head_backward(g, zt, Wm, ls, act, mu, bz=bzt, need_dz=False), "need_dz=False", False)
    outs = (_nan((c.A, c.H), dev), _nan((c.A,), dev), _nan((c.A,), dev),
            _nan((c.H,), dev) if with_bz else None)
    ws = None
    if hasattr(ops, "head_workspace"):
        ws = ops.head_workspace(c.n, c.H, c.A, zt.device)
        ws.fill_(255)  # all bits set: every double of it is a nan
    got = ops.head_backward(g, zt, Wm, ls, act, mu, bz=bzt, ws=ws, outs=outs)
    for a, b in zip(got[1:], outs):
        assert (a is None and b is None) or a.data_ptr() == b.data_ptr()
    same(got, "outs= and ws=")
    if streams:
        side = torch.cuda.Stream()
        got = ops.head_backward(g, zt, Wm, ls, act, mu, bz=bzt, reduce_stream=side)
        torch.cuda.current_stream().wait_stream(side)
        same(got, "reduce_stream=")
        *got, finish = ops.head_backward(g, zt, Wm, ls, act, mu, bz=bzt, defer_reduce=True)
        finish()
        same(got, "defer_reduce=True")
    return dict(zip(names, one))


def run_head_chain(ops, dev, c, with_bz):
    """head_forward, then head_backward on the mu it returned."""
    f, b = head_chain_reference(c.name, with_bz)
    z, bz = head_inputs(c, with_bz)
    g, zt, Wm, bm, ls, act = [_t(x, dev) for x in (c.g, z, c.Wm, c.bm, c.log_std, c.act)]
    bzt = _t(bz, dev) if with_bz else None
    mu, logp = ops.head_forward(zt, Wm, bm, ls, act, bz=bzt)
    check("mu", _n(mu), f.mu, f.bmu)
    check("logp", _n(logp), f.logp, f.blogp)
    got = ops.head_backward(g, zt, Wm, ls, act, mu, bz=bzt)
    check_head_backward(got, b, with_bz, sfx="_chained")
    return got


def run_layer(ops, dev, c, ref=None):
    """layer_forward (nan-filled out), layer_backward on the reference's h, layer_tangent."""
    ref = ref if ref is not None else layer_reference(c.name)
    x, W, b, dh, h, dW, db = [_t(v, dev) for v in (c.x, c.W, c.b, c.dh, ref.h, c.dW, c.db)]
    out = _nan((c.n, c.H), dev)
    hk = ops.layer_forward(x, W, b, out=out)
    assert hk.data_ptr() == out.data_ptr()
    check("h", _n(hk), ref.fwd.h, ref.fwd.bh)
    assert bits_equal(hk, ops.layer_forward(x, W, b))
    gW, gb = ops.layer_backward(dh, h, x, dW_out=_nan((c.H, c.F), dev), db_out=_nan((c.H,), dev))
    check("dW1", _n(gW), ref.bwd.dW, ref.bwd.bdW)
    check("db1", _n(gb), ref.bwd.db, ref.bwd.bdb)
    t = ops.layer_tangent(x, dW, db, h, out=_nan((c.n, c.H), dev))
    check("t1", _n(t), ref.tan.t, ref.tan.bt)
    assert np.all(_n(t)[ref.h <= 0] == 0)
    return dict(h=hk, dW=gW, db=gb, t=t)


def _snap_lists(c, dev):
    if c.snaps is None:
        return None
    return tuple([_nan((s,), dev) for s in c.sizes] if ch != "-" else None for ch in c.snaps)


def run_optim(ops, dev, c):
    """Three steps with changing scalars and gradients, then one with scal[0] == 0.  Every step
    is checked against optim_ref of the state the step started from (the f64 tensors as they
    stood: they are that step's inputs, and optim_ref's bounds come from them and the scalars);
    the snapshots hold that state bit for bit; lists not given (and the exp_avg snapshot under
    RMSprop) stay untouched.  The same steps through cpu_ops.optim_step, the numpy restatement
    of the kernel's op sequence, from the same start: OPTIM_BITS records how many elements
    differ in their bits."""
    import cpu_ops
    import torch

    adam = c.kind == 0
    p, m, v = ([_t(x.copy(), dev) for x in lst] for lst in (c.p, c.m, c.v))
    rp, rm, rv = ([torch.as_tensor(x.copy()) for x in lst] for lst in (c.p, c.m, c.v))
    differ, compared = 0, 0
    for step in range(4):
        live = step < 3
        sc = np.array([1.0 if live else 0.0, *OPTIM_SCALARS[c.kind][step % 3]])
        gs = c.gs[step % 3]
        g = [_t(x, dev) for x in gs]
        before = [[_n(t).copy() for t in lst] for lst in (p, m, v)]
        snaps = _snap_lists(c, dev)
        ops.optim_step(c.kind, p, g, m if adam else None, v, _t(sc, dev), snapshot=snaps)
        for i in range(c.count):
            if live:
                r = optim_ref(c.kind, before[0][i], gs[i], before[1][i], before[2][i], sc)
                check("optim_p", _n(p[i]), r.p, r.bp)
                check("optim_v", _n(v[i]), r.v, r.bv)
                if adam:
                    check("optim_m", _n(m[i]), r.m, r.bm)
            else:
                assert bits_equal(p[i].cpu(), torch.as_tensor(before[0][i])), "scal[0] == 0: p"
                assert bits_equal(v[i].cpu(), torch.as_tensor(before[2][i])), "scal[0] == 0: v"
            if not live or not adam:
                assert bits_equal(m[i].cpu(), torch.as_tensor(before[1][i])), "m changed"
            for k, lst in enumerate(snaps or ()):
                if lst is None:
                    continue
                if live and (adam or k != 1):
                    assert bits_equal(lst[i].cpu(), torch.as_tensor(before[k][i])), (
                        "snapshot is not the value from before the update", k, i)
                else:
                    assert bool(torch.isnan(lst[i]).all()), ("snapshot written", k, i, step)
        if live:
            cpu_ops.optim_step(c.kind, rp, [torch.as_tensor(x) for x in gs], rm if adam else None,
                               rv, torch.as_tensor(sc))
            for a, b in zip(p + v + (m if adam else []), rp + rv + (rm if adam else [])):
                a, b = _n(a), _n(b)
                differ += int(np.sum((a.view(np.int64) != b.view(np.int64))
                                     & ~(np.isnan(a) & np.isnan(b))))
                compared += a.size
    OPTIM_BITS[c.name] = (differ, compared)
    return p, m, v


# =============================================================================================
# Every case through one backend, and the table of the largest error / bound per output:
#   python tests/policy_cases.py cpu|gpu [out.json]
# =============================================================================================
def run_all(ops, dev, streams=False):
    for c in head_fwd_cases().values():
        for with_bz in (True, False):
            run_head_forward(ops, dev, c, with_bz)
    for c in head_bwd_cases().values():
        for with_bz in (True, False):
            run_head_backward(ops, dev, c, with_bz, streams=streams)
    for name in HEAD_CHAIN:
        for with_bz in (True, False):
            run_head_chain(ops, dev, head_bwd_cases()[name], with_bz)
    for c in layer_cases().values():
        run_layer(ops, dev, c)
    for c in optim_cases().values():
        run_optim(ops, dev, c)


if __name__ == "__main__":
    import json
    import os
    import sys
    import time

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time()
    if sys.argv[1] == "gpu":
        import torch

        from mepol_amd import ops as gpu_ops

        backend = (gpu_ops, torch.device("cuda"))
        run_all(*backend, streams=True)
    else:
        import cpu_ops as host_ops

        backend = (host_ops, "cpu")
        run_all(*backend)
    for key in sorted(RATIOS):
        print(f"{key:18s} {RATIOS[key]:.4f}")
    bits = sorted(OPTIM_BITS.items())
    print(f"# optimizer bits equal the numpy restatement's in {sum(b[0] == 0 for _, b in bits)} of "
          f"{len(bits)} cases" + "".join(f"\n#   {k}: {b[0]} of {b[1]} elements differ"
                                         for k, b in bits if b[0]))
    print(f"# {sys.argv[1]}: all cases within bounds, {time.time() - t0:.1f} s")
    overall = dict(RATIOS)
    # the same figure at the largest shape of each family alone
    headline = {
        "head_forward n4100_H512_A32": lambda: run_head_forward(
            *backend, head_fwd_cases()["n4100_H512_A32"], True),
        "head_backward n4100_H512_A32": lambda: run_head_backward(
            *backend, head_bwd_cases()["n4100_H512_A32"], True),
        "head_backward n4100_H300_A2": lambda: run_head_backward(
            *backend, head_bwd_cases()["n4100_H300_A2"], True),
        "head chain spread_A17": lambda: run_head_chain(
            *backend, head_bwd_cases()["spread_A17"], True),
        "layer n16449_F2_H64": lambda: run_layer(*backend, layer_cases()["n16449_F2_H64"]),
    }
    large = {}
    for title, fn in headline.items():
        RATIOS.clear()
        fn()
        large[title] = dict(RATIOS)
        print(f"{title:30s} " + "  ".join(f"{k} {v:.2g}" for k, v in sorted(RATIOS.items())))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w", encoding="utf-8") as f:
            json.dump({"overall": overall, "largest_shapes": large, "optim_bits": dict(bits)}, f,
                      indent=1, sort_keys=True)
