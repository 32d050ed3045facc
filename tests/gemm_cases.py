"""Cases, 80-bit references and error bounds for the f64 matrix-core (MFMA) GEMM kernels.

TEST INFRASTRUCTURE ONLY (host code; torch is imported lazily and nothing here needs a GPU).

The kernels of csrc/gemm.hip (gemm_nt, dh1_layer1_backward, hidden_backward, hidden_tangent),
csrc/wgrad.hip (weight_grad) and csrc/policy_fwd.hip (policy_forward) are tested op by op, the way
tests/policy_cases.py tests the head: every case goes through an `ops`-shaped module
(tests/cpu_ops.py on the CPU, mepol_amd.ops on the GPU) and every output is compared with a
reference computed here in np.longdouble.

The bounds have the shape of entropy_cases.py's (see its docstring for u0 and SLACK): m u0 A.  A
sum of K products formed in any order, with or without fused multiply-add, 4 k at a time by
v_mfma_f64_16x16x4f64, over K-slices, waves, row-block records and record groups, has every
term pass through at most one product rounding and K - 1 adds (the first add is to an exact 0):
m = K, or K + 1 with a bias added, and A = the sum of the absolute values of the terms.  Adding
exact zeros (padded k, padded rows, empty slices and groups) does not round.  An output computed
from a computed input carries that input's bound through the absolute values of what multiplies
it.  Every derivation stands next to its bound; none uses what an implementation returned.

Every ReLU and every mask is a select in the reference, [pre > 0] ? v : 0, as in the kernels
(fmax(v, 0.0) and `on ? v : 0.0`): a masked-off nan or inf is 0, and so is the relu of a nan
pre-activation; its mask bit is 0.  A pre-activation that is not finite is the same non-finite
value in f64 whatever the order of the sum (one infinity stays, two of opposite sign or 0 x inf
give nan in any order), so the select's result there is exact and its bound is 0.  The generators
assert that no finite computed pre-activation lies within its own bound of 0, except in the cases
built from small integers, where every partial sum is exact in any order and a pre-activation of
exactly 0.0 is meant.

dh1_layer1_backward's x is finite in every case: the kernel assumes it (include/mepol_amd.h).
"""
import functools
import math
import types

import numpy as np

from entropy_cases import LD, RATIOS, SLACK, U0, _n, _t, bits_equal, check, ld
from policy_cases import _mm, _mmb, head_fwd_ref

NS = types.SimpleNamespace
GEMM_VARIANTS = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10)
DZ_SCALE, W_SCALE = 1e-7, 0.05   # the workload's own magnitudes: dz ~ 1e-7, weights ~ 0.05


# =============================================================================================
# The launchers' selection lines, restated (csrc/gemm.hip, policy_fwd.hip, wgrad.hip): what the
# coverage assertions of tests/test_gemm_cases_host.py count.
# =============================================================================================
GEMM_TILES = {0: (2, 2, 4, 5), 1: (4, 2, 2, 5), 2: (2, 2, 2, 5), 3: (4, 1, 2, 10), 5: (2, 2, 4, 4),
              6: (2, 4, 2, 5), 7: (4, 1, 2, 5), 8: (2, 5, 2, 5), 9: (8, 1, 2, 5), 10: (4, 2, 2, 4)}


def gemm_tile(variant):
    """(BM, BN) of the variant's workgroup tile: WR FR 16 rows by WC FC 16 columns."""
    wr, wc, fr, fc = GEMM_TILES[variant]
    return wr * fr * 16, wc * fc * 16


def policy_fwd_instance(in_features, hidden0, h1_aligned, row_tile):
    """(FP band, form) that mepol_policy_forward_tiled launches: "split64/32/16" (layer1_kernel
    + z2_head_kernel<4/2/1>), "one_vec" (policy_fwd_kernel<FP, true>: even hidden0, h1_out not
    16-B aligned) or "one_odd" (policy_fwd_kernel<FP, false>)."""
    fp = next(v for v in (4, 8, 16, 32, 48, 64) if in_features <= v)
    if hidden0 % 2 == 0 and h1_aligned:
        tile = row_tile if row_tile else 16  # (the automatic tile of a batch under 4097 rows)
        return fp, f"split{tile}"
    return fp, "one_vec" if hidden0 % 2 == 0 else "one_odd"


def dh1_nh(in_features):
    """NH of dh1_layer1_bwd_kernel: 16-column groups of [x | 1]."""
    return min(4, (in_features + 1 + 15) // 16)


def k_tiles(k):
    """k-tiles of 16 of gemm_mainloop (the DEEP loop takes them in pairs plus a lone last one)."""
    return (k + 15) // 16


def row_blocks(n):
    """256-row blocks (records of sum_records) of dh1_layer1_backward and hidden_backward."""
    return (n + 255) // 256


# =============================================================================================
# References with their bounds
# =============================================================================================
def _gt0(v):
    with np.errstate(invalid="ignore"):
        return v > 0


def _relu(pre, b):
    """([pre > 0] ? pre : 0, its bound): the select moves a value by no more than its input
    moved; a pre-activation that is not finite is exact (module docstring)."""
    return np.where(_gt0(pre), pre, 0), np.where(np.isfinite(pre), b, 0)


def _masked(on, v, b):
    return np.where(on, v, 0), np.where(on, b, 0)


def _prod(a, b, m_extra=0, carry_a=None):
    """a [n, K] b^T [m, K] in 80-bit with the bound (K + m_extra) u0 |a| |b|^T (+ carry_a
    |b|^T for an `a` that carries the bound carry_a); the sum of absolute values too."""
    K = a.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        v = _mm(a, ld(b).T)
        A = _mmb(np.abs(a), np.abs(b).T)
        bound = (K + m_extra) * U0 * A
        if carry_a is not None:
            bound = bound + _mmb(carry_a, np.abs(b).T)
    return v, bound, A


def gemm_nt_ref(A, B, bias, relu):
    """C = act(A B^T + bias): K terms and the bias, m = K (+ 1), A = sum |A B| (+ |bias|)."""
    K = A.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        v, _, Ab = _prod(A, B)
        m = K
        if bias is not None:
            v, Ab, m = v + ld(bias), Ab + np.abs(ld(bias)), K + 1
        b = m * U0 * Ab * SLACK
    if relu:
        v, b = _relu(v, b)
    return NS(c=v, bc=b)


def _assert_decided(name, pre, bound, exact):
    """No finite pre-activation within its bound of 0; in an `exact` case (small integers) an
    exact 0 is allowed, and there is at least one."""
    fin = np.isfinite(pre)
    near = fin & (np.abs(np.where(fin, pre, 1)) <= np.where(fin, bound, 0))
    if exact:
        assert np.any(pre == 0), (name, "no pre-activation of exactly 0")
        near &= pre != 0
    assert not near.any(), (name, "a pre-activation lies within its bound of 0")


def policy_forward_ref(c):
    """pre1 = x W1^T + b1: F + 1 terms, m = F + 1.  h1 = relu(pre1).  z2 = h1 W2^T: H0 terms,
    m = H0, and h1's bound through |W2|.  pre2 = z2 + b2 rounds once; mu and logp are
    head_fwd_ref's with z2's bound passed in.  mask = [pre1 > 0]."""
    with np.errstate(invalid="ignore", over="ignore"):
        pre1, _, A1 = _prod(c.x, c.W1)
        pre1 = pre1 + ld(c.b1)
        b1 = (c.F + 1) * U0 * (A1 + np.abs(ld(c.b1))) * SLACK
        _assert_decided(c.name + " pre1", pre1, b1, c.exact)
        h1, bh1 = _relu(pre1, b1)
        z2, bz2, _ = _prod(h1, c.W2, carry_a=bh1)
        bz2 = bz2 * SLACK
        pre2 = z2 + ld(c.b2)
        _assert_decided(c.name + " pre2", pre2, bz2 + U0 * np.abs(pre2), c.exact)
        head = head_fwd_ref(z2, c.b2, c.Wm, c.bm, c.log_std, c.act,
                            dz_in=np.where(np.isfinite(bz2), bz2, 0))
    return NS(h1=h1, bh1=bh1, z2=z2, bz2=bz2, mu=head.mu, bmu=head.bmu, logp=head.logp,
              blogp=head.blogp, mask=_gt0(pre1))


def dh1_ref(dz2, W2t, on, x):
    """dh1 = dz2 W2 (K terms, m = K), dz1 = [on] ? dh1 : 0.  dW1_cf = sum_r dz1_rc x_rf: n terms,
    m = n on top of dz1's bound through |x|.  db1_c = sum_r dz1_rc (the product with the 1 of
    [x | 1] is exact): n - 1 adds on top of dz1's bound."""
    n = dz2.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        dh1, bdh1, _ = _prod(dz2, W2t)
        dz1, bdz1 = _masked(on, dh1, bdh1)
        dW, bdW, _ = _prod(dz1.T, np.asarray(x).T, carry_a=bdz1.T)
        db = np.sum(dz1, axis=0)
        bdb = np.sum(bdz1, axis=0) + (n - 1) * U0 * np.sum(np.abs(dz1), axis=0)
    return NS(dW=dW, bdW=bdW * SLACK, db=db, bdb=bdb * SLACK, A_db=np.sum(np.abs(dz1), axis=0))


def weight_grad_ref(dy, x):
    """dW_oi = sum_r dy_ro x_ri: n terms in any order over the K-slices: m = n."""
    with np.errstate(invalid="ignore", over="ignore"):
        dW, b, A = _prod(np.asarray(dy).T, np.asarray(x).T)
    return NS(dW=dW, bdW=b * SLACK, A=A)


def hidden_backward_ref(dz_out, W, h_in):
    """dz_in = [h_in > 0] ? dz_out W : 0 (K = out terms, m = K); db_c = sum_r dz_in_rc: n - 1
    adds on top of dz_in's bound."""
    n = dz_out.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        v, b, _ = _prod(dz_out, np.asarray(W).T)
        dz, bdz = _masked(_gt0(ld(h_in)), v, b)
        db = np.sum(dz, axis=0)
        bdb = np.sum(bdz, axis=0) + (n - 1) * U0 * np.sum(np.abs(dz), axis=0)
    return NS(dz=dz, bdz=bdz * SLACK, db=db, bdb=bdb * SLACK)


def hidden_tangent_ref(c):
    """t = [mask_src + mask_bias > 0] ? t_in W^T + h_in dW^T + db : 0: the two products share
    one accumulator, 2 K terms and db: m = 2 K + 1.  The mask's sum rounds once: no finite
    mask_src + mask_bias within u0 (|mask_src| + |mask_bias|) of 0 but the exact zeros."""
    K = c.t_in.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        v1, _, A1 = _prod(c.t_in, c.W)
        v2, _, A2 = _prod(c.h_in, c.dW)
        v = v1 + v2 + ld(c.db)
        b = (2 * K + 1) * U0 * (A1 + A2 + np.abs(ld(c.db))) * SLACK
        pre = ld(c.mask_src) + (ld(c.mask_bias) if c.mask_bias is not None else 0)
        mag = np.abs(ld(c.mask_src)) + (np.abs(ld(c.mask_bias)) if c.mask_bias is not None else 0)
    fin = np.isfinite(pre)
    near = fin & (pre != 0) & (np.abs(np.where(fin, pre, 1)) <= 4 * U0 * np.where(fin, mag, 0))
    assert not near.any(), c.name
    t, bt = _masked(_gt0(pre), v, b)
    return NS(t=t, bt=bt, pre=pre)


# =============================================================================================
# Case generators (seeded; plain numpy arrays)
# =============================================================================================
def _poison(arr, spot, value):
    """value at an interior element ("mid") or at the last row's last column ("last"): the
    element every clamped load re-reads."""
    arr = np.array(arr, dtype=np.float64)
    idx = tuple(s // 2 for s in arr.shape) if spot == "mid" else tuple(s - 1 for s in arr.shape)
    arr[idx] = value
    return arr


POISONS = tuple((spot, value) for value in (np.inf, np.nan) for spot in ("mid", "last"))


def _ptag(operand, spot, value):
    return f"{operand}_{'inf' if np.isinf(value) else 'nan'}_{spot}"


def _relu_like(rng, shape):
    """A ReLU output as a mask source: about half zeros, a 0.0 and a -0.0 at fixed places (the
    first and the last element) whatever the draw."""
    h = np.maximum(rng.standard_normal(shape), 0.0)
    h.flat[0] = -0.0
    h.flat[-1] = 0.0
    if h.size > 2:
        h.flat[h.size // 2] = -0.0
    return h


# ---- gemm_nt --------------------------------------------------------------------------------
def gemm_case(name, n, k, m, seed, variant=0, bias=True, relu=False, work=False, strided=False,
              poison=None):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k)) * (DZ_SCALE if work else 1.0)
    B = rng.standard_normal((m, k)) * (W_SCALE if work else 1.0)
    bv = rng.standard_normal(m) * (DZ_SCALE * W_SCALE if work else 1.0)
    c = NS(name=name, n=n, k=k, m=m, variant=variant, A=A, B=B, bias=bv if bias else None,
           relu=relu, strided=strided)
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, _poison(getattr(c, operand), spot, value))
    return c


GEMM_BIG = (257, 18, 401)   # > 1 row block and a ragged last column block for every tiling
GEMM_K = (2, 16, 18, 32, 34)
GEMM_SMALL = (83, 18, 85)


@functools.lru_cache(maxsize=None)
def gemm_cases():
    out, s = [], 7000
    for v in GEMM_VARIANTS:
        for work in (False, True):
            s += 1
            out.append(gemm_case(f"v{v}_{'work' if work else 'unit'}", *GEMM_BIG, s, variant=v,
                                 relu=True, work=work))
        s += 1
        out.append(gemm_case(f"v{v}_strided", *GEMM_BIG, s, variant=v, strided=True))
    for v in (0, 2):
        s += 1
        out.append(gemm_case(f"v{v}_1x2x1", 1, 2, 1, s, variant=v))
        for k in GEMM_K:
            s += 1
            out.append(gemm_case(f"v{v}_k{k}", 67, k, 85, s, variant=v, work=k == 34))
        for bias in (False, True):
            for relu in (False, True):
                s += 1
                out.append(gemm_case(f"v{v}_bias{int(bias)}_relu{int(relu)}", *GEMM_SMALL, s,
                                     variant=v, bias=bias, relu=relu))
        for operand in ("A", "B", "bias"):
            for spot, value in POISONS:
                s += 1
                out.append(gemm_case(f"v{v}_" + _ptag(operand, spot, value), *GEMM_SMALL, s,
                                     variant=v, relu=operand == "bias",
                                     poison=(operand, spot, value)))
    return {c.name: c for c in out}


def gemm_groups():
    names = list(gemm_cases())
    g = {f"variant{v}": [k for k in names if k.startswith(f"v{v}_") and "inf" not in k
                         and "nan" not in k] for v in GEMM_VARIANTS}
    g["containment"] = [k for k in names if "_inf_" in k or "_nan_" in k]
    assert sorted(sum(g.values(), [])) == sorted(names)
    return g


@functools.lru_cache(maxsize=None)
def gemm_reference(name):
    c = gemm_cases()[name]
    return gemm_nt_ref(c.A, c.B, c.bias, c.relu)


# ---- policy_forward -------------------------------------------------------------------------
PF_F = (1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64)
PF_N, PF_H0, PF_H1 = 83, (10, 11), 34
PF_ACTIONS = (1, 4, 5, 8, 9, 17)
PF_FORMS = ("split64", "split32", "split16", "one_vec", "one_odd")


def pf_case(name, F, h0, h1w, A, seed, n=PF_N, work=False, exact=False, poison=None):
    rng = np.random.default_rng(seed)
    ws = W_SCALE if work else 1.0
    if exact:  # small integers: every partial sum of pre1 and of z2 + b2 is exact in any order
        x = rng.integers(-2, 3, (n, F)).astype(np.float64)
        W1 = rng.integers(-2, 3, (h0, F)).astype(np.float64)
        b1 = rng.integers(-1, 2, h0).astype(np.float64)
        W2 = rng.integers(-1, 2, (h1w, h0)).astype(np.float64)
        b2 = rng.integers(-2, 3, h1w).astype(np.float64)
    else:
        x = rng.standard_normal((n, F))
        W1 = rng.standard_normal((h0, F)) / math.sqrt(F) * ws
        b1 = 0.3 * rng.standard_normal(h0) * ws
        W2 = rng.standard_normal((h1w, h0)) / math.sqrt(h0) * ws
        b2 = 0.3 * rng.standard_normal(h1w) * ws * ws
    Wm = rng.standard_normal((A, h1w)) / math.sqrt(h1w) * ws
    bm = 0.1 * rng.standard_normal(A)
    log_std = rng.uniform(-1.0, 0.5, A)
    act = rng.standard_normal((n, A))
    c = NS(name=name, n=n, F=F, h0=h0, h1w=h1w, A=A, x=x, W1=W1, b1=b1, W2=W2, b2=b2, Wm=Wm,
           bm=bm, log_std=log_std, act=act, exact=exact)
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, _poison(getattr(c, operand), spot, value))
    return c


PF_OPERANDS = ("x", "W1", "b1", "W2", "b2", "Wm", "bm", "log_std", "act")


@functools.lru_cache(maxsize=None)
def pf_cases():
    out, s = [], 8000
    for F in PF_F:
        for h0 in PF_H0:
            s += 1
            out.append(pf_case(f"F{F}_h{h0}", F, h0, PF_H1, 3, s, work=F in (9, 33)))
    for i, A in enumerate(PF_ACTIONS):
        for h0 in PF_H0:
            s += 1
            out.append(pf_case(f"A{A}_h{h0}", 5, h0, (300, 320)[i % 2], A, s, work=A == 9))
    for h0 in (50, 51):   # 4 k-tiles of hidden0 and more than one row block per tile
        s += 1
        out.append(pf_case(f"tiles_h{h0}", 5, h0, 82, 2, s, n=131))
    for h0 in PF_H0:
        s += 1
        out.append(pf_case(f"zeros_h{h0}", 5, h0, PF_H1, 3, s, exact=True))
    for operand in PF_OPERANDS:
        for spot, value in POISONS:
            for h0 in PF_H0:
                s += 1
                out.append(pf_case(_ptag(operand, spot, value) + f"_h{h0}", 5, h0, PF_H1, 3, s,
                                   poison=(operand, spot, value)))
    return {c.name: c for c in out}


def pf_groups():
    names = list(pf_cases())
    g = {"bands": [k for k in names if k.startswith("F")],
         "actions": [k for k in names if k.startswith(("A", "tiles", "zeros"))]}
    for operand in PF_OPERANDS:
        g[f"containment_{operand}"] = [k for k in names if k.startswith((operand + "_inf",
                                                                          operand + "_nan"))]
    assert sorted(sum(g.values(), [])) == sorted(names)
    return g


def pf_forms(c):
    """The forms the case runs in: (form, row_tile, h1_out misaligned)."""
    if c.h0 % 2:
        return (("one_odd", 0, False),)
    return (("split64", 64, False), ("split32", 32, False), ("split16", 16, False),
            ("one_vec", 0, True))


@functools.lru_cache(maxsize=None)
def pf_reference(name):
    return policy_forward_ref(pf_cases()[name])


# ---- dh1_layer1_backward and hidden_backward ------------------------------------------------
DH1_F = (1, 15, 16, 31, 32, 47, 48, 63)
DEEP_K = (2, 16, 18, 32, 34, 50)
DH1_M = (2, 80, 82, 400)
HB_M = (2, 78, 80, 82)
DEEP_N = (1, 255, 256, 257, 4097)


def dh1_case(name, n, K, M, F, seed, work=False, poison=None):
    rng = np.random.default_rng(seed)
    c = NS(name=name, n=n, K=K, M=M, F=F,
           dz2=rng.standard_normal((n, K)) * (DZ_SCALE if work else 1.0),
           W2t=rng.standard_normal((M, K)) * (W_SCALE if work else 1.0),
           h1=_relu_like(rng, (n, M)), x=rng.standard_normal((n, F)))
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, _poison(getattr(c, operand), spot, value))
    return c


@functools.lru_cache(maxsize=None)
def dh1_cases():
    out, s = [], 9000
    for work in (False, True):
        tag = "work" if work else "unit"
        for F in DH1_F:
            s += 1
            out.append(dh1_case(f"F{F}_{tag}", 257, 18, 82, F, s, work))
        for K in DEEP_K:
            s += 1
            out.append(dh1_case(f"K{K}_{tag}", 255, K, 80, 5, s, work))
        for M in DH1_M:
            s += 1
            out.append(dh1_case(f"M{M}_{tag}", 83, 18, M, 17, s, work))
        for n in DEEP_N:
            s += 1
            out.append(dh1_case(f"n{n}_{tag}", n, 18, 82, 3, s, work))
    for operand in ("dz2", "W2t", "h1"):
        for spot, value in POISONS:
            s += 1
            out.append(dh1_case(_ptag(operand, spot, value), 83, 18, 82, 5, s,
                                poison=(operand, spot, value)))
    # an inf in W2 whose column is on in the last row alone: dW1 and db1 of that column are that
    # one row's infinity, not a nan (the rows past n, whose dh1 is 0 x inf, must stay out)
    c = dh1_case("W2t_inf_one_row_on", 3, 18, 82, 5, 9900)
    c.h1[:, 40] = (0.0, -0.0, 1.5)
    c.W2t[40, 3] = np.inf
    out.append(c)
    return {c.name: c for c in out}


def _sweep_groups(names):
    g = {}
    for k in names:
        key = "containment" if ("_inf_" in k or "_nan_" in k) else k[0] + "_" + k.split("_")[-1]
        g.setdefault(key, []).append(k)
    return g


def dh1_groups():
    return _sweep_groups(dh1_cases())


@functools.lru_cache(maxsize=None)
def dh1_reference(name):
    c = dh1_cases()[name]
    return dh1_ref(c.dz2, c.W2t, _gt0(ld(c.h1)), c.x)


def hb_case(name, n, K, M, seed, work=False, poison=None):
    rng = np.random.default_rng(seed)
    c = NS(name=name, n=n, K=K, M=M,
           dz_out=rng.standard_normal((n, K)) * (DZ_SCALE if work else 1.0),
           W=rng.standard_normal((K, M)) * (W_SCALE if work else 1.0),
           h_in=_relu_like(rng, (n, M)))
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, _poison(getattr(c, operand), spot, value))
    return c


@functools.lru_cache(maxsize=None)
def hb_cases():
    out, s = [], 10000
    for work in (False, True):
        tag = "work" if work else "unit"
        for K in DEEP_K:
            s += 1
            out.append(hb_case(f"K{K}_{tag}", 257, K, 82, s, work))
        for M in HB_M:
            s += 1
            out.append(hb_case(f"M{M}_{tag}", 83, 18, M, s, work))
        for n in DEEP_N:
            s += 1
            out.append(hb_case(f"n{n}_{tag}", n, 18, 82, s, work))
    for operand in ("dz_out", "W", "h_in"):
        for spot, value in POISONS:
            s += 1
            out.append(hb_case(_ptag(operand, spot, value), 83, 18, 82, s,
                               poison=(operand, spot, value)))
    return {c.name: c for c in out}


def hb_groups():
    return _sweep_groups(hb_cases())


@functools.lru_cache(maxsize=None)
def hb_reference(name):
    c = hb_cases()[name]
    return hidden_backward_ref(c.dz_out, c.W, c.h_in)


# ---- hidden_tangent -------------------------------------------------------------------------
def ht_case(name, n, k, m, seed, variant=0, with_bias=False, work=False, poison=None):
    """mask_src = h_out (a ReLU output) with no mask_bias, or the pre-bias z with mask_bias = b;
    then mask_src = -mask_bias exactly at a few places (relu'(0) = 0) and -0.0 in column 0."""
    rng = np.random.default_rng(seed)
    c = NS(name=name, n=n, k=k, m=m, variant=variant,
           t_in=rng.standard_normal((n, k)) * (DZ_SCALE if work else 1.0),
           h_in=np.maximum(rng.standard_normal((n, k)), 0.0),
           W=rng.standard_normal((m, k)) * (W_SCALE if work else 1.0),
           dW=rng.standard_normal((m, k)) * (DZ_SCALE if work else 1.0),
           db=rng.standard_normal(m) * (DZ_SCALE if work else 1.0), mask_bias=None)
    if with_bias:
        c.mask_src = rng.standard_normal((n, m))
        c.mask_bias = 0.5 * rng.standard_normal(m)
        c.mask_bias[0] = 0.0
        c.mask_src[0, 0] = -0.0
        for r, col in ((n - 1, m - 1), (n // 2, m // 2), (0, m - 1)):
            c.mask_src[r, col] = -c.mask_bias[col]
    else:
        c.mask_src = _relu_like(rng, (n, m))
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, _poison(getattr(c, operand), spot, value))
    return c


@functools.lru_cache(maxsize=None)
def ht_cases():
    out, s = [], 11000
    for v in GEMM_VARIANTS:
        for with_bias in (False, True):
            s += 1
            out.append(ht_case(f"v{v}_bias{int(with_bias)}", *GEMM_BIG, s, variant=v,
                               with_bias=with_bias, work=with_bias))
    for operand in ("t_in", "h_in", "W", "dW", "db", "mask_src", "mask_bias"):
        for spot, value in POISONS:
            s += 1
            out.append(ht_case(_ptag(operand, spot, value), *GEMM_SMALL, s, variant=2,
                               with_bias=True, poison=(operand, spot, value)))
    return {c.name: c for c in out}


def ht_groups():
    names = list(ht_cases())
    g = {f"variant{v}": [k for k in names if k.startswith(f"v{v}_")] for v in GEMM_VARIANTS}
    g["containment"] = [k for k in names if not k.startswith("v")]
    assert sorted(sum(g.values(), [])) == sorted(names)
    return g


@functools.lru_cache(maxsize=None)
def ht_reference(name):
    return hidden_tangent_ref(ht_cases()[name])


# ---- weight_grad ----------------------------------------------------------------------------
# out_features -> (full o-blocks, fragments of the last o-block): fol 1 .. 4 with and without
WG_O = (16, 17, 44, 64, 80, 96, 300, 128)
WG_I = (17, 30, 80, 81, 400)
WG_N = (1, 3, 5, 300)
# a narrow I at about 2,560 rows: the full and the short o-blocks get different slice counts,
# one of them no multiple of 8 (asserted from the plan in tests/test_gemm_cases_host.py)
WG_UNEVEN = (2560, 300, 17)


def wg_fol(O):
    nob = (O + 63) // 64
    return nob, (O - 64 * (nob - 1) + 15) // 16


def wg_case(name, n, O, I, seed, work=False, poison=None):
    rng = np.random.default_rng(seed)
    c = NS(name=name, n=n, O=O, I=I, dy=rng.standard_normal((n, O)) * (DZ_SCALE if work else 1.0),
           x=np.maximum(rng.standard_normal((n, I)), 0.0) if work else rng.standard_normal((n, I)))
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, _poison(getattr(c, operand), spot, value))
    return c


@functools.lru_cache(maxsize=None)
def wg_cases():
    out, s = [], 12000
    for i, O in enumerate(WG_O):
        for j, n in enumerate(WG_N):
            s += 1
            I = WG_I[(i + j) % len(WG_I)]
            out.append(wg_case(f"O{O}_n{n}_I{I}", n, O, I, s, work=(i + j) % 2 == 1))
    n, O, I = WG_UNEVEN
    out.append(wg_case("uneven_unit", n, O, I, 12900))
    out.append(wg_case("uneven_work", n, O, I, 12901, work=True))
    for operand in ("dy", "x"):
        for spot, value in POISONS:
            s += 1
            out.append(wg_case(_ptag(operand, spot, value), 37, 44, 30, s,
                               poison=(operand, spot, value)))
    return {c.name: c for c in out}


def wg_groups():
    names = list(wg_cases())
    g = {f"O{O}": [k for k in names if k.startswith(f"O{O}_")] for O in WG_O}
    g["uneven"] = [k for k in names if k.startswith("uneven")]
    g["containment"] = [k for k in names if "_inf_" in k or "_nan_" in k]
    assert sorted(sum(g.values(), [])) == sorted(names)
    return g


@functools.lru_cache(maxsize=None)
def wg_reference(name):
    c = wg_cases()[name]
    return weight_grad_ref(c.dy, c.x)


# =============================================================================================
# Runners: one case through an `ops`-shaped module, every output checked
# =============================================================================================
def _nan(shape, dev):
    import torch

    return torch.full(tuple(shape), float("nan"), dtype=torch.float64, device=dev)


def _junk_ws(ops, fn, dev, *sizes):
    """A caller-owned workspace filled with 0x7F bytes (every double of it is a huge value)."""
    ws = getattr(ops, fn)(*sizes, dev)
    ws.fill_(0x7F)
    return ws


def _view(x, rows, cols, dev):
    """x as a view into a larger nan-filled buffer with `cols` doubles per row."""
    buf = _nan((rows, cols), dev)
    v = buf[:x.shape[0], :x.shape[1]]
    v.copy_(_t(x, dev))
    return buf, v


def run_gemm_nt(ops, dev, c, ref=None):
    ref = ref if ref is not None else gemm_reference(c.name)
    bias = _t(c.bias, dev) if c.bias is not None else None
    if not c.strided:
        out = _nan((c.n, c.m), dev)
        C = ops.gemm_nt(_t(c.A, dev), _t(c.B, dev), bias=bias, relu=c.relu, out=out,
                        variant=c.variant)
        assert C.data_ptr() == out.data_ptr()
        check("gemm_c", _n(C), ref.c, ref.bc)
        return dict(c=C)
    # A, B and C are views: lda = k + 2, ldb = k + 4, ldc = m + 3; C's gaps keep their bits
    _, A = _view(c.A, c.n + 1, c.k + 2, dev)
    _, B = _view(c.B, c.m + 1, c.k + 4, dev)
    cbuf = _nan((c.n + 1, c.m + 3), dev)
    cbuf[:, c.m:] = -7.25
    cbuf[c.n:] = -7.25
    before = cbuf.clone()
    C = ops.gemm_nt(A, B, bias=bias, relu=c.relu, out=cbuf[:c.n, :c.m], variant=c.variant)
    assert (A.stride(0), B.stride(0), C.stride(0)) == (c.k + 2, c.k + 4, c.m + 3)
    check("gemm_c", _n(C), ref.c, ref.bc)
    assert bits_equal(cbuf[:, c.m:], before[:, c.m:]) and bits_equal(cbuf[c.n:], before[c.n:]), (
        "gemm_nt wrote between the rows of a strided C")
    return dict(c=cbuf)


def _pack_mask(on):
    import cpu_ops

    return cpu_ops._pack_mask(np.asarray(on))


def run_policy_forward(ops, dev, c, ref=None):
    """Every form of pf_forms(c) into nan-filled outputs: each checked; the mask bit for bit
    against [pre1 > 0]; the three row tiles with equal bits."""
    import torch

    ref = ref if ref is not None else pf_reference(c.name)
    args = [_t(v, dev) for v in (c.x, c.W1, c.b1, c.W2, c.b2, c.Wm, c.bm, c.log_std, c.act)]
    want_mask = torch.as_tensor(_pack_mask(ref.mask))
    got = {}
    for form, tile, misaligned in pf_forms(c):
        if misaligned:  # h1_out starts at an odd element: 8-byte but not 16-byte aligned
            hbuf = _nan((c.n * c.h0 + 3,), dev)
            h1_out = hbuf[1:1 + c.n * c.h0].view(c.n, c.h0)
            if hasattr(h1_out, "data_ptr") and str(dev) != "cpu":
                assert h1_out.data_ptr() % 16 == 8
        else:
            hbuf, h1_out = None, _nan((c.n, c.h0), dev)
        mask = ops.h1_mask_buffer(c.n, c.h0, dev)
        mask.fill_(-1)
        h1, z2, mu, logp = ops.policy_forward(
            *args, h1_out=h1_out, z2_out=_nan((c.n, c.h1w), dev), mu_out=_nan((c.n, c.A), dev),
            logp_out=_nan((c.n,), dev), mask_out=mask, row_tile=tile)
        try:
            check("pf_h1", _n(h1), ref.h1, ref.bh1)
            check("pf_z2", _n(z2), ref.z2, ref.bz2)
            check("pf_mu", _n(mu), ref.mu, ref.bmu)
            check("pf_logp", _n(logp), ref.logp, ref.blogp)
        except AssertionError as err:
            raise AssertionError(f"{form}: {err}") from None
        assert torch.equal(mask.cpu(), want_mask), f"{form}: the bit mask is not [pre1 > 0]"
        if hbuf is not None:
            edge = torch.cat([hbuf[:1], hbuf[1 + c.n * c.h0:]])
            assert bool(torch.isnan(edge).all()), "wrote outside the misaligned h1_out"
        got[form] = dict(h1=h1, z2=z2, mu=mu, logp=logp, mask=mask)
    if "split64" in got:
        for form in ("split32", "split16"):
            for key, v in got["split64"].items():
                assert bits_equal(v, got[form][key]), (form, key, "row tiles differ in bits")
    return {f"{form}_{k}": v for form, d in got.items() for k, v in d.items()}


def run_dh1(ops, dev, c, ref=None):
    """The h1 form checked; the mask= and w2= forms with its bits.  Workspace of 0x7F bytes."""
    ref = ref if ref is not None else dh1_reference(c.name)
    dz2, W2t, h1, x = [_t(v, dev) for v in (c.dz2, c.W2t, c.h1, c.x)]
    with np.errstate(invalid="ignore"):
        mask = _t(_pack_mask(c.h1 > 0), dev)

    def one(**kw):
        ws = _junk_ws(ops, "dh1_layer1_workspace", dev, c.n, c.M, c.F)
        return ops.dh1_layer1_backward(dz2, kw.pop("W2t", W2t), kw.pop("h1", h1), x, ws=ws,
                                       dW_out=_nan((c.M, c.F), dev), db_out=_nan((c.M,), dev),
                                       **kw)

    dW, db = one()
    check("dh1_dW1", _n(dW), ref.dW, ref.bdW)
    check("dh1_db1", _n(db), ref.db, ref.bdb)
    out = dict(dW=dW, db=db)
    if not np.isnan(c.h1).any():  # (a nan in h1 has no bit: both give 0 there, as the reference)
        for what, kw in (("mask", dict(mask=mask)),
                         ("w2", dict(mask=mask, h1=None, W2t=None, w2=W2t.t().contiguous()))):
            gW, gb = one(**kw)
            assert bits_equal(gW, dW) and bits_equal(gb, db), f"the {what}= form differs in bits"
    return out


def run_hidden_backward(ops, dev, c, ref=None):
    ref = ref if ref is not None else hb_reference(c.name)
    dz_out, W, h_in = [_t(v, dev) for v in (c.dz_out, c.W, c.h_in)]
    ws = _junk_ws(ops, "hidden_backward_workspace", dev, c.n, c.M)
    dz, db = ops.hidden_backward(dz_out, W, h_in, ws=ws, dz_out_buf=_nan((c.n, c.M), dev),
                                 db_out=_nan((c.M,), dev))
    check("hb_dz", _n(dz), ref.dz, ref.bdz)
    check("hb_db", _n(db), ref.db, ref.bdb)
    with np.errstate(invalid="ignore"):
        assert np.all(_n(dz)[~(c.h_in > 0)] == 0), "dz_in is not 0 where h_in <= 0"
    return dict(dz=dz, db=db)


def run_hidden_tangent(ops, dev, c, ref=None):
    ref = ref if ref is not None else ht_reference(c.name)
    args = [_t(v, dev) for v in (c.t_in, c.h_in, c.W, c.dW, c.db, c.mask_src)]
    mb = _t(c.mask_bias, dev) if c.mask_bias is not None else None
    t = ops.hidden_tangent(*args, mask_bias=mb, out=_nan((c.n, c.m), dev), variant=c.variant)
    check("ht_t", _n(t), ref.t, ref.bt)
    assert np.all(_n(t)[~_gt0(ref.pre)] == 0), "t_out is not 0 where the pre-activation is <= 0"
    return dict(t=t)


def run_weight_grad(ops, dev, c, ref=None):
    ref = ref if ref is not None else wg_reference(c.name)
    ws = _junk_ws(ops, "weight_grad_workspace", dev, c.n, c.O, c.I)
    dW = ops.weight_grad(_t(c.dy, dev), _t(c.x, dev), out=_nan((c.O, c.I), dev), ws=ws)
    check("wgrad_dW", _n(dW), ref.dW, ref.bdW)
    return dict(dW=dW)


FAMILIES = {
    "gemm_nt": (gemm_cases, gemm_groups, run_gemm_nt),
    "policy_forward": (pf_cases, pf_groups, run_policy_forward),
    "dh1_layer1_backward": (dh1_cases, dh1_groups, run_dh1),
    "hidden_backward": (hb_cases, hb_groups, run_hidden_backward),
    "hidden_tangent": (ht_cases, ht_groups, run_hidden_tangent),
    "weight_grad": (wg_cases, wg_groups, run_weight_grad),
}


def family_groups():
    """[(family, group)] for the tests' parametrisation."""
    return [(fam, g) for fam, (_, groups, _) in FAMILIES.items() for g in groups()]


def run_group(ops, dev, family, group, twice=False):
    """Every case of the group; twice: each case again, with the first run's bits."""
    cases, groups, run = FAMILIES[family]
    for name in groups()[group]:
        c = cases()[name]
        a = run(ops, dev, c)
        if twice:
            b = run(ops, dev, c)
            for key in a:
                assert bits_equal(a[key], b[key]), (family, name, key, "two runs differ in bits")


# =============================================================================================
# Every case through one backend, and the table of the largest error / bound per output:
#   python tests/gemm_cases.py cpu|gpu
# =============================================================================================
if __name__ == "__main__":
    import os
    import sys
    import time

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time()
    if sys.argv[1] == "gpu":
        import torch

        from mepol_amd import ops as backend

        device = torch.device("cuda")
    else:
        import cpu_ops as backend

        device = "cpu"
    failed = []
    for fam, (all_cases, _, runner) in FAMILIES.items():
        for case in all_cases().values():
            try:
                runner(backend, device, case)
            except AssertionError as err:  # keep going: the table below is for the record
                failed.append((fam, case.name, str(err)[:300]))
    for key in sorted(RATIOS):
        if key.startswith(("gemm_", "pf_", "dh1_", "wgrad_", "hb_", "ht_")):
            print(f"{key:12s} {RATIOS[key]:.4f}")
    for item in failed:
        print("# FAILED", *item)
    print(f"# {sys.argv[1]}: {'all cases within bounds' if not failed else 'FAILURES'}, "
          f"{time.time() - t0:.1f} s")
    sys.exit(1 if failed else 0)
