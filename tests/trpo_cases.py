"""Cases, 80-bit references and error bounds for the mean layer of TRPO's Fisher-vector product.

TEST INFRASTRUCTURE ONLY (host code; torch is imported lazily and nothing here needs a GPU).

mean_tangent_kernel<AP> and mean_bwd_kernel<AP> (csrc/head.hip) are tested op by op, the way
tests/policy_cases.py tests the Gaussian head: every case goes through an `ops`-shaped module
(tests/cpu_ops.py on the CPU, mepol_amd.ops on the GPU) and every output is compared with a
reference computed here in np.longdouble from the formulas of include/mepol_amd.h.  The bounds have
policy_cases.py's shape (m u0 A with A the sum of the absolute values of the terms on the output's
path and m the roundings on it for ANY summation order, times SLACK, plus the propagated bound of
an input that was itself computed); adding an exact 0 (padded lanes, padded actions, rows past n,
empty record groups) does not round.  No bound uses what an implementation returned.

The ReLU masks are exact by the argument of policy_cases.py's docstring; tangent_reference and
backward_reference assert that no pre-activation lies within its bound of 0 except where a case
puts it at exactly +-0.0.
"""
import functools
import math
import types

import numpy as np

import policy_cases as P
from entropy_cases import LD, RATIOS, SLACK, U0, _n, _t, bits_equal, check, ld  # noqa: F401

_mm, _mmb = P._mm, P._mmb


# =============================================================================================
# The launchers' selection lines, restated (mepol_mean_tangent, mepol_mean_backward)
# =============================================================================================
def tangent_instance(N, H, A):
    """What mepol_mean_tangent launches: AP actions per chunk, nch chunks (grid.y), ncl column
    steps, grid.x blocks of 4 waves; a wave takes 4 rows per group and loops while groups remain."""
    ap = 1 if A <= 1 else 2 if A <= 2 else 4 if A <= 4 else 8
    nch = (A + ap - 1) // ap
    ncl = (H + 15) // 16
    groups = (N + 3) // 4
    gx = max(1, min(2048, (groups + 3) // 4))
    return types.SimpleNamespace(ap=ap, nch=nch, ncl=ncl, gx=gx, last_chunk=A - (nch - 1) * ap,
                                 last_rows=N - 4 * (groups - 1), second_group=groups > 4 * gx)


def bwd_records(N):
    """Partial records (blocks) of mean_bwd_kernel: 8 rows per block at least, 512 at most."""
    return max(1, min(512, (N + 7) // 8))


def bwd_instance(N, H, A):
    """What mepol_mean_backward launches: AP padded actions, a block of hs threads (one column per
    lane, hs / 64 waves), nb blocks that walk row pairs at stride 2 nb; sum_records adds the nb
    records in 8 strided groups, each by 4 waves of every 32nd record."""
    ap = 2 if A <= 2 else 4 if A <= 4 else 8 if A <= 8 else 16 if A <= 16 else 32
    hs = (H + 63) // 64 * 64
    nb = bwd_records(N)
    pairs = (N + 1) // 2
    return types.SimpleNamespace(ap=ap, hs=hs, waves=hs // 64, nb=nb,
                                 passes=(pairs + nb - 1) // nb, half_pair=N % 2 == 1)


# =============================================================================================
# References with their bounds
# =============================================================================================
def mean_tangent_ref(t, z, bz, Wm, dWm, dbm, scale):
    """c_ia = scale_a s_ia, s_ia = sum_j t_ij Wm_aj + x_ij dWm_aj + dbm_a, x = relu(z + bz): 2 H + 1
    terms.  Each product rounds once (not at all under fma: looser, never tighter) and the 2 H
    adds round once each in whatever order (16 lanes of strided columns, the exchange tree, dbm
    last): m = 2 H + 1 over A = sum_j |t Wm| + |x dWm| + |dbm|; the x terms also carry the one
    rounding of z + bz (none without a bz): u0 sum_j |x dWm|.  The product by scale rounds once:
    |scale| bs + u0 |c|.  t is NOT masked by this kernel: hidden_tangent masked it already."""
    H = z.shape[1]
    pre, x, ux = P._relu_in(z, bz)
    s = _mm(t, ld(Wm).T) + _mm(x, ld(dWm).T) + ld(dbm)
    Ax = _mmb(x, np.abs(dWm).T)
    As = _mmb(np.abs(t), np.abs(Wm).T) + Ax + np.abs(ld(dbm))
    bs = (2 * H + 1) * U0 * As + ux * Ax
    c = ld(scale) * s
    bc = (np.abs(ld(scale)) * bs + U0 * np.abs(c)) * SLACK
    return types.SimpleNamespace(c=c, bc=bc, pre=pre)


def mean_bwd_ref(c, z, bz, Wm, dc_in=None):
    """The backward from a cotangent c [n, A] on mu (dc_in bounds its error in the chained case).
    dWm_aj = sum_i c_ia x_ij: x's rounding (with a bz) and the product's, n - 1 adds in any order
    (row pairs at stride 2 nb inside a block, the blocks' records in strided groups, the groups in
    order): (ux + u0) A + (n - 1) u0 A, A = sum_i |c x|, + sum_i dc_in x.
    dbm_a = sum_i c_ia: n - 1 adds, A = sum_i |c|, + sum_i dc_in.
    dz_ij = [z + bz > 0] sum_a c_ia Wm_aj: A terms, one rounding per product and A - 1 adds (the
    fma chain starts at an exact 0 and also adds the padded actions' exact zeros): A u0 sum_a
    |c Wm| + sum_a dc_in |Wm|.
    dbz_j = sum_i dz_ij: dz's bounds and n - 1 adds, A = sum_i |dz|."""
    n, H = z.shape
    A = Wm.shape[0]
    pre, x, ux = P._relu_in(z, bz)
    W, cl = ld(Wm), ld(c)
    din = np.zeros((n, A), LD) if dc_in is None else ld(dc_in)
    ca = np.abs(cl)
    dWm = _mm(cl.T, x)
    AW = _mmb(ca.T, x)
    bdWm = (_mmb(din.T, x) + (ux + U0) * AW + (n - 1) * U0 * AW) * SLACK
    dbm = np.sum(cl, axis=0)
    bdbm = (np.sum(din, axis=0) + (n - 1) * U0 * np.sum(ca, axis=0)) * SLACK
    mask = pre > 0
    dz = np.where(mask, _mm(cl, W), 0)
    Az = _mmb(ca, np.abs(W))
    bdz = np.where(mask, _mmb(din, np.abs(W)) + A * U0 * Az, 0) * SLACK
    dbz = np.sum(dz, axis=0)
    bdbz = (np.sum(bdz, axis=0) + (n - 1) * U0 * np.sum(np.abs(dz), axis=0)) * SLACK
    return types.SimpleNamespace(dz=dz, bdz=bdz, dWm=dWm, bdWm=bdWm, dbm=dbm, bdbm=bdbm, dbz=dbz,
                                 bdbz=bdbz, pre=pre, x=x)


# =============================================================================================
# Cases
# =============================================================================================
# every AP of both kernels; last tangent chunks of 1..7 actions (9, 10, 11, 12, 5, 14, 7 / 15 /
# 31); padded backward actions in every AP
MEAN_A = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 24, 25, 31, 32)
# both sides of the 16-column step and of the 64-column wave; 1 to 8 waves per backward block
MEAN_H = (1, 15, 16, 17, 18, 63, 64, 65, 129, 256, 300, 321, 448, 511, 512)
MEAN_CROSS_N = 7
TAN_ROW_SHAPES = ((16, 2), (18, 9))    # (H, A)
TAN_ROWS_N = (1, 2, 3, 4, 5, 9, 1025, 32768, 32769, 32773)
BWD_ROW_SHAPES = ((18, 3), (300, 2))
BWD_ROWS_N = (1, 2, 3, 7, 8, 9, 16, 17, 57, 64, 65, 257, 4088, 4089, 4100)
BWD_BIG = "n4100_H512_A32"
SHARP = "n517_H300_A2"


def mean_case(name, n, H, A, seed, zero_pos=False, zero_row=None, signed_scale=False, zpat=None):
    """t, z [n, H], bz [H], Wm, dWm [A, H] of order 1 / sqrt(H), dbm, a positive scale that differs
    per action, and the backward's cotangent c [n, A] whose last row is the largest in every
    component (a clamped row n - 1 that is counted twice shows).
    zero_pos: z + bz is exactly +0.0 at a few (r, j), the first and the last column among them
    (z = -bz there; z = 0.0 without a bz), and exactly -0.0 at one more (z = -0.0 under a bz
    entry of -0.0).  zero_row: that row of z + bz is all +0.0.
    signed_scale: scale[0] = 0 and scale[1] < 0.
    zpat "lastcol": z + bz > 0 in the last column only; "lastact": only the last action has
    weights (Wm, dWm are 0 in every other row)."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((n, H))
    z = rng.standard_normal((n, H))
    bz = 0.5 * rng.standard_normal(H)
    Wm = rng.standard_normal((A, H)) / math.sqrt(H)
    dWm = rng.standard_normal((A, H)) / math.sqrt(H)
    dbm = 0.1 * rng.standard_normal(A)
    scale = rng.uniform(0.2, 2.0, A)
    c = rng.standard_normal((n, A))
    c[n - 1] = np.where(rng.random(A) < 0.5, -1.0, 1.0) * (np.abs(c).max(axis=0) + 1.0)
    if signed_scale:
        assert A >= 3
        scale[0], scale[1] = 0.0, -scale[1]
    if zpat == "lastcol":
        z = -np.abs(z) - 4.0
        z[:, H - 1] = np.abs(z[:, H - 1]) + 4.0
        assert np.abs(bz).max() < 3.0
    if zpat == "lastact":
        Wm[:A - 1] = 0.0
        dWm[:A - 1] = 0.0
    pos, neg = (), None
    if zero_pos:
        pos = tuple(sorted({(0, 0), (n - 1, H - 1), (n // 2, H // 2), (n - 1, 0), (1 % n, H - 1)}))
        neg = (n // 3, H // 3)
        assert neg not in pos and neg[1] not in (0, H - 1, H // 2)
        bz[neg[1]] = -0.0
    return types.SimpleNamespace(name=name, n=n, H=H, A=A, t=t, z=z, bz=bz, Wm=Wm, dWm=dWm, dbm=dbm,
                                 scale=scale, c=c, zero_pos=pos, neg_zero=neg, zero_row=zero_row)


def mean_inputs(c, with_bz):
    """(z, bz or None) of the case: the exact-zero positions follow the variant."""
    z = c.z.copy()
    for r, col in c.zero_pos:
        z[r, col] = -c.bz[col] if with_bz else 0.0
    if c.zero_row is not None:
        z[c.zero_row] = -c.bz if with_bz else 0.0
    if c.neg_zero is not None:
        z[c.neg_zero] = -0.0
    return z, (c.bz if with_bz else None)


def zero_mask(c):
    zero = np.zeros((c.n, c.H), bool)
    for r, col in c.zero_pos:
        zero[r, col] = True
    if c.neg_zero is not None:
        zero[c.neg_zero] = True
    if c.zero_row is not None:
        zero[c.zero_row] = True
    return zero


def _assert_masks_decided(c, pre, with_bz):
    """No pre-activation within its bound (one rounding: u0 (|z| + |bz|); 4 of them asked for) of
    0 but the exact zeros that the case sets; those are there, with the sign the case states."""
    z, bz = mean_inputs(c, with_bz)
    mag = ld(np.abs(z) + (np.abs(bz) if with_bz else 0))
    zero = zero_mask(c)
    assert np.all(pre[zero] == 0), c.name
    assert np.all(np.abs(pre[~zero]) > 4 * U0 * mag[~zero]), c.name
    if c.neg_zero is not None:
        f64 = z[c.neg_zero] + bz[c.neg_zero[1]] if with_bz else z[c.neg_zero]
        assert f64 == 0 and np.signbit(f64), c.name
        r, col = c.zero_pos[0]
        assert not np.signbit(z[r, col] + bz[col] if with_bz else z[r, col])


@functools.lru_cache(maxsize=None)
def mean_cases():
    out, i = [], 0
    for A in MEAN_A:
        for H in MEAN_H:
            out.append(mean_case(f"x_A{A}_H{H}", MEAN_CROSS_N, H, A, 7000 + i))
            i += 1
    for H, A in TAN_ROW_SHAPES:
        for n in TAN_ROWS_N:
            out.append(mean_case(f"t{n}_H{H}_A{A}", n, H, A, 8000 + i))
            i += 1
    for H, A in BWD_ROW_SHAPES:
        for n in BWD_ROWS_N:
            out.append(mean_case(f"n{n}_H{H}_A{A}", n, H, A, 9000 + i))
            i += 1
    out.append(mean_case(BWD_BIG, 4100, 512, 32, 9900))
    out.append(mean_case(SHARP, 517, 300, 2, 9901))
    out.append(mean_case("zero_pos_A3", 9, 18, 3, 9902, zero_pos=True))
    out.append(mean_case("zero_pos_A9", 7, 65, 9, 9903, zero_pos=True))
    out.append(mean_case("zero_row_A2", 9, 33, 2, 9904, zero_row=8))
    out.append(mean_case("zero_row_A17", 9, 300, 17, 9905, zero_row=3))
    out.append(mean_case("signed_scale_A3", 9, 18, 3, 9906, signed_scale=True))
    out.append(mean_case("signed_scale_A17", 7, 300, 17, 9907, signed_scale=True))
    out.append(mean_case("lastcol_A2", 9, 17, 2, 9908, zpat="lastcol"))
    out.append(mean_case("lastcol_A9", 7, 300, 9, 9909, zpat="lastcol"))
    out.append(mean_case("lastact_A3", 9, 18, 3, 9910, zpat="lastact"))
    out.append(mean_case("lastact_A9", 7, 65, 9, 9911, zpat="lastact"))
    return {c.name: c for c in out}


SPECIAL = ("zero", "signed", "lastcol", "lastact")


def _special_names():
    return [k for k in mean_cases() if k.startswith(SPECIAL)]


def tangent_groups():
    """Test-sized groups of the tangent's cases."""
    groups = {f"cross_A{A}": [f"x_A{A}_H{H}" for H in MEAN_H] for A in MEAN_A}
    for H, A in TAN_ROW_SHAPES:
        groups[f"rows_H{H}_A{A}"] = [f"t{n}_H{H}_A{A}" for n in TAN_ROWS_N]
    groups["special"] = _special_names()
    return groups


def backward_groups():
    """Test-sized groups of the backward's cases; the largest shape stands alone."""
    groups = {f"cross_A{A}": [f"x_A{A}_H{H}" for H in MEAN_H] for A in MEAN_A}
    for H, A in BWD_ROW_SHAPES:
        groups[f"rows_H{H}_A{A}"] = [f"n{n}_H{H}_A{A}" for n in BWD_ROWS_N]
    groups["special"] = _special_names() + [SHARP]
    groups["big"] = [BWD_BIG]
    return groups


def variants(name):
    """with_bz values a case runs with: the largest shape's 3 s reference is computed once."""
    return (True,) if name == BWD_BIG else (True, False)


MEAN_CHAIN = ("n257_H300_A2", "n4100_H18_A3", "x_A17_H511")


@functools.lru_cache(maxsize=None)
def tangent_reference(name, with_bz):
    c = mean_cases()[name]
    z, bz = mean_inputs(c, with_bz)
    ref = mean_tangent_ref(c.t, z, bz, c.Wm, c.dWm, c.dbm, c.scale)
    _assert_masks_decided(c, ref.pre, with_bz)
    zero = zero_mask(c)
    if zero.any():  # the t Wm term counts there although x = 0: the kernel must not mask t
        assert np.all(np.maximum(ref.pre, 0)[zero] == 0)
        rows = np.unique(np.nonzero(zero)[0])
        tw = _mm(np.where(zero, c.t, 0)[rows], ld(c.Wm).T) * ld(c.scale)
        live = ld(c.scale) != 0
        if name.startswith("zero"):
            assert np.all(np.abs(tw[:, live]) > 1e6 * ref.bc[rows][:, live]), name
    return ref


@functools.lru_cache(maxsize=None)
def backward_reference(name, with_bz):
    c = mean_cases()[name]
    z, bz = mean_inputs(c, with_bz)
    ref = mean_bwd_ref(c.c, z, bz, c.Wm)
    _assert_masks_decided(c, ref.pre, with_bz)
    zero = zero_mask(c)
    assert np.all(ref.dz[zero] == 0) and np.all(ref.x[zero] == 0)
    if c.zero_pos:  # the unmasked c Wm is not 0 there: relu'(0) = 1 would show
        assert np.all(_mm(c.c, c.Wm)[zero] != 0)
    assert np.all(np.abs(c.c[c.n - 1]) >= np.abs(c.c).max(axis=0))
    return ref


@functools.lru_cache(maxsize=None)
def chain_reference(name, with_bz):
    """mean_tangent then mean_backward on its c: the backward reference from the exact c, the
    tangent's bound carried into it."""
    c = mean_cases()[name]
    z, bz = mean_inputs(c, with_bz)
    f = mean_tangent_ref(c.t, z, bz, c.Wm, c.dWm, c.dbm, c.scale)
    return f, mean_bwd_ref(f.c, z, bz, c.Wm, dc_in=f.bc)


# =============================================================================================
# Runners: one case through an `ops`-shaped module, every output checked
# =============================================================================================
_nan = P._nan


def _tangent_args(c, with_bz, dev):
    z, bz = mean_inputs(c, with_bz)
    args = [_t(x, dev) for x in (c.t, z, c.Wm, c.dWm, c.dbm, c.scale)]
    return args, (_t(bz, dev) if with_bz else None)


def run_mean_tangent(ops, dev, c, with_bz, ref=None):
    """mean_tangent into a nan-filled out (every element is written) and into a fresh one."""
    ref = ref if ref is not None else tangent_reference(c.name, with_bz)
    args, bzt = _tangent_args(c, with_bz, dev)
    out = _nan((c.n, c.A), dev)
    got = ops.mean_tangent(*args, bz=bzt, out=out)
    assert got.data_ptr() == out.data_ptr()
    check("c", _n(got), ref.c, ref.bc)
    assert bits_equal(got, ops.mean_tangent(*args, bz=bzt)), "c depends on the buffer"
    return dict(c=got)


NAMES = ("dz", "dWm", "dbm", "dbz")


def check_mean_backward(got, ref, with_bz, need_dz=True, sfx=""):
    dz, dWm, dbm, dbz = got
    if need_dz:
        check("mean_dz" + sfx, _n(dz), ref.dz, ref.bdz)
        assert np.all(_n(dz)[np.asarray(ref.pre <= 0)] == 0), "dz is not 0 where z + bz <= 0"
    else:
        assert dz is None
    check("mean_dWm" + sfx, _n(dWm), ref.dWm, ref.bdWm)
    check("mean_dbm" + sfx, _n(dbm), ref.dbm, ref.bdbm)
    if with_bz:
        check("mean_dbz" + sfx, _n(dbz), ref.dbz, ref.bdbz)
    else:
        assert dbz is None


def run_mean_backward(ops, dev, c, with_bz, ref=None):
    """mean_backward as one call, checked; then its call forms, each with the one call's bits:
    need_dz=False; nan-filled outs= and dz_out= with a nan-filled caller-owned ws."""
    ref = ref if ref is not None else backward_reference(c.name, with_bz)
    z, bz = mean_inputs(c, with_bz)
    ct, zt, Wm = [_t(x, dev) for x in (c.c, z, c.Wm)]
    bzt = _t(bz, dev) if with_bz else None
    one = ops.mean_backward(ct, zt, Wm, bz=bzt)
    assert len(one) == 4
    check_mean_backward(one, ref, with_bz)

    def same(other, what, dz=True):
        for k, a, b in zip(NAMES, one, other):
            if k == "dz" and not dz:
                assert b is None, what
            else:
                assert bits_equal(a, b), (what, k)

    same(ops.mean_backward(ct, zt, Wm, bz=bzt, need_dz=False), "need_dz=False", False)
    outs = (_nan((c.A, c.H), dev), _nan((c.A,), dev), _nan((c.H,), dev) if with_bz else None)
    dz_out = _nan((c.n, c.H), dev)
    ws = None
    if hasattr(ops, "mean_backward_workspace"):
        ws = ops.mean_backward_workspace(c.n, c.H, c.A, zt.device)
        ws.fill_(255)  # all bits set: every double of it is a nan
    got = ops.mean_backward(ct, zt, Wm, bz=bzt, ws=ws, dz_out=dz_out, outs=outs)
    assert got[0].data_ptr() == dz_out.data_ptr()
    for a, b in zip(got[1:], outs):
        assert (a is None and b is None) or a.data_ptr() == b.data_ptr()
    same(got, "outs=, dz_out= and ws=")
    return dict(zip(NAMES, one))


def run_mean_chain(ops, dev, c, with_bz):
    """mean_tangent, then mean_backward on the c it returned."""
    f, b = chain_reference(c.name, with_bz)
    args, bzt = _tangent_args(c, with_bz, dev)
    got_c = ops.mean_tangent(*args, bz=bzt)
    check("c", _n(got_c), f.c, f.bc)
    got = ops.mean_backward(got_c, args[1], args[2], bz=bzt)
    check_mean_backward(got, b, with_bz, sfx="_chained")
    return got


# =============================================================================================
# Every case through one backend, and the table of the largest error / bound per output:
#   python tests/trpo_cases.py cpu|gpu [out.json]
# (the batch kernels' figures come from tests/goal_rl_cases.py's families, run here as well)
# =============================================================================================
def run_all(ops, dev):
    import goal_rl_cases as C

    cases = mean_cases()
    for names in tangent_groups().values():
        for k in names:
            for with_bz in variants(k):
                run_mean_tangent(ops, dev, cases[k], with_bz)
    for names in backward_groups().values():
        for k in names:
            for with_bz in variants(k):
                run_mean_backward(ops, dev, cases[k], with_bz)
    for k in MEAN_CHAIN:
        for with_bz in (True, False):
            run_mean_chain(ops, dev, cases[k], with_bz)
    C.run_all(ops, dev)


if __name__ == "__main__":
    import json
    import os
    import sys
    import time

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time()
    if sys.argv[1] == "gpu":
        import torch

        from mepol_amd import ops as backend_ops

        backend = (backend_ops, torch.device("cuda"))
    else:
        import cpu_ops as backend_ops

        backend = (backend_ops, "cpu")
    run_all(*backend)
    for key in sorted(RATIOS):
        print(f"{key:18s} {RATIOS[key]:.4f}")
    print(f"# {sys.argv[1]}: all cases within bounds, {time.time() - t0:.1f} s")
    overall = dict(RATIOS)
    headline = {
        "mean_tangent t32773_H18_A9": lambda: run_mean_tangent(
            *backend, mean_cases()["t32773_H18_A9"], True),
        "mean_backward " + BWD_BIG: lambda: run_mean_backward(
            *backend, mean_cases()[BWD_BIG], True),
        "mean_backward n4100_H300_A2": lambda: run_mean_backward(
            *backend, mean_cases()["n4100_H300_A2"], True),
        "mean chain n4100_H18_A3": lambda: run_mean_chain(
            *backend, mean_cases()["n4100_H18_A3"], True),
    }
    large = {}
    for title, fn in headline.items():
        RATIOS.clear()
        fn()
        large[title] = dict(RATIOS)
        print(f"{title:30s} " + "  ".join(f"{k} {v:.2g}" for k, v in sorted(RATIOS.items())))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w", encoding="utf-8") as f:
            json.dump({"overall": overall, "largest_shapes": large}, f, indent=1, sort_keys=True)
