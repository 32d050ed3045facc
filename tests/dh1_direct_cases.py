"""Cases for the register-fed form of dh1_layer1_backward (csrc/gemm.hip, dh1_direct_kernel).

TEST INFRASTRUCTURE ONLY (host code; torch is imported lazily and nothing here needs a GPU).

The mask forms of the op (mask=, and w2= with W2 as stored) can run the register-fed kernel when K
and hidden0 are even and in_features <= 31 (NH <= 2).  Left to itself the library takes it where
the grid has more tiles than the chip has CUs (256) and the LDS kernel everywhere else; form=
"direct" names it at any size, which is how the small shapes below reach it, and one case with 265
tiles checks the automatic choice.  The register-fed kernel is built to give the LDS kernel's
bits: the same k-steps in the same lanes (k = 16 kt + 4 g + s for lane group g at step s), the
two 32-row halves of each of its four waves summed apart and the eight partials of a row block
added in row order, then sum_records<16>.  So
the 80-bit reference, the m u0 A bounds of tests/gemm_cases.py and its kernel-ordered summation
(8 parts of 32 rows per 256-row block) apply as they stand, and on the GPU the f64-h1 form, which
always runs the LDS kernel, is a bit-for-bit reference for every case.

The shapes are the smallest at which this kernel can go wrong, one parameter swept at a time from
a small base: n around a wave's 64 rows, a workgroup's 256 rows, three row blocks with a last one
one row deep, and more row blocks than sum_records' 16 groups; K of one stage (mostly tail, and
exact), a k-tile's tail stage with one and three live pairs, three stages (the ring wraps), and
the workload's 300; M narrowest, one fragment, around the 80-column tile, and the workload's 400;
F narrowest, the ones-column at the 16 / 17 boundary (NH 1 -> 2), the workload's 29, the last NH
= 2 width 31, and 32, which is NH = 3 and must take the LDS kernel.
"""
import functools

import numpy as np

import gemm_cases as G
from entropy_cases import _n, _t, bits_equal, check

NS = G.NS

SWEEP_N = (1, 63, 64, 65, 255, 256, 257, 513, 17 * 256 + 5)
SWEEP_K = (2, 6, 8, 10, 14, 18, 300)
SWEEP_M = (2, 16, 78, 80, 82, 400)
SWEEP_F = (1, 15, 16, 29, 31, 32)   # 32: NH = 3, the LDS kernel
MASKS = ("on", "off", "checker", "zeros")


def direct_fits(K, M, F):
    """l1d::direct_fits of csrc/gemm.hip, restated: where form="direct" is available."""
    return K % 2 == 0 and M % 2 == 0 and (F + 1 + 15) // 16 <= 2


def direct_auto(n, K, M, F):
    """The automatic choice, restated: it fits and the grid has more tiles than CUs."""
    return direct_fits(K, M, F) and ((n + 255) // 256) * ((M + 79) // 80) > 256


def _h1(rng, n, M, pattern):
    """An h1 whose [h1 > 0] is the pattern: all on, all off, a checkerboard, or a ReLU output
    with exact 0.0 and -0.0 in it (both give bit 0)."""
    if pattern == "on":
        return np.full((n, M), 0.5)
    if pattern == "off":
        h = np.zeros((n, M))
        h[::2] = -0.0
        return h
    if pattern == "checker":
        r, c = np.indices((n, M))
        return np.where((r + c) % 2 == 0, 1.0, 0.0)
    return G._relu_like(rng, (n, M))


def case(name, n, K, M, F, seed, mask="zeros", work=False, poison=None):
    rng = np.random.default_rng(seed)
    c = NS(name=name, n=n, K=K, M=M, F=F,
           dz2=rng.standard_normal((n, K)) * (G.DZ_SCALE if work else 1.0),
           W2t=rng.standard_normal((M, K)) * (G.W_SCALE if work else 1.0),
           h1=_h1(rng, n, M, mask), x=rng.standard_normal((n, F)))
    if poison is not None:
        operand, spot, value = poison
        setattr(c, operand, G._poison(getattr(c, operand), spot, value))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out, s = [], 15000
    for n in SWEEP_N:
        s += 1
        out.append(case(f"n{n}", n, 18, 82, 5, s))
    for K in SWEEP_K:
        s += 1
        out.append(case(f"K{K}", 65, K, 80, 5, s, work=K == 300))
    for M in SWEEP_M:
        s += 1
        out.append(case(f"M{M}", 65, 18, M, 17, s, work=M == 400))
    for F in SWEEP_F:
        s += 1
        out.append(case(f"F{F}", 257, 18, 82, F, s))
    for m in MASKS:
        s += 1
        out.append(case(f"mask_{m}", 257, 18, 82, 17, s, mask=m))
    # containment: n = 83 is no multiple of 64, so the second wave's rows past n re-read row 82
    # (the "last" spots) and 0 x inf must not leak into any column
    for operand in ("W2t", "dz2"):
        for spot, value in G.POISONS:
            s += 1
            out.append(case(G._ptag(operand, spot, value), 83, 18, 82, 17, s, mask="on",
                            poison=(operand, spot, value)))
    # an inf in W2 whose column is on in the last row alone (gemm_cases' W2t_inf_one_row_on)
    c = case("W2t_inf_one_row_on", 3, 18, 82, 5, 15900)
    c.h1[:, 40] = (0.0, -0.0, 1.5)
    c.W2t[40, 3] = np.inf
    out.append(c)
    # 53 row blocks x 5 column tiles = 265 tiles: the automatic choice is the register-fed kernel
    out.append(case("auto_many_tiles", 53 * 256 - 255, 6, 400, 1, 15901))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def reference(name):
    c = cases()[name]
    return G.dh1_ref(c.dz2, c.W2t, G._gt0(G.ld(c.h1)), c.x)


def run(ops, dev, c, plan=None, form=None, want=None, lds_reference=False):
    """The mask= and w2= forms of one case: each twice into nan-filled outputs with a workspace
    of 0x7F bytes, equal bits on both calls and between the forms, every output within its bound
    of the 80-bit reference (non-finite values exactly where the reference has them: with n no
    multiple of 64, dW1 and db1 stay finite wherever the reference is).  form: passed on to
    ops.dh1_layer1_backward when given.  plan(n, K, M, F, w2): the kernel the library reports for
    that call, asserted to be `want` before anything runs.  lds_reference: the f64-h1 form, which
    always runs the LDS kernel, must give the same bits."""
    ref = reference(c.name)
    dz2, W2t, h1, x = [_t(v, dev) for v in (c.dz2, c.W2t, c.h1, c.x)]
    mask = _t(G._pack_mask(c.h1 > 0), dev)
    extra = {} if form is None else {"form": form}
    got = {}
    for which, kw in (("mask", dict(W2t=W2t, h1=h1, mask=mask)),
                      ("w2", dict(W2t=None, h1=None, mask=mask, w2=W2t.t().contiguous()))):
        if plan is not None:
            p = plan(c.n, c.K, c.M, c.F, which == "w2")
            assert p["form"] == want, (c.name, which, p)
        pair = []
        for _ in range(2):
            ws = G._junk_ws(ops, "dh1_layer1_workspace", dev, c.n, c.M, c.F)
            dW, db = ops.dh1_layer1_backward(dz2, kw["W2t"], kw["h1"], x, ws=ws,
                                             dW_out=G._nan((c.M, c.F), dev),
                                             db_out=G._nan((c.M,), dev), mask=kw["mask"],
                                             w2=kw.get("w2"), **extra)
            pair.append((dW, db))
        assert bits_equal(pair[0][0], pair[1][0]) and bits_equal(pair[0][1], pair[1][1]), \
            f"{c.name}: the {which}= form gives other bits on a second call"
        check(f"dh1d_dW1_{which}", _n(pair[0][0]), ref.dW, ref.bdW)
        check(f"dh1d_db1_{which}", _n(pair[0][1]), ref.db, ref.bdb)
        got[which] = pair[0]
    assert bits_equal(got["mask"][0], got["w2"][0]) and bits_equal(got["mask"][1], got["w2"][1]), \
        f"{c.name}: the mask= and w2= forms differ in bits"
    if lds_reference:
        ws = G._junk_ws(ops, "dh1_layer1_workspace", dev, c.n, c.M, c.F)
        dW, db = ops.dh1_layer1_backward(dz2, W2t, h1, x, ws=ws, dW_out=G._nan((c.M, c.F), dev),
                                         db_out=G._nan((c.M,), dev))
        assert bits_equal(dW, got["mask"][0]) and bits_equal(db, got["mask"][1]), \
            f"{c.name}: the {want} kernel's bits are not the LDS kernel's"
    return got
