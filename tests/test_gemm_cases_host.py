"""The f64 matrix-core GEMM cases through the CPU stand-ins, the plan, and the negative controls.

No GPU.  As tests/test_policy_cases_host.py does for the head, this file shows that
  * the plain-f64 numpy stand-ins of tests/cpu_ops.py meet every bound of tests/gemm_cases.py,
    and so does a second set that sums in the kernels' shape (k in MFMA steps of 4, the
    weight gradient's K-slices in slice order, 8 waves per 256-row block in wave order, the row
    blocks' records in 16 strided groups of 4 strided waves, the head's 4 column waves in wave
    order): the bounds are not tighter than correct f64 arithmetic;
  * the weight gradient's launch plan (mepol_weight_grad_plan_info, host only) gives every
    (K-slice, tile) to exactly one workgroup and its slices cover the rows once;
  * the case lists select every tiling, FP band and form, NH, fol and k-tile count they claim to;
  * stand-ins with one mistake each fail at least one case of their family.
tests/test_gpu_gemm_ops.py runs the same cases and checkers over the HIP kernels.
"""
import types

import numpy as np
import pytest
import torch

import cpu_ops
import gemm_cases as G

DEV = "cpu"


# ---------------------------------------------------------------------------------------------
# every case through the stand-ins of cpu_ops
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,group", G.family_groups())
def test_standins_meet_every_bound(family, group):
    G.run_group(cpu_ops, DEV, family, group, twice=family == "gemm_nt")


# ---------------------------------------------------------------------------------------------
# a second set that sums in the kernels' shape
# ---------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.numpy()


def _mm4(a, b, acc=None):
    """acc + a [n, K] b^T [m, K] in f64, k in steps of 4 as v_mfma_f64_16x16x4f64 takes it."""
    acc = np.zeros((a.shape[0], b.shape[0])) if acc is None else acc
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, a.shape[1], 4):
            acc = acc + a[:, k0:k0 + 4] @ b[:, k0:k0 + 4].T
    return acc


def _sum_records(recs):
    """reduce.hpp: records in 16 strided groups, 4 waves each taking every fourth record of the
    group, the 4 wave sums in order, then the 16 group sums in order."""
    total = 0.0
    for g in range(16):
        waves = []
        for w in range(4):
            s = 0.0
            for b in range(g + 16 * w, len(recs), 64):
                s = s + recs[b]
            waves.append(s)
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return total


def _blocks(n):
    return [(r, min(n, r + 256)) for r in range(0, n, 256)]


def _waves(lo, hi):
    return [(r, min(hi, r + 32)) for r in range(lo, hi, 32)]


def k_gemm_nt(A, B, bias=None, relu=False, out=None, variant=0):
    v = _mm4(_np(A), _np(B))
    with np.errstate(invalid="ignore"):
        v = v + _np(bias) if bias is not None else v
    return cpu_ops._into(out, cpu_ops._sel(cpu_ops._gt0(v), v) if relu else v)


def k_hidden_tangent(t_in, h_in, W, dW, db, mask_src, mask_bias=None, out=None, variant=0):
    acc = _mm4(_np(h_in), _np(dW), _mm4(_np(t_in), _np(W)))
    with np.errstate(invalid="ignore"):
        pre = _np(mask_src) + (_np(mask_bias) if mask_bias is not None else 0.0)
        return cpu_ops._into(out, cpu_ops._sel(cpu_ops._gt0(pre), acc + _np(db)))


def k_policy_forward(x, W1, b1, W2, b2, Wm, bm, log_std, act, h1_out=None, z2_out=None,
                     mu_out=None, logp_out=None, mask_out=None, row_tile=0):
    with np.errstate(invalid="ignore", over="ignore"):
        pre = _mm4(_np(x), _np(W1)) + _np(b1)
        h1 = cpu_ops._sel(cpu_ops._gt0(pre), pre)
        z2 = _mm4(h1, _np(W2))
        pre2 = z2 + _np(b2)
        rv, wm = cpu_ops._sel(cpu_ops._gt0(pre2), pre2), _np(Wm)
        mu = 0.0
        for c0 in range(0, 320, 80):  # the 4 column waves, in wave order
            mu = mu + rv[:, c0:c0 + 80] @ wm[:, c0:c0 + 80].T
        mu = mu + _np(bm)
        ls = _np(log_std)
        sd = np.exp(ls) + 1e-7
        d = _np(act) - mu
        logp = (-0.5 * (cpu_ops._LOG2PI + 2.0 * ls + d * d / (sd * sd))).sum(axis=1)
    if mask_out is not None:
        mask_out.copy_(torch.as_tensor(cpu_ops._pack_mask(h1 > 0.0)))
    into = cpu_ops._into
    return into(h1_out, h1), into(z2_out, z2), into(mu_out, mu), into(logp_out, logp)


def k_dh1(dz2, W2t, h1, x, ws=None, dW_out=None, db_out=None, mask=None, w2=None):
    Wt = np.ascontiguousarray(_np(w2).T) if w2 is not None else _np(W2t)
    on = cpu_ops._unpack_mask(mask, Wt.shape[0]) if mask is not None else cpu_ops._gt0(_np(h1))
    dz2, x = _np(dz2), _np(x)
    x1 = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)  # [x | 1]: db in column F
    recs = []
    for lo, hi in _blocks(dz2.shape[0]):
        rec = 0.0
        for a, b in _waves(lo, hi):
            dz1 = cpu_ops._sel(on[a:b], _mm4(dz2[a:b], Wt))
            rec = rec + _mm4(dz1.T, x1[a:b].T)
        recs.append(rec)
    tot = _sum_records(recs)
    return cpu_ops._into(dW_out, tot[:, :-1]), cpu_ops._into(db_out, tot[:, -1])


def k_hidden_backward(dz_out, W, h_in, ws=None, dz_out_buf=None, db_out=None):
    dzo, Wn, on = _np(dz_out), _np(W), cpu_ops._gt0(_np(h_in))
    dz = cpu_ops._sel(on, _mm4(dzo, np.ascontiguousarray(Wn.T)))
    recs = []
    for lo, hi in _blocks(dzo.shape[0]):
        rec = 0.0
        with np.errstate(invalid="ignore"):
            for a, b in _waves(lo, hi):
                rec = rec + dz[a:b].sum(axis=0)
        recs.append(rec)
    return cpu_ops._into(dz_out_buf, dz), cpu_ops._into(db_out, _sum_records(recs))


def k_weight_grad(dy, x, out=None, ws=None):
    from mepol_amd import ops

    dy, x = _np(dy), _np(x)
    n, O = dy.shape
    p = ops.weight_grad_plan(n, O, x.shape[1])
    of = 64 * (p["nob"] - 1)
    dW = np.zeros((O, x.shape[1]))
    for o0, o1, S, rows in ((0, of, p["Sf"], p["rows_f"]), (of, O, p["Ss"], p["rows_s"])):
        v = 0.0
        for s in range(S):  # an empty slice adds its zeros
            a, b = min(n, s * rows), min(n, (s + 1) * rows)
            v = v + _mm4(dy[a:b, o0:o1].T, x[a:b].T)
        if o1 > o0:
            dW[o0:o1] = v
    return cpu_ops._into(out, dW)


KOPS = types.SimpleNamespace(**{k: v for k, v in vars(cpu_ops).items() if not k.startswith("__")})
KOPS.gemm_nt, KOPS.hidden_tangent = k_gemm_nt, k_hidden_tangent
KOPS.policy_forward = k_policy_forward
KOPS.dh1_layer1_backward, KOPS.hidden_backward = k_dh1, k_hidden_backward
KOPS.weight_grad = k_weight_grad


@pytest.mark.parametrize("family,group", G.family_groups())
def test_kernel_ordered_standins_meet_every_bound(family, group):
    G.run_group(KOPS, DEV, family, group)


# ---------------------------------------------------------------------------------------------
# the weight gradient's plan
# ---------------------------------------------------------------------------------------------
PLAN_N = (1, 5, 300, 2051, 2560, 8000, 200000)
PLAN_OI = ((300, 400), (44, 30), (64, 80), (17, 400), (80, 17), (400, 400))


@pytest.mark.parametrize("O,I", PLAN_OI)
@pytest.mark.parametrize("n", PLAN_N)
def test_plan_gives_every_slice_and_tile_to_one_workgroup(n, O, I):
    from mepol_amd import ops

    p = ops.weight_grad_plan(n, O, I)
    nob, nib = (O + 63) // 64, (I + 79) // 80
    assert (p["nob"], p["nib"], p["fol"]) == (nob, nib, G.wg_fol(O)[1])
    assert (p["Sf"] == 0) == (nob == 1) and p["Ss"] >= 1
    full, short = {}, {}
    tf = (nob - 1) * nib
    for b in range(8 * p["grid8"]):  # the walk of wgrad_kernel
        xcd, j = b & 7, b >> 3
        if j < p["fend"][xcd]:
            key = (p["fbase"][xcd] + j // tf, j % tf)
            full[key] = full.get(key, 0) + 1
        elif j < p["send"][xcd]:
            j -= p["fend"][xcd]
            key = (p["sbase"][xcd] + j // nib, j % nib)
            short[key] = short.get(key, 0) + 1
    assert full == {(s, t): 1 for s in range(p["Sf"]) for t in range(tf)}
    assert short == {(s, t): 1 for s in range(p["Ss"]) for t in range(nib)}
    for S, rows in ((p["Sf"], p["rows_f"]), (p["Ss"], p["rows_s"])):
        if S:  # slice s holds rows [s rows, (s + 1) rows): disjoint, and they reach n
            assert rows > 0 and rows % 4 == 0 and S * rows >= n
    of = 64 * (nob - 1)
    assert (p["Sf"] * of + p["Ss"] * (O - of)) * I * 8 == ops._ws_bytes("weight_grad", n, O, I)


def test_plan_info_refuses_bad_arguments():
    from mepol_amd import ops
    from mepol_amd._lib import MepolInputError

    for args in ((0, 300, 400), (10, 0, 400), (10, 300, 0)):
        with pytest.raises(MepolInputError):
            ops.weight_grad_plan(*args)


# ---------------------------------------------------------------------------------------------
# coverage of the case lists, from the launchers' selection lines restated in gemm_cases.py
# ---------------------------------------------------------------------------------------------
def test_every_gemm_nt_variant_runs_ragged_with_epilogue_and_strides():
    cases = G.gemm_cases().values()
    for what in (lambda c: c.relu and c.bias is not None, lambda c: c.strided):
        assert {c.variant for c in cases if what(c) and (c.n, c.k, c.m) == G.GEMM_BIG} == set(
            G.GEMM_VARIANTS)
    n, k, m = G.GEMM_BIG
    for v in G.GEMM_VARIANTS:
        bm, bn = G.gemm_tile(v)
        assert n > bm and m > bn and m % bn and n % bm and k % 16 == 2
    assert max(G.gemm_tile(v)[0] for v in G.GEMM_VARIANTS) == 256
    assert max(G.gemm_tile(v)[1] for v in G.GEMM_VARIANTS) == 400
    assert {G.k_tiles(k) for k in G.GEMM_K} == {1, 2, 3} and any(c.n == c.m == 1 for c in cases)
    assert {(c.bias is not None, c.relu) for c in cases} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert {c.variant for c in G.ht_cases().values() if c.mask_bias is None} == set(
        G.GEMM_VARIANTS) == {c.variant for c in G.ht_cases().values() if c.mask_bias is not None}


def test_every_policy_forward_band_runs_in_every_form():
    got = set()
    for c in G.pf_cases().values():
        for _, tile, misaligned in G.pf_forms(c):
            got.add(G.policy_fwd_instance(c.F, c.h0, not misaligned, tile))
    assert got == {(fp, form) for fp in (4, 8, 16, 32, 48, 64) for form in G.PF_FORMS}
    for lo, hi in ((1, 4), (5, 8), (9, 16), (17, 32), (33, 48), (49, 64)):  # both ends of a band
        assert lo in G.PF_F and hi in G.PF_F
        band = {G.policy_fwd_instance(f, 10, True, 0)[0] for f in (lo, hi)}
        assert len(band) == 1
    shapes = {(c.h1w, c.A) for c in G.pf_cases().values()}
    assert {h for h, _ in shapes} >= {300, 320} and {a for _, a in shapes} >= set(G.PF_ACTIONS)


def test_dh1_and_hidden_backward_sweeps_reach_every_path():
    assert {G.dh1_nh(F) for F in G.DH1_F} == {1, 2, 3, 4}
    for F in (15, 31, 47):  # F + 1 on both sides of a multiple of 16
        assert F in G.DH1_F and F + 1 in G.DH1_F and G.dh1_nh(F) + 1 == G.dh1_nh(F + 1)
    assert [G.k_tiles(K) for K in G.DEEP_K] == [1, 1, 2, 2, 3, 4]
    assert [G.row_blocks(n) for n in G.DEEP_N] == [1, 1, 1, 2, 17] and 17 > 16
    for cases in (G.dh1_cases(), G.hb_cases()):
        assert {c.K for c in cases.values()} >= set(G.DEEP_K)
        assert {c.n for c in cases.values()} >= set(G.DEEP_N)
    assert {c.M for c in G.dh1_cases().values()} >= set(G.DH1_M)
    assert {c.M for c in G.hb_cases().values()} >= set(G.HB_M)
    assert all(c.M % 2 == 0 for c in G.dh1_cases().values())  # the w2= form runs in every case
    assert all(np.isfinite(c.x).all() for c in G.dh1_cases().values())  # the stated precondition


def test_weight_grad_cases_reach_every_fol_and_an_uneven_plan():
    from mepol_amd import ops

    kinds = {(nob > 1, fol) for nob, fol in map(G.wg_fol, G.WG_O)}
    assert kinds == {(full, fol) for full in (False, True) for fol in (1, 2, 3, 4)}
    cases = G.wg_cases().values()
    assert {c.n for c in cases} >= {1, 3, 5, 300}
    p = ops.weight_grad_plan(*G.WG_UNEVEN)
    assert p["Sf"] != p["Ss"] and (p["Sf"] % 8 or p["Ss"] % 8) and 2500 <= G.WG_UNEVEN[0] <= 2600
    p = ops.weight_grad_plan(1, 300, 400)  # one row: every slice but the first is empty
    assert p["rows_f"] >= 1 and p["Sf"] > 1 and p["Ss"] > 1


# ---------------------------------------------------------------------------------------------
# negative controls: stand-ins with one mistake each
# ---------------------------------------------------------------------------------------------
def _bad(**replaced):
    ns = types.SimpleNamespace(**{k: v for k, v in vars(cpu_ops).items()
                                  if not k.startswith("__")})
    for k, v in replaced.items():
        setattr(ns, k, v)
    return ns


def _caught(ops, family):
    """The groups of the family in which at least one case fails its checks."""
    hit = []
    for fam, group in G.family_groups():
        if fam == family:
            try:
                G.run_group(ops, DEV, fam, group)
            except AssertionError:
                hit.append(group)
    return hit


def _gemm_with(fn):
    def gemm_nt(A, B, bias=None, relu=False, out=None, variant=0):
        return fn(A, B, bias, relu, out)
    return gemm_nt


def _plain(A, B, bias, relu):
    with np.errstate(invalid="ignore"):
        v = A @ B.T
        v = v + bias if bias is not None else v
    return cpu_ops._sel(cpu_ops._gt0(v), v) if relu else v


def _ldc_ignored(A, B, bias, relu, out):
    v = _plain(_np(A), _np(B), _np(bias), relu)
    flat = torch.as_strided(out, (v.size,), (1,))  # rows packed, as if ldc were m
    flat.copy_(torch.as_tensor(v.reshape(-1)))
    return out


GEMM_MISTAKES = {
    "last k pair dropped": lambda A, B, bias, relu, out: cpu_ops._into(
        out, _plain(_np(A)[:, :-2], _np(B)[:, :-2], _np(bias), relu)),
    "bias omitted": lambda A, B, bias, relu, out: cpu_ops._into(
        out, _plain(_np(A), _np(B), None, relu)),
    "ldc ignored": _ldc_ignored,
    "one operand rounded to f32": lambda A, B, bias, relu, out: cpu_ops._into(
        out, _plain(_np(A).astype(np.float32).astype(np.float64), _np(B), _np(bias), relu)),
}


@pytest.mark.parametrize("mistake", list(GEMM_MISTAKES))
def test_gemm_nt_mistakes_are_caught(mistake):
    hit = _caught(_bad(gemm_nt=_gemm_with(GEMM_MISTAKES[mistake])), "gemm_nt")
    assert hit, mistake
    if mistake == "ldc ignored":
        assert all(g.startswith("variant") for g in hit)  # the strided cases alone


def _wg_last_row_dropped(dy, x, out=None, ws=None):
    with np.errstate(invalid="ignore"):
        return cpu_ops._into(out, _np(dy)[:-1].T @ _np(x)[:-1])


def _wg_padded_row(dy, x, out=None, ws=None):
    """The clamped loads re-read the last row for the rows past n of the last k-step of 4."""
    dy, x = _np(dy), _np(x)
    pad = -dy.shape[0] % 4
    with np.errstate(invalid="ignore"):
        return cpu_ops._into(out, dy.T @ x + pad * np.outer(dy[-1], x[-1]))


def _hb(mask=cpu_ops._gt0, db_from=None, twice=False):
    def hidden_backward(dz_out, W, h_in, ws=None, dz_out_buf=None, db_out=None):
        with np.errstate(invalid="ignore", over="ignore"):
            full = _np(dz_out) @ _np(W)
            dz = cpu_ops._sel(mask(_np(h_in)), full)
            db = (full if db_from == "unmasked" else dz).sum(axis=0)
            if twice:  # the row at a 256-row block's edge (or the last row) counted twice
                db = db + dz[min(255, dz.shape[0] - 1)]
        return cpu_ops._into(dz_out_buf, dz), cpu_ops._into(db_out, db)
    return hidden_backward


def _ge0(v):
    with np.errstate(invalid="ignore"):
        return v >= 0.0


def _pf_z2_post_bias(*args, **kw):
    h1, z2, mu, logp = cpu_ops.policy_forward(*args, **kw)
    z2 += args[4]
    return h1, z2, mu, logp


def _ht(ignore_bias=False, second=True):
    def hidden_tangent(t_in, h_in, W, dW, db, mask_src, mask_bias=None, out=None, variant=0):
        with np.errstate(invalid="ignore", over="ignore"):
            pre = _np(mask_src) + (_np(mask_bias) if mask_bias is not None and not ignore_bias
                                   else 0.0)
            v = _np(t_in) @ _np(W).T + _np(db)
            v = v + _np(h_in) @ _np(dW).T if second else v
        return cpu_ops._into(out, cpu_ops._sel(cpu_ops._gt0(pre), v))
    return hidden_tangent


OTHER_MISTAKES = {
    "last row of a K-slice dropped": ("weight_grad", dict(weight_grad=_wg_last_row_dropped)),
    "a padded row's value let through": ("weight_grad", dict(weight_grad=_wg_padded_row)),
    "a boundary row counted twice": ("hidden_backward", dict(hidden_backward=_hb(twice=True))),
    "mask >= for >": ("hidden_backward", dict(hidden_backward=_hb(mask=_ge0))),
    "db summed from the unmasked product": ("hidden_backward",
                                            dict(hidden_backward=_hb(db_from="unmasked"))),
    "z2 written post-bias": ("policy_forward", dict(policy_forward=_pf_z2_post_bias)),
    "mask_bias ignored": ("hidden_tangent", dict(hidden_tangent=_ht(ignore_bias=True))),
    "the tangent's second product omitted": ("hidden_tangent",
                                             dict(hidden_tangent=_ht(second=False))),
}


@pytest.mark.parametrize("mistake", list(OTHER_MISTAKES))
def test_other_mistakes_are_caught(mistake):
    family, replaced = OTHER_MISTAKES[mistake]
    assert _caught(_bad(**replaced), family), mistake


def test_dh1_mask_mistake_is_caught():
    def dh1(dz2, W2t, h1, x, ws=None, dW_out=None, db_out=None, mask=None, w2=None):
        if mask is not None:
            return cpu_ops.dh1_layer1_backward(dz2, W2t, h1, x, ws, dW_out, db_out, mask, w2)
        dz1 = cpu_ops._sel(_ge0(_np(h1)), _np(dz2) @ _np(W2t).T)
        return cpu_ops._into(dW_out, dz1.T @ _np(x)), cpu_ops._into(db_out, dz1.sum(axis=0))

    assert _caught(_bad(dh1_layer1_backward=dh1), "dh1_layer1_backward")


def test_a_tenth_of_one_dropped_term_is_outside_the_bound():
    """At the largest n used: an output's mean term is A / n, and a tenth of it exceeds the
    output's bound (n u0 A and the carried bounds) in every element with a term."""
    for name in ("n4097_unit", "n4097_work"):
        c, ref = G.dh1_cases()[name], G.dh1_reference(name)
        assert c.n == max(G.DEEP_N)
        has = ref.A_db > 0
        assert has.any() and np.all(0.1 * ref.A_db[has] / c.n > ref.bdb[has])
    for name in ("uneven_unit", "uneven_work"):
        c, ref = G.wg_cases()[name], G.wg_reference(name)
        has = ref.A > 0
        assert has.any() and np.all(0.1 * ref.A[has] / c.n > ref.bdW[has])
