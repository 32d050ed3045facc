"""The head / input-layer / optimizer cases through the CPU stand-ins, and the negative controls.

No GPU.  As tests/test_entropy_cases_host.py does for the entropy ops, this file shows that
  * the plain-f64 numpy stand-ins of tests/cpu_ops.py meet every bound of tests/policy_cases.py,
    and so does a second set that sums in the kernels' shape (16 lanes of strided columns and an
    exchange tree in the forward; rows strided over waves, per-block records, records in 8
    strided groups in the backward): the bounds are not tighter than correct f64 arithmetic;
  * stand-ins with one mistake each fail at least one case of their family, so the cases and
    bounds would notice that mistake in a kernel;
  * the case lists select every template instantiation, FP band and record count they claim to.
tests/test_gpu_policy_ops.py runs the same cases and checkers over the HIP kernels.
"""
import types

import numpy as np
import pytest
import torch

import cpu_ops
import policy_cases as P

DEV = "cpu"
BZ = [True, False]


# ---------------------------------------------------------------------------------------------
# every case through the stand-ins of cpu_ops
# ---------------------------------------------------------------------------------------------
FWD_GROUPS, BWD_GROUPS = P.head_fwd_groups(), P.head_bwd_groups()


@pytest.mark.parametrize("group", list(FWD_GROUPS))
def test_head_forward(group):
    for name in FWD_GROUPS[group]:
        for with_bz in BZ:
            P.run_head_forward(cpu_ops, DEV, P.head_fwd_cases()[name], with_bz)


@pytest.mark.parametrize("group", list(BWD_GROUPS))
def test_head_backward(group):
    for name in BWD_GROUPS[group]:
        for with_bz in BZ:
            P.run_head_backward(cpu_ops, DEV, P.head_bwd_cases()[name], with_bz)


@pytest.mark.parametrize("with_bz", BZ)
@pytest.mark.parametrize("name", P.HEAD_CHAIN)
def test_head_forward_then_backward(name, with_bz):
    P.run_head_chain(cpu_ops, DEV, P.head_bwd_cases()[name], with_bz)


@pytest.mark.parametrize("name", list(P.layer_cases()))
def test_layer(name):
    P.run_layer(cpu_ops, DEV, P.layer_cases()[name])


@pytest.mark.parametrize("name", list(P.optim_cases()))
def test_optim_step(name):
    P.run_optim(cpu_ops, DEV, P.optim_cases()[name])
    assert P.OPTIM_BITS[name][0] == 0  # cpu_ops.optim_step against itself


# ---------------------------------------------------------------------------------------------
# coverage of the case lists
# ---------------------------------------------------------------------------------------------
def test_forward_cross_product_selects_all_49_instantiations():
    got = {P.head_fwd_instance(H, A) for A in P.HEAD_FWD_A for H in P.HEAD_FWD_H}
    want = {(ap, ncl, nch) for ap, nch in ((1, 1), (2, 1), (4, 1), (8, 1), (8, 2), (8, 3), (8, 4))
            for ncl in (4, 8, 12, 16, 20, 24, 32)}
    assert got == want and len(got) == 49
    # both ends of every NCL band
    for lo, hi in ((1, 64), (65, 128), (129, 192), (193, 256), (257, 320), (321, 384), (385, 512)):
        assert lo in P.HEAD_FWD_H and hi in P.HEAD_FWD_H
        assert P.head_fwd_instance(lo, 1)[1] == P.head_fwd_instance(hi, 1)[1]
    c = P.head_fwd_cases()
    assert all(c[f"x_A{A}_H{H}"].n == 37 for A in P.HEAD_FWD_A for H in P.HEAD_FWD_H)


def test_backward_cross_products_select_all_37_instantiations():
    narrow = {P.head_bwd_instance(H, A) for A in P.HEAD_BWD_NARROW_A for H in P.HEAD_BWD_NARROW_H}
    assert narrow == {("narrow", ap, nc) for ap in (1, 2, 4, 8) for nc in range(1, 9)}
    wide = {P.head_bwd_instance(H, A) for A in P.HEAD_BWD_WIDE_A for H in P.HEAD_BWD_WIDE_H}
    assert {w[1] for w in wide} == {12, 16, 20, 24, 32}
    assert {w[2] for w in wide} == {64, 128, 320, 512}
    assert len(narrow) + len({w[1] for w in wide}) == 37


def test_row_sweeps_reach_the_record_counts_and_the_row_edges():
    assert {P.head_bwd_records(n) for n in P.HEAD_BWD_SWEEP_N} >= {1, 2, 5, 9, 33}
    assert [P.head_bwd_records(n) for n in (1, 129, 517, 1025, 4100)] == [1, 2, 5, 9, 33]
    assert any(n % 2 for n in P.HEAD_BWD_SWEEP_N)        # the wide kernel's half-empty row pair
    assert {n % 4 for n in P.HEAD_FWD_SWEEP_N} == {0, 1, 2, 3}   # last groups of 1..4 rows
    assert P.HEAD_CROSS_N == 37 and 37 % 4 == 1


def test_layer_shapes_cover_every_band_and_chunk_edge():
    shapes = P.layer_shapes()
    assert {P.layer_fp(F) for _, F, _ in shapes} == {2, 4, 8, 16, 32, 64}
    for lo, hi in ((1, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, 64)):
        assert lo in P.LAYER_F and hi in P.LAYER_F and P.layer_fp(lo) == P.layer_fp(hi)
    for F in P.LAYER_F:
        assert len({n for n, f, _ in shapes if f == F}) >= 3, F
    for H in P.LAYER_H:
        assert len({n for n, _, h in shapes if h == H}) >= 3, H
    for n in P.LAYER_N:
        assert len({f for m, f, _ in shapes if m == n}) >= 2, n
    assert {n % 64 for n in P.LAYER_N} >= {1, 3, 5, 17, 63, 0}
    n, F, H = P.LAYER_TWO_CHUNKS
    assert (n, F, H) == (16449, 2, 64) and n == 256 * 64 + 65 and (n, F, H) in shapes


def test_optim_cases_cover_the_sizes_and_snapshot_patterns():
    cases = P.optim_cases().values()
    assert {c.count for c in cases} == {1, 8, 9, 16}
    for count, sizes in P.OPTIM_SIZES.items():
        assert len(sizes) == count and 262145 in sizes
        if count >= 8:
            assert {0, 1, 255, 256, 257} <= set(sizes)
    assert 262145 == 1024 * 256 + 1
    assert 262145 in P.OPTIM_SIZES[9][8:] and 262145 in P.OPTIM_SIZES[16][8:]  # second launch
    for kind in (0, 1):
        assert {c.snaps for c in cases if c.kind == kind} == set(P.OPTIM_SNAPS)


# ---------------------------------------------------------------------------------------------
# the kernels' summation shape in numpy, with optional mistakes (one flag each)
# ---------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.numpy()


def _out(buf, value):
    value = torch.as_tensor(np.ascontiguousarray(value))
    return value if buf is None else buf.copy_(value.reshape(buf.shape))


def _lanes_forward(no_eps=False, mask_z=False, drop_col=False, drop_act=False):
    """head_fwd16_kernel's order: lane q of 16 adds the products of columns q, q + 16, ... in turn,
    the 16 lane sums meet in a 4-step exchange tree, the bias comes last."""
    def head_forward(z, Wm, bm, log_std, act, bz=None, mu_out=None, logp_out=None):
        zn, W = _np(z), _np(Wm)
        n, H = zn.shape
        A = W.shape[0]
        pre = zn + _np(bz) if bz is not None else zn
        x = np.where(zn > 0, pre, 0.0) if mask_z else np.maximum(pre, 0.0)
        Hp = -(-H // 16) * 16
        xp, Wp = np.zeros((n, Hp)), np.zeros((A, Hp))
        xp[:, :H - 1 if drop_col else H] = x[:, :H - 1 if drop_col else H]
        Wp[:, :H] = W
        acc = np.zeros((n, A, 16))
        for j in range(Hp // 16):
            acc = acc + xp[:, None, 16 * j:16 * j + 16] * Wp[None, :, 16 * j:16 * j + 16]
        for bit in (8, 4, 2, 1):
            acc = acc + acc[..., np.arange(16) ^ bit]
        mu = acc[..., 0] + _np(bm)
        ls = _np(log_std)
        sd = np.exp(ls) + (0.0 if no_eps else 1e-7)
        d = _np(act) - mu
        term = -0.5 * (float(np.log(2 * np.pi)) + 2.0 * ls + d * d * (1.0 / (sd * sd)))
        logp = np.zeros(n)
        for a in range(A - 1 if drop_act else A):
            logp = logp + term[:, a]
        return _out(mu_out, mu), _out(logp_out, logp)
    return head_forward


def _records_backward(relu0=False, mask_z=False, drop_col=False, drop_act=False,
                      clamp_twice=False, drop_record=False, inv_sigma2=False, dbz_unmasked=False):
    """head_bwd_kernel's order: block b's wave w takes rows 4 b + w, + 4 nb, ...; the block's
    record [dWm | dbm | dlog_std | dbz] is its waves' sums added in order; the nb records are
    summed in 8 strided groups (each by 4 waves of every fourth record), the groups in order."""
    def head_backward(grad_logp, z, Wm, log_std, act, mu, bz=None, need_dz=True, ws=None,
                      outs=None, reduce_stream=None, defer_reduce=False):
        zn, W = _np(z), _np(Wm)
        n, H = zn.shape
        A = W.shape[0]
        pre = zn + _np(bz) if bz is not None else zn
        src = zn if mask_z else pre
        mask = src >= 0 if relu0 else src > 0
        x = np.where(src > 0, pre, 0.0) if mask_z else np.maximum(pre, 0.0)
        e = np.exp(_np(log_std))
        sd = e + 1e-7
        g = _np(grad_logp).reshape(n, 1)
        d = _np(act) - _np(mu)
        dmu = g * d * (1.0 / (sd * sd))
        tls = g * (-1.0 + d * d * ((1.0 / (sd * sd)) if inv_sigma2 else (e / (sd * sd * sd))))
        dmz = dmu.copy()
        if drop_act:
            dmz[:, A - 1] = 0.0
        dh = dmz @ W
        dz = np.where(mask, dh, 0.0)
        if drop_col:
            dz[:, H - 1] = 0.0
            x = x.copy()
            x[:, H - 1] = 0.0
        zsum = dh if dbz_unmasked else dz
        nb = P.head_bwd_records(n)

        def rows_sum(rows):
            return np.concatenate([(dmz[rows].T @ x[rows]).reshape(-1), dmz[rows].sum(axis=0),
                                   tls[rows].sum(axis=0),
                                   zsum[rows].sum(axis=0)])

        m = A * H + 2 * A + H
        recs = np.zeros((nb, m))
        for b in range(nb):
            for w in range(4):
                recs[b] = recs[b] + rows_sum(np.arange(4 * b + w, n, 4 * nb))
        if clamp_twice and n % 2 == 1:  # the row pair past n, clamped to n - 1, counted as a row
            recs[((n - 1) // 2) % nb] += rows_sum(np.array([n - 1]))
        if drop_act:
            recs[:, A * H + 2 * A - 1] = 0.0
        if drop_record:
            recs = recs[:nb - 1]
        grp = np.zeros((8, m))
        for gi in range(8):
            part = [np.zeros(m) for _ in range(4)]
            for w in range(4):
                for b in range(gi + 8 * w, recs.shape[0], 32):
                    part[w] = part[w] + recs[b]
            grp[gi] = ((part[0] + part[1]) + part[2]) + part[3]
        tot = np.zeros(m)
        for gi in range(8):
            tot = tot + grp[gi]
        o = outs if outs is not None else (None, None, None, None)
        res = (torch.as_tensor(dz) if need_dz else None, _out(o[0], tot[:A * H].reshape(A, H)),
               _out(o[1], tot[A * H:A * H + A]), _out(o[2], tot[A * H + A:A * H + 2 * A]),
               _out(o[3], tot[A * H + 2 * A:]) if bz is not None else None)
        return res + ((lambda: None),) if defer_reduce else res
    return head_backward


def _bad_layer_forward(x, W, b, out=None):
    """Features F..FP-1 not zeroed: the padded lanes read on into the next row of x and of W."""
    xn, Wn = _np(x), _np(W)
    n, F = xn.shape
    FP = P.layer_fp(F)
    xf, Wf = xn.reshape(-1), Wn.reshape(-1)
    pre = xn @ Wn.T + _np(b)
    for f in range(F, FP):
        xe = xf[np.minimum(np.arange(n) * F + f, xf.size - 1)]
        we = Wf[np.minimum(np.arange(Wn.shape[0]) * F + f, Wf.size - 1)]
        pre = pre + xe[:, None] * we[None, :]
    return _out(out, np.maximum(pre, 0.0))


def _bad_layer_backward(ge=False, stale=False):
    def layer_backward(dh, h, x, ws=None, dW_out=None, db_out=None):
        hn, xn = _np(h), _np(x)
        dz = np.where(hn >= 0 if ge else hn > 0, _np(dh), 0.0)
        dW = dz.T @ xn
        if stale:
            # a block's later chunk of nrow < 64 rows also takes rows nrow..63 of the chunk it
            # staged before, with the dz of its clamped last row
            n = xn.shape[0]
            gx = min(256, -(-n // 64))
            for r0 in range(gx * 64, n, 64):
                nrow = min(64, n - r0)
                prev = r0 - gx * 64
                for rr in range(nrow, 64):
                    dW = dW + np.outer(dz[r0 + nrow - 1], xn[prev + rr])
        return _out(dW_out, dW), _out(db_out, dz.sum(axis=0))
    return layer_backward


def _bad_optim(eps_inside=False, snap_after=False, snap_when_off=False, first_pass_only=False):
    def optim_step(kind, params, grads, exp_avg, exp_avg_sq, scalars, snapshot=None):
        sc = [float(s) for s in scalars.numpy()]
        snaps = snapshot if snapshot is not None else (None, None, None)
        srcs = (params, exp_avg if kind == 0 else None, exp_avg_sq)

        def take(i):
            for lst, src in zip(snaps, srcs):
                if lst is not None and src is not None:
                    lst[i].copy_(src[i])

        n = len(params)
        if sc[0] == 0.0:
            if snap_when_off:
                for i in range(n):
                    take(i)
            return
        for i in range(n):
            if not snap_after:
                take(i)
            lo = i // 8 * 8
            nmax = max([1] + [t.numel() for t in params[lo:lo + 8]])
            cover = min(-(-nmax // 256), 1024) * 256 if first_pass_only else params[i].numel()
            view = [t[i][:cover] if t is not None else None
                    for t in (params, grads, exp_avg, exp_avg_sq)]
            if eps_inside and kind == 0:
                p, g, m, v = (t.numpy() for t in view)
                step_size, bc2_sqrt, b1, b2, eps = sc[1:6]
                with np.errstate(all="ignore"):
                    m[...] = m + (1.0 - b1) * (g - m)
                    v[...] = v * b2 + (1.0 - b2) * (g * g)
                    p[...] = p + (-step_size) * (m / (np.sqrt(v + eps) / bc2_sqrt))
            else:
                cpu_ops.optim_step(kind, [view[0]], [view[1]], [view[2]] if kind == 0 else None,
                                   [view[3]], scalars)
            if snap_after:
                take(i)
    return optim_step


def _with(**fns):
    ns = types.SimpleNamespace(**{k: getattr(cpu_ops, k) for k in dir(cpu_ops)
                                  if not k.startswith("_")})
    for k, f in fns.items():
        setattr(ns, k, f)
    return ns


KERNEL_ORDER = _with(head_forward=_lanes_forward(), head_backward=_records_backward())


@pytest.mark.parametrize("group", list(FWD_GROUPS))
def test_lane_strided_forward_meets_the_bounds(group):
    for name in FWD_GROUPS[group]:
        for with_bz in BZ:
            P.run_head_forward(KERNEL_ORDER, DEV, P.head_fwd_cases()[name], with_bz)


@pytest.mark.parametrize("group", list(BWD_GROUPS))
def test_record_sums_backward_meets_the_bounds(group):
    for name in BWD_GROUPS[group]:
        for with_bz in BZ:
            P.run_head_backward(KERNEL_ORDER, DEV, P.head_bwd_cases()[name], with_bz)


@pytest.mark.parametrize("name", P.HEAD_CHAIN)
def test_kernel_order_chain_meets_the_bounds(name):
    P.run_head_chain(KERNEL_ORDER, DEV, P.head_bwd_cases()[name], True)


# ---------------------------------------------------------------------------------------------
# negative controls: one mistake each; at least one case of the family must fail
# ---------------------------------------------------------------------------------------------
def _control_names(cases):
    """The family a control runs: the special cases, the row sweeps up to 1025 rows at two
    shapes, and the cross product at its smallest, a middle and its largest hidden width."""
    keep = []
    for k, c in cases.items():
        if k.startswith("x_"):
            if c.H in (1, 65, 300, 512):
                keep.append(k)
        elif k.startswith("n"):
            if c.n <= 1025 and (c.H, c.A) in ((33, 3), (300, 17)):
                keep.append(k)
        else:
            keep.append(k)
    return keep


def _family(ops, family):
    if family == "head_forward":
        c = P.head_fwd_cases()
        return [lambda k=k, b=b: P.run_head_forward(ops, DEV, c[k], b)
                for k in _control_names(c) for b in BZ]
    if family == "head_backward":
        c = P.head_bwd_cases()
        return [lambda k=k, b=b: P.run_head_backward(ops, DEV, c[k], b)
                for k in _control_names(c) for b in BZ]
    if family == "layer":
        return [lambda c=c: P.run_layer(ops, DEV, c) for c in P.layer_cases().values()]
    if family == "optim":  # the cases with a snapshot list, so every control has something to miss
        return [lambda c=c: P.run_optim(ops, DEV, c) for c in P.optim_cases().values()
                if c.snaps is not None and c.count >= 8]
    raise KeyError(family)


def _fails_somewhere(runs):
    failed = 0
    for run in runs:
        try:
            run()
        except AssertionError:
            failed += 1
    return failed


CONTROLS = {
    "sigma_without_1e-7": ("head_forward", dict(head_forward=_lanes_forward(no_eps=True))),
    "forward_mask_from_z_not_z_plus_bz": ("head_forward",
                                          dict(head_forward=_lanes_forward(mask_z=True))),
    "forward_drops_last_column": ("head_forward", dict(head_forward=_lanes_forward(drop_col=True))),
    "forward_drops_last_action": ("head_forward", dict(head_forward=_lanes_forward(drop_act=True))),
    "backward_mask_from_z_not_z_plus_bz": ("head_backward",
                                           dict(head_backward=_records_backward(mask_z=True))),
    "relu_derivative_at_0_is_1": ("head_backward",
                                  dict(head_backward=_records_backward(relu0=True))),
    "backward_drops_last_column": ("head_backward",
                                   dict(head_backward=_records_backward(drop_col=True))),
    "backward_drops_last_action": ("head_backward",
                                   dict(head_backward=_records_backward(drop_act=True))),
    "clamped_row_past_n_counted_again": ("head_backward",
                                         dict(head_backward=_records_backward(clamp_twice=True))),
    "last_partial_record_dropped": ("head_backward",
                                    dict(head_backward=_records_backward(drop_record=True))),
    "dlog_std_with_1_over_sigma2": ("head_backward",
                                    dict(head_backward=_records_backward(inv_sigma2=True))),
    "dbz_from_unmasked_dz": ("head_backward",
                             dict(head_backward=_records_backward(dbz_unmasked=True))),
    "layer_backward_mask_h_ge_0": ("layer", dict(layer_backward=_bad_layer_backward(ge=True))),
    "layer_backward_adds_previous_chunk": ("layer",
                                           dict(layer_backward=_bad_layer_backward(stale=True))),
    "layer_features_past_F_not_zeroed": ("layer", dict(layer_forward=_bad_layer_forward)),
    "adam_eps_inside_the_square_root": ("optim", dict(optim_step=_bad_optim(eps_inside=True))),
    "snapshot_taken_after_the_update": ("optim", dict(optim_step=_bad_optim(snap_after=True))),
    "disabled_step_still_writes_snapshot": ("optim",
                                            dict(optim_step=_bad_optim(snap_when_off=True))),
    "second_grid_pass_left_untouched": ("optim", dict(optim_step=_bad_optim(first_pass_only=True))),
}
CONTROL_FAILURES = {}


@pytest.mark.parametrize("control", list(CONTROLS))
def test_negative_control_is_caught(control):
    family, fns = CONTROLS[control]
    saved, saved_bits = dict(P.RATIOS), dict(P.OPTIM_BITS)  # a wrong stand-in measures nothing
    try:
        runs = _family(_with(**fns), family)
        failed = _fails_somewhere(runs)
    finally:
        P.RATIOS.clear()
        P.RATIOS.update(saved)
        P.OPTIM_BITS.clear()
        P.OPTIM_BITS.update(saved_bits)
    CONTROL_FAILURES[control] = (failed, len(runs))
    print(f"{control}: {failed} of {len(runs)} {family} cases fail")
    assert failed >= 1, f"{control}: no case of the {family} family noticed it"


# ---------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------
def test_bounds_reject_a_tenth_of_a_dropped_term():
    """At n = 517 a tenth of one row's contribution to dWm, dbm, dlog_std and dW1 is outside the
    bound, while the reference rounded to f64 is inside it."""
    row = 258
    for name in ("n517_H300_A2", "n517_H300_A17"):
        c, ref = P.head_bwd_cases()[name], P.head_bwd_reference(name, True)
        assert c.g[row] != 0
        z, bz = P.head_inputs(c, True)
        s = P._sigma_terms(c.log_std)
        d = P.ld(c.act[row]) - P.ld(P.head_bwd_mu(c, True)[row])
        dmu = P.ld(c.g[row]) * d * s.inv
        x = np.maximum(P.ld(z[row]) + P.ld(bz), 0)
        parts = {"dWm": (ref.dWm, ref.bdWm, np.outer(dmu, x)), "dbm": (ref.dbm, ref.bdbm, dmu),
                 "dls": (ref.dls, ref.bdls, P.ld(c.g[row]) * (-1 + d * d * s.es3))}
        for key, (val, bound, term) in parts.items():
            assert np.any(term != 0)
            P.check("sharp_ok", np.asarray(val, dtype=np.float64), val, bound)
            with pytest.raises(AssertionError):
                P.check("sharp_bad", np.asarray(val - term / 10, dtype=np.float64), val, bound)
    lname = next(k for k, c in P.layer_cases().items() if c.n == 517)
    c, ref = P.layer_cases()[lname], P.layer_reference(lname)
    term = np.outer(np.where(ref.h[row] > 0, c.dh[row], 0), c.x[row])
    assert np.any(term != 0)
    P.check("sharp_ok", np.asarray(ref.bwd.dW, dtype=np.float64), ref.bwd.dW, ref.bwd.bdW)
    with pytest.raises(AssertionError):
        P.check("sharp_bad", np.asarray(ref.bwd.dW - P.ld(term) / 10, dtype=np.float64),
                ref.bwd.dW, ref.bwd.bdW)
    P.RATIOS.pop("sharp_ok", None)
    P.RATIOS.pop("sharp_bad", None)
