"""The mean-layer cases through the CPU stand-ins, their coverage, and the negative controls.

No GPU.  As tests/test_policy_cases_host.py does for the Gaussian head, this file shows that
  * the plain-f64 numpy stand-ins of tests/cpu_ops.py (mean_tangent, mean_backward) meet every
    bound of tests/trpo_cases.py, and so does a second set that sums in the kernels' shape (16
    lanes of strided columns and an exchange tree in the tangent; row pairs at stride 2 nb, one
    record per block, the records in 8 strided groups in the backward);
  * stand-ins with one mistake each fail at least one case, so the cases and bounds would notice
    that mistake in a kernel;
  * the case lists reach every template instantiation, chunk size, wave count and record count
    that the launchers' selection lines (restated in trpo_cases.py) can choose.
tests/test_gpu_trpo_ops.py runs the same cases and checkers over the HIP kernels.
"""
import types

import numpy as np
import pytest
import torch

import cpu_ops
import trpo_cases as T

DEV = "cpu"
TAN_GROUPS, BWD_GROUPS = T.tangent_groups(), T.backward_groups()
CASES = T.mean_cases()


@pytest.mark.parametrize("group", list(TAN_GROUPS))
def test_mean_tangent(group):
    for name in TAN_GROUPS[group]:
        for with_bz in T.variants(name):
            T.run_mean_tangent(cpu_ops, DEV, CASES[name], with_bz)


@pytest.mark.parametrize("group", list(BWD_GROUPS))
def test_mean_backward(group):
    for name in BWD_GROUPS[group]:
        for with_bz in T.variants(name):
            T.run_mean_backward(cpu_ops, DEV, CASES[name], with_bz)


@pytest.mark.parametrize("with_bz", [True, False])
@pytest.mark.parametrize("name", T.MEAN_CHAIN)
def test_mean_tangent_then_backward(name, with_bz):
    T.run_mean_chain(cpu_ops, DEV, CASES[name], with_bz)


# ---------------------------------------------------------------------------------------------
# coverage of the case lists
# ---------------------------------------------------------------------------------------------
def _tangent_shapes():
    return [(CASES[k].n, CASES[k].H, CASES[k].A) for names in TAN_GROUPS.values() for k in names]


def _backward_shapes():
    return [(CASES[k].n, CASES[k].H, CASES[k].A) for names in BWD_GROUPS.values() for k in names]


def test_tangent_cases_reach_every_instance_chunk_and_row_group():
    inst = [T.tangent_instance(*s) for s in _tangent_shapes()]
    assert {i.ap for i in inst} == {1, 2, 4, 8}
    assert {i.nch for i in inst} == {1, 2, 3, 4}
    # a last action chunk of every size the chunked kernel (AP = 8, A <= 32) can be left with
    assert {i.last_chunk for i in inst if i.ap == 8} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {i.last_chunk for i in inst if i.ap == 8 and i.nch > 1} >= {1, 2, 3, 4, 6, 7, 8}
    assert {i.last_chunk for i in inst if i.ap == 4} == {3, 4}
    assert {A for _, _, A in _tangent_shapes() if T.tangent_instance(7, 16, A).last_chunk == 1
            and A > 8} == {9, 17, 25}
    # column steps: one, both sides of 16 and of 64, the largest; a width that is no multiple of 16
    assert {i.ncl for i in inst} >= {1, 2, 4, 5, 19, 32}
    assert {H % 16 for _, H, _ in _tangent_shapes()} >= {0, 1, 2, 15}
    # rows: fewer than 4, last groups of 1..4 rows, more than one block, a wave's second group
    assert {n for n, _, _ in _tangent_shapes()} >= {1, 2, 3, 4, 5, 1025, 32768, 32769, 32773}
    assert {i.last_rows for i in inst} == {1, 2, 3, 4}
    second = {s[0] for s, i in zip(_tangent_shapes(), inst) if i.second_group}
    assert second == {32769, 32773} and not T.tangent_instance(32768, 16, 2).second_group
    assert T.tangent_instance(32769, 16, 2).gx == 2048 and T.tangent_instance(1025, 16, 2).gx == 65


def test_backward_cases_reach_every_instance_wave_count_and_record_count():
    shapes = _backward_shapes()
    inst = [T.bwd_instance(*s) for s in shapes]
    assert {i.ap for i in inst} == {2, 4, 8, 16, 32}
    assert {i.waves for i in inst} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {(i.ap, i.waves) for i in inst} >= {(ap, w) for ap in (2, 4, 8, 16, 32)
                                               for w in range(1, 9)}
    # padded actions in every AP: 1 of 2, 3 of 4, 5 and 7 of 8, 9 and 15 of 16, 17 and 31 of 32
    assert {A for _, _, A in shapes} >= {1, 3, 5, 7, 9, 15, 17, 31, 2, 4, 8, 16, 32}
    nb = {s[0]: i.nb for s, i in zip(shapes, inst)}
    assert [nb[n] for n in (1, 7, 8, 9, 57, 64, 65, 257, 4088, 4089, 4100)] == [
        1, 1, 1, 2, 8, 8, 9, 33, 511, 512, 512]
    assert any(v < 8 for v in nb.values()) and 8 in nb.values()       # empty record groups; none
    assert any(32 < v < 512 for v in nb.values()) and 512 in nb.values()  # a wave's second record
    assert T.bwd_instance(4100, 512, 32).passes >= 2                  # a second stride pass
    assert T.bwd_instance(4089, 18, 3).nb == 512 and T.bwd_instance(4089, 18, 3).passes == 4
    assert {i.half_pair for i in inst} == {True, False}               # odd n: a half-empty pair
    assert T.MEAN_CROSS_N == 7
    big = CASES[T.BWD_BIG]
    assert (big.n, big.H, big.A) == (4100, 512, 32)


def test_value_cases_hold_what_they_claim():
    c = CASES["zero_pos_A3"]
    assert (0, 0) in c.zero_pos and (c.n - 1, c.H - 1) in c.zero_pos and c.neg_zero is not None
    for name in ("signed_scale_A3", "signed_scale_A17"):
        s = CASES[name].scale
        assert s[0] == 0 and s[1] < 0 and len(set(s.tolist())) == len(s)
    for name in ("lastcol_A2", "lastcol_A9"):
        c = CASES[name]
        for with_bz in (True, False):
            pre = T.backward_reference(name, with_bz).pre
            assert np.all(pre[:, :c.H - 1] < 0) and np.all(pre[:, c.H - 1] > 0)
    for name in ("lastact_A3", "lastact_A9"):
        c = CASES[name]
        assert not c.Wm[:c.A - 1].any() and not c.dWm[:c.A - 1].any() and c.Wm[c.A - 1].all()
    assert T.tangent_instance(7, 65, 9).last_chunk == 1   # lastact_A9: alone in the last chunk
    for c in CASES.values():
        assert len(set(c.scale.tolist())) == c.A           # scale differs per action


# ---------------------------------------------------------------------------------------------
# the kernels' summation shape in numpy, with optional mistakes (one flag each)
# ---------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.numpy()


def _out(buf, value):
    value = torch.as_tensor(np.ascontiguousarray(value))
    return value if buf is None else buf.copy_(value.reshape(buf.shape))


def _lanes_tangent(mask_z=False, t_masked=False, scale_first=False, drop_col=False,
                   drop_act=False):
    """mean_tangent_kernel's order: lane q of 16 adds, for columns q, q + 16, ... in turn, the t
    Wm product and then the x dWm product; the 16 lane sums meet in a 4-step exchange tree; dbm
    is added last and the sum is scaled."""
    def mean_tangent(t, z, Wm, dWm, dbm, scale, bz=None, out=None):
        tn, zn, W, D = _np(t), _np(z), _np(Wm), _np(dWm)
        n, H = zn.shape
        A = W.shape[0]
        pre = zn + _np(bz) if bz is not None else zn
        on = (zn if mask_z else pre) > 0
        x = np.where(on, pre, 0.0)
        if t_masked:
            tn = np.where(on, tn, 0.0)
        keep = H - 1 if drop_col else H
        Hp = -(-H // 16) * 16
        xp, tp, Wp, Dp = (np.zeros((n, Hp)), np.zeros((n, Hp)), np.zeros((A, Hp)),
                          np.zeros((A, Hp)))
        xp[:, :keep], tp[:, :keep] = x[:, :keep], tn[:, :keep]
        Wp[:, :H], Dp[:, :H] = W, D
        if drop_act:  # the last action of the last chunk takes no products
            Wp[A - 1], Dp[A - 1] = 0.0, 0.0
        acc = np.zeros((n, A, 16))
        for j in range(Hp // 16):
            s = slice(16 * j, 16 * j + 16)
            acc = acc + tp[:, None, s] * Wp[None, :, s]
            acc = acc + xp[:, None, s] * Dp[None, :, s]
        for bit in (8, 4, 2, 1):
            acc = acc + acc[..., np.arange(16) ^ bit]
        v = acc[..., 0]
        c = _np(scale) * v + _np(dbm) if scale_first else _np(scale) * (v + _np(dbm))
        return _out(out, c)
    return mean_tangent


def _records_backward(relu0=False, mask_z=False, drop_col=False, drop_act=False,
                      clamp_twice=False, drop_record=False, dbm_per_wave=False,
                      dbz_unmasked=False):
    """mean_bwd_kernel's order: block b takes the row pairs 2 b, 2 b + 2 nb, ... and adds their
    terms in turn; its record is [dWm | dbm | dbz]; the nb records are summed in 8 strided groups
    (each by 4 waves of every 32nd record), the groups in order."""
    def mean_backward(c, z, Wm, bz=None, need_dz=True, ws=None, dz_out=None, outs=None):
        cn, zn, W = _np(c), _np(z), _np(Wm)
        n, H = zn.shape
        A = W.shape[0]
        pre = zn + _np(bz) if bz is not None else zn
        src = zn if mask_z else pre
        mask = src >= 0 if relu0 else src > 0
        x = np.where(src > 0, pre, 0.0) if mask_z else np.maximum(pre, 0.0)
        cz = cn.copy()
        if drop_act:
            cz[:, A - 1] = 0.0
        dh = cz @ W
        dz = np.where(mask, dh, 0.0)
        if drop_col:
            dz[:, H - 1] = 0.0
            x = x.copy()
            x[:, H - 1] = 0.0
        zsum = dh if dbz_unmasked else dz
        nb = T.bwd_records(n)
        waves = T.bwd_instance(n, H, A).waves
        m = A * H + A + H
        recs = np.zeros((nb, m))
        for b in range(nb):
            for i in range(2 * b, n, 2 * nb):
                rows = [r for r in (i, i + 1) if r < n]
                if clamp_twice and i + 1 == n:  # the row past n, clamped to n - 1, counted as a row
                    rows.append(n - 1)
                for r in rows:
                    recs[b, :A * H] += np.outer(cz[r], x[r]).reshape(-1)
                    recs[b, A * H:A * H + A] += cz[r] * (waves if dbm_per_wave else 1)
                    recs[b, A * H + A:] += zsum[r]
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
        o = outs if outs is not None else (None, None, None)
        return (_out(dz_out, dz) if need_dz else None, _out(o[0], tot[:A * H].reshape(A, H)),
                _out(o[1], tot[A * H:A * H + A]),
                _out(o[2], tot[A * H + A:]) if bz is not None else None)
    return mean_backward


def _with(**fns):
    ns = types.SimpleNamespace(**{k: getattr(cpu_ops, k) for k in dir(cpu_ops)
                                  if not k.startswith("_")})
    for k, f in fns.items():
        setattr(ns, k, f)
    return ns


KERNEL_ORDER = _with(mean_tangent=_lanes_tangent(), mean_backward=_records_backward())


def _control_names(groups, family):
    """The cases a control (and the kernel-order stand-in) runs: the special cases, the row
    sweeps up to 1025 rows (the tangent's: all), the cross product at four hidden widths."""
    keep = []
    for names in groups.values():
        for k in names:
            c = CASES[k]
            if k.startswith("x_"):
                if c.H in (1, 65, 300, 512):
                    keep.append(k)
            elif family == "tangent" or c.n <= 1025:
                keep.append(k)
    return keep


@pytest.mark.parametrize("group", list(TAN_GROUPS))
def test_lane_strided_tangent_meets_the_bounds(group):
    for name in TAN_GROUPS[group]:
        for with_bz in T.variants(name):
            T.run_mean_tangent(KERNEL_ORDER, DEV, CASES[name], with_bz)


def test_record_sums_backward_meets_the_bounds():
    for name in _control_names(BWD_GROUPS, "backward") + ["n4089_H18_A3", "n4100_H300_A2"]:
        for with_bz in T.variants(name):
            T.run_mean_backward(KERNEL_ORDER, DEV, CASES[name], with_bz)


def test_kernel_order_chain_meets_the_bounds():
    T.run_mean_chain(KERNEL_ORDER, DEV, CASES[T.MEAN_CHAIN[0]], True)


# ---------------------------------------------------------------------------------------------
# negative controls: one mistake each; at least one case of the family must fail
# ---------------------------------------------------------------------------------------------
CONTROLS = {
    "tangent_mask_from_z_not_z_plus_bz": ("tangent",
                                          dict(mean_tangent=_lanes_tangent(mask_z=True))),
    "tangent_t_masked_by_the_relu": ("tangent", dict(mean_tangent=_lanes_tangent(t_masked=True))),
    "scale_applied_before_dbm_is_added": ("tangent",
                                          dict(mean_tangent=_lanes_tangent(scale_first=True))),
    "tangent_drops_last_column": ("tangent", dict(mean_tangent=_lanes_tangent(drop_col=True))),
    "tangent_drops_last_action_of_last_chunk": ("tangent",
                                                dict(mean_tangent=_lanes_tangent(drop_act=True))),
    "backward_mask_from_z_not_z_plus_bz": ("backward",
                                           dict(mean_backward=_records_backward(mask_z=True))),
    "relu_derivative_at_0_is_1": ("backward", dict(mean_backward=_records_backward(relu0=True))),
    "backward_drops_last_column": ("backward",
                                   dict(mean_backward=_records_backward(drop_col=True))),
    "backward_drops_last_action": ("backward",
                                   dict(mean_backward=_records_backward(drop_act=True))),
    "clamped_row_past_n_counted_again": ("backward",
                                         dict(mean_backward=_records_backward(clamp_twice=True))),
    "last_partial_record_dropped": ("backward",
                                    dict(mean_backward=_records_backward(drop_record=True))),
    "dbm_counted_once_per_wave": ("backward",
                                  dict(mean_backward=_records_backward(dbm_per_wave=True))),
    "dbz_from_unmasked_c_Wm": ("backward",
                               dict(mean_backward=_records_backward(dbz_unmasked=True))),
}
CONTROL_FAILURES = {}


def _family(ops, family):
    if family == "tangent":
        return [lambda k=k, b=b: T.run_mean_tangent(ops, DEV, CASES[k], b)
                for k in _control_names(TAN_GROUPS, family) for b in T.variants(k)]
    return [lambda k=k, b=b: T.run_mean_backward(ops, DEV, CASES[k], b)
            for k in _control_names(BWD_GROUPS, family) for b in T.variants(k)]


@pytest.mark.parametrize("control", list(CONTROLS))
def test_negative_control_is_caught(control):
    family, fns = CONTROLS[control]
    saved = dict(T.RATIOS)  # a wrong stand-in measures nothing
    failed = 0
    try:
        runs = _family(_with(**fns), family)
        for run in runs:
            try:
                run()
            except AssertionError:
                failed += 1
    finally:
        T.RATIOS.clear()
        T.RATIOS.update(saved)
    CONTROL_FAILURES[control] = (failed, len(runs))
    print(f"{control}: {failed} of {len(runs)} {family} cases fail")
    assert failed >= 1, f"{control}: no case of the {family} family noticed it"


# ---------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------
def test_bounds_reject_a_tenth_of_a_dropped_term():
    """At n = 517 a tenth of one row's contribution to dWm, dbm and dbz is outside the bound,
    while the reference rounded to f64 is inside it."""
    row = 258
    c, ref = CASES[T.SHARP], T.backward_reference(T.SHARP, True)
    assert c.n == 517
    cr = T.ld(c.c[row])
    parts = {"dWm": (ref.dWm, ref.bdWm, np.outer(cr, ref.x[row])), "dbm": (ref.dbm, ref.bdbm, cr),
             "dbz": (ref.dbz, ref.bdbz, ref.dz[row])}
    for key, (val, bound, term) in parts.items():
        assert np.any(term != 0)
        T.check("sharp_ok", np.asarray(val, dtype=np.float64), val, bound)
        with pytest.raises(AssertionError):
            T.check("sharp_bad", np.asarray(val - term / 10, dtype=np.float64), val, bound)
    T.RATIOS.pop("sharp_ok", None)
    T.RATIOS.pop("sharp_bad", None)
