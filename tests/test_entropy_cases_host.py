"""The entropy-op cases through the CPU stand-ins, and the negative controls (no GPU).

Two things are shown here, on any machine:
  * the plain-f64 numpy stand-ins of tests/cpu_ops.py (and a numpy restatement of the kernels'
    64-lane chunked scans) meet every bound of tests/entropy_cases.py, so the bounds are not
    tighter than correct f64 arithmetic can be;
  * a set of deliberately wrong stand-ins, each with one of the mistakes such kernels make,
    fails at least one case, so the cases and bounds would notice that mistake in a kernel.
tests/test_gpu_entropy_ops.py runs the same cases and checkers over the HIP kernels.
"""
import types

import numpy as np
import pytest
import torch

import cpu_ops
import entropy_cases as E

DEV = "cpu"


# ---------------------------------------------------------------------------------------------
# every case through the stand-ins
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.iw_cases()))
def test_iw(name):
    E.run_iw(cpu_ops, DEV, E.iw_cases()[name])


@pytest.mark.parametrize("name", list(E.entropy_cases()))
def test_entropy_forward(name):
    E.run_entropy(cpu_ops, DEV, E.entropy_cases()[name])


def test_entropy_forward_emit_twice():
    c = E.entropy_cases()
    E.run_entropy_emit(cpu_ops, DEV, c["ns7_eps1e-15"], c["ns2_eps0"])


@pytest.mark.parametrize("name", list(E.table_cases()))
def test_csr_tables_are_valid(name):
    """The generator's own promises: ids in range, the hub list's length, the empty ids."""
    c = E.table_cases()[name]
    assert c.idxT.dtype == np.int32 and c.idxT.shape == (c.k, c.nq)
    assert c.idxT.min() >= 0 and c.idxT.max() < c.n_ids
    off, rows, _, _ = E.csr_reference(name)
    assert off[0] == 0 and off[-1] == c.nq * c.k and np.all(np.diff(off) >= 0)
    if c.hub_len:
        assert off[c.hub + 1] - off[c.hub] == c.hub_len
    for j in c.empties:
        assert off[j + 1] == off[j]


@pytest.mark.parametrize("name,world", [("hub129_k2", 2), ("hub129_k2", 3), ("hub208_k30", 2),
                                        ("hub208_k30", 3), ("nq1_k30", 2), ("n4095_k2", 3)])
def test_csr_rank_slices_concatenate(name, world):
    E.run_csr(cpu_ops, DEV, E.table_cases()[name], world)


@pytest.mark.parametrize("name", list(E.gamma_cases()))
def test_gamma(name):
    E.run_gamma(cpu_ops, DEV, E.gamma_cases()[name])


@pytest.mark.parametrize("gH", [1.0, -1.0, 0.37])
@pytest.mark.parametrize("name", list(E.reverse_cases()))
def test_reverse_scan(name, gH):
    E.run_reverse(cpu_ops, DEV, E.reverse_cases()[name], gH)


@pytest.mark.parametrize("world,n,nt", E.GATHER_SHAPES)
def test_gathered_normalise_and_emit(world, n, nt):
    c = E.gather_case(world, n, nt)
    E.run_gathered(cpu_ops, DEV, c)
    E.run_emit(cpu_ops, DEV, c)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_sliced_round_trip(world):
    E.run_chain(cpu_ops, DEV, world)


def test_ragged_chain_feeds_the_reverse_scan():
    E.run_chain(cpu_ops, DEV, 1, 0.37, "ragged_drift")


def test_chain_case_is_ragged_and_splits_evenly():
    c = E.chain_case().iw  # even3000
    assert c.N == 3000 and 0 in c.lengths and max(c.lengths) <= c.T
    for world in (2, 3):
        per = c.nt // world
        assert [int(c.offsets[r * per]) for r in range(world + 1)] == [
            r * c.N // world for r in range(world + 1)]


# ---------------------------------------------------------------------------------------------
# the kernels' scan shape in numpy: one 64-lane wave per trajectory, chunk = ceil(len / 64)
# ---------------------------------------------------------------------------------------------
def _wave_scan(s, strict, reverse=False):
    """Inclusive Hillis-Steele scan over 64 lane values (suffix scan with reverse).  strict is
    the mistake `l > m` for `l >= m`: lane m misses the carry of step m."""
    incl = s.copy()
    lanes = np.arange(E.LANES)
    m = 1
    while m < E.LANES:
        o = np.zeros_like(incl)
        if reverse:
            o[:-m] = incl[m:]
            take = lanes + m < E.LANES
        else:
            o[m:] = incl[:-m]
            take = lanes > m if strict else lanes >= m
        incl = np.where(take, incl + o, incl)
        m *= 2
    return incl


def _chunked_iw_forward(strict):
    def iw_forward(logp_t, logp_b, offsets, n_particles, normalize=True):
        lt, lb, off = logp_t.numpy(), logp_b.numpy(), offsets.numpy()
        u, ts = np.zeros(n_particles), np.zeros(lt.shape[0])
        for n in range(lt.shape[0]):
            L = int(off[n + 1] - off[n])
            chunk = -(-L // E.LANES)
            d = lt[n, :L] - lb[n, :L]
            s = np.array([d[l * chunk:(l + 1) * chunk].sum() for l in range(E.LANES)])
            run = _wave_scan(s, strict) - s
            for l in range(E.LANES):
                b, e = l * chunk, min(L, (l + 1) * chunk)
                if b < e:
                    u[off[n] + b:off[n] + e] = np.exp(run[l] + np.cumsum(d[b:e]))
            ts[n] = u[off[n]:off[n + 1]].sum()
        u, ts = torch.as_tensor(u), torch.as_tensor(ts)
        if not normalize:
            return u, ts, None, None
        U = ts.sum()
        return u, ts, u / U, U
    return iw_forward


def _chunked_reverse_scan(zero_tail):
    def entropy_reverse_scan(gamma, w, partials, nparts, offsets, nt, T_stride, grad_H,
                             S_ext=None):
        S = float(S_ext) if S_ext is not None else float(partials[:nparts].sum())
        c = (gamma.numpy() - S) * w.numpy()
        off = offsets.numpy()
        out = np.full((nt, T_stride), np.nan)
        for n in range(nt):
            L = int(off[n + 1] - off[n])
            chunk = -(-L // E.LANES)
            seg = c[off[n]:off[n + 1]]
            s = np.array([seg[l * chunk:(l + 1) * chunk].sum() for l in range(E.LANES)])
            run = _wave_scan(s, False, reverse=True) - s
            for l in range(E.LANES):
                b, e = l * chunk, min(L, (l + 1) * chunk)
                if b < e:
                    out[n, b:e] = float(grad_H) * (run[l] + np.cumsum(seg[b:e][::-1])[::-1])
            if zero_tail:
                out[n, L:] = 0.0
        return torch.as_tensor(out)
    return entropy_reverse_scan


def _with(**fns):
    ns = types.SimpleNamespace(**{k: getattr(cpu_ops, k) for k in dir(cpu_ops)
                                  if not k.startswith("_")})
    for k, f in fns.items():
        setattr(ns, k, f)
    return ns


@pytest.mark.parametrize("name", ["ragged", "ragged_drift", "nt4_zero_ends", "nt2049"])
def test_chunked_scan_meets_the_iw_bounds(name):
    """The kernels' summation order (lane chunks, wave scan, `incl - s`) is inside the bounds."""
    E.run_iw(_with(iw_forward=_chunked_iw_forward(False)), DEV, E.iw_cases()[name])


@pytest.mark.parametrize("name", list(E.reverse_cases()))
def test_chunked_reverse_scan_meets_the_bounds(name):
    E.run_reverse(_with(entropy_reverse_scan=_chunked_reverse_scan(True)), DEV,
                  E.reverse_cases()[name], 0.37)


# ---------------------------------------------------------------------------------------------
# negative controls: one mistake each; at least one case of the family must fail
# ---------------------------------------------------------------------------------------------
def _bad_gamma(skip_second_pass=False, drop_tail=False):
    def entropy_gamma(g, w_own, csr_off, csr_rows):
        g, w = g.numpy(), w_own.numpy()
        off, rows = csr_off.numpy(), csr_rows.numpy()
        n = w.shape[0]
        gamma = np.zeros(n)
        for j in range(n if not skip_second_pass else min(n, E.GAMMA_STRIDE)):
            b, e = int(off[j]), int(off[j + 1])
            if drop_tail:
                e -= (e - b) % 16
            gamma[j] = g[rows[b:e]].sum()
        return torch.as_tensor(gamma), torch.as_tensor(np.array([(gamma * w).sum()])), 1
    return entropy_gamma


def _bad_csr_build(idxT, k, n_own, col_offset=0, row_offset=0, nq=None):
    return cpu_ops.csr_build(idxT, k, n_own, col_offset=0, row_offset=row_offset, nq=nq)


def _bad_gathered(xu_all, world, n, nt, w_out):
    x = xu_all.numpy()
    U = sum(x[r * n + n:r * n + n + nt].sum() for r in range(world))
    for r in range(world):
        w_out[r * n:(r + 1) * n] = torch.as_tensor(x[r * n:r * n + n] / U)
    return w_out


def _bad_entropy_kl_by_n(w, idxT, D, k, ns, G, B, eps, n_w=None, **kw):
    out4, W, g = cpu_ops.entropy_forward(w, idxT, D, k, ns, G, B, eps, n_w=n_w, **kw)
    out4[1] = out4[3] / D.shape[0]
    return out4, W, g


def _bad_emit_new_h(w, idxT, D, k, ns, G, B, eps, n_w=None, g_out=None, out4=None, vals=None):
    res = cpu_ops.entropy_forward(w, idxT, D, k, ns, G, B, eps, n_w=n_w, g_out=g_out, out4=out4,
                                  vals=vals)
    if vals is not None:
        vals[0] = out4[0]
    return res


def _bad_sharded_emit_new_h(x_all, world, stride, off, B, n_global, sums_cur, vals):
    cpu_ops.sharded_emit(x_all, world, stride, off, B, n_global, sums_cur, vals)
    vals[0] = B - float(sums_cur[0])


def _fails_somewhere(runs):
    """Number of the given thunks that raise AssertionError (each runs one case)."""
    failed = 0
    for run in runs:
        try:
            run()
        except AssertionError:
            failed += 1
    return failed


def _family(ops, family):
    if family == "iw":
        return [lambda c=c: E.run_iw(ops, DEV, c) for c in E.iw_cases().values()]
    if family == "entropy":
        return [lambda c=c: E.run_entropy(ops, DEV, c) for c in E.entropy_cases().values()]
    if family == "emit":
        c = E.entropy_cases()
        return [lambda: E.run_entropy_emit(ops, DEV, c["ns7_eps1e-15"], c["ns2_eps0"])]
    if family == "csr":
        t = E.table_cases()
        return [lambda w=w: E.run_csr(ops, DEV, t["hub129_k2"], w) for w in (2, 3)]
    if family == "gamma":
        return [lambda c=c: E.run_gamma(ops, DEV, c) for c in E.gamma_cases().values()]
    if family == "reverse":
        return [lambda c=c: E.run_reverse(ops, DEV, c, -1.0) for c in E.reverse_cases().values()]
    if family == "gathered":
        return [lambda s=s: E.run_gathered(ops, DEV, E.gather_case(*s)) for s in E.GATHER_SHAPES]
    if family == "sharded_emit":
        return [lambda s=s: E.run_emit(ops, DEV, E.gather_case(*s)) for s in E.GATHER_SHAPES]
    raise KeyError(family)


CONTROLS = {
    "scan_drops_lane_boundary_carry": ("iw", dict(iw_forward=_chunked_iw_forward(True))),
    "reverse_scan_leaves_padded_tail": ("reverse",
                                        dict(entropy_reverse_scan=_chunked_reverse_scan(False))),
    "gamma_skips_second_grid_stride_pass": ("gamma",
                                            dict(entropy_gamma=_bad_gamma(skip_second_pass=True))),
    "gamma_drops_len_mod_16_tail": ("gamma", dict(entropy_gamma=_bad_gamma(drop_tail=True))),
    "csr_build_ignores_col_offset": ("csr", dict(csr_build=_bad_csr_build)),
    "gathered_normalise_stride_n": ("gathered", dict(iw_normalize_gathered=_bad_gathered)),
    "kl_divided_by_n_not_n_w": ("entropy", dict(entropy_forward=_bad_entropy_kl_by_n)),
    "emit_returns_new_h": ("emit", dict(entropy_forward=_bad_emit_new_h)),
    "sharded_emit_returns_new_h": ("sharded_emit",
                                   dict(sharded_emit=_bad_sharded_emit_new_h)),
}
CONTROL_FAILURES = {}


@pytest.mark.parametrize("control", list(CONTROLS))
def test_negative_control_is_caught(control):
    family, fns = CONTROLS[control]
    saved = dict(E.RATIOS)  # a wrong stand-in's ratios are not measurements
    try:
        runs = _family(_with(**fns), family)
        failed = _fails_somewhere(runs)
    finally:
        E.RATIOS.clear()
        E.RATIOS.update(saved)
    CONTROL_FAILURES[control] = (failed, len(runs))
    assert failed >= 1, f"{control}: no case of the {family} family noticed it"


def test_the_unmutated_families_pass():
    """The same family lists the controls run, over the right stand-ins: none fails."""
    for family in sorted({f for f, _ in CONTROLS.values()}):
        assert _fails_somewhere(_family(cpu_ops, family)) == 0, family


def test_bounds_reject_a_tenth_of_a_dropped_term():
    """Sharpness: weights off by 0.1 / N relative (a tenth of what one dropped 1/N term does)
    fail their bound, while the reference rounded to f64 passes it."""
    c = E.iw_cases()["ragged"]
    ref = E.iw_reference("ragged")
    w = np.asarray(ref.w, dtype=np.float64)
    E.check("w_sharpness_ok", w, ref.w, ref.bw)
    with pytest.raises(AssertionError):
        E.check("w_sharpness_bad", w * (1 + 0.1 / c.N), ref.w, ref.bw)
    E.RATIOS.pop("w_sharpness_ok", None)
    E.RATIOS.pop("w_sharpness_bad", None)
