"""TRPO's mean-layer and batch kernels op by op: 80-bit references, exact restatements, edges.

Every case of tests/trpo_cases.py (mean_tangent_kernel, mean_bwd_kernel of csrc/head.hip) and of
tests/goal_rl_cases.py's families (traj_budget_kernel, gae_kernel, std_partial / std_apply of
csrc/trpo_batch.hip) goes through mepol_amd.ops with the checkers that the host files
(test_trpo_cases_host.py, test_goal_rl_cases_host.py) apply to the CPU stand-ins: the mean layer
within m u0 A of the np.longdouble reference, traj_budget and gae exactly / bit-equal to the
sequential restatements, standardize within the fixed-order bound.  The shapes are the smallest
that reach each branch (the host files assert which).  Every op runs twice, same bits.
"""
import types

import numpy as np
import pytest
import torch

import goal_rl_cases as C
import trpo_cases as T

TAN_GROUPS, BWD_GROUPS = T.tangent_groups(), T.backward_groups()
CASES = T.mean_cases()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    return gpu_ops


def _same(a, b):
    for key in a:
        assert T.bits_equal(a[key], b[key]), key


# ---------------------------------------------------------------------------------------------
# mean layer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(TAN_GROUPS))
def test_mean_tangent(cuda, ops, group):
    for name in TAN_GROUPS[group]:
        for with_bz in T.variants(name):
            _same(T.run_mean_tangent(ops, cuda, CASES[name], with_bz),
                  T.run_mean_tangent(ops, cuda, CASES[name], with_bz))


@pytest.mark.parametrize("group", list(BWD_GROUPS))
def test_mean_backward(cuda, ops, group):
    """One call, checked; need_dz=False and nan-filled outs=, dz_out= and ws= with the one
    call's bits; the whole of it twice."""
    for name in BWD_GROUPS[group]:
        for with_bz in T.variants(name):
            _same(T.run_mean_backward(ops, cuda, CASES[name], with_bz),
                  T.run_mean_backward(ops, cuda, CASES[name], with_bz))


@pytest.mark.parametrize("with_bz", [True, False])
@pytest.mark.parametrize("name", T.MEAN_CHAIN)
def test_mean_tangent_then_backward(cuda, ops, name, with_bz):
    a = T.run_mean_chain(ops, cuda, CASES[name], with_bz)
    b = T.run_mean_chain(ops, cuda, CASES[name], with_bz)
    assert all(T.bits_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# batch kernels
# ---------------------------------------------------------------------------------------------
def _budget_into_ff(ops):
    """ops with a traj_budget that hands the entry point outputs whose bytes are all 0xff: every
    one of the n + n + (n + 1) + 2 words must be written (-1 is no value of the restatement)."""
    from mepol_amd._lib import call, ptr

    def traj_budget(lens, dones, budget):
        n = lens.numel()
        dev = lens.device
        outs = (torch.full((n,), -1, dtype=torch.int32, device=dev),
                torch.full((n,), -1, dtype=torch.int32, device=dev),
                torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
                torch.full((2,), -1, dtype=torch.int64, device=dev))
        call("mepol_traj_budget", ptr(lens), ptr(dones), n, int(budget), *(ptr(o) for o in outs),
             ops._stream())
        return outs

    return types.SimpleNamespace(traj_budget=traj_budget)


@pytest.mark.parametrize("name", list(C.budget_cases()))
def test_traj_budget(cuda, ops, name):
    c = C.budget_cases()[name]
    C.run_budget(ops, cuda, c)
    C.run_budget(_budget_into_ff(ops), cuda, c)
    if name == C.BUDGET_BIG:
        assert C.budget_reference(name)[c.total][2][-1] > 2 ** 31


@pytest.mark.parametrize("name", list(C.gae_cases()))
def test_gae(cuda, ops, name):
    C.run_gae(ops, cuda, C.gae_cases()[name])


@pytest.mark.parametrize("name", list(C.std_cases()))
def test_standardize(cuda, ops, name):
    C.run_standardize(ops, cuda, C.std_cases()[name])


# ---------------------------------------------------------------------------------------------
# gae's guards on device-side len / offsets: the malformed trajectory writes nothing anywhere,
# every other one is bit-equal to the restatement
# ---------------------------------------------------------------------------------------------
SENTINEL = -7.25
GUARD_J = 3   # not the batch's last trajectory, and in the first workgroup of two


def _interior(arr, slack, fill, dev):
    """(whole, view): `arr` as an interior view of a larger allocation filled with `fill`."""
    a = torch.as_tensor(np.ascontiguousarray(arr))
    whole = torch.full((a.numel() + 2 * slack,), fill, dtype=a.dtype, device=dev)
    view = whole[slack:slack + a.numel()].view(a.shape)
    view.copy_(a)
    return whole, view


def _slack_untouched(whole, slack, fill):
    ends = torch.cat([whole[:slack], whole[whole.numel() - slack:]])
    return bool(torch.isnan(ends).all()) if fill != fill else bool((ends == fill).all())


GUARDS = ("len_T_plus_1", "len_minus_3", "offset_minus_1", "offset_one_past_fit", "offset_2_62")


@pytest.mark.parametrize("kind", GUARDS)
def test_gae_skips_a_malformed_trajectory(cuda, ops, kind):
    """len outside [0, T] or packed rows outside [0, n_out): nothing is written for that
    trajectory (it is never clamped: offsets was computed for the len that was given).  Every
    pointer is an interior view of a sentinel-filled allocation of the test's, with more than
    T + 1 rows of slack on both sides."""
    from mepol_amd._lib import call, ptr

    c = C.gae_case("guard", 20, 65, 3, 5, 0.995, 0.98, 650)
    j, L = GUARD_J, int(c.lens[GUARD_J])
    assert 0 < L < c.T and j < c.n - 1 and c.n > 16
    ref = C.gae_batch(c.R, c.V, c.lens, c.dones, c.S, c.A, c.gamma, c.lambd)
    lens, off = c.lens.copy(), c.off.copy()
    if kind == "len_T_plus_1":
        lens[j] = c.T + 1
    elif kind == "len_minus_3":
        lens[j] = -3
    elif kind == "offset_minus_1":
        off[j] = -1
    elif kind == "offset_one_past_fit":
        off[j] = c.n_out - L + 1
    else:
        off[j] = 2 ** 62
    slack = 4 * (c.T + 1) * max(c.nf, c.a)
    nan = float("nan")
    ins = [_interior(x, slack, f, cuda) for x, f in (
        (c.R, nan), (c.V, nan), (lens, 0), (c.dones.astype(np.int32), 0), (off, 0), (c.S, nan),
        (c.A, nan))]
    R, V, dl, dd, do, S, A = (v for _, v in ins)
    shapes = ((c.n_out,), (c.n_out,), (c.n_out, c.nf), (c.n_out, c.a))
    outs = [_interior(np.full(s, SENTINEL), slack, SENTINEL, cuda) for s in shapes]
    tg, ad, st, ac = (v for _, v in outs)
    call("mepol_gae", ptr(R), ptr(V), ptr(dl), ptr(dd), ptr(do), c.n, c.T, c.n_out, c.gamma,
         c.lambd, ptr(S), c.nf, ptr(A), c.a, ptr(tg), ptr(ad), ptr(st), ptr(ac), ops._stream())
    torch.cuda.synchronize()
    lo, hi = int(c.off[j]), int(c.off[j]) + L
    for key, got, want, (whole, _) in zip(("targets", "adv", "states", "actions"),
                                          (tg, ad, st, ac), ref, outs):
        assert _slack_untouched(whole, slack, SENTINEL), (kind, key, "written outside n_out rows")
        want = np.array(want, dtype=np.float64)
        want[lo:hi] = SENTINEL
        g = got.cpu().numpy()
        assert np.array_equal(g[lo:hi], want[lo:hi]), (kind, key, "the malformed row was written")
        assert np.array_equal(g.view(np.int64), want.view(np.int64)), (kind, key)
    for (whole, _), fill in zip(ins, (nan, nan, 0, 0, 0, nan, nan)):
        assert _slack_untouched(whole, slack, fill)


# ---------------------------------------------------------------------------------------------
# host-side refusals of the mean layer: nothing is launched, nothing is written
# ---------------------------------------------------------------------------------------------
N, H, A = 8, 64, 2


@pytest.fixture()
def bufs(cuda, ops):
    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float64, device=cuda)

    t = dict(t=full(N, H), z=full(N, H), bz=full(H), Wm=full(A, H), dWm_in=full(A, H),
             dbm_in=full(A), scale=full(A), c=full(N, A), dz=full(N, H), dWm=full(A, H),
             dbm=full(A), dbz=full(H))
    t["ws"] = ops.mean_backward_workspace(N, H, A, cuda)
    yield t
    torch.cuda.synchronize()
    for key, v in t.items():
        if v.dtype == torch.float64:
            assert bool((v == SENTINEL).all()), f"{key} was written"


def _mean_tan(t, n, hidden, a_dim, st):
    from mepol_amd._lib import call, ptr

    call("mepol_mean_tangent", ptr(t["t"]), ptr(t["z"]), n, hidden, ptr(t["bz"]), ptr(t["Wm"]),
         ptr(t["dWm_in"]), ptr(t["dbm_in"]), ptr(t["scale"]), a_dim, ptr(t["c"]), st)


def _mean_bwd(t, n, hidden, a_dim, st, ws_bytes=None):
    from mepol_amd._lib import call, ptr

    ws = t["ws"]
    call("mepol_mean_backward", ptr(t["c"]), ptr(t["z"]), n, hidden, ptr(t["bz"]), ptr(t["Wm"]),
         a_dim, ptr(t["dz"]), ptr(t["dWm"]), ptr(t["dbm"]), ptr(t["dbz"]), ptr(ws),
         ws.numel() if ws_bytes is None else ws_bytes, st)


def test_mean_sizes_past_the_kernels_limits_are_refused(cuda, ops, bufs):
    from mepol_amd._lib import MepolError

    st = ops._stream()
    for hidden, a_dim in ((513, A), (H, 33)):
        with pytest.raises(MepolError, match="rc=1003"):
            _mean_tan(bufs, N, hidden, a_dim, st)
        with pytest.raises(MepolError, match="rc=1003"):
            _mean_bwd(bufs, N, hidden, a_dim, st)


def test_mean_backward_workspace_one_byte_short_is_refused(cuda, ops, bufs):
    from mepol_amd._lib import MepolError, MepolInputError

    need = bufs["ws"].numel()
    assert need == ops._ws_bytes("mean_backward", N, H, A)
    with pytest.raises(MepolError, match="rc=1002") as err:
        _mean_bwd(bufs, N, H, A, ops._stream(), ws_bytes=need - 1)
    assert not isinstance(err.value, MepolInputError)


def test_mean_zero_rows(cuda, ops, bufs):
    """n <= 0: the tangent succeeds and writes nothing; the backward refuses it (bad argument), as
    head_backward and layer_backward do: its outputs are sums over rows, written, not
    accumulated, and a silent success would leave the caller's bytes in them."""
    from mepol_amd._lib import MepolInputError

    st = ops._stream()
    _mean_tan(bufs, 0, H, A, st)
    for n in (0, -1):
        with pytest.raises(MepolInputError):
            _mean_bwd(bufs, n, H, A, st)
