"""TRPO's batch-kernel cases through the CPU stand-ins, their coverage and the negative controls.

No GPU.  The case families of tests/goal_rl_cases.py (traj_budget, gae, standardize) run through
tests/cpu_ops.py with the checkers that tests/test_gpu_trpo_ops.py applies to the HIP kernels of
csrc/trpo_batch.hip; a model of the kernels' loop bounds shows that the cases reach the chunk
edges they claim to; restatements with one mistake each must fail at least one case.
"""
import types

import numpy as np
import pytest
import torch

import cpu_ops
import goal_rl_cases as C

DEV = "cpu"


@pytest.mark.parametrize("name", list(C.budget_cases()))
def test_traj_budget(name):
    C.run_budget(cpu_ops, DEV, C.budget_cases()[name])


@pytest.mark.parametrize("name", list(C.gae_cases()))
def test_gae(name):
    C.run_gae(cpu_ops, DEV, C.gae_cases()[name])


@pytest.mark.parametrize("name", list(C.std_cases()))
def test_standardize(name):
    """numpy's f64 evaluation (pairwise sums) is inside the fixed-order bound, also for the input
    with mean 1000 and std 1: std_bound asserts the derivation's second-order claim for it."""
    C.run_standardize(cpu_ops, DEV, C.std_cases()[name])


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
def test_budget_cases_reach_the_chunk_edges_and_the_int64_total():
    cases = C.budget_cases()
    assert {C.budget_chunk(c.n) for c in cases.values()} >= {1, 2, 3, 256}
    assert [C.budget_chunk(n) for n in (255, 256, 257, 511, 513, 65536)] == [1, 1, 2, 2, 3, 256]
    big = cases[C.BUDGET_BIG]
    assert big.n == 65536 and big.total == 65536 * 40000 and big.total > 2 ** 31
    ref = C.budget_reference(C.BUDGET_BIG)[big.total]
    assert int(ref[2][-1]) == big.total and ref[2].dtype == np.int64
    assert ref[3] == (65536, big.total)
    assert int(ref[2].astype(np.int32)[-1]) != big.total          # int32 offsets would wrap
    for c in cases.values():
        assert any(b > 2 ** 31 for b in c.budgets) and {0, 1} <= set(c.budgets)
        assert {c.total - 1, c.total, c.total + 7} <= set(c.budgets) | {-1}
        if c.n >= 8 and c.name != C.BUDGET_BIG:
            assert c.lens[0] == 0 and c.lens[3] == 0 and c.lens[2] > 0 and c.lens[4] > 0
            assert (c.lens < 0).any() and set(c.dones.tolist()) == set(C.DONE_VALUES)
            # a zero-length done trajectory inside the budget stays done; at the budget it is unused
            p3 = int(np.maximum(c.lens[:3], 0).sum())
            assert {p3 - 1, p3, p3 + 1} <= set(c.budgets)
            lo, do, off, (m, kept) = C.budget_reference(c.name)[p3]
            assert m == 3 and not do[3]
            assert C.budget_reference(c.name)[p3 + 1][1][3]


def test_gae_cases_reach_the_staging_chunks_and_the_partial_workgroup():
    cases = C.gae_cases()
    groups = [g for c in cases.values() for g in C.gae_chunks(c.lens)]
    assert {g[0] for g in groups} >= {0, 1, 2, 3}                # staging chunks per workgroup
    assert any(g[1] for g in groups)      # a lane ends inside an earlier chunk than the longest
    assert any(C.gae_chunks(c.lens)[-1][2] == 1 for c in cases.values() if c.n > 1)
    assert any(C.gae_chunks(c.lens)[0][2] == 16 and c.n == 16 for c in cases.values())
    lens = {int(v) for c in cases.values() for v in c.lens}
    assert {0, 1, 63, 64, 65, 129} <= lens
    for c in cases.values():
        if c.n >= 2 and c.name != "all_zero":
            first = [int(v) for v in c.lens[:16]]
            assert 1 in first and c.T in first                   # mixed in one workgroup
    assert {(c.nf, c.a) for c in cases.values()} >= set(C.GAE_DIMS)
    assert {(c.gamma, c.lambd) for c in cases.values()} >= set(C.GAE_GL)
    assert {(c.n, c.T) for c in cases.values()} >= {(n, T) for n in C.GAE_N for T in C.GAE_T}
    for c in cases.values():   # behind len everything is nan, values[i, len] of a done one too
        for i in range(c.n):
            L = int(c.lens[i])
            assert np.isnan(c.R[i, L:]).all() and np.isnan(c.V[i, L + 1:]).all()
            assert np.isnan(c.S[i, L:]).all() and np.isnan(c.A[i, L:]).all()
            assert np.isnan(c.V[i, L]) == bool(c.dones[i])
    assert any(not c.dones[i] and c.lens[i] > 0 for c in cases.values() for i in range(c.n))


def test_rewards_are_not_short_decimals():
    """The widening of a reward has more digits than its f32 shortest form: converting late (after
    an f32 operation) or through a decimal would change the f64 value."""
    for c in C.gae_cases().values():
        r = c.R[np.isfinite(c.R)]
        if r.size:
            assert all(repr(float(v)) != str(v) and len(repr(float(v))) > 12 for v in r[:50])


def test_standardize_cases_sit_at_the_block_edges():
    blocks = {c.N: -(-c.N // C.STD_BLOCK) for c in C.std_cases().values()}
    assert [blocks[n] for n in (2047, 2048, 2049, 8192, 8193, 32769)] == [1, 1, 2, 4, 5, 17]
    assert {255, 256, 257} <= set(blocks)                        # the 256-thread edge
    far = [c for c in C.std_cases().values() if c.name.startswith("far")]
    assert far and all(abs(c.x.mean() - 1e3) < 1 and 0.8 < c.x.std() < 1.2 for c in far)
    for c in C.std_cases().values():
        if c.N > 1:
            _, a = C.std_bound(c.x, C.standardize_ld(c.x))
            assert (a > 500) == c.name.startswith("far")


# ---------------------------------------------------------------------------------------------
# restatements with one mistake each
# ---------------------------------------------------------------------------------------------
def _np(t):
    return t.numpy()


def _bad_budget(cut_stays_done=False, counts_at_budget=False, int32_offsets=False):
    def traj_budget(lens, dones, budget):
        lens, dones, steps = _np(lens), _np(dones), int(budget)
        n = len(lens)
        lo, do = np.zeros(n, np.int32), np.zeros(n, np.int32)
        run, m = 0, 0
        for i in range(n):
            if run > steps if counts_at_budget else run >= steps:
                break
            L = max(int(lens[i]), 0)
            keep = min(L, steps - run)
            lo[i] = keep
            do[i] = bool(dones[i]) and (cut_stays_done or keep == L)
            run += keep
            m += 1
        if int32_offsets:
            with np.errstate(over="ignore"):
                off = np.concatenate([[0], np.cumsum(lo, dtype=np.int32)]).astype(np.int64)
        else:
            off = np.concatenate([[0], np.cumsum(lo, dtype=np.int64)])
        return (torch.as_tensor(lo), torch.as_tensor(do), torch.as_tensor(off),
                torch.as_tensor(np.array([m, run], dtype=np.int64)))
    return traj_budget


GL_ASSOC_DIFF = {}


def _chunked_gae(boot_done=False, boot_last=False, vn_reset=False, assoc=False):
    """gae_kernel's recurrences, one lane's work in its order (chunks of 64 steps, last first)."""
    def gae(rewards, values, lens, dones, offsets, n_out, gamma, lambd, states_rec, actions_rec):
        R, V, lens, dones = _np(rewards), _np(values), _np(lens), _np(dones)
        S, A = _np(states_rec), _np(actions_rec)
        gamma, lambd = np.float64(gamma), np.float64(lambd)
        gl = gamma * lambd
        tg, ad = np.zeros(int(n_out)), np.zeros(int(n_out))
        st = np.zeros((int(n_out), S.shape[2]))
        ac = np.zeros((int(n_out), A.shape[2]))
        off = _np(offsets)
        with np.errstate(invalid="ignore"):
            for i in range(len(lens)):
                L, o = int(lens[i]), int(off[i])
                if L == 0:
                    continue
                r = R[i, :L].astype(np.float64)
                if boot_last:
                    boot = np.float64(0.0) if dones[i] else V[i, L - 1]
                else:
                    boot = np.float64(0.0) if dones[i] and not boot_done else V[i, L]
                c, a, vn = boot, np.float64(0.0), boot
                for t in reversed(range(L)):
                    if vn_reset and t % 64 == 63:
                        vn = boot
                    c = r[t] + gamma * c
                    a = ((r[t] + gamma * vn) - V[i, t]) + (gamma * (lambd * a) if assoc else gl * a)
                    vn = V[i, t]
                    tg[o + t], ad[o + t] = c, a
                st[o:o + L] = S[i, :L]
                ac[o:o + L] = A[i, :L]
        return tuple(torch.as_tensor(x) for x in (tg, ad, st, ac))
    return gae


def _bad_standardize(sample_std=False, drop_last_block=False):
    def standardize(x, out=None):
        xn = _np(x).copy()
        N = len(xn)
        with np.errstate(all="ignore"):
            nb = -(-N // C.STD_BLOCK)
            head = xn[:(nb - 1) * C.STD_BLOCK] if drop_last_block and nb > 1 else xn
            mean = head.sum() / N
            d = xn - mean
            z = d / np.sqrt((d * d).sum() / (N - 1 if sample_std else N))
        z = torch.as_tensor(z)
        return z if out is None else out.copy_(z)
    return standardize


def _with(**fns):
    ns = types.SimpleNamespace(**{k: getattr(cpu_ops, k) for k in dir(cpu_ops)
                                  if not k.startswith("_")})
    for k, f in fns.items():
        setattr(ns, k, f)
    return ns


@pytest.mark.parametrize("name", list(C.gae_cases()))
def test_kernel_order_gae_is_the_restatement(name):
    """The chunked loop without a mistake gives gae_batch's bits: the controls differ from it by
    their one mistake only."""
    C.run_gae(_with(gae=_chunked_gae()), DEV, C.gae_cases()[name])


CONTROLS = {
    "done_trajectory_bootstrapped": ("gae", dict(gae=_chunked_gae(boot_done=True))),
    "boot_from_values_len_minus_1": ("gae", dict(gae=_chunked_gae(boot_last=True))),
    "vn_reset_at_a_chunk_edge": ("gae", dict(gae=_chunked_gae(vn_reset=True))),
    "gamma_times_lambda_A": ("gae", dict(gae=_chunked_gae(assoc=True))),
    "cut_trajectory_stays_done": ("budget", dict(traj_budget=_bad_budget(cut_stays_done=True))),
    "trajectory_at_the_budget_counted": ("budget",
                                         dict(traj_budget=_bad_budget(counts_at_budget=True))),
    "int32_offsets": ("budget", dict(traj_budget=_bad_budget(int32_offsets=True))),
    "sample_std": ("standardize", dict(standardize=_bad_standardize(sample_std=True))),
    "last_block_left_out_of_the_mean": ("standardize",
                                        dict(standardize=_bad_standardize(drop_last_block=True))),
}
CONTROL_FAILURES = {}


def _family(ops, family):
    cases, run = {"gae": (C.gae_cases(), C.run_gae), "budget": (C.budget_cases(), C.run_budget),
                  "standardize": (C.std_cases(), C.run_standardize)}[family]
    return {k: (lambda c=c: run(ops, DEV, c)) for k, c in cases.items()}


@pytest.mark.parametrize("control", list(CONTROLS))
def test_negative_control_is_caught(control):
    family, fns = CONTROLS[control]
    saved = dict(C.RATIOS)
    failed = []
    try:
        runs = _family(_with(**fns), family)
        for k, run in runs.items():
            try:
                run()
            except AssertionError:
                failed.append(k)
    finally:
        C.RATIOS.clear()
        C.RATIOS.update(saved)
    CONTROL_FAILURES[control] = (len(failed), len(runs))
    print(f"{control}: {len(failed)} of {len(runs)} {family} cases fail")
    assert failed, f"{control}: no case of the {family} family noticed it"
    if control == "vn_reset_at_a_chunk_edge":   # only a trajectory of more than 64 steps shows it
        assert all(C.gae_cases()[k].lens.max() > 64 for k in failed)
    if control == "int32_offsets":
        assert failed == [C.BUDGET_BIG]
    if control == "last_block_left_out_of_the_mean":
        assert all(C.std_cases()[k].N > C.STD_BLOCK for k in failed)


def test_gamma_lambda_association_differs_in_bits():
    """gamma (lambd A) and (gamma lambd) A are different f64 values somewhere in the cases: the
    bit-equality check tells the two associations apart (the reference computes gamma * lambd
    first, trpo.py:197-198)."""
    differ = 0
    for c in C.gae_cases().values():
        if c.n_out == 0:
            continue
        args = (torch.as_tensor(c.R), torch.as_tensor(c.V), torch.as_tensor(c.lens),
                torch.as_tensor(c.dones.astype(np.int32)), torch.as_tensor(c.off), c.n_out,
                c.gamma, c.lambd, torch.as_tensor(c.S), torch.as_tensor(c.A))
        a, b = _chunked_gae()(*args)[1].numpy(), _chunked_gae(assoc=True)(*args)[1].numpy()
        differ += int(np.sum(a.view(np.int64) != b.view(np.int64)))
    print(f"advantages that differ in bits between the two associations: {differ}")
    assert differ >= 1
