"""Sequential numpy restatements of TRPO's sampling and batch processing, shared by
test_goal_rl_host.py (CPU) and test_gpu_goal_rl.py (the HIP kernels): the goal test, truncation
of an un-terminated rollout at its first hit, the step budget, GAE in f64 and the standardisation
in extended precision.  Independent of mepol_amd.algorithms.trpo (it must not import it).

The second half holds the case families of the batch kernels (traj_budget, gae, standardize) with
their runners; expected values come from the restatements of the first half alone."""
import functools
import types

import numpy as np

from entropy_cases import RATIOS, U0, _n, _t, bits_equal, check, ld  # noqa: F401

GAMMA, LAMBD = 0.995, 0.98


def goal_hit(s, goal, radius=0.1):
    """np.linalg.norm(s - goal) <= radius for f32 states [..., 2] and an f32 goal, the norm in
    f32 and the comparison in f64 (the reference's numpy 1.x; numpy >= 2 compares in f32)."""
    s = np.asarray(s, dtype=np.float32)
    goal = np.asarray(goal, dtype=np.float32)
    nrm = np.linalg.norm(s - goal, axis=-1)
    assert nrm.dtype == np.float32
    return np.float64(nrm) <= radius


def first_hit(S, goal, radius=0.1):
    """(len int32 [n], done bool [n]) of the episodes inside an un-terminated rollout S
    [n, T+1, 2]: an episode ends with the first step t whose next state S[:, t+1] hits the goal
    (len = t + 1, done), or after T steps."""
    n, T1, _ = S.shape
    hit = goal_hit(S[:, 1:], goal, radius)
    done = hit.any(axis=1)
    lens = np.where(done, hit.argmax(axis=1) + 1, T1 - 1).astype(np.int32)
    return lens, done


def truncate(S, A, lens, dones):
    """The records of episodes of these lengths: states up to row len, actions up to row
    len - 1, zeros behind; rewards 1 at len - 1 of done episodes, zero elsewhere."""
    n, T, _ = A.shape
    St, At = np.zeros_like(S), np.zeros_like(A)
    R = np.zeros((n, T), dtype=np.float32)
    for i in range(n):
        L = int(lens[i])
        St[i, :L + 1] = S[i, :L + 1]
        At[i, :L] = A[i, :L]
        if dones[i]:
            R[i, L - 1] = 1
    return St, At, R


def budget(lens, dones, steps):
    """The reference's `steps == batch_size` rule over a batch rolled out in parallel:
    trajectories in index order while the running sum is below `steps`, the last one cut; a cut
    trajectory is not done.  A negative length counts as 0, as the kernel's max(len, 0) does; any
    non-zero `done` is done.  Returns (len_out [n], done_out [n], offsets [n+1], (m, kept))."""
    n = len(lens)
    len_out, done_out = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    run, m = 0, 0
    for i in range(n):
        if run >= steps:
            break
        L = max(int(lens[i]), 0)
        keep = min(L, steps - run)
        len_out[i] = keep
        done_out[i] = bool(dones[i]) and keep == L
        run += keep
        m += 1
    offsets = np.concatenate([[0], np.cumsum(len_out, dtype=np.int64)]).astype(np.int64)
    return len_out, done_out, offsets, (m, run)


def gae_traj(rewards, values, boot, gamma=GAMMA, lambd=LAMBD):
    """process_traj in f64, one operation at a time in the reference's order; rewards f32."""
    n = len(rewards)
    r = np.asarray(rewards, dtype=np.float32).astype(np.float64)
    v = np.asarray(values, dtype=np.float64)
    gamma, lambd, boot = np.float64(gamma), np.float64(lambd), np.float64(boot)
    targets, adv = np.zeros(n), np.zeros(n)
    c = boot
    for t in reversed(range(n)):
        c = r[t] + gamma * c
        targets[t] = c
    gl = gamma * lambd
    a = np.float64(0.0)
    for t in reversed(range(n)):
        vn = boot if t == n - 1 else v[t + 1]
        a = ((r[t] + gamma * vn) - v[t]) + gl * a
        adv[t] = a
    return targets, adv


def gae_batch(rewards, values, lens, dones, states, actions, gamma=GAMMA, lambd=LAMBD):
    """(targets [N], adv [N], states [N, nf] f64, actions [N, a] f64) packed in trajectory order;
    a trajectory that is not done bootstraps from values[i, len]."""
    out = []
    for i in range(len(lens)):
        L = int(lens[i])
        if L == 0:
            continue
        boot = 0.0 if dones[i] else values[i, L]
        t, a = gae_traj(rewards[i, :L], values[i, :L], boot, gamma, lambd)
        out.append((t, a, states[i, :L].astype(np.float64), actions[i, :L].astype(np.float64)))
    return tuple(np.concatenate(x) for x in zip(*out))


def standardize_ld(x):
    """(x - mean) / population std in np.longdouble, returned as longdouble."""
    x = np.asarray(x, dtype=np.longdouble)
    mean = x.sum() / len(x)
    d = x - mean
    return d / np.sqrt((d * d).sum() / len(x))


def scripted_parallel(ep_lens, traj_len):
    """(len, done) of a parallel batch whose episodes have these scripted lengths."""
    ep = np.asarray(ep_lens, dtype=np.int64)
    return np.minimum(ep, traj_len).astype(np.int32), ep <= traj_len


# =============================================================================================
# Case families for the batch kernels of csrc/trpo_batch.hip, run through an `ops`-shaped module
# (tests/cpu_ops.py on the CPU, mepol_amd.ops on the GPU) by test_goal_rl_cases_host.py and
# test_gpu_trpo_ops.py.  Expected values come from the restatements above alone.
# =============================================================================================
# ---- traj_budget -----------------------------------------------------------------------------
BUDGET_N = (1, 2, 255, 256, 257, 511, 513, 65536)   # 256 threads: chunk 1 up to 256, 2 from 257
BUDGET_BIG = "all40000_n65536"
DONE_VALUES = (0, 1, 2, -1)                          # any non-zero value is done


def budget_chunk(n):
    """Trajectories per thread of traj_budget_kernel."""
    return (n + 255) // 256


def budget_case(name, n, seed, big=False):
    """lens in [0, 40) with a leading 0, zeros between used trajectories and one negative length
    (n >= 8); done in {0, 1, 2, -1}.  Budgets: 0, 1, every exact prefix sum of the first three
    trajectories with -1 and +1 (a trajectory that would start exactly at the budget is unused),
    total - 1, total, total + 7 and one above 2^31.  big: all lengths 40,000 (the step total
    passes 2^31: only int64 offsets hold it)."""
    rng = np.random.default_rng(seed)
    if big:
        lens = np.full(n, 40000, dtype=np.int32)
    else:
        lens = rng.integers(1, 40, n).astype(np.int32)
        lens[0] = 0 if n > 1 else 5
        if n >= 8:
            lens[3], lens[n // 2], lens[n - 2], lens[5] = 0, 0, 0, -3
    dones = rng.choice(np.array(DONE_VALUES, dtype=np.int32), n)
    if n >= 8:
        dones[1:5] = (2, -1, 1, 0)  # trajectory 3 has length 0 and is done
    pos = np.maximum(lens.astype(np.int64), 0)
    total = int(pos.sum())
    prefix = [int(v) for v in np.cumsum(pos[:3])]
    budgets = {0, 1, total - 1, total, total + 7, 2 ** 31 + 12345}
    for p in prefix:
        budgets |= {p - 1, p, p + 1}
    if big:
        budgets |= {2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 40000 * 53688}
    return types.SimpleNamespace(name=name, n=n, lens=lens, dones=dones, total=total,
                                 budgets=tuple(sorted(b for b in budgets if b >= 0)))


@functools.lru_cache(maxsize=None)
def budget_cases():
    out = [budget_case(f"n{n}", n, 300 + n) for n in BUDGET_N]
    out.append(budget_case(BUDGET_BIG, 65536, 399, big=True))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def budget_reference(name):
    c = budget_cases()[name]
    return {b: budget(c.lens, c.dones, b) for b in c.budgets}


def run_budget(ops, dev, c):
    """Every budget of the case, every output word exactly the restatement's: len_out [n],
    done_out [n] (0 or 1), offsets [n + 1] int64 and meta [2]."""
    ref = budget_reference(c.name)
    dl, dd = _t(c.lens, dev), _t(c.dones, dev)
    for b in c.budgets:
        lo, do, off, (m, kept) = ref[b]
        assert kept == min(b, c.total) and off[-1] == kept
        got = ops.traj_budget(dl, dd, b)
        g_lo, g_do, g_off, g_meta = (_n(x) for x in got)
        assert g_off.dtype == np.int64 and g_meta.dtype == np.int64, (c.name, b)
        assert g_lo.shape == (c.n,) and g_do.shape == (c.n,) and g_off.shape == (c.n + 1,)
        assert np.array_equal(g_lo, lo), (c.name, b, "len_out")
        assert np.array_equal(g_do, do.astype(np.int32)), (c.name, b, "done_out")
        assert np.array_equal(g_off, off), (c.name, b, "offsets")
        assert g_meta.tolist() == [m, kept], (c.name, b, "meta", g_meta.tolist(), [m, kept])
        again = ops.traj_budget(dl, dd, b)
        assert all(bits_equal(x, y) for x, y in zip(got, again))


# ---- gae -------------------------------------------------------------------------------------
GAE_N = (1, 15, 16, 17, 33)
GAE_T = (1, 63, 64, 65, 129)
GAE_DIMS = ((1, 1), (2, 1), (2, 2), (3, 5), (29, 8))     # (num_features, a_dim)
GAE_GL = ((0.995, 0.98), (1.0, 1.0), (0.995, 0.0), (0.0, 0.98))
GAE_TRAJ, GAE_CHUNK = 16, 64                             # kGaeTraj, kGaeChunk


def gae_chunks(lens):
    """Per workgroup of 16 trajectories: (staging chunks of the longest, True if a trajectory with
    steps ends inside an earlier chunk than the longest, trajectories in the workgroup)."""
    out = []
    for g in range(0, len(lens), GAE_TRAJ):
        grp = [int(v) for v in lens[g:g + GAE_TRAJ]]
        mx = max(grp)
        if mx == 0:
            out.append((0, False, len(grp)))
            continue
        last = (mx - 1) // GAE_CHUNK
        out.append((last + 1, any(0 < v and (v - 1) // GAE_CHUNK < last for v in grp), len(grp)))
    return out


def gae_case(name, n, T, nf, a, gamma, lambd, seed, lens=None):
    """Lengths cycle through 1, T, 0, 63, 64, 65 (those that T allows) and random ones, so the
    first workgroup mixes a length-1 with a length-T trajectory; done for about half, among them
    one of length T.  Rewards are random f32 (their widenings have 24 significant bits, not a
    short decimal).  Everything behind a trajectory's len is NaN: rewards[i, len:], values[i,
    len + 1:] and values[i, len] too when it is done, states_rec[i, len:] (row len is the state
    after the last step: not packed), actions_rec[i, len:].  No NaN may reach an output; values[i,
    len] of a trajectory that is not done must (the restatement bootstraps from it)."""
    rng = np.random.default_rng(seed)
    lens_in = lens
    want = [v for v in (1, T, 0, 63, 64, 65, T, 1) if v <= T]
    lens = rng.integers(1, T + 1, n).astype(np.int32)
    lens[:min(n, len(want))] = want[:n]
    if lens_in is not None:
        lens = np.asarray(lens_in, dtype=np.int32)
    dones = rng.random(n) < 0.5
    if n >= 2:
        dones[0], dones[1] = False, True
    R = rng.standard_normal((n, T)).astype(np.float32)
    V = rng.standard_normal((n, T + 1))
    S = rng.standard_normal((n, T + 1, nf)).astype(np.float32)
    A = rng.standard_normal((n, T, a)).astype(np.float32)
    for i in range(n):
        L = int(lens[i])
        R[i, L:] = np.nan
        V[i, L + 1:] = np.nan
        if dones[i]:
            V[i, L] = np.nan
        S[i, L:] = np.nan
        A[i, L:] = np.nan
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    return types.SimpleNamespace(name=name, n=n, T=T, nf=nf, a=a, gamma=gamma, lambd=lambd,
                                 lens=lens, dones=dones, R=R, V=V, S=S, A=A, off=off,
                                 n_out=int(off[-1]))


@functools.lru_cache(maxsize=None)
def gae_cases():
    out, i = [], 0
    for n in GAE_N:
        for T in GAE_T:
            nf, a = GAE_DIMS[(i + i // len(GAE_T)) % len(GAE_DIMS)]  # every pair with every n
            g, lam = GAE_GL[i % len(GAE_GL)]
            out.append(gae_case(f"n{n}_T{T}_f{nf}_a{a}_g{g}_l{lam}", n, T, nf, a, g, lam, 500 + i))
            i += 1
    # all-zero lengths: nothing is written, n_out = 0
    out.append(gae_case("all_zero", 17, 5, 2, 2, 0.995, 0.98, 599, lens=np.zeros(17, np.int32)))
    return {c.name: c for c in out}


def gae_case_with_lens(c, lens):
    """The case with other lengths (and their offsets); the NaN fill of the longer case stays."""
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    d = dict(vars(c))
    d.update(lens=lens.astype(np.int32), off=off, n_out=int(off[-1]))
    return types.SimpleNamespace(**d)


@functools.lru_cache(maxsize=None)
def gae_reference(name):
    c = gae_cases()[name]
    if c.n_out == 0:
        return (np.zeros(0), np.zeros(0), np.zeros((0, c.nf)), np.zeros((0, c.a)))
    ref = gae_batch(c.R, c.V, c.lens, c.dones, c.S, c.A, c.gamma, c.lambd)
    assert all(np.isfinite(x).all() for x in ref), name  # the restatement reads nothing behind len
    return ref


def run_gae(ops, dev, c, ref=None):
    """Targets, advantages and the packed states / actions bit-equal to the restatement's."""
    ref = ref if ref is not None else gae_reference(c.name)
    args = (_t(c.R, dev), _t(c.V, dev), _t(c.lens, dev), _t(c.dones.astype(np.int32), dev),
            _t(c.off, dev), c.n_out, c.gamma, c.lambd, _t(c.S, dev), _t(c.A, dev))
    got = ops.gae(*args)
    shapes = ((c.n_out,), (c.n_out,), (c.n_out, c.nf), (c.n_out, c.a))
    for key, g, e, shp in zip(("targets", "adv", "states", "actions"), got, ref, shapes):
        g = _n(g)
        assert g.shape == shp and g.dtype == np.float64, (c.name, key)
        assert not np.isnan(g).any(), (c.name, key, "a nan from behind len reached the output")
        assert np.array_equal(g.view(np.int64), np.ascontiguousarray(e).view(np.int64)), (
            c.name, key, int(np.sum(g != e)))
    again = ops.gae(*args)
    assert all(bits_equal(x, y) for x, y in zip(got, again))
    return got


# ---- standardize -----------------------------------------------------------------------------
STD_N = (1, 2, 255, 256, 257, 2047, 2048, 2049, 8192, 8193, 32769)
STD_BLOCK = 2048   # kStdPerBlock: 8192 -> 4 records (the group count), 8193 -> 5, 32769 -> 17


def std_case(name, N, seed, mean=0.3, std=2.0):
    rng = np.random.default_rng(seed)
    return types.SimpleNamespace(name=name, N=N, x=mean + std * rng.standard_normal(N))


@functools.lru_cache(maxsize=None)
def std_cases():
    out = [std_case(f"N{N}", N, 700 + i) for i, N in enumerate(STD_N)]
    out += [std_case(f"far_N{N}", N, 750 + i, mean=1e3, std=1.0)
            for i, N in enumerate((257, 8193, 32769))]
    return {c.name: c for c in out}


def std_bound(x, z):
    """|computed - exact| per element of z = (x - mean) / std for fixed-order f64 sums of N terms,
    u = 2^-53, a = sum|x| / (N std) from the data in longdouble:
      mean   a fixed-order sum errs by (N - 1) u sum|x|, the division by u |mean| <= u sum|x| / N,
             so |d mean| / std <= N u a;
      std    sum d_i = 0, so the mean's error enters the variance only in second order ((N u a)^2
             relative: below u for every input here, asserted); each (x_i - mean)^2 is off by
             3 u relatively, their fixed-order sum by (N - 1) u, the division and the root by u
             each and the root halves the rest: |d std| / std <= (N / 2 + 3) u;
      z_i    the subtraction and the division add 2 u |z_i|.
    Together |d z_i| <= N u a + (N / 2 + 5) u |z_i|.  The longdouble reference's own error is
    2^-11 of that."""
    N = len(x)
    xl = ld(x)
    mean = xl.sum() / N
    sd = np.sqrt(((xl - mean) ** 2).sum() / N)
    a = np.abs(xl).sum() / (N * sd)
    assert (N * U0 * a) ** 2 < U0, "the mean's error is not second order in the variance"
    return N * U0 * a + (ld(N) / 2 + 5) * U0 * np.abs(z), float(a)


def run_standardize(ops, dev, c):
    """Within std_bound of the longdouble reference; a second call and the in-place call
    (out = x) give the same bits; N = 1 and a constant vector are non-finite, as numpy's are."""
    dx = _t(c.x, dev)
    got = ops.standardize(dx)
    assert bits_equal(got, ops.standardize(dx)), "a second call gives other bits"
    xin = dx.clone()
    res = ops.standardize(xin, out=xin)
    assert res.data_ptr() == xin.data_ptr() and bits_equal(res, got), "in place differs"
    assert bits_equal(dx, _t(c.x, dev)), "the input was written"
    g = _n(got)
    const = _t(np.full(c.N, 1.5), dev)   # 1.5 N is exact, so the mean is: 0 / 0, as numpy
    assert not np.isfinite(_n(ops.standardize(const))).any()
    if c.N == 1:
        assert not np.isfinite(g).any()
        return got
    z = standardize_ld(c.x)
    bound, a = std_bound(c.x, z)
    assert a <= 16 or c.name.startswith("far"), c.name
    check("std_z", g, z, bound)
    return got


def run_all(ops, dev):
    for c in budget_cases().values():
        run_budget(ops, dev, c)
    for c in gae_cases().values():
        run_gae(ops, dev, c)
    for c in std_cases().values():
        run_standardize(ops, dev, c)
