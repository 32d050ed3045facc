"""Cases for the cut kernel (mepol_traj_cut, csrc/trpo_batch.hip: every trajectory of an
un-terminated rollout cut at its first done step), shared by test_traj_cut_host.py (CPU: the
table reaches what it claims) and test_gpu_traj_cut.py.  cut_reference is a numpy restatement of
the header's semantics and the only source of expected values; test_gpu_cut_sampler.py applies it
to the rollout kernels' own records.

A case is (n, T, a_dim) with nf = 2.  Its rows cycle through KINDS, the patterns of done_step that
matter to a kernel whose 256 threads scan t = tid, tid + 256, ...: a hit on the first or the last
step, none, all, two hits (the first wins), a single hit on either side of the thread-stride seam
(t = 255, 256, 257) and a late hit found by a LOWER thread than an early one ("wrap": t = 256 is
thread 0's second step, t = 1 thread 1's first).  Set bytes cycle through BYTES (any non-zero
value is done).  Kept rewards carry a NaN with a payload and a -0.0; everything behind an
episode's end is filled with 0xffffffff words in all three buffers, so only zeros that the kernel
wrote pass."""
import functools
import itertools
import types

import numpy as np

T_VALUES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
N_VALUES = (1, 3, 257)
A_VALUES = (1, 2, 8)
NF = 2
THREADS = 256                         # kCutThreads
BYTES = (1, 0x80, 0xFF, 2)
NAN_PAYLOAD = np.uint32(0x7FC12345)   # a quiet NaN whose payload must survive
NEG_ZERO = np.uint32(0x80000000)
FILL = np.uint32(0xFFFFFFFF)          # behind the end: a NaN no kernel would write
KINDS = ("t0", "last", "none", "all", "two", "seam255", "seam256", "seam257", "wrap", "random")


def cut_reference(done_step, rewards, states, actions):
    """(rewards, states, actions, len int32 [n], done int32 [n]) after the cut: with f the first t
    whose done_step[i, t] is non-zero, len = f + 1 and done = 1, else len = T and done = 0;
    rewards[i, len:], actions[i, len:] and states[i, len + 1:] are +0.0 and every other word is
    the input's, bit for bit (the copies are made on uint32 views)."""
    done_step = np.asarray(done_step)
    n, T = done_step.shape
    R, S, A = (np.array(x, dtype=np.float32, copy=True) for x in (rewards, states, actions))
    assert R.shape == (n, T) and S.shape[:2] == (n, T + 1) and A.shape[:2] == (n, T)
    lens, dones = np.empty(n, np.int32), np.empty(n, np.int32)
    for i in range(n):
        hits = np.flatnonzero(done_step[i].view(np.uint8) if done_step.dtype == bool
                              else done_step[i])
        L = int(hits[0]) + 1 if len(hits) else T
        lens[i], dones[i] = L, 1 if len(hits) else 0
        R[i, L:] = 0.0
        A[i, L:] = 0.0
        S[i, L + 1:] = 0.0
    return R, S, A, lens, dones


def kind_hits(kind, T, rng):
    """The hit steps of a row of this kind, or None where T has no room for it."""
    if kind == "t0":
        return [0]
    if kind == "last":
        return [T - 1]
    if kind == "none":
        return []
    if kind == "all":
        return list(range(T))
    if kind == "two":
        return [T // 3, T - 1] if T >= 2 else None
    if kind.startswith("seam"):
        t = int(kind[4:])
        return [t] if t < T else None
    if kind == "wrap":
        return [1, THREADS] if T > THREADS else None
    return sorted(set(rng.integers(0, T, max(1, T // 50)).tolist()))


def _words(rng, shape):
    """Random finite f32 values (as float32)."""
    return rng.standard_normal(shape).astype(np.float32)


def make_case(n, T, a_dim, index):
    rng = np.random.default_rng(4000 + index)
    done = np.zeros((n, T), dtype=np.uint8)
    kinds = []
    for i in range(n):
        k = (i + index) % len(KINDS)          # rotate, so that n = 1 cases differ
        hits = kind_hits(KINDS[k], T, rng)
        if hits is None:
            k, hits = KINDS.index("random"), kind_hits("random", T, rng)
        kinds.append(KINDS[k])
        for j, t in enumerate(hits):
            done[i, t] = BYTES[(i + j + index) % len(BYTES)]
    R, S, A = _words(rng, (n, T)), _words(rng, (n, T + 1, NF)), _words(rng, (n, T, a_dim))
    _, _, _, lens, dones = cut_reference(done, R, S, A)
    Ru, Su, Au = R.view(np.uint32), S.view(np.uint32), A.view(np.uint32)
    for i in range(n):
        L = int(lens[i])
        if (i + index) % 2 == 0:
            Ru[i, 0] = NAN_PAYLOAD
            if L >= 2:
                Ru[i, L - 1] = NEG_ZERO
        else:
            Ru[i, L - 1] = NEG_ZERO
        Ru[i, L:] = FILL
        Au[i, L:] = FILL
        Su[i, L + 1:] = FILL
    for x in (done, R, S, A, lens, dones):
        x.setflags(write=False)
    return types.SimpleNamespace(name=f"n{n}_T{T}_a{a_dim}", n=n, T=T, a_dim=a_dim, done=done,
                                 R=R, S=S, A=A, lens=lens, dones=dones, kinds=tuple(kinds))


def case_keys():
    return [(n, T, a) for T, n, a in itertools.product(T_VALUES, N_VALUES, A_VALUES)]


@functools.lru_cache(maxsize=None)
def case(n, T, a_dim):
    return make_case(n, T, a_dim, case_keys().index((n, T, a_dim)))


def case_ids():
    return [f"n{n}_T{T}_a{a}" for n, T, a in case_keys()]


def bits(x):
    """The array's 32-bit words: NaN payloads and signed zeros count in a comparison."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x
