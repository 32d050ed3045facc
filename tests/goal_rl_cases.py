"""Sequential numpy restatements of TRPO's sampling and batch processing, shared by
test_goal_rl_host.py (CPU) and test_gpu_goal_rl.py (the HIP kernels): the goal test, truncation
of an un-terminated rollout at its first hit, the step budget, GAE in f64 and the standardisation
in extended precision.  Independent of mepol_amd.algorithms.trpo (it must not import it)."""
import numpy as np

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
    trajectory is not done.  Returns (len_out [n], done_out [n], offsets [n+1], (m, kept))."""
    n = len(lens)
    len_out, done_out = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    run, m = 0, 0
    for i in range(n):
        if run >= steps:
            break
        keep = min(int(lens[i]), steps - run)
        len_out[i] = keep
        done_out[i] = bool(dones[i]) and keep == int(lens[i])
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
