"""Cases for the threshold goals of the one-launch rollouts (mepol_rollout_goal_threshold,
mepol_rollout_deep_goal_threshold: state[coord] >= threshold on MountainCar and GridWorld), shared
by test_threshold_goal_cases_host.py (CPU: the cases are what they claim) and
test_gpu_threshold_goal.py.  Everything is built from rollout_cases.make_case / case_policy and is
as small as there: 3 or 4 trajectories of T = 12 steps.

MountainCar "climb": four trajectories that start with the velocity clamp's value and are pushed
uphill by a saturated force (noise +BIG on every step, as env_edges_cases does), from positions
chosen so that the hilltop (position >= 0.45, reached only through the wall's clip) is crossed at
step 1, at step 5, at step 12 = T, and never.  So all four kinds of episode occur: len 1, a
mid-episode hit, a hit on step T, T without a hit."""
import numpy as np

import rollout_cases as R

HILLTOP = (0, 0.45)                  # (coord, threshold) of goal_rl's MountainCarGoal
CLIMB_P0 = (0.40, 0.15, -0.30, -0.50)
CLIMB_V0 = 0.07
CLIMB_LENS = (1, 5, R.T, R.T)        # the episodes' lengths ...
CLIMB_DONE = (True, True, True, False)  # ... and whether they end at the hilltop
# Within every episode the pre-clip position p + v' stays this far from 0.45 on either side (the
# closest are 0.40 + 0.07 at trajectory 0's only step and trajectory 2 one step before it crosses,
# 0.0193 below): seven orders of magnitude above anything cos() could move.
CLIMB_GAP = 0.019
KINDS = {"len1", "mid_done", "T_done", "T_not_done"}

TWO_LAYER = ((5, 65), (64, 48))      # rollout_cases.goal_cases()'s shapes
WIDE = (300, 300)                    # the CLI's shape, once
DEEP = ((70, 9, 66), (64, 130, 6, 33, 10, 65))  # test_gpu_rollout_deep_goal.py's edge shapes


def climb_case(hidden):
    init = np.array([[p, CLIMB_V0] for p in CLIMB_P0], dtype=np.float64)
    noise = np.full((R.T, len(CLIMB_P0), 1), R.BIG)
    return R.make_case("climb-" + "x".join(map(str, hidden)), "mountaincar", hidden,
                       n=len(CLIMB_P0), init=init, noise=noise)


def mc_case(hidden):
    """A MountainCar case with rollout_cases' spread starts and random noise, for the thresholds
    taken from a rollout's own values."""
    return R.make_case("thr-mc-" + "x".join(map(str, hidden)), "mountaincar", hidden, seed=97)


def gw_case(hidden):
    """rollout_cases.goal_cases()'s starts (the same seed), for any hidden shape."""
    return R.make_case("thr-gw-" + "x".join(map(str, hidden)), "gridworld", hidden, seed=95)


def first_hit(V, coord, threshold):
    """(len int32 [n], done bool [n]) of the episodes inside an un-terminated rollout whose states
    AFTER each step are V [n, T, 2] (f64, or f32: it widens exactly): an episode ends with the
    first step t at which V[:, t, coord] >= threshold in f64 (len = t + 1, done), or after T
    steps.  A NaN state is no hit."""
    V = np.asarray(V)
    with np.errstate(invalid="ignore"):
        hit = V[:, :, coord].astype(np.float64) >= np.float64(threshold)
    done = hit.any(axis=1)
    lens = np.where(done, hit.argmax(axis=1) + 1, V.shape[1]).astype(np.int32)
    return lens, done


def kinds(lens, dones, T):
    out = set()
    for L, d in zip(np.asarray(lens).tolist(), np.asarray(dones).tolist()):
        out.add("len1" if L == 1 else "mid_done" if 1 < L < T and d else
                "T_done" if L == T and d else "T_not_done" if L == T else "other")
    return out


def climb_f64(hidden):
    """The climb case rolled out on the host in f64 (rollout_cases.f64_rollout): states after each
    step [n, T, 2] and, per step and trajectory, the pre-clip position p + v' [T, n] and the
    margin of every comparison of the env step (rollout_cases.mc_margins)."""
    case = climb_case(hidden)
    S, A = R.f64_rollout(case)                      # [T+1, n, 2], [T, n]
    pre = np.empty((case["T"], case["n"]))
    margin = np.empty((case["T"], case["n"]))
    for t in range(case["T"]):
        p, v = S[t][:, 0], S[t][:, 1]
        force = np.minimum(np.maximum(A[t], -1.0), 1.0)
        v1 = np.minimum(np.maximum(v + (force * 0.0015 - 0.0025 * np.cos(3 * p)), -0.07), 0.07)
        pre[t] = p + v1
        margin[t], _ = R.mc_margins(S[t], A[t])
    return np.transpose(S[1:], (1, 0, 2)).copy(), pre, margin, A
