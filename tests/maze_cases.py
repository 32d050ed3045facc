"""Cases for the box maze (mepol_amd/envs/maze.py, the kernels' env 2), shared by
test_maze_cases_host.py (CPU: the cases are what they claim) and test_gpu_maze.py.

Three mazes: the default GridWorld as a maze, four rooms, and a 16-wall maze with unequal bounds
and its own max_delta (a swapped coordinate, a wall that is never tested or a constant left in the
kernel shows there).  Per maze:
  edge_steps     single steps that land exactly on every side and corner of every wall and on every
                 bound (blocked), one f64 ulp outside / inside (free unless another wall is there),
                 inside the last wall alone, and with +-inf, NaN and +-max_delta actions;
  rollout_cases  n = 3 trajectories of T = 8 steps whose noise is scripted: trajectory j starts
                 0.1 beside its target (a wall or a bound), is pushed into it on even steps (noise
                 +-BIG saturates the clip whatever the policy's mean) and drifts on odd ones.  The
                 targets run over every wall and the four bounds; the host test proves the
                 coverage with the numpy class.  Everything random comes from the seeds here.
The expectations of edge_steps come from `blockers`, a restatement of the geometry that shares no
code with the class."""
import functools

import numpy as np
import torch

import rollout_cases as R
from mepol_amd.envs import BoxMazeContinuous

N, T = 3, 8
BIG = 50.0
# of rollout_cases.SHAPES: one part; three parts; h0 past the multi-workgroup form's LDS limit
TWO_LAYER = [(5, 65), (68, 192), (307, 64)]
DEEP = (70, 9, 66)
BIAS = np.array([0.015625, -0.03125])  # mean.bias of the exact-action policies
GOAL_T = 5


def sixteen():
    """16 disjoint walls on a 4 x 4 lattice inside x in (-3, 5), y in (-2, 7); max_delta 0.25."""
    walls = []
    for k in range(16):
        cx, cy = -2.0 + 2.0 * (k % 4), -0.75 + 2.25 * (k // 4)
        walls.append((cx - 0.3, cx + 0.3, cy - 0.25, cy + 0.25))
    return BoxMazeContinuous((-3.0, 5.0, -2.0, 7.0), walls, 0.25, ((-2.9, -1.9), (-2.5, -1.5)))


MAZES = {"gridworld": BoxMazeContinuous.gridworld, "four_rooms": BoxMazeContinuous.four_rooms,
         "sixteen": sixteen}
NAMES = tuple(MAZES)


@functools.lru_cache(maxsize=None)
def maze(name):
    return MAZES[name]()


# ---- geometry, restated ------------------------------------------------------------------------
def blockers(mz, px, py):
    """(indices of the walls whose closed box holds (px, py), names of the bounds it lies on or
    beyond)."""
    walls = [k for k, (x0, x1, y0, y1) in enumerate(mz.walls)
             if px >= x0 and px <= x1 and py >= y0 and py <= y1]
    xlo, xhi, ylo, yhi = mz.bounds
    bounds = [b for b, out in (("xlo", px <= xlo), ("xhi", px >= xhi), ("ylo", py <= ylo),
                               ("yhi", py >= yhi)) if out]
    return walls, bounds


def is_free(mz, px, py):
    walls, bounds = blockers(mz, px, py)
    return not walls and not bounds


def _approach(target, away):
    """An f32 start coordinate about 0.1 from `target` on the side `away` (+-1, or 0: any) and the
    f64 action that lands exactly on it: float(start) + action == target."""
    for off in (0.1, 0.125, 0.09375, 0.0625):
        for sign in ((away,) if away else (-1.0, 1.0)):
            x = np.float32(target + sign * off)
            dx = target - float(x)
            if float(x) + dx == target:
                return x, dx
    raise AssertionError(f"no exact approach to {target!r}")


def _step_to(px, py, away=(0.0, 0.0)):
    x, dx = _approach(px, away[0])
    y, dy = _approach(py, away[1])
    return (x, y), (dx, dy)


def _ulp(v, direction):
    return float(np.nextafter(v, np.inf if direction > 0 else -np.inf)) if direction else v


def _free_coordinate(mz, axis, at):
    """A coordinate c on the other axis where the point `at` on `axis` lies in no wall."""
    lo, hi = (mz.bounds[2:] if axis == 0 else mz.bounds[:2])
    for c in np.linspace(lo + 0.4, hi - 0.4, 41):
        p = (at, float(c)) if axis == 0 else (float(c), at)
        if not blockers(mz, *p)[0]:
            return float(c)
    raise AssertionError("no free coordinate")


@functools.lru_cache(maxsize=None)
def edge_steps(name):
    """dict(name [m], S f32 [m, 2], A f64 [m, 2], expect [m]): expect is "blocked" / "free" from
    `blockers` on the landing point, or "class" where only the numpy class says (NaN, inf)."""
    mz = maze(name)
    rows = []

    def add(label, p, away=(0.0, 0.0)):
        s, a = _step_to(*p, away)
        assert abs(a[0]) < mz.max_delta and abs(a[1]) < mz.max_delta  # no clip on the way
        rows.append((label, s, a, "free" if is_free(mz, *p) else "blocked"))

    for w, (x0, x1, y0, y1) in enumerate(mz.walls):
        xm, ym = (x0 + x1) / 2, (y0 + y1) / 2
        spots = {"side_x0": ((x0, ym), (-1, 0)), "side_x1": ((x1, ym), (1, 0)),
                 "side_y0": ((xm, y0), (0, -1)), "side_y1": ((xm, y1), (0, 1)),
                 "corner_00": ((x0, y0), (-1, -1)), "corner_10": ((x1, y0), (1, -1)),
                 "corner_01": ((x0, y1), (-1, 1)), "corner_11": ((x1, y1), (1, 1))}
        for label, (p, out) in spots.items():
            assert w in blockers(mz, *p)[0]
            add(f"wall{w}/{label}/on", p, out)
            add(f"wall{w}/{label}/ulp_out", (_ulp(p[0], out[0]), _ulp(p[1], out[1])), out)
    xlo, xhi, ylo, yhi = mz.bounds
    for label, axis, b, inward in (("xlo", 0, xlo, 1), ("xhi", 0, xhi, -1), ("ylo", 1, ylo, 1),
                                   ("yhi", 1, yhi, -1)):
        c = _free_coordinate(mz, axis, b)
        on = (float(b), c) if axis == 0 else (c, float(b))
        inside = (_ulp(float(b), inward), c) if axis == 0 else (c, _ulp(float(b), inward))
        away = (inward, 0) if axis == 0 else (0, inward)
        assert blockers(mz, *on) == ([], [label]) and is_free(mz, *inside)
        add(f"bound/{label}/on", on, away)
        add(f"bound/{label}/ulp_in", inside, away)
    last = len(mz.walls) - 1
    x0, x1, y0, y1 = mz.walls[last]
    centre = ((x0 + x1) / 2, (y0 + y1) / 2)
    assert blockers(mz, *centre) == ([last], [])
    add("last_wall_only", centre)
    # special actions from the middle of the start box (free, with room on every side)
    (ix0, iy0), (ix1, iy1) = mz.init_box
    s0 = (np.float32((ix0 + ix1) / 2), np.float32((iy0 + iy1) / 2))
    md, inf, nan = float(mz.max_delta), float("inf"), float("nan")
    for label, a in (("inf/+-", (inf, -inf)), ("inf/-+", (-inf, inf)), ("nan/x", (nan, 0.1)),
                     ("nan/y", (0.1, nan)), ("nan/xy", (nan, nan)), ("clip/at+-", (md, -md)),
                     ("clip/at-+", (-md, md)),
                     ("clip/past", (float(np.nextafter(md, inf)), -float(np.nextafter(md, inf))))):
        rows.append((label, s0, a, "class"))
    out = dict(name=np.array([r[0] for r in rows]),
               S=np.array([r[1] for r in rows], dtype=np.float32),
               A=np.array([r[2] for r in rows], dtype=np.float64),
               expect=np.array([r[3] for r in rows]))
    for v in out.values():
        v.setflags(write=False)
    return out


def class_steps(mz, S, A):
    """The numpy class stepped once from every row of S with the action of A: f32 [m, 2]."""
    out = []
    with np.errstate(invalid="ignore"):
        for s, a in zip(S, A):
            mz.state = np.array(s, dtype=np.float32)
            out.append(mz.step(a)[0])
    return np.array(out, dtype=np.float32)


# ---- rollout cases -----------------------------------------------------------------------------
def _target_start(mz, target):
    """(start f32 [2], push direction [2]) 0.1 beside a wall (an int) or a bound (a name)."""
    if isinstance(target, str):
        axis, b, inward = {"xlo": (0, mz.bounds[0], 1), "xhi": (0, mz.bounds[1], -1),
                           "ylo": (1, mz.bounds[2], 1), "yhi": (1, mz.bounds[3], -1)}[target]
        c = _free_coordinate(mz, axis, b + 0.1 * inward)
        p = (b + 0.1 * inward, c) if axis == 0 else (c, b + 0.1 * inward)
        push = (-inward, 0) if axis == 0 else (0, -inward)
        assert is_free(mz, *p)
        return np.array(p, dtype=np.float32), np.array(push, dtype=np.float64)
    x0, x1, y0, y1 = mz.walls[target]
    xm, ym = (x0 + x1) / 2, (y0 + y1) / 2
    for p, push in (((x0 - 0.1, ym), (1, 0)), ((x1 + 0.1, ym), (-1, 0)), ((xm, y0 - 0.1), (0, 1)),
                    ((xm, y1 + 0.1), (0, -1))):
        land = (p[0] + push[0] * mz.max_delta, p[1] + push[1] * mz.max_delta)
        if is_free(mz, *p) and blockers(mz, *land) == ([target], []):
            return np.array(p, dtype=np.float32), np.array(push, dtype=np.float64)
    raise AssertionError(f"wall {target} has no free side")


@functools.lru_cache(maxsize=None)
def rollout_cases(name, seed=0):
    """The maze's cases: dict(name, maze, hidden, deep, init f32 [N, 2], noise f64 [T, N, 2],
    targets).  Case c takes two-layer shape c mod 3."""
    mz = maze(name)
    targets = list(range(len(mz.walls))) + ["xlo", "xhi", "ylo", "yhi"]
    targets += targets[:(-len(targets)) % N]
    rng = np.random.default_rng(2000 + seed)
    cases = []
    for c in range(len(targets) // N):
        mine = targets[N * c:N * c + N]
        init = np.zeros((N, 2), dtype=np.float32)
        noise = np.zeros((T, N, 2))
        for j, tg in enumerate(mine):
            init[j], push = _target_start(mz, tg)
            tangent = push[::-1]
            for t in range(T):
                noise[t, j] = (BIG * push if t % 2 == 0 else
                               0.05 * rng.standard_normal() * tangent
                               + 0.01 * rng.standard_normal() * push)
        init.setflags(write=False)
        noise.setflags(write=False)
        cases.append(dict(name=f"{name}-{c}", maze=name, hidden=TWO_LAYER[c % len(TWO_LAYER)],
                          deep=DEEP, init=init, noise=noise, targets=tuple(mine), n=N, T=T,
                          a_dim=2))
    return cases


@functools.lru_cache(maxsize=None)
def class_rollout(name, c):
    """The numpy class under the exact-action policies (action = BIAS + noise, one rounded f64
    add): S f32 [N, T+1, 2], A f32 [N, T, 2], V f64 [N, T, 2] and per step the (walls, bounds)
    `blockers` finds at the landing point of the clipped action, with whether the class moved."""
    case = rollout_cases(name)[c]
    mz = maze(name)
    S = np.zeros((N, T + 1, 2), dtype=np.float32)
    A = np.zeros((N, T, 2), dtype=np.float32)
    events = []
    for j in range(N):
        mz.state = case["init"][j].copy()
        S[j, 0] = mz.state
        for t in range(T):
            a = BIAS + case["noise"][t, j]
            A[j, t] = a
            d = np.clip(a, -mz.max_delta, mz.max_delta)
            land = (float(S[j, t, 0]) + float(d[0]), float(S[j, t, 1]) + float(d[1]))
            S[j, t + 1] = mz.step(a)[0]
            moved = not np.array_equal(S[j, t + 1], S[j, t])
            events.append((j, t, *blockers(mz, *land), moved))
    out = (S, A, S[:, 1:].astype(np.float64), events)
    for x in out[:3]:
        x.setflags(write=False)
    return out


# ---- policies ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_policy(hidden):
    """Random hidden layers, mean.weight = 0, mean.bias = BIAS, log_std = 0: the f64 action is
    BIAS + noise whatever the state is."""
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(23)
    pol = GaussianPolicy(list(hidden), 2, 2, 0.0)
    with torch.no_grad():
        pol.mean.weight.zero_()
        pol.mean.bias.copy_(torch.as_tensor(BIAS))
        pol.log_std.zero_()
    return pol


def real_policy(hidden):
    return R.policy(tuple(hidden), 2, -1.5)


# ---- goals taken from a rollout's own records ---------------------------------------------------
def ball_goal(S):
    """(goal f32 [2], radius): trajectory 0's state at GOAL_T lies exactly on the ball's rim."""
    at = S[0, GOAL_T]
    goal = (at + R.GOAL_OFF).astype(np.float32)
    return goal, float(R.goal_distance(at, goal))


def ball_hits(S, goal, radius):
    """bool [n, T]: the host's goal test on the state after every step."""
    n, T1, _ = S.shape
    return np.array([[float(R.goal_distance(S[i, t + 1], goal)) <= radius for t in range(T1 - 1)]
                     for i in range(n)])


def threshold_hits(V, coord, threshold):
    return V[:, :, coord] >= threshold


def first_hit(hit):
    """(lens int32 [n], dones bool [n]) of episodes that end at their first hit, or after T."""
    n, Tn = hit.shape
    dones = hit.any(axis=1)
    lens = np.where(dones, hit.argmax(axis=1) + 1, Tn).astype(np.int32)
    return lens, dones
