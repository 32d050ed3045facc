"""ErgodicEnv: ignore the done signal (src/envs/wrappers.py:4-15).  CustomRewardEnv: a reward
and termination function of the caller's (:40-52), and two such functions: GridGoal, the GridWorld
goals of src/experiments/goal_rl.py:61-77, and ThresholdGoal, the coordinate thresholds of its
other goals (:91-107).  BatchReward is the protocol of rewards that TRPO's sampler can evaluate for
a whole round at once, with BoxGoal and AnyGoal (build extensions) as its shipped cases."""
import numpy as np
import torch


class _EnvWrapper:
    """What the wrappers share: attribute access, reset, seed and unwrapped go through to the
    wrapped env."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        if name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        e = self.env
        while isinstance(e, _EnvWrapper):
            e = e.env
        return e

    def reset(self):
        return self.env.reset()

    def seed(self, seed=None):
        return self.env.seed(seed)


class ErgodicEnv(_EnvWrapper):
    def step(self, a):
        s, r, _, i = self.env.step(a)
        return s, r, False, i


class CustomRewardEnv(_EnvWrapper):
    """Replaces the env's reward and done signal by get_reward(s, r, d, i) -> (reward, done).  It
    is no ErgodicEnv: its episodes end."""

    def __init__(self, env, get_reward):
        super().__init__(env)
        self.get_reward = get_reward

    def step(self, a):
        s, r, d, i = self.env.step(a)
        r, d = self.get_reward(s, r, d, i)
        return s, r, d, i


class GridGoal:
    """Sparse goal reward (goal_rl.py:61-77): (1, True) when the f32 state is within `radius` of
    the f32 goal, else (0, False).  The test is the rollout kernel's (mepol_rollout_goal): the
    norm in f32, each operation rounded on its own, compared with the radius in f64 -- what
    np.linalg.norm(s - goal) <= 1e-1 computes under the reference's numpy 1.x."""

    def __init__(self, goal_xy, radius=0.1):
        self.goal = np.asarray(goal_xy, dtype=np.float32).reshape(2)
        self.radius = float(radius)

    def hit(self, s):
        """The test for states [..., 2]; a bool array of shape [...]."""
        d = np.asarray(s, dtype=np.float32) - self.goal
        q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32)
        return np.sqrt(q).astype(np.float64) <= self.radius

    def batch(self, states):
        """hit() restated in torch for a BatchReward's members (AnyGoal): the f64 states cast to
        f32 (exact for GridWorld's), sub, mul, mul, add and sqrt as separate f32 ops, the result
        widened and compared with the f64 radius.  Returns (reward, done) as BatchReward.batch."""
        s = states.to(torch.float32)
        goal = torch.as_tensor(self.goal, device=s.device)
        dx = torch.sub(s[..., 0], goal[0])
        dy = torch.sub(s[..., 1], goal[1])
        q = torch.add(torch.mul(dx, dx), torch.mul(dy, dy))
        done = torch.sqrt(q).to(torch.float64) <= self.radius
        return done.to(torch.float32), done

    def __call__(self, s, r, d, i):
        return (1, True) if bool(self.hit(s)) else (0, False)


class ThresholdGoal:
    """Sparse goal reward "a state coordinate reaches a threshold", the shape of every
    non-GridWorld goal of goal_rl.py:91-107 (s[0] >= 7, s[2] >= 3, s[2] >= 1): (1, True) when
    s[index] >= threshold, else (0, False).  The comparison is in f64 on the env's own state
    (an f32 state widens exactly), as Python compares an array element with a float, and a NaN
    state is no hit: the rollout kernels' test (mepol_rollout_goal_threshold)."""

    def __init__(self, index, threshold):
        self.index = int(index)
        self.threshold = float(threshold)

    def hit(self, s):
        """The test for states [..., nf]; a bool array of shape [...]."""
        return np.asarray(s)[..., self.index].astype(np.float64) >= self.threshold

    def batch(self, states):
        """hit() restated in torch for a BatchReward's members (AnyGoal): an ordered f64 compare
        on the given f64 states.  Returns (reward, done) as BatchReward.batch."""
        done = states[..., self.index] >= self.threshold
        return done.to(torch.float32), done

    def __call__(self, s, r, d, i):
        return (1, True) if bool(self.hit(s)) else (0, False)


class BatchReward:
    """A reward and termination function of the REACHED STATE alone, defined once for whole
    batches.  A subclass writes

        batch(states) -> (reward, done)

    for an f64 tensor states [n, T, nf] on any device, the env's OWN state after each step
    (MountainCar's f64 (p, v), GridWorld's f32 (x, y) widened exactly); reward is a float tensor
    [n, T] and done a bool tensor [n, T].  __call__, what CustomRewardEnv calls per step, is
    derived from batch and is not to be overridden: the host loop and the device route then cannot
    disagree.  Keep batch's arithmetic in eager torch ops on the given tensor, so that its f32 /
    f64 rounding is the same on the CPU and the GPU.

    Such a reward does not influence the dynamics, so an episode is a prefix of the un-terminated
    trajectory: TRPO's sampler rolls whole rounds out on the one-launch kernels, calls batch once
    per round and cuts each trajectory at its first done (kernel_path.cut_sampler, ops.traj_cut).
    A reward that needs the action, the base env's reward or its info is outside this protocol: it
    stays a plain function and keeps the host loop."""

    def batch(self, states):
        raise NotImplementedError

    def __call__(self, s, r, d, i):
        x = torch.as_tensor(np.asarray(s, dtype=np.float64)).reshape(1, 1, -1)
        reward, done = self.batch(x)
        return float(reward.reshape(())), bool(done.reshape(()))


class BoxGoal(BatchReward):
    """Sparse goal reward "the state is inside a box": done = all(low <= s) and all(s <= high),
    compared in f64 on the env's own state without arithmetic; the box is closed, a NaN state is
    no hit, and a bound may be +-inf (a half-space).  reward = done as 0 / 1."""

    def __init__(self, low, high):
        self.low = np.asarray(low, dtype=np.float64).reshape(-1)
        self.high = np.asarray(high, dtype=np.float64).reshape(-1)
        if self.low.shape != self.high.shape:
            raise ValueError("BoxGoal: low and high of one length")
        if np.isnan(self.low).any() or np.isnan(self.high).any():
            raise ValueError("BoxGoal: a bound is NaN")

    def batch(self, states):
        low = torch.as_tensor(self.low, device=states.device)
        high = torch.as_tensor(self.high, device=states.device)
        done = ((low <= states) & (states <= high)).all(dim=-1)
        return done.to(torch.float32), done


class AnyGoal(BatchReward):
    """"Any of these goals": done is the OR of the members' done and reward = done as 0 / 1.  A
    member is anything with batch(states) -> (reward, done): a BatchReward, a GridGoal, a
    ThresholdGoal."""

    def __init__(self, *goals):
        if not goals or not all(callable(getattr(g, "batch", None)) for g in goals):
            raise ValueError("AnyGoal: one or more goals with a batch method")
        self.goals = tuple(goals)

    def batch(self, states):
        done = self.goals[0].batch(states)[1]
        for g in self.goals[1:]:
            done = done | g.batch(states)[1]
        return done.to(torch.float32), done


def unwrap(env):
    while hasattr(env, "env") and not hasattr(type(env), "batched_kind"):
        env = env.env
    return env
