"""ErgodicEnv: ignore the done signal (src/envs/wrappers.py:4-15).  CustomRewardEnv: a reward
and termination function of the caller's (:40-52), and two such functions: GridGoal, the GridWorld
goals of src/experiments/goal_rl.py:61-77, and ThresholdGoal, the coordinate thresholds of its
other goals (:91-107)."""
import numpy as np


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

    def __call__(self, s, r, d, i):
        return (1, True) if bool(self.hit(s)) else (0, False)


def unwrap(env):
    while hasattr(env, "env") and not hasattr(type(env), "batched_kind"):
        env = env.env
    return env
