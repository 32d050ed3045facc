"""Continuous 2-D maze whose layout is data: bounds, step size, start box and a list of
axis-aligned wall boxes.  GridWorldContinuous (envs/gridworld.py) is one instance of it
(BoxMazeContinuous.gridworld()), and its step is GridWorld's with the constants made data, in the
same IEEE order, so that instance reproduces GridWorld bit for bit.

Single-env numpy API for compatibility; the rollouts step batches of it on the GPU inside the
one-launch kernels (``batched_kind``, csrc/env_step.hpp Maze::step, the kernels' env 2), with the
layout passed as a kernel argument.  Rendering is out of scope.
"""
import math

import numpy as np

from .spaces import Box

MAZE_MAX_WALLS = 16  # MEPOL_MAZE_MAX_WALLS, include/mepol_amd.h


class BoxMazeContinuous:
    """A point that moves by a clipped action inside the open rectangle `bounds` = (xlo, xhi, ylo,
    yhi) among `walls`, closed boxes (x0, x1, y0, y1).  A move whose landing point lies in a wall,
    or on or outside a bound, is undone (both coordinates).  The test is made at the landing point
    only, as in the reference's GridWorld: a wall thinner than `max_delta` can be stepped over.
    The start state is uniform over `init_box` = ((x_lo, y_lo), (x_hi, y_hi)), rounded to f32.

    At most MAZE_MAX_WALLS walls (zero is legal), every number finite, x0 <= x1 and y0 <= y1,
    lo < hi for the bounds, and the start box inside the closed bounds; otherwise ValueError."""

    batched_kind = "maze"

    def __init__(self, bounds, walls=(), max_delta=0.2, init_box=None):
        try:
            xlo, xhi, ylo, yhi = bounds
            walls = [tuple(w) for w in walls]
            if any(len(w) != 4 for w in walls):
                raise TypeError
        except TypeError:
            raise ValueError("BoxMazeContinuous: bounds = (xlo, xhi, ylo, yhi) and walls = "
                             "[(x0, x1, y0, y1), ...]") from None
        if init_box is None:
            init_box = ((xlo, ylo), (xhi, yhi))
        (ix0, iy0), (ix1, iy1) = init_box
        if len(walls) > MAZE_MAX_WALLS:
            raise ValueError(f"BoxMazeContinuous: {len(walls)} walls, at most {MAZE_MAX_WALLS}")
        numbers = [xlo, xhi, ylo, yhi, max_delta, ix0, iy0, ix1, iy1] + [v for w in walls for v in w]
        if not all(math.isfinite(v) for v in numbers):
            raise ValueError("BoxMazeContinuous: every number must be finite")
        if not (xlo < xhi and ylo < yhi):
            raise ValueError("BoxMazeContinuous: bounds need lo < hi")
        for (x0, x1, y0, y1) in walls:
            if not (x0 <= x1 and y0 <= y1):
                raise ValueError(f"BoxMazeContinuous: wall {(x0, x1, y0, y1)} is inverted "
                                 "(need x0 <= x1 and y0 <= y1)")
        if not (xlo <= ix0 <= ix1 <= xhi and ylo <= iy0 <= iy1 <= yhi):
            raise ValueError("BoxMazeContinuous: the start box must lie inside the closed bounds")
        self.num_features = 2
        self.bounds = (xlo, xhi, ylo, yhi)
        self.max_delta = max_delta
        self.walls = walls
        self.init_box = ((ix0, iy0), (ix1, iy1))
        ma = np.array([max_delta, max_delta], dtype=np.float32)
        self.action_space = Box(-ma, ma, dtype=np.float32)
        self.observation_space = Box(np.array([xlo, ylo], dtype=np.float32),
                                     np.array([xhi, yhi], dtype=np.float32), dtype=np.float32)
        self.init_states = Box(np.array([ix0, iy0], dtype=np.float32),
                               np.array([ix1, iy1], dtype=np.float32), dtype=np.float32)
        self.state = None

    @classmethod
    def gridworld(cls, dim=6, max_delta=0.2, wall_width=2.5):
        """The maze equal to GridWorldContinuous(dim, max_delta, wall_width): the same seven wall
        tuples by the same expressions, bounds +-dim, the same start box."""
        h, w, d = wall_width / 2, wall_width, dim
        walls = [(-h, h, -w, w), (-w, -h, -h, h), (h, w, -h, h), (-d, -(d - w), -h, h),
                 (-h, h, -d, -(d - w)), (d - w, d, -h, h), (-h, h, d - w, d)]
        return cls((-dim, dim, -dim, dim), walls, max_delta,
                   ((-dim, -dim), (-dim + 2, -dim + 2)))

    @classmethod
    def four_rooms(cls):
        """A +-6 square split into four rooms by a cross of 0.5-thick walls; each of the cross's
        four arms has one door, 1.0 wide (six wall boxes).  Starts in the lower-left corner, as
        GridWorld; max_delta 0.2."""
        t = 0.25  # half the wall thickness
        pieces = [(-6.0, -3.5), (-2.5, 2.5), (3.5, 6.0)]  # doors at 2.5 .. 3.5 on either side
        walls = [(-t, t, a, b) for a, b in pieces] + [(a, b, -t, t) for a, b in pieces]
        return cls((-6.0, 6.0, -6.0, 6.0), walls, 0.2, ((-6.0, -6.0), (-4.0, -4.0)))

    def kernel_key(self):
        """What the HIP step depends on, hashable: two mazes with equal keys step alike."""
        return (tuple(float(v) for v in self.bounds), float(self.max_delta),
                tuple(tuple(float(v) for v in w) for w in self.walls))

    def seed(self, seed=None):
        self.init_states.seed(seed)
        return [seed]

    def reset(self):
        self.state = self.init_states.sample()
        return self.state

    def reset_batch_torch(self, n, device, generator=None):
        """n initial states [n, 2] as f32 tensor on device (same distribution as reset())."""
        return self.init_states.sample_torch(n, device, generator).to(dtype=__import__("torch").float32)

    def step(self, action):
        x, y = self.state
        dx = np.clip(action[0], -self.max_delta, self.max_delta)
        dy = np.clip(action[1], -self.max_delta, self.max_delta)
        nx, ny = float(x) + float(dx), float(y) + float(dy)
        for (x0, x1, y0, y1) in self.walls:
            if x0 <= nx <= x1 and y0 <= ny <= y1:
                nx, ny = x, y
        xlo, xhi, ylo, yhi = self.bounds
        # (not a negated "inside": a NaN coordinate is not blocked, as GridWorld's abs(nx) >= dim)
        if nx <= xlo or nx >= xhi or ny <= ylo or ny >= yhi:
            nx, ny = x, y
        self.state = np.array([nx, ny], dtype=np.float32)
        return self.state, 0, False, {}
