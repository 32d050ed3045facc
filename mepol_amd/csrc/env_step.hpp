// MountainCar / GridWorld / box-maze steps shared by the env kernels (envs.hip) and the deep rollout
// (rollout_deep.hip): the same IEEE operations, in the same order, as the reference's
// numpy / Python scalar code (see the header of envs.hip).
#pragma once
#include "common.hpp"

namespace mepol {
namespace envs {

// The reference's clips, min(max(a, lo), hi) in Python and np.clip: +-inf clips to the ends and a
// NaN action stays NaN, where fmin(fmax(a, lo), hi) alone returns lo.  Written as the two
// min / max instructions plus one unordered compare and select beside them, not as two ordered
// compares and selects: this sits on the serial tail of every rollout step, and the second form
// measured 0.09 us per step slower at [300, 300] (profiles/r18/rollout_ops).
__device__ __forceinline__ double clip_action(double a, double lo, double hi) {
  const double c = fmin(fmax(a, lo), hi);
  return a != a ? a : c;
}

struct MountainCar {
  static constexpr double kMinPos = -1.2, kMaxPos = 0.6, kMaxSpeed = 0.07, kGoal = 0.45;
  static constexpr double kPower = 0.0015;
  __device__ static void step(double& p, double& v, double a0) {
    const double force = clip_action(a0, -1.0, 1.0);
    // velocity += force*power - 0.0025*cos(3*position)
    const double t1 = __dmul_rn(force, kPower);
    const double t2 = __dmul_rn(0.0025, cos(__dmul_rn(3.0, p)));
    v = __dadd_rn(v, __dsub_rn(t1, t2));
    if (v > kMaxSpeed) v = kMaxSpeed;
    if (v < -kMaxSpeed) v = -kMaxSpeed;
    p = __dadd_rn(p, v);
    if (p > kMaxPos) p = kMaxPos;
    if (p < kMinPos) p = kMinPos;
    if (p == kMinPos && v < 0) v = 0.0;
    if (p > kGoal) {
      p = kGoal;
      v = 0.0;
    }
  }
};

struct GridWorld {
  static constexpr double kDim = 6.0, kMaxDelta = 0.2, kWall = 2.5;
  __device__ static bool inside(double x, double y, double x0, double x1, double y0, double y1) {
    return x0 <= x && x <= x1 && y0 <= y && y <= y1;
  }
  __device__ static void step(float& sx, float& sy, double ax, double ay) {
    const double dx = clip_action(ax, -kMaxDelta, kMaxDelta);
    const double dy = clip_action(ay, -kMaxDelta, kMaxDelta);
    const double x = (double)sx, y = (double)sy;
    double nx = __dadd_rn(x, dx), ny = __dadd_rn(y, dy);
    constexpr double h = kWall / 2;
    bool hit = inside(nx, ny, -h, h, -kWall, kWall) || inside(nx, ny, -kWall, -h, -h, h) ||
               inside(nx, ny, h, kWall, -h, h) || inside(nx, ny, -kDim, -(kDim - kWall), -h, h) ||
               inside(nx, ny, -h, h, -kDim, -(kDim - kWall)) ||
               inside(nx, ny, kDim - kWall, kDim, -h, h) ||
               inside(nx, ny, -h, h, kDim - kWall, kDim);
    if (hit) {
      nx = x;
      ny = y;
    }
    if (fabs(nx) >= kDim || fabs(ny) >= kDim) {
      nx = x;
      ny = y;
    }
    sx = (float)nx;
    sy = (float)ny;
  }
};

// A 2-D box maze (envs/maze.py BoxMazeContinuous): GridWorld's step with its constants made data.
// The kernels' ENV = 2 instances take one of these by value, so it lives in the kernel-argument
// segment: every read is a scalar load at a constant offset, uniform across the workgroup, and
// takes no LDS and no private memory.  The host validates it before every launch
// (maze_args_ok): finite numbers, 0 <= n_walls <= kMazeMaxWalls, no inverted box.
constexpr int kMazeMaxWalls = MEPOL_MAZE_MAX_WALLS;
using MazeArgs = ::mepol_maze;  // include/mepol_amd.h: the C ABI's struct is the kernels' argument

// What every maze entry point checks before it launches: false, with the message set, for a NULL
// maze, n_walls outside 0 .. 16, a number that is not finite among those in use, an inverted wall
// box or inverted bounds.  Walls behind n_walls are never read on the device and are not checked.
inline bool maze_args_ok(const MazeArgs* m, const char* who) {
  auto fin = [](double v) { return v - v == 0.0; };
  if (!m) {
    set_error("%s: maze is NULL", who);
    return false;
  }
  if (m->n_walls < 0 || m->n_walls > kMazeMaxWalls) {
    set_error("%s: maze n_walls %d outside 0 .. %d", who, m->n_walls, kMazeMaxWalls);
    return false;
  }
  if (!fin(m->xlo) || !fin(m->xhi) || !fin(m->ylo) || !fin(m->yhi) || !fin(m->max_delta)) {
    set_error("%s: maze bounds and max_delta must be finite", who);
    return false;
  }
  if (!(m->xlo < m->xhi) || !(m->ylo < m->yhi)) {
    set_error("%s: maze bounds inverted (need lo < hi)", who);
    return false;
  }
  for (int w = 0; w < m->n_walls; ++w) {
    const double* b = m->walls[w];
    if (!fin(b[0]) || !fin(b[1]) || !fin(b[2]) || !fin(b[3])) {
      set_error("%s: maze wall %d has a number that is not finite", who, w);
      return false;
    }
    if (!(b[0] <= b[1]) || !(b[2] <= b[3])) {
      set_error("%s: maze wall %d is inverted (need x0 <= x1 and y0 <= y1)", who, w);
      return false;
    }
  }
  return true;
}

struct Maze {
  // GridWorld::step in the same IEEE order.  The wall loop has the compile-time trip count
  // kMazeMaxWalls and a guard on n_walls (never a device-read loop bound), so it unrolls into
  // constant-offset reads; `hit` is taken on the landing point for every wall, which is what the
  // class's sequential loop gives (a move once undone is not undone differently by a later wall).
  __device__ static void step(float& sx, float& sy, double ax, double ay, const MazeArgs& m) {
    const double dx = clip_action(ax, -m.max_delta, m.max_delta);
    const double dy = clip_action(ay, -m.max_delta, m.max_delta);
    const double x = (double)sx, y = (double)sy;
    double nx = __dadd_rn(x, dx), ny = __dadd_rn(y, dy);
    // (Short-circuit on purpose: the uniform `w < n_walls` becomes a scalar branch that skips the
    // unused walls.  A branch-free form, 64 compares whatever n_walls is, measured the same at 16
    // walls and 0.46 us per step slower at 7: DESIGN.md section 3, Rollout.)
    bool hit = false;
#pragma unroll
    for (int w = 0; w < kMazeMaxWalls; ++w)
      hit |= w < m.n_walls && GridWorld::inside(nx, ny, m.walls[w][0], m.walls[w][1],
                                                m.walls[w][2], m.walls[w][3]);
    if (hit) {
      nx = x;
      ny = y;
    }
    // not a negated "inside": a NaN coordinate is not blocked, as GridWorld's fabs(nx) >= kDim
    if (nx <= m.xlo || nx >= m.xhi || ny <= m.ylo || ny >= m.yhi) {
      nx = x;
      ny = y;
    }
    sx = (float)nx;
    sy = (float)ny;
  }
};

// The step of an f32-state env: GridWorld (ENV 1, no further argument) or the maze (ENV 2, its
// MazeArgs).  The kernels carry the maze as a trailing parameter pack that is empty for ENV 0 and
// 1, so those instances keep the argument blocks and the code they had before the maze existed.
template <int ENV, typename... MZ>
__device__ __forceinline__ void grid_step(float& sx, float& sy, double ax, double ay,
                                          const MZ&... mz) {
  static_assert(ENV == 1 || ENV == 2, "an f32-state env");
  static_assert(sizeof...(MZ) == (ENV == 2 ? 1 : 0), "MazeArgs with ENV 2 and only there");
  if constexpr (ENV == 2)
    Maze::step(sx, sy, ax, ay, mz...);
  else
    GridWorld::step(sx, sy, ax, ay);
}

}  // namespace envs
}  // namespace mepol
