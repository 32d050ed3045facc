// Goal mode of the one-launch rollouts, shared by the two-layer kernels (envs.hip) and the deep one
// (rollout_deep.hip): the sparse-reward episodes of goal_rl.py:61-107 under CustomRewardEnv
// (wrappers.py:40-52).  The kernels' GOAL template argument names the kind of goal, so that each
// instance holds one hit test and no run-time choice between them:
//   kGoalNone       no goal mode (GoalArgs is never read);
//   kGoalBall       GridWorld and the maze (the f32-state envs): the f32 state within `radius` of
//                   the f32 goal (goal_hit);
//   kGoalThreshold  any env: state[coord] >= threshold on the env's own state, MountainCar's
//                   f64 (p, v) or GridWorld's / the maze's f32 (sx, sy) widened exactly
//                   (goal_hit_threshold).
// After each env step the state is tested; a hit at step t gives rewards[i, t] = 1,
// len[i] = t + 1, done[i] = 1, s_{t+1} is recorded and the trajectory's workgroup(s) leave.  Every
// output row past the end is written as zeros, so the caller's buffers need no clearing.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "env_step.hpp"

namespace mepol {
namespace envs {

constexpr int kGoalNone = 0, kGoalBall = 1, kGoalThreshold = 2;

inline bool goal_kind_ok(int kind) {
  return kind == kGoalNone || kind == kGoalBall || kind == kGoalThreshold;
}

// The one mapping from a run-time (env_id, goal kind) to the rollout kernels' <ENV, GOAL, MZ...>
// instance, for every launcher and occupancy query of envs.hip and rollout_deep.hip:
//   rollout_instance(env_id, kind, mz, [&](auto E, auto G, const auto&... m) {
//     ... kernel<E(), G(), std::decay_t<decltype(m)>...> ...; return 0; });
// calls f once with std::integral_constant tags and the kernels' trailing pack: empty for env 0
// and 1, *mz for env 2 (where mz must point at a MazeArgs, if only for its type).  The instances
// are env 0 x {none, threshold} and env 1, 2 x {none, ball, threshold}: the ball goal needs an
// f32-state env, and that pair is never instantiated.  f returns an int, 0 or an error code,
// which is passed on; a pair outside the eight is refused with kErrUnsupported, f not called (the
// entry points' argument checks let none through).
template <typename F>
int rollout_instance(int env_id, int kind, const MazeArgs* mz, F&& f) {
  auto with_goal = [&](auto E, const auto&... m) -> int {
    if (kind == kGoalNone) return f(E, std::integral_constant<int, kGoalNone>{}, m...);
    if (kind == kGoalThreshold) return f(E, std::integral_constant<int, kGoalThreshold>{}, m...);
    if constexpr (E() != 0)
      if (kind == kGoalBall) return f(E, std::integral_constant<int, kGoalBall>{}, m...);
    set_error("no rollout kernel for env %d with goal kind %d", (int)E(), kind);
    return kErrUnsupported;
  };
  if (env_id == 0) return with_goal(std::integral_constant<int, 0>{});
  if (env_id == 1) return with_goal(std::integral_constant<int, 1>{});
  if (env_id == 2 && mz) return with_goal(std::integral_constant<int, 2>{}, *mz);
  set_error("no rollout kernel for env %d", env_id);
  return kErrUnsupported;
}

// One layout for both kinds (the threshold's two values share the ball's words), so that the
// kernels' argument blocks, and with them the ball instances' code, are what they were before the
// threshold kind existed.
struct GoalArgs {
  union {
    float x;    // kGoalBall: the goal, with y
    int coord;  // kGoalThreshold: the state coordinate tested, 0 or 1
  };
  float y;
  union {
    double radius;     // kGoalBall
    double threshold;  // kGoalThreshold
  };
  float* rewards;  // [n, T]
  int* len;        // [n]
  int* done;       // [n]
};

inline GoalArgs threshold_goal(int coord, double threshold, float* rewards, int* len, int* done) {
  GoalArgs g{};
  g.coord = coord;
  g.threshold = threshold;
  g.rewards = rewards;
  g.len = len;
  g.done = done;
  return g;
}

// The goal of the entry points that take the kind as an argument (mepol_rollout_maze,
// mepol_rollout_deep_maze): their rule for the goal's arguments and the GoalArgs of a kind with a
// goal.  False when the rule refuses them: a goal needs its three outputs and T <= INT32_MAX;
// the ball a goal that is not NaN and value (its radius) >= 0; the threshold coord 0 or 1 and a
// value that is not NaN.
inline bool goal_from_kind(int kind, float x, float y, int coord, double value, int64_t T,
                           float* rewards, int* len, int* done, GoalArgs* goal) {
  *goal = GoalArgs{};
  if (kind == kGoalNone) return true;
  if (!rewards || !len || !done || T > INT32_MAX) return false;
  if (kind == kGoalBall) {
    *goal = GoalArgs{{x}, y, {value}, rewards, len, done};
    return x == x && y == y && value >= 0.0;
  }
  *goal = threshold_goal(coord, value, rewards, len, done);
  return (coord == 0 || coord == 1) && value == value;
}

// np.linalg.norm(s - goal) <= radius with an f32 state and goal and a Python-float radius
// (numpy 1.x: the f32 norm is widened for the comparison): every operation rounded on its own.
__device__ __forceinline__ bool goal_hit(float sx, float sy, const GoalArgs& g) {
  const float dx = __fsub_rn(sx, g.x), dy = __fsub_rn(sy, g.y);
  const float q = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  return (double)__fsqrt_rn(q) <= g.radius;
}

// s[coord] >= threshold as Python compares a state array's element with a float: in f64, and a
// NaN state is no hit (an ordered compare).
__device__ __forceinline__ bool goal_hit_threshold(double s0, double s1, const GoalArgs& g) {
  return (g.coord ? s1 : s0) >= g.threshold;
}

// (The hit test of a GOAL instance on ENV's own state: EnvState<ENV>::hit<GOAL>, rollout_core.hpp.)

// Zeros behind an episode of `len` < T steps of trajectory i: states rows len + 1 .. T, action
// and reward rows len .. T - 1, by all nthr threads of one workgroup.
__device__ __forceinline__ void goal_zero_tail(int64_t i, int64_t len, int64_t T, int a_dim,
                                               float* __restrict__ states_rec,
                                               float* __restrict__ actions_rec,
                                               float* __restrict__ rewards, int tid, int nthr) {
  float* s = states_rec + (i * (T + 1) + len + 1) * 2;
  for (int64_t e = tid; e < (T - len) * 2; e += nthr) s[e] = 0.f;
  float* a = actions_rec + (i * T + len) * a_dim;
  for (int64_t e = tid; e < (T - len) * a_dim; e += nthr) a[e] = 0.f;
  float* r = rewards + i * T + len;
  for (int64_t e = tid; e < T - len; e += nthr) r[e] = 0.f;
}

}  // namespace envs
}  // namespace mepol
