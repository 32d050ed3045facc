// Goal mode of the one-launch rollouts (GOAL = true, GridWorld only), shared by the two-layer
// kernels (envs.hip) and the deep one (rollout_deep.hip): the sparse-reward episodes of
// goal_rl.py:61-77 under CustomRewardEnv (wrappers.py:40-52).  After each env step the f32 state is
// tested against the goal; a hit at step t gives rewards[i, t] = 1, len[i] = t + 1, done[i] = 1,
// s_{t+1} is recorded and the trajectory's workgroup(s) leave.  Every output row past the end is
// written as zeros, so the caller's buffers need no clearing.  GOAL = false never reads GoalArgs.
#pragma once
#include "common.hpp"

namespace mepol {
namespace envs {

struct GoalArgs {
  float x, y;      // the goal
  double radius;
  float* rewards;  // [n, T]
  int* len;        // [n]
  int* done;       // [n]
};

// np.linalg.norm(s - goal) <= radius with an f32 state and goal and a Python-float radius
// (numpy 1.x: the f32 norm is widened for the comparison): every operation rounded on its own.
__device__ __forceinline__ bool goal_hit(float sx, float sy, const GoalArgs& g) {
  const float dx = __fsub_rn(sx, g.x), dy = __fsub_rn(sy, g.y);
  const float q = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  return (double)__fsqrt_rn(q) <= g.radius;
}

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
