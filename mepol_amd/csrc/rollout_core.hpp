// What the rollout kernels share: rollout_step_kernel, rollout_mlp_kernel and
// rollout_mlp_mw_kernel (envs.hip) and rollout_deep_kernel (rollout_deep.hip).  The env state
// (EnvState), the records, and the pieces of the policy's forward pass whose order is a contract.
// Every helper is __forceinline__ and computes only on its arguments; an index the kernel shares
// between several arrays (2 * i) is passed in, not recomputed here.  Written this way the GridWorld
// and maze instances of all four kernels compile to the instructions they had with these lines in
// their bodies (profiles/rollout_core/README.md); a helper that indexes the kernel's arrays itself,
// or holds a loop over the actions, does not, which is why the trajectory code around the layers
// stays in the kernels.
//
// Summation order (what the k-ordered oracle, oracle/native/rollout_kordered.c, the shards and all
// three one-launch kernels commit to, so that the host may pick any form for a call):
//   layer 1       relu((x0 w0 + x1 w1) + b), explicit _rn operations (layer1);
//   layer l >= 2  column j: kRollChunks fma chains over the k ranges [r Lc, min(r Lc + Lc, hp)),
//                 Lc = ceil(hp / kRollChunks), hp the width below, each from 0.0 in k order (an
//                 empty range is 0.0), combined as ((c0 + c1) + c2) + c3, then + b, then ReLU
//                 (chunked_column; one chain per wave in the multi-workgroup form);
//   mean layer    per 64 columns the products Wm[a][j] h[j] summed by the xor butterfly
//                 32, 16, .. 1 (wave_sum; columns past the last width are 0.0), those sums added
//                 in order, then + bm[a];
//   action        mu + noise * exp(log_std), explicit _rn operations (gaussian_action).
#pragma once
#include <type_traits>

#include "common.hpp"
#include "env_step.hpp"
#include "goal_mode.hpp"

namespace mepol {
namespace envs {

constexpr int kRollMaxH = 512;   // widest hidden layer (= the largest workgroup)
constexpr int kRollMaxA = 8;     // most actions
constexpr int kRollChunks = 4;   // fma chains per layer-2+ column
constexpr int kRollU = 8;        // streamed W^T rows per batch of loads

// The state of one trajectory's env in its own dtype: MountainCar's f64 (p, v) for ENV 0, the f32
// (x, y) of GridWorld (ENV 1) and the box maze (ENV 2).
template <int ENV>
struct EnvState {
  // (s1 before s0: the compiler numbers the two values in declaration order, and in this order
  // the kernels' code is what it was with two local variables)
  std::conditional_t<ENV == 0, double, float> s1 = 0, s0 = 0;

  // a row of the env's state array, f64 [n, 2] for ENV 0, else f32 [n, 2] (the other is not
  // read).  at = 2 * i, the index of row i's first element, comes from the kernel: it uses the
  // same index for its other [n, 2] arrays and computes it once.
  __device__ __forceinline__ void load(const double* f64, const float* f32, int64_t at) {
    if constexpr (ENV == 0) {
      s0 = f64[at];
      s1 = f64[at + 1];
    } else {
      s0 = f32[at];
      s1 = f32[at + 1];
    }
  }
  __device__ __forceinline__ void store(double* f64, float* f32, int64_t at) const {
    if constexpr (ENV == 0) {
      f64[at] = s0;
      f64[at + 1] = s1;
    } else {
      f32[at] = s0;
      f32[at + 1] = s1;
    }
  }
  // the policy's two inputs (an f32 state widens exactly)
  __device__ __forceinline__ double x0() const { return (double)s0; }
  __device__ __forceinline__ double x1() const { return (double)s1; }
  // MZ: MazeArgs for ENV 2, else empty (grid_step, env_step.hpp)
  template <typename... MZ>
  __device__ __forceinline__ void step(const double* act, const MZ&... mz) {
    if constexpr (ENV == 0)
      MountainCar::step(s0, s1, act[0]);
    else
      grid_step<ENV>(s0, s1, act[0], act[1], mz...);
  }
  // the hit test of a GOAL instance on this state (goal_mode.hpp)
  template <int GOAL>
  __device__ __forceinline__ bool hit(const GoalArgs& g) const {
    static_assert(GOAL == kGoalBall || GOAL == kGoalThreshold, "a goal kind");
    static_assert(GOAL != kGoalBall || ENV != 0, "the ball goal needs an f32-state env");
    if constexpr (GOAL == kGoalBall)
      return goal_hit(s0, s1, g);
    else
      return goal_hit_threshold(x0(), x1(), g);
  }
};

// ---- records (mepol.py:74-75, 82-86) -----------------------------------------------------------
// states_rec [n, T + 1, 2] f32: row t + 1 is the state after step t, row 0 (t = -1) the initial
// state; visited [n, T, 2] f64 (nullable) the states after the steps, unrounded; final_state
// [n, 2] f64 (nullable).
__device__ __forceinline__ void record_state(float* states_rec, int64_t i, int64_t T,
                                             int64_t t, double x0, double x1) {
  states_rec[(i * (T + 1) + t + 1) * 2 + 0] = (float)x0;
  states_rec[(i * (T + 1) + t + 1) * 2 + 1] = (float)x1;
}

__device__ __forceinline__ void record_visited(double* visited, int64_t i, int64_t T,
                                               int64_t t, double x0, double x1) {
  if (visited) {
    visited[(i * T + t) * 2 + 0] = x0;
    visited[(i * T + t) * 2 + 1] = x1;
  }
}

// (at = 2 * i and the null test are the caller's, as EnvState::load's index is)
__device__ __forceinline__ void record_final(double* final_state, int64_t at, double x0,
                                             double x1) {
  final_state[at] = x0;
  final_state[at + 1] = x1;
}

// ---- the policy's pieces -----------------------------------------------------------------------
// column of layer 1 (nf = 2)
__device__ __forceinline__ double layer1(double x0, double x1, double w0, double w1, double b) {
  return fmax(__dadd_rn(__dadd_rn(__dmul_rn(x0, w0), __dmul_rn(x1, w1)), b), 0.0);
}

// Column j of a layer behind the first, before bias and ReLU: sum_r c_r over the kRollChunks row
// ranges of W^T [hp][hl] in the order above.  Rows below KL come from LDS (sw, row stride
// sw_stride, this column at sw[k * sw_stride]), the rest stream from L2 (col = W^T + j) in batches
// of U loads with the next batch in flight while this one is summed (L2 latency-bound: U rows per
// round trip).  live = false sums zeros in place of the streamed words: a thread without a column
// whose col points at column 0 (its LDS words are 0.0 already).  rollout_deep_kernel calls this;
// rollout_mlp_kernel's layer 2 is the same sum written in its body (sw_stride = blockDim.x,
// live = c1): called from there it compiled to other code.
// (Taking the four ranges as one stream of loads that runs ahead across the range boundaries was
// slower, 33.6 us per step at [300, 300, 300] against 28.0 with U = 8 and 36.4 with U = 16:
// DESIGN.md section 3, Rollout.)
template <int U>
__device__ __forceinline__ double chunked_column(const double* sw, int sw_stride,
                                                 const double* col,
                                                 const double* hin, int hp, int hl,
                                                 int KL, bool live) {
  const int Lc = (hp + kRollChunks - 1) / kRollChunks;
  double acc = 0.0;
  for (int r = 0; r < kRollChunks; ++r) {
    const int ka = min(r * Lc, hp), kb = min(ka + Lc, hp);
    double c = 0.0;
    int k = ka;
    for (; k < min(kb, KL); ++k) c = fma(sw[k * sw_stride], hin[k], c);
    double cur[U], nxt[U];
    const int kend = k + ((kb - k) / U) * U;
    if (k < kend) {
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = col[(int64_t)(k + u) * hl];
      for (; k < kend; k += U) {
        if (k + U < kend) {
#pragma unroll
          for (int u = 0; u < U; ++u) nxt[u] = col[(int64_t)(k + U + u) * hl];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) c = fma(live ? cur[u] : 0.0, hin[k + u], c);
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
      }
    }
    for (; k < kb; ++k) c = fma(live ? col[(int64_t)k * hl] : 0.0, hin[k], c);
    acc = r == 0 ? c : acc + c;
  }
  return acc;
}

// the mean layer's partial over a wave's 64 columns, in every lane (rollout_mlp_mw_kernel; the
// one-workgroup kernels keep the same loop in their bodies: see the header)
__device__ __forceinline__ double wave_sum(double q) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m, kWave);
  return q;
}

// output = mean + randn * exp(log_std)   (policy.py:59)
__device__ __forceinline__ double gaussian_action(double mu, double noise, double sd) {
  return __dadd_rn(mu, __dmul_rn(noise, sd));
}

}  // namespace envs
}  // namespace mepol
