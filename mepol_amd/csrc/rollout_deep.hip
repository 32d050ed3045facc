// Whole rollout in one launch for ReLU policies with 3 to 6 hidden layers (mepol_rollout_deep):
// all T steps of collect_particles (mepol.py:81-90) for nf = 2 -> [h_1 .. h_L] -> a_dim in f64
// on MountainCar / GridWorld / a box maze (ENV 2, mepol_rollout_deep_maze).  One workgroup per
// trajectory, as rollout_mlp_kernel (envs.hip):
// thread j owns column j of every layer.  Layer 1 (nf = 2) runs from registers; the hidden
// activations ping-pong between two LDS vectors; the transposed weights W_l^T ([h_{l-1}][h_l],
// k-major) of layers 2 .. L are read coalesced from L2 every step (one 8-byte word per thread
// per k), except the leading rows of the packed W_2^T .. W_L^T buffer that fit in dynamic LDS
// (MEPOL_ROLLOUT_KL caps their number) and stay there for all T steps.  Thread 0 forms the
// action, steps the env and records, with the next step's noise loaded a step ahead: the same
// trajectory text as rollout_mlp_kernel's, on the helpers of rollout_core.hpp.
// Only __syncthreads(): L + 1 barriers per step, no exchange between workgroups.
//
// Summation order: rollout_core.hpp's, the contract shards and any later form rely on.
//
// Goal mode (GOAL = kGoalBall, GridWorld and the maze: mepol_rollout_deep_goal,
// mepol_rollout_deep_maze; GOAL = kGoalThreshold, any env: mepol_rollout_deep_goal_threshold,
// mepol_rollout_deep_maze): rollout_mlp_kernel's, with the helpers of goal_mode.hpp.  Thread 0
// tests the env's state after its step (EnvState::hit), writes the reward and, on a hit, sets a
// __shared__ flag before the step's closing barrier; behind that barrier every thread reads the
// flag and the workgroup leaves the step loop together (no further barrier), then zeroes the rows
// behind the episode.  Up to each episode's end the records are the bits the GOAL = kGoalNone
// instance writes.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "rollout_core.hpp"

namespace mepol {
namespace envs {

constexpr int kDeepMinL = 3, kDeepMaxL = 6;
constexpr int kDeepLdsBytes = 150 * 1024;  // dynamic LDS for resident W^T rows (as rollout_mlp)

struct DeepShape {
  int L;                // hidden layers
  int h[kDeepMaxL];     // their widths
  int kl[kDeepMaxL];    // kl[l], l >= 1: leading rows of layer l + 1's W^T resident in LDS
};

// MZ: MazeArgs for ENV 2 (the box maze), else empty (grid_step, env_step.hpp).
template <int ENV, int GOAL = kGoalNone, typename... MZ>
__global__ __launch_bounds__(kRollMaxH) void rollout_deep_kernel(
    const double* __restrict__ W1, const double* __restrict__ b1, const double* __restrict__ Wt,
    const double* __restrict__ bt, const double* __restrict__ Wm, const double* __restrict__ bm,
    const double* __restrict__ log_std, int a_dim, const double* __restrict__ init64,
    const float* __restrict__ init32, const double* __restrict__ noise, int64_t n, int64_t T,
    float* __restrict__ states_rec, float* __restrict__ actions_rec,
    double* __restrict__ visited, double* __restrict__ final_state, DeepShape sh,
    GoalArgs goal, MZ... mz) {
  static_assert(GOAL != kGoalBall || ENV != 0, "the ball goal needs an f32-state env");
  extern __shared__ double sW[];  // resident rows of W_2^T .. W_L^T, layer after layer
  __shared__ double sx[2];
  __shared__ int sgoal;  // GOAL: the step just taken reached the goal (thread 0 writes it)
  __shared__ double shid[2][kRollMaxH];  // hidden activations, ping-pong
  __shared__ double spart[kRollMaxH / 64][kRollMaxA];
  const int64_t i = blockIdx.x;
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int L = sh.L;
  const bool c0 = j < sh.h[0];
  const double w1a = c0 ? W1[2 * j] : 0.0, w1b = c0 ? W1[2 * j + 1] : 0.0;
  const double bb1 = c0 ? b1[j] : 0.0;
  // the resident rows of layers 2 .. L into LDS
  {
    int64_t woff = 0;
    int soff = 0;
    for (int l = 1; l < L; ++l) {
      const int words = sh.kl[l] * sh.h[l];
      for (int w = j; w < words; w += blockDim.x) sW[soff + w] = Wt[woff + w];
      woff += (int64_t)sh.h[l - 1] * sh.h[l];
      soff += words;
    }
  }
  const int hL = sh.h[L - 1];
  const bool cL = j < hL;
  double wm[kRollMaxA];
#pragma unroll
  for (int a = 0; a < kRollMaxA; ++a) wm[a] = (cL && a < a_dim) ? Wm[a * hL + j] : 0.0;
  const int nwL = (hL + 63) >> 6;  // waves that hold columns of the last hidden layer
  // ---- the trajectory around the layers: prologue here, thread 0's serial tail and the goal exit
  // in the step loop, the epilogue behind it.  The same text stands in rollout_mlp_kernel
  // (envs.hip); change the two together.  It is built from rollout_core.hpp's helpers but is
  // not one itself: as helpers these pieces compiled to other, slower code.
  EnvState<ENV> env;  // thread 0's
  if (j == 0) {
    env.load(init64, init32, 2 * i);
    sx[0] = env.x0();
    sx[1] = env.x1();
    record_state(states_rec, i, T, -1, sx[0], sx[1]);
    if constexpr (GOAL != kGoalNone) sgoal = 0;
  }
  int64_t steps = T;  // GOAL: the episode's length
  // thread 0: exp(log_std) once, and the next step's noise loaded a step ahead (its global
  // latency would otherwise sit on the serial tail of every step); the load of step t + 1 is
  // consumed inside step t (nz = nz_next), so none is pending when a GOAL workgroup leaves
  double sd[kRollMaxA], nz[kRollMaxA];
  if (j == 0) {
    for (int a = 0; a < a_dim; ++a) {
      sd[a] = exp(log_std[a]);
      nz[a] = noise[i * a_dim + a];
    }
  }
  __syncthreads();
  for (int64_t t = 0; t < T; ++t) {
    double nz_next[kRollMaxA];
    if (j == 0 && t + 1 < T)
      for (int a = 0; a < a_dim; ++a) nz_next[a] = noise[((t + 1) * n + i) * a_dim + a];
    // layer 1 (nf = 2)
    if (c0)
      shid[0][j] = layer1(sx[0], sx[1], w1a, w1b, bb1);
    __syncthreads();
    // layers 2 .. L: layer l + 1 reads shid[(l - 1) & 1] and writes shid[l & 1]; the last one
    // keeps its column in a register for the mean layer
    double hv = 0.0;
    {
      int64_t woff = 0;
      int boff = 0, soff = 0;
      for (int l = 1; l < L; ++l) {
        const int hp = sh.h[l - 1], hl = sh.h[l], kl = sh.kl[l];
        hv = 0.0;
        if (j < hl) {
          const double bias = bt[boff + j];  // (an L2 hit, in flight under the column sum)
          hv = fmax(chunked_column<kRollU>(sW + soff + j, hl, Wt + woff + j, shid[(l - 1) & 1], hp,
                                           hl, kl, true) + bias, 0.0);
        }
        if (l + 1 < L) {
          if (j < hl) shid[l & 1][j] = hv;
          __syncthreads();
        }
        woff += (int64_t)hp * hl;
        boff += hl;
        soff += kl * hl;
      }
    }
    // mean layer: per-wave partial sums over its 64 columns, then waves in order
#pragma unroll
    for (int a = 0; a < kRollMaxA; ++a) {
      if (a < a_dim) {
        double q = wm[a] * hv;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m, kWave);
        if (lane == 0) spart[wave][a] = q;
      }
    }
    __syncthreads();
    if (j == 0) {
      double act[kRollMaxA];
      for (int a = 0; a < a_dim; ++a) {
        double mu = spart[0][a];
        for (int w = 1; w < nwL; ++w) mu += spart[w][a];
        mu += bm[a];
        // output = mean + randn * exp(log_std)   (policy.py:59)
        act[a] = gaussian_action(mu, nz[a], sd[a]);
        actions_rec[(i * T + t) * a_dim + a] = (float)act[a];
      }
      if (t + 1 < T)
        for (int a = 0; a < a_dim; ++a) nz[a] = nz_next[a];
      env.step(act, mz...);
      sx[0] = env.x0();
      sx[1] = env.x1();
      record_state(states_rec, i, T, t, sx[0], sx[1]);
      record_visited(visited, i, T, t, sx[0], sx[1]);
      if constexpr (GOAL != kGoalNone) {
        const bool hit = env.template hit<GOAL>(goal);
        goal.rewards[i * T + t] = hit ? 1.f : 0.f;
        if (hit) sgoal = 1;
      }
    }
    __syncthreads();
    if constexpr (GOAL != kGoalNone) {
      if (sgoal) {  // workgroup-uniform: written before the barrier, never cleared
        steps = t + 1;
        break;
      }
    }
  }
  if (j == 0 && final_state) record_final(final_state, 2 * i, sx[0], sx[1]);
  if constexpr (GOAL != kGoalNone) {
    if (j == 0) {
      goal.len[i] = (int)steps;
      goal.done[i] = sgoal;
    }
    goal_zero_tail(i, steps, T, a_dim, states_rec, actions_rec, goal.rewards, j, blockDim.x);
  }
}

constexpr size_t kDeepWorkspaceBytes = 256;  // the error-word header

// Host-side validation shared by the two entry points; the error text names the limits.
static bool deep_shape_ok(int env_id, int n_hidden, const int* widths, int a_dim) {
  bool ok = env_id >= 0 && env_id <= 1 && n_hidden >= kDeepMinL && n_hidden <= kDeepMaxL &&
            widths && a_dim >= 1 && a_dim <= kRollMaxA && !(env_id == 1 && a_dim != 2);
  for (int l = 0; ok && l < n_hidden; ++l) ok = widths[l] >= 1 && widths[l] <= kRollMaxH;
  return ok;
}

static int deep_bad_args(const char* who) {
  set_error("%s: bad arguments (env 0 or 1, %d <= n_hidden <= %d, 1 <= width <= %d, "
            "1 <= a_dim <= %d, GridWorld a_dim = 2, no null pointers)",
            who, kDeepMinL, kDeepMaxL, kRollMaxH, kRollMaxA);
  return kErrBadArg;
}

// What a launch at this shape looks like, for the launchers and the occupancy query alike: the
// kernel's shape argument, the workgroup size and the dynamic LDS.
struct DeepPlan {
  DeepShape sh;
  unsigned threads;
  size_t lds;
};

static DeepPlan deep_plan(int n_hidden, const int* widths) {
  DeepPlan p;
  DeepShape& sh = p.sh;
  sh.L = n_hidden;
  int wmax = 0;
  for (int l = 0; l < kDeepMaxL; ++l) {
    sh.h[l] = l < n_hidden ? widths[l] : 0;
    sh.kl[l] = 0;
    wmax = std::max(wmax, sh.h[l]);
  }
  // leading rows of the packed W_2^T .. W_L^T kept in LDS: whole rows, layer after layer, while
  // they fit (MEPOL_ROLLOUT_KL caps their number); everything behind them streams
  const char* klv = getenv("MEPOL_ROLLOUT_KL");
  int rows_left = klv ? std::max(0, atoi(klv)) : INT_MAX;
  int words_left = kDeepLdsBytes / (int)sizeof(double);
  p.lds = 0;
  for (int l = 1; l < n_hidden; ++l) {
    const int rows = std::min({sh.h[l - 1], words_left / sh.h[l], rows_left});
    sh.kl[l] = rows;
    words_left -= rows * sh.h[l];
    rows_left -= rows;
    p.lds += (size_t)rows * sh.h[l] * sizeof(double);
    if (rows < sh.h[l - 1]) break;
  }
  p.threads = (unsigned)((wmax + 63) / 64 * 64);
  return p;
}

// mepol_rollout_deep (kind kGoalNone, ga unused), mepol_rollout_deep_goal (kGoalBall, env 1) and
// mepol_rollout_deep_goal_threshold (kGoalThreshold) behind their argument checks: the same
// plan, workspace header and launch, the kernel's GOAL instances for the last two.  env_id 2
// (mepol_rollout_deep_maze, any kind): the ENV = 2 instances with *mz, already validated.
static int deep_run(int env_id, int kind, const GoalArgs& ga, int n_hidden, const int* widths,
                    const double* W1, const double* b1, const double* Wt, const double* bt,
                    const double* Wm, const double* bm, const double* log_std, int a_dim,
                    const double* init64, const float* init32, const double* noise, int64_t n,
                    int64_t T, float* states_rec, float* actions_rec, double* visited,
                    double* final_state, void* workspace, void* stream,
                    const MazeArgs* mz = nullptr) {
  const DeepPlan p = deep_plan(n_hidden, widths);
  hipStream_t st = (hipStream_t)stream;
  if (workspace) MEPOL_HIP(hipMemsetAsync(workspace, 0, kDeepWorkspaceBytes, st));
  const dim3 g((unsigned)n), b(p.threads);
  return rollout_instance(env_id, kind, mz, [&](auto E, auto G, const auto&... m) {
    constexpr auto kernel = rollout_deep_kernel<E(), G(), std::decay_t<decltype(m)>...>;
    MEPOL_HIP((max_dynamic_lds<kernel>(kDeepLdsBytes)));
    hipLaunchKernelGGL(kernel, g, b, p.lds, st, W1, b1, Wt, bt, Wm, bm, log_std, a_dim, init64,
                       init32, noise, n, T, states_rec, actions_rec, visited, final_state, p.sh, ga,
                       m...);
    MEPOL_CHECK_LAUNCH();
    return 0;
  });
}

// The deep *_plan_info entry points behind their own argument checks: workgroups of the
// (env, kind) instance the device holds at once for this shape, the kernel's occupancy at the
// block size and dynamic LDS the launcher chooses, times the CU count.
static int deep_resident(int env_id, int kind, int n_hidden, const int* widths,
                         int* resident_workgroups) {
  const DeepPlan p = deep_plan(n_hidden, widths);
  int dev = 0, cus = 0, per_cu = 0;
  MEPOL_HIP(hipGetDevice(&dev));
  MEPOL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const MazeArgs type_only{};  // (the query reads no maze)
  const int rc =
      rollout_instance(env_id, kind, &type_only, [&](auto E, auto G, const auto&... m) {
        constexpr auto kernel = rollout_deep_kernel<E(), G(), std::decay_t<decltype(m)>...>;
        MEPOL_HIP((max_dynamic_lds<kernel>(kDeepLdsBytes)));
        MEPOL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)p.threads,
                                                               p.lds));
        return 0;
      });
  if (rc) return rc;
  *resident_workgroups = per_cu * cus;
  return 0;
}

}  // namespace envs
}  // namespace mepol

using namespace mepol;
using namespace mepol::envs;

extern "C" int mepol_rollout_deep_workspace_size(int64_t n, int64_t T, int n_hidden,
                                                 const int* widths, int a_dim, size_t* bytes) {
  // (the env does not change the size: MountainCar's a_dim range covers GridWorld's)
  if (n < 0 || T < 0 || !bytes || !deep_shape_ok(0, n_hidden, widths, a_dim))
    return deep_bad_args("mepol_rollout_deep_workspace_size");
  *bytes = kDeepWorkspaceBytes;
  return 0;
}

extern "C" int mepol_rollout_deep(int env_id, int n_hidden, const int* widths, const double* W1,
                                  const double* b1, const double* Wt, const double* bt,
                                  const double* Wm, const double* bm, const double* log_std,
                                  int a_dim, const double* init64, const float* init32,
                                  const double* noise, int64_t n, int64_t T, float* states_rec,
                                  float* actions_rec, double* visited, double* final_state,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (!deep_shape_ok(env_id, n_hidden, widths, a_dim) || (env_id == 0 && !init64) ||
      (env_id == 1 && !init32) || !W1 || !b1 || !Wt || !bt || !Wm || !bm || !log_std || !noise ||
      !states_rec || !actions_rec)
    return deep_bad_args("mepol_rollout_deep");
  if (workspace && workspace_bytes < kDeepWorkspaceBytes) {
    set_error("mepol_rollout_deep: workspace of %zu bytes, %zu needed", workspace_bytes,
              kDeepWorkspaceBytes);
    return kErrWorkspace;
  }
  return deep_run(env_id, kGoalNone, GoalArgs{}, n_hidden, widths, W1, b1, Wt, bt, Wm, bm, log_std,
                  a_dim, init64, init32, noise, n, T, states_rec, actions_rec, visited,
                  final_state, workspace, stream);
}

// Workgroups (= trajectories) of mepol_rollout_deep itself the device holds at once: the
// occupancy of the instance without a goal on this env, as mepol_rollout_deep_goal_plan_info
// reports the goal instance's.
extern "C" int mepol_rollout_deep_plan_info(int env_id, int n_hidden, const int* widths, int a_dim,
                                            int* resident_workgroups) {
  if (!resident_workgroups || !deep_shape_ok(env_id, n_hidden, widths, a_dim))
    return deep_bad_args("mepol_rollout_deep_plan_info");
  return deep_resident(env_id, kGoalNone, n_hidden, widths, resident_workgroups);
}

// mepol_rollout_deep on GridWorld with early termination at a goal: mepol_rollout_goal's episode
// semantics and outputs for 3 to 6 hidden layers, one workgroup per trajectory (no error word is
// ever set).  The workspace is mepol_rollout_deep_workspace_size's.
extern "C" int mepol_rollout_deep_goal(int env_id, int n_hidden, const int* widths,
                                       const double* W1, const double* b1, const double* Wt,
                                       const double* bt, const double* Wm, const double* bm,
                                       const double* log_std, int a_dim, const float* init32,
                                       const double* noise, int64_t n, int64_t T, float goal_x,
                                       float goal_y, double radius, float* states_rec,
                                       float* actions_rec, float* rewards_rec, int32_t* len_out,
                                       int32_t* done_out, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (a_dim != 2 || !deep_shape_ok(env_id, n_hidden, widths, a_dim) || T > INT32_MAX || !init32 ||
      !W1 || !b1 || !Wt || !bt || !Wm || !bm || !log_std || !noise || !states_rec ||
      !actions_rec || !rewards_rec || !len_out || !done_out || !(goal_x == goal_x) ||
      !(goal_y == goal_y) || !(radius >= 0.0)) {
    set_error("mepol_rollout_deep_goal: bad arguments (%d <= n_hidden <= %d, 1 <= width <= %d, "
              "a_dim = 2, radius >= 0, no null pointers)",
              kDeepMinL, kDeepMaxL, kRollMaxH);
    return kErrBadArg;
  }
  if (env_id != 1) {
    set_error("mepol_rollout_deep_goal: only GridWorld (env_id 1) has a goal mode");
    return kErrUnsupported;
  }
  if (workspace && workspace_bytes < kDeepWorkspaceBytes) {
    set_error("mepol_rollout_deep_goal: workspace of %zu bytes, %zu needed", workspace_bytes,
              kDeepWorkspaceBytes);
    return kErrWorkspace;
  }
  const GoalArgs goal{{goal_x}, goal_y, {radius}, rewards_rec, len_out, done_out};
  return deep_run(1, kGoalBall, goal, n_hidden, widths, W1, b1, Wt, bt, Wm, bm, log_std, a_dim,
                  nullptr, init32, noise, n, T, states_rec, actions_rec, nullptr, nullptr,
                  workspace, stream);
}

// Workgroups of the goal-mode instance the device holds at once for this shape: the kernel's
// occupancy at the block size and dynamic LDS the launcher chooses, times the CU count.  A round
// of at most this many trajectories runs in one wave of workgroups.
extern "C" int mepol_rollout_deep_goal_plan_info(int n_hidden, const int* widths, int a_dim,
                                                 int* resident_workgroups) {
  if (a_dim != 2 || !resident_workgroups || !deep_shape_ok(1, n_hidden, widths, a_dim)) {
    set_error("mepol_rollout_deep_goal_plan_info: bad arguments (%d <= n_hidden <= %d, "
              "1 <= width <= %d, a_dim = 2)",
              kDeepMinL, kDeepMaxL, kRollMaxH);
    return kErrBadArg;
  }
  return deep_resident(1, kGoalBall, n_hidden, widths, resident_workgroups);
}

// mepol_rollout_deep_goal with the threshold test of mepol_rollout_goal_threshold, on either env.
extern "C" int mepol_rollout_deep_goal_threshold(
    int env_id, int n_hidden, const int* widths, const double* W1, const double* b1,
    const double* Wt, const double* bt, const double* Wm, const double* bm, const double* log_std,
    int a_dim, const double* init64, const float* init32, const double* noise, int64_t n,
    int64_t T, int coord, double threshold, float* states_rec, float* actions_rec,
    float* rewards_rec, int32_t* len_out, int32_t* done_out, void* workspace,
    size_t workspace_bytes, void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (!deep_shape_ok(env_id, n_hidden, widths, a_dim) || a_dim != (env_id == 0 ? 1 : 2) ||
      T > INT32_MAX || (env_id == 0 && !init64) || (env_id == 1 && !init32) || !W1 || !b1 || !Wt ||
      !bt || !Wm || !bm || !log_std || !noise || !states_rec || !actions_rec || !rewards_rec ||
      !len_out || !done_out || (coord != 0 && coord != 1) || threshold != threshold) {
    set_error("mepol_rollout_deep_goal_threshold: bad arguments (env 0 with a_dim = 1 and init64 "
              "or env 1 with a_dim = 2 and init32, %d <= n_hidden <= %d, 1 <= width <= %d, coord "
              "0 or 1, threshold not NaN, no null pointers)",
              kDeepMinL, kDeepMaxL, kRollMaxH);
    return kErrBadArg;
  }
  if (workspace && workspace_bytes < kDeepWorkspaceBytes) {
    set_error("mepol_rollout_deep_goal_threshold: workspace of %zu bytes, %zu needed",
              workspace_bytes, kDeepWorkspaceBytes);
    return kErrWorkspace;
  }
  const GoalArgs goal = threshold_goal(coord, threshold, rewards_rec, len_out, done_out);
  return deep_run(env_id, kGoalThreshold, goal, n_hidden, widths, W1, b1, Wt, bt, Wm, bm, log_std,
                  a_dim, init64, init32, noise, n, T, states_rec, actions_rec, nullptr, nullptr,
                  workspace, stream);
}

// mepol_rollout_deep_goal_plan_info for the threshold instance of this env.
extern "C" int mepol_rollout_deep_goal_threshold_plan_info(int env_id, int n_hidden,
                                                           const int* widths, int a_dim,
                                                           int* resident_workgroups) {
  if (!resident_workgroups || !deep_shape_ok(env_id, n_hidden, widths, a_dim) ||
      a_dim != (env_id == 0 ? 1 : 2)) {
    set_error("mepol_rollout_deep_goal_threshold_plan_info: bad arguments (env 0 with a_dim = 1 "
              "or env 1 with a_dim = 2, %d <= n_hidden <= %d, 1 <= width <= %d)",
              kDeepMinL, kDeepMaxL, kRollMaxH);
    return kErrBadArg;
  }
  return deep_resident(env_id, kGoalThreshold, n_hidden, widths, resident_workgroups);
}

// ---- box mazes (env 2) -------------------------------------------------------------------------
// mepol_rollout_deep, mepol_rollout_deep_goal and mepol_rollout_deep_goal_threshold folded by goal
// kind (include/mepol_amd.h): the ENV = 2 instances behind the same checks plus maze_args_ok.
static int deep_maze_bad_args(const char* who) {
  set_error("%s: bad arguments (goal kind 0 .. 2, %d <= n_hidden <= %d, 1 <= width <= %d, "
            "a_dim = 2; ball: radius >= 0; threshold: coord 0 or 1, threshold not NaN; no null "
            "pointers)",
            who, kDeepMinL, kDeepMaxL, kRollMaxH);
  return kErrBadArg;
}

static bool deep_maze_shape_ok(int goal_kind, int n_hidden, const int* widths, int a_dim) {
  return goal_kind_ok(goal_kind) && a_dim == 2 && deep_shape_ok(1, n_hidden, widths, a_dim);
}

extern "C" int mepol_rollout_deep_maze_workspace_size(int64_t n, int64_t T, int n_hidden,
                                                      const int* widths, int a_dim,
                                                      size_t* bytes) {
  if (n < 0 || T < 0 || !bytes || !deep_maze_shape_ok(kGoalNone, n_hidden, widths, a_dim))
    return deep_maze_bad_args("mepol_rollout_deep_maze_workspace_size");
  *bytes = kDeepWorkspaceBytes;
  return 0;
}

extern "C" int mepol_rollout_deep_maze_plan_info(int goal_kind, int n_hidden, const int* widths,
                                                 int a_dim, int* resident_workgroups) {
  if (!resident_workgroups || !deep_maze_shape_ok(goal_kind, n_hidden, widths, a_dim))
    return deep_maze_bad_args("mepol_rollout_deep_maze_plan_info");
  return deep_resident(2, goal_kind, n_hidden, widths, resident_workgroups);
}

extern "C" int mepol_rollout_deep_maze(
    const mepol_maze* maze, int goal_kind, int n_hidden, const int* widths, const double* W1,
    const double* b1, const double* Wt, const double* bt, const double* Wm, const double* bm,
    const double* log_std, int a_dim, const float* init32, const double* noise, int64_t n,
    int64_t T, float goal_x, float goal_y, int coord, double goal_value, float* states_rec,
    float* actions_rec, double* visited, double* final_state, float* rewards_rec,
    int32_t* len_out, int32_t* done_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!maze_args_ok(maze, "mepol_rollout_deep_maze")) return kErrBadArg;
  GoalArgs goal;
  const bool goal_ok = goal_from_kind(goal_kind, goal_x, goal_y, coord, goal_value, T, rewards_rec,
                                      len_out, done_out, &goal);
  if (!deep_maze_shape_ok(goal_kind, n_hidden, widths, a_dim) || !goal_ok || !init32 || !W1 ||
      !b1 || !Wt || !bt || !Wm || !bm || !log_std || !noise || !states_rec || !actions_rec)
    return deep_maze_bad_args("mepol_rollout_deep_maze");
  if (workspace && workspace_bytes < kDeepWorkspaceBytes) {
    set_error("mepol_rollout_deep_maze: workspace of %zu bytes, %zu needed", workspace_bytes,
              kDeepWorkspaceBytes);
    return kErrWorkspace;
  }
  if (n <= 0 || T <= 0) return 0;
  return deep_run(2, goal_kind, goal, n_hidden, widths, W1, b1, Wt, bt, Wm, bm, log_std, a_dim,
                  nullptr, init32, noise, n, T, states_rec, actions_rec, visited, final_state,
                  workspace, stream, maze);
}
