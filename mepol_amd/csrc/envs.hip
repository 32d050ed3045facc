// Batched environment steppers for the MEPOL rollout (collect_particles, mepol.py:70-111).
//
//  MountainCar   src/envs/mountain_car_wall.py:13-45 (+ gym 0.17.2 Continuous_MountainCarEnv
//                constants: position in [-1.2, 0.6], |v| <= 0.07, power 0.0015, goal 0.45).
//                State is f64 (np.array([position, velocity]), :44).
//  GridWorld     src/envs/gridworld_continuous.py:128-154, walls :66-76.  State is f32
//                (:150); the move is evaluated in f64 (f32 state + f64 clipped action).
//  Box maze      mepol_amd/envs/maze.py (no counterpart in the reference): GridWorld's step with
//                bounds, max_delta and up to 16 wall boxes as data, a kernel argument of the
//                ENV = 2 instances (env_step.hpp Maze::step, MazeArgs).
//  ErgodicEnv    src/envs/wrappers.py:12-15: done is always False, every trajectory runs T steps.
//
// Each step is evaluated with the same IEEE operations, in the same order, as the reference's
// numpy/Python scalar code (explicit _rn intrinsics: no contraction), so a step is bit-exact
// except for cos() in MountainCar, whose last-ulp rounding may differ from glibc.
//
// The fused rollout step takes the policy mean from the PyTorch MLP and Gaussian noise, forms
// a = mean + noise * exp(log_std) (policy.py:59), records (s_t, a_t) as f32 (mepol.py:74-75,
// 82-86) and advances the env state, all in one launch per step.
#include "rollout_core.hpp"

namespace mepol {
namespace envs {

__global__ void step_mc_kernel(double* __restrict__ s, const double* __restrict__ a, int64_t n,
                               int64_t a_stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p = s[2 * i], v = s[2 * i + 1];
  MountainCar::step(p, v, a[i * a_stride]);
  s[2 * i] = p;
  s[2 * i + 1] = v;
}

__global__ void step_gw_kernel(float* __restrict__ s, const double* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = s[2 * i], y = s[2 * i + 1];
  GridWorld::step(x, y, a[2 * i], a[2 * i + 1]);
  s[2 * i] = x;
  s[2 * i + 1] = y;
}

__global__ void step_maze_kernel(float* __restrict__ s, const double* __restrict__ a, int64_t n,
                                 MazeArgs mz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = s[2 * i], y = s[2 * i + 1];
  Maze::step(x, y, a[2 * i], a[2 * i + 1], mz);
  s[2 * i] = x;
  s[2 * i + 1] = y;
}

// One rollout step for n trajectories.  env_f64: MountainCar state [n,2] (f64);
// env_f32: GridWorld / maze state [n,2] (f32).  policy_in [n,2] f64 receives the next policy input.
// states_rec [n, T+1, 2] f32, actions_rec [n, T, a_dim] f32.  MZ: MazeArgs for ENV 2, else empty
// (EnvState::step, rollout_core.hpp).
template <int ENV, typename... MZ>
__global__ void rollout_step_kernel(double* __restrict__ env_f64, float* __restrict__ env_f32,
                                    const double* __restrict__ mean,
                                    const double* __restrict__ noise,
                                    const double* __restrict__ log_std, int64_t n, int a_dim,
                                    int64_t t, int64_t T, float* __restrict__ states_rec,
                                    float* __restrict__ actions_rec,
                                    double* __restrict__ policy_in, MZ... mz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double act[8];
  for (int j = 0; j < a_dim && j < 8; ++j) {
    act[j] = gaussian_action(mean[i * a_dim + j], noise[i * a_dim + j], exp(log_std[j]));
    actions_rec[(i * T + t) * a_dim + j] = (float)act[j];
  }
  EnvState<ENV> env;
  env.load(env_f64, env_f32, 2 * i);
  env.step(act, mz...);
  env.store(env_f64, env_f32, 2 * i);
  policy_in[2 * i] = env.x0();
  policy_in[2 * i + 1] = env.x1();
  record_state(states_rec, i, T, t, env.x0(), env.x1());
}

// ---- whole rollout in one launch -----------------------------------------------------------
// One workgroup per trajectory runs all T steps of collect_particles (mepol.py:81-90) for the
// reference's 2-hidden-layer ReLU policy: x -> relu(W1 x + b1) -> relu(W2 h1 + b2) -> mean
// (policy.py:21-28, 53-61) -> a = mean + noise * exp(log_std) -> env step, with the states /
// actions recorded as f32.  Thread j owns hidden column j; its W1 row, biases and mean-layer
// column stay in registers, the first KL rows of W2^T (k-major, [h0][h1]) in LDS, and the rest
// of W2^T streams from L2 each step (coalesced: one 8-byte word per thread per k).  Replaces
// the per-step launch sequence (3 GEMMs + bias/ReLU + rollout_step, ~58 us per step even as a
// replayed graph) with ~3 barriers per step.
// Summation order: rollout_core.hpp's, which is also the multi-workgroup form's (one layer-2
// chain per wave there), so both forms give the same bits and the host may pick either (or fall
// back from one to the other) per call.
// Goal mode (GOAL = kGoalBall, GridWorld and the maze, or kGoalThreshold, any env): goal_mode.hpp.
// MZ: MazeArgs for ENV 2, else empty (EnvState::step).
template <int ENV, int GOAL = kGoalNone, typename... MZ>
__global__ __launch_bounds__(kRollMaxH) void rollout_mlp_kernel(
    const double* __restrict__ W1, const double* __restrict__ b1, int h0,
    const double* __restrict__ W2t, const double* __restrict__ b2, int h1,
    const double* __restrict__ Wm, const double* __restrict__ bm,
    const double* __restrict__ log_std, int a_dim, const double* __restrict__ init64,
    const float* __restrict__ init32, const double* __restrict__ noise, int64_t n, int64_t T,
    float* __restrict__ states_rec, float* __restrict__ actions_rec,
    double* __restrict__ visited, double* __restrict__ final_state, int KL, GoalArgs goal,
    MZ... mz) {
  static_assert(GOAL != kGoalBall || ENV != 0, "the ball goal needs an f32-state env");
  constexpr int U = kRollU;
  extern __shared__ double sW2[];  // [KL][blockDim.x]: W2^T rows 0 .. KL - 1
  __shared__ double sx[2];
  __shared__ int sgoal;  // GOAL: the step just taken reached the goal (thread 0 writes it)
  __shared__ double sh1[kRollMaxH];
  __shared__ double spart[kRollMaxH / 64][kRollMaxA];
  const int64_t i = blockIdx.x;
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6, nw = blockDim.x >> 6;
  const bool c0 = j < h0, c1 = j < h1;
  const double w1a = c0 ? W1[2 * j] : 0.0, w1b = c0 ? W1[2 * j + 1] : 0.0;
  const double bb1 = c0 ? b1[j] : 0.0, bb2 = c1 ? b2[j] : 0.0;
  double wm[kRollMaxA];
#pragma unroll
  for (int a = 0; a < kRollMaxA; ++a) wm[a] = (c1 && a < a_dim) ? Wm[a * h1 + j] : 0.0;
  for (int k = 0; k < KL; ++k) sW2[k * blockDim.x + j] = c1 ? W2t[(int64_t)k * h1 + j] : 0.0;
  const int L = (h0 + kRollChunks - 1) / kRollChunks;
  // ---- the trajectory around the layers: prologue here, thread 0's serial tail and the goal exit
  // in the step loop, the epilogue behind it.  The same text stands in rollout_deep_kernel
  // (rollout_deep.hip); change the two together.  It is built from rollout_core.hpp's helpers but is
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
  // latency would otherwise sit on the serial tail of every step)
  double sd[kRollMaxA], nz[kRollMaxA];
  if (j == 0) {
    for (int a = 0; a < a_dim; ++a) {
      sd[a] = exp(log_std[a]);
      nz[a] = noise[i * a_dim + a];
    }
  }
  __syncthreads();
  const double* col = W2t + (c1 ? j : 0);
  for (int64_t t = 0; t < T; ++t) {
    double nz_next[kRollMaxA];
    if (j == 0 && t + 1 < T)
      for (int a = 0; a < a_dim; ++a) nz_next[a] = noise[((t + 1) * n + i) * a_dim + a];
    // layer 1 (nf = 2)
    if (c0) sh1[j] = layer1(sx[0], sx[1], w1a, w1b, bb1);
    __syncthreads();
    // layer 2: h2_j = relu(sum_r c_r + b2[j]); the column sum is chunked_column (rollout_core.hpp)
    // with sw_stride = blockDim.x and live = c1, written here (see there)
    double acc = 0.0;
    for (int r = 0; r < kRollChunks; ++r) {
      const int ka = min(r * L, h0), kb = min(ka + L, h0);
      double c = 0.0;
      int k = ka;
      for (; k < min(kb, KL); ++k) c = fma(sW2[k * blockDim.x + j], sh1[k], c);
      double cur[U], nxt[U];
      const int kend = k + ((kb - k) / U) * U;
      if (k < kend) {
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = col[(int64_t)(k + u) * h1];
        for (; k < kend; k += U) {
          if (k + U < kend) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = col[(int64_t)(k + U + u) * h1];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) c = fma(c1 ? cur[u] : 0.0, sh1[k + u], c);
#pragma unroll
          for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
      }
      for (; k < kb; ++k) c = fma(c1 ? col[(int64_t)k * h1] : 0.0, sh1[k], c);
      acc = r == 0 ? c : acc + c;
    }
    const double h2 = c1 ? fmax(acc + bb2, 0.0) : 0.0;
    // mean layer: per-wave partial sums over its 64 columns, then waves in order
#pragma unroll
    for (int a = 0; a < kRollMaxA; ++a) {
      if (a < a_dim) {
        double q = wm[a] * h2;
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
        for (int w = 1; w < nw; ++w) mu += spart[w][a];
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

// ---- whole rollout, several workgroups per trajectory --------------------------------------
// rollout_mlp_kernel puts a trajectory on ONE CU, which then streams most of W2^T from L2 every
// step (11.7 us per step at C2's [300, 300]).  Here NP = ceil(h1 / 64) workgroups share a
// trajectory: workgroup p owns hidden-2 columns [64 p, 64 p + 64) and keeps their W2^T slice
// ([h0][64] f64, <= 154 KB) in LDS for all T steps.  Per step:
//   layer 1   all h0 columns (redundantly in every workgroup), 256 threads;
//   layer 2   its 64 columns; wave w of the 4 sums chunk w of rollout_core.hpp's order as one
//             fma chain (a single chain over 300 rows was 5.6 of the 8.4 us step:
//             tools/rollout_probe.py), and the column total is ((c0 + c1) + c2) + c3;
//   mean      wave 0's partial of the mean layer over its 64 columns (xor shuffle tree),
//             published as NP * a_dim self-validating 8-byte mail words (sc1 stores) and polled
//             with sc1 loads by wave 0 of every workgroup of the trajectory (bounded: err = 1);
//   env       every thread sums the NP partials in part order, adds bm and the noise and steps
//             the env (the same state in every thread).
// The order is oracle/native/rollout_kordered.c's with k_chunks = 4 (mepol_rollout_mlp_plan_info
// reports it).  Needs all n * NP workgroups resident at once (one per CU by LDS): the host
// launches it only when n * NP <= the CU count.
// PROBE (tools/variants/rollout_probe.hip only): thread 0 of each workgroup accumulates
// s_memtime spans of the step's phases into probe[blockIdx.x][8]; the product has PROBE = false.
constexpr int kRollMwWaves = kRollChunks;  // one layer-2 chain per wave
// mail word not yet published (memset 0xff): a NaN bit pattern no f64 partial sum of the
// policy's finite weights and activations produces
constexpr unsigned long long kMailEmpty = ~0ull;
// MZ: MazeArgs for ENV 2, else empty (EnvState::step); every thread of every part reads the same
// one.
template <int ENV, bool PROBE = false, int GOAL = kGoalNone, typename... MZ>
__global__ __launch_bounds__(64 * kRollMwWaves) void rollout_mlp_mw_kernel(
    const double* __restrict__ W1, const double* __restrict__ b1, int h0,
    const double* __restrict__ W2t, const double* __restrict__ b2, int h1,
    const double* __restrict__ Wm, const double* __restrict__ bm,
    const double* __restrict__ log_std, int a_dim, const double* __restrict__ init64,
    const float* __restrict__ init32, const double* __restrict__ noise, int64_t n, int64_t T,
    float* __restrict__ states_rec, float* __restrict__ actions_rec,
    double* __restrict__ visited, double* __restrict__ final_state, int np, int nw,
    unsigned long long* __restrict__ mail, int* __restrict__ err, int* __restrict__ ticket,
    long long* __restrict__ probe, GoalArgs goal, MZ... mz) {
  static_assert(GOAL != kGoalBall || ENV != 0, "the ball goal needs an f32-state env");
  extern __shared__ double sW2[];  // [h0][64]: W2^T rows, this part's 64 columns
  __shared__ double sh1[kRollMaxH];
  __shared__ double spart[kRollMwWaves][64];
  __shared__ double sword[64];
  __shared__ int sbad;
  long long pr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt = 0;
  auto stamp = [&](int k, double dep) {
    if constexpr (PROBE) {
      // readfirstlane waits for dep's VALU result, so the stamp follows the phase's work
      const int sink = __builtin_amdgcn_readfirstlane(__double2hiint(dep));
      const long long now = (long long)__builtin_amdgcn_s_memtime();
      if (k >= 0) pr[k] += now - pt;
      pr[7] += sink & 1;
      pt = now;
    }
  };
  // (trajectory, part) from a dispatch-order ticket, not from blockIdx: when a workgroup takes
  // ticket t, every ticket below t is held by a running workgroup, so the parts a workgroup
  // waits for are either running or next in line for a free slot.  With the whole grid
  // resident (the host's occupancy check) all parts run at once; with fewer slots (another
  // kernel on the CUs) complete trajectories still finish and free theirs: no deadlock without
  // a cooperative launch.
  // GOAL: every part steps the same env state, so all parts of a trajectory see the hit at the
  // same step t.  A part leaves only below, after it has published its own mail word of step t
  // and read every part's word of step t (it needs them for the action that caused the hit), so
  // no peer ever waits for a word that will not be written; leaving early only frees its slot
  // sooner for the tickets behind it.
  // That rests on every part taking the `break` at the same step: a part that left a step
  // before its peers would leave them polling a word it never writes, which is a hang (bounded
  // by the spin limit: err = 1), not a wrong number.  It holds for both envs and both goal
  // kinds because every thread of every part computes the hit itself, from its own copy of the
  // state (its own EnvState), never from a flag another part wrote, and the copies are the same
  // bits: each is stepped by the same instruction sequence (MountainCar::step, its cos()
  // included, or GridWorld::step) on the same action, the part-ordered sum of the same mail
  // words.  Keep the env step and the hit test free of anything that differs between parts.
  // (The maze's walls are a kernel argument: the same bytes in every part.)
  __shared__ int sticket;
  if (threadIdx.x == 0) sticket = atomicAdd(ticket, 1);
  __syncthreads();
  const int64_t i = sticket / np;
  const int p = sticket % np;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = 64 * p + lane;
  const bool c1 = j < h1;
  for (int k = wv; k < h0; k += kRollMwWaves)
    sW2[k * 64 + lane] = c1 ? W2t[(int64_t)k * h1 + j] : 0.0;
  // this wave's rows of the layer-2 sum (wave-uniform)
  const int L = (h0 + kRollMwWaves - 1) / kRollMwWaves;
  const int kb = min(wv * L, h0), len = min(kb + L, h0) - kb;
  constexpr int kU1 = kRollMaxH / (64 * kRollMwWaves);  // layer-1 columns per thread
  double w1a[kU1], w1b[kU1], bb1[kU1];
#pragma unroll
  for (int u = 0; u < kU1; ++u) {
    const int c = tid + 64 * kRollMwWaves * u;
    const bool ok = c < h0;
    w1a[u] = ok ? W1[2 * c] : 0.0;
    w1b[u] = ok ? W1[2 * c + 1] : 0.0;
    bb1[u] = ok ? b1[c] : 0.0;
  }
  const double bb2 = c1 ? b2[j] : 0.0;
  double wm[kRollMaxA], sd[kRollMaxA], nz[kRollMaxA], bmv[kRollMaxA];
#pragma unroll
  for (int a = 0; a < kRollMaxA; ++a) {
    wm[a] = (c1 && a < a_dim) ? Wm[a * h1 + j] : 0.0;
    bmv[a] = a < a_dim ? bm[a] : 0.0;
    sd[a] = a < a_dim ? exp(log_std[a]) : 0.0;
    nz[a] = a < a_dim ? noise[i * a_dim + a] : 0.0;
  }
  // env state, stepped identically by every thread of every part of the trajectory
  EnvState<ENV> env;
  env.load(init64, init32, 2 * i);
  double x0 = env.x0(), x1 = env.x1();
  const bool rec = p == 0 && tid == 0;
  if (rec) record_state(states_rec, i, T, -1, x0, x1);
  if (tid == 0) sbad = 0;
  int64_t steps = T;  // GOAL: the episode's length
  bool hit = false;
  __syncthreads();
  if constexpr (PROBE) pr[6] = -(long long)__builtin_amdgcn_s_memrealtime();
  stamp(-1, 0.0);
  for (int64_t t = 0; t < T; ++t) {
    double nz_next[kRollMaxA];
    if (t + 1 < T)
      for (int a = 0; a < a_dim; ++a) nz_next[a] = noise[((t + 1) * n + i) * a_dim + a];
    // layer 1, every column
#pragma unroll
    for (int u = 0; u < kU1; ++u) {
      const int c = tid + 64 * kRollMwWaves * u;
      if (c < h0) sh1[c] = layer1(x0, x1, w1a[u], w1b[u], bb1[u]);
    }
    __syncthreads();
    stamp(0, sh1[lane]);
    // layer 2, this wave's rows of this part's columns: one fma chain in k order; the LDS
    // operands of the next 8 rows are loaded while these 8 are summed (constant offsets from
    // one base: no per-row address arithmetic)
    {
      constexpr int U = 8;
      const double* wp = sW2 + kb * 64 + lane;
      const double* hp = sh1 + kb;
      double acc = 0.0, wc[U], hc[U], wn[U], hn[U];
      int k = 0;
      if (len >= U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          wc[u] = wp[u * 64];
          hc[u] = hp[u];
        }
        for (; k + 2 * U <= len; k += U) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            wn[u] = wp[(k + U + u) * 64];
            hn[u] = hp[k + U + u];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) acc = fma(wc[u], hc[u], acc);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            wc[u] = wn[u];
            hc[u] = hn[u];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fma(wc[u], hc[u], acc);
        k += U;
      }
      // the last < U rows: all loads issued, then the chain (one LDS round trip, not one per row)
#pragma unroll
      for (int u = 0; u < U - 1; ++u)
        if (k + u < len) {
          wc[u] = wp[(k + u) * 64];
          hc[u] = hp[k + u];
        }
#pragma unroll
      for (int u = 0; u < U - 1; ++u)
        if (k + u < len) acc = fma(wc[u], hc[u], acc);
      spart[wv][lane] = acc;
    }
    __syncthreads();
    unsigned long long* slot = mail + (i * T + t) * np * a_dim;
    if (wv == 0) {
      double s = spart[0][lane];
#pragma unroll
      for (int w = 1; w < kRollMwWaves; ++w) s += spart[w][lane];
      const double h2 = c1 ? fmax(s + bb2, 0.0) : 0.0;
      stamp(1, h2);
      // mean layer: this part's partial over its 64 columns (wave_sum), lane 0's, to this
      // step's own mail words (pre-filled with kMailEmpty, which no partial can equal: each word
      // validates itself, no flag)
#pragma unroll
      for (int a = 0; a < kRollMaxA; ++a) {
        if (a < a_dim) {
          const double q = wave_sum(wm[a] * h2);
          if (lane == 0)
            __hip_atomic_store(slot + p * a_dim + a, __double_as_longlong(q), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      stamp(2, 0.0);
      // every part's partials of this step: lane l < np a_dim polls word l (part l / a_dim,
      // action l % a_dim) with sc1 loads until it is published
      const int nword = np * a_dim;
      unsigned spins = 0;
      unsigned long long v = 0;
      while (true) {
        if (lane < nword)
          v = __hip_atomic_load(slot + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!__ballot(lane < nword && v == kMailEmpty)) break;
        if (++spins > (1u << 24)) {
          if (lane == 0) {
            atomicExch(err, 1);
            sbad = 1;
          }
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if constexpr (PROBE) pr[5] += spins;
      sword[lane] = __longlong_as_double(v);
      stamp(3, sword[lane]);
    }
    __syncthreads();
    if (sbad) return;  // workgroup-uniform: every wave leaves together
    double act[kRollMaxA];
    for (int a = 0; a < a_dim; ++a) {
      // the parts' words loaded together, then summed in part order
      constexpr int kMaxP = kRollMaxH / 64;
      double wq[kMaxP];
#pragma unroll
      for (int q = 0; q < kMaxP; ++q)
        if (q < np) wq[q] = sword[q * a_dim + a];
      double mu = wq[0];
#pragma unroll
      for (int q = 1; q < kMaxP; ++q)
        if (q < np) mu += wq[q];
      for (int q = np; q < nw; ++q) mu += 0.0;  // rollout_mlp_kernel's waves without columns
      mu += bmv[a];
      act[a] = gaussian_action(mu, nz[a], sd[a]);
      if (rec) actions_rec[(i * T + t) * a_dim + a] = (float)act[a];
    }
    if (t + 1 < T)
      for (int a = 0; a < a_dim; ++a) nz[a] = nz_next[a];
    env.step(act, mz...);
    x0 = env.x0();
    x1 = env.x1();
    if (rec) {
      record_state(states_rec, i, T, t, x0, x1);
      record_visited(visited, i, T, t, x0, x1);
    }
    stamp(4, x0);
    if constexpr (GOAL != kGoalNone) {
      // the same value in every thread of every part
      hit = env.template hit<GOAL>(goal);
      if (rec) goal.rewards[i * T + t] = hit ? 1.f : 0.f;
      if (hit) {
        steps = t + 1;
        break;
      }
    }
  }
  if (rec && final_state) record_final(final_state, 2 * i, x0, x1);
  if constexpr (GOAL != kGoalNone) {
    if (rec) {
      goal.len[i] = (int)steps;
      goal.done[i] = hit ? 1 : 0;
    }
    if (p == 0)
      goal_zero_tail(i, steps, T, a_dim, states_rec, actions_rec, goal.rewards, tid,
                     64 * kRollMwWaves);
  }
  if constexpr (PROBE) {
    pr[6] += (long long)__builtin_amdgcn_s_memrealtime();
    if (tid < 8) {
      long long v = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) v = tid == k ? pr[k] : v;
      probe[blockIdx.x * 8 + tid] = v;
    }
  }
}
}  // namespace envs
}  // namespace mepol

using namespace mepol;
using namespace mepol::envs;

extern "C" int mepol_step_mountaincar(double* state, const double* action, int64_t n,
                                      int64_t action_stride, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(step_mc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, state, action, n, action_stride);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

extern "C" int mepol_step_gridworld(float* state, const double* action, int64_t n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(step_gw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, state, action, n);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

// env_id: 0 = MountainCar (env_f64 state), 1 = GridWorld (env_f32 state).
extern "C" int mepol_rollout_step(int env_id, double* env_f64, float* env_f32, const double* mean,
                                  const double* noise, const double* log_std, int64_t n, int a_dim,
                                  int64_t t, int64_t T, float* states_rec, float* actions_rec,
                                  double* policy_in, void* stream) {
  if (n <= 0) return 0;
  if (a_dim <= 0 || a_dim > 8 || t < 0 || t >= T || (env_id == 0 && !env_f64) ||
      (env_id == 1 && (!env_f32 || a_dim != 2)) || env_id < 0 || env_id > 1) {
    set_error("mepol_rollout_step: bad arguments (env %d, a_dim %d, t %lld)", env_id, a_dim,
              (long long)t);
    return kErrBadArg;
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 g((unsigned)((n + 255) / 256));
  if (env_id == 0)
    hipLaunchKernelGGL(rollout_step_kernel<0>, g, dim3(256), 0, st, env_f64, env_f32, mean, noise,
                       log_std, n, a_dim, t, T, states_rec, actions_rec, policy_in);
  else
    hipLaunchKernelGGL(rollout_step_kernel<1>, g, dim3(256), 0, st, env_f64, env_f32, mean, noise,
                       log_std, n, a_dim, t, T, states_rec, actions_rec, policy_in);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

// env_id 0 = MountainCar (init64 [n,2] f64), 1 = GridWorld (init32 [n,2] f32).  The policy is
// nf = 2 -> [h0, h1] -> a_dim with ReLU: W1 [h0,2], b1, W2t = W2^T [h0,h1], b2, Wm [a,h1], bm,
// log_std [a]; noise [T,n,a_dim] f64.  Writes states_rec [n,T+1,2] f32, actions_rec [n,T,a] f32,
// visited [n,T,2] f64 (nullable), final_state [n,2] f64 (nullable).
// Workspace: word 0 = error flag (zeroed by every call that gets a workspace), then for the
// multi-workgroup form the mail [n][T][np][a_dim] 8-byte words (kMailEmpty).
static size_t rollout_mw_bytes(int64_t n, int64_t T, int h1, int a_dim) {
  const int64_t np = (h1 + 63) / 64;
  return 256 + (size_t)n * T * np * a_dim * 8;
}
// [h0][64] f64 slice (dynamic) + sh1, spart, sword (static, 6.5 KB) within 160 KB of LDS
static constexpr int kRollMwMaxH0 = 306;

// The multi-workgroup form's parts exchange partial sums every step.  Its workgroups take
// (trajectory, part) from a dispatch-order ticket (see the kernel), which makes the exchange
// deadlock-free whenever a trajectory's np parts fit on the device; it is chosen only when the
// occupancy of the kernel at this LDS size times the CU count holds the whole grid (all parts
// in flight at once).  Otherwise the one-workgroup form runs, which sums in the same order and
// so gives the same bits.  (Round 4 used hipLaunchCooperativeKernel for the co-residency; its
// dedicated queue crashed the process at exit under rocprofv3: HIP's teardown of that queue
// faulted inside libhsa-runtime64 after the profiler had shut its queue interception down,
// profiles/r5/rollout_exit_crash.txt.)
// The occupancy asked is that of the instance that will run, env x goal kind: each has its own
// register count.  The maze (env 2) takes no LDS (its description is a kernel argument), so the
// LDS sizes here and the KL budget of the one-workgroup form are those of the other envs.
static int rollout_use_mw(int env_id, int64_t n, int h0, int h1, int a_dim, int goal) {
  const int np = (h1 + 63) / 64;
  const char* mw = getenv("MEPOL_ROLLOUT_MW");
  if (h0 > kRollMwMaxH0 || np * a_dim > 64 || (mw && mw[0] == '0')) return 0;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  const size_t lds = (size_t)h0 * 64 * sizeof(double);
  // the instance's workgroups per CU at this dynamic LDS size; 0 on any error
  int per_cu = 0;
  const MazeArgs type_only{};  // (the query reads no maze)
  rollout_instance(env_id, goal, &type_only, [&](auto E, auto G, const auto&... m) {
    constexpr auto kernel = rollout_mlp_mw_kernel<E(), false, G(), std::decay_t<decltype(m)>...>;
    MEPOL_HIP((max_dynamic_lds<kernel>(kRollMwMaxH0 * 64 * (int)sizeof(double))));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * kRollMwWaves, lds) !=
        hipSuccess) {
      (void)hipGetLastError();
      per_cu = 0;
    }
    return 0;
  });
  return per_cu > 0 && n * np <= (int64_t)per_cu * cus;
}

// The answers of the four *_plan_info and *_workspace_size families behind their own argument
// checks: the form the (env, kind) instance's occupancy gives, and the workspace of that form.
static int rollout_plan_info(int env_id, int kind, int64_t n, int h0, int h1, int a_dim,
                             int* workgroups_per_traj, int* k_chunks) {
  const int mw = rollout_use_mw(env_id, n, h0, h1, a_dim, kind);
  *workgroups_per_traj = mw ? (h1 + 63) / 64 : 1;
  *k_chunks = kRollChunks;  // both forms
  return 0;
}

static int rollout_workspace_size(int env_id, int kind, int64_t n, int64_t T, int h0, int h1,
                                  int a_dim, size_t* bytes) {
  // the mail only when the multi-workgroup form would run; the error word always
  *bytes = (n > 0 && rollout_use_mw(env_id, n, h0, h1, a_dim, kind))
               ? rollout_mw_bytes(n, T, h1, a_dim)
               : 256;
  return 0;
}

extern "C" int mepol_rollout_mlp_plan_info(int64_t n, int h0, int h1, int a_dim,
                                           int* workgroups_per_traj, int* k_chunks) {
  if (n <= 0 || h0 <= 0 || h1 <= 0 || h0 > kRollMaxH || h1 > kRollMaxH || a_dim <= 0 ||
      a_dim > kRollMaxA || !workgroups_per_traj || !k_chunks) {
    set_error("mepol_rollout_mlp_plan_info: bad arguments");
    return kErrBadArg;
  }
  // (GridWorld and MountainCar kernels have the same resources: env 1 stands for both)
  return rollout_plan_info(1, kGoalNone, n, h0, h1, a_dim, workgroups_per_traj, k_chunks);
}

extern "C" int mepol_rollout_mlp_workspace_size(int64_t n, int64_t T, int h0, int h1, int a_dim,
                                                size_t* bytes) {
  if (n < 0 || T < 0 || h0 <= 0 || h1 <= 0 || a_dim <= 0 || a_dim > kRollMaxA || !bytes) {
    set_error("mepol_rollout_mlp_workspace_size: bad arguments");
    return kErrBadArg;
  }
  return rollout_workspace_size(1, kGoalNone, n, T, h0, h1, a_dim, bytes);
}

// mepol_rollout_mlp_plan_info for mepol_rollout_goal: the goal-mode instance's own occupancy
// decides its form.
extern "C" int mepol_rollout_goal_plan_info(int64_t n, int h0, int h1, int a_dim,
                                            int* workgroups_per_traj, int* k_chunks) {
  if (n <= 0 || h0 <= 0 || h1 <= 0 || h0 > kRollMaxH || h1 > kRollMaxH || a_dim != 2 ||
      !workgroups_per_traj || !k_chunks) {
    set_error("mepol_rollout_goal_plan_info: bad arguments");
    return kErrBadArg;
  }
  return rollout_plan_info(1, kGoalBall, n, h0, h1, a_dim, workgroups_per_traj, k_chunks);
}

// mepol_rollout_mlp (kind kGoalNone, ga unused), mepol_rollout_goal (kGoalBall, env 1) and
// mepol_rollout_goal_threshold (kGoalThreshold) behind their argument checks: the same choice of
// form, workspace layout and launches, the kernels' GOAL instances for the last two.
// env_id 2 (mepol_rollout_maze, any kind): the ENV = 2 instances with *mz, already validated.
static int rollout_mlp_run(int env_id, int kind, const GoalArgs& ga, const double* W1,
                           const double* b1, int h0, const double* W2t, const double* b2, int h1,
                           const double* Wm, const double* bm, const double* log_std, int a_dim,
                           const double* init64, const float* init32, const double* noise,
                           int64_t n, int64_t T, float* states_rec, float* actions_rec,
                           double* visited, double* final_state, void* workspace,
                           size_t workspace_bytes, void* stream, const MazeArgs* mz = nullptr) {
  const int threads = ((h0 > h1 ? h0 : h1) + 63) / 64 * 64;
  hipStream_t st = (hipStream_t)stream;
  int* err = (int*)workspace;
  if (err) MEPOL_HIP(hipMemsetAsync(err, 0, sizeof(int), st));  // whichever form runs
  {
    // several workgroups per trajectory when all of them can be resident at once
    const int np = (h1 + 63) / 64, nw = threads / 64;
    if (workspace && workspace_bytes >= rollout_mw_bytes(n, T, h1, a_dim) &&
        rollout_use_mw(env_id, n, h0, h1, a_dim, kind)) {
      unsigned long long* mail = (unsigned long long*)((char*)workspace + 256);
      int* ticket = err + 1;  // word 1 of the 256-byte header: the dispatch-order counter
      MEPOL_HIP(hipMemsetAsync(ticket, 0, sizeof(int), st));
      // every mail word starts as kMailEmpty (all ones)
      MEPOL_HIP(hipMemsetAsync(mail, 0xff, (size_t)n * T * np * a_dim * 8, st));
      const int e = rollout_instance(env_id, kind, mz, [&](auto E, auto G, const auto&... m) {
        long long* probe = nullptr;
        hipLaunchKernelGGL(
            (rollout_mlp_mw_kernel<E(), false, G(), std::decay_t<decltype(m)>...>),
            dim3((unsigned)(n * np)), dim3(64 * kRollMwWaves),
            (unsigned)((size_t)h0 * 64 * sizeof(double)), st, W1, b1, h0, W2t, b2, h1, Wm, bm,
            log_std, a_dim, init64, init32, noise, n, T, states_rec, actions_rec, visited,
            final_state, np, nw, mail, err, ticket, probe, ga, m...);
        return (int)hipGetLastError();
      });
      if (e == 0) return 0;
      (void)hipGetLastError();  // launch refused: the one-workgroup form
    }
  }
  const dim3 g((unsigned)n);
  // W2^T rows kept in LDS, the rest streamed: up to ~150 KB (MEPOL_ROLLOUT_KL caps it)
  const char* klv = getenv("MEPOL_ROLLOUT_KL");
  int KL = (int)((150 * 1024) / ((size_t)threads * sizeof(double)));
  if (klv) KL = std::min(KL, atoi(klv));
  KL = std::max(0, std::min(KL, h0));
  const size_t lds = (size_t)KL * threads * sizeof(double);
  return rollout_instance(env_id, kind, mz, [&](auto E, auto G, const auto&... m) {
    constexpr auto kernel = rollout_mlp_kernel<E(), G(), std::decay_t<decltype(m)>...>;
    MEPOL_HIP((max_dynamic_lds<kernel>(150 * 1024)));
    hipLaunchKernelGGL(kernel, g, dim3(threads), lds, st, W1, b1, h0, W2t, b2, h1, Wm, bm, log_std,
                       a_dim, init64, init32, noise, n, T, states_rec, actions_rec, visited,
                       final_state, KL, ga, m...);
    MEPOL_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int mepol_rollout_mlp(int env_id, const double* W1, const double* b1, int h0,
                                 const double* W2t, const double* b2, int h1, const double* Wm,
                                 const double* bm, const double* log_std, int a_dim,
                                 const double* init64, const float* init32, const double* noise,
                                 int64_t n, int64_t T, float* states_rec, float* actions_rec,
                                 double* visited, double* final_state, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (h0 <= 0 || h1 <= 0 || h0 > kRollMaxH || h1 > kRollMaxH || a_dim <= 0 ||
      a_dim > kRollMaxA || env_id < 0 || env_id > 1 || (env_id == 0 && !init64) ||
      (env_id == 1 && (!init32 || a_dim != 2)) || !W1 || !b1 || !W2t || !b2 || !Wm || !bm ||
      !log_std || !noise || !states_rec || !actions_rec ||
      (workspace && workspace_bytes < sizeof(int))) {
    set_error("mepol_rollout_mlp: bad arguments (hidden <= %d, a_dim <= %d)", kRollMaxH,
              kRollMaxA);
    return kErrBadArg;
  }
  return rollout_mlp_run(env_id, kGoalNone, GoalArgs{}, W1, b1, h0, W2t, b2, h1, Wm, bm, log_std,
                         a_dim, init64, init32, noise, n, T, states_rec, actions_rec, visited,
                         final_state, workspace, workspace_bytes, stream);
}

// The goal-mode workspace: the same layout as mepol_rollout_mlp's, sized by the goal-mode
// kernel's own occupancy.
extern "C" int mepol_rollout_goal_workspace_size(int env_id, int64_t n, int64_t T, int h0, int h1,
                                                 int a_dim, size_t* bytes) {
  if (n < 0 || T < 0 || h0 <= 0 || h1 <= 0 || a_dim <= 0 || a_dim > kRollMaxA || env_id < 0 ||
      env_id > 1 || !bytes) {
    set_error("mepol_rollout_goal_workspace_size: bad arguments");
    return kErrBadArg;
  }
  if (env_id != 1) {
    set_error("mepol_rollout_goal: only GridWorld (env_id 1) has a goal mode");
    return kErrUnsupported;
  }
  return rollout_workspace_size(1, kGoalBall, n, T, h0, h1, a_dim, bytes);
}

extern "C" int mepol_rollout_goal(int env_id, const double* W1, const double* b1, int h0,
                                  const double* W2t, const double* b2, int h1, const double* Wm,
                                  const double* bm, const double* log_std, int a_dim,
                                  const float* init32, const double* noise, int64_t n, int64_t T,
                                  float goal_x, float goal_y, double radius, float* states_rec,
                                  float* actions_rec, float* rewards_rec, int32_t* len_out,
                                  int32_t* done_out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (env_id < 0 || env_id > 1 || h0 <= 0 || h1 <= 0 || h0 > kRollMaxH || h1 > kRollMaxH ||
      a_dim != 2 || T > INT32_MAX || !init32 || !W1 || !b1 || !W2t || !b2 || !Wm || !bm ||
      !log_std || !noise || !states_rec || !actions_rec || !rewards_rec || !len_out ||
      !done_out || !(goal_x == goal_x) || !(goal_y == goal_y) || !(radius >= 0.0) ||
      (workspace && workspace_bytes < sizeof(int))) {
    set_error("mepol_rollout_goal: bad arguments (hidden <= %d, a_dim = 2, radius >= 0)",
              kRollMaxH);
    return kErrBadArg;
  }
  if (env_id != 1) {
    set_error("mepol_rollout_goal: only GridWorld (env_id 1) has a goal mode");
    return kErrUnsupported;
  }
  const GoalArgs goal{{goal_x}, goal_y, {radius}, rewards_rec, len_out, done_out};
  return rollout_mlp_run(1, kGoalBall, goal, W1, b1, h0, W2t, b2, h1, Wm, bm, log_std, a_dim,
                         nullptr, init32, noise, n, T, states_rec, actions_rec, nullptr, nullptr,
                         workspace, workspace_bytes, stream);
}

// ---- threshold goals (either env) -------------------------------------------------------------
// The shape and env checks the three mepol_rollout_goal_threshold* entry points share: the limits
// of mepol_rollout_mlp, and the env's own action count.
static bool threshold_shape_ok(int env_id, int h0, int h1, int a_dim) {
  return env_id >= 0 && env_id <= 1 && h0 > 0 && h1 > 0 && h0 <= kRollMaxH && h1 <= kRollMaxH &&
         a_dim == (env_id == 0 ? 1 : 2);
}

extern "C" int mepol_rollout_goal_threshold_plan_info(int env_id, int64_t n, int h0, int h1,
                                                      int a_dim, int* workgroups_per_traj,
                                                      int* k_chunks) {
  if (n <= 0 || !threshold_shape_ok(env_id, h0, h1, a_dim) || !workgroups_per_traj || !k_chunks) {
    set_error("mepol_rollout_goal_threshold_plan_info: bad arguments (env 0 with a_dim = 1 or "
              "env 1 with a_dim = 2, hidden <= %d)", kRollMaxH);
    return kErrBadArg;
  }
  return rollout_plan_info(env_id, kGoalThreshold, n, h0, h1, a_dim, workgroups_per_traj,
                           k_chunks);
}

extern "C" int mepol_rollout_goal_threshold_workspace_size(int env_id, int64_t n, int64_t T,
                                                           int h0, int h1, int a_dim,
                                                           size_t* bytes) {
  if (n < 0 || T < 0 || !threshold_shape_ok(env_id, h0, h1, a_dim) || !bytes) {
    set_error("mepol_rollout_goal_threshold_workspace_size: bad arguments (env 0 with a_dim = 1 "
              "or env 1 with a_dim = 2, hidden <= %d)", kRollMaxH);
    return kErrBadArg;
  }
  return rollout_workspace_size(env_id, kGoalThreshold, n, T, h0, h1, a_dim, bytes);
}

extern "C" int mepol_rollout_goal_threshold(
    int env_id, const double* W1, const double* b1, int h0, const double* W2t, const double* b2,
    int h1, const double* Wm, const double* bm, const double* log_std, int a_dim,
    const double* init64, const float* init32, const double* noise, int64_t n, int64_t T,
    int coord, double threshold, float* states_rec, float* actions_rec, float* rewards_rec,
    int32_t* len_out, int32_t* done_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (!threshold_shape_ok(env_id, h0, h1, a_dim) || T > INT32_MAX || (env_id == 0 && !init64) ||
      (env_id == 1 && !init32) || !W1 || !b1 || !W2t || !b2 || !Wm || !bm || !log_std || !noise ||
      !states_rec || !actions_rec || !rewards_rec || !len_out || !done_out ||
      (coord != 0 && coord != 1) || threshold != threshold ||
      (workspace && workspace_bytes < sizeof(int))) {
    set_error("mepol_rollout_goal_threshold: bad arguments (env 0 with a_dim = 1 and init64 or "
              "env 1 with a_dim = 2 and init32, hidden <= %d, coord 0 or 1, threshold not NaN, "
              "no null pointers)", kRollMaxH);
    return kErrBadArg;
  }
  const GoalArgs goal = threshold_goal(coord, threshold, rewards_rec, len_out, done_out);
  return rollout_mlp_run(env_id, kGoalThreshold, goal, W1, b1, h0, W2t, b2, h1, Wm, bm, log_std,
                         a_dim, init64, init32, noise, n, T, states_rec, actions_rec, nullptr,
                         nullptr, workspace, workspace_bytes, stream);
}

// ---- box mazes (env 2) -------------------------------------------------------------------------
// The env_id 1 entry points above folded by goal kind (include/mepol_amd.h): the ENV = 2 instances
// behind the same argument checks plus maze_args_ok.
extern "C" int mepol_step_maze(const mepol_maze* maze, float* state, const double* action,
                               int64_t n, void* stream) {
  if (!maze_args_ok(maze, "mepol_step_maze")) return kErrBadArg;
  if (n <= 0) return 0;
  if (!state || !action) {
    set_error("mepol_step_maze: null state or action");
    return kErrBadArg;
  }
  hipLaunchKernelGGL(step_maze_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, state, action, n, *maze);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

extern "C" int mepol_rollout_step_maze(const mepol_maze* maze, float* env_f32, const double* mean,
                                       const double* noise, const double* log_std, int64_t n,
                                       int a_dim, int64_t t, int64_t T, float* states_rec,
                                       float* actions_rec, double* policy_in, void* stream) {
  if (!maze_args_ok(maze, "mepol_rollout_step_maze")) return kErrBadArg;
  if (a_dim != 2 || t < 0 || t >= T || !env_f32 || !mean || !noise || !log_std || !states_rec ||
      !actions_rec || !policy_in) {
    set_error("mepol_rollout_step_maze: bad arguments (a_dim %d must be 2, t %lld in [0, T), no "
              "null pointers)", a_dim, (long long)t);
    return kErrBadArg;
  }
  if (n <= 0) return 0;
  double* env_f64 = nullptr;
  hipLaunchKernelGGL((rollout_step_kernel<2, MazeArgs>), dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, env_f64, env_f32, mean, noise, log_std, n,
                     a_dim, t, T, states_rec, actions_rec, policy_in, *maze);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

static bool maze_shape_ok(int goal_kind, int h0, int h1, int a_dim) {
  return goal_kind_ok(goal_kind) && h0 > 0 && h1 > 0 && h0 <= kRollMaxH && h1 <= kRollMaxH &&
         a_dim == 2;
}

extern "C" int mepol_rollout_maze_plan_info(int goal_kind, int64_t n, int h0, int h1, int a_dim,
                                            int* workgroups_per_traj, int* k_chunks) {
  if (n <= 0 || !maze_shape_ok(goal_kind, h0, h1, a_dim) || !workgroups_per_traj || !k_chunks) {
    set_error("mepol_rollout_maze_plan_info: bad arguments (goal kind 0 .. 2, a_dim = 2, hidden "
              "<= %d)", kRollMaxH);
    return kErrBadArg;
  }
  return rollout_plan_info(2, goal_kind, n, h0, h1, a_dim, workgroups_per_traj, k_chunks);
}

extern "C" int mepol_rollout_maze_workspace_size(int goal_kind, int64_t n, int64_t T, int h0,
                                                 int h1, int a_dim, size_t* bytes) {
  if (n < 0 || T < 0 || !maze_shape_ok(goal_kind, h0, h1, a_dim) || !bytes) {
    set_error("mepol_rollout_maze_workspace_size: bad arguments (goal kind 0 .. 2, a_dim = 2, "
              "hidden <= %d)", kRollMaxH);
    return kErrBadArg;
  }
  return rollout_workspace_size(2, goal_kind, n, T, h0, h1, a_dim, bytes);
}

extern "C" int mepol_rollout_maze(const mepol_maze* maze, int goal_kind, const double* W1,
                                  const double* b1, int h0, const double* W2t, const double* b2,
                                  int h1, const double* Wm, const double* bm,
                                  const double* log_std, int a_dim, const float* init32,
                                  const double* noise, int64_t n, int64_t T, float goal_x,
                                  float goal_y, int coord, double goal_value, float* states_rec,
                                  float* actions_rec, double* visited, double* final_state,
                                  float* rewards_rec, int32_t* len_out, int32_t* done_out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!maze_args_ok(maze, "mepol_rollout_maze")) return kErrBadArg;
  GoalArgs goal;
  const bool goal_ok = goal_from_kind(goal_kind, goal_x, goal_y, coord, goal_value, T, rewards_rec,
                                      len_out, done_out, &goal);
  if (!maze_shape_ok(goal_kind, h0, h1, a_dim) || !goal_ok || !init32 || !W1 || !b1 || !W2t ||
      !b2 || !Wm || !bm || !log_std || !noise || !states_rec || !actions_rec ||
      (workspace && workspace_bytes < sizeof(int))) {
    set_error("mepol_rollout_maze: bad arguments (goal kind 0 .. 2, hidden <= %d, a_dim = 2; "
              "ball: radius >= 0; threshold: coord 0 or 1, threshold not NaN; no null pointers)",
              kRollMaxH);
    return kErrBadArg;
  }
  if (n <= 0 || T <= 0) return 0;
  return rollout_mlp_run(2, goal_kind, goal, W1, b1, h0, W2t, b2, h1, Wm, bm, log_std, a_dim,
                         nullptr, init32, noise, n, T, states_rec, actions_rec, visited,
                         final_state, workspace, workspace_bytes, stream, maze);
}
