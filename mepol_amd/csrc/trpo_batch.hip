// TRPO's batch processing between the rollout and the policy step (src/algorithms/trpo.py):
//
//  traj_budget   the `steps == batch_size` rule of collect_sample_batch (:98-140) applied to a batch
//                that was rolled out in parallel: trajectories are taken in index order until the
//                step budget is spent, the last one cut.  Integer arithmetic: any scan order gives
//                the same result.
//  traj_cut      the episodes inside un-terminated rollouts: each trajectory is cut at the first
//                step whose state a batched reward marked done, with the GOAL instances' zeros
//                behind the end (goal_mode.hpp), so that any reward of the reached state samples
//                on the one-launch rollouts.
//  gae          process_traj (:175-201) over ragged trajectories plus the concatenation of
//                :308-326: discounted targets, GAE advantages and the packed f64 states / actions.
//                The two recurrences run backwards in f64, one lane per trajectory, every operation
//                rounded on its own (_rn intrinsics: no contraction) in the reference's operator
//                order, so a sequential numpy f64 loop reproduces them bit for bit.
//  standardize   (x - mean) / std of :331 (population std), two passes through fixed-order block
//                partials (reduce.hpp): the same bits on every call.
#include <climits>

#include "common.hpp"
#include "reduce.hpp"

namespace mepol {
namespace trpo {

// ---- step budget ---------------------------------------------------------------------------
constexpr int kBudgetThreads = 256;
constexpr int64_t kBudgetMaxTraj = 65536;

// One workgroup; thread j owns trajectories [j c, j c + c), c = ceil(n / 256).
__global__ __launch_bounds__(kBudgetThreads) void traj_budget_kernel(
    const int* __restrict__ len, const int* __restrict__ done, int n, long long budget,
    int* __restrict__ len_out, int* __restrict__ done_out, long long* __restrict__ offsets,
    long long* __restrict__ meta) {
  __shared__ long long ssum[kBudgetThreads];
  __shared__ int sused[kBudgetThreads];
  const int tid = threadIdx.x, c = (n + kBudgetThreads - 1) / kBudgetThreads;
  const int lo = min(tid * c, n), hi = min(lo + c, n);
  long long s = 0;
  for (int i = lo; i < hi; ++i) s += max(len[i], 0);
  ssum[tid] = s;
  __syncthreads();
  if (tid == 0) {  // exclusive scan of the 256 chunk sums
    long long run = 0;
    for (int k = 0; k < kBudgetThreads; ++k) {
      const long long t = ssum[k];
      ssum[k] = run;
      run += t;
    }
    const long long kept = min(run, budget);
    offsets[n] = kept;
    meta[1] = kept;
  }
  __syncthreads();
  long long pre = ssum[tid];
  int used = 0;
  for (int i = lo; i < hi; ++i) {
    const long long L = max(len[i], 0);
    const bool in = pre < budget;  // still below the budget when this trajectory starts
    const long long keep = in ? min(L, budget - pre) : 0;
    offsets[i] = min(pre, budget);
    len_out[i] = (int)keep;
    done_out[i] = (in && done[i] != 0 && keep == L) ? 1 : 0;  // a cut trajectory is not done
    used += in ? 1 : 0;
    pre += L;
  }
  sused[tid] = used;
  __syncthreads();
  if (tid == 0) {
    long long m = 0;
    for (int k = 0; k < kBudgetThreads; ++k) m += sused[k];
    meta[0] = m;
  }
}

// ---- cut at the first done -----------------------------------------------------------------
// One workgroup per trajectory (a grid-stride loop beyond kCutMaxBlocks of them).  Thread tid
// scans steps tid, tid + 256, ... for its first non-zero done_step byte; the minimum over the
// workgroup (the wave's xor butterfly, then the 4 waves through LDS: integers, any order) is the
// episode's last step f, and all threads zero the three tails behind len = f + 1 with coalesced
// stores, as goal_zero_tail (goal_mode.hpp) does for the GOAL instances.  Nothing in front of the
// end is written, so kept rewards keep their bits.
constexpr int kCutThreads = 256;
constexpr int64_t kCutMaxBlocks = 1 << 20;

__global__ __launch_bounds__(kCutThreads) void traj_cut_kernel(
    const uint8_t* __restrict__ done_step, int64_t n, int64_t T, float* __restrict__ rewards,
    float* __restrict__ states_rec, int nf, float* __restrict__ actions_rec, int a_dim,
    int* __restrict__ len, int* __restrict__ done) {
  __shared__ int sfirst[kCutThreads / kWave];
  const int tid = threadIdx.x;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint8_t* d = done_step + i * T;
    int64_t first = T;  // T <= INT_MAX - 1
    for (int64_t t = tid; t < T; t += kCutThreads) {
      if (d[t] != 0) {
        first = t;
        break;
      }
    }
    int f = (int)first;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) f = min(f, __shfl_xor(f, m, kWave));
    if (lane_id() == 0) sfirst[tid / kWave] = f;
    __syncthreads();
    f = min(min(sfirst[0], sfirst[1]), min(sfirst[2], sfirst[3]));
    __syncthreads();  // sfirst is rewritten by the next trajectory of this workgroup
    const bool hit = f < T;
    const int64_t L = hit ? (int64_t)f + 1 : T;
    if (tid == 0) {
      len[i] = (int)L;
      done[i] = hit ? 1 : 0;
    }
    const int64_t rest = T - L;  // steps behind the end
    float* s = states_rec + (i * (T + 1) + L + 1) * nf;
    for (int64_t e = tid; e < rest * nf; e += kCutThreads) s[e] = 0.f;
    float* a = actions_rec + (i * T + L) * a_dim;
    for (int64_t e = tid; e < rest * a_dim; e += kCutThreads) a[e] = 0.f;
    float* r = rewards + i * T + L;
    for (int64_t e = tid; e < rest; e += kCutThreads) r[e] = 0.f;
  }
}

// ---- targets, advantages, packing ----------------------------------------------------------
// A workgroup of one wave takes kGaeTraj trajectories.  Steps are staged through LDS in chunks
// of kGaeChunk, last chunk first: the wave loads one trajectory's 64 values / rewards per
// (coalesced) instruction, lane r < kGaeTraj then runs its trajectory's recurrences over the
// chunk out of LDS and leaves the results there, and the wave writes them, and the chunk's
// states and actions, to the packed arrays with coalesced stores.  No global load depends on the
// step before it.  Rows are padded to kGaeChunk + 1 words: lane r reads row r, bank r + s.
constexpr int kGaeTraj = 16, kGaeChunk = 64, kGaeRow = kGaeChunk + 1;

__global__ __launch_bounds__(kWave) void gae_kernel(
    const float* __restrict__ rewards, const double* __restrict__ values,
    const int* __restrict__ len, const int* __restrict__ done,
    const long long* __restrict__ offsets, int64_t n, int64_t T, int64_t n_out, double gamma,
    double lambd, const float* __restrict__ states_rec, int nf,
    const float* __restrict__ actions_rec, int a_dim, double* __restrict__ targets,
    double* __restrict__ adv, double* __restrict__ states_out, double* __restrict__ actions_out) {
  __shared__ double sv[kGaeTraj][kGaeRow];  // values in, targets out
  __shared__ double sa[kGaeTraj][kGaeRow];  // advantages out
  __shared__ float sr[kGaeTraj][kGaeRow];
  __shared__ int slen[kGaeTraj];
  __shared__ long long soff[kGaeTraj];
  const int lane = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kGaeTraj;
  if (lane < kGaeTraj) {
    const int64_t i = i0 + lane;
    int l = i < n ? len[i] : 0;
    long long o = i < n ? offsets[i] : 0;
    // lengths and offsets are device data the host cannot check: a row whose len is outside
    // [0, T] or whose packed rows [o, o + len) do not lie inside [0, n_out) is skipped, so nothing
    // outside the inputs' [.., T] rows is read and nothing outside the n_out packed rows is
    // written.  n_out - l cannot overflow (both are in [0, 2^63) by then); o + l could.
    if (l < 0 || l > T || o < 0 || o > n_out - l) l = 0;
    slen[lane] = l;
    soff[lane] = o;
  }
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int r = 0; r < kGaeTraj; ++r) maxlen = max(maxlen, slen[r]);
  if (maxlen == 0) return;  // workgroup-uniform
  const bool own = lane < kGaeTraj;
  const int mylen = own ? slen[lane] : 0;
  const int64_t me = i0 + (own ? lane : 0);
  // last state value: null after a termination, bootstrapped otherwise (trpo.py:290-296)
  double boot = 0.0;
  if (mylen > 0 && done[me] == 0) boot = values[me * (T + 1) + mylen];
  const double gl = __dmul_rn(gamma, lambd);
  double c = boot, A = 0.0, vn = boot;
  for (int t0 = (maxlen - 1) / kGaeChunk * kGaeChunk; t0 >= 0; t0 -= kGaeChunk) {
    const int t = t0 + lane;
#pragma unroll 4
    for (int r = 0; r < kGaeTraj; ++r) {
      if (t < slen[r]) {
        sv[r][lane] = values[(i0 + r) * (T + 1) + t];
        sr[r][lane] = rewards[(i0 + r) * T + t];
      }
    }
    __syncthreads();
    if (own) {
      for (int s = min(kGaeChunk, mylen - t0) - 1; s >= 0; --s) {
        const double rw = (double)sr[lane][s], v = sv[lane][s];
        // targets[i] = rewards[i] + gamma * curr_target                       (trpo.py:189)
        c = __dadd_rn(rw, __dmul_rn(gamma, c));
        // advantages[i] = ((rewards[i] + gamma * v_next - vfuncs[i])
        //                  + gamma * lambd * curr_advantage)                   (trpo.py:197-198)
        A = __dadd_rn(__dsub_rn(__dadd_rn(rw, __dmul_rn(gamma, vn)), v), __dmul_rn(gl, A));
        vn = v;
        sv[lane][s] = c;
        sa[lane][s] = A;
      }
    }
    __syncthreads();
    for (int r = 0; r < kGaeTraj; ++r) {
      const int cnt = min(kGaeChunk, slen[r] - t0);  // steps of this chunk in trajectory r
      if (cnt <= 0) continue;
      const int64_t o = soff[r] + t0;
      if (lane < cnt) {
        targets[o + lane] = sv[r][lane];
        adv[o + lane] = sa[r][lane];
      }
      const float* ss = states_rec + ((i0 + r) * (T + 1) + t0) * nf;
      for (int e = lane; e < cnt * nf; e += kWave) states_out[o * nf + e] = (double)ss[e];
      const float* as = actions_rec + ((i0 + r) * T + t0) * a_dim;
      for (int e = lane; e < cnt * a_dim; e += kWave) actions_out[o * a_dim + e] = (double)as[e];
    }
    __syncthreads();
  }
}

// ---- standardisation -----------------------------------------------------------------------
constexpr int kStdThreads = 256, kStdPerBlock = 2048, kStdGroups = 4;
constexpr size_t kStdHeader = 128;  // stats {mean, std} ahead of the block records

inline int64_t std_blocks(int64_t n) { return (n + kStdPerBlock - 1) / kStdPerBlock; }
inline size_t std_ws_bytes(int64_t n) {
  return kStdHeader + sum_records_bytes<kStdGroups>(std_blocks(n), 1);
}

// Block b's record: the sum of x (CENTERED: of (x - mean)^2) over its 2048 elements -- per
// thread in index order (stride 256), the wave's 64 by the xor butterfly, the 4 waves in order.
template <bool CENTERED>
__global__ __launch_bounds__(kStdThreads) void std_partial_kernel(const double* __restrict__ x,
                                                                  int64_t n,
                                                                  const double* __restrict__ stats,
                                                                  double* __restrict__ part) {
  __shared__ double sw[kStdThreads / kWave];
  const int64_t base = (int64_t)blockIdx.x * kStdPerBlock;
  const double mean = CENTERED ? stats[0] : 0.0;
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < kStdPerBlock / kStdThreads; ++u) {
    const int64_t e = base + u * kStdThreads + threadIdx.x;
    if (e < n) {
      const double d = CENTERED ? __dsub_rn(x[e], mean) : x[e];
      s = __dadd_rn(s, CENTERED ? __dmul_rn(d, d) : d);
    }
  }
  s = wave_sum(s);
  if (lane_id() == 0) sw[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

struct ScatterMean {  // stats[0] = sum / n
  double* stats;
  double n;
  __device__ void operator()(int64_t, double t) const { stats[0] = __ddiv_rn(t, n); }
};
struct ScatterStd {  // stats[1] = sqrt(sum / n)
  double* stats;
  double n;
  __device__ void operator()(int64_t, double t) const { stats[1] = __dsqrt_rn(__ddiv_rn(t, n)); }
};

__global__ __launch_bounds__(kStdThreads) void std_apply_kernel(const double* __restrict__ x,
                                                                int64_t n,
                                                                const double* __restrict__ stats,
                                                                double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kStdThreads + threadIdx.x;
  if (e < n) out[e] = __ddiv_rn(__dsub_rn(x[e], stats[0]), stats[1]);
}

}  // namespace trpo
}  // namespace mepol

using namespace mepol;
using namespace mepol::trpo;

extern "C" int mepol_traj_budget(const int32_t* len, const int32_t* done, int64_t n,
                                 int64_t budget, int32_t* len_out, int32_t* done_out,
                                 int64_t* offsets, int64_t* meta, void* stream) {
  if (n <= 0) return 0;
  if (!len || !done || !len_out || !done_out || !offsets || !meta || budget < 0) {
    set_error("mepol_traj_budget: bad arguments (null pointer or negative budget)");
    return kErrBadArg;
  }
  if (n > kBudgetMaxTraj) {
    set_error("mepol_traj_budget: at most %lld trajectories", (long long)kBudgetMaxTraj);
    return kErrUnsupported;
  }
  hipLaunchKernelGGL(traj_budget_kernel, dim3(1), dim3(kBudgetThreads), 0, (hipStream_t)stream,
                     len, done, (int)n, (long long)budget, len_out, done_out, (long long*)offsets,
                     (long long*)meta);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

extern "C" int mepol_traj_cut(const uint8_t* done_step, int64_t n, int64_t T, float* rewards,
                              float* states_rec, int num_features, float* actions_rec, int a_dim,
                              int32_t* len, int32_t* done, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || !done_step || !rewards || !states_rec || !actions_rec || !len || !done || T <= 0 ||
      T > INT_MAX - 1 || num_features <= 0 || a_dim <= 0) {
    set_error("mepol_traj_cut: bad arguments (null pointer, n < 0, T outside [1, 2^31 - 2], "
              "num_features or a_dim < 1)");
    return kErrBadArg;
  }
  const int64_t blocks = n < kCutMaxBlocks ? n : kCutMaxBlocks;
  hipLaunchKernelGGL(traj_cut_kernel, dim3((unsigned)blocks), dim3(kCutThreads), 0,
                     (hipStream_t)stream, done_step, n, T, rewards, states_rec, num_features,
                     actions_rec, a_dim, len, done);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

extern "C" int mepol_gae(const float* rewards, const double* values, const int32_t* len,
                         const int32_t* done, const int64_t* offsets, int64_t n, int64_t T,
                         int64_t n_out, double gamma, double lambd, const float* states_rec,
                         int num_features, const float* actions_rec, int a_dim, double* targets,
                         double* adv, double* states_out, double* actions_out, void* stream) {
  if (n <= 0) return 0;
  // n_out == 0: there is no packed row to write (the kernel's guard skips every trajectory with
  // steps), so the outputs may be null then: an empty tensor has no storage
  const bool outs_ok = n_out == 0 || (targets && adv && states_out && actions_out);
  if (!rewards || !values || !len || !done || !offsets || !states_rec || !actions_rec ||
      !outs_ok || T <= 0 || T > INT_MAX - 1 || n_out < 0 || num_features <= 0 || a_dim <= 0 ||
      !(gamma == gamma) || !(lambd == lambd)) {
    set_error("mepol_gae: bad arguments");
    return kErrBadArg;
  }
  if (n_out == 0) return 0;
  const int64_t blocks = (n + kGaeTraj - 1) / kGaeTraj;
  if (blocks > INT_MAX || num_features > (INT_MAX / kGaeChunk) || a_dim > (INT_MAX / kGaeChunk)) {
    set_error("mepol_gae: batch too large");
    return kErrUnsupported;
  }
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)blocks), dim3(kWave), 0, (hipStream_t)stream,
                     rewards, values, len, done, (const long long*)offsets, n, T, n_out, gamma,
                     lambd, states_rec, num_features, actions_rec, a_dim, targets, adv, states_out,
                     actions_out);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

extern "C" int mepol_standardize_workspace_size(int64_t n, size_t* bytes) {
  if (n < 0 || !bytes) {
    set_error("mepol_standardize_workspace_size: bad arguments");
    return kErrBadArg;
  }
  *bytes = std_ws_bytes(n);
  return 0;
}

extern "C" int mepol_standardize(const double* x, int64_t n, double* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (n <= 0) return 0;
  if (!x || !out || !workspace) {
    set_error("mepol_standardize: bad arguments");
    return kErrBadArg;
  }
  if (std_blocks(n) > INT_MAX) {
    set_error("mepol_standardize: too many elements");
    return kErrUnsupported;
  }
  if (workspace_bytes < std_ws_bytes(n)) {
    set_error("mepol_standardize: workspace too small (%zu < %zu)", workspace_bytes,
              std_ws_bytes(n));
    return kErrWorkspace;
  }
  hipStream_t st = (hipStream_t)stream;
  double* stats = (double*)workspace;
  double* part = (double*)((char*)workspace + kStdHeader);
  const int nb = (int)std_blocks(n);
  hipLaunchKernelGGL(std_partial_kernel<false>, dim3(nb), dim3(kStdThreads), 0, st, x, n, stats,
                     part);
  MEPOL_CHECK_LAUNCH();
  if (int rc = sum_records<kStdGroups>(part, nb, 1, ScatterMean{stats, (double)n}, st)) return rc;
  hipLaunchKernelGGL(std_partial_kernel<true>, dim3(nb), dim3(kStdThreads), 0, st, x, n, stats,
                     part);
  MEPOL_CHECK_LAUNCH();
  if (int rc = sum_records<kStdGroups>(part, nb, 1, ScatterStd{stats, (double)n}, st)) return rc;
  hipLaunchKernelGGL(std_apply_kernel, dim3((unsigned)((n + kStdThreads - 1) / kStdThreads)),
                     dim3(kStdThreads), 0, st, x, n, stats, out);
  MEPOL_CHECK_LAUNCH();
  return 0;
}
