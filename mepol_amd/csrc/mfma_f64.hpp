// Building blocks shared by the f64 matrix-core kernels of the policy network
// (policy_fwd.hip, gemm.hip, wgrad.hip, head.hip): the v_mfma_f64_16x16x4f64 fragment map, the
// XCD tile order, the register-ring K loop of the kernels that read their operands straight
// from L2, the 16-lane reduce-scatter and the Gaussian head epilogue on a tile of z2
// accumulators.
#pragma once
#include "common.hpp"

namespace mepol {
namespace mfma {

typedef double d4 __attribute__((ext_vector_type(4)));

// C/D fragment of the f64 16x16x4 MFMA: element q (0..3) of a lane's d4 is
// (row = (lane >> 4) + 4 q, col = lane & 15) of the 16 x 16 tile.
__device__ __forceinline__ int frag_col(int lane) { return lane & 15; }
__device__ __forceinline__ int frag_row(int lane, int q) { return (lane >> 4) + 4 * q; }

// XCD-aware tile order for a 1-D grid: workgroup L runs on XCD L % 8, so consecutive tiles
// (the column tiles of one row block, which share the A rows) are given to consecutive
// workgroups of the SAME XCD and meet in its L2.  A bijection on [0, ntiles).
__device__ __forceinline__ int xcd_tile(int L, int ntiles) {
  const int x = L & 7, s = L >> 3, q = ntiles >> 3, r = ntiles & 7;
  return x * q + min(x, r) + s;
}

// K loop of a kernel whose operands go from L2 into the MFMA fragments through a ring of NS
// register slots (no LDS, no barrier): stage s is multiplied from slot s % NS while the loads
// of stage s + NS - 1 are in flight.  The first nfull stages are whole; stages nfull .. nst - 1
// (at most one) are ragged.  The caller owns the slots and gives
//   load(slot, s)       issue the loads of stage s into a slot (s < nst; clamped addresses)
//   zero_tail(slot, s)  zero what the ragged stage s read past the end of K
//   mul(slot)           the MFMAs of a slot
// Slot numbers are compile-time after unrolling, so the ring stays in registers.
// PIN: scheduling barriers hold the compiled code to this issue order -- the loads of stage
// s + NS - 1, then the MFMAs of stage s, which wait only for loads a whole MFMA block old.
// Without them the scheduler is free to sink a slot's loads below the MFMAs that should cover
// them (it did in wgrad_kernel: both slots' loads back to back after the first MFMA block, so
// every second stage started with no lookahead).  The caller chooses: a kernel whose free
// schedule already interleaves the loads with the previous MFMAs is better left unpinned.
template <int NS, bool PIN, typename I, typename Load, typename ZeroTail, typename Mul>
__device__ __forceinline__ void ring_k_loop(I nfull, I nst, Load load, ZeroTail zero_tail,
                                            Mul mul) {
#pragma unroll
  for (int p = 0; p < NS - 1; ++p) load(p, min((I)p, nst - 1));
  I s = 0;
  // steady state, unrolled by NS: stage s is in slot s % NS
#pragma nounroll
  for (; s + NS <= nfull; s += NS) {
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      load((p + NS - 1) % NS, min(s + p + NS - 1, nst - 1));
      if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
      mul(p);
      if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the remaining (< NS) full stages and the ragged last one, in the same ring rotation
#pragma unroll
  for (int p = 0; p < NS; ++p) {
    if (s + p < nst) {  // uniform
      if (s + p + NS - 1 < nst) load((p + NS - 1) % NS, s + p + NS - 1);
      if (s + p >= nfull) zero_tail(p, s + p);
      if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
      mul(p);
      if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Reduce-scatter of AP per-lane values over groups of G lanes (G a power of two <= 64, lanes
// of a group consecutive): halving exchanges, then a butterfly over the remaining lanes.  Lane
// l ends with the group's sum for component a_out; lanes of a group agreeing on the bits
// log2(G)-1 .. log2(G)-log2(AP) hold the same component.
// Every array index is a compile-time constant (the recursion halves AP and G), so the values
// stay in registers.
template <int AP, int G>
__device__ __forceinline__ double reduce_scatter_g(const double (&v)[AP], int l, int& a_out) {
  if constexpr (AP == 1) {
    double x = v[0];
#pragma unroll
    for (int bit = G / 2; bit >= 1; bit >>= 1) x += __shfl_xor(x, bit, kWave);
    a_out = 0;
    return x;
  } else {
    constexpr int half = AP / 2, bit = G / 2;
    const bool upper = (l & bit) != 0;
    double h[half];
#pragma unroll
    for (int a = 0; a < half; ++a) {
      const double send = upper ? v[a] : v[a + half];
      const double keep = upper ? v[a + half] : v[a];
      h[a] = keep + __shfl_xor(send, bit, kWave);
    }
    int sub;
    const double x = reduce_scatter_g<half, bit>(h, l, sub);
    a_out = (upper ? half : 0) + sub;
    return x;
  }
}

constexpr double kLog2Pi = 1.8378770664093453;
constexpr double kStdEps = 1e-7;

// Epilogue of a z2 = h1 W2^T tile held in MFMA accumulators: z2 (pre-bias) to HBM, then the
// Gaussian head mu = relu(z2 + b2) Wm^T + bm and logp = sum_a log N(act | mu, exp(log_std) +
// 1e-7) for the block's BM rows.  Every wave holds FR x FC fragments: rows rl0 .. rl0 + 16 FR of
// the block, columns 16 FC wc .. of z2 (wc < NW column waves).  AC actions per pass: per-lane
// partial means over the lane's FC columns, reduce-scatter over the 16 lanes of a row, then the
// NW column waves' partials are summed in wave order through sMu ([NW][BM][AC] doubles of LDS)
// by thread (row tid / AC, action slot tid % AC).  The block must have BM * AC threads: the
// caller asserts that against its launch bounds.
template <int FR, int FC, int AC, int NW, int BM>
__device__ __forceinline__ void head_epilogue(
    const d4 (&acc)[FR][FC], int64_t row0, int rl0, int wc, int64_t N,
    const double* __restrict__ b2, int H2, const double* __restrict__ Wm,
    const double* __restrict__ bm, const double* __restrict__ log_std,
    const double* __restrict__ act, int A, double* __restrict__ z2_out,
    double* __restrict__ mu_out, double* __restrict__ logp_out, double* sMu) {
  static_assert(AC == 4 || AC == 8, "actions per pass");
  static_assert(BM % 16 == 0 && BM * AC <= 1024, "the block has BM * AC threads");
  const int tid = threadIdx.x, lane = tid & 63;
  const int fr = frag_col(lane);
  const int col0 = wc * FC * 16;
  double b2v[FC];
#pragma unroll
  for (int j = 0; j < FC; ++j) {
    const int c = col0 + j * 16 + fr;
    b2v[j] = c < H2 ? b2[c] : 0.0;
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = row0 + rl0 + i * 16 + frag_row(lane, q);
        if (c < H2 && r < N) z2_out[r * H2 + c] = acc[i][j][q];
      }
  }
  const int er = tid / AC, ea = tid % AC;  // combine step: row er of the block, action slot ea
  double lp = 0.0;
  for (int a0 = 0; a0 < A; a0 += AC) {
    double wmv[FC][AC];
#pragma unroll
    for (int j = 0; j < FC; ++j) {
      const int c = col0 + j * 16 + fr;
#pragma unroll
      for (int a = 0; a < AC; ++a)
        wmv[j][a] = (c < H2 && a0 + a < A) ? Wm[(int64_t)(a0 + a) * H2 + c] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double p[AC];
#pragma unroll
        for (int a = 0; a < AC; ++a) p[a] = 0.0;
#pragma unroll
        for (int j = 0; j < FC; ++j) {
          const double rv = fmax(acc[i][j][q] + b2v[j], 0.0);
#pragma unroll
          for (int a = 0; a < AC; ++a) p[a] = fma(rv, wmv[j][a], p[a]);
        }
        int comp;
        const double v = reduce_scatter_g<AC, 16>(p, fr, comp);
        // lanes of a row with equal component: 16 / AC of them; the lowest one writes
        if ((fr & (16 / AC - 1)) == 0)
          sMu[(wc * BM + rl0 + i * 16 + frag_row(lane, q)) * AC + comp] = v;
      }
    __syncthreads();
    {
      const int a = a0 + ea;
      const int64_t r = row0 + er;
      double term = 0.0;
      if (a < A && r < N) {
        double m = sMu[(0 * BM + er) * AC + ea];
#pragma unroll
        for (int w = 1; w < NW; ++w) m += sMu[(w * BM + er) * AC + ea];
        m += bm[a];
        const double lsa = log_std[a];
        const double sd = exp(lsa) + kStdEps;
        const double d = act[r * A + a] - m;
        mu_out[r * A + a] = m;
        term = -0.5 * (kLog2Pi + 2.0 * lsa + d * d / (sd * sd));
      }
#pragma unroll
      for (int bit = AC / 2; bit >= 1; bit >>= 1) term += __shfl_xor(term, bit, kWave);
      lp += term;
    }
    __syncthreads();
  }
  if (ea == 0 && row0 + er < N) logp_out[row0 + er] = lp;
}

}  // namespace mfma
}  // namespace mepol
