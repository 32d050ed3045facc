// TRPO's critic fit in one launch: n_steps sequential Adam steps of the reference's mini-batch
// update (src/algorithms/trpo.py:441-457: loss = mean((v(x_b) - t_b)^2), optimizer.step()) on
// the critic Linear(nf, h0) -> ReLU -> Linear(h0, h1) -> ReLU -> Linear(h1, 1), f64.
//
// The steps depend on each other and one step is ~1.6 Mflop, so the whole fit runs on ONE
// resident workgroup of 256 threads (4 waves, one per SIMD of a CU).  Parameters live in LDS for
// the whole launch and go back to HBM once at the end; the Adam moments live in the registers of
// the threads that own the elements; the mini-batches are gathered through `index`, two steps
// ahead (indices) and one step ahead (rows), so no step waits for HBM.
//
// LDS image (doubles; 64 x 64 tiles are stored swizzled, see sw()):
//   sW2 [64][64]  W2[o][i]            sH1 [64][64]  h1[b][i]
//   sDz [64][64]  dz2[b][o]           sD1 [64][64]  dz1[b][i]
//   sW1 [64][17]  W1[o][f]            sX  [64][17], sT [64]   the mini-batch
//   sB1, sB2, sW3 [64], sB3           sP  per-wave partial sums of the column reductions
// Everything is zeroed once; rows and columns past (B, h0, h1) are never written with anything
// but zeros, so the fragments of ragged shapes are padded inside the kernel, and the code below
// has no per-element bounds branch: a padded element's gradient and moments are 0 and stay 0, and
// its parameter is stored as 0 whatever Adam makes of it (0 / eps; NaN when eps == 0, which would
// reach the next step's products as 0 * NaN).
//
// One step, five workgroup barriers:
//   A   rows of the step (loaded a step ago) -> sX, sT
//  ---
//   B   h1 = relu(x W1^T + b1): MFMA over K = nf (padded to 4), wave w owns rows 16 w ..
//  ---
//   C   z2 = h1 W2^T on the f64 MFMA; wave w owns rows 16 w ..; on the accumulators: h2 =
//       relu(z2 + b2), v = h2 W3^T + b3 (16-lane butterfly), err = v - t, dv = 2 err / B,
//       dz2 = dv W3 (z2 > 0) -> sDz, and the wave's partial column sums of dz2 (db2), dv h2
//       (dW3), dv (db3) and err^2 (the loss) -> sP
//  ---
//   D   dW2 = dz2^T h1 (MFMA; wave w owns rows o = 16 w ..); dh1 = dz2 W2 (MFMA), dz1 = dh1
//       (h1 > 0) -> sD1 and its partial column sums (db1) -> sP; Adam on the dW2 fragments in
//       registers
//  ---
//   E   new W2 -> sW2;  b1, b2, W3, b3: partials summed in wave order, Adam;  dW1 = dz1^T x
//       (MFMA; wave w owns rows o = 16 w .., one column fragment of nf <= 16), Adam;  loss_out[s]
//  ---
// All sums run in a fixed order: the same inputs give the same bits.
//
// Swizzle: element (r, c) of a 64 x 64 tile is at r * 64 + (c ^ g(r)), g(r) = 2 * ((r ^ 8 (r &
// 1)) & 15).  The MFMA fragments are read two ways -- 16 rows x 2 consecutive columns per group
// of 32 lanes (A of z2 and dh1, B of z2), and 2 consecutive rows x 16 columns (both operands of
// dW2, B of dh1: the reads down the batch dimension).  With ds_read_b64 (32 banks of 8 bytes per
// 32-lane group) both are conflict-free: in the first, bits 1..4 of g differ over 16 rows; in
// the second, bit 4 of g differs between rows r and r + 1.  sX and sW1 are plain rows of 17: 16
// rows x 2 columns hit 32 banks.
#include "adam_math.hpp"
#include "mfma_f64.hpp"

namespace mepol {
namespace critic {

using mfma::d4;
using mfma::frag_col;
using mfma::frag_row;
using optim::adam_element;
using optim::AdamStep;

constexpr int kThreads = 256, kWaves = 4;
constexpr int kMaxH = 64, kMaxB = 64, kMaxF = 16;
constexpr int kW1S = kMaxF + 1, kXS = kMaxF + 1;   // row strides of sW1, sX: odd
constexpr int kGather = kMaxB * kMaxF / kThreads;  // gathered elements per thread (4)

// LDS offsets in doubles
constexpr int kTile = 64 * 64;
constexpr int oW2 = 0, oH1 = oW2 + kTile, oDz = oH1 + kTile, oD1 = oDz + kTile;
constexpr int oW1 = oD1 + kTile, oX = oW1 + kMaxH * kW1S, oT = oX + kMaxB * kXS;
constexpr int oB1 = oT + kMaxB, oB2 = oB1 + kMaxH, oW3 = oB2 + kMaxH, oB3 = oW3 + kMaxH;
constexpr int oPdb1 = oB3 + 8, oPdb2 = oPdb1 + kWaves * kMaxH, oPdw3 = oPdb2 + kWaves * kMaxH;
constexpr int oPdv = oPdw3 + kWaves * kMaxH, oPloss = oPdv + kWaves;
constexpr int kLdsDoubles = oPloss + kWaves;
constexpr size_t kLdsBytes = (size_t)kLdsDoubles * sizeof(double);
static_assert(kLdsBytes <= 160 * 1024, "one CU's LDS");

__device__ __forceinline__ int sw(int r, int c) {
  return r * 64 + (c ^ (((r ^ ((r & 1) << 3)) & 15) << 1));
}

struct Args {
  const double* states;   // [N, nf]
  const double* targets;  // [N]
  const int* index;       // [n_steps * B]
  const double* scal;     // [n_steps][2] = (step_size, bc2_sqrt)
  double* p[6];           // W1 [h0, nf], b1, W2 [h1, h0], b2, W3 [1, h1], b3
  double* m[6];           // exp_avg
  double* v[6];           // exp_avg_sq
  double* loss_out;       // [n_steps] or nullptr
  int64_t N, n_steps;
  int nf, h0, h1, B;
  double beta1, beta2, eps;
};

// acc[j] = A[16 rows][K] B[K][16 columns of fragment j] for j < NCF (0 for the others) over
// ksteps >= 1 steps of four k, the operands of step ks + 1 read while step ks multiplies.  This
// lane's operand elements are ld_a(k) = A[lane & 15][k] and ld_b(k, j) = B_j[k][lane & 15] at
// k = 4 ks + (lane >> 4).
template <int NCF, typename LdA, typename LdB>
__device__ __forceinline__ void gemm_strip_n(LdA ld_a, LdB ld_b, int ksteps, d4 (&acc)[4]) {
  const int kk = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  double a = ld_a(kk), b[NCF];
#pragma unroll
  for (int j = 0; j < NCF; ++j) b[j] = ld_b(kk, j);
  for (int ks = 0; ks < ksteps; ++ks) {
    const int kn = 4 * min(ks + 1, ksteps - 1) + kk;
    const double an = ld_a(kn);
    double bn[NCF];
#pragma unroll
    for (int j = 0; j < NCF; ++j) bn[j] = ld_b(kn, j);
#pragma unroll
    for (int j = 0; j < NCF; ++j)
      acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[j], 0, 0, 0);
    a = an;
#pragma unroll
    for (int j = 0; j < NCF; ++j) b[j] = bn[j];
  }
}

// ncf (1..4, uniform) column fragments: one branch-free K loop per count.
template <typename LdA, typename LdB>
__device__ __forceinline__ void gemm_strip(LdA ld_a, LdB ld_b, int ksteps, int ncf,
                                           d4 (&acc)[4]) {
  if (ncf == 4)
    gemm_strip_n<4>(ld_a, ld_b, ksteps, acc);
  else if (ncf == 3)
    gemm_strip_n<3>(ld_a, ld_b, ksteps, acc);
  else if (ncf == 2)
    gemm_strip_n<2>(ld_a, ld_b, ksteps, acc);
  else
    gemm_strip_n<1>(ld_a, ld_b, ksteps, acc);
}

// Sum of a per-lane value over the wave's 16 rows of a C fragment column: the lane's four rows
// are in `x` already; the four lane groups follow.
__device__ __forceinline__ double rows_sum(double x) {
  x += __shfl_xor(x, 16, kWave);
  x += __shfl_xor(x, 32, kWave);
  return x;
}

__global__ __launch_bounds__(kThreads) void critic_fit_kernel(Args a) {
  extern __shared__ double lds[];
  double* sW2 = lds + oW2;
  double* sH1 = lds + oH1;
  double* sDz = lds + oDz;
  double* sD1 = lds + oD1;
  double* sW1 = lds + oW1;
  double* sX = lds + oX;
  double* sT = lds + oT;
  double* sB1 = lds + oB1;
  double* sB2 = lds + oB2;
  double* sW3 = lds + oW3;
  double* sB3 = lds + oB3;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nf = a.nf, H0 = a.h0, H1 = a.h1, B = a.B;
  const int64_t N = a.N, n_steps = a.n_steps;
  const int fc = frag_col(lane), fg = lane >> 4;

  for (int i = tid; i < kLdsDoubles; i += kThreads) lds[i] = 0.0;
  __syncthreads();

  // parameters -> LDS
  for (int e = tid; e < H0 * nf; e += kThreads) sW1[(e / nf) * kW1S + e % nf] = a.p[0][e];
  for (int e = tid; e < H1 * H0; e += kThreads) sW2[sw(e / H0, e % H0)] = a.p[2][e];
  if (tid < H0) sB1[tid] = a.p[1][tid];
  if (tid < H1) {
    sB2[tid] = a.p[3][tid];
    sW3[tid] = a.p[4][tid];
  }
  if (tid == 0) sB3[0] = a.p[5][0];

  // moments -> registers of the owners
  // W2: the C fragments of dW2: (o = 16 w + fg + 4 q, i = 16 j + fc)
  double mW2[4][4], vW2[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = 16 * w + frag_row(lane, q), i = 16 * j + fc;
      const bool on = o < H1 && i < H0;
      mW2[j][q] = on ? a.m[2][o * H0 + i] : 0.0;
      vW2[j][q] = on ? a.v[2][o * H0 + i] : 0.0;
    }
  // W1: the C fragment of dW1: (o = 16 w + fg + 4 q, f = fc)
  double mW1[4], vW1[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = 16 * w + frag_row(lane, q);
    const bool on = o < H0 && fc < nf;
    mW1[q] = on ? a.m[0][o * nf + fc] : 0.0;
    vW1[q] = on ? a.v[0][o * nf + fc] : 0.0;
  }
  // the vectors: b2 in wave 0, W3 in wave 1, b1 in wave 2, b3 in thread 192
  const int misc = (w == 0 && lane < H1)   ? 3
                   : (w == 1 && lane < H1) ? 4
                   : (w == 2 && lane < H0) ? 1
                   : tid == 192            ? 5
                                           : -1;
  double mM = 0.0, vM = 0.0;
  if (misc >= 0) {
    mM = a.m[misc][misc == 5 ? 0 : lane];
    vM = a.v[misc][misc == 5 ? 0 : lane];
  }

  // the gather slots of this thread: element e = tid + 256 i of the B x nf mini-batch
  int gb[kGather], gf[kGather];
  bool gon[kGather];
#pragma unroll
  for (int i = 0; i < kGather; ++i) {
    const int e = tid + kThreads * i;
    gon[i] = e < B * nf;
    gb[i] = gon[i] ? e / nf : 0;
    gf[i] = gon[i] ? e - gb[i] * nf : 0;
  }
  const int tb = tid < B ? tid : 0;
  // Loads are unconditional at clamped addresses, and an index outside [0, N) reads row 0 and
  // turns into NaN: nothing outside the caller's tensors is touched, and the result shows it.
  // (The NaN select waits until store_rows: next to the loads it would wait for them.)
  const double kNaN = __builtin_nan("");
  int ix[kGather], it;
  double xv[kGather], tv;
  bool okx[kGather], okt;
  auto load_idx = [&](int64_t s) {
#pragma unroll
    for (int i = 0; i < kGather; ++i) ix[i] = a.index[s * B + gb[i]];
    it = a.index[s * B + tb];
  };
  auto load_rows = [&]() {
#pragma unroll
    for (int i = 0; i < kGather; ++i) {
      okx[i] = ix[i] >= 0 && ix[i] < N;
      xv[i] = a.states[(okx[i] ? (int64_t)ix[i] : 0) * nf + gf[i]];
    }
    okt = it >= 0 && it < N;
    tv = a.targets[okt ? it : 0];
  };
  auto store_rows = [&]() {
#pragma unroll
    for (int i = 0; i < kGather; ++i)
      if (gon[i]) sX[gb[i] * kXS + gf[i]] = okx[i] ? xv[i] : kNaN;
    if (tid < B) sT[tid] = okt ? tv : kNaN;
  };
  load_idx(0);
  load_rows();
  if (n_steps > 1) load_idx(1);
  double step_size = a.scal[0], bc2_sqrt = a.scal[1];

  const int nfB = (B + 15) >> 4, nfH0 = (H0 + 15) >> 4, nfH1 = (H1 + 15) >> 4;  // 16-wide frags
  const int ksB = (B + 3) >> 2, ksH0 = (H0 + 3) >> 2, ksH1 = (H1 + 3) >> 2;     // k-steps
  const int ksF = (nf + 3) >> 2;
  const int r0 = 16 * w + fc;  // the operand row / column of this lane in its wave's strip
  const double dB = (double)B;
  __syncthreads();

  for (int64_t s = 0; s < n_steps; ++s) {
    const AdamStep st = optim::adam_step(step_size, bc2_sqrt, a.beta1, a.beta2, a.eps);
    // ---- A: this step's rows; then the loads of step s + 1's rows and step s + 2's indices,
    // which stay in flight for the whole step
    store_rows();
    if (s + 1 < n_steps) {
      load_rows();
      step_size = a.scal[2 * (s + 1)];
      bc2_sqrt = a.scal[2 * (s + 1) + 1];
      if (s + 2 < n_steps) load_idx(s + 2);
    }
    __syncthreads();

    // ---- B: h1 = relu(x W1^T + b1)
    if (w < nfB) {
      d4 acc[4];
      gemm_strip([&](int k) { return sX[r0 * kXS + k]; },
                 [&](int k, int j) { return sW1[(16 * j + fc) * kW1S + k]; }, ksF, nfH0, acc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = 16 * j + fc;
        const double b1 = sB1[o];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int b = 16 * w + frag_row(lane, q);
          const double z = acc[j][q] + b1;  // 0 in a padded column: its W1 row and b1 are 0
          sH1[sw(b, o)] = (b < B && z > 0.0) ? z : 0.0;
        }
      }
    }
    __syncthreads();

    // ---- C: z2 and the head on its accumulators
    if (w < nfB) {
      d4 acc[4];
      gemm_strip([&](int k) { return sH1[sw(r0, k)]; },
                 [&](int k, int j) { return sW2[sw(16 * j + fc, k)]; }, ksH0, nfH1, acc);
      const double b3 = sB3[0];
      double pv[4] = {0.0, 0.0, 0.0, 0.0};
      double w3[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = 16 * j + fc;
        const double b2 = sB2[o];
        w3[j] = sW3[o];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double z = acc[j][q] + b2;  // 0 in a padded column: its W2 row and b2 are 0
          const double h = z > 0.0 ? z : 0.0;
          acc[j][q] = h;  // h2
          pv[q] += h * w3[j];
        }
      }
      double dv[4], sdv = 0.0, sl = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int bit = 8; bit >= 1; bit >>= 1) pv[q] += __shfl_xor(pv[q], bit, kWave);
        const int b = 16 * w + frag_row(lane, q);
        const double err = b < B ? (pv[q] + b3) - sT[b] : 0.0;
        dv[q] = b < B ? 2.0 * err / dB : 0.0;
        sdv += dv[q];
        sl += err * err;
      }
      sdv = rows_sum(sdv);
      sl = rows_sum(sl);
      if (lane == 0) {
        lds[oPdv + w] = sdv;
        lds[oPloss + w] = sl;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = 16 * j + fc;
        double sdb = 0.0, sdw = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int b = 16 * w + frag_row(lane, q);
          const double h = acc[j][q];
          const double dz = (b < B && h > 0.0) ? dv[q] * w3[j] : 0.0;
          sDz[sw(b, o)] = dz;
          sdb += dz;
          sdw += b < B ? dv[q] * h : 0.0;
        }
        sdb = rows_sum(sdb);
        sdw = rows_sum(sdw);
        if (fg == 0) {
          lds[oPdb2 + w * kMaxH + o] = sdb;
          lds[oPdw3 + w * kMaxH + o] = sdw;
        }
      }
    }
    __syncthreads();

    // ---- D: dW2 and its Adam update in registers; dh1 -> dz1 and db1's partials
    d4 nW2[4];
    if (w < nfH1)
      gemm_strip([&](int k) { return sDz[sw(k, r0)]; },
                 [&](int k, int j) { return sH1[sw(k, 16 * j + fc)]; }, ksB, nfH0, nW2);
    if (w < nfB) {
      d4 acc[4];
      gemm_strip([&](int k) { return sDz[sw(r0, k)]; },
                 [&](int k, int j) { return sW2[sw(k, 16 * j + fc)]; }, ksH1, nfH0, acc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double sdb = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int at = sw(16 * w + frag_row(lane, q), 16 * j + fc);
          const double dz = sH1[at] > 0.0 ? acc[j][q] : 0.0;
          sD1[at] = dz;
          sdb += dz;
        }
        sdb = rows_sum(sdb);
        if (fg == 0) lds[oPdb1 + w * kMaxH + 16 * j + fc] = sdb;
      }
    }
    if (w < nfH1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= nfH0) continue;  // an all-padding fragment: nW2[j] is 0 and stays 0
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int o = 16 * w + frag_row(lane, q), i = 16 * j + fc;
          double p = sW2[sw(o, i)];
          adam_element(st, nW2[j][q], p, mW2[j][q], vW2[j][q]);
          nW2[j][q] = (o < H1 && i < H0) ? p : 0.0;  // padded: 0 / eps, NaN when eps == 0
        }
      }
    }
    __syncthreads();

    // ---- E: the other updates
    if (w < nfH1) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) sW2[sw(16 * w + frag_row(lane, q), 16 * j + fc)] = nW2[j][q];
    }
    if (misc >= 0) {
      const int po = misc == 1   ? oPdb1 + lane
                     : misc == 3 ? oPdb2 + lane
                     : misc == 4 ? oPdw3 + lane
                                 : oPdv;
      const int ps = misc == 5 ? 1 : kMaxH;
      const double g = ((lds[po] + lds[po + ps]) + lds[po + 2 * ps]) + lds[po + 3 * ps];
      double* pp = misc == 1 ? sB1 + lane : misc == 3 ? sB2 + lane : misc == 4 ? sW3 + lane : sB3;
      double p = *pp;
      adam_element(st, g, p, mM, vM);
      *pp = p;
    }
    if (tid == 193 && a.loss_out) {
      const double* pl = lds + oPloss;
      a.loss_out[s] = (((pl[0] + pl[1]) + pl[2]) + pl[3]) / dB;
    }
    if (w < nfH0) {
      // dW1[o][f] = sum_b dz1[b][o] x[b][f]: rows o = 16 w .., one column fragment f = fc
      d4 acc[4];
      gemm_strip_n<1>([&](int k) { return sD1[sw(k, r0)]; },
                      [&](int k, int) { return sX[k * kXS + fc]; }, ksB, acc);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = 16 * w + frag_row(lane, q);
        double* pp = sW1 + o * kW1S + fc;
        double p = *pp;
        adam_element(st, acc[0][q], p, mW1[q], vW1[q]);
        *pp = (o < H0 && fc < nf) ? p : 0.0;  // as for W2
      }
    }
    __syncthreads();
  }

  // parameters and moments -> HBM
  for (int e = tid; e < H0 * nf; e += kThreads) a.p[0][e] = sW1[(e / nf) * kW1S + e % nf];
  for (int e = tid; e < H1 * H0; e += kThreads) a.p[2][e] = sW2[sw(e / H0, e % H0)];
  if (tid < H0) a.p[1][tid] = sB1[tid];
  if (tid < H1) {
    a.p[3][tid] = sB2[tid];
    a.p[4][tid] = sW3[tid];
  }
  if (tid == 0) a.p[5][0] = sB3[0];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = 16 * w + frag_row(lane, q), i = 16 * j + fc;
      if (o < H1 && i < H0) {
        a.m[2][o * H0 + i] = mW2[j][q];
        a.v[2][o * H0 + i] = vW2[j][q];
      }
    }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = 16 * w + frag_row(lane, q);
    if (o < H0 && fc < nf) {
      a.m[0][o * nf + fc] = mW1[q];
      a.v[0][o * nf + fc] = vW1[q];
    }
  }
  if (misc >= 0) {
    a.m[misc][misc == 5 ? 0 : lane] = mM;
    a.v[misc][misc == 5 ? 0 : lane] = vM;
  }
}

bool shape_ok(int nf, int h0, int h1, int B) {
  return nf >= 1 && nf <= kMaxF && h0 >= 1 && h0 <= kMaxH && h1 >= 1 && h1 <= kMaxH && B >= 1 &&
         B <= kMaxB;
}

}  // namespace critic
}  // namespace mepol

using namespace mepol;
using namespace mepol::critic;

extern "C" int mepol_critic_fit_plan_info(int nf, int h0, int h1, int batch, int* threads,
                                          int* lds_bytes, int* accepted) {
  if (threads) *threads = kThreads;
  if (lds_bytes) *lds_bytes = (int)kLdsBytes;
  if (accepted) *accepted = shape_ok(nf, h0, h1, batch) ? 1 : 0;
  return 0;
}

extern "C" int mepol_critic_fit(const double* states, const double* targets, int64_t n,
                                const int32_t* index, int64_t n_steps, int batch, int nf, int h0,
                                int h1, double* const* params, double* const* exp_avg,
                                double* const* exp_avg_sq, const double* scal, double beta1,
                                double beta2, double eps, double* loss_out, void* stream) {
  if (!shape_ok(nf, h0, h1, batch)) {
    set_error("mepol_critic_fit: shape (nf %d, h0 %d, h1 %d, batch %d) outside 1 <= nf <= %d, "
              "1 <= h0, h1 <= %d, 1 <= batch <= %d",
              nf, h0, h1, batch, kMaxF, kMaxH, kMaxB);
    return kErrBadArg;
  }
  if (n_steps < 1 || n < 1 || n > INT32_MAX) {
    set_error("mepol_critic_fit: n_steps >= 1 and 1 <= n < 2^31 are needed (n_steps %lld, n %lld)",
              (long long)n_steps, (long long)n);
    return kErrBadArg;
  }
  if (!states || !targets || !index || !params || !exp_avg || !exp_avg_sq || !scal) {
    set_error("mepol_critic_fit: null argument");
    return kErrBadArg;
  }
  Args a{};
  a.states = states;
  a.targets = targets;
  a.index = index;
  a.scal = scal;
  for (int i = 0; i < 6; ++i) {
    if (!params[i] || !exp_avg[i] || !exp_avg_sq[i]) {
      set_error("mepol_critic_fit: null tensor %d", i);
      return kErrBadArg;
    }
    a.p[i] = params[i];
    a.m[i] = exp_avg[i];
    a.v[i] = exp_avg_sq[i];
  }
  a.loss_out = loss_out;
  a.N = n;
  a.n_steps = n_steps;
  a.nf = nf;
  a.h0 = h0;
  a.h1 = h1;
  a.B = batch;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  MEPOL_HIP((max_dynamic_lds<critic_fit_kernel>((int)kLdsBytes)));
  hipLaunchKernelGGL(critic_fit_kernel, dim3(1), dim3(kThreads), kLdsBytes, (hipStream_t)stream,
                     a);
  MEPOL_CHECK_LAUNCH();
  return 0;
}
