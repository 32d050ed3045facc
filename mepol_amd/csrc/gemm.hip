// f64 GEMM on the CDNA4 matrix cores (v_mfma_f64_16x16x4f64) for the policy's hidden layer:
// C[n][m] = act(sum_k A[n][k] B[m][k] + bias[m]) with A [N x K] and B [M x K] row-major ("NT"),
// which is z2 = h1 W2^T of GaussianPolicy.net (src/policy.py:21-26, the 400 -> 300 Linear) and,
// with B = W2^T, dh1 = dz2 W2 of its backward.
//
// Tiling: a workgroup owns a BM x BN tile of C (WR x WC waves, each FR x FC 16x16 fragments,
// accumulators in registers), streams K through LDS in k-tiles of 16 (double-buffered, one
// barrier per tile).  The k order inside a tile is permuted so that each lane's four k-steps
// are contiguous (lane group g = lane>>4 feeds k = 4g + s at step s for both operands), i.e.
// two b128 reads give a lane all of its fragment data for the tile.  Rows of both operand
// tiles are 128 B (two to a 256-B bank row) with the 16-B slots XOR-swizzled per row
// (lds_slot): a ds_read_b128 is serviced in the lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31} (+32), i.e. rows fr 0-3, 12-15 of one k-slot with rows 4-11 of the next
// one, and the swizzle puts each group's 16 reads on 16 distinct slots (the round-5 144-B
// padded stride left two of them 2-way: SQ_LDS_BANK_CONFLICT 3.3e7 per C3 dh1 call); the
// stores (8-lane groups, one row) stay conflict-free.
// d4, the fragment map and xcd_tile come from mfma_f64.hpp, the fixed-order sum of the dh1
// kernel's row-block partials from reduce.hpp.
#include "mfma_f64.hpp"
#include "reduce.hpp"

#include <type_traits>

namespace mepol {
namespace gemm {

constexpr int KT = 16;  // k per LDS tile
constexpr int KP = 16;  // LDS row (doubles), swizzled by lds_slot

// physical 16-B slot of logical slot c (k = 2c, 2c + 1 of the tile) in LDS row r: c ^ h(r) with
// h(r) in {0, 1, 4, 5} from bits 1 and 3 of r.  Read group {rows 0-3, 12-15 at slot j, rows
// 4-11 at j + 2}: h over rows {0, 2, 12, 14} (and the odd ones) is {0, 1, 4, 5}, over rows
// {4, 6, 8, 10} the same set, so j ^ h and (j + 2) ^ h never meet (bit 1 differs).
__device__ __forceinline__ int lds_slot(int r, int c) {
  return c ^ (((r >> 1) & 1) | (((r >> 3) & 1) << 2));
}
using mfma::d4;
using mfma::frag_col;
using mfma::frag_row;
using mfma::xcd_tile;

template <int WR, int WC, int FR, int FC>
struct Cfg {
  static constexpr int kThreads = WR * WC * 64;
  static constexpr int BM = WR * FR * 16, BN = WC * FC * 16;
  static constexpr int CA = BM * (KT / 2), CB = BN * (KT / 2);  // 16-B chunks per k-tile
  static constexpr int PA = (CA + kThreads - 1) / kThreads, PB = (CB + kThreads - 1) / kThreads;
  static constexpr size_t kLds = 2ull * (BM + BN) * KP * sizeof(double);
};

// The main loop shared by the kernels below: acc[i][j] += A[rows of fragment i] B[cols of
// fragment j]^T over all of K for the workgroup tile (row0, col0).  Operand loads read clamped
// (always valid) addresses; out-of-range values are zeroed when the registers are written to
// LDS, after the MFMA block, so no select waits on a load right after issuing it.
// DEEP: two register sets, the global loads of tile t + 2 issued while tile t is computed (the
// store of tile t + 1 then waits on loads a whole tile older); 24 more VGPRs.
// BT: B given as [K][M] row-major (ldb = its row stride, M even, 16-B aligned rows): a lane loads
// B[k][m, m + 1] (consecutive lanes consecutive m: coalesced) and writes the pair into LDS rows
// m and m + 1 of the [BN][KT] image (two 8-B stores).  Lets dh1 = dz2 W2 read the Linear weight
// as stored instead of a per-step W2^T copy.
// ZERO = false: acc is added to, not zeroed first (a second operand pair summed into the same
// accumulators: hidden_tangent_kernel).
template <int WR, int WC, int FR, int FC, bool DEEP = false, bool BT = false, bool ZERO = true>
__device__ __forceinline__ void gemm_mainloop(const double* __restrict__ A, int64_t N, int K,
                                              int64_t lda, const double* __restrict__ B, int M,
                                              int64_t ldb, int64_t row0, int col0, double* lds,
                                              d4 (&acc)[FR][FC]) {
  using P = Cfg<WR, WC, FR, FC>;
  constexpr int T = P::kThreads, BM = P::BM, BN = P::BN;
  double* sA = lds;                  // [2][BM][KP]
  double* sB = lds + 2 * BM * KP;    // [2][BN][KP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int nkt = (K + KT - 1) / KT;
  const int k2 = K - 2;  // last 16-B aligned pair start (K even)

  using RA = double2[P::PA];
  using RB = double2[P::PB];
  auto gload = [&](int kt, RA& ra, RB& rb) __attribute__((always_inline)) {
    const int kb = kt * KT;
#pragma unroll
    for (int p = 0; p < P::PA; ++p) {
      const int ch = min(tid + p * T, P::CA - 1), r = ch >> 3, k = kb + 2 * (ch & 7);
      ra[p] = *reinterpret_cast<const double2*>(A + min<int64_t>(row0 + r, N - 1) * lda +
                                                min(k, k2));
    }
#pragma unroll
    for (int p = 0; p < P::PB; ++p) {
      const int ch = min(tid + p * T, P::CB - 1);
      if constexpr (BT) {
        const int kl = ch / (BN / 2), m = 2 * (ch % (BN / 2));
        rb[p] = *reinterpret_cast<const double2*>(B + (int64_t)min(kb + kl, K - 1) * ldb +
                                                  min(col0 + m, M - 2));
      } else {
        const int r = ch >> 3, k = kb + 2 * (ch & 7);
        rb[p] = *reinterpret_cast<const double2*>(B + (int64_t)min(col0 + r, M - 1) * ldb +
                                                  min(k, k2));
      }
    }
  };
  auto lstore = [&](int kt, int buf, const RA& ra, const RB& rb) __attribute__((always_inline)) {
    const int kb = kt * KT;
#pragma unroll
    for (int p = 0; p < P::PA; ++p) {
      const int ch = tid + p * T, r = ch >> 3, k = kb + 2 * (ch & 7);
      if (ch < P::CA) {
        const bool ok = row0 + r < N && k < K;
        *reinterpret_cast<double2*>(sA + (buf * BM + r) * KP + 2 * lds_slot(r, ch & 7)) =
            ok ? ra[p] : double2{0.0, 0.0};
      }
    }
#pragma unroll
    for (int p = 0; p < P::PB; ++p) {
      const int ch = tid + p * T;
      if (ch < P::CB) {
        if constexpr (BT) {
          const int kl = ch / (BN / 2), m = 2 * (ch % (BN / 2));
          const bool ok = col0 + m < M && kb + kl < K;  // M even: m + 1 < M with m
          const int off = 2 * lds_slot(m, kl >> 1) + (kl & 1);  // rows m, m + 1: same swizzle
          const int off1 = 2 * lds_slot(m + 1, kl >> 1) + (kl & 1);
          sB[(buf * BN + m) * KP + off] = ok ? rb[p].x : 0.0;
          sB[(buf * BN + m + 1) * KP + off1] = ok ? rb[p].y : 0.0;
        } else {
          const int r = ch >> 3, k = kb + 2 * (ch & 7);
          const bool ok = col0 + r < M && k < K;
          *reinterpret_cast<double2*>(sB + (buf * BN + r) * KP + 2 * lds_slot(r, ch & 7)) =
              ok ? rb[p] : double2{0.0, 0.0};
        }
      }
    }
  };

  if constexpr (ZERO) {
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int j = 0; j < FC; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  }

  const int fr = lane & 15, g = lane >> 4;
  // a lane's two slots in its fragment rows (every fragment row is fr mod 16: same swizzle)
  const int sl0 = 2 * lds_slot(fr, 2 * g), sl1 = 2 * lds_slot(fr, 2 * g + 1);
  auto compute = [&](int buf) __attribute__((always_inline)) {
    double2 a[FR][2], b[FC][2];
#pragma unroll
    for (int i = 0; i < FR; ++i) {
      const double* p = sA + (buf * BM + wr * FR * 16 + i * 16 + fr) * KP;
      a[i][0] = *reinterpret_cast<const double2*>(p + sl0);
      a[i][1] = *reinterpret_cast<const double2*>(p + sl1);
    }
#pragma unroll
    for (int j = 0; j < FC; ++j) {
      const double* p = sB + (buf * BN + wc * FC * 16 + j * 16 + fr) * KP;
      b[j][0] = *reinterpret_cast<const double2*>(p + sl0);
      b[j][1] = *reinterpret_cast<const double2*>(p + sl1);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int i = 0; i < FR; ++i) {
        const double av = (s & 1) ? a[i][s >> 1].y : a[i][s >> 1].x;
#pragma unroll
        for (int j = 0; j < FC; ++j) {
          const double bv = (s & 1) ? b[j][s >> 1].y : b[j][s >> 1].x;
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[i][j], 0, 0, 0);
        }
      }
    }
  };

  RA ra0, ra1;
  RB rb0, rb1;
  gload(0, ra0, rb0);
  lstore(0, 0, ra0, rb0);
  if constexpr (DEEP) {
    if (nkt > 1) gload(1, ra1, rb1);
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < nkt; kt += 2) {  // tile kt in buffer 0, kt + 1 in buffer 1
      if (kt + 2 < nkt) gload(kt + 2, ra0, rb0);
      compute(0);
      lstore(kt + 1, 1, ra1, rb1);
      __syncthreads();
      if (kt + 3 < nkt) gload(kt + 3, ra1, rb1);
      compute(1);
      if (kt + 2 < nkt) lstore(kt + 2, 0, ra0, rb0);
      __syncthreads();
    }
    if (kt < nkt) {
      compute(0);
      __syncthreads();
    }
  } else {
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nkt) gload(kt + 1, ra0, rb0);
      compute(buf);
      if (kt + 1 < nkt) lstore(kt + 1, buf ^ 1, ra0, rb0);
      __syncthreads();
    }
  }
}

template <int WR, int WC, int FR, int FC>
__global__ __launch_bounds__(WR * WC * 64) void gemm_nt_kernel(
    const double* __restrict__ A, int64_t N, int K, int64_t lda, const double* __restrict__ B,
    int M, int64_t ldb, const double* __restrict__ bias, int relu, double* __restrict__ C,
    int64_t ldc) {
  using P = Cfg<WR, WC, FR, FC>;
  constexpr int BM = P::BM, BN = P::BN;
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int ncb = (M + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int64_t row0 = (int64_t)(tile / ncb) * BM;
  const int col0 = (tile % ncb) * BN;
  d4 acc[FR][FC];
  gemm_mainloop<WR, WC, FR, FC>(A, N, K, lda, B, M, ldb, row0, col0, lds, acc);

#pragma unroll
  for (int j = 0; j < FC; ++j) {
    const int c = col0 + wc * FC * 16 + j * 16 + frag_col(lane);
    if (c >= M) continue;
    const double bc = bias ? bias[c] : 0.0;
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = row0 + wr * FR * 16 + i * 16 + frag_row(lane, q);
        if (r < N) {
          double v = acc[i][j][q] + bc;
          if (relu) v = fmax(v, 0.0);
          C[r * ldc + c] = v;
        }
      }
  }
}

// ---- dh1 GEMM + first-layer backward (GaussianPolicy.net[0], src/policy.py:21-26) ------------
// dh1 = dz2 W2 is never written: the epilogue masks it with relu'(h1) (h1 > 0, read from the
// forward's h1) and reduces dz1^T [x | 1] over the tile's rows on the matrix cores, i.e. the
// tile's contribution to dW1 (and db1 in column F).  The MFMA accumulator of dh1 already is
// the A operand of that product (its k index = row); x comes from HBM as the B operand.
// Row-block partials part[rb][c][F + 1] are summed in a fixed order by sum_records.
// Tiling: 8 waves x (32 rows x 80 cols), 256 x 80 tile: 5 column tiles for h0 = 400.
namespace l1b {
constexpr int WR = 8, WC = 1, FR = 2, FC = 5;
using P = Cfg<WR, WC, FR, FC>;
constexpr int kGroups = 16;  // sum_records' groups of row blocks

inline int row_blocks(int64_t n) { return (int)((n + P::BM - 1) / P::BM); }
inline size_t ws_bytes(int64_t n, int m, int F) {
  return sum_records_bytes<kGroups>(row_blocks(n), (size_t)m * (F + 1));
}

// element e = c (F + 1) + f of the summed record: dW[c][f], db[c] in column F
struct ScatterW1 {
  int F;
  double *dW, *db;
  __device__ void operator()(int64_t e, double t) const {
    const int c = (int)(e / (F + 1)), f = (int)(e % (F + 1));
    if (f < F)
      dW[(int64_t)c * F + f] = t;
    else if (db)
      db[c] = t;
  }
};
}  // namespace l1b

// MASK: relu'(h1) comes as the forward's bit mask (uint16 word kt of row r holds
// h1[r][16 kt + b] > 0 in bit b, mepol_policy_forward_masked) instead of the f64 h1 values:
// 2 B per 16 columns instead of 128 B, which the epilogue waited for with the MFMAs idle
// (one workgroup per CU).  The same bits either way.
// BT: W2t is the Linear weight W2 as stored, [K][M] (gemm_mainloop's BT)
template <int NH, bool MASK, bool BT>  // NH = ceil((F + 1) / 16) column groups of [x | 1]
__global__ __launch_bounds__(l1b::P::kThreads) void dh1_layer1_bwd_kernel(
    const double* __restrict__ dz2, int64_t N, int K, const double* __restrict__ W2t, int M,
    const void* __restrict__ h1v, const double* __restrict__ x, int F,
    double* __restrict__ part) {
  using namespace l1b;
  constexpr int BM = P::BM, BN = P::BN, T = P::kThreads;
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int ncb = (M + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rb = tile / ncb;
  const int64_t row0 = (int64_t)rb * BM;
  const int col0 = (tile % ncb) * BN;
  d4 acc[FR][FC];
  gemm_mainloop<WR, WC, FR, FC, true, BT>(dz2, N, K, K, W2t, M, BT ? M : K, row0, col0, lds,
                                         acc);

  // Every epilogue operand in ONE batch of unconditional loads (clamped addresses) before the
  // first use: the ReLU mask of h1 at the wave's accumulator elements and the [x | 1] operands.
  // Loaded where they were used, the h1 loads waited out their HBM latency in FC batches
  // (0.40 of the kernel's 1.23 ms went to this epilogue, profiles/r5/f64/).
  // B operands [x | 1] for k-step (i, q): lane (fr, g) holds x[row(i, q, g)][16 h + fr]
  double xb[FR][4][NH];
  using HT = typename std::conditional<MASK, uint32_t, double>::type;
  HT hv[FC][FR][4];
  const double* h1 = static_cast<const double*>(h1v);
  const uint16_t* hm = static_cast<const uint16_t*>(h1v);
  const int mw = (M + 15) / 16;
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // accumulator element (row g + 4 q of fragment i, col fr) is A[m = fr][k = g] of
      // k-step (i, q): rows 16 i + 4 q + g
      const int64_t r = row0 + wave * FR * 16 + i * 16 + 4 * q + g;
      const double* xr = x + min<int64_t>(r, N - 1) * F;
#pragma unroll
      for (int h = 0; h < NH; ++h) xb[i][q][h] = xr[min(16 * h + fr, F - 1)];
      if constexpr (MASK) {
        const uint16_t* mr = hm + min<int64_t>(r, N - 1) * mw;
#pragma unroll
        for (int j = 0; j < FC; ++j) hv[j][i][q] = mr[min((col0 >> 4) + j, mw - 1)];
      } else {
        const double* hr = h1 + min<int64_t>(r, N - 1) * M;
#pragma unroll
        for (int j = 0; j < FC; ++j) hv[j][i][q] = hr[min(col0 + j * 16 + fr, M - 1)];
      }
    }
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool rin = row0 + wave * FR * 16 + i * 16 + 4 * q + g < N;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        // arithmetic, not a select: a select lets hipcc sink the load into a branch and wait
        // for it there (the clamped x value is a finite state coordinate: x * 0 = 0)
        const int f = 16 * h + fr;
        const double keep = (rin && f < F) ? 1.0 : 0.0, one = (rin && f == F) ? 1.0 : 0.0;
        xb[i][q][h] = fma(xb[i][q][h], keep, one);
      }
    }
  // The wave partials of JB column fragments per LDS round (2 when they fit beside each other:
  // 6 workgroup barriers instead of 10 for FC = 5); the per-element sum over the WR waves keeps
  // its order.  The main loop's last barrier retired its LDS reads.
  constexpr int NE = NH * 4 * 64;
  constexpr int JB = 2 * WR * NE * sizeof(double) <= P::kLds ? 2 : 1;
  double* red = lds;  // [JB][WR][NH][4][64]
#pragma unroll
  for (int j0 = 0; j0 < FC; j0 += JB) {
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
      const int j = j0 + jj;
      if (j < FC) {
        const int c = col0 + j * 16 + fr;
        d4 dacc[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) dacc[h] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            bool on;
            if constexpr (MASK)
              on = ((hv[j][i][q] >> fr) & 1u) != 0;
            else
              on = hv[j][i][q] > 0.0;
            // (a row past N has acc = 0 x W2: nan where W2 holds an inf, and its clamped mask
            // is the last row's: the row test keeps that nan out of the column's sums)
            const bool rin = row0 + wave * FR * 16 + i * 16 + 4 * q + g < N;
            const double dz = (on && rin && c < M) ? acc[i][j][q] : 0.0;
#pragma unroll
            for (int h = 0; h < NH; ++h)
              dacc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(dz, xb[i][q][h], dacc[h], 0, 0, 0);
          }
        // dacc[h][r'] = sum over the wave's rows of dz1[.][col0 + 16 j + g + 4 r'] *
        // [x|1][16 h + fr]
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            red[(jj * WR + wave) * NE + (h * 4 + q) * 64 + lane] = dacc[h][q];
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < JB * NE; e += T) {
      const int jj = e / NE, ee = e - jj * NE, j = j0 + jj;
      if (j < FC) {
        double s = red[jj * WR * NE + ee];
#pragma unroll
        for (int w = 1; w < WR; ++w) s += red[(jj * WR + w) * NE + ee];
        const int l = ee & 63, q = (ee >> 6) & 3, h = ee >> 8;
        const int cc = col0 + j * 16 + (l >> 4) + 4 * q, f = 16 * h + (l & 15);
        if (cc < M && f <= F) part[((int64_t)rb * M + cc) * (F + 1) + f] = s;
      }
    }
    __syncthreads();
  }
}

// ---- the same op with its K loop fed from registers ------------------------------------------
// The masked dh1 + layer-1 backward in the shape of z2_head_kernel / wgrad_kernel: 4 waves x
// (64 rows x 80 columns) on the same 256 x 80 tile, xcd_tile order and grid.  Both operands go
// from L2 straight into the MFMA fragments through mfma::ring_k_loop, no LDS and no barrier in
// the K loop, two workgroups per CU.
// The bits are the LDS form's.  Its k-tile of 16 gives lane group g the k-steps 4 g + s, s = 0
// .. 3; here stage st = 2 kt + hf reads the pair k = 16 kt + 4 g + 2 hf + {0, 1} per lane and
// fragment, and its two MFMAs are steps s = 2 hf and 2 hf + 1 of that k-tile: the same operands
// in the same lanes in the same order, all-zero padded steps included.  The epilogue keeps the
// two 32-row halves of a wave apart and adds the eight half-wave partials in the order of the
// LDS form's eight waves.
// BT: W2 as stored, [K][M]: two 8-B loads per fragment and stage (rows k, k + 1; the 16 lanes of
// a row group read 128 contiguous bytes); else W2^T [M][K], one 16-B load.
// Operand addresses are 32-bit byte offsets from workgroup-uniform bases (dz2 + row0 K, W2):
// 9 address registers instead of 18 next to the 160 accumulator registers; direct_fits() bounds
// the sizes so that they cannot overflow.
// Epilogue, built to live beside the accumulators:
//  1. the wave's 64 x 16 NH block of [x | 1] goes once through registers (the ring is dead) into
//     LDS, already zeroed for rows past N and features past F (a select at the store: a clamped
//     x value never reaches a sum), 8 values of a lane at a time;
//  2. dz1 = dh1 . relu'(h1) in place, one row fragment's mask words at a time; a row past N and a
//     column past M become exact zeros here (their accumulators hold clamped copies, nan where
//     W2 holds an inf);
//  3. per column fragment j: NH output fragments per 32-row half, dz1^T [x | 1] with the
//     accumulator as the A operand and [x | 1] read back from LDS per MFMA; then the partials
//     summed through LDS in row order into the row block's record, two waves per round.
// LDS: 40 KB x NH per workgroup, so NH <= 2 keeps two workgroups on a CU.
namespace l1d {
constexpr int NW = 4, FO = 4, FI = 5, NS = 2, NL = FO + FI;
constexpr int BM = NW * 16 * FO, BN = 16 * FI;
static_assert(BM == l1b::P::BM && BN == l1b::P::BN, "the LDS form's tiles, grid and records");
constexpr int kThreads = 64 * NW;
constexpr int kOcc = 2;  // waves per SIMD the register budget is cut for: 256 VGPRs
// The K loop's issue order is left to the scheduler (mfma_f64.hpp's PIN): pinned, every stage
// waits vmcnt(23 .. 14) behind its own 14 loads; free, every second stage waits vmcnt(7 .. 1).
// Both keep 0 scratch; the free order measured 0.4 ms per C3 epoch faster on average and never
// slower (profiles/r15/dh1_direct/).
constexpr bool kPin = false;
constexpr int kMaxNH = 2;  // 3 and 4 need 120 / 160 KB of LDS: one workgroup per CU
template <int NH>
constexpr size_t lds_bytes() {
  return (size_t)NW * (64 * 16 * NH + NH * 4 * 64) * sizeof(double);
}
inline size_t lds_bytes(int nh) { return (size_t)nh * lds_bytes<1>(); }
// the 32-bit operand offsets: (255 K + K) elements of dz2 from the row block's base, K M of W2
inline bool direct_fits(int k, int m, int F) {
  const int nh = (F + 1 + 15) / 16;
  return !(k & 1) && !(m & 1) && nh <= kMaxNH && (int64_t)BM * k < (1 << 28) &&
         (int64_t)k * m < (1 << 28);
}
// Automatic choice: only a grid with more tiles than the chip has CUs.  What this form gains is
// its second workgroup on a CU (and its place beside wgrad_kernel's waves); a grid that leaves
// CUs empty gains nothing from that, and measured on such grids it was slower than the LDS form
// as often as faster (20 to 235 tiles, profiles/r15/dh1_direct/).  The bits do not depend on it.
constexpr int kCUs = 256;
inline bool direct_pays(int64_t n, int m) {
  return (int64_t)l1b::row_blocks(n) * ((m + BN - 1) / BN) > kCUs;
}
// form asked for: 0 = automatic, 1 = the LDS kernel, 2 = this one (must fit)
enum { kAuto = 0, kLds = 1, kDirect = 2 };
inline bool use_direct(int form, int64_t n, int k, int m, int F) {
  return form == kDirect || (form == kAuto && direct_fits(k, m, F) && direct_pays(n, m));
}
}  // namespace l1d

template <int NH, bool BT>
__global__ __launch_bounds__(l1d::kThreads) __attribute__((amdgpu_waves_per_eu(l1d::kOcc))) void
dh1_direct_kernel(const double* __restrict__ dz2, int64_t N, int K, const double* __restrict__ W2,
                  int M, const uint16_t* __restrict__ hm, const double* __restrict__ x, int F,
                  double* __restrict__ part) {
  using namespace l1d;
  constexpr int NE = NH * 4 * 64, XW = 16 * NH;  // doubles of a wave's partial; of an [x | 1] row
  extern __shared__ double lds[];
  const int tid = threadIdx.x, l = tid & 63;
  int fr = l & 15, g = l >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* xs = lds + w * 64 * XW;    // [NW][64][XW], 16-value groups swizzled by the row's bit 0
  double* red = lds + NW * 64 * XW;  // [4][NE]: the half-wave partials of two waves
  const int ncb = (M + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  // (the division runs on the vector ALU: without readfirstlane rb, row0 and col0 would sit in
  // vector registers across the K loop)
  const int rb = __builtin_amdgcn_readfirstlane(tile / ncb);
  const int64_t row0 = (int64_t)rb * BM, wr0 = row0 + 64 * w;
  const int col0 = (tile - rb * ncb) * BN;
  const double* abase = dz2 + row0 * K;  // uniform
  uint32_t ao[FO], bo[FI];  // byte offsets: base + zero-extended 32 bits is one address mode
#pragma unroll
  for (int t = 0; t < FO; ++t)
    ao[t] = 8u * (uint32_t)((int)(min<int64_t>(wr0 + 16 * t + fr, N - 1) - row0) * K + 4 * g);
#pragma unroll
  for (int u = 0; u < FI; ++u) {
    const int c = min(col0 + 16 * u + fr, M - 1);
    bo[u] = 8u * (uint32_t)(BT ? 4 * g * M + c : c * K + 4 * g);
  }
  const char* ab = reinterpret_cast<const char*>(abase);
  const char* bb = reinterpret_cast<const char*>(W2);
  d4 acc[FO][FI];
#pragma unroll
  for (int t = 0; t < FO; ++t)
#pragma unroll
    for (int u = 0; u < FI; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
  // stage st reads k = 16 (st / 2) + 4 g + 2 (st % 2) (+1); K is even, so a pair is whole or
  // past the end.  The address is clamped to the last pair and the pairs past K of the last
  // k-tile's two stages are zeroed at use (ring_k_loop's tail takes both: nfull is even).
  const int nst = 2 * ((K + 15) / 16), nfull = 2 * (K / 16);
  double2 R[NS][NL];
  auto load = [&](double2 (&D)[NL], int st) __attribute__((always_inline)) {
    // k + 4 g <= K - 2; a negative k wraps with the offset it is added to, which holds + 4 g
    const int k = min(16 * (st >> 1) + 2 * (st & 1), K - 2 - 4 * g);
    const uint32_t ka = 8u * (uint32_t)k, kb = BT ? ka * (uint32_t)M : ka;
#pragma unroll
    for (int t = 0; t < FO; ++t) D[t] = *reinterpret_cast<const double2*>(ab + (ao[t] + ka));
#pragma unroll
    for (int u = 0; u < FI; ++u) {
      if constexpr (BT) {
        D[FO + u].x = *reinterpret_cast<const double*>(bb + (bo[u] + kb));
        D[FO + u].y = *reinterpret_cast<const double*>(bb + (bo[u] + kb + 8u * (uint32_t)M));
      } else {
        D[FO + u] = *reinterpret_cast<const double2*>(bb + (bo[u] + kb));
      }
    }
  };
  auto mma = [&](const double2 (&D)[NL]) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < FO; ++t)
#pragma unroll
      for (int u = 0; u < FI; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[t].x, D[FO + u].x, acc[t][u], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < FO; ++t)
#pragma unroll
      for (int u = 0; u < FI; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[t].y, D[FO + u].y, acc[t][u], 0, 0, 0);
  };
  mfma::ring_k_loop<NS, kPin>(
      nfull, nst, [&](int p, int st) __attribute__((always_inline)) { load(R[p], st); },
      [&](int p, int st) __attribute__((always_inline)) {
        if (16 * (st >> 1) + 2 * (st & 1) + 4 * g >= K) {  // the last k-tile's missing pairs
#pragma unroll
          for (int v = 0; v < NL; ++v) R[p][v] = double2{0.0, 0.0};
        }
      },
      [&](int p) __attribute__((always_inline)) { mma(R[p]); });

  // ---- epilogue: acc[t][u][q] = dh1[row wr0 + 16 t + g + 4 q][col col0 + 16 u + fr] ----------
  // 1. [x | 1] of the wave's rows into LDS: lane (fr, g) takes feature 16 h + fr of rows 4 it +
  //    g, which is the B operand of k-step it = 4 i + q (B[k = g][n = fr]).  Group h of a row
  //    sits at group h ^ (row & 1): the two rows a 32-lane half reads are 16 XW B apart (a
  //    whole number of 256-B bank rows for even NH), the swizzle puts them on different banks.
  // (32-bit offsets from the row block's base here too: rows 0 .. nr - 1 of it exist)
  // The lane index is taken again through an opaque copy: nothing the epilogue needs is then a
  // value of the prologue's, kept in a register across the K loop (that cost scratch).
  int le = threadIdx.x;
  asm volatile("" : "+v"(le));
  fr = le & 15, g = (le >> 4) & 3;
  const int nr = (int)min<int64_t>(N - row0, BM);
  const int wl = 64 * w;  // the wave's first row in the row block
  const double* xbase = x + row0 * F;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const int f = 16 * h + fr;
#pragma unroll
    for (int i0 = 0; i0 < 16; i0 += 8) {  // 8 loads in flight, then their 8 stores
      int xo = 0;
      asm volatile("" : "+s"(xo));
      double xv[8];
#pragma unroll
      for (int it = 0; it < 8; ++it)
        xv[it] = xbase[xo + min(wl + 4 * (i0 + it) + g, nr - 1) * F + min(f, F - 1)];
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const bool rin = wl + 4 * (i0 + it) + g < nr;
        const double v = (rin && f < F) ? xv[it] : ((rin && f == F) ? 1.0 : 0.0);
        xs[(4 * (i0 + it) + g) * XW + 16 * (h ^ (g & 1 & (NH - 1))) + fr] = v;
      }
    }
  }
  // 2. dz1 = dh1 * relu'(h1) in place.  Lane (fr, g) loads word min(fr, 4) of the tile's five
  //    mask words of row 16 i + 4 q + g (16 loads for the whole tile) and takes word j from
  //    lane j of its row group: one register per row instead of five.
  const int mw = (M + 15) / 16;
  const uint16_t* hmb = hm + row0 * mw;
  const int hc = min((col0 >> 4) + min(fr, FI - 1), mw - 1);
#pragma unroll
  for (int i = 0; i < FO; ++i) {
    uint32_t hv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) hv[q] = hmb[min(wl + 16 * i + 4 * q + g, nr - 1) * mw + hc];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool rin = wl + 16 * i + 4 * q + g < nr;
#pragma unroll
      for (int j = 0; j < FI; ++j) {
        const uint32_t wj = (uint32_t)__shfl((int)hv[q], 16 * g + j, mepol::kWave);
        const bool on = rin && col0 + 16 * j + fr < M && ((wj >> fr) & 1u) != 0;
        acc[i][j][q] = on ? acc[i][j][q] : 0.0;
      }
    }
  }
  __syncthreads();  // xs is wave-private, but this is the cheapest fence that orders it
  // 3. per column fragment j: dz1^T [x | 1] on the matrix cores (k-step (i, q): A[m = fr][k =
  //    g] = dz1 at (row 16 i + 4 q + g, col fr of fragment j), B[k = g][n = fr] = [x | 1] at
  //    (that row, feature 16 h + fr)), rows 0-31 and 32-63 of the wave into partials of their
  //    own.  The record is ((((((p0 + p1) + p2) + p3) + p4) + p5) + p6) + p7 over the row
  //    block's eight 32-row parts: waves 0 and 1 hand over p0 .. p3, then waves 2 and 3 p4 ..
  //    p7, through the same four LDS slots; thread e keeps the running sums of its NH elements.
#pragma unroll
  for (int j = 0; j < FI; ++j) {
    // [x | 1] is re-read from LDS for every j: an opaque offset (not an opaque pointer, which
    // would lose the LDS address space) keeps the compiler from holding all 16 NH values of a
    // lane in registers across the j loop
    int xo = 0;
    asm volatile("" : "+s"(xo));
    const double* xj = xs + xo;
    d4 dacc[2][NH];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int h = 0; h < NH; ++h) dacc[hf][h] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 2 * hf; i < 2 * hf + 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int h = 0; h < NH; ++h)
            dacc[hf][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                acc[i][j][q],
                xj[(16 * i + 4 * q + g) * XW + 16 * (h ^ (g & 1 & (NH - 1))) + fr], dacc[hf][h],
                0, 0, 0);
    }
    // dacc[hf][h][r'] = sum over the half's rows of dz1[.][col0 + 16 j + g + 4 r'] *
    // [x | 1][16 h + fr]
    double run[NH];
#pragma unroll
    for (int rnd = 0; rnd < 2; ++rnd) {
      if ((w >> 1) == rnd) {  // uniform
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              red[(2 * (w & 1) + hf) * NE + (h * 4 + q) * 64 + (le & 63)] = dacc[hf][h][q];
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int e = le + kThreads * h;  // NE = kThreads NH
        double sum = rnd == 0 ? red[e] : run[h] + red[e];
#pragma unroll
        for (int v = 1; v < 4; ++v) sum += red[v * NE + e];
        run[h] = sum;
      }
      __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int e = le + kThreads * h;
      const int ll = e & 63, q = (e >> 6) & 3;  // (e >> 8 is h)
      const int cc = col0 + j * 16 + (ll >> 4) + 4 * q, f = 16 * h + (ll & 15);
      if (cc < M && f <= F) part[((int64_t)rb * M + cc) * (F + 1) + f] = run[h];
    }
  }
}

// ---- backward through a hidden layer (GaussianPolicy.net[2 l], l >= 1, src/policy.py:21-26) ---
// dz_in = (dz_out W) . relu'(h_in) for W [K][M] as stored (gemm_mainloop's BT form) and the
// layer's ReLU input h_in [N][M], plus the previous layer's bias gradient db_in[c] = sum_r
// dz_in[r][c].  The epilogue loads h_in at the accumulator positions, masks and stores dz_in,
// sums each lane's rows, the four row groups of a wave by two exchanges and the WR waves through
// LDS in wave order into the row block's record part[rb][M]; sum_records adds the records.
// Tiling: dh1's 8 waves x (32 rows x 80 cols) with the DEEP main loop.
namespace hbw {
constexpr int WR = 8, WC = 1, FR = 2, FC = 5;
using P = Cfg<WR, WC, FR, FC>;
constexpr int kGroups = 16;  // sum_records' groups of row blocks

inline int row_blocks(int64_t n) { return (int)((n + P::BM - 1) / P::BM); }
inline size_t ws_bytes(int64_t n, int m) {
  return sum_records_bytes<kGroups>(row_blocks(n), (size_t)m);
}

struct ScatterDb {
  double* db;
  __device__ void operator()(int64_t e, double t) const { db[e] = t; }
};
}  // namespace hbw

__global__ __launch_bounds__(hbw::P::kThreads) void hidden_bwd_kernel(
    const double* __restrict__ dz_out, int64_t N, int K, const double* __restrict__ W, int M,
    const double* __restrict__ h_in, double* __restrict__ dz_in, double* __restrict__ part) {
  using namespace hbw;
  constexpr int BM = P::BM, BN = P::BN;
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = frag_col(lane);
  const int ncb = (M + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rb = tile / ncb;
  const int64_t row0 = (int64_t)rb * BM;
  const int col0 = (tile % ncb) * BN;
  d4 acc[FR][FC];
  gemm_mainloop<WR, WC, FR, FC, true, true>(dz_out, N, K, K, W, M, M, row0, col0, lds, acc);

  // h_in at every accumulator element in ONE batch of unconditional loads (clamped addresses)
  // before the first use, as in dh1_layer1_bwd_kernel; rows and columns past the end are
  // zeroed by the mask below
  double hv[FC][FR][4];
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = row0 + wave * FR * 16 + i * 16 + frag_row(lane, q);
      const double* hr = h_in + min<int64_t>(r, N - 1) * M;
#pragma unroll
      for (int j = 0; j < FC; ++j) hv[j][i][q] = hr[min(col0 + j * 16 + fr, M - 1)];
    }
  double* red = lds;  // [WR][BN]; the main loop's last barrier retired its LDS reads
#pragma unroll
  for (int j = 0; j < FC; ++j) {
    const int c = col0 + j * 16 + fr;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = row0 + wave * FR * 16 + i * 16 + frag_row(lane, q);
        const bool in = r < N && c < M;
        const double v = (in && hv[j][i][q] > 0.0) ? acc[i][j][q] : 0.0;
        if (in) dz_in[r * M + c] = v;
        s += v;
      }
    // the wave's four row groups (lanes fr, fr + 16, fr + 32, fr + 48): the same bits in all
    s += __shfl_xor(s, 16, mepol::kWave);
    s += __shfl_xor(s, 32, mepol::kWave);
    if (lane < 16) red[wave * BN + j * 16 + fr] = s;
  }
  if (part) {  // uniform
    __syncthreads();
    const int t = threadIdx.x;
    if (t < BN && col0 + t < M) {
      double s = red[t];
#pragma unroll
      for (int w = 1; w < WR; ++w) s += red[w * BN + t];
      part[(int64_t)rb * M + col0 + t] = s;
    }
  }
}

// ---- tangent (forward-mode) pass through a hidden layer (TRPO's Fisher-vector product) --------
// t_out = (t_in W^T + h_in dW^T + db) . [mask_src + mask_bias > 0] for h_out = relu(h_in W^T + b):
// the directional derivative of h_out along (dW, db) given the tangent t_in of h_in.  Two operand
// pairs, (t_in, W) and (h_in, dW), both [.][K] row-major, run through gemm_mainloop one after the
// other into the same accumulators (the second with ZERO = false; the first loop's last barrier
// retired its LDS reads).  The epilogue loads the mask source at the accumulator positions in one
// batch of unconditional loads (clamped addresses) before the first use, as hidden_bwd_kernel.
// relu'(0) = 0 as torch: a pre-activation of exactly 0 gives t_out = 0.
template <int WR, int WC, int FR, int FC>
__global__ __launch_bounds__(WR * WC * 64) void hidden_tangent_kernel(
    const double* __restrict__ t_in, const double* __restrict__ h_in, int64_t N, int K,
    const double* __restrict__ W, const double* __restrict__ dW, const double* __restrict__ db,
    int M, const double* __restrict__ mask_src, const double* __restrict__ mask_bias,
    double* __restrict__ t_out) {
  using P = Cfg<WR, WC, FR, FC>;
  constexpr int BM = P::BM, BN = P::BN;
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int fr = frag_col(lane);
  const int ncb = (M + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int64_t row0 = (int64_t)(tile / ncb) * BM;
  const int col0 = (tile % ncb) * BN;
  d4 acc[FR][FC];
  gemm_mainloop<WR, WC, FR, FC>(t_in, N, K, K, W, M, K, row0, col0, lds, acc);
  gemm_mainloop<WR, WC, FR, FC, false, false, false>(h_in, N, K, K, dW, M, K, row0, col0, lds,
                                                     acc);

  double mv[FC][FR][4];
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = row0 + wr * FR * 16 + i * 16 + frag_row(lane, q);
      const double* mr = mask_src + min<int64_t>(r, N - 1) * M;
#pragma unroll
      for (int j = 0; j < FC; ++j) mv[j][i][q] = mr[min(col0 + wc * FC * 16 + j * 16 + fr, M - 1)];
    }
#pragma unroll
  for (int j = 0; j < FC; ++j) {
    const int c = col0 + wc * FC * 16 + j * 16 + fr;
    if (c >= M) continue;
    const double dbc = db[c];
    const double mb = mask_bias ? mask_bias[c] : 0.0;
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = row0 + wr * FR * 16 + i * 16 + frag_row(lane, q);
        if (r < N) t_out[r * M + c] = (mv[j][i][q] + mb > 0.0) ? acc[i][j][q] + dbc : 0.0;
      }
  }
}

template <int WR, int WC, int FR, int FC>
int launch_tangent(const double* t_in, const double* h_in, int64_t n, int k, const double* W,
                   const double* dW, const double* db, int m, const double* mask_src,
                   const double* mask_bias, double* t_out, hipStream_t st) {
  using P = Cfg<WR, WC, FR, FC>;
  MEPOL_HIP((max_dynamic_lds<hidden_tangent_kernel<WR, WC, FR, FC>>((int)P::kLds)));
  const int64_t tiles = (int64_t)((m + P::BN - 1) / P::BN) * ((n + P::BM - 1) / P::BM);
  hipLaunchKernelGGL((hidden_tangent_kernel<WR, WC, FR, FC>), dim3((unsigned)tiles),
                     dim3(P::kThreads), P::kLds, st, t_in, h_in, n, k, W, dW, db, m, mask_src,
                     mask_bias, t_out);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

template <int WR, int WC, int FR, int FC>
int launch_nt(const double* A, int64_t n, int k, int64_t lda, const double* B, int m,
              int64_t ldb, const double* bias, int relu, double* C, int64_t ldc,
              hipStream_t st) {
  using P = Cfg<WR, WC, FR, FC>;
  MEPOL_HIP((max_dynamic_lds<gemm_nt_kernel<WR, WC, FR, FC>>((int)P::kLds)));
  const int64_t tiles = (int64_t)((m + P::BN - 1) / P::BN) * ((n + P::BM - 1) / P::BM);
  hipLaunchKernelGGL((gemm_nt_kernel<WR, WC, FR, FC>), dim3((unsigned)tiles), dim3(P::kThreads), P::kLds, st, A,
                     n, k, lda, B, m, ldb, bias, relu, C, ldc);
  MEPOL_CHECK_LAUNCH();
  return 0;
}


}  // namespace gemm
}  // namespace mepol

using namespace mepol::gemm;

// C = act(A B^T + bias): A [n, k] (row stride lda), B [m, k] (row stride ldb), C [n, m] (row
// stride ldc), f64; k even and lda, ldb even (16-B operand loads).  `variant` picks the tiling
// (0 = default; others for tuning).
extern "C" int mepol_gemm_nt(const double* A, int64_t n, int k, int64_t lda, const double* B,
                             int m, int64_t ldb, const double* bias, int relu, double* C,
                             int64_t ldc, int variant, void* stream) {
  if (n < 0 || k <= 0 || m <= 0 || (k & 1) || (lda & 1) || (ldb & 1) || lda < k || ldb < k ||
      ldc < m || !A || !B || !C || ((uintptr_t)A & 15) || ((uintptr_t)B & 15)) {
    mepol::set_error("mepol_gemm_nt: bad arguments (k, lda, ldb even; 16-B aligned operands)");
    return mepol::kErrBadArg;
  }
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (variant) {
    case 0: return launch_nt<2, 2, 4, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 1: return launch_nt<4, 2, 2, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 2: return launch_nt<2, 2, 2, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 3: return launch_nt<4, 1, 2, 10>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 5: return launch_nt<2, 2, 4, 4>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 6: return launch_nt<2, 4, 2, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 7: return launch_nt<4, 1, 2, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 8: return launch_nt<2, 5, 2, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 9: return launch_nt<8, 1, 2, 5>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    case 10: return launch_nt<4, 2, 2, 4>(A, n, k, lda, B, m, ldb, bias, relu, C, ldc, st);
    default:
      mepol::set_error("mepol_gemm_nt: unknown variant %d", variant);
      return mepol::kErrBadArg;
  }
}


// dW1 [m, F], db1 [m] (nullable) of h1 = relu(x W1^T + b1) given dz2 [n, k] and W2t = W2^T
// [m, k] (dh1 = dz2 W2 = dz2 W2t^T, not materialised), the forward's h1 [n, m] and x [n, F].
extern "C" int mepol_dh1_layer1_workspace_size(int64_t n, int m, int in_features,
                                               size_t* bytes) {
  if (!bytes) return mepol::kErrBadArg;
  *bytes = mepol::gemm::l1b::ws_bytes(n, m, in_features);
  return 0;
}

// Host only (no GPU call): which kernel mepol_dh1_layer1_backward{,_masked,_w2,_form} launches
// at these sizes (mask: the bit-mask forms; w2: W2 as stored, which implies mask; ask: the form
// argument of mepol_dh1_layer1_backward_form, 0 for the other three calls), its grid and the
// layout of the workspace.
//   form            0 = the LDS kernel (dh1_layer1_bwd_kernel), 1 = the register-fed one
//   nh              16-column groups of [x | 1]
//   row_blocks, col_tiles   the grid is their product; tile (rb, ct) = xcd_tile(block)
//   threads, lds_bytes      of one workgroup
//   waves_per_block, rows_per_wave   a row block's record is the ordered sum of these waves
//   record_doubles  hidden0 (in_features + 1): one row block's record
//   group_offset    byte offset of sum_records' 16 group sums (after the row_blocks records)
//   ws_bytes        what mepol_dh1_layer1_workspace_size reports
extern "C" int mepol_dh1_layer1_plan_info(int64_t n, int k, int hidden0, int in_features, int mask,
                                          int w2, int ask, int* form, int* nh, int* row_blocks,
                                          int* col_tiles, int* threads, int* lds_bytes,
                                          int* waves_per_block, int* rows_per_wave,
                                          int64_t* record_doubles, size_t* group_offset,
                                          size_t* ws_bytes) {
  namespace B = mepol::gemm::l1b;
  namespace D = mepol::gemm::l1d;
  const int m = hidden0, F = in_features;
  if (n <= 0 || k <= 0 || (k & 1) || m <= 0 || F <= 0 || F > 63 || (w2 && (!mask || (m & 1))) ||
      ask < 0 || ask > 2 || !form || !nh || !row_blocks || !col_tiles || !threads || !lds_bytes || !waves_per_block ||
      !rows_per_wave || !record_doubles || !group_offset || !ws_bytes) {
    mepol::set_error("mepol_dh1_layer1_plan_info: bad arguments (n, k, hidden0 positive, k even, "
                     "in_features in 1..63, w2 only with mask and hidden0 even, ask in 0..2; "
                     "every output non-null)");
    return mepol::kErrBadArg;
  }
  if (ask == D::kDirect && !(mask && D::direct_fits(k, m, F))) {
    mepol::set_error("mepol_dh1_layer1_plan_info: the register-fed kernel is not available at "
                     "these sizes (mask forms, k and hidden0 even, in_features <= 31)");
    return mepol::kErrUnsupported;
  }
  const bool direct = mask && D::use_direct(ask, n, k, m, F);
  *form = direct ? 1 : 0;
  *nh = (F + 1 + 15) / 16;
  *row_blocks = B::row_blocks(n);
  *col_tiles = (m + B::P::BN - 1) / B::P::BN;
  *threads = direct ? D::kThreads : B::P::kThreads;
  *lds_bytes = direct ? (int)D::lds_bytes(*nh) : (int)B::P::kLds;
  *waves_per_block = direct ? D::NW : B::WR;
  *rows_per_wave = B::P::BM / *waves_per_block;
  *record_doubles = (int64_t)m * (F + 1);
  *group_offset = (size_t)*row_blocks * (size_t)*record_doubles * sizeof(double);
  *ws_bytes = B::ws_bytes(n, m, F);
  return 0;
}

template <bool MASK, bool BT = false>
static int dh1_layer1_backward(const double* dz2, int64_t n, int k, const double* W2t, int m,
                               const void* h1, const double* x, int in_features, double* dW1,
                               double* db1, void* workspace, size_t workspace_bytes,
                               void* stream, int form = 0) {
  using namespace mepol::gemm::l1b;
  using mepol::gemm::dh1_layer1_bwd_kernel;
  const int F = in_features;
  if (form < 0 || form > 2 || (form == 2 && !(MASK && F > 0 && k > 0 && m > 0 &&
                                              mepol::gemm::l1d::direct_fits(k, m, F)))) {
    mepol::set_error("mepol_dh1_layer1_backward: form %d is not available at these sizes (0 = "
                     "automatic, 1 = LDS kernel, 2 = register-fed kernel: k and hidden0 even, "
                     "in_features <= 31)", form);
    return form < 0 || form > 2 ? mepol::kErrBadArg : mepol::kErrUnsupported;
  }
  if (n <= 0 || k <= 0 || (k & 1) || m <= 0 || F <= 0 || F > 63 || !dz2 || !W2t || !h1 || !x ||
      !dW1 || !workspace || ((uintptr_t)dz2 & 15) || ((uintptr_t)W2t & 15) || (BT && (m & 1))) {
    mepol::set_error("mepol_dh1_layer1_backward: bad arguments (k even, in_features <= 63, "
                     "16-B aligned dz2 / W2t%s)",
                     BT ? "; the W2 form needs hidden0 even: 16-B aligned W2 rows" : "");
    return mepol::kErrBadArg;
  }
  const int nrb = row_blocks(n);
  const size_t need = ws_bytes(n, m, F);
  if (workspace_bytes < need) {
    mepol::set_error("mepol_dh1_layer1_backward: workspace %zu < %zu", workspace_bytes, need);
    return mepol::kErrWorkspace;
  }
  hipStream_t st = (hipStream_t)stream;
  const int ncb = (m + P::BN - 1) / P::BN;
  const unsigned tiles = (unsigned)((int64_t)nrb * ncb);
  double* part = (double*)workspace;
  const int nh = (F + 1 + 15) / 16;
  // The mask forms take the register-fed kernel where it fits (l1d::direct_fits: K and M even,
  // NH <= 2) and pays (l1d::direct_pays: more tiles than CUs), or where the caller asks for it.
  // Its resource report at NH = 1 and 2, both W2 forms: no scratch, no AGPRs, two waves per
  // SIMD.  NH = 3 and 4 would need 120 and 160 KB of LDS for the [x | 1] block, one workgroup
  // per CU, and are not instantiated: they, the f64-h1 form and odd sizes keep the LDS kernel.
  // Both kernels give the same bits.
  if constexpr (MASK) {
    if (mepol::gemm::l1d::use_direct(form, n, k, m, F)) {
      namespace D = mepol::gemm::l1d;
      using mepol::gemm::dh1_direct_kernel;
      const uint16_t* hm = static_cast<const uint16_t*>(h1);
#define MEPOL_L1D(NHV)                                                                         \
  do {                                                                                         \
    MEPOL_HIP((mepol::max_dynamic_lds<dh1_direct_kernel<NHV, BT>>((int)D::lds_bytes<NHV>())));  \
    hipLaunchKernelGGL((dh1_direct_kernel<NHV, BT>), dim3(tiles), dim3(D::kThreads),           \
                       D::lds_bytes<NHV>(), st, dz2, n, k, W2t, m, hm, x, F, part);            \
  } while (0)
      if (nh == 1)
        MEPOL_L1D(1);
      else
        MEPOL_L1D(2);
#undef MEPOL_L1D
      MEPOL_CHECK_LAUNCH();
      return mepol::sum_records<kGroups>(part, nrb, (int64_t)m * (F + 1), ScatterW1{F, dW1, db1},
                                         st);
    }
  }
#define MEPOL_L1B(NHV)                                                                        \
  do {                                                                                         \
    MEPOL_HIP((mepol::max_dynamic_lds<dh1_layer1_bwd_kernel<NHV, MASK, BT>>((int)P::kLds)));   \
    hipLaunchKernelGGL((dh1_layer1_bwd_kernel<NHV, MASK, BT>), dim3(tiles), dim3(P::kThreads),  \
                       P::kLds, st,                                                            \
                       dz2, n, k, W2t, m, h1, x, F, part);                                     \
  } while (0)
  switch (nh) {
    case 1: MEPOL_L1B(1); break;
    case 2: MEPOL_L1B(2); break;
    case 3: MEPOL_L1B(3); break;
    default: MEPOL_L1B(4); break;
  }
#undef MEPOL_L1B
  MEPOL_CHECK_LAUNCH();
  return mepol::sum_records<kGroups>(part, nrb, (int64_t)m * (F + 1), ScatterW1{F, dW1, db1}, st);
}

extern "C" int mepol_dh1_layer1_backward(const double* dz2, int64_t n, int k, const double* W2t,
                                         int m, const double* h1, const double* x,
                                         int in_features, double* dW1, double* db1,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return dh1_layer1_backward<false>(dz2, n, k, W2t, m, h1, x, in_features, dW1, db1, workspace,
                                    workspace_bytes, stream);
}

extern "C" int mepol_dh1_layer1_backward_masked(const double* dz2, int64_t n, int k,
                                                const double* W2t, int m,
                                                const uint16_t* h1_mask, const double* x,
                                                int in_features, double* dW1, double* db1,
                                                void* workspace, size_t workspace_bytes,
                                                void* stream) {
  return dh1_layer1_backward<true>(dz2, n, k, W2t, m, h1_mask, x, in_features, dW1, db1,
                                   workspace, workspace_bytes, stream);
}

extern "C" int mepol_dh1_layer1_backward_w2(const double* dz2, int64_t n, int k, const double* W2,
                                            int m, const uint16_t* h1_mask, const double* x,
                                            int in_features, double* dW1, double* db1,
                                            void* workspace, size_t workspace_bytes,
                                            void* stream) {
  return dh1_layer1_backward<true, true>(dz2, n, k, W2, m, h1_mask, x, in_features, dW1, db1,
                                         workspace, workspace_bytes, stream);
}

// The two mask forms (w2 == 0: W = W2^T [hidden0][k]; w2 != 0: W = W2 as stored) with the kernel
// chosen by the caller: form 0 = automatic (what the two calls above do), 1 = the LDS kernel,
// 2 = the register-fed kernel (MEPOL_ERR_UNSUPPORTED where it does not fit).  The same bits
// whichever runs.
extern "C" int mepol_dh1_layer1_backward_form(const double* dz2, int64_t n, int k, const double* W,
                                              int m, const uint16_t* h1_mask, const double* x,
                                              int in_features, double* dW1, double* db1,
                                              void* workspace, size_t workspace_bytes, int w2,
                                              int form, void* stream) {
  if (w2)
    return dh1_layer1_backward<true, true>(dz2, n, k, W, m, h1_mask, x, in_features, dW1, db1,
                                           workspace, workspace_bytes, stream, form);
  return dh1_layer1_backward<true>(dz2, n, k, W, m, h1_mask, x, in_features, dW1, db1, workspace,
                                   workspace_bytes, stream, form);
}


// Backward through a hidden layer: dz_in [n, in] = (dz_out W) . (h_in > 0) for dz_out [n, out]
// and W [out, in] as stored, db_in [in] (nullable) = the column sums of dz_in.
extern "C" int mepol_hidden_backward_workspace_size(int64_t n, int in_features, size_t* bytes) {
  if (!bytes || n < 0 || in_features <= 0) {
    mepol::set_error("mepol_hidden_backward_workspace_size: bad arguments (n >= 0, "
                     "in_features > 0, bytes non-null)");
    return mepol::kErrBadArg;
  }
  *bytes = mepol::gemm::hbw::ws_bytes(n, in_features);
  return 0;
}

extern "C" int mepol_hidden_backward(const double* dz_out, int64_t n, int out_features,
                                     const double* W, const double* h_in, int in_features,
                                     double* dz_in, double* db_in, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  using namespace mepol::gemm::hbw;
  const int k = out_features, m = in_features;
  if (n <= 0 || k <= 0 || m <= 0 || (k & 1) || (m & 1) || !dz_out || !W || !h_in || !dz_in ||
      !workspace || ((uintptr_t)dz_out & 15) || ((uintptr_t)W & 15)) {
    mepol::set_error("mepol_hidden_backward: bad arguments (n > 0; out_features and in_features "
                     "even and positive; dz_out, W, h_in, dz_in and workspace non-null; dz_out "
                     "and W 16-B aligned)");
    return mepol::kErrBadArg;
  }
  const int nrb = row_blocks(n);
  const size_t need = ws_bytes(n, m);
  if (workspace_bytes < need) {
    mepol::set_error("mepol_hidden_backward: workspace %zu < %zu", workspace_bytes, need);
    return mepol::kErrWorkspace;
  }
  hipStream_t st = (hipStream_t)stream;
  const int ncb = (m + P::BN - 1) / P::BN;
  const unsigned tiles = (unsigned)((int64_t)nrb * ncb);
  double* part = db_in ? (double*)workspace : nullptr;
  MEPOL_HIP((mepol::max_dynamic_lds<mepol::gemm::hidden_bwd_kernel>((int)P::kLds)));
  hipLaunchKernelGGL(mepol::gemm::hidden_bwd_kernel, dim3(tiles), dim3(P::kThreads), P::kLds, st,
                     dz_out, n, k, W, m, h_in, dz_in, part);
  MEPOL_CHECK_LAUNCH();
  if (!db_in) return 0;
  return mepol::sum_records<kGroups>(part, nrb, (int64_t)m, ScatterDb{db_in}, st);
}


// Tangent pass through a hidden layer h_out = relu(h_in W^T + b): t_out [n, m] = (t_in W^T +
// h_in dW^T + db) . [mask_src + mask_bias > 0] for t_in, h_in [n, k], W, dW [m, k] as stored,
// db [m], mask_src [n, m], mask_bias [m] (nullable).  `variant` as for mepol_gemm_nt.
extern "C" int mepol_hidden_tangent(const double* t_in, const double* h_in, int64_t n, int k,
                                    const double* W, const double* dW, const double* db, int m,
                                    const double* mask_src, const double* mask_bias,
                                    double* t_out, int variant, void* stream) {
  if (k <= 0 || m <= 0 || (k & 1) || !t_in || !h_in || !W || !dW || !db || !mask_src || !t_out ||
      ((uintptr_t)t_in & 15) || ((uintptr_t)h_in & 15) || ((uintptr_t)W & 15) ||
      ((uintptr_t)dW & 15)) {
    mepol::set_error("mepol_hidden_tangent: bad arguments (k even and positive, m positive; "
                     "t_in, h_in, W, dW, db, mask_src and t_out non-null; t_in, h_in, W and dW "
                     "16-B aligned)");
    return mepol::kErrBadArg;
  }
  const bool known = (variant >= 0 && variant <= 3) || (variant >= 5 && variant <= 10);
  if (!known) {
    mepol::set_error("mepol_hidden_tangent: unknown variant %d", variant);
    return mepol::kErrBadArg;
  }
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define MEPOL_TANGENT(WR, WC, FR, FC)                                                           \
  return launch_tangent<WR, WC, FR, FC>(t_in, h_in, n, k, W, dW, db, m, mask_src, mask_bias,    \
                                        t_out, st)
  switch (variant) {  // mepol_gemm_nt's tilings
    case 0: MEPOL_TANGENT(2, 2, 4, 5);
    case 1: MEPOL_TANGENT(4, 2, 2, 5);
    case 2: MEPOL_TANGENT(2, 2, 2, 5);
    case 3: MEPOL_TANGENT(4, 1, 2, 10);
    case 5: MEPOL_TANGENT(2, 2, 4, 4);
    case 6: MEPOL_TANGENT(2, 4, 2, 5);
    case 7: MEPOL_TANGENT(4, 1, 2, 5);
    case 8: MEPOL_TANGENT(2, 5, 2, 5);
    case 9: MEPOL_TANGENT(8, 1, 2, 5);
    default: MEPOL_TANGENT(4, 2, 2, 4);
  }
#undef MEPOL_TANGENT
}
