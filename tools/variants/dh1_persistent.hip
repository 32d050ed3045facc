// DROPPED (round 12, measured slower): dh1_layer1_bwd_kernel with persistent workgroups.  Every
// form passed tests/test_gpu_gemm.py, tests/test_gpu_kloop.py and tests/test_gpu_gemm_tiles.py
// (the h1, mask and stored-W2 forms torch.equal), but at C3 the kernel's own time was 996 us
// against 974 (1030 with the k loop unpeeled, which then spills 24 B), C3 102.3-102.8 ms per step
// against 101.6-101.8, and wgrad_reduce_kernel on the forked stream waited out the persistent
// workgroups (33 us -> 1.0 ms): profiles/r12/gemm_tiles/README.md.  Not built.
//
// Textually it replaced dh1_layer1_bwd_kernel in csrc/gemm.hip, inside namespace mepol::gemm:
// TileOps are gemm_mainloop's gload / lstore / compute lambdas as a struct (gemm_mainloop itself
// built on them compiles to the same registers for every kernel of the file); the launcher
// passed `tiles` as ntiles and took
//   grid = min(tiles, max(8, cu_count & ~7))
// so that a grid under the tile count is a multiple of 8 and a workgroup's tiles stay on
// xcd_tile's XCD.
#include "../../mepol_amd/csrc/mfma_f64.hpp"

// The k-tile steps of a workgroup tile (row0, col0) of C = A B^T, shared by the main loops below:
// global -> registers (gload), registers -> LDS (lstore), LDS -> MFMAs (compute).  Operand loads
// read clamped (always valid) addresses; out-of-range values are zeroed when the registers are
// written to LDS, after the MFMA block, so no select waits on a load right after issuing it.
// BT: B given as [K][M] row-major (ldb = its row stride, M even, 16-B aligned rows): a lane loads
// B[k][m, m + 1] (consecutive lanes consecutive m: coalesced) and writes the pair into LDS rows
// m and m + 1 of the [BN][KT] image (two 8-B stores).  Lets dh1 = dz2 W2 read the Linear weight
// as stored instead of a per-step W2^T copy.
template <int WR, int WC, int FR, int FC, bool BT>
struct TileOps {
  using P = Cfg<WR, WC, FR, FC>;
  static constexpr int T = P::kThreads, BM = P::BM, BN = P::BN;
  using RA = double2[P::PA];
  using RB = double2[P::PB];
  const double* __restrict__ A;
  const double* __restrict__ B;
  int64_t N, lda, ldb;
  int K, M, k2;  // k2: last 16-B aligned pair start (K even)
  double *sA, *sB;  // [2][BM][KP], [2][BN][KP]
  int tid, wr, wc, fr, sl0, sl1;

  __device__ __forceinline__ TileOps(const double* __restrict__ A_, int64_t N_, int K_,
                                     int64_t lda_, const double* __restrict__ B_, int M_,
                                     int64_t ldb_, double* lds, int tid_)
      : A(A_), B(B_), N(N_), lda(lda_), ldb(ldb_), K(K_), M(M_), k2(K_ - 2), sA(lds),
        sB(lds + 2 * BM * KP), tid(tid_) {
    const int lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    wr = wave / WC, wc = wave % WC, fr = lane & 15;
    // a lane's two slots in its fragment rows (every fragment row is fr mod 16: same swizzle)
    sl0 = 2 * lds_slot(fr, 2 * g), sl1 = 2 * lds_slot(fr, 2 * g + 1);
  }

  __device__ __forceinline__ void gload(int64_t row0, int col0, int kt, RA& ra, RB& rb) const {
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
  }

  __device__ __forceinline__ void lstore(int64_t row0, int col0, int kt, int buf, const RA& ra,
                                         const RB& rb) const {
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
  }

  __device__ __forceinline__ void compute(int buf, d4 (&acc)[FR][FC]) const {
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
  }
};


namespace l1b {
// Compute units of the current device, asked once (the library drives one device per process).
inline hipError_t cu_count(int* out) {
  static int cus = 0;
  static const hipError_t rc = [] {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return e;
  }();
  *out = cus;
  return rc;
}
}  // namespace l1b

// MASK: relu'(h1) comes as the forward's bit mask (uint16 word kt of row r holds
// h1[r][16 kt + b] > 0 in bit b, mepol_policy_forward_masked) instead of the f64 h1 values:
// 2 B per 16 columns instead of 128 B, which the epilogue waited for with the MFMAs idle
// (one workgroup per CU).  The same bits either way.
// BT: W2t is the Linear weight W2 as stored, [K][M] (TileOps' BT)
//
// Persistent: the grid is min(tiles, CUs) workgroups and workgroup b walks the tiles
// xcd_tile(t, ntiles), t = b, b + grid, ... (grid a multiple of 8 or the tile count itself, so
// a workgroup's tiles keep xcd_tile's XCD).  The assignment is static; a tile computes and
// writes exactly what a one-tile workgroup did.  With one workgroup per CU nothing else covers a
// tile's first loads and its epilogue's, so the walk issues them under MFMAs:
//   - the first k-tile of the NEXT tile is loaded (both register sets are dead by then) after
//     the last k-tile's MFMAs, ahead of the epilogue;
//   - EARLY_X: the epilogue's x loads are issued ahead of the last k-tile's MFMAs, where they fit
//     the 256-VGPR budget without scratch: the bit-mask forms up to NH = 2.
// The k-tile order of the main loop is gemm_mainloop's DEEP one.  Only the bit-mask forms up to
// NH = 3 compile without scratch as a walk; the others were launched one tile per workgroup.
template <int NH, bool MASK, bool BT>  // NH = ceil((F + 1) / 16) column groups of [x | 1]
__global__ __launch_bounds__(l1b::P::kThreads) void dh1_persistent_kernel(
    const double* __restrict__ dz2, int64_t N, int K, const double* __restrict__ W2t, int M,
    const void* __restrict__ h1v, const double* __restrict__ x, int F, int ntiles,
    double* __restrict__ part) {
  using namespace l1b;
  using Ops = TileOps<WR, WC, FR, FC, BT>;
  constexpr int BM = P::BM, BN = P::BN, T = P::kThreads;
  // x ahead of the last k-tile: 240 VGPRs at NH = 2.  The mask words instead: 242.  Both: 52 B of
  // scratch.  None of the three measured apart from the others.
  constexpr bool EARLY_X = MASK && NH <= 2;
  extern __shared__ double lds[];
  const int ncb = (M + BN - 1) / BN;
  const int nkt = (K + KT - 1) / KT;
  const double* h1 = static_cast<const double*>(h1v);
  const uint16_t* hm = static_cast<const uint16_t*>(h1v);
  const int mw = (M + 15) / 16;

  typename Ops::RA ra0, ra1;
  typename Ops::RB rb0, rb1;
  int t = blockIdx.x;  // < ntiles: the grid is no larger
  int tile = xcd_tile(t, ntiles);
  Ops(dz2, N, K, K, W2t, M, BT ? M : K, lds, threadIdx.x)
      .gload((int64_t)(tile / ncb) * BM, (tile % ncb) * BN, 0, ra0, rb0);
  for (;;) {
    // The thread index is made opaque per tile: every lane constant derived from it (chunk and
    // fragment offsets, epilogue indices) is then computed again for each tile, as a one-tile
    // workgroup did, instead of being hoisted out of the walk and held in registers through it
    // (hoisted, every form of the kernel spilled: 132 to 448 B of scratch per lane).
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const Ops ops(dz2, N, K, K, W2t, M, BT ? M : K, lds, tid);
    const int rb = tile / ncb;
    const int64_t row0 = (int64_t)rb * BM;
    const int col0 = (tile % ncb) * BN;
    d4 acc[FR][FC];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int j = 0; j < FC; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

    // Every epilogue operand in ONE batch of unconditional loads (clamped addresses) before the
    // first use: the ReLU mask of h1 at the wave's accumulator elements and the [x | 1] operands.
    // Loaded where they were used, the h1 loads waited out their HBM latency in FC batches
    // (0.40 of the kernel's 1.23 ms went to this epilogue, profiles/r5/f64/).
    // B operands [x | 1] for k-step (i, q): lane (fr, g) holds x[row(i, q, g)][16 h + fr]
    double xb[FR][4][NH];
    using HT = typename std::conditional<MASK, uint32_t, double>::type;
    HT hv[FC][FR][4];
    // accumulator element (row g + 4 q of fragment i, col fr) is A[m = fr][k = g] of k-step
    // (i, q): rows 16 i + 4 q + g
    auto x_loads = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t r = row0 + wave * FR * 16 + i * 16 + 4 * q + g;
          const double* xr = x + min<int64_t>(r, N - 1) * F;
#pragma unroll
          for (int h = 0; h < NH; ++h) xb[i][q][h] = xr[min(16 * h + fr, F - 1)];
        }
    };
    auto mask_loads = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t r = row0 + wave * FR * 16 + i * 16 + 4 * q + g;
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
    };

    // k-tile kt in buffer kt & 1, in gemm_mainloop's DEEP order with the last k-tile peeled;
    // ra0 / rb0 hold this tile's k-tile 0 on entry
    ops.lstore(row0, col0, 0, 0, ra0, rb0);
    if (nkt > 1) ops.gload(row0, col0, 1, ra1, rb1);
    __syncthreads();
    int kt = 0;
    for (; kt + 2 < nkt; kt += 2) {
      ops.gload(row0, col0, kt + 2, ra0, rb0);
      ops.compute(0, acc);
      ops.lstore(row0, col0, kt + 1, 1, ra1, rb1);
      __syncthreads();
      if (kt + 3 < nkt) ops.gload(row0, col0, kt + 3, ra1, rb1);
      ops.compute(1, acc);
      ops.lstore(row0, col0, kt + 2, 0, ra0, rb0);
      __syncthreads();
    }
    if (kt + 1 < nkt) {  // two k-tiles left
      ops.compute(0, acc);
      ops.lstore(row0, col0, kt + 1, 1, ra1, rb1);
      __syncthreads();
    }
    if constexpr (EARLY_X) {
      x_loads();
      __builtin_amdgcn_sched_barrier(0);  // the loads stay ahead of the MFMAs that cover them
    }
    ops.compute((nkt - 1) & 1, acc);
    const int tn = t + (int)gridDim.x;
    const int tile_n = tn < ntiles ? xcd_tile(tn, ntiles) : tile;
    if (tn < ntiles) {  // uniform
      ops.gload((int64_t)(tile_n / ncb) * BM, (tile_n % ncb) * BN, 0, ra0, rb0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!EARLY_X) x_loads();
    mask_loads();
    __syncthreads();  // the last k-tile's LDS reads are done: the epilogue reuses the buffers

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
    // 6 workgroup barriers instead of 10 for FC = 5); the per-element sum over the WR waves
    // keeps its order.
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
              const double dz = (on && c < M) ? acc[i][j][q] : 0.0;
#pragma unroll
              for (int h = 0; h < NH; ++h)
                dacc[h] =
                    __builtin_amdgcn_mfma_f64_16x16x4f64(dz, xb[i][q][h], dacc[h], 0, 0, 0);
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
      for (int e = tid; e < JB * NE; e += T) {
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
      __syncthreads();  // the last one also frees the buffers for the next tile's k-tile 0
    }
    if (tn >= ntiles) break;
    t = tn;
    tile = tile_n;
  }
}
