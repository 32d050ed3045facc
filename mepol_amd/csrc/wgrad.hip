// Weight gradient of a linear layer over a tall batch, dW = dy^T x (dy [n, O], x [n, I], both
// row-major f64; dW [O, I]): the policy's dW2 = dz2^T h1 (src/policy.py:21-26 Linear, its
// autograd weight gradient at mepol.py:278), K = n = the particle count.
//
// Split-K on the f64 matrix cores with no LDS and no barrier: both operands are read straight
// from L2 into the MFMA fragments, because with K running down the rows each fragment is whole
// cache lines -- v_mfma_f64_16x16x4f64 takes A[m][k] in lane (m = l & 15, k = l >> 4) and
// B[k][n] in lane (k, n = l & 15), i.e. dy[r0 + k][o0 + m] and x[r0 + k][i0 + n]: four rows of
// 16 consecutive doubles (4 x 128 B) per wave-instruction.  One wave owns a 64 (o) x 80 (i)
// output block (20 accumulators) over one K-slice, with the fragments of the next k-step
// in flight; the K-slices' partial blocks are summed in a fixed order by a second launch (the
// same bits every run).  The last o-block's tiles hold only the row fragments that reach below
// O and run proportionally longer K-slices (Plan below).  The tiles of one K-slice are
// dispatched back to back onto one XCD, so its rows come from HBM once and from that XCD's L2
// for the other tiles.  (That slice -> XCD map is not mfma::xcd_tile, which keeps the column
// tiles of one row block together: here the unit that shares rows is a whole K-slice, and
// slices, not tiles, are dealt round the XCDs.)
// d4 and the fragment map come from mfma_f64.hpp, and the K loop is its ring_k_loop, shared with
// z2_head_kernel (policy_fwd.hip).
//
// Replaces rocBLAS's split-K bmm + torch.sum (policy._weight_grad) on the off-policy
// iteration's dW2: 1.04 ms + reduce at C3 (46 TF/s on 48 GF).
#include "mfma_f64.hpp"

#include <algorithm>

namespace mepol {
namespace wgrad {

using mfma::d4;
using mfma::frag_col;
using mfma::frag_row;
constexpr int FO = 4, FI = 5;      // 16 x 16 fragments per wave: 64 (o) x 80 (i)
constexpr int kOcc = 2;            // waves per SIMD (VGPR budget 256)
constexpr int BO = 16 * FO, BI = 16 * FI;
// k-steps of operands in the register ring (3 spills at this tile).  Measured slower
// (tools/wgrad_probe.py, profiles/r5/f64/wgrad_probe.txt): 64 x 64 tiles with 3 stages, and
// 80 x 80 tiles at one wave per SIMD with 2 or 3 stages.
constexpr int NS = 2;
// ... and of a short tile (fewer than FO row fragments, see Plan): its k-step has 15, 10 or 5
// MFMAs behind 8, 7 or 6 loads, so one k-step of lookahead covers less of the load latency, and
// the registers of the third slot are free there.  C3 (3 fragments): 779 -> 761 us.  Tiles of 1
// and 2 fragments (O = 400, O = 17) take the same three slots and are not measured.
constexpr int kShortStages = 3;
// ring_k_loop's issue order is pinned: left to the scheduler, both slots' loads were issued back
// to back after the first MFMA block, and every second k-step began with no load lookahead.
// Pinned (profiles/r7/kloop/): 891 -> 800 us at C3.  A third stage (it fits in 235 VGPRs with
// the row addresses as a uniform base plus 32-bit lane offsets) measured no faster than two.
constexpr bool kPin = true;
constexpr int kMaxSlices = 128;
constexpr int kSliceRowsMin = 256;

// The launch plan.  The o-blocks 0 .. nob - 2 hold 4 row fragments ("full" tiles); the last one
// holds fol = 1 .. 4, the fragments that reach below O ("short" tiles: no MFMA multiplies a whole
// fragment of padding).  Each kind has its own K-slice count, Sf and Ss ~ Sf fol / 4, so a short
// tile's wave runs a proportionally longer slice and every wave has about the same MFMA count;
// together they fill one round of the 1024 SIMDs at the kernel's occupancy.  No slice is shorter
// than kSliceRowsMin rows, and no kind has fewer than 8 slices.
// Slice -> XCD map: workgroup b runs on XCD b % 8, and an XCD holds 1024 / 8 * kOcc waves.  XCD x
// runs nf[x] full slices (dealt round robin) and then as many short slices as still fit in its
// wave slots, the tiles of a slice back to back; the grid is 8 x the longest XCD's list, and the
// workgroups past an XCD's list exit at once.  The 8 XCDs of 256 wave slots are gfx950's, as
// constants: on a part with other numbers the map still gives every (slice, tile) to exactly one
// workgroup and the sums keep their order; only the one-round fit is lost.
struct XcdMap {  // per XCD: its list is [0, fend) full-tile waves, [fend, send) short ones,
  int fend[8], send[8], fbase[8], sbase[8];  // from its first full and short slice on
};
struct Plan {
  int nob, nib, fol;    // o-blocks, i-blocks, row fragments of the last o-block
  int Sf, Ss;           // K-slices of the full o-blocks (0 if there is none) and of the last one
  int64_t rows_f, rows_s;  // rows per slice: whole k-steps but the last
  int grid8;            // workgroups per XCD
  XcdMap m;
};
constexpr int kXcdWaves = 1024 / 8 * kOcc;

inline int64_t slice_rows_of(int64_t n, int S) { return ((n + S - 1) / S + 3) / 4 * 4; }

inline Plan plan_for(int64_t n, int O, int I) {
  Plan p{};
  p.nob = (O + BO - 1) / BO;
  p.nib = (I + BI - 1) / BI;
  p.fol = (O - BO * (p.nob - 1) + 15) / 16;
  const int nfo = p.nob - 1;
  const int64_t lim = std::max<int64_t>(8, n / kSliceRowsMin);
  const int64_t slots = 8 * kXcdWaves;
  int64_t want_s;
  if (nfo > 0) {
    // slots >= nib (nfo Sf + Ss) with Ss = Sf fol / 4
    const int64_t sf = 4 * slots / ((int64_t)p.nib * (4 * nfo + p.fol));
    p.Sf = (int)std::min<int64_t>({(int64_t)kMaxSlices, lim, std::max<int64_t>(8, sf)});
    // the XCD with one slice more than the others must still hold its full tiles in one round
    if ((int64_t)((p.Sf + 7) / 8) * nfo * p.nib > kXcdWaves) p.Sf = std::max(8, p.Sf & ~7);
    want_s = ((int64_t)p.Sf * p.fol + 3) / 4;
  } else {
    want_s = slots / p.nib;
  }
  want_s = std::min<int64_t>({(int64_t)kMaxSlices, lim, std::max<int64_t>(8, want_s)});
  const int tf = nfo * p.nib, ts = p.nib;
  int nf[8], cap[8], ns[8];
  int64_t capsum = 0;
  for (int x = 0; x < 8; ++x) {
    nf[x] = p.Sf / 8 + (x < p.Sf % 8 ? 1 : 0);
    cap[x] = std::max(0, (kXcdWaves - nf[x] * tf) / ts);
    capsum += cap[x];
    ns[x] = 0;
  }
  if (capsum < 8)  // more tiles than one round holds: the slots do not bind, deal evenly
    for (int x = 0; x < 8; ++x) cap[x] = kMaxSlices;
  else
    want_s = std::min(want_s, capsum);
  p.Ss = (int)want_s;
  // dealt from XCD 7 down: the XCDs with one full slice fewer come first
  for (int left = p.Ss, x = 7; left > 0; x = (x + 7) % 8)
    if (ns[x] < cap[x]) {
      ++ns[x];
      --left;
    }
  int fb = 0, sb = 0;
  for (int x = 0; x < 8; ++x) {
    p.m.fend[x] = nf[x] * tf;
    p.m.send[x] = p.m.fend[x] + ns[x] * ts;
    p.m.fbase[x] = fb;
    p.m.sbase[x] = sb;
    fb += nf[x];
    sb += ns[x];
    p.grid8 = std::max(p.grid8, p.m.send[x]);
  }
  p.rows_f = p.Sf ? slice_rows_of(n, p.Sf) : 0;
  p.rows_s = slice_rows_of(n, p.Ss);
  return p;
}

// the K-slices' partial blocks: [Sf][BO (nob - 1)][I] of the full o-blocks, then [Ss][the last
// o-block's rows][I]
inline size_t ws_bytes(int64_t n, int O, int I) {
  const Plan p = plan_for(n, O, I);
  const int64_t of = (int64_t)BO * (p.nob - 1);
  return (size_t)(p.Sf * of + p.Ss * (O - of)) * I * sizeof(double);
}

// One wave's block: FOV (o) x FI (i) fragments at (o0, ib) over the rows of K-slice s, into
// part[s][o - g0][i] of a [.][og][I] partial array (g0: the first row of the tile's kind).
template <int FOV>
__device__ __forceinline__ void wgrad_tile(const double* __restrict__ dy, int64_t n, int O,
                                           const double* __restrict__ x, int I, int o0, int g0,
                                           int og, int ib, int64_t s, int64_t slice_rows,
                                           double* __restrict__ part) {
  constexpr int NLV = FOV + FI;  // operand loads per lane and k-step
  constexpr int NS = FOV < FO ? kShortStages : wgrad::NS;
  const int l = threadIdx.x, fr = l & 15, g = l >> 4;
  const int64_t r_begin = s * slice_rows;
  const int64_t r_end = min(n, r_begin + slice_rows);
  if (r_begin >= r_end) {  // an empty slice still owns its partial block: zeros
    for (int t = 0; t < FOV; ++t)
      for (int q = 0; q < 4; ++q) {
        const int o = o0 + 16 * t + frag_row(l, q);
        for (int u = 0; u < FI; ++u) {
          const int i = ib * BI + 16 * u + frag_col(l);
          if (o < O && i < I) part[((int64_t)s * og + o - g0) * I + i] = 0.0;
        }
      }
    return;
  }
  // this lane's columns (clamped: columns past O / I only feed outputs that are not stored)
  int oc[FOV], ic[FI];
#pragma unroll
  for (int t = 0; t < FOV; ++t) oc[t] = min(o0 + 16 * t + fr, O - 1);
#pragma unroll
  for (int u = 0; u < FI; ++u) ic[u] = min(ib * BI + 16 * u + fr, I - 1);

  d4 acc[FOV][FI];
#pragma unroll
  for (int t = 0; t < FOV; ++t)
#pragma unroll
    for (int u = 0; u < FI; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};

  double R[NS][NLV];
  // k-step ks reads rows r_begin + 4 ks + (0..3); rows past the slice are clamped here and
  // zeroed at use (only the last k-step can hold them)
  auto load = [&](double (&D)[NLV], int64_t ks) __attribute__((always_inline)) {
    const int64_t r = min(r_begin + 4 * ks + g, r_end - 1);
    const double* yr = dy + r * O;
    const double* xr = x + r * I;
#pragma unroll
    for (int t = 0; t < FOV; ++t) D[t] = yr[oc[t]];
#pragma unroll
    for (int u = 0; u < FI; ++u) D[FOV + u] = xr[ic[u]];
  };
  auto mma = [&](const double (&D)[NLV]) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < FOV; ++t)
#pragma unroll
      for (int u = 0; u < FI; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[t], D[FOV + u], acc[t][u], 0, 0, 0);
  };
  const int64_t rows = r_end - r_begin;
  const int64_t nfull = rows / 4;  // k-steps with 4 rows in the slice
  const int64_t nks = (rows + 3) / 4;
  mfma::ring_k_loop<NS, kPin>(
      nfull, nks, [&](int p, int64_t ks) __attribute__((always_inline)) { load(R[p], ks); },
      [&](int p, int64_t ks) __attribute__((always_inline)) {
        const bool ok = r_begin + 4 * ks + g < r_end;  // rows past the slice end contribute zero
#pragma unroll
        for (int v = 0; v < NLV; ++v) R[p][v] = ok ? R[p][v] : 0.0;
      },
      [&](int p) __attribute__((always_inline)) { mma(R[p]); });
#pragma unroll
  for (int t = 0; t < FOV; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = o0 + 16 * t + frag_row(l, q);
#pragma unroll
      for (int u = 0; u < FI; ++u) {
        const int i = ib * BI + 16 * u + frag_col(l);
        if (o < O && i < I) part[((int64_t)s * og + o - g0) * I + i] = acc[t][u][q];
      }
    }
}

// One kernel for both kinds of tile: a wave takes the body compiled for its tile's row fragments
// (4 for a full tile, fol for one of the last o-block), a uniform branch.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kOcc))) void wgrad_kernel(
    const double* __restrict__ dy, int64_t n, int O, const double* __restrict__ x, int I,
    int nob, int nib, int fol, int Sf, int64_t rows_f, int64_t rows_s, XcdMap m,
    double* __restrict__ part) {
  // workgroup b is the j-th of XCD b % 8 under the round-robin dispatch
  const int xcd = blockIdx.x & 7;
  int j = blockIdx.x >> 3;
  const int of = BO * (nob - 1);  // rows of the full o-blocks
  int fo, o0, g0, og, ib;
  int64_t s, rows;
  if (j < m.fend[xcd]) {
    const int tf = (nob - 1) * nib, tile = j % tf;
    fo = FO, o0 = (tile / nib) * BO, g0 = 0, og = of, ib = tile % nib;
    s = m.fbase[xcd] + j / tf, rows = rows_f;
  } else if (j < m.send[xcd]) {
    j -= m.fend[xcd];
    fo = fol, o0 = of, g0 = of, og = O - of, ib = j % nib;
    s = m.sbase[xcd] + j / nib, rows = rows_s;
    part += (int64_t)Sf * of * I;
  } else {
    return;
  }
  if (fo == 4)
    wgrad_tile<4>(dy, n, O, x, I, o0, g0, og, ib, s, rows, part);
  else if (fo == 3)
    wgrad_tile<3>(dy, n, O, x, I, o0, g0, og, ib, s, rows, part);
  else if (fo == 2)
    wgrad_tile<2>(dy, n, O, x, I, o0, g0, og, ib, s, rows, part);
  else
    wgrad_tile<1>(dy, n, O, x, I, o0, g0, og, ib, s, rows, part);
}

// out[o][i] = sum over the K-slices s = 0 .. S - 1 of its o-block kind of part[s][o][i], in that
// order; the loads of eight slices are in flight at once, the adds stay sequential
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const double* __restrict__ part, int of,
                                                          int Sf, int Ss, int O, int I,
                                                          double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)O * I) return;
  const bool full = e < (int64_t)of * I;
  const int S = full ? Sf : Ss;
  const int64_t stride = (int64_t)(full ? of : O - of) * I;
  const double* p0 = full ? part + e : part + (int64_t)Sf * of * I + (e - (int64_t)of * I);
  double v = 0.0;
  for (int s = 0; s < S; s += 8) {  // the last batch may be short: clamped loads, skipped adds
    double p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = p0[min(s + u, S - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v = s + u < S ? v + p[u] : v;
  }
  out[e] = v;
}

}  // namespace wgrad
}  // namespace mepol

extern "C" int mepol_weight_grad_workspace_size(int64_t n, int out_features, int in_features,
                                                size_t* bytes) {
  if (!bytes || n < 0 || out_features <= 0 || in_features <= 0) return mepol::kErrBadArg;
  *bytes = mepol::wgrad::ws_bytes(n, out_features, in_features);
  return 0;
}

// Host only (no GPU call): the launch plan of mepol_weight_grad at these sizes.
extern "C" int mepol_weight_grad_plan_info(int64_t n, int out_features, int in_features, int* nob,
                                           int* nib, int* fol, int* Sf, int* Ss, int64_t* rows_f,
                                           int64_t* rows_s, int* grid8, int* fend, int* send,
                                           int* fbase, int* sbase) {
  if (n <= 0 || out_features <= 0 || in_features <= 0 || !nob || !nib || !fol || !Sf || !Ss ||
      !rows_f || !rows_s || !grid8 || !fend || !send || !fbase || !sbase) {
    mepol::set_error("mepol_weight_grad_plan_info: bad arguments (n, out_features, in_features "
                     "positive; every output non-null)");
    return mepol::kErrBadArg;
  }
  const mepol::wgrad::Plan p = mepol::wgrad::plan_for(n, out_features, in_features);
  *nob = p.nob, *nib = p.nib, *fol = p.fol, *Sf = p.Sf, *Ss = p.Ss;
  *rows_f = p.rows_f, *rows_s = p.rows_s, *grid8 = p.grid8;
  for (int x = 0; x < 8; ++x) {
    fend[x] = p.m.fend[x], send[x] = p.m.send[x];
    fbase[x] = p.m.fbase[x], sbase[x] = p.m.sbase[x];
  }
  return 0;
}

extern "C" int mepol_weight_grad(const double* dy, int64_t n, int out_features, const double* x,
                                 int in_features, double* dW, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  using namespace mepol::wgrad;
  const int O = out_features, I = in_features;
  if (n <= 0 || O <= 0 || I <= 0 || !dy || !x || !dW || !workspace) {
    mepol::set_error("mepol_weight_grad: bad arguments");
    return mepol::kErrBadArg;
  }
  const Plan p = plan_for(n, O, I);
  const size_t need = ws_bytes(n, O, I);
  if (workspace_bytes < need) {
    mepol::set_error("mepol_weight_grad: workspace %zu < %zu", workspace_bytes, need);
    return mepol::kErrWorkspace;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = 8u * (unsigned)p.grid8;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(wgrad_kernel, dim3(blocks), dim3(64), 0, st, dy, n, O, x, I, p.nob, p.nib,
                     p.fol, p.Sf, p.rows_f, p.rows_s, p.m, part);
  MEPOL_CHECK_LAUNCH();
  const int64_t elems = (int64_t)O * I;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st,
                     part, BO * (p.nob - 1), p.Sf, p.Ss, O, I, dW);
  MEPOL_CHECK_LAUNCH();
  return 0;
}
