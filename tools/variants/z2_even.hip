// DROPPED (round 12, measured slower): z2_head_kernel<4> with hidden1's column fragments dealt
// evenly over the four waves.  Correct (tests/test_gpu_gemm_tiles.py and
// test_policy_forward_kernel_matches_torch pass with it, z2 torch.equal to the 32- and 16-row
// kernels), but it does not fit the 256-VGPR budget of two waves per SIMD: at NX = 3 (hidden1 =
// 300) the gfx950 resource report gives 256 VGPRs and 292 B of scratch per lane, with scratch
// loads and stores of operands inside the K loop (812 B with ring_k_loop pinned; NX = 0 and 1 fit
// in 220 and 250 VGPRs, NX = 2 spills 24 B, NX = 4 340 B).  At C3 the kernel takes 1611 / 1623 /
// 1614 us against 880 / 885 / 884 for z2_head_kernel<4>, and C3 126.3 / 126.3 / 126.1 ms per step
// against 101.9 / 101.5 / 102.3 (profiles/r12/gemm_tiles/README.md).  Not built.
//
// It was textually included into namespace mepol::pfwd of csrc/policy_fwd.hip, after
// z2_head_kernel, and launch_split called launch_z2_even(H2, blocks, st, <the kernel's
// arguments>) in place of MEPOL_Z2(4) for the 64-row tile.
//
// z2_head_kernel gives wave w the column fragments 5 w .. 5 w + 4 of all four row fragments: 20
// fragments for hidden1 = 300, whose 19th is the last that holds a column.  Here wave w owns the
// column fragments 4 w .. 4 w + 3 of all four row fragments and, of the fragments from 16 upward
// (NX = ceil(hidden1 / 16) - 16 of them), those of row fragment w alone: 16 + NX accumulators,
// 2 (16 + NX) MFMAs per stage (38 against 40 at NX = 3) and 4 + 4 + NX operand pairs per stage,
// whichever SIMD a wave lands on.
// Registers: ring slot t of the A operand holds row fragment (t + w) & 3, so the extra fragments
// always multiply slot 0 and no operand is picked by a wave-dependent index; operand addresses
// are a uniform base plus a 32-bit lane offset (11 registers where 11 pointers would take 22).
// Head epilogue: a row's mean is the four waves' partials over their 64 columns in wave order,
// then the extra fragments' partials in fragment order.  That is NOT z2_head_kernel's order
// (partials over 80 columns), so mu and logp differ in their last bits from the 32- and 16-row
// kernels; z2 keeps its bits (every accumulator is its own chain over the same k order).  A
// version to merge would also need that order in the 32- and 16-row kernels
// (tests/test_gpu_small_batch.py holds mu and logp torch.equal across the tiles), and to skip
// the whole fragments past a narrow hidden1, which this one still multiplies.
namespace zh {
constexpr int FC = 4;  // column fragments a wave owns in every row fragment
}

template <int NX>
__global__ __launch_bounds__(64 * zh::NW) __attribute__((amdgpu_waves_per_eu(zh::kOcc))) void
z2_head_even_kernel(const double* __restrict__ h1, int64_t N, int H1, const double* __restrict__ W2,
                    const double* __restrict__ b2, int H2, const double* __restrict__ Wm,
                    const double* __restrict__ bm, const double* __restrict__ log_std,
                    const double* __restrict__ act, int A, double* __restrict__ z2_out,
                    double* __restrict__ mu_out, double* __restrict__ logp_out) {
  constexpr int FO = 4, FC = zh::FC, NW = zh::NW, NS = zh::NS, NB = FC + NX, NL = FO + NB;
  constexpr int ZM = 16 * FO, AC = 4;
  __shared__ double sMu[(NW + NX) * ZM * AC];
  const int tid = threadIdx.x, l = tid & 63, fr = l & 15, g = l >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * ZM;
  const int last = (int)min<int64_t>(N - 1 - row0, ZM - 1);  // last row of the block that exists
  const char* abase = reinterpret_cast<const char*>(h1 + row0 * H1);
  const char* bbase = reinterpret_cast<const char*>(W2);
  uint32_t ao[FO], bo[NB];  // byte offsets of the lane's 16-B pair at k = 0
#pragma unroll
  for (int t = 0; t < FO; ++t)
    ao[t] = 8u * (uint32_t)(min(16 * ((t + w) & 3) + fr, last) * H1 + 2 * g);
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int c = u < FC ? 16 * (FC * w + u) + fr : 16 * (FC * NW + u - FC) + fr;
    bo[u] = 8u * (uint32_t)(min(c, H2 - 1) * H1 + 2 * g);
  }
  d4 acc[FO][FC], accx[NX > 0 ? NX : 1];
#pragma unroll
  for (int t = 0; t < FO; ++t)
#pragma unroll
    for (int u = 0; u < FC; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int e = 0; e < NX; ++e) accx[e] = d4{0.0, 0.0, 0.0, 0.0};
  const int nst = (H1 + 7) / 8, nfull = H1 / 8;
  double2 R[NS][NL];
  auto load = [&](double2 (&D)[NL], int st) __attribute__((always_inline)) {
    const uint32_t kb = 8u * (uint32_t)min(8 * st, H1 - 2 - 2 * g);  // k + 2 g <= H1 - 2
#pragma unroll
    for (int t = 0; t < FO; ++t) D[t] = *reinterpret_cast<const double2*>(abase + (ao[t] + kb));
#pragma unroll
    for (int u = 0; u < NB; ++u)
      D[FO + u] = *reinterpret_cast<const double2*>(bbase + (bo[u] + kb));
  };
  auto mma = [&](const double2 (&D)[NL]) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < FO; ++t)
#pragma unroll
      for (int u = 0; u < FC; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[t].x, D[FO + u].x, acc[t][u], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < NX; ++e)
      accx[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[0].x, D[FO + FC + e].x, accx[e], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < FO; ++t)
#pragma unroll
      for (int u = 0; u < FC; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[t].y, D[FO + u].y, acc[t][u], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < NX; ++e)
      accx[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[0].y, D[FO + FC + e].y, accx[e], 0, 0, 0);
  };
  mfma::ring_k_loop<NS, false>(
      nfull, nst, [&](int p, int st) __attribute__((always_inline)) { load(R[p], st); },
      [&](int p, int st) __attribute__((always_inline)) {
        if (8 * st + 2 * g >= H1) {  // the tail stage's missing pairs
#pragma unroll
          for (int v = 0; v < NL; ++v) R[p][v] = double2{0.0, 0.0};
        }
      },
      [&](int p) __attribute__((always_inline)) { mma(R[p]); });

  // ---- epilogue: z2 out, then the head on relu(z2 + b2) ------------------------------------
  double b2v[FC], b2x[NX > 0 ? NX : 1];
#pragma unroll
  for (int u = 0; u < FC; ++u) {
    const int c = 16 * (FC * w + u) + fr;
    b2v[u] = c < H2 ? b2[c] : 0.0;
#pragma unroll
    for (int t = 0; t < FO; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = row0 + 16 * ((t + w) & 3) + g + 4 * q;
        if (c < H2 && r < N) z2_out[r * H2 + c] = acc[t][u][q];
      }
  }
#pragma unroll
  for (int e = 0; e < NX; ++e) {
    const int c = 16 * (FC * NW + e) + fr;
    b2x[e] = c < H2 ? b2[c] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = row0 + 16 * w + g + 4 * q;
      if (c < H2 && r < N) z2_out[r * H2 + c] = accx[e][q];
    }
  }
  const int er = tid >> 2, ea = tid & 3;  // combine step: row er of the block, action slot ea
  double lp = 0.0;
  for (int a0 = 0; a0 < A; a0 += AC) {
    double wmv[FC][AC], wmx[NX > 0 ? NX : 1][AC];
#pragma unroll
    for (int u = 0; u < FC; ++u) {
      const int c = 16 * (FC * w + u) + fr;
#pragma unroll
      for (int a = 0; a < AC; ++a)
        wmv[u][a] = (c < H2 && a0 + a < A) ? Wm[(int64_t)(a0 + a) * H2 + c] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
      const int c = 16 * (FC * NW + e) + fr;
#pragma unroll
      for (int a = 0; a < AC; ++a)
        wmx[e][a] = (c < H2 && a0 + a < A) ? Wm[(int64_t)(a0 + a) * H2 + c] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < FO; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double p[AC];
#pragma unroll
        for (int a = 0; a < AC; ++a) p[a] = 0.0;
#pragma unroll
        for (int u = 0; u < FC; ++u) {
          const double rv = fmax(acc[t][u][q] + b2v[u], 0.0);
#pragma unroll
          for (int a = 0; a < AC; ++a) p[a] = fma(rv, wmv[u][a], p[a]);
        }
        int comp;
        const double v = mfma::reduce_scatter_g<AC, 16>(p, fr, comp);
        if ((fr & 3) == 0) sMu[(w * ZM + 16 * ((t + w) & 3) + g + 4 * q) * AC + comp] = v;
      }
#pragma unroll
    for (int e = 0; e < NX; ++e)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double p[AC];
        const double rv = fmax(accx[e][q] + b2x[e], 0.0);
#pragma unroll
        for (int a = 0; a < AC; ++a) p[a] = rv * wmx[e][a];
        int comp;
        const double v = mfma::reduce_scatter_g<AC, 16>(p, fr, comp);
        if ((fr & 3) == 0) sMu[((NW + e) * ZM + 16 * w + g + 4 * q) * AC + comp] = v;
      }
    __syncthreads();
    {
      const int a = a0 + ea;
      const int64_t r = row0 + er;
      double term = 0.0;
      if (a < A && r < N) {
        double m = sMu[(0 * ZM + er) * AC + ea];
#pragma unroll
        for (int v = 1; v < NW + NX; ++v) m += sMu[(v * ZM + er) * AC + ea];
        m += bm[a];
        const double lsa = log_std[a];
        const double sd = exp(lsa) + kStdEps;
        const double d = act[r * A + a] - m;
        mu_out[r * A + a] = m;
        term = -0.5 * (kLog2Pi + 2.0 * lsa + d * d / (sd * sd));
      }
      term += __shfl_xor(term, 2, kWave);
      term += __shfl_xor(term, 1, kWave);
      lp += term;
    }
    __syncthreads();
  }
  if (ea == 0 && row0 + er < N) logp_out[row0 + er] = lp;
}

template <typename... Args>
void launch_z2_even(int H2, unsigned blocks, hipStream_t st, Args... args) {
  const int nx = (H2 + 15) / 16 - zh::FC * zh::NW;
#define MEPOL_Z2_EVEN_LAUNCH(NXV)                                                         \
  hipLaunchKernelGGL(z2_head_even_kernel<NXV>, dim3(blocks), dim3(64 * zh::NW), 0, st, args...)
  switch (nx < 0 ? 0 : nx) {
    case 0: MEPOL_Z2_EVEN_LAUNCH(0); break;
    case 1: MEPOL_Z2_EVEN_LAUNCH(1); break;
    case 2: MEPOL_Z2_EVEN_LAUNCH(2); break;
    case 3: MEPOL_Z2_EVEN_LAUNCH(3); break;
    default: MEPOL_Z2_EVEN_LAUNCH(4); break;
  }
#undef MEPOL_Z2_EVEN_LAUNCH
}
