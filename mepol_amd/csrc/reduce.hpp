// Fixed-order sum of per-block partial records (nb records of m doubles, one after another) in
// two stages: one block column per 64 elements with all records serial per wave was
// latency-bound (79 us for 782 x 12000 partials).  Stage 1 sums record group g (G strided
// groups: records g, g + G, ...) for 64 elements per block; stage 2 adds the G group sums in
// order and hands element e's total to scatter(e, total).  G, the grids and the order of the
// additions decide the bits: the same result every run.
#pragma once
#include "common.hpp"

namespace mepol {

template <int G>
__global__ __launch_bounds__(256) void sum_records_kernel(const double* __restrict__ part, int nb,
                                                          int64_t m, double* __restrict__ grp) {
  __shared__ double sh[4][64];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + l;
  const int gi = blockIdx.y;
  double s = 0.0;
  if (e < m)  // wave w takes every fourth record of the group; the 4 wave sums add in order
    for (int b = gi + G * w; b < nb; b += 4 * G) s += part[(int64_t)b * m + e];
  sh[w][l] = s;
  __syncthreads();
  if (w == 0 && e < m) grp[(int64_t)gi * m + e] = ((sh[0][l] + sh[1][l]) + sh[2][l]) + sh[3][l];
}

template <int G, typename Scatter>
__global__ __launch_bounds__(256) void sum_groups_kernel(const double* __restrict__ grp, int64_t m,
                                                         Scatter scatter) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  double t = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) t += grp[(int64_t)g * m + e];
  scatter(e, t);
}

// bytes of nb records of m doubles followed by the G group sums
template <int G>
inline size_t sum_records_bytes(int64_t nb, size_t m) {
  return ((size_t)nb + G) * m * sizeof(double);
}

// part: nb records, then room for the G group sums (sum_records_bytes)
template <int G, typename Scatter>
int sum_records(const double* part, int nb, int64_t m, Scatter scatter, hipStream_t st) {
  double* grp = const_cast<double*>(part) + (size_t)nb * m;
  hipLaunchKernelGGL(sum_records_kernel<G>, dim3((unsigned)((m + 63) / 64), G), dim3(256), 0, st,
                     part, nb, m, grp);
  MEPOL_CHECK_LAUNCH();
  hipLaunchKernelGGL((sum_groups_kernel<G, Scatter>), dim3((unsigned)((m + 255) / 256)), dim3(256),
                     0, st, grp, m, scatter);
  MEPOL_CHECK_LAUNCH();
  return 0;
}

}  // namespace mepol
