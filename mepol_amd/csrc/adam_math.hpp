// Element arithmetic of torch.optim.Adam's multi-tensor (foreach) step, one IEEE rounding per
// torch op (the tree builds with -ffp-contract=off); shared by adam_kernel (optim.hip) and
// critic_fit_kernel (critic_fit.hip):
//   m = m + (1-b1)(g - m)                       _foreach_lerp_ (weight < 0.5 branch)
//   v = v*b2;  v = v + (1-b2)(g*g)              _foreach_mul_, _foreach_addcmul_
//   d = sqrt(v) / bc2_sqrt + eps                _foreach_sqrt, _div_, _add_
//   p = p + (-step_size)(m / d)                 _foreach_addcdiv_
#pragma once
#include "common.hpp"

namespace mepol {
namespace optim {

// What one step shares over its elements: w1 = 1 - beta1, w2 = 1 - beta2, neg_step = -lr /
// bias_correction1, bc2_sqrt = sqrt(bias_correction2).
struct AdamStep {
  double w1, w2, b2, neg_step, bc2_sqrt, eps;
};

__device__ __forceinline__ AdamStep adam_step(double step_size, double bc2_sqrt, double b1,
                                              double b2, double eps) {
  return AdamStep{1.0 - b1, 1.0 - b2, b2, -step_size, bc2_sqrt, eps};
}

// One element in two halves, so that a caller can store the moments before the division of the
// second: the moments m, v updated in place from the gradient g, returning the denominator d;
// then the parameter from the new m and d.
__device__ __forceinline__ double adam_moments(const AdamStep& s, double g, double& m, double& v) {
  const double mi = m + s.w1 * (g - m);
  const double vi = v * s.b2 + s.w2 * (g * g);
  m = mi;
  v = vi;
  return sqrt(vi) / s.bc2_sqrt + s.eps;
}

__device__ __forceinline__ double adam_param(const AdamStep& s, double p, double m, double d) {
  return p + s.neg_step * (m / d);
}

// Both halves: gradient g, parameter p and moments m, v updated in place.
__device__ __forceinline__ void adam_element(const AdamStep& s, double g, double& p, double& m,
                                             double& v) {
  const double d = adam_moments(s, g, m, v);
  p = adam_param(s, p, m, d);
}

}  // namespace optim
}  // namespace mepol
