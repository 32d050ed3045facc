// MountainCar / GridWorld steps shared by the env kernels (envs.hip) and the deep rollout
// (rollout_deep.hip): the same IEEE operations, in the same order, as the reference's
// numpy / Python scalar code (see the header of envs.hip).
#pragma once
#include "common.hpp"

namespace mepol {
namespace envs {

// The reference's clips, min(max(a, lo), hi) in Python and np.clip: +-inf clips to the ends and a
// NaN action stays NaN, where fmin(fmax(a, lo), hi) alone returns lo.  Written as the two
// min / max instructions plus one unordered compare and select beside them, not as two ordered
// compares and selects: this sits on the serial tail of every rollout step, and the second form
// measured 0.09 us per step slower at [300, 300] (profiles/r18/rollout_ops).
__device__ __forceinline__ double clip_action(double a, double lo, double hi) {
  const double c = fmin(fmax(a, lo), hi);
  return a != a ? a : c;
}

struct MountainCar {
  static constexpr double kMinPos = -1.2, kMaxPos = 0.6, kMaxSpeed = 0.07, kGoal = 0.45;
  static constexpr double kPower = 0.0015;
  __device__ static void step(double& p, double& v, double a0) {
    const double force = clip_action(a0, -1.0, 1.0);
    // velocity += force*power - 0.0025*cos(3*position)
    const double t1 = __dmul_rn(force, kPower);
    const double t2 = __dmul_rn(0.0025, cos(__dmul_rn(3.0, p)));
    v = __dadd_rn(v, __dsub_rn(t1, t2));
    if (v > kMaxSpeed) v = kMaxSpeed;
    if (v < -kMaxSpeed) v = -kMaxSpeed;
    p = __dadd_rn(p, v);
    if (p > kMaxPos) p = kMaxPos;
    if (p < kMinPos) p = kMinPos;
    if (p == kMinPos && v < 0) v = 0.0;
    if (p > kGoal) {
      p = kGoal;
      v = 0.0;
    }
  }
};

struct GridWorld {
  static constexpr double kDim = 6.0, kMaxDelta = 0.2, kWall = 2.5;
  __device__ static bool inside(double x, double y, double x0, double x1, double y0, double y1) {
    return x0 <= x && x <= x1 && y0 <= y && y <= y1;
  }
  __device__ static void step(float& sx, float& sy, double ax, double ay) {
    const double dx = clip_action(ax, -kMaxDelta, kMaxDelta);
    const double dy = clip_action(ay, -kMaxDelta, kMaxDelta);
    const double x = (double)sx, y = (double)sy;
    double nx = __dadd_rn(x, dx), ny = __dadd_rn(y, dy);
    constexpr double h = kWall / 2;
    bool hit = inside(nx, ny, -h, h, -kWall, kWall) || inside(nx, ny, -kWall, -h, -h, h) ||
               inside(nx, ny, h, kWall, -h, h) || inside(nx, ny, -kDim, -(kDim - kWall), -h, h) ||
               inside(nx, ny, -h, h, -kDim, -(kDim - kWall)) ||
               inside(nx, ny, kDim - kWall, kDim, -h, h) ||
               inside(nx, ny, -h, h, kDim - kWall, kDim);
    if (hit) {
      nx = x;
      ny = y;
    }
    if (fabs(nx) >= kDim || fabs(ny) >= kDim) {
      nx = x;
      ny = y;
    }
    sx = (float)nx;
    sy = (float)ny;
  }
};

}  // namespace envs
}  // namespace mepol
