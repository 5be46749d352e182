// sfm_pose_rays.h -- what the operations on a relative pose of a pair of views share (sfm_twoview_pose.hip: the four
// candidates and their vote; sfm_twoview_refine.hip: the refinement of the winner): the rays of a match through the
// triangular intrinsics, the small vector algebra, the midpoint of the two rays of a match, and the host check of an
// intrinsic matrix.
//
// Compiled WITHOUT automatic contraction, the FMAs spelled out: include it after sfm_obs_test.h and sfm_match_norm.h.
#pragma once

#include <cmath>

#include "sfm_obs_test.h"
#include "sfm_match_norm.h"

namespace sfm {

struct PoseRays { double a0, a1, b0, b1; };

// (x, y, 1) = K (r0, r1, 1) solved from the bottom row up, K upper triangular with K[8] = 1.
__device__ __forceinline__ void pose_ray(const double* K, double x, double y, double& r0, double& r1) {
  r1 = (y - K[5]) / K[4];
  r0 = (__builtin_fma(-K[1], r1, x) - K[2]) / K[0];
}

// The rays of a match and whether all four of their components are finite.
__device__ __forceinline__ bool pose_rays_of(const double* Kl, const double* Kr, const TvMatch& m, PoseRays& r) {
  pose_ray(Kl, m.xl, m.yl, r.a0, r.a1);
  pose_ray(Kr, m.xr, m.yr, r.b0, r.b1);
  return ((r.a0 + r.a1 + r.b0 + r.b1) * 0.0) == 0.0;
}

__host__ __device__ inline bool pose_finite9(const double* m) {
  double probe = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) probe += m[k] * 0.0;
  return probe == 0.0;
}

__host__ __device__ inline void pose_cross(const double* u, const double* v, double* w) {
  w[0] = __builtin_fma(u[1], v[2], -(u[2] * v[1]));
  w[1] = __builtin_fma(u[2], v[0], -(u[0] * v[2]));
  w[2] = __builtin_fma(u[0], v[1], -(u[1] * v[0]));
}

__host__ __device__ inline double pose_dot(const double* u, const double* v) {
  return __builtin_fma(u[2], v[2], __builtin_fma(u[1], v[1], u[0] * v[0]));
}

// The midpoint of the two rays of a match in the right frame, taken back to the left one: P is R row-major, then t.  A
// value, not a decision.
__device__ __forceinline__ void pose_midpoint(const double* P, const PoseRays& r, double* X) {
  const PoseTerms w = pose_terms(P, P + 9, r.a0, r.a1, r.b0, r.b1);
  const double l1 = w.m1 / w.d, l2 = w.m2 / w.d;
  const double b[3] = {r.b0, r.b1, 1.0};
  double y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = 0.5 * (__builtin_fma(l1, w.ap[k], P[9 + k]) + l2 * b[k]) - P[9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = __builtin_fma(P[6 + k], y[2], __builtin_fma(P[3 + k], y[1], P[k] * y[0]));     // R^T (y - t)
}

// An intrinsic matrix the pose operations accept: finite, upper triangular, K[2][2] = 1.
inline int pose_check_k(const char* who, const char* name, const double* K) {
  if (K == nullptr) { set_error("%s: null %s", who, name); return SFM_E_SHAPE; }
  bool finite = true;
  for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(K[k]);
  if (!finite || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0) {
    set_error("%s: %s must be finite and upper triangular with %s[2][2] = 1", who, name, name);
    return SFM_E_SHAPE;
  }
  return SFM_OK;
}

}  // namespace sfm
