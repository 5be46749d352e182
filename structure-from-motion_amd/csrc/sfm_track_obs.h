// sfm_track_obs.h — the per-observation arithmetic of the ragged-track kernels (sfm_tri_tracks.hip, sfm_tri_ransac.hip).
//
// Everything here is compiled WITHOUT automatic contraction and spells its FMAs out: every kernel that includes it
// executes the same operations per observation, so a point's bits do not depend on which instantiation serves it.
// The pragma stays in force for the rest of the translation unit: include this header AFTER the code that is to keep the
// default contraction (tri_tracks_linear_kernel), outside any namespace.  The residual is sfm_obs_test.h's.
#pragma once

#include "sfm_obs_test.h"      // contraction is off from here on

namespace sfm {

struct TrackSums { double a00, a10, a11, a20, a21, a22, b0, b1, b2, c; };

__device__ __forceinline__ void track_project(const double* P, double x0, double x1, double x2, double x3, double* s) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    s[r] = __builtin_fma(P[4 * r + 3], x3, __builtin_fma(P[4 * r + 2], x2, __builtin_fma(P[4 * r + 1], x1, P[4 * r] * x0)));
}

// One observation of the linearisation: tri_nonlinear_kernel's `view` (tri:209-228, 261-269) plus the squared residual.
// 97 flops (FMA = 2, v_rcp_f64 = 1): projection 21, reciprocal 7, iz^2 1, Jacobian 24, residual 4, sums 36, cost 4.
__device__ __forceinline__ void track_view(const double* P, double ku, double kv, double x0, double x1, double x2, double x3,
                                           TrackSums& S) {
  double s[3], j[6];
  track_project(P, x0, x1, x2, x3, s);
  const double iz = obs_inv_depth(s), iz2 = iz * iz;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    j[c] = __builtin_fma(-s[0], P[8 + c], s[2] * P[c]) * iz2;
    j[3 + c] = __builtin_fma(-s[1], P[8 + c], s[2] * P[4 + c]) * iz2;
  }
  double eu, ev;
  obs_residual(s, ku, kv, eu, ev);      // (divides by the same reciprocal: it is formed once)
  S.a00 = __builtin_fma(j[3], j[3], __builtin_fma(j[0], j[0], S.a00));
  S.a10 = __builtin_fma(j[4], j[3], __builtin_fma(j[1], j[0], S.a10));
  S.a11 = __builtin_fma(j[4], j[4], __builtin_fma(j[1], j[1], S.a11));
  S.a20 = __builtin_fma(j[5], j[3], __builtin_fma(j[2], j[0], S.a20));
  S.a21 = __builtin_fma(j[5], j[4], __builtin_fma(j[2], j[1], S.a21));
  S.a22 = __builtin_fma(j[5], j[5], __builtin_fma(j[2], j[2], S.a22));
  S.b0 = __builtin_fma(j[3], ev, __builtin_fma(j[0], eu, S.b0));
  S.b1 = __builtin_fma(j[4], ev, __builtin_fma(j[1], eu, S.b1));
  S.b2 = __builtin_fma(j[5], ev, __builtin_fma(j[2], eu, S.b2));
  S.c = __builtin_fma(ev, ev, __builtin_fma(eu, eu, S.c));
}

// The residual alone (the evaluation after the last iteration): the same eu / ev as track_view, and s[2] <= 0.
__device__ __forceinline__ void track_residual(const double* P, double ku, double kv, double x0, double x1, double x2,
                                               double x3, double& c, double& behind) {
  double s[3];
  track_project(P, x0, x1, x2, x3, s);
  double eu, ev;
  obs_residual(s, ku, kv, eu, ev);
  c = __builtin_fma(ev, ev, __builtin_fma(eu, eu, c));
  if (s[2] <= 0.0) behind += 1.0;
}

// d = A^-1 b for the symmetric 3x3 A = (a00; a10 a11; a20 a21 a22) by the adjugate (np.linalg.inv in the reference,
// tri:227).  False for a zero determinant or a non-finite solution.
__device__ __forceinline__ bool track_solve3(double a00, double a10, double a11, double a20, double a21, double a22, double b0,
                                             double b1, double b2, double& d0, double& d1, double& d2) {
  const double c00 = a11 * a22 - a21 * a21;
  const double c10 = a20 * a21 - a10 * a22;
  const double c20 = a10 * a21 - a20 * a11;
  const double det = a00 * c00 + a10 * c10 + a20 * c20;
  const double id = rcp_nr(det);
  const double c11 = a00 * a22 - a20 * a20;
  const double c21 = a10 * a20 - a00 * a21;
  const double c22 = a00 * a11 - a10 * a10;
  d0 = (c00 * b0 + c10 * b1 + c20 * b2) * id;
  d1 = (c10 * b0 + c11 * b1 + c21 * b2) * id;
  d2 = (c20 * b0 + c21 * b1 + c22 * b2) * id;
  return !(det == 0.0 || !isfinite(d0) || !isfinite(d1) || !isfinite(d2));
}

}  // namespace sfm
