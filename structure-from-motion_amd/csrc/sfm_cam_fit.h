// sfm_cam_fit.h -- one damped step of a camera over its own observations, the points held: the loader of an entry of a
// camera's list, the per-observation sums, their fold to slices of 64 consecutive observations and the serial 7x7 step.
// Shared as they are by the motion-only refinement (sfm_ba_motion.hip) and the refit of the robust resection
// (sfm_resect.hip), which differ in which observations they pass.  Compiled under the compiler's default contraction:
// include it ahead of sfm_obs_test.h.  The loop of a workgroup over 1 024 entries stays written out in its three kernels:
// under that contraction the operand order of their sums, and with it their bits, follows the shape of the code around
// mo_accumulate.
#pragma once

#include "sfm_ba_terms.h"

namespace sfm {

constexpr int kMoPerLane = 4;        // consecutive observations a lane keeps in registers: a slice (kCamSlice) is 16 lanes' worth
constexpr int kMoSums = 36;          // U lower triangle (28) | g (7) | cost share

struct MoObs { double u, v, X, Y, Z; };

// entry e of camera cam's list (CamObsView, sfm_ba.h); on request the camera's scale and the observation's index
__device__ __forceinline__ void cam_obs_load(const CamObsView& w, int cam, int e, MoObs& ob, double* scale = nullptr,
                                             int* index = nullptr) {
  const int o = w.obs ? w.obs[e] : e;
  const int p = w.obs_pt ? w.obs_pt[o] : o;
  ob.u = w.u[o]; ob.v = w.v[o];
  ob.X = w.px[p]; ob.Y = w.py[p]; ob.Z = w.pz[p];
  if (scale) *scale = w.cam_scale ? w.cam_scale[cam] : 1.0;
  if (index) *index = o;
}

// one observation into the 36 sums; behind: s[2] <= 0 at this camera
template <int LOSS>
__device__ __forceinline__ void mo_accumulate(const CamPrep& c, const MoObs& ob, int quirks, const LossArg<LOSS>& la,
                                              double (&acc)[kMoSums], int& behind) {
  double r[2], Jp[14], Jx[6], rho = 0;
  obs_terms_loss<LOSS>(c, ob.X, ob.Y, ob.Z, ob.u, ob.v, quirks, la, r, Jp, Jx, rho);
  if constexpr (LOSS == SFM_LOSS_NONE) rho = r[0] * r[0] + r[1] * r[1];
  double s[3];
  project_cam(c, ob.X, ob.Y, ob.Z, 1.0, s);
  behind |= s[2] <= 0.0 ? 1 : 0;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) { acc[k] += Jp[i] * Jp[j] + Jp[7 + i] * Jp[7 + j]; ++k; }
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[28 + i] += Jp[i] * r[0] + Jp[7 + i] * r[1];
  acc[35] += rho;
}

// which three of the 36 sums a lane holds after mo_fold_row
__device__ __forceinline__ void mo_fold_own(int lane, int (&own)[3]) {
  int i36[kMoSums], i18[18], i9[9], i5[5];
#pragma unroll
  for (int k = 0; k < kMoSums; ++k) i36[k] = k;
  fold_index(i36, i18, (lane & 8) != 0);
  fold_index(i18, i9, (lane & 4) != 0);
  fold_index(i9, i5, (lane & 2) != 0);
  fold_index(i5, own, (lane & 1) != 0);
}

// the 36 totals of a 16-lane row (one slice) -> row[36] in LDS (fold_half, sfm_common.h)
__device__ __forceinline__ void mo_fold_row(const double (&acc)[kMoSums], const int (&own)[3], int lane, double* row) {
  double f18[18], f9[9], f5[5], f3[3];
  fold_half<0x140>(acc, f18, (lane & 8) != 0);
  fold_half<0x141>(f18, f9, (lane & 4) != 0);
  fold_half<0x4E>(f9, f5, (lane & 2) != 0);
  fold_half<0xB1>(f5, f3, (lane & 1) != 0);
#pragma unroll
  for (int j = 0; j < 3; ++j) row[own[j]] = f3[j];
}

// 0.0 when every one of the n values is finite, NaN otherwise
__device__ __forceinline__ double mo_finite_probe(const double* v, int n) {
  double chk = 0;
  for (int k = 0; k < n; ++k) chk += v[k] * 0.0;
  return chk;
}

// The serial part, carried out by every thread on the same sums: dp = (U + lambda I)^-1 g, cam += dp, q /= |q|, and the next
// prepared camera.  The quaternion was normalised two lines up, so the determinant / inverse test of the rotation cannot
// fire (cam_prepare_dev<false>, sfm_common.h); false: a non-finite camera or qw ~ 0.
__device__ __forceinline__ bool mo_step(const double* sums, double lambda, double (&params)[7], CamPrep& c) {
  double a[28], b[7];
#pragma unroll
  for (int k = 0; k < 28; ++k) a[k] = sums[k];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    a[i * (i + 1) / 2 + i] += lambda;
    b[i] = sums[28 + i];
  }
  solve7_spd(a, b);
#pragma unroll
  for (int i = 0; i < 7; ++i) params[i] += b[i];
  const double inq = rsqrt_nr(params[3] * params[3] + params[4] * params[4] + params[5] * params[5] + params[6] * params[6]);
#pragma unroll
  for (int i = 3; i < 7; ++i) params[i] *= inq;
  const double chk = mo_finite_probe(params, 7);
  const int st = cam_prepare_dev<false>(params, &c);
  return st == SFM_OK && chk == 0.0;
}

}  // namespace sfm
