// sfm_ba_terms.h — the terms of one observation as a bundle-adjustment linearisation forms them, and the robust loss that
// reweights them: shared by the iteration kernels (sfm_ba.hip) and the motion-only refinement (sfm_ba_motion.hip).
#pragma once

#include "sfm_ba.h"

namespace sfm {

// Residual + Jacobians of one observation at the prepared camera (ba_processor.py:317-349).
__device__ __forceinline__ void obs_terms(const CamPrep& c, double X, double Y, double Z, double u, double v,
                                          int quirks, double* r, double* Jp, double* Jx) {
  double p[3];
  project_cam(c, X, Y, Z, 1.0, p);
  const double iz = rcp_nr(p[2]);        // one reciprocal (v_rcp_f64 + two Newton steps) per observation; f = p * iz (ba:339-342)
  jac_cam_iz(c, X, Y, Z, p, iz, quirks, Jp);
  jac_pt_cam_iz(c, p, iz, Jx);
  r[0] = u - p[0] * iz;        // b - f (ba:376)
  r[1] = v - p[1] * iz;
}

__device__ __forceinline__ void load_cam(CamPrep& dst, const CamPrep* src) {
  const double* s = reinterpret_cast<const double*>(src);
  double* d = reinterpret_cast<double*>(&dst);
#pragma unroll
  for (int k = 0; k < 19; ++k) d[k] = s[k];
}

// Robust loss (sfm_ba_set_loss) as a compile-time switch: LOSS = SFM_LOSS_NONE instantiates exactly the plain least-squares
// kernels (LossArg<0> is empty, obs_terms_loss<0> is obs_terms).  With a loss every observation's r, Jp, Jx are scaled
// by sqrt(w(s)), s = |b - f|^2 / delta^2 at the linearisation point: one IRLS step, no second-order correction.
template <int LOSS> struct LossArg { double inv_d2, d2; };      // 1 / delta^2, delta^2
template <> struct LossArg<SFM_LOSS_NONE> {};

// s -> w, sqrt(w), rho.  Huber: s <= 1 is the quadratic zone (w = 1 exactly, no reciprocal square root of 0);
// a NaN s fails the comparison and comes out as NaN weights, as a NaN residual does without a loss.
template <int LOSS>
__device__ __forceinline__ void loss_eval(double s, double& w, double& sw, double& rho) {
  if (LOSS == SFM_LOSS_HUBER) {
    if (s <= 1.0) { w = 1.0; sw = 1.0; rho = s; }
    else { const double q = sqrt(s); w = 1.0 / q; sw = 1.0 / sqrt(q); rho = 2.0 * q - 1.0; }
  } else {
    const double t = 1.0 + s;
    w = 1.0 / t; sw = 1.0 / sqrt(t); rho = log1p(s);
  }
}

// obs_terms, reweighted; rho_d2 = delta^2 rho(s), this observation's share of the robust cost.
template <int LOSS>
__device__ __forceinline__ void obs_terms_loss(const CamPrep& c, double X, double Y, double Z, double u, double v, int quirks,
                                               const LossArg<LOSS>& la, double* r, double* Jp, double* Jx, double& rho_d2) {
  obs_terms(c, X, Y, Z, u, v, quirks, r, Jp, Jx);
  if constexpr (LOSS != SFM_LOSS_NONE) {
    double w, sw, rho;
    loss_eval<LOSS>((r[0] * r[0] + r[1] * r[1]) * la.inv_d2, w, sw, rho);
    rho_d2 = la.d2 * rho;
    r[0] *= sw; r[1] *= sw;
#pragma unroll
    for (int k = 0; k < 14; ++k) Jp[k] *= sw;
#pragma unroll
    for (int k = 0; k < 6; ++k) Jx[k] *= sw;
  }
}

// the handle's loss as the kernel argument of its instantiation
template <int LOSS>
inline LossArg<LOSS> loss_arg(const sfm_ba_problem* p) {
  if constexpr (LOSS == SFM_LOSS_NONE) return {};
  else { const double d2 = p->loss_delta * p->loss_delta; return {1.0 / d2, d2}; }
}

}  // namespace sfm
