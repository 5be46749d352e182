// sfm_ba_terms.h — the terms of one observation as a bundle-adjustment linearisation forms them, and the robust loss that
// reweights them, plus the device pieces more than one operation on the resident scene uses as they are: the loss dispatch,
// the slices of the camera-major list, the packed 3x3 point block and the per-point cost reduction.  Shared by the iteration
// kernels (sfm_ba.hip), the motion-only refinement (sfm_ba_motion.hip), the covariance (sfm_ba_cov.hip) and the
// matrix-free PCG (sfm_ba_pcg.hip).
#pragma once

#include <type_traits>

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

// The step from a run-time loss kind to a template argument, as dispatch_group does for the group width:
// f(std::integral_constant<int, LOSS>()), the plain instantiation for anything that is not a loss.
template <class F>
inline auto dispatch_loss(int kind, F&& f) {
  switch (kind) {
    case SFM_LOSS_HUBER: return f(std::integral_constant<int, SFM_LOSS_HUBER>());
    case SFM_LOSS_CAUCHY: return f(std::integral_constant<int, SFM_LOSS_CAUCHY>());
    default: return f(std::integral_constant<int, SFM_LOSS_NONE>());
  }
}

// ---- slices of the camera-major list: kCamSlice consecutive entries of one camera, one workspace row each ----
constexpr int kCamSlice = 64;
template <class T> __host__ __device__ inline T cam_slice_count(T n) { return (n + kCamSlice - 1) / kCamSlice; }      // in n's own width
// First workspace row of camera `cam`, whose list starts at entry `base`: camera k has at most n_k / 64 + 1 slices, so the
// rows of the cameras before it end at or before base / 64 + cam -- no scan is needed and no two cameras share a row.
__host__ __device__ inline size_t cam_slice_first_row(int base, int cam) { return (size_t)(base / kCamSlice) + cam; }
// ... and the rows that numbering needs for M entries and V cameras
inline size_t cam_slice_rows(long long M, int V) { return (size_t)(M / kCamSlice) + V + 1; }

// ---- the 3x3 block D_p of a point, packed (xx xy xz yy yz zz) ----
// The last pivot of its Cholesky factor must exceed this share of a22: a rank-2 block (one observation, lambda = 0) leaves
// rounding noise there.
constexpr double kPtPivotTol = 1e-14;

// D^-1 = L^-T L^-1 from li = L^-1 = (i00 i10 i11 i20 i21 i22)
__device__ __forceinline__ void sym3_from_li(const double* li, double* di) {
  di[0] = li[0] * li[0] + li[1] * li[1] + li[3] * li[3];
  di[1] = li[1] * li[2] + li[3] * li[4];
  di[2] = li[3] * li[5];
  di[3] = li[2] * li[2] + li[4] * li[4];
  di[4] = li[4] * li[5];
  di[5] = li[5] * li[5];
}

// `ok` and every entry finite, else zeros: a block that is not positive definite takes its point out of the system
__device__ __forceinline__ bool sym3_finite_or_zero(bool ok, double* di) {
  ok = ok && isfinite(di[0] + di[1] + di[2] + di[3] + di[4] + di[5]);
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 6; ++k) di[k] = 0.0;
  }
  return ok;
}

__device__ __forceinline__ void sym3_apply(const double* di, const double* g, double* out) {
  out[0] = di[0] * g[0] + di[1] * g[1] + di[2] * g[2];
  out[1] = di[1] * g[0] + di[3] * g[1] + di[4] * g[2];
  out[2] = di[2] * g[0] + di[4] * g[1] + di[5] * g[2];
}

// out[0] = sum of the per-point cost shares and, with pt_ptr, out[1] = the number of points that have a track (without:
// out[1] is not written): one workgroup of 256, thread t sums points t, t + 256, ... in ascending order, then a fixed tree.
// (defined once, in sfm_ba_host.hip)
__global__ void ba_point_cost_reduce_kernel(int N, const double* __restrict__ cost_pt, const int* __restrict__ pt_ptr,
                                            double* __restrict__ out);

// cams [V][7] -> their expanded form, one thread per camera; status[2]: first failing code and its camera (cam_prepare).
// (defined once, in sfm_ba.hip)
__global__ void ba_cam_prep_kernel(int V, const double* __restrict__ cams, CamPrep* __restrict__ prep, int* __restrict__ status);

}  // namespace sfm
