// sfm_resect.hip — robust resection of cameras: three-point hypotheses, inlier refit (gfx950).
//
// sfm_ba_refine_cameras fits a camera by least squares over EVERY observation it owns; here the consistent subset of the
// camera's observations is found first (the rule is stated in sfm_hip.h, block "robust resection"):
//   hyp      one lane per (camera, hypothesis): unranks its triple, solves Grunert's quartic (Ferrari's closed form, two
//            Newton steps on the quartic itself), forms up to four poses [R^T | t] from the two frames, applies the
//            triple gate and writes the poses with their valid bits
//   score    the hot path: a workgroup of 256 owns 1 024 observations of one camera, four per lane, in registers; the
//            camera's poses pass through LDS in batches of 64 hypotheses, every lane reads the pose under test from the
//            same address (a broadcast), tests its four observations without a branch, a wave adds the popcounts of its
//            four ballots and issues one integer atomicAdd per pose
//   pick     one wave per camera: the lexicographic arg-best over (count, h, r), the winner as [C, q]
//   refit    one workgroup per camera, 1 024 observations at a time in every pass: sfm_ba_refine_cameras' step
//            (sfm_cam_fit.h) over the winner's inliers, the mask recomputed from the winner's pose in every pass, then the
//            acceptance
//   judge    one workgroup per camera, after the cameras that stand have been expanded by the kernel every other
//            operation expands them with: obs_inlier, n_inliers and the summary through sfm_ba_screen's projection
// One body serves the free form (contiguous observations, a point per observation) and the resident scene (its
// camera-major list) through CamObsView.  No floating-point value is accumulated with an atomic; the counts are integers;
// the refit's 36 sums are formed per slice of 64 consecutive observations and added in slice order: a camera's bits depend
// on its own observations, their points and the options only.
// Shared with the robust two-view geometry, in sfm_robust.h: the plan of the hypotheses (HypPlan, hyp_owner), the batch
// loop of `score` (robust_score_block), the tie rule of `pick` (wave_arg_best), the block reductions of `refit` and `judge`
// (block_count, slice_totals, block_sum_int), the summary and the host frame.
#include <climits>
#include <cmath>

#include "sfm_ba.h"
#include "sfm_cam_fit.h"
#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"

namespace sfm {

constexpr int kRsMinCount = 4;       // a winner explains at least one observation besides its own three
constexpr int kRsThreads = 256;
constexpr int kRsBlockObs = kRsThreads * kMoPerLane;      // 1 024 observations per workgroup and round
constexpr int kRsBatch = 64;          // hypotheses per LDS batch: 64 x 4 x 12 doubles = 24 576 bytes, six workgroups per CU
constexpr int kRsPose = 12;           // R^T row-major (9) | t (3)
constexpr double kRsRootImag = 1e-7;  // a conjugate pair whose imaginary part is below this (relative to 1 + |real|) counts as a double root

struct RsArgs {
  CamObsView w;
  const unsigned char* mask;    // [V] or null: cameras with a zero entry are held
  const int* hyp_off;           // [V + 1] first hypothesis of every camera (a held or too small camera has none)
  const int2* blocks;           // score: workgroup -> (camera, first entry of its 1 024 observations, relative)
  double max_err2;
  int max_hyp;
  double lambda;
  int iters, quirks;
  const double* cams_in;        // [V][7] or null (= the identity at the origin)
  double* cams_out;             // [V][7], may equal cams_in
  double* poses;                // [hypotheses][4][12]
  unsigned char* pose_ok;       // [hypotheses] bit r: pose r is valid
  int* counts;                  // [hypotheses][4]
  int* best_hyp;                // [V]
  int* win_count;               // [V]
  double* win_pose;             // [V][12]
  double* win_cam;              // [V][7]
  int* status;                  // [V]
  const CamPrep* prep;          // [V] judge: the cameras that stand, expanded
  unsigned char* obs_inlier;    // [M] or null
  int* n_inliers;               // [V] or null
  unsigned long long* summary;  // [6]
};

// Everything below is compiled WITHOUT automatic contraction and spells its FMAs out; the test of an observation is
// sfm_obs_test.h's, the one sfm_ba_screen applies.
// s = m X + t of a pose [m | t] (m row-major), in track_project's operation order
__device__ __forceinline__ void rs_project_pose(const double* m, const double* t, const MoObs& o, double* s) {
#pragma unroll
  for (int r = 0; r < 3; ++r) s[r] = __builtin_fma(m[3 * r + 2], o.Z, __builtin_fma(m[3 * r + 1], o.Y, m[3 * r] * o.X)) + t[r];
}

// Is the observation an inlier of the pose / of the prepared camera?
__device__ __forceinline__ bool rs_inlier_pose(const double* m, const double* t, const MoObs& o, double scale, double max_err2) {
  double s[3];
  rs_project_pose(m, t, o, s);
  return obs_passes(s, obs_err2(s, o.u, o.v, scale), max_err2);
}
__device__ __forceinline__ bool rs_inlier_cam(const CamPrep& c, const MoObs& o, double scale, double max_err2) {
  double s[3];
  obs_project_cam(c, o.X, o.Y, o.Z, s);
  return obs_passes(s, obs_err2(s, o.u, o.v, scale), max_err2);
}

// ---------------------------------------------------------------------------------------------
// hyp: the poses of a triple
// ---------------------------------------------------------------------------------------------
// The two roots of z^2 + B z + C; NaN where the pair is complex beyond kRsRootImag (shift: what is added to z to give y).
__device__ __forceinline__ void rs_quadratic(double B, double C, double shift, double& z0, double& z1) {
  const double disc = B * B - 4.0 * C;
  const double lim = kRsRootImag * (1.0 + fabs(-0.5 * B + shift));
  const bool real = disc >= -4.0 * lim * lim;
  const double sq = sqrt(fmax(disc, 0.0));
  const double t = -0.5 * (B + copysign(sq, B));
  z0 = real ? t : __builtin_nan("");
  z1 = real ? (t != 0.0 ? C / t : 0.0) : __builtin_nan("");
}

// The real roots of A4 y^4 + A3 y^3 + A2 y^2 + A1 y + A0 (A4 != 0) by Ferrari's factorisation into two quadratics over
// the largest real root of the resolvent cubic, polished by two Newton steps on the quartic itself; NaN in unused slots.
__device__ __forceinline__ void rs_quartic(double A4, double A3, double A2, double A1, double A0, double (&y)[4]) {
  const double a = A3 / A4, b = A2 / A4, c = A1 / A4, d = A0 / A4;
  const double a2 = a * a;
  const double p = b - 0.375 * a2;
  const double q = c - 0.5 * a * b + 0.125 * a2 * a;
  const double r = d - 0.25 * a * c + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
  const double shift = -0.25 * a;
  // resolvent: m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0, value -q^2 / 8 <= 0 at m = 0: its largest real root is >= 0
  const double cB = 0.25 * p * p - r, cC = -0.125 * q * q;
  const double P = cB - p * p / 3.0;
  const double Q = 2.0 * p * p * p / 27.0 - p * cB / 3.0 + cC;
  const double disc = 0.25 * Q * Q + P * P * P / 27.0;
  double t;
  if (disc > 0.0) {
    const double w = cbrt(-0.5 * Q - copysign(sqrt(disc), Q));
    t = w != 0.0 ? w - P / (3.0 * w) : 0.0;
  } else {
    const double rr = sqrt(fmax(-P / 3.0, 0.0));
    const double arg = rr > 0.0 ? fmin(1.0, fmax(-1.0, 1.5 * Q / (P * rr))) : 1.0;
    t = 2.0 * rr * cos(acos(arg) / 3.0);
  }
  double m = t - p / 3.0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double val = ((m + p) * m + cB) * m + cC, der = (3.0 * m + 2.0 * p) * m + cB;
    const double step = val / der;
    m = isfinite(step) ? m - step : m;
  }
  if (m > 0.0) {
    const double s = sqrt(2.0 * m), h = 0.5 * q / s;
    rs_quadratic(-s, 0.5 * p + m + h, shift, y[0], y[1]);
    rs_quadratic(s, 0.5 * p + m - h, shift, y[2], y[3]);
  } else {      // q = 0 to rounding: a quadratic in z^2
    double w0, w1;
    rs_quadratic(p, r, 0.0, w0, w1);
    const double z0 = sqrt(w0), z1 = sqrt(w1);      // NaN for a negative or complex w
    y[0] = z0; y[1] = -z0; y[2] = z1; y[3] = -z1;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double v = y[k] + shift;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const double val = (((A4 * v + A3) * v + A2) * v + A1) * v + A0;
      const double der = ((4.0 * A4 * v + 3.0 * A3) * v + 2.0 * A2) * v + A1;
      const double step = val / der;
      v = isfinite(step) ? v - step : v;
    }
    y[k] = v;
  }
}

// The right-handed frame spanned by (b - a, (b - a) x (c - a)): e[0..2] = e1, e[3..5] = e2, e[6..8] = e3; false for a
// zero or non-finite normal.
__device__ __forceinline__ bool rs_frame(const double* a, const double* b, const double* c, double* e) {
  const double d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
  const double f0 = c[0] - a[0], f1 = c[1] - a[1], f2 = c[2] - a[2];
  const double n0 = d1 * f2 - d2 * f1, n1 = d2 * f0 - d0 * f2, n2 = d0 * f1 - d1 * f0;
  const double nn = n0 * n0 + n1 * n1 + n2 * n2;
  const double id = 1.0 / sqrt(d0 * d0 + d1 * d1 + d2 * d2), in = 1.0 / sqrt(nn);
  e[0] = d0 * id; e[1] = d1 * id; e[2] = d2 * id;
  e[6] = n0 * in; e[7] = n1 * in; e[8] = n2 * in;
  e[3] = e[7] * e[2] - e[8] * e[1];
  e[4] = e[8] * e[0] - e[6] * e[2];
  e[5] = e[6] * e[1] - e[7] * e[0];
  return nn > 0.0 && isfinite(nn);
}

__device__ __forceinline__ void rs_swap_if(bool sw, double& a, double& b) {
  const double x = sw ? b : a, y = sw ? a : b;
  a = x; b = y;
}

__global__ __launch_bounds__(kRsThreads) void resect_hyp_kernel(RsArgs a, int n_hyp) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_hyp) return;
  const int cam = hyp_owner(a.hyp_off, a.w.V, g), h = g - a.hyp_off[cam];
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  const long long T = triple_count(n);
  int idx[3];
  triple_of(n, ransac_pair_number(T, a.max_hyp, h), &idx[0], &idx[1], &idx[2]);
  MoObs ob[3];
  double scale = 1.0, f[3][3], X[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    cam_obs_load(a.w, cam, base + idx[k], ob[k], &scale);
    const double inv = 1.0 / sqrt(ob[k].u * ob[k].u + ob[k].v * ob[k].v + 1.0);
    f[k][0] = ob[k].u * inv; f[k][1] = ob[k].v * inv; f[k][2] = inv;
    X[k][0] = ob[k].X; X[k][1] = ob[k].Y; X[k][2] = ob[k].Z;
  }
  auto dist2 = [&](int i, int j) {
    const double d0 = X[i][0] - X[j][0], d1 = X[i][1] - X[j][1], d2 = X[i][2] - X[j][2];
    return d0 * d0 + d1 * d1 + d2 * d2;
  };
  auto dot = [&](int i, int j) { return f[i][0] * f[j][0] + f[i][1] * f[j][1] + f[i][2] * f[j][2]; };
  const double a2 = dist2(1, 2), b2 = dist2(0, 2), c2 = dist2(0, 1);
  const double ca = dot(1, 2), cb = dot(0, 2), cg = dot(0, 1);
  const double p = (a2 - c2) / b2, q = (a2 + c2) / b2;
  const double A4 = (p - 1) * (p - 1) - 4 * (c2 / b2) * ca * ca;
  const double A3 = 4 * (p * (1 - p) * cb - (1 - q) * ca * cg + 2 * (c2 / b2) * ca * ca * cb);
  const double A2 = 2 * (p * p - 1 + 2 * p * p * cb * cb + 2 * ((b2 - c2) / b2) * ca * ca - 4 * q * ca * cb * cg + 2 * ((b2 - a2) / b2) * cg * cg);
  const double A1 = 4 * (-p * (1 + p) * cb + 2 * (a2 / b2) * cg * cg * cb - (1 - q) * ca * cg);
  const double A0 = (1 + p) * (1 + p) - 4 * (a2 / b2) * cg * cg;
  double ew[9];
  bool ok = isfinite(a2) && isfinite(b2) && isfinite(c2) && a2 != 0.0 && b2 != 0.0 && c2 != 0.0;
  ok = ok && isfinite(A4) && isfinite(A3) && isfinite(A2) && isfinite(A1) && isfinite(A0) && A4 != 0.0;
  ok = rs_frame(X[0], X[1], X[2], ew) && ok;

  double y[4], x[4], s1[4];
  rs_quartic(A4, A3, A2, A1, A0, y);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double div = 2 * (cg - y[k] * ca);
    x[k] = ((p - 1) * y[k] * y[k] - 2 * p * cb * y[k] + 1 + p) / div;
    s1[k] = sqrt(b2 / (1 + y[k] * y[k] - 2 * y[k] * cb));
    const bool good = ok && div != 0.0 && isfinite(x[k]) && isfinite(s1[k]) && x[k] > 0.0 && y[k] > 0.0 && s1[k] > 0.0;
    s1[k] = good ? s1[k] : __builtin_inf();                // a slot without a pose sorts behind every pose
  }
  // ascending s_i: a five-comparator network on (s1, x, y)
#define RS_CMP(i, j) { const bool sw = s1[j] < s1[i]; rs_swap_if(sw, s1[i], s1[j]); rs_swap_if(sw, x[i], x[j]); rs_swap_if(sw, y[i], y[j]); }
  RS_CMP(0, 1) RS_CMP(2, 3) RS_CMP(0, 2) RS_CMP(1, 3) RS_CMP(1, 2)
#undef RS_CMP

  int bits = 0;
  double* out = a.poses + (size_t)g * 4 * kRsPose;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double Pc[3][3], ec[9], m[9], t[3], rot[9], quat[4];
    const double d[3] = {s1[k], x[k] * s1[k], y[k] * s1[k]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Pc[i][j] = d[i] * f[i][j];
    bool good = s1[k] < __builtin_inf();
    good = rs_frame(Pc[0], Pc[1], Pc[2], ec) && good;
    double chk = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        m[3 * i + j] = ec[i] * ew[j] + ec[3 + i] * ew[3 + j] + ec[6 + i] * ew[6 + j];      // M Fw = Fc
        rot[3 * j + i] = m[3 * i + j];
        chk += m[3 * i + j] * 0.0;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      t[i] = Pc[0][i] - (m[3 * i] * X[0][0] + m[3 * i + 1] * X[0][1] + m[3 * i + 2] * X[0][2]);
      chk += t[i] * 0.0;
    }
    good = good && chk == 0.0 && rot_to_quat(rot, quat) == SFM_OK;
    // the triple gate
    good = good && rs_inlier_pose(m, t, ob[0], scale, a.max_err2) && rs_inlier_pose(m, t, ob[1], scale, a.max_err2) &&
           rs_inlier_pose(m, t, ob[2], scale, a.max_err2);
    bits |= good ? 1 << k : 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[kRsPose * k + i] = m[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[kRsPose * k + 9 + i] = t[i];
  }
  a.pose_ok[g] = (unsigned char)bits;
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void resect_score_kernel(RsArgs a) {
  __shared__ double pose[kRsBatch * 4 * kRsPose];
  __shared__ unsigned char okb[kRsBatch];
  const int tid = threadIdx.x;
  const int2 blk = a.blocks[blockIdx.x];
  const int cam = blk.x;
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  const int h0 = a.hyp_off[cam], H = a.hyp_off[cam + 1] - h0;
  // four observations per lane; an entry beyond the camera carries a NaN scale and is nobody's inlier
  MoObs ob[kMoPerLane];
  double sc[kMoPerLane];
#pragma unroll
  for (int k = 0; k < kMoPerLane; ++k) {
    const int i = blk.y + kMoPerLane * tid + k;
    cam_obs_load(a.w, cam, base + (i < n ? i : n - 1), ob[k], &sc[k]);
    if (!(i < n)) sc[k] = __builtin_nan("");
  }
  robust_score_block<kRsThreads, kRsBatch, 4 * kRsPose, 4, kMoPerLane>(
      a.poses, a.pose_ok, a.counts, h0, H, pose, okb,
      [&](const double* m, int k) { return rs_inlier_pose(m, m + 9, ob[k], sc[k], a.max_err2); });
}

// ---------------------------------------------------------------------------------------------
// pick: the winner of every camera
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void resect_pick_kernel(RsArgs a) {
  const int cam = blockIdx.x, lane = threadIdx.x;
  const int h0 = a.hyp_off[cam], H = a.hyp_off[cam + 1] - h0;
  // index 4 h + r ascends with (h, r): the first of the largest counts wins
  int best_cnt, best_i;
  wave_arg_best(lane, 4 * H, [&](int i) { return a.pose_ok[h0 + (i >> 2)] >> (i & 3) & 1; },
                [&](int i) { return a.counts[(size_t)h0 * 4 + i]; }, best_cnt, best_i);
  if (lane != 0) return;
  const bool won = best_cnt >= kRsMinCount;
  a.best_hyp[cam] = won ? best_i >> 2 : -1;
  a.win_count[cam] = won ? best_cnt : 0;
  if (!won) return;
  const double* m = a.poses + ((size_t)h0 * 4 + best_i) * kRsPose;
  double rot[9], quat[4] = {1, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) rot[3 * j + i] = m[3 * i + j];
  (void)rot_to_quat(rot, quat);                            // it succeeded in resect_hyp_kernel, on the same bits
  double* wc = a.win_cam + 7 * (size_t)cam;
#pragma unroll
  for (int i = 0; i < 3; ++i) wc[i] = -(rot[3 * i] * m[9] + rot[3 * i + 1] * m[10] + rot[3 * i + 2] * m[11]);      // C = -R t
#pragma unroll
  for (int i = 0; i < 4; ++i) wc[3 + i] = quat[i];
#pragma unroll
  for (int i = 0; i < kRsPose; ++i) a.win_pose[kRsPose * (size_t)cam + i] = m[i];
}

// ---------------------------------------------------------------------------------------------
// refit and acceptance
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void resect_refit_kernel(RsArgs a) {
  constexpr int ROWS = kRsThreads / 16;
  __shared__ double red[ROWS][kMoSums];
  __shared__ double sums[kMoSums];
  const int cam = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  const bool held = a.mask != nullptr && a.mask[cam] == 0;
  const int bh = a.best_hyp[cam];
  int flags = held ? SFM_RESECT_HELD : (n < 4 ? SFM_RESECT_TOO_FEW : (bh < 0 ? SFM_RESECT_NO_MODEL : 0));
  if (!held && n >= 4 && triple_count(n) > (long long)a.max_hyp) flags |= SFM_RESECT_SAMPLED;
  const bool solved = !(flags & (SFM_RESECT_HELD | SFM_RESECT_TOO_FEW | SFM_RESECT_NO_MODEL));
  double params[7] = {0, 0, 0, 1, 0, 0, 0};
  if (solved) {
    double hyp[7], wp[kRsPose];
#pragma unroll
    for (int k = 0; k < 7; ++k) params[k] = hyp[k] = a.win_cam[7 * (size_t)cam + k];
#pragma unroll
    for (int k = 0; k < kRsPose; ++k) wp[k] = a.win_pose[kRsPose * (size_t)cam + k];
    const int hc = a.win_count[cam];
    const int n_blocks = (n + kRsBlockObs - 1) / kRsBlockObs;
    int own[3];
    mo_fold_own(lane, own);
    CamPrep c;
    (void)cam_prepare_dev<true>(params, &c);               // R is a product of two orthonormal frames: the checks cannot fire
    const LossArg<SFM_LOSS_NONE> la = {};
    bool ok = true;
    for (int it = 0; ok && it < a.iters; ++it) {
      double run = 0;                                      // threads 0 .. 35: the running total of their sum
      for (int blk = 0; blk < n_blocks; ++blk) {
        double acc[kMoSums];
#pragma unroll
        for (int k = 0; k < kMoSums; ++k) acc[k] = 0;
        int behind = 0;
#pragma unroll
        for (int k = 0; k < kMoPerLane; ++k) {
          const int i = blk * kRsBlockObs + kMoPerLane * tid + k;
          if (i < n) {
            MoObs ob;
            double scale;
            cam_obs_load(a.w, cam, base + i, ob, &scale);
            if (rs_inlier_pose(wp, wp + 9, ob, scale, a.max_err2)) mo_accumulate<SFM_LOSS_NONE>(c, ob, a.quirks, la, acc, behind);
          }
        }
        mo_fold_row(acc, own, lane, red[tid >> 4]);
        slice_totals<kMoSums, ROWS>(red, sums, run, blk == 0, blk == n_blocks - 1, tid);
      }
      // from here on every thread holds the same values: the branches are uniform
      ok = mo_finite_probe(sums, kMoSums) == 0.0 && mo_step(sums, a.lambda, params, c);
    }
    // the refit's own inlier count over all n
    int rc = 0;
    if (ok) {
      for (int blk = 0; blk < n_blocks; ++blk) {
        int mine = 0;
#pragma unroll
        for (int k = 0; k < kMoPerLane; ++k) {
          const int i = blk * kRsBlockObs + kMoPerLane * tid + k;
          if (i < n) {
            MoObs ob;
            double scale;
            cam_obs_load(a.w, cam, base + i, ob, &scale);
            mine += rs_inlier_cam(c, ob, scale, a.max_err2);
          }
        }
        rc += block_count(mine);
      }
    }
    if (!(ok && rc >= hc)) {
#pragma unroll
      for (int k = 0; k < 7; ++k) params[k] = hyp[k];
      flags |= SFM_RESECT_KEPT_HYPOTHESIS;
    }
  } else if (a.cams_in) {
#pragma unroll
    for (int k = 0; k < 7; ++k) params[k] = a.cams_in[7 * (size_t)cam + k];
  }
  if (tid != 0) return;
  a.status[cam] = flags;
  if (solved || a.cams_out != a.cams_in) {                 // an unsolved or held camera in place is not touched at all
#pragma unroll
    for (int k = 0; k < 7; ++k) a.cams_out[7 * (size_t)cam + k] = params[k];
  }
}

// ---------------------------------------------------------------------------------------------
// judge: what the cameras that stand make of their observations
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void resect_judge_kernel(RsArgs a) {
  __shared__ int total;
  const int cam = blockIdx.x, tid = threadIdx.x;
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  const int flags = a.status[cam];
  const bool solved = !(flags & (SFM_RESECT_HELD | SFM_RESECT_TOO_FEW | SFM_RESECT_NO_MODEL));
  const bool judged = solved || (flags & SFM_RESECT_HELD);
  CamPrep c;
  load_cam(c, a.prep + cam);
  int nin = 0;
  for (int i = tid; i < n; i += kRsThreads) {
    MoObs ob;
    double scale;
    int index;      // the observation: obs_inlier is by observation
    cam_obs_load(a.w, cam, base + i, ob, &scale, &index);
    const bool in = judged & rs_inlier_cam(c, ob, scale, a.max_err2);
    if (a.obs_inlier) a.obs_inlier[index] = in ? 1 : 0;
    nin += in;
  }
  nin = block_sum_int(nin, &total);
  if (tid != 0) return;
  if (a.n_inliers) a.n_inliers[cam] = nin;
  robust_summary_add(a.summary, solved, flags & SFM_RESECT_HELD, flags & SFM_RESECT_TOO_FEW, flags & SFM_RESECT_KEPT_HYPOTHESIS, n, nin);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// T = n (n - 1) (n - 2) / 6 must fit 63 bits
static int resect_check_counts(const char* who, int V, const int* ptr) {
  for (int c = 0; c < V; ++c) {
    const int n = ptr[c + 1] - ptr[c];
    if (n > kTripleMaxObs) { set_error("%s: camera %d has %d observations; at most %d are supported", who, c, n, kTripleMaxObs); return SFM_E_SHAPE; }
  }
  return SFM_OK;
}

static int resect_check_views(const char* who, int n_views, const int* view_ptr, long long M) {
  SFM_TRY(robust_check_offsets(who, "view", "view_ptr", n_views, view_ptr, M, false));
  return n_views ? resect_check_counts(who, n_views, view_ptr) : SFM_OK;
}

// What a call keeps on the device besides the caller's arrays.
struct ResectWork {
  HypPlan plan;
  RobustStandIns stand_in;
  DevBuf<int> win_count, counts, prep_status;
  DevBuf<double> poses, win_pose, win_cam;
  DevBuf<unsigned char> pose_ok;
  DevBuf<CamPrep> prep;
};

// Enqueue the kernels up to the refit on s.  h_ptr / h_mask: the host's copy of the list offsets (checked: no camera beyond
// 2^20 observations) and the mask, from which the launches are planned.  a.best_hyp / a.status / a.summary may be null: the work buffers stand in.
static int resect_enqueue(const char* who, RsArgs& a, ResectWork& w, const int* h_ptr, const unsigned char* h_mask, hipStream_t s) {
  const int V = a.w.V;
  if (a.max_hyp == 0) a.max_hyp = kHypDefault;
  SFM_TRY(w.plan.build(who, V, h_ptr, kRsBlockObs, INT_MAX / (4 * kRsPose), [&](int c, int n, long long& hyps) {
    hyps = hyp_count(triple_count(n), a.max_hyp);
    return n >= 4 && !(h_mask && h_mask[c] == 0);
  }, s));
  const size_t v = (size_t)V, nh = w.plan.n_hyp;
  SFM_TRY(w.poses.alloc(nh * 4 * kRsPose, s)); SFM_TRY(w.pose_ok.alloc(nh, s)); SFM_TRY(w.counts.alloc(nh * 4, s));
  SFM_TRY(w.win_count.alloc(v, s)); SFM_TRY(w.win_pose.alloc(v * kRsPose, s)); SFM_TRY(w.win_cam.alloc(v * 7, s));
  SFM_TRY(w.stand_in.fill(a, v, true, s));
  a.hyp_off = w.plan.hyp_off.p; a.blocks = w.plan.blocks.p;
  a.poses = w.poses.p; a.pose_ok = w.pose_ok.p; a.counts = w.counts.p;
  a.win_count = w.win_count.p; a.win_pose = w.win_pose.p; a.win_cam = w.win_cam.p;
  if (nh) {
    SFM_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * nh * 4, s));
    resect_hyp_kernel<<<(unsigned)((nh + kRsThreads - 1) / kRsThreads), kRsThreads, 0, s>>>(a, (int)nh);
    resect_score_kernel<<<w.plan.n_blocks, kRsThreads, 0, s>>>(a);
  }
  resect_pick_kernel<<<V, 64, 0, s>>>(a);
  resect_refit_kernel<<<V, kRsThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// The one body of sfm_resect_ransac and sfm_resect_ransac_dev: checked arguments and device pointers in (n_views > 0), the
// kernels enqueued on s out.  w lives until the caller has waited for s.
static int resect_run(const char* who, int n_views, const int* view_ptr, long long M, const double* d_uv, const double* d_X,
                      const double* d_cam_scale, double max_err2, int max_hyp, double lambda, int iters, int quirks,
                      const double* d_cams_init, double* d_cams_out, const RobustPtrs& out, DevBuf<int>& d_ptr, ResectWork& w,
                      hipStream_t s) {
  SFM_TRY(d_ptr.upload(view_ptr, (size_t)n_views + 1, s));
  RsArgs a = {};
  a.w = cam_obs_view_free(n_views, d_ptr.p, M, d_uv, d_X, d_cam_scale);
  a.max_err2 = max_err2; a.max_hyp = max_hyp; a.lambda = lambda; a.iters = iters; a.quirks = quirks;
  a.cams_in = d_cams_init; a.cams_out = d_cams_out;
  out.into(a);
  SFM_TRY(resect_enqueue(who, a, w, view_ptr, nullptr, s));
  // the cameras that stand, expanded as every operation on a scene expands them (a camera that fails its checks there is
  // still projected with its R(q) and t)
  SFM_TRY(w.prep.alloc((size_t)n_views, s));
  SFM_TRY(w.prep_status.alloc(2, s));
  SFM_HIP(hipMemsetAsync(w.prep_status.p, 0, 2 * sizeof(int), s));
  ba_cam_prep_kernel<<<(n_views + 63) / 64, 64, 0, s>>>(n_views, d_cams_out, w.prep.p, w.prep_status.p);
  SFM_HIP(hipGetLastError());
  a.prep = w.prep.p;
  resect_judge_kernel<<<n_views, kRsThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_resect_triple(int n, int max_hyp, int h, int* i, int* j, int* l) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (n < 3 || n > kTripleMaxObs || max_hyp < 1 || max_hyp > kHypMax) return 0;
  const long long T = triple_count(n);
  const int H = hyp_count(T, max_hyp);
  if (h >= 0 && h < H && i != nullptr && j != nullptr && l != nullptr) triple_of(n, ransac_pair_number(T, max_hyp, h), i, j, l);
  return H;
}

int sfm_resect_ransac_dev(int n_views, const int* view_ptr, int64_t M, const double* d_uv, const double* d_X,
                          const double* d_cam_scale, double max_err2, int max_hyp, double lambda, int iters, int quirks,
                          const double* d_cams_init, double* d_cams_out, unsigned char* d_obs_inlier, int* d_n_inliers,
                          int* d_best_hyp, int* d_status, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_resect_ransac_dev";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, lambda, iters));
  SFM_TRY(resect_check_views(who, n_views, view_ptr, M));
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_views == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  if (d_cams_out == nullptr || (M > 0 && (d_uv == nullptr || d_X == nullptr))) { set_error("%s: null device pointer", who); return SFM_E_SHAPE; }
  DevBuf<int> dPtr;
  ResectWork w;
  SFM_TRY(resect_run(who, n_views, view_ptr, M, d_uv, d_X, d_cam_scale, max_err2, max_hyp, lambda, iters, quirks, d_cams_init,
                     d_cams_out, RobustPtrs{d_obs_inlier, d_n_inliers, d_best_hyp, d_status, d_summary}, dPtr, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_resect_ransac(int n_views, const int* view_ptr, int64_t M, const double* uv, const double* X, const double* cam_scale,
                      double max_err2, int max_hyp, double lambda, int iters, int quirks, const double* cams_init, double* cams_out,
                      unsigned char* obs_inlier, int* n_inliers, int* best_hyp, int* status, int64_t* summary) {
  const char* who = "sfm_resect_ransac";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, lambda, iters));
  SFM_TRY(resect_check_views(who, n_views, view_ptr, M));
  robust_summary_clear(summary);
  if (n_views == 0) return SFM_OK;
  if (cams_out == nullptr || (M > 0 && (uv == nullptr || X == nullptr))) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_views, m = (size_t)M;
  DevBuf<int> dPtr;
  DevBuf<double> dUV, dX, dSc, dIn;
  HostOut<double> oCams;
  RobustOut o;
  ResectWork w;
  SFM_TRY(dUV.upload(uv, 2 * m, s));
  SFM_TRY(dX.upload(X, 3 * m, s));
  SFM_TRY(dSc.upload_if(cam_scale, v, s));
  SFM_TRY(dIn.upload_if(cams_init, 7 * v, s));
  SFM_TRY(oCams.want(cams_out, 7 * v, s));
  SFM_TRY(o.want(m, v, obs_inlier, n_inliers, best_hyp, status, summary, s));
  SFM_TRY(resect_run(who, n_views, view_ptr, M, dUV.p, dX.p, dSc.p, max_err2, max_hyp, lambda, iters, quirks, dIn.p, oCams.dev(),
                     o.dev(), dPtr, w, s));
  SFM_TRY(oCams.fetch(s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

int sfm_ba_resect(sfm_ba_problem* p, double max_err2, int max_hyp, double lambda, int iters, int quirks, const unsigned char* cam_mask,
                  const double* cam_scale, unsigned char* obs_inlier, int* n_inliers, int* best_hyp, int* status, int64_t* summary) {
  const char* who = "sfm_ba_resect";
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, lambda, iters));
  SFM_TRY(ba_refuse_comm(p, who, "the points are sharded; the replicas would diverge"));
  BaDev& d = p->dev;
  const int V = d.V;
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  robust_summary_clear(summary);
  if (d.N == 0 || d.M == 0) {                            // no observation anywhere: every camera that is not held has too few
    for (int c = 0; c < V; ++c) {
      const bool held = cam_mask && cam_mask[c] == 0;
      if (status) status[c] = held ? SFM_RESECT_HELD : SFM_RESECT_TOO_FEW;
      if (n_inliers) n_inliers[c] = 0;
      if (best_hyp) best_hyp[c] = -1;
      if (summary && !held) ++summary[2];
    }
    return SFM_OK;
  }
  SFM_TRY(ba_prepared_cameras(p, who));
  SFM_TRY(ba_cam_list_ensure(p));
  SFM_TRY(resect_check_counts(who, V, p->h_cam_ptr.data()));
  int v_free = 0, first_free = -1;
  ba_free_cameras(cam_mask, V, &v_free, &first_free);
  hipStream_t s = p->stream;
  const size_t v = (size_t)V, m = (size_t)d.M;
  DevBuf<unsigned char> dMask;
  DevBuf<double> dSc;
  RobustOut o;
  ResectWork w;
  SFM_TRY(dMask.upload_if(cam_mask, v, s));
  SFM_TRY(dSc.upload_if(cam_scale, v, s));
  p->upload_bytes += (long long)((cam_mask ? v : 0) + (cam_scale ? sizeof(double) * v : 0));
  SFM_TRY(o.want(m, v, obs_inlier, n_inliers, best_hyp, status, summary, s));
  RsArgs a = {};
  a.w = cam_obs_view_resident(p, dSc.p);
  a.mask = dMask.p;
  a.max_err2 = max_err2; a.max_hyp = max_hyp; a.lambda = lambda; a.iters = iters; a.quirks = quirks;
  a.cams_in = d.cams; a.cams_out = d.cams;               // in place: only solved cameras are written
  o.dev().into(a);
  SFM_TRY(resect_enqueue(who, a, w, p->h_cam_ptr.data(), cam_mask, s));
  if (v_free > 0) SFM_TRY(ba_enqueue_prep(p));           // the expansion sfm_ba_screen will read, of the cameras that stand
  a.prep = d.prep[p->cur];
  resect_judge_kernel<<<V, kRsThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  SFM_TRY(ba_state_changed(p));                          // new cameras
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
