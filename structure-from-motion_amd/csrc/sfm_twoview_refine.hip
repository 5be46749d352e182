// sfm_twoview_refine.hip — refinement of the relative pose of a verified pair: damped Gauss-Newton on the Sampson distance
// in pixels, over the five parameters of a calibrated pair (gfx950).
//
// What follows sfm_twoview_pose (sfm_twoview_pose.hip): the pose (R, t), X_right = R X_left + t, |t| = 1, of every set of
// matches is moved to the minimum of the sum of squared Sampson distances of its selected matches, and the matches are
// judged against the result.  The rule is stated in sfm_hip.h, block "refinement of a relative pose".  Two kernels, one
// workgroup per set each:
//   iterate  all passes of a set in one launch.  Per pass six lanes form the model of the standing pose -- F and its five
//            derivatives in the chart of the pose, 54 doubles, refine_model_part in sfm_obs_test.h -- in LDS, where every lane
//            reads it at the same address (a broadcast); every lane takes its matches' residuals and Jacobian rows
//            (refine_residual, the one function of the judge and of sfm_twoview_refine_test too) and adds the 21 sums
//            c = sum r^2, U = sum J^T J, g = sum J^T r per slice of 64 consecutive matches; the slices are added in slice
//            order (slice_totals); one lane solves (U + lambda diag U) d = -g by Cholesky and moves the pose.  A set of up
//            to 1 024 matches stays in registers across the passes, a larger one re-reads its blocks of 1 024.
//   judge    the walk over every match of the set at the output pose: obs_res, obs_inlier, obs_front, X_out, the counts,
//            F_out, the summary.
// No floating-point atomic; a set's bits depend on its own matches, its pose, the intrinsics and the options only.
#include <climits>
#include <cmath>

#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"
#include "sfm_match_norm.h"
#include "sfm_pose_rays.h"

namespace sfm {

constexpr int kRefSums = 21;                              // c, the upper triangle of U (15), g (5)
constexpr int kRefRows = kMatchBlockObs / 64;             // slices of 64 matches per pass of 1 024
constexpr int kRefMinUsed = 8;
// The workgroup of the iterate kernel: 256 lanes, four consecutive matches each.  -DSFM_REFINE_THREADS=512 or 1024 builds the
// kernel with two matches or one match per lane for a comparison (DESIGN.md section 33 has the outcome: both need scratch).
#ifndef SFM_REFINE_THREADS
#define SFM_REFINE_THREADS 256
#endif
constexpr int kRefThreads = SFM_REFINE_THREADS;
static_assert(kRefThreads == 256 || kRefThreads == 512 || kRefThreads == 1024, "a slice of 64 matches is 16, 32 or 64 lanes");
constexpr double kRefGuard = 1.0 + 9.313225746154785e-10; // 1 + 2^-30

struct RefineArgs {
  int n_sets;
  long long M;
  const int* ptr;               // [n_sets + 1]
  const double* left;           // [2][M]
  const double* right;          // [2][M]
  const unsigned char* mask;    // [M] or null
  const double* R_in;           // [n_sets][9]
  const double* t_in;           // [n_sets][3]
  double Kl[9], Kr[9];
  double lambda, max_err2, cos2_min;
  int iters;
  double* R_out;                // [n_sets][9]
  double* t_out;                // [n_sets][3]
  int* n_used;                  // [n_sets]; a work buffer stands in for a null of the caller, as for status
  int* status;
  double* F_out;                // [n_sets][9] or null; so are all below
  double* cost;                 // [2][n_sets]
  double* info;                 // [n_sets][15]
  double* obs_res;              // [M]
  unsigned char* obs_inlier;    // [M]
  unsigned char* obs_front;     // [M]
  double* X_out;                // [3][M]
  int* n_inliers;
  int* n_front;
  int* n_parallax;
  unsigned long long* summary;  // [6]
};

__device__ __forceinline__ MatchView refine_view(const RefineArgs& a) { return {a.left, a.right, a.M}; }

__device__ __forceinline__ bool refine_finite4(const TvMatch& m) { return ((m.xl + m.yl + m.xr + m.yr) * 0.0) == 0.0; }

// The index of U[i][j], i <= j, in the packed upper triangle.
__host__ __device__ constexpr int refine_u(int i, int j) { return i * 5 - i * (i - 1) / 2 + (j - i); }

// (U + lambda diag U) d = -g by a Cholesky factorisation, in place: A holds the packed upper triangle of U on entry and the
// factor on exit, d holds g on entry and the step on exit (both in LDS: one lane works, and the workgroup's registers are
// the passes').  False if a pivot is not finite or not > 0.
__device__ bool refine_solve(double* A, double* d, double lambda) {
  for (int j = 0; j < 5; ++j) {
    double p = __builtin_fma(lambda, A[refine_u(j, j)], A[refine_u(j, j)]);
    for (int k = 0; k < j; ++k) p = __builtin_fma(-A[refine_u(k, j)], A[refine_u(k, j)], p);
    if (!(p > 0.0) || !isfinite(p)) return false;
    const double root = sqrt(p);
    A[refine_u(j, j)] = root;
    for (int i = j + 1; i < 5; ++i) {
      double v = A[refine_u(j, i)];
      for (int k = 0; k < j; ++k) v = __builtin_fma(-A[refine_u(k, i)], A[refine_u(k, j)], v);
      A[refine_u(j, i)] = v / root;
    }
  }
  for (int i = 0; i < 5; ++i) {
    double v = -d[i];
    for (int k = 0; k < i; ++k) v = __builtin_fma(-A[refine_u(k, i)], d[k], v);
    d[i] = v / A[refine_u(i, i)];
  }
  for (int i = 4; i >= 0; --i) {
    double v = d[i];
    for (int k = i + 1; k < 5; ++k) v = __builtin_fma(-A[refine_u(i, k)], d[k], v);
    d[i] = v / A[refine_u(i, i)];
  }
  return true;
}

// The pose P = (R row-major, t) moved by the step d in the chart of the model m: R <- exp([w]x) R by Rodrigues' formula,
// t <- (t + d3 b1 + d4 b2) / |.|.
__device__ void refine_move(double* P, const RefineModel& m, const double* d) {
  const double th2 = __builtin_fma(d[2], d[2], __builtin_fma(d[1], d[1], d[0] * d[0]));
  const double th = sqrt(th2), sh = sin(0.5 * th);
  const double A = th > 0.0 ? sin(th) / th : 1.0, B = th > 0.0 ? (2.0 * (sh * sh)) / th2 : 0.5;
  double G1[9], G2[9];
  refine_cross_mat(d, P, G1);
  refine_cross_mat(d, G1, G2);
#pragma unroll
  for (int k = 0; k < 9; ++k) P[k] = __builtin_fma(B, G2[k], __builtin_fma(A, G1[k], P[k]));
  double u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = __builtin_fma(d[4], m.b2[k], __builtin_fma(d[3], m.b1[k], P[9 + k]));
  const double nrm = sqrt(pose_dot(u, u));
#pragma unroll
  for (int k = 0; k < 3; ++k) P[9 + k] = u[k] / nrm;
}

// ---------------------------------------------------------------------------------------------
// iterate: every pass of a set
// ---------------------------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void refine_iterate_kernel(RefineArgs a) {
  constexpr int PER = kMatchBlockObs / THREADS;           // consecutive matches per lane
  constexpr int G = 64 / PER;                             // adjacent lanes that hold one slice of 64 matches
  __shared__ RefineModel model;
  __shared__ double red[kRefRows][kRefSums];
  __shared__ double sums[kRefSums];
  __shared__ double pose[12], first_U[15], sys[20];
  __shared__ int ctl[2], total;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int n_blocks = (n + kMatchBlockObs - 1) / kMatchBlockObs;
  const MatchView view = refine_view(a);
  TvMatch m[PER];
  bool on[PER];
  int held = -1;
  auto load_block = [&](int blk) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = blk * kMatchBlockObs + PER * tid + k;
      m[k] = TvMatch{0.0, 0.0, 0.0, 0.0};
      on[k] = false;
      if (i < n) {
        m[k] = match_load(view, (long long)base + i);
        on[k] = refine_finite4(m[k]) & (a.mask ? a.mask[(size_t)base + i] != 0 : true);
      }
    }
    held = blk;
  };
  int mine = 0;
  for (int blk = 0; blk < n_blocks; ++blk) {
    load_block(blk);
#pragma unroll
    for (int k = 0; k < PER; ++k) mine += on[k];
  }
  if (tid == 0) {
    // step 2: the pose has to be finite with a translation that can be scaled to length 1
    double P[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) P[k] = a.R_in[9 * (size_t)s + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[9 + k] = a.t_in[3 * (size_t)s + k];
    const double ss = pose_dot(P + 9, P + 9);
    const bool good = pose_finite9(P) && ss > 0.0 && isfinite(ss);
    const double nrm = sqrt(ss);
#pragma unroll
    for (int k = 0; k < 9; ++k) pose[k] = P[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose[9 + k] = P[9 + k] / nrm;
    ctl[0] = good ? 0 : SFM_REFINE_BAD_POSE;
  }
  const int n_used = block_sum_int(mine, &total);         // its barriers publish pose and ctl[0]
  int flags = ctl[0];
  if (n_used == 0) flags |= SFM_REFINE_EMPTY;
  if (n_used < kRefMinUsed) flags |= SFM_REFINE_TOO_FEW;
  double c_in = 0.0, c_out = 0.0;
  int steps = 0;
  const bool passes = flags == 0;                          // the same for the whole workgroup
  for (int pass = 0; passes; ++pass) {
    if (tid < 6) refine_model_part(pose, pose + 9, a.Kl, a.Kr, tid, model);        // six lanes, a matrix each
    __syncthreads();
    double run = 0.0;
    for (int blk = 0; blk < n_blocks; ++blk) {
      if (blk != held) load_block(blk);
      double acc[kRefSums];
#pragma unroll
      for (int k = 0; k < kRefSums; ++k) acc[k] = 0.0;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        double J[5];
        double r = refine_residual(model.F, model.dF, m[k].xl, m[k].yl, m[k].xr, m[k].yr, J);
        r = on[k] ? r : 0.0;                               // an unselected match adds zeros
#pragma unroll
        for (int j = 0; j < 5; ++j) J[j] = on[k] ? J[j] : 0.0;
        acc[0] = __builtin_fma(r, r, acc[0]);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
#pragma unroll
          for (int j = i; j < 5; ++j) acc[1 + refine_u(i, j)] = __builtin_fma(J[i], J[j], acc[1 + refine_u(i, j)]);
          acc[16 + i] = __builtin_fma(J[i], r, acc[16 + i]);
        }
      }
#pragma unroll
      for (int k = 0; k < kRefSums; ++k) acc[k] = group_sum<G>(acc[k]);
      if ((tid & (G - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < kRefSums; ++k) red[tid / G][k] = acc[k];
      }
      slice_totals<kRefSums, kRefRows>(red, sums, run, blk == 0, blk == n_blocks - 1, tid);
    }
    if (tid == 0) {
      bool stop = pass == a.iters;
      if (pass == 0) {
        c_in = sums[0];
#pragma unroll
        for (int k = 0; k < 15; ++k) first_U[k] = sums[1 + k];
      }
      if (!stop) {
        for (int k = 0; k < 20; ++k) sys[k] = sums[1 + k];
        if (refine_solve(sys, sys + 15, a.lambda)) {
          refine_move(pose, model, sys + 15);
          ++steps;
        } else {
          flags |= SFM_REFINE_SINGULAR;                    // the iterations end at the standing pose
          stop = true;
        }
      }
      c_out = sums[0];
      ctl[1] = stop;
    }
    __syncthreads();
    if (ctl[1]) break;
  }
  if (tid != 0) return;
  // step 7, the guard: the iterated pose stands iff it and its cost are finite and the cost did not grow
  bool moved = steps > 0;
  if (moved) {
    double probe = (c_in + c_out) * 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) probe += pose[k] * 0.0;
    if (!(probe == 0.0)) flags |= SFM_REFINE_NONFINITE;
    moved = probe == 0.0 && c_out <= c_in * kRefGuard;
  } else if (passes && !(((c_in) * 0.0) == 0.0)) {
    flags |= SFM_REFINE_NONFINITE;
  }
  if (!moved) flags |= SFM_REFINE_KEPT_INPUT;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.R_out[9 * (size_t)s + k] = moved ? pose[k] : a.R_in[9 * (size_t)s + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.t_out[3 * (size_t)s + k] = moved ? pose[9 + k] : a.t_in[3 * (size_t)s + k];
  if (a.cost) {
    a.cost[s] = c_in;
    a.cost[(size_t)a.n_sets + s] = moved ? c_out : c_in;
  }
  if (a.info)
    for (int k = 0; k < 15; ++k) a.info[15 * (size_t)s + k] = passes ? (moved ? sums[1 + k] : first_U[k]) : 0.0;
  a.n_used[s] = n_used;
  a.status[s] = flags;
}

// ---------------------------------------------------------------------------------------------
// judge: what the output pose makes of the matches
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void refine_judge_kernel(RefineArgs a) {
  __shared__ RefineModel model;
  __shared__ double Fn[9];
  __shared__ int total[3], fn_ok;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int flags = a.status[s];
  const bool good = !(flags & SFM_REFINE_BAD_POSE);
  double P[12];
#pragma unroll
  for (int k = 0; k < 9; ++k) P[k] = a.R_out[9 * (size_t)s + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) P[9 + k] = a.t_out[3 * (size_t)s + k];
  if (tid < 6) refine_model_part(P, P + 9, a.Kl, a.Kr, tid, model);
  __syncthreads();
  if (tid == 0) {
    double g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = model.F[k];
    const bool ok = canon9(g) && good;                     // the norm and sign rule of sfm_twoview_ransac's F_out
#pragma unroll
    for (int k = 0; k < 9; ++k) Fn[k] = ok ? g[k] : 0.0;
    fn_ok = ok;
    if (a.F_out)
      for (int k = 0; k < 9; ++k) a.F_out[9 * (size_t)s + k] = Fn[k];
  }
  __syncthreads();
  const bool has_f = fn_ok != 0;
  int nin = 0, nf = 0, np = 0;
  for (int i = tid; i < n; i += kMatchThreads) {
    const size_t at = (size_t)base + i;
    const TvMatch mt = match_load(refine_view(a), (long long)at);
    const bool finite = refine_finite4(mt);
    const bool on = finite & (a.mask ? a.mask[at] != 0 : true);
    const double r = refine_residual(model.F, model.dF, mt.xl, mt.yl, mt.xr, mt.yr, nullptr);
    const bool in = (bool)((int)twoview_inlier(Fn, mt.xl, mt.yl, mt.xr, mt.yr, a.max_err2) & (int)has_f & (int)finite);
    PoseRays ray;
    const bool rays_ok = pose_rays_of(a.Kl, a.Kr, mt, ray);
    bool par;
    const bool front = (bool)((int)pose_front(P, P + 9, ray.a0, ray.a1, ray.b0, ray.b1, a.cos2_min, &par) & (int)rays_ok & (int)good);
    par = par & front;
    nin += in & on; nf += front & on; np += par & on;
    if (a.obs_res) a.obs_res[at] = (good & finite) ? r : __builtin_nan("");
    if (a.obs_inlier) a.obs_inlier[at] = in ? 1 : 0;
    if (a.obs_front) a.obs_front[at] = front ? (par ? 2 : 1) : 0;
    if (a.X_out) {
      double x[3];
      pose_midpoint(P, ray, x);
#pragma unroll
      for (int k = 0; k < 3; ++k) a.X_out[(size_t)k * a.M + at] = front ? x[k] : __builtin_nan("");
    }
  }
  nin = block_sum_int(nin, &total[0]);
  nf = block_sum_int(nf, &total[1]);
  np = block_sum_int(np, &total[2]);
  if (tid != 0) return;
  if (a.n_inliers) a.n_inliers[s] = nin;
  if (a.n_front) a.n_front[s] = nf;
  if (a.n_parallax) a.n_parallax[s] = np;
  // slot 1 takes the sets with a bad pose, slot 2 the other sets that had too few matches for a pass
  const bool refined = !(flags & (SFM_REFINE_BAD_POSE | SFM_REFINE_EMPTY | SFM_REFINE_TOO_FEW));
  if (a.summary) robust_summary_add(a.summary, refined, false, good, flags & SFM_REFINE_KEPT_INPUT, a.n_used[s], nin);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The outputs as device pointers, any of them null but R and t.
struct RefinePtrs {
  double *R, *t, *F, *cost, *info;
  int *n_used, *status;
  double* obs_res;
  unsigned char *obs_inlier, *obs_front;
  double* X;
  int *n_inliers, *n_front, *n_parallax;
  int64_t* summary;
};

// ... and as a host-pointer entry point keeps them for n sets of m matches.
struct RefineOut {
  HostOut<double> R, t, F, cost, info, res, X;
  HostOut<int> used, status, nin, nfront, npar;
  HostOut<unsigned char> inlier, front;
  HostOut<int64_t> summary;
  int want(size_t v, size_t m, double* R_out, double* t_out, double* F_out, double* cost_out, double* info_out, int* n_used, int* st,
           double* obs_res, unsigned char* obs_inlier, unsigned char* obs_front, double* X_out, int* n_inliers, int* n_front,
           int* n_parallax, int64_t* sum, hipStream_t s) {
    SFM_TRY(R.want(R_out, 9 * v, s)); SFM_TRY(t.want(t_out, 3 * v, s)); SFM_TRY(F.want(F_out, 9 * v, s));
    SFM_TRY(cost.want(cost_out, 2 * v, s)); SFM_TRY(info.want(info_out, 15 * v, s)); SFM_TRY(used.want(n_used, v, s));
    SFM_TRY(status.want(st, v, s)); SFM_TRY(res.want(obs_res, m, s)); SFM_TRY(inlier.want(obs_inlier, m, s));
    SFM_TRY(front.want(obs_front, m, s)); SFM_TRY(X.want(X_out, 3 * m, s)); SFM_TRY(nin.want(n_inliers, v, s));
    SFM_TRY(nfront.want(n_front, v, s)); SFM_TRY(npar.want(n_parallax, v, s)); return summary.want(sum, 6, s);
  }
  RefinePtrs dev() const {
    return {R.dev(), t.dev(), F.dev(), cost.dev(), info.dev(), used.dev(), status.dev(), res.dev(), inlier.dev(), front.dev(), X.dev(),
            nin.dev(), nfront.dev(), npar.dev(), summary.dev()};
  }
  int fetch(hipStream_t s) const {
    SFM_TRY(R.fetch(s)); SFM_TRY(t.fetch(s)); SFM_TRY(F.fetch(s)); SFM_TRY(cost.fetch(s)); SFM_TRY(info.fetch(s)); SFM_TRY(used.fetch(s));
    SFM_TRY(status.fetch(s)); SFM_TRY(res.fetch(s)); SFM_TRY(inlier.fetch(s)); SFM_TRY(front.fetch(s)); SFM_TRY(X.fetch(s));
    SFM_TRY(nin.fetch(s)); SFM_TRY(nfront.fetch(s)); SFM_TRY(npar.fetch(s)); return summary.fetch(s);
  }
};

// What a call keeps on the device besides the caller's arrays.
struct RefineWork {
  DevBuf<int> ptr, n_used, status;
};

// Everything the entry points refuse, without a device.
static int refine_check_args(const char* who, int n_sets, const int* set_ptr, long long M, const double* K_left, const double* K_right,
                             double lambda, int iters, double max_err2, double cos2_min) {
  if (!(lambda >= 0.0)) { set_error("%s: lambda = %g must be >= 0", who, lambda); return SFM_E_SHAPE; }
  if (iters < 0) { set_error("%s: iters = %d must be >= 0", who, iters); return SFM_E_SHAPE; }
  if (!(max_err2 >= 0.0)) { set_error("%s: max_err2 = %g must be >= 0", who, max_err2); return SFM_E_SHAPE; }
  if (!(cos2_min >= 0.0 && cos2_min <= 1.0)) { set_error("%s: cos2_min = %g must be in [0, 1]", who, cos2_min); return SFM_E_SHAPE; }
  SFM_TRY(robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true));
  SFM_TRY(pose_check_k(who, "K_left", K_left));
  return pose_check_k(who, "K_right", K_right);
}

// The one body of the entry points: checked arguments and device pointers in (n_sets > 0), the kernels enqueued on s out.
// w lives until the caller has waited for s.
static int refine_run(int n_sets, const int* set_ptr, long long M, const double* d_left, const double* d_right,
                      const unsigned char* d_mask, const double* d_R_in, const double* d_t_in, const double* K_left,
                      const double* K_right, double lambda, int iters, double max_err2, double cos2_min, const RefinePtrs& out,
                      RefineWork& w, hipStream_t s) {
  const size_t v = (size_t)n_sets;
  RefineArgs a = {};
  a.n_sets = n_sets; a.M = M; a.left = d_left; a.right = d_right; a.mask = d_mask; a.R_in = d_R_in; a.t_in = d_t_in;
  for (int k = 0; k < 9; ++k) { a.Kl[k] = K_left[k]; a.Kr[k] = K_right[k]; }
  a.lambda = lambda; a.iters = iters; a.max_err2 = max_err2; a.cos2_min = cos2_min;
  SFM_TRY(w.ptr.upload(set_ptr, v + 1, s));
  a.ptr = w.ptr.p;
  a.R_out = out.R; a.t_out = out.t; a.F_out = out.F; a.cost = out.cost; a.info = out.info; a.n_used = out.n_used; a.status = out.status;
  a.obs_res = out.obs_res; a.obs_inlier = out.obs_inlier; a.obs_front = out.obs_front; a.X_out = out.X; a.n_inliers = out.n_inliers;
  a.n_front = out.n_front; a.n_parallax = out.n_parallax; a.summary = reinterpret_cast<unsigned long long*>(out.summary);
  if (!a.n_used) { SFM_TRY(w.n_used.alloc(v, s)); a.n_used = w.n_used.p; }
  if (!a.status) { SFM_TRY(w.status.alloc(v, s)); a.status = w.status.p; }
  if (a.summary) SFM_HIP(hipMemsetAsync(a.summary, 0, 6 * sizeof(unsigned long long), s));
  refine_iterate_kernel<kRefThreads><<<n_sets, kRefThreads, 0, s>>>(a);
  refine_judge_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_twoview_refine_test(const double R[9], const double t[3], const double K_left[9], const double K_right[9], double xl, double yl,
                            double xr, double yr, double* r, double J[5]) {
  const char* who = "sfm_twoview_refine_test";
  if (!R || !t || !r || !J) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  SFM_TRY(pose_check_k(who, "K_left", K_left));
  SFM_TRY(pose_check_k(who, "K_right", K_right));
  RefineModel m;
  refine_model(R, t, K_left, K_right, m);
  *r = refine_residual(m.F, m.dF, xl, yl, xr, yr, J);
  return SFM_OK;
}

int sfm_twoview_refine_dev(int n_sets, const int* set_ptr, int64_t M, const double* d_left, const double* d_right,
                           const unsigned char* d_obs_mask, const double* d_R_in, const double* d_t_in, const double K_left[9],
                           const double K_right[9], double lambda, int iters, double max_err2, double cos2_min, double* d_R_out,
                           double* d_t_out, double* d_F_out, double* d_cost, double* d_info, int* d_n_used, int* d_status,
                           double* d_obs_res, unsigned char* d_obs_inlier, unsigned char* d_obs_front, double* d_X_out,
                           int* d_n_inliers, int* d_n_front, int* d_n_parallax, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_twoview_refine_dev";
  SFM_TRY(refine_check_args(who, n_sets, set_ptr, M, K_left, K_right, lambda, iters, max_err2, cos2_min));
  if (n_sets > 0 && (!d_R_out || !d_t_out || !d_R_in || !d_t_in || (M > 0 && (!d_left || !d_right)))) {
    set_error("%s: null pointer", who); return SFM_E_SHAPE;
  }
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_sets == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  RefineWork w;
  SFM_TRY(refine_run(n_sets, set_ptr, M, d_left, d_right, d_obs_mask, d_R_in, d_t_in, K_left, K_right, lambda, iters, max_err2, cos2_min,
                     RefinePtrs{d_R_out, d_t_out, d_F_out, d_cost, d_info, d_n_used, d_status, d_obs_res, d_obs_inlier, d_obs_front,
                                d_X_out, d_n_inliers, d_n_front, d_n_parallax, d_summary}, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_twoview_refine(int n_sets, const int* set_ptr, int64_t M, const double* left, const double* right, const unsigned char* obs_mask,
                       const double* R_in, const double* t_in, const double K_left[9], const double K_right[9], double lambda, int iters,
                       double max_err2, double cos2_min, double* R_out, double* t_out, double* F_out, double* cost, double* info,
                       int* n_used, int* status, double* obs_res, unsigned char* obs_inlier, unsigned char* obs_front, double* X_out,
                       int* n_inliers, int* n_front, int* n_parallax, int64_t* summary) {
  const char* who = "sfm_twoview_refine";
  SFM_TRY(refine_check_args(who, n_sets, set_ptr, M, K_left, K_right, lambda, iters, max_err2, cos2_min));
  if (n_sets > 0 && (!R_out || !t_out || !R_in || !t_in || (M > 0 && (!left || !right)))) {
    set_error("%s: null pointer", who); return SFM_E_SHAPE;
  }
  SFM_TRY(ensure_init());
  robust_summary_clear(summary);
  if (n_sets == 0) return SFM_OK;
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_sets, m = (size_t)M;
  DevBuf<double> dL, dR, dRin, dTin;
  DevBuf<unsigned char> dMask;
  RefineOut o;
  RefineWork w;
  SFM_TRY(dL.upload(left, 2 * m, s));
  SFM_TRY(dR.upload(right, 2 * m, s));
  SFM_TRY(dMask.upload_if(obs_mask, m, s));
  SFM_TRY(dRin.upload(R_in, 9 * v, s));
  SFM_TRY(dTin.upload(t_in, 3 * v, s));
  SFM_TRY(o.want(v, m, R_out, t_out, F_out, cost, info, n_used, status, obs_res, obs_inlier, obs_front, X_out, n_inliers, n_front,
                 n_parallax, summary, s));
  SFM_TRY(refine_run(n_sets, set_ptr, M, dL.p, dR.p, dMask.p, dRin.p, dTin.p, K_left, K_right, lambda, iters, max_err2, cos2_min, o.dev(),
                     w, s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

// TrackStore.refine_pairs: the pairs of table[ref][que] (sfm_track_pairs_dev, into pool buffers) and the refinement of their
// pose on the same stream, as sfm_twoview_pose_pairs poses them: only the count comes down between the two, no coordinate.
int sfm_twoview_refine_pairs(sfm_track_store* store, int ref, int que, const unsigned char* inlier, const double R_in[9],
                             const double t_in[3], const double K_left[9], const double K_right[9], double lambda, int iters,
                             double max_err2, double cos2_min, int* n, int* r_idx, int* q_idx, double R_out[9], double t_out[3],
                             double F_out[9], double cost[2], double info[15], int* n_used, int* status, double* obs_res,
                             unsigned char* obs_inlier, unsigned char* obs_front, double* X_out, int* n_inliers, int* n_front,
                             int* n_parallax) {
  const char* who = "sfm_twoview_refine_pairs";
  const int none[2] = {0, 0};
  SFM_TRY(refine_check_args(who, 1, none, 0, K_left, K_right, lambda, iters, max_err2, cos2_min));
  if (!n || !R_out || !t_out || !R_in || !t_in) { set_error("%s: n, R_in, t_in, R_out or t_out is NULL", who); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
  int64_t keys = 0;
  SFM_TRY(sfm_track_info(store, SFM_TRACK_INFO_N_KEYS, ref, &keys));
  const size_t cap = (size_t)(keys > 0 ? keys : 1);
  hipStream_t s = ctx().stream;
  DevBuf<int> dCnt, dR, dQ;
  DevBuf<double> dRef, dQue, dRin, dTin;
  SFM_TRY(dCnt.alloc(2, s)); SFM_TRY(dR.alloc(cap, s)); SFM_TRY(dQ.alloc(cap, s));
  SFM_TRY(dRef.alloc(3 * cap, s)); SFM_TRY(dQue.alloc(3 * cap, s));
  SFM_TRY(sfm_track_pairs_dev(store, ref, que, dCnt.p, dR.p, dQ.p, dRef.p, dQue.p, s));
  int cnt[2] = {0, 0};
  SFM_TRY(dCnt.download(cnt, 2, s));
  SFM_TRY(stream_sync(s));
  *n = cnt[0];
  if (cnt[1]) { set_error("%s: table %d row %d names a key the view %d does not have", who, ref, que, que); return SFM_E_SHAPE; }
  const size_t m = (size_t)cnt[0];
  const int set_ptr[2] = {0, cnt[0]};
  DevBuf<unsigned char> dMask;
  RefineOut o;
  RefineWork w;
  SFM_TRY(dMask.upload_if(inlier, m, s));
  SFM_TRY(dRin.upload(R_in, 9, s));
  SFM_TRY(dTin.upload(t_in, 3, s));
  SFM_TRY(o.want(1, m, R_out, t_out, F_out, cost, info, n_used, status, obs_res, obs_inlier, obs_front, X_out, n_inliers, n_front,
                 n_parallax, nullptr, s));
  // rows 0 and 1 of the (3, n) point arrays are the [2][n] coordinates as they are
  SFM_TRY(refine_run(1, set_ptr, cnt[0], dRef.p, dQue.p, dMask.p, dRin.p, dTin.p, K_left, K_right, lambda, iters, max_err2,
                     cos2_min, o.dev(), w, s));
  SFM_TRY(o.fetch(s));
  if (r_idx) SFM_TRY(dR.download(r_idx, m, s));
  if (q_idx) SFM_TRY(dQ.download(q_idx, m, s));
  return stream_sync(s);
}

}  // extern "C"
