// sfm_tri_ransac.hip — robust triangulation of ragged multi-view tracks: pair hypotheses, inlier refit (gfx950).
//
// sfm_tri_tracks / sfm_ba_refine_points solve a point by least squares over EVERY observation of its track; here the
// consistent subset of the track is found first (the rule is stated in sfm_hip.h, block "robust triangulation"):
//   centres  free form only: one thread per view, C = -M^-1 p4 of projs = [M | p4]
//   score    a group of G lanes owns a point; the track is staged in an LDS tile (per observation u, v, the twelve
//            projection entries and the scale); lane l takes hypotheses l, l + G, ..., forms its point and the gates from
//            its pair alone, then walks the tile -- every lane of the group reads the same address, a broadcast -- and
//            counts inliers in an integer register; one lexicographic arg-best over the group on (count, cosine, h)
//   refit    lane l takes observations l, l + G, ... in track order: the inhomogeneous linear solve over the winner's
//            inliers, `iters` damped Gauss-Newton steps with the mask fixed (track_view / track_solve3 of
//            sfm_track_obs.h, the nine sums through group_sum<G>), then the judgement of the point that stands
// No floating-point value is summed across lanes in `score`, and nothing is accumulated with atomics but the six summary
// counters: the winner does not depend on G, on the other points of the call or on timing; a point's bits depend on
// its track, its input, the options and G only.  The summary counters and the host frame of the entry points are
// sfm_robust.h's, shared with the resection and the two-view geometry; the scoring (one lane per hypothesis, a cosine
// tie-break) is this file's own.
#include <climits>
#include <cmath>

#include "sfm_ba.h"
#include "sfm_track_obs.h"      // contraction is off from here on
#include "sfm_robust.h"

namespace sfm {

constexpr int kRanSlots = 6;        // observations per lane of the LDS tile: a track of up to 6 G observations is staged once
constexpr int kRanObs = 15;         // doubles per staged observation: u, v, P[12], scale
constexpr int kRanBlock = 64;       // 64 * 6 * 15 doubles = 46 080 bytes of LDS: three workgroups per CU (160 KB)

static_assert(sizeof(CamPrep) == 19 * sizeof(double), "the centres of the prepared cameras are read with a stride of 19 doubles");

struct RansacArgs {
  TrackView t;                  // null input rows stand for (0, 0, 0, 1)
  const double* centres;        // camera c's centre at centres + centre_stride * c
  int centre_stride;
  const double* cam_scale;      // [V] or null (= 1)
  double max_err2, cos_min_angle;
  int max_hyp;
  double lambda;
  int iters;
  int* best_hyp;                // [n_pts] score -> refit, and an output
  int* hyp_count;               // [n_pts] score -> refit: the winner's inlier count
  double* hyp_x;                // [3][n_pts] score -> refit: the winner's point
  unsigned char* obs_inlier;    // [M] or null
  int* n_inliers;               // [n_pts] or null
  int* status;                  // [n_pts] or null
  unsigned long long* summary;  // [6]
};

// Is the observation an inlier of (x, 1)?  track_project, then the observation test (sfm_obs_test.h).
__device__ __forceinline__ bool ransac_inlier(const double* P, double ku, double kv, double scale, double x0, double x1, double x2,
                                              double max_err2) {
  double s[3];
  track_project(P, x0, x1, x2, 1.0, s);
  return obs_passes(s, obs_err2(s, ku, kv, scale), max_err2);
}

// The two rows a = u p3 - p1 and a = v p3 - p2 of an observation, added to N = sum a[0:3] a[0:3]^T and g = -sum a[3] a[0:3].
__device__ __forceinline__ void ransac_rows(const double* P, double ku, double kv, TrackSums& S) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double k = r ? kv : ku;
    const double a0 = __builtin_fma(k, P[8], -P[4 * r]), a1 = __builtin_fma(k, P[9], -P[4 * r + 1]);
    const double a2 = __builtin_fma(k, P[10], -P[4 * r + 2]), a3 = __builtin_fma(k, P[11], -P[4 * r + 3]);
    S.a00 = __builtin_fma(a0, a0, S.a00);
    S.a10 = __builtin_fma(a1, a0, S.a10);
    S.a11 = __builtin_fma(a1, a1, S.a11);
    S.a20 = __builtin_fma(a2, a0, S.a20);
    S.a21 = __builtin_fma(a2, a1, S.a21);
    S.a22 = __builtin_fma(a2, a2, S.a22);
    S.b0 = __builtin_fma(-a3, a0, S.b0);
    S.b1 = __builtin_fma(-a3, a1, S.b1);
    S.b2 = __builtin_fma(-a3, a2, S.b2);
  }
}

// Hypothesis h of a track of n observations starting at beg: its point, the cosine between the rays to the two
// generating cameras, and whether it is valid (steps 2 to 4 of the rule).  One lane, the pair alone.
__device__ __forceinline__ bool ransac_hypothesis(const RansacArgs& a, int beg, int n, long long P, int h, double& x0, double& x1,
                                                  double& x2, double& cs) {
  int i, j;
  ransac_pair_of(n, ransac_pair_number(P, a.max_hyp, h), &i, &j);
  const int oi = beg + i, oj = beg + j;
  const int ci = a.t.cam_idx[oi], cj = a.t.cam_idx[oj];
  const double* Pi = a.t.projs + 12 * (size_t)ci;
  const double* Pj = a.t.projs + 12 * (size_t)cj;
  const double ui = a.t.u[oi], vi = a.t.v[oi], uj = a.t.u[oj], vj = a.t.v[oj];
  TrackSums S = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  ransac_rows(Pi, ui, vi, S);
  ransac_rows(Pj, uj, vj, S);
  if (!track_solve3(S.a00, S.a10, S.a11, S.a20, S.a21, S.a22, S.b0, S.b1, S.b2, x0, x1, x2)) return false;
  const double* Ci = a.centres + (size_t)a.centre_stride * ci;
  const double* Cj = a.centres + (size_t)a.centre_stride * cj;
  const double d0 = Ci[0] - x0, d1 = Ci[1] - x1, d2 = Ci[2] - x2;
  const double e0 = Cj[0] - x0, e1 = Cj[1] - x1, e2 = Cj[2] - x2;
  const double di = rsqrt_nr(__builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0)));
  const double ei = rsqrt_nr(__builtin_fma(e2, e2, __builtin_fma(e1, e1, e0 * e0)));
  cs = __builtin_fma(d2 * di, e2 * ei, __builtin_fma(d1 * di, e1 * ei, (d0 * di) * (e0 * ei)));
  if (!isfinite(cs)) return false;
  if (a.cos_min_angle < 1.0 && cs > a.cos_min_angle) return false;
  return ransac_inlier(Pi, ui, vi, a.cam_scale ? a.cam_scale[ci] : 1.0, x0, x1, x2, a.max_err2) &&
         ransac_inlier(Pj, uj, vj, a.cam_scale ? a.cam_scale[cj] : 1.0, x0, x1, x2, a.max_err2);
}

// A track of up to kRanSlots * G observations is staged once, before the first batch of hypotheses.  A longer one is
// staged tile by tile for every batch of G hypotheses, each lane keeping the running count of its own (the fallback:
// any length, nothing held per observation).
template <int G>
__global__ __launch_bounds__(kRanBlock) void tri_ransac_score_kernel(RansacArgs a) {
  constexpr int kCap = kRanSlots * G;
  __shared__ double tile_all[kRanBlock * kRanSlots * kRanObs];
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)(t / G), lane = (int)(threadIdx.x % G);
  if (p >= a.t.n_pts) return;               // whole groups leave together
  double* tile = tile_all + (size_t)(threadIdx.x - lane) * kRanSlots * kRanObs;      // kCap observations of this group
  const int beg = a.t.pt_ptr[p], end = a.t.pt_ptr[p + 1], n = end - beg;

  int best_cnt = 0, best_h = -1;
  double best_cos = 2.0, b0 = 0, b1 = 0, b2 = 0;
  if (n >= 2) {
    const long long P = ransac_pair_count(n);
    const int H = hyp_count(P, a.max_hyp);
    const bool one = n <= kCap;
    for (int hb = 0; hb < H; hb += G) {
      const int h = hb + lane;
      double x0 = 0, x1 = 0, x2 = 0, cs = 2.0;
      const bool valid = h < H && ransac_hypothesis(a, beg, n, P, h, x0, x1, x2, cs);
      int cnt = 0;
      for (int tb = beg; tb < end; tb += kCap) {
        const int te = min(end, tb + kCap);
        if (!one || hb == 0) {
          for (int o = tb + lane; o < te; o += G) {
            const int c = a.t.cam_idx[o];
            const double* P12 = a.t.projs + 12 * (size_t)c;
            double* w = tile + kRanObs * (o - tb);
            w[0] = a.t.u[o]; w[1] = a.t.v[o];
#pragma unroll
            for (int k = 0; k < 12; ++k) w[2 + k] = P12[k];
            w[14] = a.cam_scale ? a.cam_scale[c] : 1.0;
          }
          group_lds_sync();
        }
        if (valid) {
          // one wave per SIMD is resident (the tile): four independent tests in flight are what hides their latency
#pragma unroll 4
          for (int k = 0; k < te - tb; ++k) {
            const double* w = tile + kRanObs * k;
            cnt += ransac_inlier(w + 2, w[0], w[1], w[14], x0, x1, x2, a.max_err2);
          }
        }
        if (!one) group_lds_sync();
      }
      // h ascends on a lane: only a strictly better (count, cosine) replaces what the lane holds
      if (valid && (cnt > best_cnt || (cnt == best_cnt && cs < best_cos))) {
        best_cnt = cnt; best_cos = cs; best_h = h;
        b0 = x0; b1 = x1; b2 = x2;
      }
    }
  }

  // lexicographic arg-best over the group: the count, then the smaller cosine, then the lower h
  const int own_h = best_h;
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    const int oc = __shfl_xor(best_cnt, off, 64), oh = __shfl_xor(best_h, off, 64);
    const double os = __shfl_xor(best_cos, off, 64);
    const bool better = oh >= 0 && (best_h < 0 || oc > best_cnt ||
                                    (oc == best_cnt && (os < best_cos || (os == best_cos && oh < best_h))));
    if (better) { best_cnt = oc; best_cos = os; best_h = oh; }
  }
  if (best_h >= 0 && own_h == best_h) {      // the lane that formed the winner still holds its point
    a.hyp_x[p] = b0; a.hyp_x[(size_t)a.t.n_pts + p] = b1; a.hyp_x[2 * (size_t)a.t.n_pts + p] = b2;
  }
  if (lane == 0) { a.best_hyp[p] = best_h; a.hyp_count[p] = best_cnt; }
}

template <int G>
__global__ __launch_bounds__(256) void tri_ransac_refit_kernel(RansacArgs a) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)(t / G), lane = (int)(threadIdx.x % G);
  if (p >= a.t.n_pts) return;               // whole groups leave together
  const int beg = a.t.pt_ptr[p], end = a.t.pt_ptr[p + 1], n = end - beg;
  double x0 = 0, x1 = 0, x2 = 0, x3 = 1.0;
  if (a.t.xin[0]) {
    x0 = a.t.xin[0][p]; x1 = a.t.xin[1][p]; x2 = a.t.xin[2][p];
    if (a.t.xin[3]) x3 = a.t.xin[3][p];
  }
  const int bh = a.best_hyp[p];
  int flags = n < 2 ? SFM_RANSAC_TOO_FEW : (bh < 0 ? SFM_RANSAC_NO_MODEL : 0);
  if (n >= 2 && ransac_pair_count(n) > (long long)a.max_hyp) flags |= SFM_RANSAC_SAMPLED;
  const bool solved = !(flags & (SFM_RANSAC_TOO_FEW | SFM_RANSAC_NO_MODEL));

  if (solved) {
    const double h0 = a.hyp_x[p], h1 = a.hyp_x[(size_t)a.t.n_pts + p], h2 = a.hyp_x[2 * (size_t)a.t.n_pts + p];
    const int hc = a.hyp_count[p];
    // the inhomogeneous solve over the winner's inliers, then the damped steps with that mask
    double y0 = 0, y1 = 0, y2 = 0;
    bool ok = true;
    for (int it = -1; ok && it < a.iters; ++it) {
      TrackSums S = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int o = beg + lane; o < end; o += G) {
        const int c = a.t.cam_idx[o];
        const double* P = a.t.projs + 12 * (size_t)c;
        const double ku = a.t.u[o], kv = a.t.v[o];
        if (!ransac_inlier(P, ku, kv, a.cam_scale ? a.cam_scale[c] : 1.0, h0, h1, h2, a.max_err2)) continue;
        if (it < 0) ransac_rows(P, ku, kv, S);
        else track_view(P, ku, kv, y0, y1, y2, 1.0, S);
      }
      const double lam = it < 0 ? 0.0 : a.lambda;
      const double a00 = group_sum<G>(S.a00) + lam, a10 = group_sum<G>(S.a10), a11 = group_sum<G>(S.a11) + lam;
      const double a20 = group_sum<G>(S.a20), a21 = group_sum<G>(S.a21), a22 = group_sum<G>(S.a22) + lam;
      const double g0 = group_sum<G>(S.b0), g1 = group_sum<G>(S.b1), g2 = group_sum<G>(S.b2);
      double d0, d1, d2;
      ok = track_solve3(a00, a10, a11, a20, a21, a22, g0, g1, g2, d0, d1, d2);      // the same bits on every lane of the group
      if (it < 0) { y0 = d0; y1 = d1; y2 = d2; }
      else { y0 -= d0; y1 -= d1; y2 -= d2; }
    }
    ok = ok && isfinite(y0) && isfinite(y1) && isfinite(y2);
    int rc = 0;
    if (ok) {
      for (int o = beg + lane; o < end; o += G) {
        const int c = a.t.cam_idx[o];
        rc += ransac_inlier(a.t.projs + 12 * (size_t)c, a.t.u[o], a.t.v[o], a.cam_scale ? a.cam_scale[c] : 1.0, y0, y1, y2, a.max_err2);
      }
      rc = group_sum<G>(rc);
    }
    if (ok && rc >= hc) { x0 = y0; x1 = y1; x2 = y2; }
    else { x0 = h0; x1 = h1; x2 = h2; flags |= SFM_RANSAC_KEPT_HYPOTHESIS; }
    x3 = 1.0;
  }

  // the judgement of the point that stands
  int nin = 0;
  for (int o = beg + lane; o < end; o += G) {
    bool in = false;
    if (solved) {
      const int c = a.t.cam_idx[o];
      in = ransac_inlier(a.t.projs + 12 * (size_t)c, a.t.u[o], a.t.v[o], a.cam_scale ? a.cam_scale[c] : 1.0, x0, x1, x2, a.max_err2);
    }
    if (a.obs_inlier) a.obs_inlier[o] = in ? 1 : 0;
    nin += in;
  }
  nin = group_sum<G>(nin);
  if (lane != 0) return;
  a.t.xout[0][p] = x0; a.t.xout[1][p] = x1; a.t.xout[2][p] = x2;
  if (a.t.xout[3]) a.t.xout[3][p] = x3;
  if (a.n_inliers) a.n_inliers[p] = nin;
  if (a.status) a.status[p] = flags;
  robust_summary_add(a.summary, solved, false, flags & SFM_RANSAC_TOO_FEW, flags & SFM_RANSAC_KEPT_HYPOTHESIS, n, nin);
}

// C = -M^-1 p4 of every projection [M | p4] (the free form; the resident scene reads the centres of its cameras)
__global__ void tri_ransac_centres_kernel(int V, const double* __restrict__ projs, double* __restrict__ centres) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= V) return;
  const double* P = projs + 12 * (size_t)c;
  const double c00 = P[5] * P[10] - P[6] * P[9], c01 = P[6] * P[8] - P[4] * P[10], c02 = P[4] * P[9] - P[5] * P[8];
  const double det = P[0] * c00 + P[1] * c01 + P[2] * c02;
  const double id = 1.0 / det;
  const double m[9] = {c00, P[2] * P[9] - P[1] * P[10], P[1] * P[6] - P[2] * P[5],
                       c01, P[0] * P[10] - P[2] * P[8], P[2] * P[4] - P[0] * P[6],
                       c02, P[1] * P[8] - P[0] * P[9], P[0] * P[5] - P[1] * P[4]};      // adjugate, row-major
#pragma unroll
  for (int r = 0; r < 3; ++r) centres[3 * (size_t)c + r] = -(m[3 * r] * P[3] + m[3 * r + 1] * P[7] + m[3 * r + 2] * P[11]) * id;
}

#pragma clang fp contract(on)

template <int G>
static void launch_ransac(const RansacArgs& a, hipStream_t s) {
  const long long threads = (long long)a.t.n_pts * G;
  tri_ransac_score_kernel<G><<<dim3((unsigned)((threads + kRanBlock - 1) / kRanBlock)), dim3(kRanBlock), 0, s>>>(a);
  tri_ransac_refit_kernel<G><<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(a);
}

static int ransac_check_args(const char* who, int n_pts, int n_views, long long M, double max_err2, double cos_min_angle,
                             int max_hyp, double lambda, int iters, int group) {
  if (n_pts < 0 || n_views < 1 || M < 0 || M > INT_MAX) {
    set_error("%s: bad sizes n_pts=%d n_views=%d M=%lld", who, n_pts, n_views, M);
    return SFM_E_SHAPE;
  }
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, lambda, iters));
  if (!(cos_min_angle >= -1.0)) { set_error("%s: cos_min_angle = %g must be >= -1 (>= 1 switches the gate off)", who, cos_min_angle); return SFM_E_SHAPE; }
  return group_width_check(who, group);
}

// What a call keeps on the device besides the caller's arrays.
struct RansacWork {
  RobustStandIns stand_in;
  DevBuf<int> hyp_count;
  DevBuf<double> hyp_x, centres;      // centres: the free form only
};

// Enqueue both kernels on s; the CSR has been validated, max_track is its longest track.  a.best_hyp / a.summary may be
// null: the work buffers stand in.  `group` = 0: the rule of sfm_tri_tracks unchanged -- the
// narrowest group whose tile holds the longest track, widened while the call is short of waves.
static int ransac_enqueue(RansacArgs a, RansacWork& w, int group, long long M, int max_track, hipStream_t s) {
  const size_t n = (size_t)a.t.n_pts;
  if (a.max_hyp == 0) a.max_hyp = kHypDefault;
  SFM_TRY(w.stand_in.fill(a, n, false, s));      // the refit tests a.status itself
  SFM_TRY(w.hyp_count.alloc(n, s));
  SFM_TRY(w.hyp_x.alloc(3 * n, s));
  a.hyp_count = w.hyp_count.p; a.hyp_x = w.hyp_x.p;
  if (a.t.n_pts <= 0) return SFM_OK;
  const int g = group ? group : sfm_tri_tracks_auto_group(a.t.n_pts, M, max_track);
  dispatch_group<1>(g, [&](auto G) { launch_ransac<decltype(G)::value>(a, s); });
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// The one body of sfm_tri_tracks_ransac and sfm_tri_tracks_ransac_dev: checked arguments and device pointers in
// (n_pts > 0), the kernels enqueued on s out.  w lives until the caller has waited for s.
static int ransac_run(const char* who, int n_pts, int n_views, long long M, const int* d_pt_ptr, const int* d_cam_idx,
                      const double* d_uv, const double* d_projs, const double* d_cam_scale, double max_err2, double cos_min_angle,
                      int max_hyp, double lambda, int iters, int group, const double* d_X_init, double* d_X_out,
                      const RobustPtrs& out, RansacWork& w, hipStream_t s) {
  int max_track = 0;
  SFM_TRY(tracks_validate(who, n_pts, n_views, M, d_pt_ptr, d_cam_idx, &max_track, s));
  SFM_TRY(w.centres.alloc(3 * (size_t)n_views, s));
  tri_ransac_centres_kernel<<<(n_views + 255) / 256, 256, 0, s>>>(n_views, d_projs, w.centres.p);
  SFM_HIP(hipGetLastError());
  RansacArgs a = {};
  a.t = track_view_free(n_pts, n_views, M, d_pt_ptr, d_cam_idx, d_uv, d_projs, d_X_init, d_X_out);
  a.centres = w.centres.p; a.centre_stride = 3; a.cam_scale = d_cam_scale;
  a.max_err2 = max_err2; a.cos_min_angle = cos_min_angle; a.max_hyp = max_hyp; a.lambda = lambda; a.iters = iters;
  out.into(a);
  return ransac_enqueue(a, w, group, M, max_track, s);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_tri_ransac_pair(int n, int max_hyp, int h, int* i, int* j) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (n < 2 || max_hyp < 1 || max_hyp > kHypMax) return 0;
  const long long P = ransac_pair_count(n);
  const int H = hyp_count(P, max_hyp);
  if (h >= 0 && h < H && i != nullptr && j != nullptr) ransac_pair_of(n, ransac_pair_number(P, max_hyp, h), i, j);
  return H;
}

int sfm_tri_tracks_ransac_dev(int n_pts, int n_views, int64_t M, const int* d_pt_ptr, const int* d_cam_idx, const double* d_uv,
                              const double* d_projs, const double* d_cam_scale, double max_err2, double cos_min_angle,
                              int max_hyp, double lambda, int iters, int group, const double* d_X_init, double* d_X_out,
                              unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_status, int64_t* d_summary,
                              void* hip_stream) {
  const char* who = "sfm_tri_tracks_ransac_dev";
  SFM_TRY(ensure_init());
  SFM_TRY(ransac_check_args(who, n_pts, n_views, M, max_err2, cos_min_angle, max_hyp, lambda, iters, group));
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_pts == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  SFM_TRY(tracks_check_ptrs(who, "null device pointer", M, d_pt_ptr, d_cam_idx, d_uv, d_projs, d_X_out));
  RansacWork w;
  SFM_TRY(ransac_run(who, n_pts, n_views, M, d_pt_ptr, d_cam_idx, d_uv, d_projs, d_cam_scale, max_err2, cos_min_angle, max_hyp,
                     lambda, iters, group, d_X_init, d_X_out, RobustPtrs{d_obs_inlier, d_n_inliers, d_best_hyp, d_status, d_summary},
                     w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_tri_tracks_ransac(int n_pts, int n_views, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv,
                          const double* projs, const double* cam_scale, double max_err2, double cos_min_angle, int max_hyp,
                          double lambda, int iters, int group, const double* X_init, double* X_out, unsigned char* obs_inlier,
                          int* n_inliers, int* best_hyp, int* status, int64_t* summary) {
  const char* who = "sfm_tri_tracks_ransac";
  SFM_TRY(ensure_init());
  SFM_TRY(ransac_check_args(who, n_pts, n_views, M, max_err2, cos_min_angle, max_hyp, lambda, iters, group));
  robust_summary_clear(summary);
  if (n_pts == 0) return SFM_OK;
  SFM_TRY(tracks_check_ptrs(who, "null pointer", M, pt_ptr, cam_idx, uv, projs, X_out));
  hipStream_t s = ctx().stream;
  const size_t n = (size_t)n_pts, m = (size_t)M;
  DevBuf<int> dPtr, dCam;
  DevBuf<double> dUV, dP, dSc, dX;
  HostOut<double> oX;
  RobustOut o;
  RansacWork w;
  SFM_TRY(dPtr.upload(pt_ptr, n + 1, s));
  SFM_TRY(dCam.upload(cam_idx, m, s));
  SFM_TRY(dUV.upload(uv, 2 * m, s));
  SFM_TRY(dP.upload(projs, 12 * (size_t)n_views, s));
  SFM_TRY(dSc.upload_if(cam_scale, (size_t)n_views, s));
  SFM_TRY(dX.upload_if(X_init, 4 * n, s));
  SFM_TRY(oX.want(X_out, 4 * n, s));
  SFM_TRY(o.want(m, n, obs_inlier, n_inliers, best_hyp, status, summary, s));
  SFM_TRY(ransac_run(who, n_pts, n_views, M, dPtr.p, dCam.p, dUV.p, dP.p, dSc.p, max_err2, cos_min_angle, max_hyp, lambda, iters,
                     group, dX.p, oX.dev(), o.dev(), w, s));
  SFM_TRY(oX.fetch(s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

int sfm_ba_retriangulate(sfm_ba_problem* p, double max_err2, double cos_min_angle, int max_hyp, double lambda, int iters,
                         int group, const double* cam_scale, unsigned char* obs_inlier, int* n_inliers, int* best_hyp,
                         int* status, int64_t* summary) {
  const char* who = "sfm_ba_retriangulate";
  SFM_TRY(ba_check_handle(p));
  BaDev& d = p->dev;
  SFM_TRY(ransac_check_args(who, d.N, d.V > 0 ? d.V : 1, d.M, max_err2, cos_min_angle, max_hyp, lambda, iters, group));
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  robust_summary_clear(summary);
  if (d.N == 0) return SFM_OK;
  SFM_TRY(ba_prepared_cameras(p, who));                  // the expanded cameras the linearisation reads
  hipStream_t s = p->stream;
  const size_t n = (size_t)d.N, m = (size_t)d.M;
  DevBuf<double> dP, dSc;
  RobustOut o;
  RansacWork w;
  RansacArgs a = {};
  SFM_TRY(track_view_resident(p, dP, &a.t));
  SFM_TRY(dSc.upload_if(cam_scale, (size_t)d.V, s));
  if (cam_scale) p->upload_bytes += (long long)(sizeof(double) * d.V);
  SFM_TRY(o.want(m, n, obs_inlier, n_inliers, best_hyp, status, summary, s));
  a.centres = d.prep[p->cur]->C; a.centre_stride = 19;      // the centres of the prepared cameras
  a.cam_scale = dSc.p;
  a.max_err2 = max_err2; a.cos_min_angle = cos_min_angle; a.max_hyp = max_hyp; a.lambda = lambda; a.iters = iters;
  o.dev().into(a);
  SFM_TRY(ransac_enqueue(a, w, group, d.M, p->max_track, s));
  SFM_TRY(ba_reset_stats(p));                            // new points, as after sfm_ba_set_points
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

}  // extern "C"

