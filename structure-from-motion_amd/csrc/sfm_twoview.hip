// sfm_twoview.hip — robust two-view geometry: sampled eight-point hypotheses, inlier refit (gfx950).
//
// sfm_fundamental_ransac scores host-drawn samples by an algebraic residual on normalised coordinates and returns the best
// eight-point matrix as it is.  Here the consistent subset of the matches between two views is found by the rule stated in
// sfm_hip.h, block "robust two-view geometry", for a batch of sets of matches in one call:
//   norm     one workgroup per set: the Hartley transforms over all matches of the set (slice-ordered sums), the normalised
//            matches [M][4] and T_l, T_r
//   hyp      one wave per (set, hypothesis): the stratified sample (sfm_hyp_number.h), the eight-point solve of
//            fund_eight_point_kernel (sfm_eight_point.h) without its division, de-normalisation, scaling, the sample gate
//   score    the hot path: a workgroup of 256 owns 1 024 matches of one set, four per lane, in registers; the set's matrices
//            pass through LDS in batches of 64 hypotheses (4.6 KB), every lane reads the matrix under test from the same
//            address (a broadcast), tests its four matches without a branch, a wave adds the popcounts of its four ballots
//            and issues one integer atomicAdd per hypothesis
//   pick     one wave per set: the lexicographic arg-best over (count, h)
//   refit    one workgroup per set, 1 024 matches at a time in every pass: the mask recomputed from the standing matrix,
//            Hartley transforms over the inliers, the 45 moment sums of their design rows, the 9x9 eigenproblem by
//            jacobi_rows_wave<9> on one wave, the count of the result and the acceptance
//   judge    one workgroup per set: obs_inlier, n_inliers and the summary of the matrix that stands
// One body per kernel serves every set size.  No floating-point value is accumulated with an atomic; the counts are
// integers; every floating-point sum over matches is formed per slice of 64 consecutive matches and the slices are added
// in ascending order: a set's bits depend on its own matches and the options only.
// Shared with the robust resection, in sfm_robust.h: the plan of the hypotheses (HypPlan, hyp_owner), the batch loop of
// `score` (robust_score_block), the tie rule of `pick` (wave_arg_best), the block reductions of `norm`, `refit` and `judge`
// (block_count, slice_totals, block_sum_int), the summary and the host frame.  Shared with the robust homography, in
// sfm_match_norm.h: the match and its load, the Hartley pass with its slice-ordered sums, the scaling of a 3x3 matrix.
#include <climits>
#include <cmath>

#include "sfm_eight_point.h"   // default contraction, as in sfm_epipolar.hip
#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"
#include "sfm_match_norm.h"     // the match, the Hartley pass and the scaling, shared with sfm_homography.hip

namespace sfm {

constexpr int kTvMinSet = 9;          // a set needs one match besides a sample's eight
constexpr int kTvMinCount = 9;        // ... and so does a winner
constexpr int kTvThreads = kMatchThreads;
constexpr int kTvPerLane = kMatchPerLane;
constexpr int kTvBlockObs = kMatchBlockObs;               // 1 024 matches per workgroup and pass
constexpr int kTvBatch = 64;          // hypotheses per LDS batch: 64 x 9 doubles = 4 608 bytes
constexpr int kTvRows = kMatchRows;
constexpr int kTvMoments = kMatchMoments;                 // upper triangle of the 9x9 moment matrix

struct TvArgs {
  int n_sets;
  long long M;
  const int* ptr;               // [n_sets + 1]
  const double* left;           // [2][M]
  const double* right;          // [2][M]
  const int* hyp_off;           // [n_sets + 1] first hypothesis of every set (a set below nine matches has none)
  const int2* blocks;           // score: workgroup -> (set, first of its 1 024 matches, relative)
  double max_err2;
  int max_hyp, iters;
  double* pairs;                // [M][4] normalised matches
  double* T;                    // [n_sets][2][9] T_l, T_r
  double* hyp_F;                // [hypotheses][9]
  unsigned char* hyp_ok;        // [hypotheses]
  int* counts;                  // [hypotheses]
  int* win_count;               // [n_sets]
  double* F_out;                // [n_sets][9]
  int* best_hyp;                // [n_sets]
  int* status;                  // [n_sets]
  unsigned char* obs_inlier;    // [M] or null
  int* n_inliers;               // [n_sets] or null
  unsigned long long* summary;  // [6]
};

__device__ __forceinline__ MatchView tv_view(const TvArgs& a) { return {a.left, a.right, a.M}; }

__device__ __forceinline__ TvMatch tv_load(const TvArgs& a, long long i) { return match_load(tv_view(a), i); }

__device__ __forceinline__ bool tv_inlier(const double (&F)[9], const TvMatch& m, double max_err2) {
  return twoview_inlier(F, m.xl, m.yl, m.xr, m.yr, max_err2);
}

// T_r^T f2 T_l, scaled by canon9; false if the result is not finite or zero.
__device__ __forceinline__ bool tv_denorm_canon(const double (&f)[9], const double (&tl)[9], const double (&tr)[9], double (&g)[9]) {
  double m[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) m[3 * r + c] = __builtin_fma(tr[6 + r], f[6 + c], __builtin_fma(tr[3 + r], f[3 + c], tr[r] * f[c]));      // T_r^T f
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      g[3 * r + c] = __builtin_fma(m[3 * r + 2], tl[6 + c], __builtin_fma(m[3 * r + 1], tl[3 + c], m[3 * r] * tl[c]));
  return canon9(g);
}

// ---------------------------------------------------------------------------------------------
// norm
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTvThreads) void twoview_norm_kernel(TvArgs a) {
  __shared__ double red[kTvRows][kTvMoments];
  __shared__ double sums[kTvMoments];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  if (n < kTvMinSet) return;
  int count;
  const TvNorm t = tv_hartley(tv_view(a), base, n, [](const TvMatch&) { return true; }, tid, red, sums, &count);
  for (int i = tid; i < n; i += kTvThreads) {
    double p[4];
    tv_normalise(t, tv_load(a, (long long)base + i), p);
    double* out = a.pairs + 4 * ((size_t)base + i);
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = p[3];
  }
  if (tid == 0) {
    double tl[9], tr[9];
    tv_transforms(t, tl, tr);
    // a transform that is not finite (a NaN coordinate, identical points) leaves NaN here: every hypothesis is invalid
    const double poison = tv_norm_finite(t) ? 0.0 : __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 9; ++k) { a.T[18 * (size_t)s + k] = tl[k] + poison; a.T[18 * (size_t)s + 9 + k] = tr[k] + poison; }
  }
}

// ---------------------------------------------------------------------------------------------
// hyp: the matrix of a sample
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void twoview_hyp_kernel(TvArgs a, int n_hyp) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= n_hyp) return;
  const int s = hyp_owner(a.hyp_off, a.n_sets, g), h = g - a.hyp_off[s];
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int idx = twoview_sample_index(n, h, lane & 7);
  double row[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) row[c] = 0.0;
  if (lane < 8) {
    eight_point_row(a.pairs + 4 * ((size_t)base + idx), row);
  } else if (lane >= 16 && lane < 25) {
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = (c == lane - 16) ? 1.0 : 0.0;
  }
  double f[9], F[9];
  eight_point_null_vector(row, lane, f);
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = 0.0;
  int ok = 0;
  if (lane == 0) {
    double f2[9], tl[9], tr[9];
    const int st = eight_point_project(f, f2);
#pragma unroll
    for (int k = 0; k < 9; ++k) { tl[k] = a.T[18 * (size_t)s + k]; tr[k] = a.T[18 * (size_t)s + 9 + k]; }
    ok = tv_denorm_canon(f2, tl, tr, F) && st == SFM_OK;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = wave_lane0(F[k]);
  // the sample gate: the eight matches of the sample, one per lane
  const bool in = tv_inlier(F, tv_load(a, (long long)base + idx), a.max_err2);
  const unsigned long long gate = __ballot(in) & 0xffULL;
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.hyp_F[9 * (size_t)g + k] = F[k];
  a.hyp_ok[g] = (ok && gate == 0xffULL) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTvThreads) void twoview_score_kernel(TvArgs a) {
  __shared__ double Fm[kTvBatch * 9];
  __shared__ unsigned char okb[kTvBatch];
  const int tid = threadIdx.x;
  const int2 blk = a.blocks[blockIdx.x];
  const int s = blk.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  // four matches per lane, a wave's loads contiguous; a slot beyond the set holds NaN and is nobody's inlier
  TvMatch m[kTvPerLane];
#pragma unroll
  for (int k = 0; k < kTvPerLane; ++k) {
    const int i = blk.y + k * kTvThreads + tid;
    m[k] = tv_load(a, (long long)base + (i < n ? i : n - 1));
    if (!(i < n)) m[k].xl = __builtin_nan("");
  }
  robust_score_block<kTvThreads, kTvBatch, 9, 1, kTvPerLane>(
      a.hyp_F, a.hyp_ok, a.counts, h0, H, Fm, okb,
      [&](const double* F, int k) { return twoview_inlier(F, m[k].xl, m[k].yl, m[k].xr, m[k].yr, a.max_err2); });
}

// ---------------------------------------------------------------------------------------------
// pick: the winner of every set
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void twoview_pick_kernel(TvArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  int best_cnt, best_h;                                    // the first of the largest counts wins
  wave_arg_best(lane, H, [&](int h) { return a.hyp_ok[h0 + h] != 0; }, [&](int h) { return a.counts[h0 + h]; }, best_cnt, best_h);
  if (lane != 0) return;
  const bool won = best_cnt >= kTvMinCount;
  a.best_hyp[s] = won ? best_h : -1;
  a.win_count[s] = won ? best_cnt : 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.F_out[9 * (size_t)s + k] = won ? a.hyp_F[9 * (size_t)(h0 + best_h) + k] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// refit and acceptance
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int tv_count(const TvArgs& a, int base, int n, const double (&F)[9], int tid) {
  int total = 0;
  for (int blk = 0; blk < n; blk += kTvBlockObs) {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTvPerLane; ++k) {
      const int i = blk + k * kTvThreads + tid;
      if (i < n) mine += tv_inlier(F, tv_load(a, (long long)base + i), a.max_err2);
    }
    total += block_count(mine);
  }
  return total;
}

__global__ __launch_bounds__(kTvThreads) void twoview_refit_kernel(TvArgs a) {
  __shared__ double red[kTvRows][kTvMoments];
  __shared__ double sums[kTvMoments];
  __shared__ double cand[9];
  __shared__ int cand_ok;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int bh = a.best_hyp[s];
  int flags = n < kTvMinSet ? SFM_TWOVIEW_TOO_FEW : (bh < 0 ? SFM_TWOVIEW_NO_MODEL : 0);
  if (flags == 0) {
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = a.F_out[9 * (size_t)s + k];
    int standing = a.win_count[s], stood = 0;
    const int n_blocks = (n + kTvBlockObs - 1) / kTvBlockObs;
    // from here on every thread holds the same values: the branches are uniform
    for (int it = 0; it < a.iters; ++it) {
      int m;
      const TvNorm t = tv_hartley(tv_view(a), base, n, [&](const TvMatch& mt) { return tv_inlier(F, mt, a.max_err2); }, tid, red, sums, &m);
      if (!tv_norm_finite(t)) break;
      double run = 0;
      for (int blk = 0; blk < n_blocks; ++blk) {
        double acc[kTvMoments];
#pragma unroll
        for (int k = 0; k < kTvMoments; ++k) acc[k] = 0;
#pragma unroll
        for (int k = 0; k < kTvPerLane; ++k) {
          const int i = blk * kTvBlockObs + kTvPerLane * tid + k;
          if (i < n) {
            const TvMatch mt = tv_load(a, (long long)base + i);
            const bool in = tv_inlier(F, mt, a.max_err2);
            double p[4], row[9];
            tv_normalise(t, mt, p);
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = in ? p[c] : 0.0;
            eight_point_row(p, row);
            row[8] = in ? 1.0 : 0.0;
            int q = 0;
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
              for (int c = r; c < 9; ++c, ++q) acc[q] = __builtin_fma(row[r], row[c], acc[q]);
          }
        }
        tv_block_sums<kTvMoments>(acc, tid, red, sums, run, blk == 0, blk == n_blocks - 1);
      }
      if (tid < 64) {                                      // one wave: the eigenvector of the smallest eigenvalue of A^T A
        double row[9], f[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          const int r0 = min(tid, c), c0 = max(tid, c);    // entry (r0, c0) of the upper triangle, row-major
          const double v = sums[tid < 9 ? r0 * 9 - r0 * (r0 - 1) / 2 + (c0 - r0) : 0];
          row[c] = tid < 9 ? v : ((tid >= 16 && tid < 25 && c == tid - 16) ? 1.0 : 0.0);
        }
        eight_point_null_vector(row, tid, f);
        if (tid == 0) {
          double f2[9], tl[9], tr[9], g[9];
          const int st = eight_point_project(f, f2);
          tv_transforms(t, tl, tr);
          const bool ok = tv_denorm_canon(f2, tl, tr, g) && st == SFM_OK;
#pragma unroll
          for (int k = 0; k < 9; ++k) cand[k] = g[k];
          cand_ok = ok ? 1 : 0;
        }
      }
      __syncthreads();
      double G[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) G[k] = cand[k];
      const bool ok = cand_ok != 0;
      const int rc = tv_count(a, base, n, G, tid);         // its barriers also close the reads of cand
      if (!(ok && rc >= standing)) break;
#pragma unroll
      for (int k = 0; k < 9; ++k) F[k] = G[k];
      standing = rc;
      ++stood;
    }
    if (a.iters > 0 && stood == 0) flags |= SFM_TWOVIEW_KEPT_HYPOTHESIS;
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a.F_out[9 * (size_t)s + k] = F[k];
    }
  }
  if (tid == 0) a.status[s] = flags;
}

// ---------------------------------------------------------------------------------------------
// judge: what the matrix that stands makes of the matches
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTvThreads) void twoview_judge_kernel(TvArgs a) {
  __shared__ int total;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int flags = a.status[s];
  const bool solved = !(flags & (SFM_TWOVIEW_TOO_FEW | SFM_TWOVIEW_NO_MODEL));
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = a.F_out[9 * (size_t)s + k];
  int nin = 0;
  for (int i = tid; i < n; i += kTvThreads) {
    const bool in = solved & tv_inlier(F, tv_load(a, (long long)base + i), a.max_err2);
    if (a.obs_inlier) a.obs_inlier[(size_t)base + i] = in ? 1 : 0;
    nin += in;
  }
  nin = block_sum_int(nin, &total);
  if (tid != 0) return;
  if (a.n_inliers) a.n_inliers[s] = nin;
  robust_summary_add(a.summary, solved, false, flags & SFM_TWOVIEW_TOO_FEW, flags & SFM_TWOVIEW_KEPT_HYPOTHESIS, n, nin);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int twoview_check_sets(const char* who, int n_sets, const int* set_ptr, long long M) {
  return robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true);
}

// What a call keeps on the device besides the caller's arrays.
struct TwoviewWork {
  HypPlan plan;
  RobustStandIns stand_in;
  DevBuf<int> ptr, counts, win_count;
  DevBuf<double> pairs, T, hyp_F;
  DevBuf<unsigned char> hyp_ok;
};

// The one body of sfm_twoview_ransac and sfm_twoview_ransac_dev: checked arguments and device pointers in (n_sets > 0),
// the kernels enqueued on s out.  w lives until the caller has waited for s.
static int twoview_run(const char* who, int n_sets, const int* set_ptr, long long M, const double* d_left, const double* d_right,
                       double max_err2, int max_hyp, int iters, double* d_F_out, const RobustPtrs& out, TwoviewWork& w,
                       hipStream_t s) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  SFM_TRY(w.plan.build(who, n_sets, set_ptr, kTvBlockObs, INT_MAX / 16, [&](int, int n, long long& hyps) {
    hyps = max_hyp;
    return n >= kTvMinSet;
  }, s));
  const size_t v = (size_t)n_sets, nh = w.plan.n_hyp;
  TvArgs a = {};
  a.n_sets = n_sets; a.M = M; a.left = d_left; a.right = d_right;
  a.max_err2 = max_err2; a.max_hyp = max_hyp; a.iters = iters; a.F_out = d_F_out;
  out.into(a);
  SFM_TRY(w.ptr.upload(set_ptr, v + 1, s));
  SFM_TRY(w.pairs.alloc(4 * (size_t)M, s)); SFM_TRY(w.T.alloc(18 * v, s));
  SFM_TRY(w.hyp_F.alloc(nh * 9, s)); SFM_TRY(w.hyp_ok.alloc(nh, s)); SFM_TRY(w.counts.alloc(nh, s));
  SFM_TRY(w.win_count.alloc(v, s));
  SFM_TRY(w.stand_in.fill(a, v, true, s));
  a.ptr = w.ptr.p; a.hyp_off = w.plan.hyp_off.p; a.blocks = w.plan.blocks.p;
  a.pairs = w.pairs.p; a.T = w.T.p; a.hyp_F = w.hyp_F.p; a.hyp_ok = w.hyp_ok.p; a.counts = w.counts.p; a.win_count = w.win_count.p;
  if (nh) {
    SFM_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * nh, s));
    twoview_norm_kernel<<<n_sets, kTvThreads, 0, s>>>(a);
    twoview_hyp_kernel<<<(unsigned)nh, 64, 0, s>>>(a, (int)nh);
    twoview_score_kernel<<<w.plan.n_blocks, kTvThreads, 0, s>>>(a);
  }
  twoview_pick_kernel<<<n_sets, 64, 0, s>>>(a);
  twoview_refit_kernel<<<n_sets, kTvThreads, 0, s>>>(a);
  twoview_judge_kernel<<<n_sets, kTvThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_twoview_sample(int n, int max_hyp, int h, int idx[8]) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (n < kTvMinSet || max_hyp < 1 || max_hyp > kHypMax) return 0;
  if (h >= 0 && h < max_hyp && idx != nullptr)
    for (int k = 0; k < 8; ++k) idx[k] = twoview_sample_index(n, h, k);
  return max_hyp;
}

int sfm_twoview_ransac_dev(int n_sets, const int* set_ptr, int64_t M, const double* d_left, const double* d_right, double max_err2,
                           int max_hyp, int iters, double* d_F_out, unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp,
                           int* d_status, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_twoview_ransac_dev";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, iters));
  SFM_TRY(twoview_check_sets(who, n_sets, set_ptr, M));
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_sets == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  if (d_F_out == nullptr || (M > 0 && (d_left == nullptr || d_right == nullptr))) { set_error("%s: null device pointer", who); return SFM_E_SHAPE; }
  TwoviewWork w;
  SFM_TRY(twoview_run(who, n_sets, set_ptr, M, d_left, d_right, max_err2, max_hyp, iters, d_F_out,
                      RobustPtrs{d_obs_inlier, d_n_inliers, d_best_hyp, d_status, d_summary}, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_twoview_ransac(int n_sets, const int* set_ptr, int64_t M, const double* left, const double* right, double max_err2,
                       int max_hyp, int iters, double* F_out, unsigned char* obs_inlier, int* n_inliers, int* best_hyp, int* status,
                       int64_t* summary) {
  const char* who = "sfm_twoview_ransac";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, iters));
  SFM_TRY(twoview_check_sets(who, n_sets, set_ptr, M));
  robust_summary_clear(summary);
  if (n_sets == 0) return SFM_OK;
  if (F_out == nullptr || (M > 0 && (left == nullptr || right == nullptr))) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_sets, m = (size_t)M;
  DevBuf<double> dL, dR;
  HostOut<double> oF;
  RobustOut o;
  TwoviewWork w;
  SFM_TRY(dL.upload(left, 2 * m, s));
  SFM_TRY(dR.upload(right, 2 * m, s));
  SFM_TRY(oF.want(F_out, 9 * v, s));
  SFM_TRY(o.want(m, v, obs_inlier, n_inliers, best_hyp, status, summary, s));
  SFM_TRY(twoview_run(who, n_sets, set_ptr, M, dL.p, dR.p, max_err2, max_hyp, iters, oF.dev(), o.dev(), w, s));
  SFM_TRY(oF.fetch(s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

// processors.verify_pairs (for a HipDeviceKeyTracker): the pairs of table[ref][que] (sfm_track_pairs_dev, into pool buffers) and their robust
// two-view geometry on the same stream.  Rows 0 and 1 of the (3, n) point arrays are the [2][n] coordinates as they are:
// only the count comes down between the two, no coordinate does.
int sfm_twoview_verify_pairs(sfm_track_store* store, int ref, int que, double max_err2, int max_hyp, int iters, int* n, int* r_idx,
                           int* q_idx, unsigned char* inlier, double F_out[9], int* best_hyp, int* status) {
  const char* who = "sfm_twoview_verify_pairs";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, iters));
  if (!n || !F_out) { set_error("%s: n or F_out is NULL", who); return SFM_E_SHAPE; }
  int64_t keys = 0;
  SFM_TRY(sfm_track_info(store, SFM_TRACK_INFO_N_KEYS, ref, &keys));
  const size_t cap = (size_t)(keys > 0 ? keys : 1);
  hipStream_t s = ctx().stream;
  DevBuf<int> dCnt, dR, dQ;
  DevBuf<double> dRef, dQue;
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
  HostOut<double> oF;
  RobustOut o;
  TwoviewWork w;
  SFM_TRY(oF.want(F_out, 9, s));
  SFM_TRY(o.want(m, 1, inlier, nullptr, best_hyp, status, nullptr, s));
  SFM_TRY(twoview_run(who, 1, set_ptr, cnt[0], dRef.p, dQue.p, max_err2, max_hyp, iters, oF.dev(), o.dev(), w, s));
  SFM_TRY(oF.fetch(s));
  SFM_TRY(o.fetch(s));
  if (r_idx) SFM_TRY(dR.download(r_idx, m, s));
  if (q_idx) SFM_TRY(dQ.download(q_idx, m, s));
  return stream_sync(s);
}

}  // extern "C"
