// sfm_homography.hip — robust homography: sampled four-point hypotheses, inlier refit (gfx950).
//
// The fourth robust estimator, next to the point (sfm_tri_ransac.hip), the camera (sfm_resect.hip) and the epipolar
// geometry of a pair of views (sfm_twoview.hip): the model that explains the matches of a plane or of a camera that only
// rotated, where a fundamental matrix is not determined.  The rule is stated in sfm_hip.h, block "robust homography"; a
// model is the pair (H, G) of 18 doubles, H mapping left to right and G right to left.  The stages are those of
// sfm_twoview.hip, for a batch of sets of matches in one call:
//   norm     one workgroup per set: the Hartley transforms over all matches of the set (slice-ordered sums), the normalised
//            matches [M][4], T_l, T_r and their inverses
//   hyp      one wave per (set, hypothesis): the stratified sample of four (sfm_hyp_number.h), the null vector of the 8x9
//            design matrix (sfm_eight_point.h), the rank test, the adjugate, de-normalisation, scaling, the sample gate
//   score    the hot path: a workgroup of 256 owns 1 024 matches of one set, four per lane, in registers; the set's models
//            pass through LDS in batches of 64 hypotheses (9 216 bytes), every lane reads the model under test from the
//            same address (a broadcast), tests its four matches without a branch or a division, a wave adds the popcounts
//            of its four ballots and issues one integer atomicAdd per hypothesis
//   pick     one wave per set: the lexicographic arg-best over (count, h)
//   refit    one workgroup per set, 1 024 matches at a time in every pass: the mask recomputed from the standing model,
//            Hartley transforms over the inliers, the 45 moment sums of their design rows (two per inlier), the 9x9
//            eigenproblem by jacobi_rows_wave<9> on one wave, the count of the result and the acceptance
//   judge    one workgroup per set: obs_inlier, n_inliers and the summary of the model that stands
// One body per kernel serves every set size.  No floating-point value is accumulated with an atomic; the counts are
// integers; every floating-point sum over matches is formed per slice of 64 consecutive matches and the slices are added
// in ascending order: a set's bits depend on its own matches and the options only.
// Shared with the other estimators: the plan, the batch loop of `score`, the tie rule of `pick`, the block reductions,
// the summary and the host frame (sfm_robust.h); the match, the Hartley pass and the scaling (sfm_match_norm.h).
#include <climits>
#include <cmath>

#include "sfm_eight_point.h"   // default contraction, as in sfm_twoview.hip
#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"
#include "sfm_match_norm.h"

namespace sfm {

constexpr int kHgMinSet = 5;          // a set needs one match besides a sample's four
constexpr int kHgMinCount = 5;        // ... and so does a winner
constexpr int kHgBatch = 64;          // hypotheses per LDS batch: 64 x 18 doubles = 9 216 bytes
constexpr int kHgModel = 18;          // H then G

struct HgArgs {
  int n_sets;
  long long M;
  const int* ptr;               // [n_sets + 1]
  const double* left;           // [2][M]
  const double* right;          // [2][M]
  const int* hyp_off;           // [n_sets + 1] first hypothesis of every set (a set below five matches has none)
  const int2* blocks;           // score: workgroup -> (set, first of its 1 024 matches, relative)
  double max_err2;
  int max_hyp, iters;
  double* pairs;                // [M][4] normalised matches
  double* T;                    // [n_sets][4][9] T_l, T_r, T_l^-1, T_r^-1
  double* hyp_HG;               // [hypotheses][18]
  unsigned char* hyp_ok;        // [hypotheses]
  int* counts;                  // [hypotheses]
  int* win_count;               // [n_sets]
  double* HG;                   // [n_sets][18] the standing model
  double* H_out;                // [n_sets][9]
  int* best_hyp;                // [n_sets]
  int* status;                  // [n_sets]
  unsigned char* obs_inlier;    // [M] or null
  int* n_inliers;               // [n_sets] or null
  unsigned long long* summary;  // [6]
};

__device__ __forceinline__ MatchView hg_view(const HgArgs& a) { return {a.left, a.right, a.M}; }

__device__ __forceinline__ bool hg_inlier(const double (&HG)[kHgModel], const TvMatch& m, double max_err2) {
  return homography_inlier(HG, m.xl, m.yl, m.xr, m.yr, max_err2);
}

// T_l, T_r and their inverses [1/s 0 mx; 0 1/s my; 0 0 1] as four row-major 3x3 matrices.
__device__ __forceinline__ void hg_transforms(const TvNorm& t, double (&T)[36]) {
  double tl[9], tr[9];
  tv_transforms(t, tl, tr);
  const double il = 1.0 / t.sl, ir = 1.0 / t.sr;
  const double li[9] = {il, 0, t.ml[0], 0, il, t.ml[1], 0, 0, 1};
  const double ri[9] = {ir, 0, t.mr[0], 0, ir, t.mr[1], 0, 0, 1};
#pragma unroll
  for (int k = 0; k < 9; ++k) { T[k] = tl[k]; T[9 + k] = tr[k]; T[18 + k] = li[k]; T[27 + k] = ri[k]; }
}

// The two design rows of one normalised match p = (x1, y1, x2, y2).
__device__ __forceinline__ void hg_rows(const double* p, double (&ra)[9], double (&rb)[9]) {
  const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
  ra[0] = -x1; ra[1] = -y1; ra[2] = -1.0; ra[3] = 0.0; ra[4] = 0.0; ra[5] = 0.0; ra[6] = x2 * x1; ra[7] = x2 * y1; ra[8] = x2;
  rb[0] = 0.0; rb[1] = 0.0; rb[2] = 0.0; rb[3] = -x1; rb[4] = -y1; rb[5] = -1.0; rb[6] = y2 * x1; rb[7] = y2 * y1; rb[8] = y2;
}

// g = a f b, scaled by canon9; false if the result is not finite or zero.
__device__ __forceinline__ bool hg_denorm_canon(const double* a, const double (&f)[9], const double* b, double* out) {
  double m[9], g[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) m[3 * r + c] = __builtin_fma(a[3 * r + 2], f[6 + c], __builtin_fma(a[3 * r + 1], f[3 + c], a[3 * r] * f[c]));
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) g[3 * r + c] = __builtin_fma(m[3 * r + 2], b[6 + c], __builtin_fma(m[3 * r + 1], b[3 + c], m[3 * r] * b[c]));
  const bool ok = canon9(g);
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = g[k];
  return ok;
}

// One lane: the model (H, G) of the normalised 3x3 matrix h under the transforms T = (T_l, T_r, T_l^-1, T_r^-1): valid iff h
// has full rank (sigma_2 > 3 eps sigma_0) and both matrices are finite.  G comes from the adjugate: no determinant divides.
__device__ __forceinline__ bool hg_model(const double (&h)[9], const double* T, double (&HG)[kHgModel]) {
  double B[3][3], V3[3][3], sig[3];
  int ord[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i][j] = h[3 * i + j];
  svd3(B, V3, sig, ord);
  bool ok = sig[ord[2]] > sig[ord[0]] * 3.0 * 2.220446049250313e-16;            // false for a NaN too
  const double adj[9] = {__builtin_fma(h[4], h[8], -(h[5] * h[7])), __builtin_fma(h[2], h[7], -(h[1] * h[8])), __builtin_fma(h[1], h[5], -(h[2] * h[4])),
                         __builtin_fma(h[5], h[6], -(h[3] * h[8])), __builtin_fma(h[0], h[8], -(h[2] * h[6])), __builtin_fma(h[2], h[3], -(h[0] * h[5])),
                         __builtin_fma(h[3], h[7], -(h[4] * h[6])), __builtin_fma(h[1], h[6], -(h[0] * h[7])), __builtin_fma(h[0], h[4], -(h[1] * h[3]))};
  ok = hg_denorm_canon(T + 27, h, T, HG) && ok;                                  // H = T_r^-1 h T_l
  ok = hg_denorm_canon(T + 18, adj, T + 9, HG + 9) && ok;                        // G = T_l^-1 adj(h) T_r
  return ok;
}

// ---------------------------------------------------------------------------------------------
// norm
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void homography_norm_kernel(HgArgs a) {
  __shared__ double red[kMatchRows][kMatchMoments];
  __shared__ double sums[kMatchMoments];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  if (n < kHgMinSet) return;
  int count;
  const TvNorm t = tv_hartley(hg_view(a), base, n, [](const TvMatch&) { return true; }, tid, red, sums, &count);
  for (int i = tid; i < n; i += kMatchThreads) {
    double p[4];
    tv_normalise(t, match_load(hg_view(a), (long long)base + i), p);
    double* out = a.pairs + 4 * ((size_t)base + i);
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = p[3];
  }
  if (tid == 0) {
    double T[36];
    hg_transforms(t, T);
    // a transform that is not finite (a NaN coordinate, identical points) leaves NaN here: every hypothesis is invalid
    double probe = 0.0;
#pragma unroll
    for (int k = 0; k < 36; ++k) probe += T[k] * 0.0;
    const double poison = (tv_norm_finite(t) && probe == 0.0) ? 0.0 : __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 36; ++k) a.T[36 * (size_t)s + k] = T[k] + poison;
  }
}

// ---------------------------------------------------------------------------------------------
// hyp: the model of a sample
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void homography_hyp_kernel(HgArgs a, int n_hyp) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= n_hyp) return;
  const int s = hyp_owner(a.hyp_off, a.n_sets, g), h = g - a.hyp_off[s];
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int idx = homography_sample_index(n, h, (lane >> 1) & 3);    // lanes 2k, 2k + 1: the two rows of match k
  double row[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) row[c] = 0.0;
  if (lane < 8) {
    double ra[9], rb[9];
    hg_rows(a.pairs + 4 * ((size_t)base + idx), ra, rb);
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = (lane & 1) ? rb[c] : ra[c];
  } else if (lane >= 16 && lane < 25) {
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = (c == lane - 16) ? 1.0 : 0.0;
  }
  double f[9], HG[kHgModel];
  eight_point_null_vector(row, lane, f);
#pragma unroll
  for (int k = 0; k < kHgModel; ++k) HG[k] = 0.0;
  int ok = 0;
  if (lane == 0) {
    double T[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) T[k] = a.T[36 * (size_t)s + k];
    ok = hg_model(f, T, HG);
  }
#pragma unroll
  for (int k = 0; k < kHgModel; ++k) HG[k] = wave_lane0(HG[k]);
  // the sample gate: the four matches of the sample, one per even lane below eight
  const bool in = hg_inlier(HG, match_load(hg_view(a), (long long)base + idx), a.max_err2);
  const unsigned long long gate = __ballot(in) & 0x55ULL;
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < kHgModel; ++k) a.hyp_HG[kHgModel * (size_t)g + k] = HG[k];
  a.hyp_ok[g] = (ok && gate == 0x55ULL) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void homography_score_kernel(HgArgs a) {
  __shared__ double Hm[kHgBatch * kHgModel];
  __shared__ unsigned char okb[kHgBatch];
  const int tid = threadIdx.x;
  const int2 blk = a.blocks[blockIdx.x];
  const int s = blk.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  // four matches per lane, a wave's loads contiguous; a slot beyond the set holds NaN and is nobody's inlier
  TvMatch m[kMatchPerLane];
#pragma unroll
  for (int k = 0; k < kMatchPerLane; ++k) {
    const int i = blk.y + k * kMatchThreads + tid;
    m[k] = match_load(hg_view(a), (long long)base + (i < n ? i : n - 1));
    if (!(i < n)) m[k].xl = __builtin_nan("");
  }
  robust_score_block<kMatchThreads, kHgBatch, kHgModel, 1, kMatchPerLane>(
      a.hyp_HG, a.hyp_ok, a.counts, h0, H, Hm, okb,
      [&](const double* HG, int k) { return homography_inlier(HG, m[k].xl, m[k].yl, m[k].xr, m[k].yr, a.max_err2); });
}

// ---------------------------------------------------------------------------------------------
// pick: the winner of every set
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void homography_pick_kernel(HgArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  int best_cnt, best_h;                                    // the first of the largest counts wins
  wave_arg_best(lane, H, [&](int h) { return a.hyp_ok[h0 + h] != 0; }, [&](int h) { return a.counts[h0 + h]; }, best_cnt, best_h);
  if (lane != 0) return;
  const bool won = best_cnt >= kHgMinCount;
  a.best_hyp[s] = won ? best_h : -1;
  a.win_count[s] = won ? best_cnt : 0;
#pragma unroll
  for (int k = 0; k < kHgModel; ++k) a.HG[kHgModel * (size_t)s + k] = won ? a.hyp_HG[kHgModel * (size_t)(h0 + best_h) + k] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// refit and acceptance
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int hg_count(const HgArgs& a, int base, int n, const double (&HG)[kHgModel], int tid) {
  int total = 0;
  for (int blk = 0; blk < n; blk += kMatchBlockObs) {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kMatchPerLane; ++k) {
      const int i = blk + k * kMatchThreads + tid;
      if (i < n) mine += hg_inlier(HG, match_load(hg_view(a), (long long)base + i), a.max_err2);
    }
    total += block_count(mine);
  }
  return total;
}

__global__ __launch_bounds__(kMatchThreads) void homography_refit_kernel(HgArgs a) {
  __shared__ double red[kMatchRows][kMatchMoments];
  __shared__ double sums[kMatchMoments];
  __shared__ double cand[kHgModel];
  __shared__ int cand_ok;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int bh = a.best_hyp[s];
  int flags = n < kHgMinSet ? SFM_HOMOGRAPHY_TOO_FEW : (bh < 0 ? SFM_HOMOGRAPHY_NO_MODEL : 0);
  double HG[kHgModel];
#pragma unroll
  for (int k = 0; k < kHgModel; ++k) HG[k] = a.HG[kHgModel * (size_t)s + k];
  if (flags == 0) {
    int standing = a.win_count[s], stood = 0;
    const int n_blocks = (n + kMatchBlockObs - 1) / kMatchBlockObs;
    // from here on every thread holds the same values: the branches are uniform
    for (int it = 0; it < a.iters; ++it) {
      int m;
      const TvNorm t = tv_hartley(hg_view(a), base, n, [&](const TvMatch& mt) { return hg_inlier(HG, mt, a.max_err2); }, tid, red, sums, &m);
      if (!tv_norm_finite(t)) break;
      double run = 0;
      for (int blk = 0; blk < n_blocks; ++blk) {
        double acc[kMatchMoments];
#pragma unroll
        for (int k = 0; k < kMatchMoments; ++k) acc[k] = 0;
#pragma unroll
        for (int k = 0; k < kMatchPerLane; ++k) {
          const int i = blk * kMatchBlockObs + kMatchPerLane * tid + k;
          if (i < n) {
            const TvMatch mt = match_load(hg_view(a), (long long)base + i);
            const bool in = hg_inlier(HG, mt, a.max_err2);
            double p[4], ra[9], rb[9];
            tv_normalise(t, mt, p);
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = in ? p[c] : 0.0;
            hg_rows(p, ra, rb);
            ra[2] = in ? -1.0 : 0.0;
            rb[5] = in ? -1.0 : 0.0;
            int q = 0;
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
              for (int c = r; c < 9; ++c, ++q) {                 // the zeros of the two rows are known: their products are left out
                if ((r < 3 || r >= 6) && (c < 3 || c >= 6)) acc[q] = __builtin_fma(ra[r], ra[c], acc[q]);
                if (r >= 3 && c >= 3) acc[q] = __builtin_fma(rb[r], rb[c], acc[q]);
              }
          }
        }
        tv_block_sums<kMatchMoments>(acc, tid, red, sums, run, blk == 0, blk == n_blocks - 1);
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
          double T[36], g[kHgModel];
          hg_transforms(t, T);
          const bool ok = hg_model(f, T, g);
#pragma unroll
          for (int k = 0; k < kHgModel; ++k) cand[k] = g[k];
          cand_ok = ok ? 1 : 0;
        }
      }
      __syncthreads();
      double G[kHgModel];
#pragma unroll
      for (int k = 0; k < kHgModel; ++k) G[k] = cand[k];
      const bool ok = cand_ok != 0;
      const int rc = hg_count(a, base, n, G, tid);         // its barriers also close the reads of cand
      if (!(ok && rc >= standing)) break;
#pragma unroll
      for (int k = 0; k < kHgModel; ++k) HG[k] = G[k];
      standing = rc;
      ++stood;
    }
    if (a.iters > 0 && stood == 0) flags |= SFM_HOMOGRAPHY_KEPT_HYPOTHESIS;
  }
  if (tid == 0) {
    const bool solved = !(flags & (SFM_HOMOGRAPHY_TOO_FEW | SFM_HOMOGRAPHY_NO_MODEL));
#pragma unroll
    for (int k = 0; k < kHgModel; ++k) a.HG[kHgModel * (size_t)s + k] = solved ? HG[k] : 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) a.H_out[9 * (size_t)s + k] = solved ? HG[k] : 0.0;
    a.status[s] = flags;
  }
}

// ---------------------------------------------------------------------------------------------
// judge: what the model that stands makes of the matches
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void homography_judge_kernel(HgArgs a) {
  __shared__ int total;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int flags = a.status[s];
  const bool solved = !(flags & (SFM_HOMOGRAPHY_TOO_FEW | SFM_HOMOGRAPHY_NO_MODEL));
  double HG[kHgModel];
#pragma unroll
  for (int k = 0; k < kHgModel; ++k) HG[k] = a.HG[kHgModel * (size_t)s + k];
  int nin = 0;
  for (int i = tid; i < n; i += kMatchThreads) {
    const bool in = solved & hg_inlier(HG, match_load(hg_view(a), (long long)base + i), a.max_err2);
    if (a.obs_inlier) a.obs_inlier[(size_t)base + i] = in ? 1 : 0;
    nin += in;
  }
  nin = block_sum_int(nin, &total);
  if (tid != 0) return;
  if (a.n_inliers) a.n_inliers[s] = nin;
  robust_summary_add(a.summary, solved, false, flags & SFM_HOMOGRAPHY_TOO_FEW, flags & SFM_HOMOGRAPHY_KEPT_HYPOTHESIS, n, nin);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// What a call keeps on the device besides the caller's arrays.
struct HomographyWork {
  HypPlan plan;
  RobustStandIns stand_in;
  DevBuf<int> ptr, counts, win_count;
  DevBuf<double> pairs, T, hyp_HG, HG;
  DevBuf<unsigned char> hyp_ok;
};

// The one body of sfm_homography_ransac and sfm_homography_ransac_dev: checked arguments and device pointers in
// (n_sets > 0), the kernels enqueued on s out.  w lives until the caller has waited for s.
static int homography_run(const char* who, int n_sets, const int* set_ptr, long long M, const double* d_left, const double* d_right,
                          double max_err2, int max_hyp, int iters, double* d_H_out, const RobustPtrs& out, HomographyWork& w,
                          hipStream_t s) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  SFM_TRY(w.plan.build(who, n_sets, set_ptr, kMatchBlockObs, INT_MAX / 32, [&](int, int n, long long& hyps) {
    hyps = max_hyp;
    return n >= kHgMinSet;
  }, s));
  const size_t v = (size_t)n_sets, nh = w.plan.n_hyp;
  HgArgs a = {};
  a.n_sets = n_sets; a.M = M; a.left = d_left; a.right = d_right;
  a.max_err2 = max_err2; a.max_hyp = max_hyp; a.iters = iters; a.H_out = d_H_out;
  out.into(a);
  SFM_TRY(w.ptr.upload(set_ptr, v + 1, s));
  SFM_TRY(w.pairs.alloc(4 * (size_t)M, s)); SFM_TRY(w.T.alloc(36 * v, s));
  SFM_TRY(w.hyp_HG.alloc(nh * kHgModel, s)); SFM_TRY(w.hyp_ok.alloc(nh, s)); SFM_TRY(w.counts.alloc(nh, s));
  SFM_TRY(w.win_count.alloc(v, s)); SFM_TRY(w.HG.alloc(kHgModel * v, s));
  SFM_TRY(w.stand_in.fill(a, v, true, s));
  a.ptr = w.ptr.p; a.hyp_off = w.plan.hyp_off.p; a.blocks = w.plan.blocks.p;
  a.pairs = w.pairs.p; a.T = w.T.p; a.hyp_HG = w.hyp_HG.p; a.hyp_ok = w.hyp_ok.p; a.counts = w.counts.p; a.win_count = w.win_count.p;
  a.HG = w.HG.p;
  if (nh) {
    SFM_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * nh, s));
    homography_norm_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
    homography_hyp_kernel<<<(unsigned)nh, 64, 0, s>>>(a, (int)nh);
    homography_score_kernel<<<w.plan.n_blocks, kMatchThreads, 0, s>>>(a);
  }
  homography_pick_kernel<<<n_sets, 64, 0, s>>>(a);
  homography_refit_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  homography_judge_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_homography_sample(int n, int max_hyp, int h, int idx[4]) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (n < kHgMinSet || max_hyp < 1 || max_hyp > kHypMax) return 0;
  if (h >= 0 && h < max_hyp && idx != nullptr)
    for (int k = 0; k < 4; ++k) idx[k] = homography_sample_index(n, h, k);
  return max_hyp;
}

int sfm_homography_ransac_dev(int n_sets, const int* set_ptr, int64_t M, const double* d_left, const double* d_right, double max_err2,
                              int max_hyp, int iters, double* d_H_out, unsigned char* d_obs_inlier, int* d_n_inliers,
                              int* d_best_hyp, int* d_status, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_homography_ransac_dev";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, iters));
  SFM_TRY(robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true));
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_sets == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  if (d_H_out == nullptr || (M > 0 && (d_left == nullptr || d_right == nullptr))) { set_error("%s: null device pointer", who); return SFM_E_SHAPE; }
  HomographyWork w;
  SFM_TRY(homography_run(who, n_sets, set_ptr, M, d_left, d_right, max_err2, max_hyp, iters, d_H_out,
                         RobustPtrs{d_obs_inlier, d_n_inliers, d_best_hyp, d_status, d_summary}, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_homography_ransac(int n_sets, const int* set_ptr, int64_t M, const double* left, const double* right, double max_err2,
                          int max_hyp, int iters, double* H_out, unsigned char* obs_inlier, int* n_inliers, int* best_hyp,
                          int* status, int64_t* summary) {
  const char* who = "sfm_homography_ransac";
  SFM_TRY(ensure_init());
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, iters));
  SFM_TRY(robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true));
  robust_summary_clear(summary);
  if (n_sets == 0) return SFM_OK;
  if (H_out == nullptr || (M > 0 && (left == nullptr || right == nullptr))) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_sets, m = (size_t)M;
  DevBuf<double> dL, dR;
  HostOut<double> oH;
  RobustOut o;
  HomographyWork w;
  SFM_TRY(dL.upload(left, 2 * m, s));
  SFM_TRY(dR.upload(right, 2 * m, s));
  SFM_TRY(oH.want(H_out, 9 * v, s));
  SFM_TRY(o.want(m, v, obs_inlier, n_inliers, best_hyp, status, summary, s));
  SFM_TRY(homography_run(who, n_sets, set_ptr, M, dL.p, dR.p, max_err2, max_hyp, iters, oH.dev(), o.dev(), w, s));
  SFM_TRY(oH.fetch(s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
