// sfm_match_norm.h -- what the robust estimators over sets of matches between two views share (sfm_twoview.hip: the
// fundamental matrix; sfm_homography.hip: the homography): a match and its load, the Hartley transforms of a set or of
// the inliers of a standing model, formed by slice-ordered sums (a workgroup of 256 takes 1 024 matches per pass, four
// consecutive ones per lane, 16 adjacent lanes one slice of 64), and the scaling of a 3x3 matrix to Frobenius norm 1.
//
// Compiled WITHOUT automatic contraction, the FMAs spelled out: include it after sfm_obs_test.h and sfm_robust.h.
#pragma once

#include "sfm_obs_test.h"
#include "sfm_robust.h"

namespace sfm {

constexpr int kMatchThreads = 256;
constexpr int kMatchPerLane = 4;
constexpr int kMatchBlockObs = kMatchThreads * kMatchPerLane;   // 1 024 matches per workgroup and pass
constexpr int kMatchRows = kMatchThreads / 16;                  // slices of 64 matches per pass: 16 lanes x 4 matches each
constexpr int kMatchMoments = 45;     // upper triangle of a 9x9 moment matrix: the widest row of sums a pass carries

// The matches of a call: left and right are [2][M], the x row then the y row.
struct MatchView { const double* left; const double* right; long long M; };

struct TvMatch { double xl, yl, xr, yr; };

__device__ __forceinline__ TvMatch match_load(const MatchView& v, long long i) {
  return {v.left[i], v.left[v.M + i], v.right[i], v.right[v.M + i]};
}

// A Hartley transform as (mean x, mean y, scale): x^ = scale x + (-(mean x) scale).
struct TvNorm { double ml[2], mr[2], sl, sr; };

__device__ __forceinline__ void tv_normalise(const TvNorm& t, const TvMatch& m, double (&p)[4]) {
  p[0] = __builtin_fma(t.sl, m.xl, -(t.ml[0] * t.sl));
  p[1] = __builtin_fma(t.sl, m.yl, -(t.ml[1] * t.sl));
  p[2] = __builtin_fma(t.sr, m.xr, -(t.mr[0] * t.sr));
  p[3] = __builtin_fma(t.sr, m.yr, -(t.mr[1] * t.sr));
}

__device__ __forceinline__ void tv_transforms(const TvNorm& t, double (&tl)[9], double (&tr)[9]) {
  const double l[9] = {t.sl, 0, -(t.ml[0] * t.sl), 0, t.sl, -(t.ml[1] * t.sl), 0, 0, 1};
  const double r[9] = {t.sr, 0, -(t.mr[0] * t.sr), 0, t.sr, -(t.mr[1] * t.sr), 0, 0, 1};
#pragma unroll
  for (int k = 0; k < 9; ++k) { tl[k] = l[k]; tr[k] = r[k]; }
}

__device__ __forceinline__ bool tv_norm_finite(const TvNorm& t) {
  const double probe = (t.ml[0] + t.ml[1] + t.mr[0] + t.mr[1] + t.sl + t.sr + t.ml[0] * t.sl + t.ml[1] * t.sl + t.mr[0] * t.sr +
                        t.mr[1] * t.sr) * 0.0;
  return probe == 0.0;
}

// The slice sums of one pass of 1 024 matches, added to the running totals in slice order.  acc: the lane's sums over its
// four consecutive matches; 16 adjacent lanes hold a slice of 64 consecutive matches.  Threads 0 .. K-1 carry `run`; with
// `last` they leave the totals in sums[].  Slices beyond the set hold zeros.  Ends with a barrier.
template <int K>
__device__ __forceinline__ void tv_block_sums(double (&acc)[K], int tid, double (*red)[kMatchMoments], double* sums, double& run,
                                              bool first, bool last) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = group_sum<16>(acc[k]);
  if ((tid & 15) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[tid >> 4][k] = acc[k];
  }
  slice_totals<K, kMatchRows>(red, sums, run, first, last, tid);
}

// The Hartley transforms (epipolar_processor.py:97-137: centroid, scale sqrt(2) / mean distance) over the matches base ..
// base + n - 1 that taken(match) accepts (the inliers of a standing model, or all of them).  Every thread of the
// workgroup returns the same values; *count is the number of matches taken.
template <class Taken>
__device__ __forceinline__ TvNorm tv_hartley(const MatchView& v, int base, int n, Taken taken, int tid,
                                             double (*red)[kMatchMoments], double* sums, int* count) {
  const int n_blocks = (n + kMatchBlockObs - 1) / kMatchBlockObs;
  double run = 0;
  int m = 0;
  for (int blk = 0; blk < n_blocks; ++blk) {
    double acc[4] = {0, 0, 0, 0};
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kMatchPerLane; ++k) {
      const int i = blk * kMatchBlockObs + kMatchPerLane * tid + k;
      if (i < n) {
        const TvMatch mt = match_load(v, (long long)base + i);
        const bool in = taken(mt);
        acc[0] += in ? mt.xl : 0.0; acc[1] += in ? mt.yl : 0.0; acc[2] += in ? mt.xr : 0.0; acc[3] += in ? mt.yr : 0.0;
        mine += in;
      }
    }
    m += block_count(mine);
    tv_block_sums<4>(acc, tid, red, sums, run, blk == 0, blk == n_blocks - 1);
  }
  TvNorm t;
  const double dm = (double)m;
  t.ml[0] = sums[0] / dm; t.ml[1] = sums[1] / dm; t.mr[0] = sums[2] / dm; t.mr[1] = sums[3] / dm;
  for (int blk = 0; blk < n_blocks; ++blk) {
    double acc[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < kMatchPerLane; ++k) {
      const int i = blk * kMatchBlockObs + kMatchPerLane * tid + k;
      if (i < n) {
        const TvMatch mt = match_load(v, (long long)base + i);
        const bool in = taken(mt);
        const double ax = mt.xl - t.ml[0], ay = mt.yl - t.ml[1], bx = mt.xr - t.mr[0], by = mt.yr - t.mr[1];
        const double dl = sqrt(__builtin_fma(ax, ax, ay * ay)), dr = sqrt(__builtin_fma(bx, bx, by * by));
        acc[0] += in ? dl : 0.0; acc[1] += in ? dr : 0.0;
      }
    }
    tv_block_sums<2>(acc, tid, red, sums, run, blk == 0, blk == n_blocks - 1);
  }
  t.sl = (1.4142135623730951 * dm) / sums[0];
  t.sr = (1.4142135623730951 * dm) / sums[1];
  __syncthreads();                                         // sums has been read: the next pass may write it
  *count = m;
  return t;
}

// g scaled to Frobenius norm 1 with its entry of largest magnitude (the first of them) positive; false if g is not
// finite or zero.
__device__ __forceinline__ bool canon9(double (&g)[9]) {
  double ss = 0, big = -1.0, sign = 1.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double v = g[k];
    ss = __builtin_fma(v, v, ss);
    const bool larger = fabs(v) > big;
    sign = larger ? (v < 0.0 ? -1.0 : 1.0) : sign;
    big = larger ? fabs(v) : big;
  }
  const double nrm = sign * sqrt(ss);
#pragma unroll
  for (int k = 0; k < 9; ++k) g[k] = g[k] / nrm;
  return ss > 0.0 && isfinite(ss);                        // an overflowing or NaN entry makes ss non-finite
}

}  // namespace sfm
