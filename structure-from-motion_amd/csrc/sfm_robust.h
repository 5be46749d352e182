// sfm_robust.h -- what the robust operations share besides the numbering of their hypotheses (sfm_hyp_number.h): the six
// summary counters and the host frame of the entry points (sfm_tri_ransac.hip, sfm_resect.hip, sfm_twoview.hip), and for
// the two estimators that score every hypothesis of a group (a camera, a set of matches) against all its observations:
// the plan of the hypotheses, the batch loop of the score kernels, the tie rule of the pick, the block reductions of the
// refit and judge kernels.  Everything here is integer arithmetic or floating-point addition only, no multiply is
// followed by an add: the results do not depend on how the including file contracts.  Include it after sfm_obs_test.h.
#pragma once

#include <algorithm>
#include <climits>
#include <vector>

#include "sfm_hyp_number.h"

namespace sfm {

// ---- the summary: 0 solved | 1 no model | 2 too few | 3 kept the hypothesis | 4 inliers | 5 outliers of the solved ----
// One point, camera or set of n observations, nin of them inliers of what stands (too_few, kept_hyp: its status bits).
// A held camera (resection only) adds its inliers to slot 4 and is counted in none of the slots 0 .. 3.
__device__ __forceinline__ void robust_summary_add(unsigned long long* summary, bool solved, bool held, int too_few, int kept_hyp,
                                                   int n, int nin) {
  if (solved) {
    atomicAdd(&summary[0], 1ULL);
    if (kept_hyp) atomicAdd(&summary[3], 1ULL);
    if (nin) atomicAdd(&summary[4], (unsigned long long)nin);
    if (n - nin) atomicAdd(&summary[5], (unsigned long long)(n - nin));
  } else if (held) {
    if (nin) atomicAdd(&summary[4], (unsigned long long)nin);
  } else {
    atomicAdd(&summary[1 + (too_few != 0)], 1ULL);
  }
}

// ---- device: hypotheses planned per group, hyp_off[n_groups + 1] their first numbers (HypPlan below) ----
// The group whose hypotheses hold g: hyp_off[lo] <= g < hyp_off[lo + 1].  A group without hypotheses is never returned.
__device__ __forceinline__ int hyp_owner(const int* hyp_off, int n_groups, int g) {
  int lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (hyp_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// The batch loop of a score kernel: a workgroup of THREADS holds PER observations per lane in registers and walks the H
// hypotheses of its group from h0 on.  A hypothesis is STRIDE doubles at hyp and CANDS candidate models of STRIDE / CANDS
// doubles each, bit r of ok[] saying whether candidate r is valid.  The hypotheses pass through lds[BATCH * STRIDE] in
// batches of BATCH (okb[BATCH] their valid bits, read uniformly); test(model, k) is the lane's observation k against the
// model, which every lane reads from the same LDS address (a broadcast), and must be false for a slot beyond the group.
// A wave adds the popcounts of its PER ballots and issues one integer atomicAdd per candidate: counts[][CANDS].  Ok is the
// word that holds the valid bits of a hypothesis: a byte up to eight candidates, wider for the ten of the five-point solver.
template <int THREADS, int BATCH, int STRIDE, int CANDS, int PER, class Test, class Ok>
__device__ __forceinline__ void robust_score_block(const double* hyp, const Ok* ok, int* counts, int h0, int H,
                                                   double* lds, Ok* okb, Test test) {
  static_assert(CANDS <= 8 * (int)sizeof(Ok), "a valid bit per candidate");
  const int tid = threadIdx.x;
  for (int hb = 0; hb < H; hb += BATCH) {
    const int nb = min(BATCH, H - hb);
    const double* src = hyp + (size_t)(h0 + hb) * STRIDE;
    for (int i = tid; i < nb * STRIDE; i += THREADS) lds[i] = src[i];
    if (tid < nb) okb[tid] = ok[h0 + hb + tid];
    __syncthreads();
    for (int hh = 0; hh < nb; ++hh) {
      const int bits = okb[hh];                            // the same for the whole workgroup: the branches are uniform
#pragma unroll
      for (int r = 0; r < CANDS; ++r) {
        if (!(bits >> r & 1)) continue;
        const double* m = lds + (hh * CANDS + r) * (STRIDE / CANDS);
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) cnt += __popcll(__ballot(test(m, k)));
        if ((tid & 63) == 0 && cnt) atomicAdd(&counts[(size_t)(h0 + hb + hh) * CANDS + r], cnt);
      }
    }
    __syncthreads();                                       // the batch has been read: the next one may be staged
  }
}

// The tie rule of the pick, one wave: among the candidates 0 .. n - 1 with valid(i), the largest count(i), and among equal
// counts the lowest i (each lane scans ascending, so only a larger count replaces what it holds).  Every lane returns
// the winner; -1 / INT_MAX without a valid candidate.
template <class Valid, class Count>
__device__ __forceinline__ void wave_arg_best(int lane, int n, Valid valid, Count count, int& best_cnt, int& best_i) {
  best_cnt = -1; best_i = INT_MAX;
  for (int i = lane; i < n; i += 64) {
    if (!valid(i)) continue;
    const int cnt = count(i);
    if (cnt > best_cnt) { best_cnt = cnt; best_i = i; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int oc = __shfl_xor(best_cnt, off, 64), oi = __shfl_xor(best_i, off, 64);
    if (oc > best_cnt || (oc == best_cnt && oi < best_i)) { best_cnt = oc; best_i = oi; }
  }
}

// The workgroup's sum of a per-thread count of 0 .. 4 (four observations per lane), on every thread.  Three barriers.
__device__ __forceinline__ int block_count(int mine) {
  return __syncthreads_count(mine & 1) + 2 * __syncthreads_count(mine & 2) + 4 * __syncthreads_count(mine & 4);
}

// The workgroup's sum of any per-thread integer through one LDS word, on every thread.  Two barriers.  The call returns
// without a barrier after the total is read, and the next call on the same word starts by zeroing it: two calls may not use
// the same word without a __syncthreads() between them.  Several sums at once: block_sums below.
__device__ __forceinline__ int block_sum_int(int v, int* lds_total) {
  if (threadIdx.x == 0) *lds_total = 0;
  __syncthreads();
  v = group_sum<64>(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(lds_total, v);
  __syncthreads();
  return *lds_total;
}

// K such sums through the K words of lds, v[k] replaced by its total on every thread.  Two barriers for all of them; the
// same rule holds for the words.
template <int K>
__device__ __forceinline__ void block_sums(int (&v)[K], int* lds) {
  if (threadIdx.x < K) lds[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = group_sum<64>(v[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&lds[k], s);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = lds[k];
}

// One pass of a slice-ordered floating-point sum: red[ROWS][] holds the K sums of the pass's slices, written by their
// owners before the call; thread k < K adds red[0 .. ROWS - 1][k] in that order onto its running total `run` (the `first`
// pass starts it) and with `last` leaves the total in sums[k].  Slices beyond the group hold zeros.  A barrier before the
// rows are read and one after: sums complete, red free for the next pass.
template <int K, int ROWS, int W>
__device__ __forceinline__ void slice_totals(const double (*red)[W], double* sums, double& run, bool first, bool last, int tid) {
  __syncthreads();
  if (tid < K) {
    double t = first ? red[0][tid] : run + red[0][tid];
#pragma unroll
    for (int w = 1; w < ROWS; ++w) t += red[w][tid];
    run = t;
    if (last) sums[tid] = t;
  }
  __syncthreads();
}

// ---- the host frame ----
inline int robust_check_args(const char* who, double max_err2, int max_hyp, double lambda, int iters) {
  if (!(max_err2 >= 0.0)) { set_error("%s: max_err2 = %g must be >= 0", who, max_err2); return SFM_E_SHAPE; }
  if (max_hyp < 0 || max_hyp > kHypMax) { set_error("%s: max_hyp = %d must be in 1 .. %d (0 = %d)", who, max_hyp, kHypMax, kHypDefault); return SFM_E_SHAPE; }
  if (iters < 0) { set_error("%s: iters = %d must be >= 0", who, iters); return SFM_E_SHAPE; }
  if (!(lambda >= 0.0)) { set_error("%s: lambda = %g must be >= 0", who, lambda); return SFM_E_SHAPE; }
  return SFM_OK;
}

// The offsets of the groups of a call on the host: name[n + 1] ("view_ptr" of n "view"s) starts at 0, never decreases and
// ends at M.  A call without groups needs no offsets unless `even_empty`.
inline int robust_check_offsets(const char* who, const char* noun, const char* name, int n, const int* ptr, long long M, bool even_empty) {
  if (n < 0 || M < 0 || M > INT_MAX) { set_error("%s: bad sizes n_%ss=%d M=%lld", who, noun, n, M); return SFM_E_SHAPE; }
  if (n == 0 && !even_empty) return SFM_OK;
  if (ptr == nullptr) { set_error("%s: null %s", who, name); return SFM_E_SHAPE; }
  if (ptr[0] != 0 || ptr[n] != M) {
    set_error("%s: %s must start at 0 and end at M = %lld (it runs from %d to %d)", who, name, M, ptr[0], ptr[n]);
    return SFM_E_SHAPE;
  }
  for (int c = 0; c < n; ++c)
    if (ptr[c + 1] < ptr[c]) { set_error("%s: %s decreases at %s %d", who, name, noun, c); return SFM_E_SHAPE; }
  return SFM_OK;
}

inline void robust_summary_clear(int64_t* summary) { if (summary) std::fill(summary, summary + 6, (int64_t)0); }

// The five optional outputs as device pointers, any of them null: [M], [n] per point, camera or set, [6].  `into` hands
// them to the kernel arguments of an operation (the members carry these names there); the counters stay below 2^63, so
// the kernels' unsigned words are the caller's int64_t as they are.
struct RobustPtrs {
  unsigned char* obs_inlier;
  int *n_inliers, *best_hyp, *status;
  int64_t* summary;
  template <class Args>
  void into(Args& a) const {
    a.obs_inlier = obs_inlier; a.n_inliers = n_inliers; a.best_hyp = best_hyp; a.status = status;
    a.summary = reinterpret_cast<unsigned long long*>(summary);
  }
};

// ... and as a host-pointer entry point keeps them: device buffers for those the caller asked for, and their download.
struct RobustOut {
  HostOut<unsigned char> inlier;
  HostOut<int> count, best, status;
  HostOut<int64_t> summary;
  int want(size_t m, size_t n, unsigned char* obs_inlier, int* n_inliers, int* best_hyp, int* st, int64_t* sum, hipStream_t s) {
    SFM_TRY(inlier.want(obs_inlier, m, s)); SFM_TRY(count.want(n_inliers, n, s)); SFM_TRY(best.want(best_hyp, n, s));
    SFM_TRY(status.want(st, n, s)); return summary.want(sum, 6, s);
  }
  RobustPtrs dev() const { return {inlier.dev(), count.dev(), best.dev(), status.dev(), summary.dev()}; }
  int fetch(hipStream_t s) const {
    SFM_TRY(inlier.fetch(s)); SFM_TRY(count.fetch(s)); SFM_TRY(best.fetch(s)); SFM_TRY(status.fetch(s)); return summary.fetch(s);
  }
};

// The outputs the kernels pass on to each other whether or not the caller asked for them: a work buffer stands in for a
// null a.best_hyp / a.summary (and a.status, where the kernels need it) of n groups; the summary is cleared on s.
struct RobustStandIns {
  DevBuf<int> best_hyp, status;
  DevBuf<unsigned long long> summary;
  template <class Args>
  int fill(Args& a, size_t n, bool need_status, hipStream_t s) {
    if (!a.best_hyp) { SFM_TRY(best_hyp.alloc(n, s)); a.best_hyp = best_hyp.p; }
    if (need_status && !a.status) { SFM_TRY(status.alloc(n, s)); a.status = status.p; }
    if (!a.summary) { SFM_TRY(summary.alloc(6, s)); a.summary = summary.p; }
    SFM_HIP(hipMemsetAsync(a.summary, 0, 6 * sizeof(unsigned long long), s));
    return SFM_OK;
  }
};

// The hypotheses of a call, planned on the host: group c (a camera, a set) of n observations takes part iff
// group(c, n, hyps) says so and then has `hyps` hypotheses, numbered from hyp_off[c] on, and one score workgroup per
// block_obs of its observations, blocks[] = (group, first observation, relative).  At most `limit` hypotheses fit the
// workspace.  Both tables are uploaded on s.
struct HypPlan {
  DevBuf<int> hyp_off;
  DevBuf<int2> blocks;
  size_t n_hyp = 0;
  unsigned n_blocks = 0;
  template <class Group>
  int build(const char* who, int n_groups, const int* ptr, int block_obs, long long limit, Group group, hipStream_t s) {
    std::vector<int> off((size_t)n_groups + 1, 0);
    std::vector<int2> blk;
    long long total = 0;
    for (int c = 0; c < n_groups; ++c) {
      const int n = ptr[c + 1] - ptr[c];
      long long hyps = 0;
      off[c] = (int)total;
      if (group(c, n, hyps)) {
        total += hyps;
        for (int b = 0; b < n; b += block_obs) blk.push_back(make_int2(c, b));
      }
      if (total > limit) { set_error("%s: %lld hypotheses are beyond the workspace", who, total); return SFM_E_SHAPE; }
    }
    off[n_groups] = (int)total;
    n_hyp = (size_t)total; n_blocks = (unsigned)blk.size();
    SFM_TRY(hyp_off.upload(off.data(), off.size(), s));
    return blocks.upload(blk.data(), blk.size(), s);
  }
};

}  // namespace sfm
