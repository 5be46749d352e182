// sfm_similarity.hip — robust 3D similarity: sampled three-point hypotheses, inlier refit (gfx950).
//
// The sixth robust estimator, next to the point (sfm_tri_ransac.hip), the camera (sfm_resect.hip) and the three models of
// a pair of views (sfm_twoview.hip, sfm_homography.hip, sfm_essential.hip): the seven-parameter map b ~ s A a + t between
// two 3D frames, from correspondences with wrong ones among them.  The rule is stated in sfm_hip.h, block "robust
// similarity".  A model is kept in two forms: the 13 doubles (s, A row-major, t) the caller receives, and the 12 doubles
// (s A, t) the test reads (similarity_inlier, sfm_obs_test.h); the second is always s * A[i][j] of the first.  The stages,
// for a batch of sets of correspondences in one call:
//   hyp      a lane per (set, hypothesis): the stratified sample of three (sfm_hyp_number.h), its centroids and centred
//            moments, the model of the moments (Umeyama 1991: a 3x3 SVD by one-sided Jacobi), the sample gate
//   score    the hot path: a workgroup of 256 owns 1 024 correspondences of one set, four per lane and six doubles each, in
//            registers; the set's models pass through LDS in batches of 64 hypotheses (6 144 bytes), every lane reads the
//            model under test from the same address (a broadcast), a wave adds the popcounts of its four ballots and
//            issues one integer atomicAdd per hypothesis
//   pick     one wave per set: the lexicographic arg-best over (count, h)
//   refit    one workgroup per set, 1 024 correspondences at a time in every pass: the 3 + 3 centroid sums over the inliers
//            of the standing model, then the 9 + 1 centred sums, both per slice of 64 in slice order; one lane solves; a
//            count pass and the acceptance
//   judge    one workgroup per set: obs_inlier, n_inliers and the summary of the model that stands
// No floating-point value is accumulated with an atomic; the counts are integers: a set's bits depend on its own
// correspondences and the options only.
// Shared with the other estimators: the plan, the batch loop of `score`, the tie rule of `pick`, the block reductions,
// the summary and the host frame (sfm_robust.h); the slice sums of a pass of 1 024 (sfm_match_norm.h).
#include <climits>
#include <cmath>

#include "sfm_eight_point.h"   // svd3, default contraction
#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"
#include "sfm_match_norm.h"

namespace sfm {

constexpr int kSimMinSet = 4;         // a set needs one correspondence besides a sample's three
constexpr int kSimMinCount = 4;       // ... and so does a winner
constexpr int kSimBatch = 64;         // hypotheses per LDS batch: 64 x 12 doubles = 6 144 bytes
constexpr int kSimTest = 12;          // (s A, t): what the test reads
constexpr int kSimModel = 13;         // (s, A, t): what the caller receives

struct SimArgs {
  int n_sets;
  long long M;
  const int* ptr;               // [n_sets + 1]
  const double* src;            // [3][M]
  const double* dst;            // [3][M]
  const int* hyp_off;           // [n_sets + 1] first hypothesis of every set (a set below four correspondences has none)
  const int2* blocks;           // score: workgroup -> (set, first of its 1 024 correspondences, relative)
  double max_err2;
  int max_hyp, iters, rigid;
  double* hyp_test;             // [hypotheses][12]
  double* hyp_sim;              // [hypotheses][13]
  unsigned char* hyp_ok;        // [hypotheses]
  int* counts;                  // [hypotheses]
  int* win_count;               // [n_sets]
  double* sim_out;              // [n_sets][13] the standing model
  int* best_hyp;                // [n_sets]
  int* status;                  // [n_sets]
  unsigned char* obs_inlier;    // [M] or null
  int* n_inliers;               // [n_sets] or null
  unsigned long long* summary;  // [6]
};

struct SimPair { double ax, ay, az, bx, by, bz; };

__device__ __forceinline__ SimPair sim_load(const SimArgs& a, long long i) {
  return {a.src[i], a.src[a.M + i], a.src[2 * a.M + i], a.dst[i], a.dst[a.M + i], a.dst[2 * a.M + i]};
}

__device__ __forceinline__ bool sim_inlier(const double (&T)[kSimTest], const SimPair& c, double max_err2) {
  return similarity_inlier(T, c.ax, c.ay, c.az, c.bx, c.by, c.bz, max_err2);
}

// The form the test reads of a model (s, A, t): s * A[i][j], one rounding each, then t.
__device__ __forceinline__ void sim_test_form(const double (&sim)[kSimModel], double (&T)[kSimTest]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) T[k] = sim[0] * sim[1 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) T[9 + k] = sim[10 + k];
}

__device__ __forceinline__ double sim_col(const double (&X)[3][3], int i, int c) { return c == 0 ? X[i][0] : (c == 1 ? X[i][1] : X[i][2]); }

// One lane: the model of the moments of m correspondences -- the centroids mu_a, mu_b, Sigma = (1/m) sum (b - mu_b)(a - mu_a)^T
// (row-major, rows by b) and var_a = (1/m) sum |a - mu_a|^2.  With Sigma = U D V^T the rotation is U diag(1, 1, det U det V) V^T:
// u_0, u_1 and v_0, v_1 are the singular vectors of the two largest singular values, and the third pair is completed as
// u_0 x u_1 and v_0 x v_1, which is that product whatever the sign the decomposition gave its own third pair -- and stays
// defined where D_2 = 0 (a sample of three spans a plane).  The scale D_0 + D_1 + det U det V D_2 is the trace of A^T Sigma.
// Valid iff everything is finite, var_a > 0, s > 0 and D_1 > 3 eps D_0.
__device__ inline bool sim_model(const double (&mu_a)[3], const double (&mu_b)[3], const double (&Sg)[9], double var_a, bool rigid,
                                 double (&sim)[kSimModel]) {
  double B[3][3], V[3][3], sig[3];
  int ord[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) B[i][j] = Sg[3 * i + j];
  svd3(B, V, sig, ord);
  const int c0 = ord[0], c1 = ord[1];
  const double d0 = c0 == 0 ? sig[0] : (c0 == 1 ? sig[1] : sig[2]), d1 = c1 == 0 ? sig[0] : (c1 == 1 ? sig[1] : sig[2]);
  double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u0[i] = sim_col(B, i, c0) / d0; u1[i] = sim_col(B, i, c1) / d1;
    v0[i] = sim_col(V, i, c0); v1[i] = sim_col(V, i, c1);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    u2[i] = __builtin_fma(u0[j], u1[k], -(u0[k] * u1[j]));
    v2[i] = __builtin_fma(v0[j], v1[k], -(v0[k] * v1[j]));
  }
  double A[9], tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[3 * i + j] = __builtin_fma(u2[i], v2[j], __builtin_fma(u1[i], v1[j], u0[i] * v0[j]));
      tr = __builtin_fma(A[3 * i + j], Sg[3 * i + j], tr);
    }
  const double s = rigid ? 1.0 : tr / var_a;
  sim[0] = s;
#pragma unroll
  for (int k = 0; k < 9; ++k) sim[1 + k] = A[k];
  double probe = s * 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double r = __builtin_fma(A[3 * i], mu_a[0], __builtin_fma(A[3 * i + 1], mu_a[1], A[3 * i + 2] * mu_a[2]));
    sim[10 + i] = __builtin_fma(-s, r, mu_b[i]);
    probe += sim[10 + i] * 0.0;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) probe += A[k] * 0.0;
  // every comparison is false for a NaN
  return (probe == 0.0) & (var_a > 0.0) & (var_a <= 1.7976931348623157e308) & (s > 0.0) & (d1 > d0 * 3.0 * 2.220446049250313e-16);
}

// ---------------------------------------------------------------------------------------------
// hyp: the model of a sample
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void similarity_hyp_kernel(SimArgs a, int n_hyp) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n_hyp) return;
  const int s = hyp_owner(a.hyp_off, a.n_sets, g), h = g - a.hyp_off[s];
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  SimPair c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = sim_load(a, (long long)base + similarity_sample_index(n, h, k));
  const double mu_a[3] = {((c[0].ax + c[1].ax) + c[2].ax) / 3.0, ((c[0].ay + c[1].ay) + c[2].ay) / 3.0, ((c[0].az + c[1].az) + c[2].az) / 3.0};
  const double mu_b[3] = {((c[0].bx + c[1].bx) + c[2].bx) / 3.0, ((c[0].by + c[1].by) + c[2].by) / 3.0, ((c[0].bz + c[1].bz) + c[2].bz) / 3.0};
  double Sg[9], var_a = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) Sg[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double da[3] = {c[k].ax - mu_a[0], c[k].ay - mu_a[1], c[k].az - mu_a[2]};
    const double db[3] = {c[k].bx - mu_b[0], c[k].by - mu_b[1], c[k].bz - mu_b[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Sg[3 * i + j] = __builtin_fma(db[i], da[j], Sg[3 * i + j]);
      var_a = __builtin_fma(da[i], da[i], var_a);
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) Sg[k] = Sg[k] / 3.0;
  var_a = var_a / 3.0;
  double sim[kSimModel], T[kSimTest];
  bool ok = sim_model(mu_a, mu_b, Sg, var_a, a.rigid != 0, sim);
  sim_test_form(sim, T);
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok & sim_inlier(T, c[k], a.max_err2);      // the sample gate
#pragma unroll
  for (int k = 0; k < kSimModel; ++k) a.hyp_sim[kSimModel * (size_t)g + k] = sim[k];
#pragma unroll
  for (int k = 0; k < kSimTest; ++k) a.hyp_test[kSimTest * (size_t)g + k] = T[k];
  a.hyp_ok[g] = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void similarity_score_kernel(SimArgs a) {
  __shared__ double Tm[kSimBatch * kSimTest];
  __shared__ unsigned char okb[kSimBatch];
  const int tid = threadIdx.x;
  const int2 blk = a.blocks[blockIdx.x];
  const int s = blk.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  // four correspondences per lane, a wave's loads contiguous; a slot beyond the set holds NaN and is nobody's inlier
  SimPair c[kMatchPerLane];
#pragma unroll
  for (int k = 0; k < kMatchPerLane; ++k) {
    const int i = blk.y + k * kMatchThreads + tid;
    c[k] = sim_load(a, (long long)base + (i < n ? i : n - 1));
    if (!(i < n)) c[k].ax = __builtin_nan("");
  }
  robust_score_block<kMatchThreads, kSimBatch, kSimTest, 1, kMatchPerLane>(
      a.hyp_test, a.hyp_ok, a.counts, h0, H, Tm, okb,
      [&](const double* T, int k) { return similarity_inlier(T, c[k].ax, c[k].ay, c[k].az, c[k].bx, c[k].by, c[k].bz, a.max_err2); });
}

// ---------------------------------------------------------------------------------------------
// pick: the winner of every set
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void similarity_pick_kernel(SimArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  int best_cnt, best_h;                                    // the first of the largest counts wins
  wave_arg_best(lane, H, [&](int h) { return a.hyp_ok[h0 + h] != 0; }, [&](int h) { return a.counts[h0 + h]; }, best_cnt, best_h);
  if (lane != 0) return;
  const bool won = best_cnt >= kSimMinCount;
  a.best_hyp[s] = won ? best_h : -1;
  a.win_count[s] = won ? best_cnt : 0;
#pragma unroll
  for (int k = 0; k < kSimModel; ++k) a.sim_out[kSimModel * (size_t)s + k] = won ? a.hyp_sim[kSimModel * (size_t)(h0 + best_h) + k] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// refit and acceptance
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int sim_count(const SimArgs& a, int base, int n, const double (&T)[kSimTest], int tid) {
  int total = 0;
  for (int blk = 0; blk < n; blk += kMatchBlockObs) {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kMatchPerLane; ++k) {
      const int i = blk + k * kMatchThreads + tid;
      if (i < n) mine += sim_inlier(T, sim_load(a, (long long)base + i), a.max_err2);
    }
    total += block_count(mine);
  }
  return total;
}

__global__ __launch_bounds__(kMatchThreads) void similarity_refit_kernel(SimArgs a) {
  __shared__ double red[kMatchRows][kMatchMoments];
  __shared__ double sums[kMatchMoments];
  __shared__ double cand[kSimModel];
  __shared__ int cand_ok;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int bh = a.best_hyp[s];
  int flags = n < kSimMinSet ? SFM_SIMILARITY_TOO_FEW : (bh < 0 ? SFM_SIMILARITY_NO_MODEL : 0);
  double sim[kSimModel], T[kSimTest];
#pragma unroll
  for (int k = 0; k < kSimModel; ++k) sim[k] = a.sim_out[kSimModel * (size_t)s + k];
  sim_test_form(sim, T);
  if (flags == 0) {
    int standing = a.win_count[s], stood = 0;
    const int n_blocks = (n + kMatchBlockObs - 1) / kMatchBlockObs;
    // from here on every thread holds the same values: the branches are uniform
    for (int it = 0; it < a.iters; ++it) {
      double run = 0;
      int m = 0;
      for (int blk = 0; blk < n_blocks; ++blk) {             // first pass: the centroids of the inliers
        double acc[6] = {0, 0, 0, 0, 0, 0};
        int mine = 0;
#pragma unroll
        for (int k = 0; k < kMatchPerLane; ++k) {
          const int i = blk * kMatchBlockObs + kMatchPerLane * tid + k;
          if (i < n) {
            const SimPair c = sim_load(a, (long long)base + i);
            const bool in = sim_inlier(T, c, a.max_err2);
            acc[0] += in ? c.ax : 0.0; acc[1] += in ? c.ay : 0.0; acc[2] += in ? c.az : 0.0;
            acc[3] += in ? c.bx : 0.0; acc[4] += in ? c.by : 0.0; acc[5] += in ? c.bz : 0.0;
            mine += in;
          }
        }
        m += block_count(mine);
        tv_block_sums<6>(acc, tid, red, sums, run, blk == 0, blk == n_blocks - 1);
      }
      const double dm = (double)m;
      const double mu_a[3] = {sums[0] / dm, sums[1] / dm, sums[2] / dm}, mu_b[3] = {sums[3] / dm, sums[4] / dm, sums[5] / dm};
      __syncthreads();                                       // sums has been read: the next pass may write it
      for (int blk = 0; blk < n_blocks; ++blk) {             // second pass: the centred moments
        double acc[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[k] = 0;
#pragma unroll
        for (int k = 0; k < kMatchPerLane; ++k) {
          const int i = blk * kMatchBlockObs + kMatchPerLane * tid + k;
          if (i < n) {
            const SimPair c = sim_load(a, (long long)base + i);
            const bool in = sim_inlier(T, c, a.max_err2);
            const double da[3] = {in ? c.ax - mu_a[0] : 0.0, in ? c.ay - mu_a[1] : 0.0, in ? c.az - mu_a[2] : 0.0};
            const double db[3] = {in ? c.bx - mu_b[0] : 0.0, in ? c.by - mu_b[1] : 0.0, in ? c.bz - mu_b[2] : 0.0};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
              for (int q = 0; q < 3; ++q) acc[3 * r + q] = __builtin_fma(db[r], da[q], acc[3 * r + q]);
              acc[9] = __builtin_fma(da[r], da[r], acc[9]);
            }
          }
        }
        tv_block_sums<10>(acc, tid, red, sums, run, blk == 0, blk == n_blocks - 1);
      }
      if (tid == 0) {                                        // one lane: the 3x3 solve
        double Sg[9], g[kSimModel];
#pragma unroll
        for (int k = 0; k < 9; ++k) Sg[k] = sums[k] / dm;
        const bool ok = sim_model(mu_a, mu_b, Sg, sums[9] / dm, a.rigid != 0, g);
#pragma unroll
        for (int k = 0; k < kSimModel; ++k) cand[k] = g[k];
        cand_ok = ok ? 1 : 0;
      }
      __syncthreads();
      double G[kSimModel], GT[kSimTest];
#pragma unroll
      for (int k = 0; k < kSimModel; ++k) G[k] = cand[k];
      sim_test_form(G, GT);
      const bool ok = cand_ok != 0;
      const int rc = sim_count(a, base, n, GT, tid);         // its barriers also close the reads of cand and sums
      if (!(ok && rc >= standing)) break;
#pragma unroll
      for (int k = 0; k < kSimModel; ++k) sim[k] = G[k];
#pragma unroll
      for (int k = 0; k < kSimTest; ++k) T[k] = GT[k];
      standing = rc;
      ++stood;
    }
    if (a.iters > 0 && stood == 0) flags |= SFM_SIMILARITY_KEPT_HYPOTHESIS;
  }
  if (tid == 0) {
    const bool solved = !(flags & (SFM_SIMILARITY_TOO_FEW | SFM_SIMILARITY_NO_MODEL));
#pragma unroll
    for (int k = 0; k < kSimModel; ++k) a.sim_out[kSimModel * (size_t)s + k] = solved ? sim[k] : 0.0;
    a.status[s] = flags;
  }
}

// ---------------------------------------------------------------------------------------------
// judge: what the model that stands makes of the correspondences
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void similarity_judge_kernel(SimArgs a) {
  __shared__ int total;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int flags = a.status[s];
  const bool solved = !(flags & (SFM_SIMILARITY_TOO_FEW | SFM_SIMILARITY_NO_MODEL));
  double sim[kSimModel], T[kSimTest];
#pragma unroll
  for (int k = 0; k < kSimModel; ++k) sim[k] = a.sim_out[kSimModel * (size_t)s + k];
  sim_test_form(sim, T);
  int nin = 0;
  for (int i = tid; i < n; i += kMatchThreads) {
    const bool in = solved & sim_inlier(T, sim_load(a, (long long)base + i), a.max_err2);
    if (a.obs_inlier) a.obs_inlier[(size_t)base + i] = in ? 1 : 0;
    nin += in;
  }
  nin = block_sum_int(nin, &total);
  if (tid != 0) return;
  if (a.n_inliers) a.n_inliers[s] = nin;
  robust_summary_add(a.summary, solved, false, flags & SFM_SIMILARITY_TOO_FEW, flags & SFM_SIMILARITY_KEPT_HYPOTHESIS, n, nin);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// What a call keeps on the device besides the caller's arrays.
struct SimilarityWork {
  HypPlan plan;
  RobustStandIns stand_in;
  DevBuf<int> ptr, counts, win_count;
  DevBuf<double> hyp_test, hyp_sim;
  DevBuf<unsigned char> hyp_ok;
};

// The options every form of the call refuses, in this order (also sfm_ba_align's, sfm_ba_host.hip).
int similarity_check_options(const char* who, double max_err2, int max_hyp, int iters, int flags) {
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, iters));
  if (flags & ~SFM_SIMILARITY_RIGID) { set_error("%s: flags = %d holds unknown bits", who, flags); return SFM_E_SHAPE; }
  return SFM_OK;
}

// The one body of sfm_similarity_ransac and sfm_similarity_ransac_dev: checked arguments and device pointers in
// (n_sets > 0), the kernels enqueued on s out.  w lives until the caller has waited for s.
static int similarity_run(const char* who, int n_sets, const int* set_ptr, long long M, const double* d_src, const double* d_dst,
                          double max_err2, int max_hyp, int iters, int flags, double* d_sim_out, const RobustPtrs& out,
                          SimilarityWork& w, hipStream_t s) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  SFM_TRY(w.plan.build(who, n_sets, set_ptr, kMatchBlockObs, INT_MAX / 32, [&](int, int n, long long& hyps) {
    hyps = max_hyp;
    return n >= kSimMinSet;
  }, s));
  const size_t v = (size_t)n_sets, nh = w.plan.n_hyp;
  SimArgs a = {};
  a.n_sets = n_sets; a.M = M; a.src = d_src; a.dst = d_dst;
  a.max_err2 = max_err2; a.max_hyp = max_hyp; a.iters = iters; a.rigid = (flags & SFM_SIMILARITY_RIGID) ? 1 : 0;
  a.sim_out = d_sim_out;
  out.into(a);
  SFM_TRY(w.ptr.upload(set_ptr, v + 1, s));
  SFM_TRY(w.hyp_test.alloc(nh * kSimTest, s)); SFM_TRY(w.hyp_sim.alloc(nh * kSimModel, s));
  SFM_TRY(w.hyp_ok.alloc(nh, s)); SFM_TRY(w.counts.alloc(nh, s)); SFM_TRY(w.win_count.alloc(v, s));
  SFM_TRY(w.stand_in.fill(a, v, true, s));
  a.ptr = w.ptr.p; a.hyp_off = w.plan.hyp_off.p; a.blocks = w.plan.blocks.p;
  a.hyp_test = w.hyp_test.p; a.hyp_sim = w.hyp_sim.p; a.hyp_ok = w.hyp_ok.p; a.counts = w.counts.p; a.win_count = w.win_count.p;
  if (nh) {
    SFM_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * nh, s));
    similarity_hyp_kernel<<<(unsigned)((nh + 63) / 64), 64, 0, s>>>(a, (int)nh);
    similarity_score_kernel<<<w.plan.n_blocks, kMatchThreads, 0, s>>>(a);
  }
  similarity_pick_kernel<<<n_sets, 64, 0, s>>>(a);
  similarity_refit_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  similarity_judge_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_similarity_sample(int n, int max_hyp, int h, int idx[3]) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (n < kSimMinSet || max_hyp < 1 || max_hyp > kHypMax) return 0;
  if (h >= 0 && h < max_hyp && idx != nullptr)
    for (int k = 0; k < 3; ++k) idx[k] = similarity_sample_index(n, h, k);
  return max_hyp;
}

int sfm_similarity_ransac_dev(int n_sets, const int* set_ptr, int64_t M, const double* d_src, const double* d_dst, double max_err2,
                              int max_hyp, int iters, int flags, double* d_sim_out, unsigned char* d_obs_inlier, int* d_n_inliers,
                              int* d_best_hyp, int* d_status, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_similarity_ransac_dev";
  SFM_TRY(similarity_check_options(who, max_err2, max_hyp, iters, flags));
  SFM_TRY(robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true));
  if (n_sets > 0 && (d_sim_out == nullptr || (M > 0 && (d_src == nullptr || d_dst == nullptr)))) { set_error("%s: null device pointer", who); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_sets == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  SimilarityWork w;
  SFM_TRY(similarity_run(who, n_sets, set_ptr, M, d_src, d_dst, max_err2, max_hyp, iters, flags, d_sim_out,
                         RobustPtrs{d_obs_inlier, d_n_inliers, d_best_hyp, d_status, d_summary}, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_similarity_ransac(int n_sets, const int* set_ptr, int64_t M, const double* src, const double* dst, double max_err2,
                          int max_hyp, int iters, int flags, double* sim_out, unsigned char* obs_inlier, int* n_inliers,
                          int* best_hyp, int* status, int64_t* summary) {
  const char* who = "sfm_similarity_ransac";
  SFM_TRY(similarity_check_options(who, max_err2, max_hyp, iters, flags));
  SFM_TRY(robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true));
  if (n_sets > 0 && (sim_out == nullptr || (M > 0 && (src == nullptr || dst == nullptr)))) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
  robust_summary_clear(summary);
  if (n_sets == 0) return SFM_OK;
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_sets, m = (size_t)M;
  DevBuf<double> dA, dB;
  HostOut<double> oS;
  RobustOut o;
  SimilarityWork w;
  SFM_TRY(dA.upload(src, 3 * m, s));
  SFM_TRY(dB.upload(dst, 3 * m, s));
  SFM_TRY(oS.want(sim_out, kSimModel * v, s));
  SFM_TRY(o.want(m, v, obs_inlier, n_inliers, best_hyp, status, summary, s));
  SFM_TRY(similarity_run(who, n_sets, set_ptr, M, dA.p, dB.p, max_err2, max_hyp, iters, flags, oS.dev(), o.dev(), w, s));
  SFM_TRY(oS.fetch(s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
