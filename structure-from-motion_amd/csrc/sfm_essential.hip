// sfm_essential.hip — robust essential matrix: sampled five-point hypotheses (gfx950).
//
// The calibrated twin of sfm_twoview.hip: the caller's intrinsics turn the matches into rays, five of them determine up to
// ten essential matrices, and every one of those is a hypothesis that is a pose already.  The rule is stated in sfm_hip.h,
// block "robust essential matrix"; there is no refit.  The stages, for a batch of sets of matches in one call:
//   hyp      a lane group of 16 per (set, hypothesis), four hypotheses per workgroup of 64: the stratified sample of five
//            (sfm_hyp_number.h), the rays (sfm_pose_rays.h), the minimal solver (sfm_five_point.h, its 5.6 KB of state per
//            hypothesis in LDS), then one lane per solution: F = K_r^-T E K_l^-1 scaled as sfm_twoview_ransac scales its
//            F_out, and the sample gate
//   score    the hot path of large sets, as in sfm_twoview.hip: a workgroup of 256 owns 1 024 matches, four per lane, in
//            registers as pixels, and ONE batch of 16 hypotheses with their ten candidates each (11 520 bytes of LDS); a
//            candidate without its valid bit costs nothing but its share of the copy.  The batches of a set go to
//            different workgroups (grid.y): about four candidates of ten are valid, so a set has four times the score
//            work of the eight-point estimator, and one pair of views has only two workgroups by its matches
//   pick     one wave per set: the lexicographic arg-best over (count, h, r), the number of valid candidates
//   judge    one workgroup per set: obs_inlier, n_inliers and the summary of the winner
// Ten candidates per hypothesis with valid bits were chosen over a compacted list: a compaction needs a scan over all
// hypotheses of the call between hyp and score and a table from slot to (h, r) for the pick, and the batch copy it saves is
// 720 bytes per hypothesis and workgroup out of LDS-resident work that tests 1 024 matches per valid candidate.
// No floating-point value is accumulated with an atomic; the counts are integers: a set's bits depend on its own
// matches, the intrinsics and the options only.
#include <climits>
#include <cmath>

#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"
#include "sfm_match_norm.h"
#include "sfm_pose_rays.h"
#include "sfm_five_point.h"

namespace sfm {

constexpr int kEsMinSet = 6;          // a set needs one match besides a sample's five
constexpr int kEsMinCount = 6;        // ... and so does a winner
constexpr int kEsCands = kFpMaxSol;   // candidates per hypothesis
constexpr int kEsBatch = 16;          // hypotheses per LDS batch of the score: 16 x 90 doubles = 11 520 bytes
constexpr int kEsGroup = 16;          // lanes per hypothesis in the hyp kernel
constexpr int kEsPerBlock = 64 / kEsGroup;

struct EsArgs {
  int n_sets;
  long long M;
  const int* ptr;               // [n_sets + 1]
  const double* left;           // [2][M]
  const double* right;          // [2][M]
  const int* hyp_off;           // [n_sets + 1] first hypothesis of every set (a set below six matches has none)
  const int2* blocks;           // score: workgroup -> (set, first of its 1 024 matches, relative)
  double Kl[9], Kr[9];
  double max_err2;
  double* hyp_E;                // [hypotheses][10][9]
  double* hyp_F;                // [hypotheses][10][9]
  unsigned short* hyp_ok;       // [hypotheses] bit r: candidate r passed the gate
  int* counts;                  // [hypotheses][10]
  double* F;                    // [n_sets][9] the winner's F (the caller's F_out or a work buffer)
  double* E_out;                // [n_sets][9]
  int* best_hyp;                // [n_sets]
  int* best_root;               // [n_sets] or null
  int* n_valid;                 // [n_sets] or null
  int* status;                  // [n_sets]
  unsigned char* obs_inlier;    // [M] or null
  int* n_inliers;               // [n_sets] or null
  unsigned long long* summary;  // [6]
};

__device__ __forceinline__ MatchView es_view(const EsArgs& a) { return {a.left, a.right, a.M}; }

// Step 3 of the rule: the pixel matrix of an essential matrix, scaled as sfm_twoview_ransac's F_out (Frobenius norm 1, the
// entry of largest magnitude positive).  False if it is not finite or zero.  Hypothesis kernel and host hook.
__host__ __device__ inline bool essential_to_pixels(const double* Kl, const double* Kr, const double* E, double* F) {
  refine_to_pixels(Kl, Kr, E, F);
  return fp_canon9(F);
}

struct EsDeviceGroup {
  int lane;
  __device__ int first() const { return lane; }
  __device__ int step() const { return kEsGroup; }
  __device__ void sync() const { __syncthreads(); }
};

// ---------------------------------------------------------------------------------------------
// hyp: the solutions of a sample
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void essential_hyp_kernel(EsArgs a, int n_hyp) {
  __shared__ FivePointWork work[kEsPerBlock];
  const int grp = threadIdx.x / kEsGroup, lane = threadIdx.x % kEsGroup;
  const int g_raw = blockIdx.x * kEsPerBlock + grp;
  const bool live = g_raw < n_hyp;
  const int g = live ? g_raw : n_hyp - 1;                  // a group past the end repeats the last hypothesis and writes nothing
  const int s = hyp_owner(a.hyp_off, a.n_sets, g), h = g - a.hyp_off[s];
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  FivePointWork& w = work[grp];
  if (lane < 5) {
    const int idx = essential_sample_index(n, h, lane);
    PoseRays r;
    pose_rays_of(a.Kl, a.Kr, match_load(es_view(a), (long long)base + idx), r);
    w.a[lane][0] = r.a0; w.a[lane][1] = r.a1; w.b[lane][0] = r.b0; w.b[lane][1] = r.b1;
  }
  __syncthreads();
  five_point_solve(EsDeviceGroup{lane}, w);
  if (lane >= kEsCands) return;
  // one lane per candidate: the pixel matrix and the gate
  double E[9], F[9];
  const bool have = lane < w.n;
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = have ? w.E[have ? lane : 0][k] : 0.0;
  bool ok = essential_to_pixels(a.Kl, a.Kr, E, F) && have;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const TvMatch m = match_load(es_view(a), (long long)base + essential_sample_index(n, h, k));
    ok = twoview_inlier(F, m.xl, m.yl, m.xr, m.yr, a.max_err2) && ok;
  }
  const unsigned long long bits = __ballot(ok) >> (grp * kEsGroup) & ((1u << kEsCands) - 1);
  if (!live) return;
  double* oE = a.hyp_E + ((size_t)g * kEsCands + lane) * 9;
  double* oF = a.hyp_F + ((size_t)g * kEsCands + lane) * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) { oE[k] = have ? E[k] : 0.0; oF[k] = have ? F[k] : 0.0; }
  if (lane == 0) a.hyp_ok[g] = (unsigned short)bits;
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void essential_score_kernel(EsArgs a) {
  __shared__ double Fm[kEsBatch * kEsCands * 9];
  __shared__ unsigned short okb[kEsBatch];
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
    m[k] = match_load(es_view(a), (long long)base + (i < n ? i : n - 1));
    if (!(i < n)) m[k].xl = __builtin_nan("");
  }
  // blockIdx.y deals the hypotheses of the set out in batches: a set of 2 000 matches has two workgroups by its matches alone
  const int c0 = blockIdx.y * kEsBatch;
  if (c0 >= H) return;
  robust_score_block<kMatchThreads, kEsBatch, kEsCands * 9, kEsCands, kMatchPerLane>(
      a.hyp_F, a.hyp_ok, a.counts, h0 + c0, min(kEsBatch, H - c0), Fm, okb,
      [&](const double* F, int k) { return twoview_inlier(F, m[k].xl, m[k].yl, m[k].xr, m[k].yr, a.max_err2); });
}

// ---------------------------------------------------------------------------------------------
// pick: the winner of every set
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void essential_pick_kernel(EsArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = a.ptr[s + 1] - a.ptr[s];
  const int h0 = a.hyp_off[s], H = a.hyp_off[s + 1] - h0;
  int best_cnt, best_i;                                    // candidate i = 10 h + r: the first of the largest counts wins
  wave_arg_best(lane, H * kEsCands, [&](int i) { return (a.hyp_ok[h0 + i / kEsCands] >> (i % kEsCands) & 1) != 0; },
                [&](int i) { return a.counts[(size_t)h0 * kEsCands + i]; }, best_cnt, best_i);
  int valid = 0;
  for (int h = lane; h < H; h += 64) valid += __popc((unsigned)a.hyp_ok[h0 + h]);
  valid = group_sum<64>(valid);
  if (lane != 0) return;
  const bool won = best_cnt >= kEsMinCount;
  a.best_hyp[s] = won ? best_i / kEsCands : -1;
  if (a.best_root) a.best_root[s] = won ? best_i % kEsCands : -1;
  if (a.n_valid) a.n_valid[s] = valid;
  a.status[s] = n < kEsMinSet ? SFM_ESSENTIAL_TOO_FEW : (won ? 0 : SFM_ESSENTIAL_NO_MODEL);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    a.E_out[9 * (size_t)s + k] = won ? a.hyp_E[((size_t)h0 * kEsCands + best_i) * 9 + k] : 0.0;
    a.F[9 * (size_t)s + k] = won ? a.hyp_F[((size_t)h0 * kEsCands + best_i) * 9 + k] : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------
// judge: what the winner makes of the matches
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void essential_judge_kernel(EsArgs a) {
  __shared__ int total;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int flags = a.status[s];
  const bool solved = flags == 0;
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = a.F[9 * (size_t)s + k];
  int nin = 0;
  for (int i = tid; i < n; i += kMatchThreads) {
    const TvMatch m = match_load(es_view(a), (long long)base + i);
    const bool in = solved & twoview_inlier(F, m.xl, m.yl, m.xr, m.yr, a.max_err2);
    if (a.obs_inlier) a.obs_inlier[(size_t)base + i] = in ? 1 : 0;
    nin += in;
  }
  nin = block_sum_int(nin, &total);
  if (tid != 0) return;
  if (a.n_inliers) a.n_inliers[s] = nin;
  robust_summary_add(a.summary, solved, false, flags & SFM_ESSENTIAL_TOO_FEW, 0, n, nin);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The outputs of a call besides those of RobustPtrs, as device pointers; any but E_out may be null.
struct EssentialPtrs { double *E_out, *F_out; int *best_root, *n_valid; };

// What a call keeps on the device besides the caller's arrays.
struct EssentialWork {
  HypPlan plan;
  RobustStandIns stand_in;
  DevBuf<int> ptr, counts;
  DevBuf<double> hyp_E, hyp_F, F;
  DevBuf<unsigned short> hyp_ok;
};

static int essential_check(const char* who, double max_err2, int max_hyp, const double* K_left, const double* K_right, int n_sets,
                           const int* set_ptr, int64_t M) {
  SFM_TRY(robust_check_args(who, max_err2, max_hyp, 0.0, 0));
  SFM_TRY(pose_check_k(who, "K_left", K_left));
  SFM_TRY(pose_check_k(who, "K_right", K_right));
  return robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true);
}

// The one body of sfm_essential_ransac and sfm_essential_ransac_dev: checked arguments and device pointers in
// (n_sets > 0), the kernels enqueued on s out.  w lives until the caller has waited for s.
static int essential_run(const char* who, int n_sets, const int* set_ptr, long long M, const double* d_left, const double* d_right,
                         const double* K_left, const double* K_right, double max_err2, int max_hyp, const EssentialPtrs& e,
                         const RobustPtrs& out, EssentialWork& w, hipStream_t s) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  SFM_TRY(w.plan.build(who, n_sets, set_ptr, kMatchBlockObs, INT_MAX / (32 * kEsCands), [&](int, int n, long long& hyps) {
    hyps = max_hyp;
    return n >= kEsMinSet;
  }, s));
  const size_t v = (size_t)n_sets, nh = w.plan.n_hyp;
  EsArgs a = {};
  a.n_sets = n_sets; a.M = M; a.left = d_left; a.right = d_right; a.max_err2 = max_err2;
  for (int k = 0; k < 9; ++k) { a.Kl[k] = K_left[k]; a.Kr[k] = K_right[k]; }
  a.E_out = e.E_out; a.F = e.F_out; a.best_root = e.best_root; a.n_valid = e.n_valid;
  out.into(a);
  SFM_TRY(w.ptr.upload(set_ptr, v + 1, s));
  SFM_TRY(w.hyp_E.alloc(nh * kEsCands * 9, s)); SFM_TRY(w.hyp_F.alloc(nh * kEsCands * 9, s));
  SFM_TRY(w.hyp_ok.alloc(nh, s)); SFM_TRY(w.counts.alloc(nh * kEsCands, s));
  if (!a.F) { SFM_TRY(w.F.alloc(9 * v, s)); a.F = w.F.p; }
  SFM_TRY(w.stand_in.fill(a, v, true, s));
  a.ptr = w.ptr.p; a.hyp_off = w.plan.hyp_off.p; a.blocks = w.plan.blocks.p;
  a.hyp_E = w.hyp_E.p; a.hyp_F = w.hyp_F.p; a.hyp_ok = w.hyp_ok.p; a.counts = w.counts.p;
  if (nh) {
    SFM_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * nh * kEsCands, s));
    essential_hyp_kernel<<<(unsigned)((nh + kEsPerBlock - 1) / kEsPerBlock), 64, 0, s>>>(a, (int)nh);
    essential_score_kernel<<<dim3(w.plan.n_blocks, (unsigned)((max_hyp + kEsBatch - 1) / kEsBatch)), kMatchThreads, 0, s>>>(a);
  }
  essential_pick_kernel<<<n_sets, 64, 0, s>>>(a);
  essential_judge_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_essential_sample(int n, int max_hyp, int h, int idx[5]) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (n < kEsMinSet || max_hyp < 1 || max_hyp > kHypMax) return 0;
  if (h >= 0 && h < max_hyp && idx != nullptr)
    for (int k = 0; k < 5; ++k) idx[k] = essential_sample_index(n, h, k);
  return max_hyp;
}

int sfm_essential_solve(const double* a, const double* b, double* E, int* n) {
  const char* who = "sfm_essential_solve";
  if (a == nullptr || b == nullptr || E == nullptr || n == nullptr) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  FivePointWork w;
  for (int k = 0; k < 5; ++k) { w.a[k][0] = a[2 * k]; w.a[k][1] = a[2 * k + 1]; w.b[k][0] = b[2 * k]; w.b[k][1] = b[2 * k + 1]; }
  five_point_solve(FpHostGroup{}, w);
  *n = w.n;
  for (int r = 0; r < kFpMaxSol; ++r)
    for (int k = 0; k < 9; ++k) E[9 * r + k] = r < w.n ? w.E[r][k] : 0.0;
  return SFM_OK;
}

int sfm_essential_ransac_dev(int n_sets, const int* set_ptr, int64_t M, const double* d_left, const double* d_right,
                             const double K_left[9], const double K_right[9], double max_err2, int max_hyp, double* d_E_out,
                             double* d_F_out, unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_best_root,
                             int* d_n_valid, int* d_status, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_essential_ransac_dev";
  SFM_TRY(essential_check(who, max_err2, max_hyp, K_left, K_right, n_sets, set_ptr, M));
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_sets == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  if (d_E_out == nullptr || (M > 0 && (d_left == nullptr || d_right == nullptr))) { set_error("%s: null device pointer", who); return SFM_E_SHAPE; }
  EssentialWork w;
  SFM_TRY(essential_run(who, n_sets, set_ptr, M, d_left, d_right, K_left, K_right, max_err2, max_hyp,
                        EssentialPtrs{d_E_out, d_F_out, d_best_root, d_n_valid},
                        RobustPtrs{d_obs_inlier, d_n_inliers, d_best_hyp, d_status, d_summary}, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_essential_ransac(int n_sets, const int* set_ptr, int64_t M, const double* left, const double* right, const double K_left[9],
                         const double K_right[9], double max_err2, int max_hyp, double* E_out, double* F_out,
                         unsigned char* obs_inlier, int* n_inliers, int* best_hyp, int* best_root, int* n_valid, int* status,
                         int64_t* summary) {
  const char* who = "sfm_essential_ransac";
  SFM_TRY(essential_check(who, max_err2, max_hyp, K_left, K_right, n_sets, set_ptr, M));
  robust_summary_clear(summary);
  if (n_sets == 0) return SFM_OK;
  if (E_out == nullptr || (M > 0 && (left == nullptr || right == nullptr))) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_sets, m = (size_t)M;
  DevBuf<double> dL, dR;
  HostOut<double> oE, oF;
  HostOut<int> oRoot, oValid;
  RobustOut o;
  EssentialWork w;
  SFM_TRY(dL.upload(left, 2 * m, s));
  SFM_TRY(dR.upload(right, 2 * m, s));
  SFM_TRY(oE.want(E_out, 9 * v, s)); SFM_TRY(oF.want(F_out, 9 * v, s));
  SFM_TRY(oRoot.want(best_root, v, s)); SFM_TRY(oValid.want(n_valid, v, s));
  SFM_TRY(o.want(m, v, obs_inlier, n_inliers, best_hyp, status, summary, s));
  SFM_TRY(essential_run(who, n_sets, set_ptr, M, dL.p, dR.p, K_left, K_right, max_err2, max_hyp,
                        EssentialPtrs{oE.dev(), oF.dev(), oRoot.dev(), oValid.dev()}, o.dev(), w, s));
  SFM_TRY(oE.fetch(s)); SFM_TRY(oF.fetch(s)); SFM_TRY(oRoot.fetch(s)); SFM_TRY(oValid.fetch(s));
  SFM_TRY(o.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
