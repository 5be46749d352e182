// sfm_twoview_pose.hip — relative pose of a verified pair: four candidates, cheirality vote, parallax (gfx950).
//
// What follows the robust two-view geometry (sfm_twoview.hip: F) and the robust homography (sfm_homography.hip: H): the
// pose (R, t), X_right = R X_left + t, of the right view of every set of matches, decided by an integer vote of the
// selected matches.  The rule is stated in sfm_hip.h, block "relative pose of a verified pair".  The stages, for a batch
// of sets in one call:
//   vote     one workgroup per set: the number of selected matches and, for a homography, the counts of b . (Hn a) > 0 and
//            < 0 that fix the sign of Hn (block_sum_int)
//   cand     one lane per set: the small algebra -- E0 = K_r^T F K_l or Hn = K_r^-1 H K_l, its singular values and vectors
//            (svd3), the two rotations ordered by trace, the canonised translation, the four candidates of 12 doubles
//            each and the bits that say which of them are valid
//   score    the hot path: a workgroup of 256 owns 1 024 matches of one set as rays, four per lane, in registers; the four
//            poses of the set (384 bytes) are broadcast from LDS; every lane tests its four matches without a branch or a
//            division (pose_front), a wave adds the popcounts of its four ballots and issues one integer atomicAdd per
//            candidate (robust_score_block with CANDS = 4, the shape of the resection's four roots)
//   judge    one workgroup per set: the pick (wave_arg_best over the four counts: the largest count, then the lowest
//            candidate), the tie, the winner's walk over the matches for obs_front, X_out, n_front and n_parallax, the
//            status and the summary
// One body per kernel serves every set size.  No floating-point value is accumulated at all; the counts are integers: a
// set's bits depend on its own matches, its model, the intrinsics and the options only.
#include <climits>
#include <cmath>

#include "sfm_eight_point.h"   // svd3, default contraction
#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_robust.h"
#include "sfm_match_norm.h"
#include "sfm_pose_rays.h"

namespace sfm {

constexpr int kPoseCands = SFM_POSE_CANDIDATES;
constexpr int kPoseModel = 12;                        // R row-major, then t
constexpr int kPoseStride = kPoseCands * kPoseModel;  // the four candidates of a set: 48 doubles
constexpr int kPoseModelOk = 16;                      // bit 4 of cand_ok: the model passed step 2 / step 3
constexpr double kPoseEps3 = 3.0 * 2.220446049250313e-16;

struct PoseArgs {
  int n_sets;
  long long M;
  const int* ptr;               // [n_sets + 1]
  const double* left;           // [2][M]
  const double* right;          // [2][M]
  const unsigned char* mask;    // [M] or null
  const double* model;          // [n_sets][9]
  const int* kind;              // [n_sets]
  const int2* blocks;           // score: workgroup -> (set, first of its 1 024 matches, relative)
  double Kl[9], Kr[9];
  double cos2_min;
  int min_parallax;
  int* vote;                    // [n_sets][3] positive, negative, selected
  double* cand;                 // [n_sets][48]
  unsigned char* cand_ok;       // [n_sets] bits 0 .. 3 the candidates, bit 4 the model
  double* normal;               // [n_sets][4][3] the plane normal of every candidate (zeros for F)
  int* counts;                  // [n_sets][4]
  double* R_out;                // [n_sets][9]
  double* t_out;                // [n_sets][3]
  double* n_out;                // [n_sets][3] or null; so are all below
  int* cand_front;              // [n_sets][4]
  int* n_front;
  int* n_parallax;
  int* best_cand;
  int* status;
  unsigned char* obs_front;     // [M]
  double* X_out;                // [3][M]
  unsigned long long* summary;  // [6]
};

__device__ __forceinline__ MatchView pose_view(const PoseArgs& a) { return {a.left, a.right, a.M}; }

// The rays of match i and whether it is SELECTED.
__device__ __forceinline__ bool pose_rays(const PoseArgs& a, long long i, PoseRays& r) {
  const bool finite = pose_rays_of(a.Kl, a.Kr, match_load(pose_view(a), i), r);
  const bool on = a.mask ? a.mask[i] != 0 : true;
  return finite & on;
}

__device__ __forceinline__ void pose_mul3(const double* A, const double* B, double* C) {   // C = A B, row-major
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = __builtin_fma(A[3 * r + 2], B[6 + c], __builtin_fma(A[3 * r + 1], B[3 + c], A[3 * r] * B[c]));
}

// Hn = K_r^-1 H K_l: the product H K_l, then every column by back substitution.
__device__ __forceinline__ void pose_hn(const PoseArgs& a, const double* H, double (&Hn)[9]) {
  double P[9];
  pose_mul3(H, a.Kl, P);
  const double* K = a.Kr;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double z = P[6 + c];
    const double y = __builtin_fma(-K[5], z, P[3 + c]) / K[4];
    const double x = __builtin_fma(-K[2], z, __builtin_fma(-K[1], y, P[c])) / K[0];
    Hn[c] = x; Hn[3 + c] = y; Hn[6 + c] = z;
  }
}

// t scaled to length 1 with its entry of largest magnitude (the first of them) positive; `flip` is the sign applied.
// False if t is not finite or zero.
__device__ __forceinline__ bool pose_canon3(double* t, double& flip) {
  double big = -1.0, sign = 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool larger = fabs(t[k]) > big;
    sign = larger ? (t[k] < 0.0 ? -1.0 : 1.0) : sign;
    big = larger ? fabs(t[k]) : big;
  }
  const double ss = pose_dot(t, t);
  const double nrm = sign * sqrt(ss);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = t[k] / nrm;
  flip = sign;
  return ss > 0.0 && isfinite(ss);
}

// ---------------------------------------------------------------------------------------------
// vote: the selected matches of every set and the sign vote of a homography
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void pose_vote_kernel(PoseArgs a) {
  __shared__ int total[3];                                 // one word per sum: a thread may enter the next while another reads the last
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const bool is_h = a.kind[s] == SFM_POSE_FROM_H;
  double Hn[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Hn[k] = 0.0;
  if (is_h) {
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = a.model[9 * (size_t)s + k];
    pose_hn(a, H, Hn);
  }
  int pos = 0, neg = 0, sel = 0;
  for (int i = tid; i < n; i += kMatchThreads) {
    PoseRays r;
    const bool on = pose_rays(a, (long long)base + i, r);
    const double h0 = __builtin_fma(Hn[0], r.a0, __builtin_fma(Hn[1], r.a1, Hn[2]));
    const double h1 = __builtin_fma(Hn[3], r.a0, __builtin_fma(Hn[4], r.a1, Hn[5]));
    const double h2 = __builtin_fma(Hn[6], r.a0, __builtin_fma(Hn[7], r.a1, Hn[8]));
    const double v = __builtin_fma(r.b0, h0, __builtin_fma(r.b1, h1, h2));
    sel += on;
    pos += on & (v > 0.0);
    neg += on & (v < 0.0);
  }
  pos = block_sum_int(pos, &total[0]);
  neg = block_sum_int(neg, &total[1]);
  sel = block_sum_int(sel, &total[2]);
  if (tid != 0) return;
  a.vote[3 * (size_t)s] = pos; a.vote[3 * (size_t)s + 1] = neg; a.vote[3 * (size_t)s + 2] = sel;
}

// ---------------------------------------------------------------------------------------------
// cand: the four candidates of every set
// ---------------------------------------------------------------------------------------------
// Two rotations (row-major) with their translations into the four candidates: the larger trace first, candidate 2 i + j
// is (R_i, t_i) for j = 0 and (R_i, -t_i) for j = 1; nrm[i] the normal that goes with (R_i, t_i).  Returns the valid bits.
__device__ __forceinline__ int pose_emit(const double (*R)[9], const double (*t)[3], const double (*nrm)[3], const bool* ok,
                                         double* cand, double* normal) {
  const double tr0 = R[0][0] + R[0][4] + R[0][8], tr1 = R[1][0] + R[1][4] + R[1][8];
  const int first = (tr1 > tr0) ? 1 : 0;
  int bits = 0;
  for (int i = 0; i < 2; ++i) {
    const int src = i == 0 ? first : 1 - first;
    for (int j = 0; j < 2; ++j) {
      double* c = cand + kPoseModel * (2 * i + j);
      const double sg = j ? -1.0 : 1.0;
      for (int k = 0; k < 9; ++k) c[k] = ok[src] ? R[src][k] : 0.0;
      for (int k = 0; k < 3; ++k) c[9 + k] = ok[src] ? sg * t[src][k] : 0.0;
      for (int k = 0; k < 3; ++k) normal[3 * (2 * i + j) + k] = ok[src] ? sg * nrm[src][k] : 0.0;
      if (ok[src]) bits |= 1 << (2 * i + j);
    }
  }
  return bits;
}

__device__ int pose_from_f(const PoseArgs& a, const double* F, double* cand, double* normal) {
  double KrT[9], P[9], E[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) KrT[3 * r + c] = a.Kr[3 * c + r];
  pose_mul3(F, a.Kl, P);
  pose_mul3(KrT, P, E);
  double B[3][3], V[3][3], sig[3];
  int ord[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i][j] = E[3 * i + j];
  svd3(B, V, sig, ord);
  const bool valid = pose_finite9(E) && sig[ord[1]] > sig[ord[0]] * kPoseEps3;      // false for a NaN too
  double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
  for (int k = 0; k < 3; ++k) {
    u0[k] = B[k][ord[0]] / sig[ord[0]]; u1[k] = B[k][ord[1]] / sig[ord[1]];
    v0[k] = V[k][ord[0]]; v1[k] = V[k][ord[1]];
  }
  pose_cross(u0, u1, u2);
  pose_cross(v0, v1, v2);
  // det [u0 u1 u2] = det [v0 v1 v2] = 1: U W V^T and U W^T V^T are rotations as they are
  double R[2][9], t[2][3], nrm[2][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double skew = __builtin_fma(u1[r], v0[c], -(u0[r] * v1[c])), axis = u2[r] * v2[c];
      R[0][3 * r + c] = axis + skew;
      R[1][3 * r + c] = axis - skew;
    }
  double flip;
  const bool tok = pose_canon3(u2, flip);
  for (int k = 0; k < 3; ++k) { t[0][k] = u2[k]; t[1][k] = u2[k]; nrm[0][k] = 0.0; nrm[1][k] = 0.0; }
  const bool all = valid && tok && pose_finite9(R[0]) && pose_finite9(R[1]);
  const bool ok[2] = {all, all};
  const int bits = pose_emit(R, t, nrm, ok, cand, normal);
  return all ? (bits | kPoseModelOk) : 0;
}

__device__ int pose_from_h(const PoseArgs& a, const double* H, int pos, int neg, double* cand, double* normal) {
  double Hn[9];
  pose_hn(a, H, Hn);
  double B[3][3], V[3][3], sig[3];
  int ord[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i][j] = Hn[3 * i + j];
  svd3(B, V, sig, ord);
  bool valid = pose_finite9(Hn) && sig[ord[2]] > sig[ord[0]] * kPoseEps3;
  const double s1 = sig[ord[1]];
  const double q0 = sig[ord[0]] / s1, q2 = sig[ord[2]] / s1;
  const double l0 = q0 * q0, l2 = q2 * q2;
  valid = valid && (l0 - l2 > 0.0);
  const double sgn = neg > pos ? -1.0 : 1.0;
  double v0[3], v1[3], v2[3], w0[3], w1[3], w2[3], raw2[3];
  for (int k = 0; k < 3; ++k) { v0[k] = V[k][ord[0]]; v1[k] = V[k][ord[1]]; raw2[k] = V[k][ord[2]]; }
  pose_cross(v0, v1, v2);
  const double s2 = pose_dot(v2, raw2) < 0.0 ? -sgn : sgn;                           // Hn v2 = +-(column of B V)
  for (int k = 0; k < 3; ++k) {                                                      // w_k = Hn v_k of the scaled, signed Hn
    w0[k] = sgn * (B[k][ord[0]] / s1); w1[k] = sgn * (B[k][ord[1]] / s1); w2[k] = s2 * (B[k][ord[2]] / s1);
  }
  double Hs[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Hs[3 * r + c] = __builtin_fma(w2[r], v2[c], __builtin_fma(w1[r], v1[c], w0[r] * v0[c]));
  const double al = sqrt(fmax(1.0 - l2, 0.0)), be = sqrt(fmax(l0 - 1.0, 0.0)), den = sqrt(l0 - l2);
  double R[2][9], t[2][3], nrm[2][3];
  bool ok[2];
  for (int i = 0; i < 2; ++i) {
    const double sb = i == 0 ? be : -be;
    double u[3], hu[3], n[3], wn[3];
    for (int k = 0; k < 3; ++k) {
      u[k] = __builtin_fma(sb, v2[k], al * v0[k]) / den;
      hu[k] = __builtin_fma(sb, w2[k], al * w0[k]) / den;
    }
    pose_cross(v1, u, n);
    pose_cross(w1, hu, wn);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[i][3 * r + c] = __builtin_fma(wn[r], n[c], __builtin_fma(hu[r], u[c], w1[r] * v1[c]));
    double T[3];
    for (int r = 0; r < 3; ++r) {
      const double hn = __builtin_fma(Hs[3 * r + 2], n[2], __builtin_fma(Hs[3 * r + 1], n[1], Hs[3 * r] * n[0]));
      const double rn = __builtin_fma(R[i][3 * r + 2], n[2], __builtin_fma(R[i][3 * r + 1], n[1], R[i][3 * r] * n[0]));
      T[r] = hn - rn;
    }
    double flip;
    const bool tok = pose_canon3(T, flip);
    ok[i] = valid && tok && pose_finite9(R[i]);
    for (int k = 0; k < 3; ++k) { t[i][k] = T[k]; nrm[i][k] = flip * n[k]; }
  }
  const int bits = pose_emit(R, t, nrm, ok, cand, normal);
  return valid ? (bits | kPoseModelOk) : 0;
}

__global__ __launch_bounds__(64) void pose_cand_kernel(PoseArgs a) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.n_sets) return;
  double m[9], cand[kPoseStride], normal[3 * kPoseCands];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = a.model[9 * (size_t)s + k];
  const int bits = a.kind[s] == SFM_POSE_FROM_H ? pose_from_h(a, m, a.vote[3 * (size_t)s], a.vote[3 * (size_t)s + 1], cand, normal)
                                                : pose_from_f(a, m, cand, normal);
  for (int k = 0; k < kPoseStride; ++k) a.cand[kPoseStride * (size_t)s + k] = (bits & kPoseModelOk) ? cand[k] : 0.0;
  for (int k = 0; k < 3 * kPoseCands; ++k) a.normal[3 * kPoseCands * (size_t)s + k] = (bits & kPoseModelOk) ? normal[k] : 0.0;
  a.cand_ok[s] = (unsigned char)bits;
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void pose_score_kernel(PoseArgs a) {
  __shared__ double poses[kPoseStride];
  __shared__ unsigned char okb[1];
  const int tid = threadIdx.x;
  const int2 blk = a.blocks[blockIdx.x];
  const int s = blk.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  // four matches per lane as rays, a wave's loads contiguous; a slot beyond the set is not selected
  PoseRays ray[kMatchPerLane];
  bool on[kMatchPerLane];
#pragma unroll
  for (int k = 0; k < kMatchPerLane; ++k) {
    const int i = blk.y + k * kMatchThreads + tid;
    on[k] = pose_rays(a, (long long)base + (i < n ? i : n - 1), ray[k]) & (i < n);
  }
  const double cos2_min = a.cos2_min;
  robust_score_block<kMatchThreads, 1, kPoseStride, kPoseCands, kMatchPerLane>(
      a.cand, a.cand_ok, a.counts, s, 1, poses, okb, [&](const double* p, int k) {
        bool par;
        return (bool)((int)pose_front(p, p + 9, ray[k].a0, ray[k].a1, ray[k].b0, ray[k].b1, cos2_min, &par) & (int)on[k]);
      });
}

// ---------------------------------------------------------------------------------------------
// judge: the pick, and what the winner makes of the matches
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMatchThreads) void pose_judge_kernel(PoseArgs a) {
  __shared__ int total[2];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int base = a.ptr[s], n = a.ptr[s + 1] - base;
  const int bits = a.cand_ok[s], n_sel = a.vote[3 * (size_t)s + 2];
  const int* counts = a.counts + kPoseCands * (size_t)s;
  int best_cnt, best_c;                                    // every wave picks for itself: the first of the largest counts wins
  wave_arg_best(tid & 63, kPoseCands, [&](int c) { return (bits >> c & 1) != 0; }, [&](int c) { return counts[c]; }, best_cnt, best_c);
  const bool won = best_cnt >= 1;
  int flags = 0;
  if (n_sel == 0) flags |= SFM_POSE_EMPTY;
  if (!(bits & kPoseModelOk)) flags |= SFM_POSE_NO_MODEL;
  if (!won) flags |= SFM_POSE_NO_POSE;
  if (won)
    for (int c = 0; c < kPoseCands; ++c)
      if (c != best_c && (bits >> c & 1) && counts[c] == best_cnt) flags |= SFM_POSE_TIED;
  double P[kPoseModel];
#pragma unroll
  for (int k = 0; k < kPoseModel; ++k) P[k] = won ? a.cand[kPoseStride * (size_t)s + kPoseModel * best_c + k] : 0.0;
  int nf = 0, np = 0;
  for (int i = tid; i < n; i += kMatchThreads) {
    PoseRays r;
    const bool on = pose_rays(a, (long long)base + i, r);
    bool par;
    const bool front = (bool)((int)pose_front(P, P + 9, r.a0, r.a1, r.b0, r.b1, a.cos2_min, &par) & (int)on & (int)won);
    par = par & front;
    nf += front; np += par;
    if (a.obs_front) a.obs_front[(size_t)base + i] = front ? (par ? 2 : 1) : 0;
    if (a.X_out) {
      double x[3];
      pose_midpoint(P, r, x);
#pragma unroll
      for (int k = 0; k < 3; ++k) a.X_out[(size_t)k * a.M + base + i] = front ? x[k] : __builtin_nan("");
    }
  }
  nf = block_sum_int(nf, &total[0]);
  np = block_sum_int(np, &total[1]);
  if (tid != 0) return;
  if (won && np < a.min_parallax) flags |= SFM_POSE_NO_PARALLAX;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.R_out[9 * (size_t)s + k] = P[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.t_out[3 * (size_t)s + k] = P[9 + k];
  if (a.n_out)
    for (int k = 0; k < 3; ++k) a.n_out[3 * (size_t)s + k] = won ? a.normal[3 * kPoseCands * (size_t)s + 3 * best_c + k] : 0.0;
  if (a.cand_front)
    for (int c = 0; c < kPoseCands; ++c) a.cand_front[kPoseCands * (size_t)s + c] = (bits >> c & 1) ? counts[c] : -1;
  if (a.n_front) a.n_front[s] = nf;
  if (a.n_parallax) a.n_parallax[s] = np;
  if (a.best_cand) a.best_cand[s] = won ? best_c : -1;
  if (a.status) a.status[s] = flags;
  // slot 1 takes every set with a selected match and no winner, slot 2 the empty ones
  if (a.summary) robust_summary_add(a.summary, won, false, flags & SFM_POSE_EMPTY, flags & SFM_POSE_TIED, n_sel, nf);
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The outputs as device pointers, any of them null but R and t.
struct PosePtrs {
  double *R, *t, *n;
  int *cand_front, *n_front, *n_parallax, *best_cand, *status;
  unsigned char* obs_front;
  double* X;
  int64_t* summary;
};

// What a call keeps on the device besides the caller's arrays.
struct PoseWork {
  HypPlan plan;
  DevBuf<int> ptr, kind, vote, counts;
  DevBuf<double> model, cand, normal;
  DevBuf<unsigned char> cand_ok;
};

// Everything the entry points refuse, without a device.
static int pose_check_args(const char* who, int n_sets, const int* set_ptr, long long M, const int* kind, const double* K_left,
                           const double* K_right, double cos2_min, int min_parallax) {
  if (!(cos2_min >= 0.0 && cos2_min <= 1.0)) { set_error("%s: cos2_min = %g must be in [0, 1]", who, cos2_min); return SFM_E_SHAPE; }
  if (min_parallax < 0) { set_error("%s: min_parallax = %d must be >= 0", who, min_parallax); return SFM_E_SHAPE; }
  SFM_TRY(robust_check_offsets(who, "set", "set_ptr", n_sets, set_ptr, M, true));
  SFM_TRY(pose_check_k(who, "K_left", K_left));
  SFM_TRY(pose_check_k(who, "K_right", K_right));
  if (n_sets > 0 && kind == nullptr) { set_error("%s: null kind", who); return SFM_E_SHAPE; }
  for (int s = 0; s < n_sets; ++s)
    if (kind[s] != SFM_POSE_FROM_F && kind[s] != SFM_POSE_FROM_H) {
      set_error("%s: kind[%d] = %d is neither SFM_POSE_FROM_F nor SFM_POSE_FROM_H", who, s, kind[s]);
      return SFM_E_SHAPE;
    }
  return SFM_OK;
}

// The one body of the entry points: checked arguments and device pointers in (n_sets > 0), the kernels enqueued on s out.
// w lives until the caller has waited for s.
static int pose_run(const char* who, int n_sets, const int* set_ptr, long long M, const double* d_left, const double* d_right,
                    const unsigned char* d_mask, const double* model, const int* kind, const double* K_left, const double* K_right,
                    double cos2_min, int min_parallax, const PosePtrs& out, PoseWork& w, hipStream_t s) {
  SFM_TRY(w.plan.build(who, n_sets, set_ptr, kMatchBlockObs, INT_MAX / 32, [&](int, int, long long& hyps) {
    hyps = 1;
    return true;
  }, s));
  const size_t v = (size_t)n_sets;
  PoseArgs a = {};
  a.n_sets = n_sets; a.M = M; a.left = d_left; a.right = d_right; a.mask = d_mask;
  for (int k = 0; k < 9; ++k) { a.Kl[k] = K_left[k]; a.Kr[k] = K_right[k]; }
  a.cos2_min = cos2_min; a.min_parallax = min_parallax;
  SFM_TRY(w.ptr.upload(set_ptr, v + 1, s)); SFM_TRY(w.kind.upload(kind, v, s)); SFM_TRY(w.model.upload(model, 9 * v, s));
  SFM_TRY(w.vote.alloc(3 * v, s)); SFM_TRY(w.counts.alloc(kPoseCands * v, s)); SFM_TRY(w.cand.alloc(kPoseStride * v, s));
  SFM_TRY(w.normal.alloc(3 * kPoseCands * v, s)); SFM_TRY(w.cand_ok.alloc(v, s));
  a.ptr = w.ptr.p; a.kind = w.kind.p; a.model = w.model.p; a.blocks = w.plan.blocks.p;
  a.vote = w.vote.p; a.counts = w.counts.p; a.cand = w.cand.p; a.normal = w.normal.p; a.cand_ok = w.cand_ok.p;
  a.R_out = out.R; a.t_out = out.t; a.n_out = out.n; a.cand_front = out.cand_front; a.n_front = out.n_front;
  a.n_parallax = out.n_parallax; a.best_cand = out.best_cand; a.status = out.status; a.obs_front = out.obs_front; a.X_out = out.X;
  a.summary = reinterpret_cast<unsigned long long*>(out.summary);
  SFM_HIP(hipMemsetAsync(a.counts, 0, sizeof(int) * kPoseCands * v, s));
  if (a.summary) SFM_HIP(hipMemsetAsync(a.summary, 0, 6 * sizeof(unsigned long long), s));
  pose_vote_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  pose_cand_kernel<<<(n_sets + 63) / 64, 64, 0, s>>>(a);
  if (w.plan.n_blocks) pose_score_kernel<<<w.plan.n_blocks, kMatchThreads, 0, s>>>(a);
  pose_judge_kernel<<<n_sets, kMatchThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_twoview_pose_test(const double R[9], const double t[3], const double a[2], const double b[2], double cos2_min, int* front,
                          int* parallax) {
  if (!R || !t || !a || !b || !front || !parallax) { set_error("sfm_twoview_pose_test: null pointer"); return SFM_E_SHAPE; }
  bool par = false;
  *front = pose_front(R, t, a[0], a[1], b[0], b[1], cos2_min, &par) ? 1 : 0;
  *parallax = par ? 1 : 0;
  return SFM_OK;
}

int sfm_twoview_pose_dev(int n_sets, const int* set_ptr, int64_t M, const double* d_left, const double* d_right,
                         const unsigned char* d_obs_mask, const double* model, const int* kind, const double K_left[9],
                         const double K_right[9], double cos2_min, int min_parallax, double* d_R_out, double* d_t_out, double* d_n_out,
                         int* d_cand_front, int* d_n_front, int* d_n_parallax, int* d_best_cand, int* d_status,
                         unsigned char* d_obs_front, double* d_X_out, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_twoview_pose_dev";
  SFM_TRY(pose_check_args(who, n_sets, set_ptr, M, kind, K_left, K_right, cos2_min, min_parallax));
  if (n_sets > 0 && (d_R_out == nullptr || d_t_out == nullptr || model == nullptr || (M > 0 && (d_left == nullptr || d_right == nullptr)))) {
    set_error("%s: null pointer", who); return SFM_E_SHAPE;
  }
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  if (n_sets == 0) {
    if (d_summary) SFM_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int64_t), s));
    return SFM_OK;
  }
  PoseWork w;
  SFM_TRY(pose_run(who, n_sets, set_ptr, M, d_left, d_right, d_obs_mask, model, kind, K_left, K_right, cos2_min, min_parallax,
                   PosePtrs{d_R_out, d_t_out, d_n_out, d_cand_front, d_n_front, d_n_parallax, d_best_cand, d_status, d_obs_front,
                            d_X_out, d_summary}, w, s));
  return stream_sync(s);      // the work buffers go back to the pool with this call
}

int sfm_twoview_pose(int n_sets, const int* set_ptr, int64_t M, const double* left, const double* right, const unsigned char* obs_mask,
                     const double* model, const int* kind, const double K_left[9], const double K_right[9], double cos2_min,
                     int min_parallax, double* R_out, double* t_out, double* n_out, int* cand_front, int* n_front, int* n_parallax,
                     int* best_cand, int* status, unsigned char* obs_front, double* X_out, int64_t* summary) {
  const char* who = "sfm_twoview_pose";
  SFM_TRY(pose_check_args(who, n_sets, set_ptr, M, kind, K_left, K_right, cos2_min, min_parallax));
  if (n_sets > 0 && (R_out == nullptr || t_out == nullptr || model == nullptr || (M > 0 && (left == nullptr || right == nullptr)))) {
    set_error("%s: null pointer", who); return SFM_E_SHAPE;
  }
  SFM_TRY(ensure_init());
  robust_summary_clear(summary);
  if (n_sets == 0) return SFM_OK;
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)n_sets, m = (size_t)M;
  DevBuf<double> dL, dR;
  DevBuf<unsigned char> dMask;
  HostOut<double> oR, oT, oN, oX;
  HostOut<int> oCand, oFront, oPar, oBest, oStatus;
  HostOut<unsigned char> oObs;
  HostOut<int64_t> oSum;
  PoseWork w;
  SFM_TRY(dL.upload(left, 2 * m, s));
  SFM_TRY(dR.upload(right, 2 * m, s));
  SFM_TRY(dMask.upload_if(obs_mask, m, s));
  SFM_TRY(oR.want(R_out, 9 * v, s)); SFM_TRY(oT.want(t_out, 3 * v, s)); SFM_TRY(oN.want(n_out, 3 * v, s));
  SFM_TRY(oX.want(X_out, 3 * m, s)); SFM_TRY(oCand.want(cand_front, kPoseCands * v, s)); SFM_TRY(oFront.want(n_front, v, s));
  SFM_TRY(oPar.want(n_parallax, v, s)); SFM_TRY(oBest.want(best_cand, v, s)); SFM_TRY(oStatus.want(status, v, s));
  SFM_TRY(oObs.want(obs_front, m, s)); SFM_TRY(oSum.want(summary, 6, s));
  SFM_TRY(pose_run(who, n_sets, set_ptr, M, dL.p, dR.p, dMask.p, model, kind, K_left, K_right, cos2_min, min_parallax,
                   PosePtrs{oR.dev(), oT.dev(), oN.dev(), oCand.dev(), oFront.dev(), oPar.dev(), oBest.dev(), oStatus.dev(),
                            oObs.dev(), oX.dev(), oSum.dev()}, w, s));
  SFM_TRY(oR.fetch(s)); SFM_TRY(oT.fetch(s)); SFM_TRY(oN.fetch(s)); SFM_TRY(oX.fetch(s)); SFM_TRY(oCand.fetch(s));
  SFM_TRY(oFront.fetch(s)); SFM_TRY(oPar.fetch(s)); SFM_TRY(oBest.fetch(s)); SFM_TRY(oStatus.fetch(s)); SFM_TRY(oObs.fetch(s));
  SFM_TRY(oSum.fetch(s));
  return stream_sync(s);
}

// processors.pose_pairs (for a HipDeviceKeyTracker): the pairs of table[ref][que] (sfm_track_pairs_dev, into pool buffers)
// and their pose on the same stream.  Rows 0 and 1 of the (3, n) point arrays are the [2][n] coordinates as they are: only
// the count comes down between the two, no coordinate does.
int sfm_twoview_pose_pairs(sfm_track_store* store, int ref, int que, const unsigned char* inlier, const double model[9], int kind,
                           const double K_left[9], const double K_right[9], double cos2_min, int min_parallax, int* n, int* r_idx,
                           int* q_idx, double R_out[9], double t_out[3], double n_out[3], int* cand_front, int* n_front,
                           int* n_parallax, int* best_cand, int* status, unsigned char* obs_front, double* X_out) {
  const char* who = "sfm_twoview_pose_pairs";
  const int none[2] = {0, 0};
  SFM_TRY(pose_check_args(who, 1, none, 0, &kind, K_left, K_right, cos2_min, min_parallax));
  if (!n || !R_out || !t_out || !model) { set_error("%s: n, R_out, t_out or model is NULL", who); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
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
  DevBuf<unsigned char> dMask;
  HostOut<double> oR, oT, oN, oX;
  HostOut<int> oCand, oFront, oPar, oBest, oStatus;
  HostOut<unsigned char> oObs;
  PoseWork w;
  SFM_TRY(dMask.upload_if(inlier, m, s));
  SFM_TRY(oR.want(R_out, 9, s)); SFM_TRY(oT.want(t_out, 3, s)); SFM_TRY(oN.want(n_out, 3, s)); SFM_TRY(oX.want(X_out, 3 * m, s));
  SFM_TRY(oCand.want(cand_front, kPoseCands, s)); SFM_TRY(oFront.want(n_front, 1, s)); SFM_TRY(oPar.want(n_parallax, 1, s));
  SFM_TRY(oBest.want(best_cand, 1, s)); SFM_TRY(oStatus.want(status, 1, s)); SFM_TRY(oObs.want(obs_front, m, s));
  SFM_TRY(pose_run(who, 1, set_ptr, cnt[0], dRef.p, dQue.p, dMask.p, model, &kind, K_left, K_right, cos2_min, min_parallax,
                   PosePtrs{oR.dev(), oT.dev(), oN.dev(), oCand.dev(), oFront.dev(), oPar.dev(), oBest.dev(), oStatus.dev(),
                            oObs.dev(), oX.dev(), nullptr}, w, s));
  SFM_TRY(oR.fetch(s)); SFM_TRY(oT.fetch(s)); SFM_TRY(oN.fetch(s)); SFM_TRY(oX.fetch(s)); SFM_TRY(oCand.fetch(s));
  SFM_TRY(oFront.fetch(s)); SFM_TRY(oPar.fetch(s)); SFM_TRY(oBest.fetch(s)); SFM_TRY(oStatus.fetch(s)); SFM_TRY(oObs.fetch(s));
  if (r_idx) SFM_TRY(dR.download(r_idx, m, s));
  if (q_idx) SFM_TRY(dQ.download(q_idx, m, s));
  return stream_sync(s);
}

}  // extern "C"
