// sfm_ba_pcg.hip — matrix-free bundle adjustment of the resident scene: the reduced camera system is solved by
// preconditioned conjugate gradients and never formed; cameras can be held (sfm_ba_iterate_pcg; gfx950).
//
// One outer iteration is one iteration of sfm_ba_iterate with the solve replaced.  With r, Jp, Jx of every observation
// from obs_terms_loss at the prepared cameras, D_p = sum Jx^T Jx + lambda I, ex_p = sum Jx^T r, W = Jp^T Jx:
//   b_c  = sum_{o in c} Jp^T (r - Jx D_p^-1 ex_p)                      rhs of the reduced system
//   S_cc = lambda I + sum_{o in c} (Jp^T Jp - W D_p^-1 W^T)            its diagonal blocks: M = blockdiag(S_cc)
//   q = S p:  t_p = D_p^-1 sum_{o in p} Jx^T (Jp p_c),  v_o = Jp p_c - Jx t_p,  q_c = lambda p_c + sum_{o in c} Jp^T v_o
// over the FREE cameras; a held camera (cam_mask[c] == 0) carries zeros in p, q, x.
//
//   pcg_linearize<G, LOSS>   G lanes per point, lanes stride over the track: J_o = (Jp | Jx) stored once per outer iteration
//                            (160 B per observation), D_p^-1, ex_p, e_o = r - Jx D_p^-1 ex_p, the point's cost share
//   pcg_blocks / _finish     the 35 sums (S_cc lower 28 | b 7) per slice of 64 consecutive entries of the camera-major
//                            list, then per camera the slices added in ascending order, the Cholesky factor of S_cc with
//                            the pivot rule of sfm_ba_covariance, and S_cc^-1 (the stored form of the preconditioner)
//   pcg_init                 x = 0, r = b, z = M^-1 r, p = z, r.z; one workgroup
//   pcg_matvec_points<G>     pass one of q = S p, by point: v_o (two doubles per observation)
//   pcg_matvec_slices        pass two, by slice of the camera-major list: the 7 sums of Jp^T v
//   pcg_update               one workgroup: q_c from its slices in ascending order, p.q, alpha, x, r, z, r.z, the
//                            convergence test, the counter and the done flag, beta, p -- nothing of it leaves the device
//   pcg_backsub<G>           pts += D_p^-1 (ex_p - sum_o W_o^T dp_c)
//   pcg_update_cams          cams += dp, q /= |q|, the prepared camera and its checks, free cameras only
//
// sfm_ba_cost and sfm_ba_minimize_pcg (Levenberg-Marquardt control: include/sfm_hip.h states the rule) add
//   ba_cost<G, LOSS>         the cost of a state from residuals alone, G lanes per point, no Jacobian written
//   lm_grad / lm_gtol        max(|rhs|_inf, |ex|_inf) of a linearisation and the gradient test, which sets the done flag
//   lm_sums / lm_decide      the six sums of a trial per wave, then one wave: the predicted decrease, the gain ratio, the
//                            verdict, the trial's row and the next lambda and nu -- the host reads that row once per trial
// and run the outer iteration through the same host functions as sfm_ba_iterate_pcg (pcg_setup, pcg_enqueue_system,
// pcg_run_cg, pcg_enqueue_step); pcg_backsub<G, true> also keeps dx_p for the step's norm.
//
// Every kernel of the CG loop returns at once when the done flag is set; the host reads the flag once per chunk of
// kPcgChunk enqueued CG iterations.  Fixed summation order everywhere and no floating-point atomic: a lane adds its
// observations in ascending order, a group or a slice is a fixed tree (group_sum), slices and workgroup partials are added
// in ascending order -- the bits depend on the scene, the arguments and `group` only.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "sfm_ba.h"
#include "sfm_ba_terms.h"

namespace sfm {

constexpr int kPcgBlockSums = 35;    // S_cc lower triangle (28) | b (7)
constexpr int kPcgJ = 20;            // doubles per observation of the stored Jacobians: Jp (2 x 7) | Jx (2 x 3)
constexpr int kPcgVecThreads = 1024; // the one workgroup of the vector update: eight lanes per camera, 128 cameras a sweep
// CG iterations enqueued between two reads of the done flag.  A launch that finds the flag set costs about 2 us of stream
// time, a read of the flag a stream synchronisation and a copy, about 15 us: with the 5 to 12 iterations the solve takes
// at the damping this project runs, eight makes it one or two reads and at most seven idle triples of launches.
constexpr int kPcgChunk = 8;
constexpr int kPcgSingular = 3;      // internal status: a diagonal block did not factor (the call returns SFM_E_SINGULAR)

struct PcgState {
  double rz, rz0, rel, tol2;
  int iters, done, status, max_iters;
  int bad_cam, bad_pts;
};

struct PcgDev {
  int V, N;
  long long M;
  int rows;                     // slices of the camera-major list (kCamSlice entries: one wave, one per lane), cam_slice_rows(M, V)
  double lambda;
  const int* pt_ptr;
  const int* cam_idx;
  const int* obs_pt;
  const int* cam_ptr;           // [V+1] the scene's camera-major list
  const int* cam_obs;           // [M]
  const unsigned char* freec;   // [V] 1 = free
  int* row_cam;                 // [rows] camera of a slice, -1: none
  double* J;                    // [M][20]
  double* v;                    // [M][2]  e_o after the linearisation, v_o inside the CG loop
  double* Dinv;                 // [N][6]  xx xy xz yy yz zz
  double* ex;                   // [N][3]
  double* cost_pt;              // [N]
  double* ws;                   // [rows][35]; the matvec uses the first 7 of a row
  double* Minv;                 // [V][49]
  double* b;                    // [V][7]
  double* x;                    // [V][7]  dp
  double* r;
  double* z;
  double* pv;                   // the search direction
  double* dx;                   // [N][3] the points' step of the last back substitution (sfm_ba_minimize_pcg only, else null)
  PcgState* st;
};

// ---------------------------------------------------------------------------------------------
// once per call: the camera of every slice
// ---------------------------------------------------------------------------------------------
__global__ void pcg_rows_kernel(PcgDev a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.V) return;
  const int n = a.cam_ptr[c + 1] - a.cam_ptr[c];
  const int first = (int)cam_slice_first_row(a.cam_ptr[c], c), ns = cam_slice_count(n);
  for (int s = 0; s < ns; ++s)
    if (first + s < a.rows) a.row_cam[first + s] = c;
}

__global__ void pcg_reset_kernel(PcgDev a, double tol2, int max_iters) {
  PcgState* st = a.st;
  st->rz = st->rz0 = st->rel = 0.0;
  st->tol2 = tol2;
  st->iters = 0; st->done = 0; st->status = SFM_PCG_CONVERGED; st->max_iters = max_iters;
  st->bad_cam = a.V; st->bad_pts = 0;
}

// ---------------------------------------------------------------------------------------------
// by point
// ---------------------------------------------------------------------------------------------
// D^-1 of D = (a00 a10 a11 a20 a21 a22) by chol3_inv_fast; false (and zeros): D is not positive definite or not finite
__device__ __forceinline__ bool pcg_point_inverse(const double* a, double* di) {
  bool ok = a[0] > 0.0;
  const double l10sq = ok ? a[1] * a[1] / a[0] : 0.0;
  const double d1 = a[2] - l10sq;
  ok = ok && d1 > 0.0;
  double li[6] = {0, 0, 0, 0, 0, 0};
  if (ok) {
    const double i00 = rsqrt_nr(a[0]), l10 = a[1] * i00, l20 = a[3] * i00;
    const double i11 = rsqrt_nr(d1), l21 = (a[4] - l20 * l10) * i11;
    const double d2 = a[5] - l20 * l20 - l21 * l21;
    ok = d2 > kPtPivotTol * a[5];
    if (ok) chol3_inv_fast(a, li);
  }
  sym3_from_li(li, di);
  return sym3_finite_or_zero(ok, di);
}

template <int G, int LOSS>
__global__ __launch_bounds__(256) void pcg_linearize_kernel(BaDev d, int cur, PcgDev a, int quirks, LossArg<LOSS> la) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pl = t / G;
  const int lane = threadIdx.x % G;
  if (pl >= a.N) return;                                     // whole groups leave together
  const int p = (int)pl;
  const int beg = a.pt_ptr[p], end = a.pt_ptr[p + 1];
  if (end == beg) {
    if (lane == 0) {
      a.cost_pt[p] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) a.Dinv[6 * (size_t)p + k] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) a.ex[3 * (size_t)p + k] = 0.0;
    }
    return;
  }
  const double X = d.px[p], Y = d.py[p], Z = d.pz[p];
  double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};              // D (a00 a10 a11 a20 a21 a22) | ex | cost
  for (int o = beg + lane; o < end; o += G) {
    CamPrep c;
    load_cam(c, d.prep[cur] + a.cam_idx[o]);
    double r[2], Jp[14], Jx[6], rho = 0;
    obs_terms_loss<LOSS>(c, X, Y, Z, d.u[o], d.v[o], quirks, la, r, Jp, Jx, rho);
    if constexpr (LOSS == SFM_LOSS_NONE) rho = r[0] * r[0] + r[1] * r[1];
    double* j = a.J + kPcgJ * (size_t)o;
#pragma unroll
    for (int k = 0; k < 14; ++k) j[k] = Jp[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) j[14 + k] = Jx[k];
    a.v[2 * (size_t)o] = r[0];
    a.v[2 * (size_t)o + 1] = r[1];
    s[0] += Jx[0] * Jx[0] + Jx[3] * Jx[3];
    s[1] += Jx[1] * Jx[0] + Jx[4] * Jx[3];
    s[2] += Jx[1] * Jx[1] + Jx[4] * Jx[4];
    s[3] += Jx[2] * Jx[0] + Jx[5] * Jx[3];
    s[4] += Jx[2] * Jx[1] + Jx[5] * Jx[4];
    s[5] += Jx[2] * Jx[2] + Jx[5] * Jx[5];
    s[6] += Jx[0] * r[0] + Jx[3] * r[1];
    s[7] += Jx[1] * r[0] + Jx[4] * r[1];
    s[8] += Jx[2] * r[0] + Jx[5] * r[1];
    s[9] += rho;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) s[k] = group_sum<G>(s[k]);
  s[0] += a.lambda; s[2] += a.lambda; s[5] += a.lambda;
  double li_order[6] = {s[0], s[1], s[2], s[3], s[4], s[5]};
  double dinv[6];
  // dinv comes out packed (xx xy xz yy yz zz)
  const bool ok = pcg_point_inverse(li_order, dinv);
  double g[3];
  sym3_apply(dinv, s + 6, g);                               // D^-1 ex
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.Dinv[6 * (size_t)p + k] = dinv[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.ex[3 * (size_t)p + k] = s[6 + k];
    a.cost_pt[p] = s[9];
    if (!ok) atomicAdd(&a.st->bad_pts, 1);
  }
  // e_o = r - Jx D^-1 ex (the lane reads back what it stored itself)
  for (int o = beg + lane; o < end; o += G) {
    const double* jx = a.J + kPcgJ * (size_t)o + 14;
    double* e = a.v + 2 * (size_t)o;
    e[0] -= jx[0] * g[0] + jx[1] * g[1] + jx[2] * g[2];
    e[1] -= jx[3] * g[0] + jx[4] * g[1] + jx[5] * g[2];
  }
}

// pass one of q = S p
template <int G>
__global__ __launch_bounds__(256) void pcg_matvec_points_kernel(PcgDev a) {
  if (a.st->done) return;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pl = t / G;
  const int lane = threadIdx.x % G;
  if (pl >= a.N) return;
  const int p = (int)pl;
  const int beg = a.pt_ptr[p], end = a.pt_ptr[p + 1];
  if (end == beg) return;
  double s[3] = {0, 0, 0};
  for (int o = beg + lane; o < end; o += G) {
    const double* j = a.J + kPcgJ * (size_t)o;
    const double* pc = a.pv + 7 * (size_t)a.cam_idx[o];
    double u0 = 0, u1 = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) { u0 += j[k] * pc[k]; u1 += j[7 + k] * pc[k]; }
    a.v[2 * (size_t)o] = u0;
    a.v[2 * (size_t)o + 1] = u1;
    s[0] += j[14] * u0 + j[17] * u1;
    s[1] += j[15] * u0 + j[18] * u1;
    s[2] += j[16] * u0 + j[19] * u1;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = group_sum<G>(s[k]);
  double di[6], tp[3];
#pragma unroll
  for (int k = 0; k < 6; ++k) di[k] = a.Dinv[6 * (size_t)p + k];
  sym3_apply(di, s, tp);
  for (int o = beg + lane; o < end; o += G) {
    const double* jx = a.J + kPcgJ * (size_t)o + 14;
    double* v = a.v + 2 * (size_t)o;
    v[0] -= jx[0] * tp[0] + jx[1] * tp[1] + jx[2] * tp[2];
    v[1] -= jx[3] * tp[0] + jx[4] * tp[1] + jx[5] * tp[2];
  }
}

// pts += D^-1 (ex - sum_o W_o^T dp_c); KEEP_DX (the controlled minimisation): dx_p is also stored in a.dx
template <int G, bool KEEP_DX>
__global__ __launch_bounds__(256) void pcg_backsub_kernel(BaDev d, PcgDev a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pl = t / G;
  const int lane = threadIdx.x % G;
  if (pl >= a.N) return;
  const int p = (int)pl;
  const int beg = a.pt_ptr[p], end = a.pt_ptr[p + 1];
  if (end == beg) return;                                    // a point with no observation is untouched
  double s[3] = {0, 0, 0};
  for (int o = beg + lane; o < end; o += G) {
    const double* j = a.J + kPcgJ * (size_t)o;
    const double* dp = a.x + 7 * (size_t)a.cam_idx[o];
    double u0 = 0, u1 = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) { u0 += j[k] * dp[k]; u1 += j[7 + k] * dp[k]; }
    s[0] += j[14] * u0 + j[17] * u1;
    s[1] += j[15] * u0 + j[18] * u1;
    s[2] += j[16] * u0 + j[19] * u1;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = group_sum<G>(s[k]);
  if (lane != 0) return;
  double di[6], g[3], dx[3];
#pragma unroll
  for (int k = 0; k < 6; ++k) di[k] = a.Dinv[6 * (size_t)p + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = a.ex[3 * (size_t)p + k] - s[k];
  sym3_apply(di, g, dx);
  d.px[p] += dx[0];
  d.py[p] += dx[1];
  d.pz[p] += dx[2];
  if constexpr (KEEP_DX) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.dx[3 * (size_t)p + k] = dx[k];
  }
}

// ---------------------------------------------------------------------------------------------
// by camera: one wave per slice of 64 consecutive entries of the camera-major list
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pcg_blocks_kernel(PcgDev a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const int cam = a.row_cam[row];
  if (cam < 0 || !a.freec[cam]) return;
  const int e = a.cam_ptr[cam] + (row - (int)cam_slice_first_row(a.cam_ptr[cam], cam)) * kCamSlice + lane;
  double acc[kPcgBlockSums];
#pragma unroll
  for (int k = 0; k < kPcgBlockSums; ++k) acc[k] = 0.0;
  if (e < a.cam_ptr[cam + 1]) {
    const int o = a.cam_obs[e];
    const int p = a.obs_pt[o];
    double j[kPcgJ], di[6];
#pragma unroll
    for (int k = 0; k < kPcgJ; ++k) j[k] = a.J[kPcgJ * (size_t)o + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) di[k] = a.Dinv[6 * (size_t)p + k];
    const double e0 = a.v[2 * (size_t)o], e1 = a.v[2 * (size_t)o + 1];
    double W[7][3], Yw[7][3];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) W[i][k] = j[i] * j[14 + k] + j[7 + i] * j[17 + k];
      sym3_apply(di, W[i], Yw[i]);
    }
    int k = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
      for (int q = 0; q <= i; ++q) {
        acc[k] = (j[i] * j[q] + j[7 + i] * j[7 + q]) - (Yw[i][0] * W[q][0] + Yw[i][1] * W[q][1] + Yw[i][2] * W[q][2]);
        ++k;
      }
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) acc[28 + i] = j[i] * e0 + j[7 + i] * e1;
  }
#pragma unroll
  for (int k = 0; k < kPcgBlockSums; ++k) acc[k] = group_sum<64>(acc[k]);
  if (lane == 0) {
    double* dst = a.ws + kPcgBlockSums * (size_t)row;
#pragma unroll
    for (int k = 0; k < kPcgBlockSums; ++k) dst[k] = acc[k];
  }
}

// ... and one wave per camera: the slices in ascending order, S_cc = L L^T, S_cc^-1.  A pivot that is not above 1e-9 of
// its diagonal entry (the rule of sfm_ba_covariance; a NaN fails it too) names the camera in st->bad_cam (the lowest wins).
__global__ __launch_bounds__(64) void pcg_blocks_finish_kernel(PcgDev a) {
  __shared__ double sums[kPcgBlockSums];
  __shared__ double A[7][7], Li[7][7];
  const int cam = blockIdx.x, tid = threadIdx.x;
  double* mi = a.Minv + 49 * (size_t)cam;
  if (!a.freec[cam]) {
    if (tid < 49) mi[tid] = 0.0;
    if (tid < 7) a.b[7 * (size_t)cam + tid] = 0.0;
    return;
  }
  const int n = a.cam_ptr[cam + 1] - a.cam_ptr[cam], ns = cam_slice_count(n);
  if (tid < kPcgBlockSums) {
    const double* part = a.ws + kPcgBlockSums * cam_slice_first_row(a.cam_ptr[cam], cam) + tid;
    double t = 0.0;
    for (int s = 0; s < ns; ++s) t += part[(size_t)s * kPcgBlockSums];
    sums[tid] = t;
  }
  __syncthreads();
  if (tid < 7) a.b[7 * (size_t)cam + tid] = sums[28 + tid];
  if (tid == 0) {
    bool bad = false;
    for (int i = 0; i < 7; ++i)
      for (int q = 0; q <= i; ++q) A[i][q] = sums[i * (i + 1) / 2 + q] + (i == q ? a.lambda : 0.0);
    for (int q = 0; q < 7; ++q) {
      const double diag0 = A[q][q];
      double dd = diag0;
      for (int k = 0; k < q; ++k) dd -= A[q][k] * A[q][k];
      if (!(dd > 1e-9 * diag0)) { bad = true; dd = 1.0; }
      const double l = sqrt(dd);
      A[q][q] = l;
      for (int i = q + 1; i < 7; ++i) {
        double v = A[i][q];
        for (int k = 0; k < q; ++k) v -= A[i][k] * A[q][k];
        A[i][q] = v / l;
      }
    }
    for (int c = 0; c < 7; ++c) {                            // column c of L^-1 by forward substitution
      for (int r = 0; r < c; ++r) Li[r][c] = 0.0;
      for (int r = c; r < 7; ++r) {
        double s = r == c ? 1.0 : 0.0;
        for (int m = c; m < r; ++m) s -= A[r][m] * Li[m][c];
        Li[r][c] = s / A[r][r];
      }
    }
    if (bad) atomicMin(&a.st->bad_cam, cam);
  }
  __syncthreads();
  if (tid < 49) {                                            // S^-1 = L^-T L^-1
    const int i = tid / 7, q = tid % 7;
    double s = 0.0;
    for (int k = (i > q ? i : q); k < 7; ++k) s += Li[k][i] * Li[k][q];
    mi[tid] = s;
  }
}

// pass two of q = S p: the 7 sums of Jp^T v over a slice
__global__ __launch_bounds__(256) void pcg_matvec_slices_kernel(PcgDev a) {
  if (a.st->done) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const int cam = a.row_cam[row];
  if (cam < 0 || !a.freec[cam]) return;
  const int e = a.cam_ptr[cam] + (row - (int)cam_slice_first_row(a.cam_ptr[cam], cam)) * kCamSlice + lane;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  if (e < a.cam_ptr[cam + 1]) {
    const int o = a.cam_obs[e];
    const double* j = a.J + kPcgJ * (size_t)o;
    const double v0 = a.v[2 * (size_t)o], v1 = a.v[2 * (size_t)o + 1];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = j[k] * v0 + j[7 + k] * v1;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) acc[k] = group_sum<64>(acc[k]);
  if (lane == 0) {
    double* dst = a.ws + kPcgBlockSums * (size_t)row;
#pragma unroll
    for (int k = 0; k < 7; ++k) dst[k] = acc[k];
  }
}

// ---------------------------------------------------------------------------------------------
// the vectors: one workgroup, eight lanes per camera (lane k < 7 owns element k), cameras t / 8, t / 8 + 128, ...
// ---------------------------------------------------------------------------------------------
// sum over the workgroup, the same value in every thread: a lane's own terms in ascending camera order, a fixed tree per
// wave, the sixteen wave totals in order
__device__ __forceinline__ double pcg_block_sum(double v, double* sh) {
  v = group_sum<64>(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kPcgVecThreads / 64; ++w) t += sh[w];
  __syncthreads();
  return t;
}

// z_k = sum_j Minv[k][j] r_j for the camera the eight lanes share
__device__ __forceinline__ double pcg_apply_minv(const double* mi, double rk, int k) {
  const int base = (threadIdx.x & 63) & ~7;
  double z = 0.0;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const double rj = __shfl(rk, base + j, 64);
    z += (k < 7 ? mi[7 * k + j] : 0.0) * rj;
  }
  return z;
}

__global__ __launch_bounds__(kPcgVecThreads) void pcg_init_kernel(PcgDev a) {
  __shared__ double sh[kPcgVecThreads / 64];
  const int k = threadIdx.x & 7;
  double part = 0.0;
  for (int c0 = 0; c0 < a.V; c0 += kPcgVecThreads / 8) {
    const int c = c0 + (threadIdx.x >> 3);
    const bool live = c < a.V && k < 7;
    const size_t i = live ? 7 * (size_t)c + k : 0;
    const double rk = live ? a.b[i] : 0.0;                   // (a held camera's b and Minv are zeros)
    const double zk = pcg_apply_minv(a.Minv + 49 * (size_t)(c < a.V ? c : 0), rk, k);
    if (live) { a.x[i] = 0.0; a.r[i] = rk; a.z[i] = zk; a.pv[i] = zk; part += rk * zk; }
  }
  const double rz = pcg_block_sum(part, sh);
  if (threadIdx.x != 0) return;
  PcgState* st = a.st;
  st->rz = st->rz0 = rz;
  if (st->bad_cam < a.V) { st->done = 1; st->status = kPcgSingular; }
  else if (rz == 0.0) { st->done = 1; st->status = SFM_PCG_CONVERGED; }
  else if (!(rz > 0.0) || !isfinite(rz)) { st->done = 1; st->status = SFM_PCG_BREAKDOWN; }
  else if (st->max_iters <= 0) { st->done = 1; st->status = SFM_PCG_MAX_ITERS; st->rel = 1.0; }
}

__global__ __launch_bounds__(kPcgVecThreads) void pcg_update_kernel(PcgDev a) {
  __shared__ double sh[kPcgVecThreads / 64];
  PcgState* st = a.st;
  if (st->done) return;                                      // (uniform: nobody has written the flag in this launch yet)
  const int k = threadIdx.x & 7;
  const double rz = st->rz, rz0 = st->rz0, tol2 = st->tol2;
  const int iters = st->iters, max_iters = st->max_iters;
  // q_c = lambda p_c + the slices of the camera in ascending order; q goes to z's place (z is dead until it is formed anew)
  double part = 0.0;
  for (int c0 = 0; c0 < a.V; c0 += kPcgVecThreads / 8) {
    const int c = c0 + (threadIdx.x >> 3);
    if (c >= a.V || k >= 7 || !a.freec[c]) continue;
    const int ns = cam_slice_count(a.cam_ptr[c + 1] - a.cam_ptr[c]);
    const double* wsp = a.ws + kPcgBlockSums * cam_slice_first_row(a.cam_ptr[c], c) + k;
    const size_t i = 7 * (size_t)c + k;
    const double pk = a.pv[i];
    double q = a.lambda * pk;
    for (int s = 0; s < ns; ++s) q += wsp[(size_t)s * kPcgBlockSums];
    a.z[i] = q;
    part += pk * q;
  }
  const double pq = pcg_block_sum(part, sh);
  if (!(pq > 0.0) || !isfinite(pq)) {
    if (threadIdx.x == 0) { st->done = 1; st->status = SFM_PCG_BREAKDOWN; }
    return;
  }
  const double alpha = rz / pq;
  part = 0.0;
  for (int c0 = 0; c0 < a.V; c0 += kPcgVecThreads / 8) {
    const int c = c0 + (threadIdx.x >> 3);
    const bool live = c < a.V && k < 7 && a.freec[c < a.V ? c : 0];
    const size_t i = live ? 7 * (size_t)c + k : 0;
    double rk = 0.0;
    if (live) {
      a.x[i] += alpha * a.pv[i];
      rk = a.r[i] - alpha * a.z[i];
      a.r[i] = rk;
    }
    const double zk = pcg_apply_minv(a.Minv + 49 * (size_t)(c < a.V ? c : 0), rk, k);
    if (live) { a.z[i] = zk; part += rk * zk; }
  }
  const double rz_new = pcg_block_sum(part, sh);
  int done = 0, status = SFM_PCG_CONVERGED;
  if (!isfinite(rz_new) || rz_new < 0.0) { done = 1; status = SFM_PCG_BREAKDOWN; }
  else if (rz_new <= tol2 * rz0) done = 1;
  else if (iters + 1 >= max_iters) { done = 1; status = SFM_PCG_MAX_ITERS; }
  if (!done) {
    const double beta = rz_new / rz;
    for (int c0 = 0; c0 < a.V; c0 += kPcgVecThreads / 8) {
      const int c = c0 + (threadIdx.x >> 3);
      if (c >= a.V || k >= 7 || !a.freec[c]) continue;
      const size_t i = 7 * (size_t)c + k;
      a.pv[i] = a.z[i] + beta * a.pv[i];
    }
  }
  if (threadIdx.x == 0) {
    st->rz = rz_new;
    st->rel = sqrt(rz_new / rz0);
    st->iters = iters + 1;
    st->status = status;
    st->done = done;
  }
}

// cams += dp, q /= |q|, and the prepared camera with the checks of an iteration (ba_back_solve); a held camera's seven
// doubles and its prepared form are never written
__global__ void pcg_update_cams_kernel(BaDev d, int cur, PcgDev a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.V || !a.freec[c]) return;
  double cam[7];
  for (int k = 0; k < 7; ++k) cam[k] = d.cams[7 * (size_t)c + k] + a.x[7 * (size_t)c + k];
  const double nq = sqrt(cam[3] * cam[3] + cam[4] * cam[4] + cam[5] * cam[5] + cam[6] * cam[6]);
  for (int k = 3; k < 7; ++k) cam[k] /= nq;
  for (int k = 0; k < 7; ++k) d.cams[7 * (size_t)c + k] = cam[k];
  CamPrep out;
  const int st = cam_prepare(cam, &out);
  d.prep[cur][c] = out;
  report_status(d.status, st, c);
}

// ---------------------------------------------------------------------------------------------
// the cost of a state, residuals only (sfm_ba_cost; every cost sfm_ba_minimize_pcg compares)
// ---------------------------------------------------------------------------------------------
// G lanes per point, lane l takes observations l, l + G, ... of the track in ascending order; the point's share goes to
// cost_pt[p] and ba_point_cost_reduce_kernel adds the points.  The residual and the loss are those of obs_terms_loss.
template <int G, int LOSS>
__global__ __launch_bounds__(256) void ba_cost_kernel(BaDev d, int cur, LossArg<LOSS> la, double* __restrict__ cost_pt) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pl = t / G;
  const int lane = threadIdx.x % G;
  if (pl >= d.N) return;                                     // whole groups leave together
  const int p = (int)pl;
  const int beg = d.pt_ptr[p], end = d.pt_ptr[p + 1];
  const double X = d.px[p], Y = d.py[p], Z = d.pz[p];
  double s = 0.0;
  for (int o = beg + lane; o < end; o += G) {
    CamPrep c;
    load_cam(c, d.prep[cur] + d.cam_idx[o]);
    double q[3];
    project_cam(c, X, Y, Z, 1.0, q);
    const double iz = rcp_nr(q[2]);
    const double r0 = d.u[o] - q[0] * iz, r1 = d.v[o] - q[1] * iz;
    double e = r0 * r0 + r1 * r1;
    if constexpr (LOSS != SFM_LOSS_NONE) {
      double w, sw, rho;
      loss_eval<LOSS>(e * la.inv_d2, w, sw, rho);
      e = la.d2 * rho;
    }
    s += e;
  }
  s = group_sum<G>(s);
  if (lane == 0) cost_pt[p] = s;
}

// ---------------------------------------------------------------------------------------------
// Levenberg-Marquardt control (sfm_ba_minimize_pcg): the scalars of a trial and its verdict stay on the device
// ---------------------------------------------------------------------------------------------
constexpr int kPcgGtol = 4;          // internal status: the gradient test stopped the trial before the solve
constexpr int kLmMaxWaves = 1024;    // waves of lm_sums (a multiple of four: workgroups of 256)
constexpr int kLmSums = 6;           // ex.D^-1 ex | x.rhs | x.r_cg | |x|^2 | sum |dx_p|^2 | |state|^2

struct LmDev {
  sfm_lm_trial row;                  // the trial just judged: what the host reads
  double lambda, nu;                 // of the next trial
  double cost;                       // F of the state that stands
  double cost_trial;                 // F of the trial state (written by the cost reduction)
  unsigned long long grad_bits;      // the running maximum of lm_grad as the bits of a non-negative double; 0 between trials
  int stop;                          // -1: go on, else SFM_LM_STOP_*
  int accepted_steps;
};

struct LmRule { double lambda_min, lambda_max, ftol, xtol, gtol; };

__global__ void lm_begin_kernel(LmDev* lm, double lambda0) {
  LmDev z = {};
  z.lambda = lambda0; z.nu = 2.0; z.stop = -1;
  *lm = z;
}

// max(|rhs|_inf, |ex|_inf): a maximum of non-negative doubles is the maximum of their bit patterns, in any order.  A NaN
// is kept (its pattern lies above every finite one), so a poisoned linearisation never passes the gradient test.
__device__ __forceinline__ double lm_max_nan(double m, double v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(256) void lm_grad_kernel(PcgDev a, LmDev* lm) {
  const long long T = (long long)gridDim.x * 256, t = (long long)blockIdx.x * 256 + threadIdx.x;
  double m = 0.0;
  for (long long i = t; i < 3LL * a.N; i += T) m = lm_max_nan(m, fabs(a.ex[i]));
  for (long long i = t; i < 7LL * a.V; i += T) m = lm_max_nan(m, fabs(a.b[i]));      // (a held camera's rhs is zero)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = lm_max_nan(m, fabs(__shfl_xor(m, off, 64)));
  if ((threadIdx.x & 63) == 0 && !(m == 0.0)) atomicMax(&lm->grad_bits, (unsigned long long)__double_as_longlong(m));
}

// ... and the gradient test: it sets the CG loop's done flag, so the solve that is enqueued behind it does nothing
__global__ void lm_gtol_kernel(PcgDev a, LmDev* lm, double gtol) {
  PcgState* st = a.st;
  const double g = __longlong_as_double((long long)lm->grad_bits);
  lm->grad_bits = 0;
  sfm_lm_trial row = {};
  row.lambda = lm->lambda; row.cost = lm->cost; row.cost_trial = lm->cost; row.grad_inf = g;
  lm->row = row;
  const bool failed = st->done && st->status != SFM_PCG_CONVERGED;      // a block that does not factor, a breakdown
  if (gtol > 0.0 && g <= gtol && !failed) { st->done = 1; st->status = kPcgGtol; lm->stop = SFM_LM_STOP_GTOL; }
}

// The six sums of a trial, per wave: thread t takes points t, t + T, ... and then camera entries t, t + T, ... in ascending
// order, a wave is a fixed tree; partial[wave][k].  save_cams / save_pts hold the state the trial was linearised at.
__global__ __launch_bounds__(256) void lm_sums_kernel(PcgDev a, const double* __restrict__ save_cams, const double* __restrict__ save_pts,
                                                      double* __restrict__ partial) {
  const long long T = (long long)gridDim.x * 256, t = (long long)blockIdx.x * 256 + threadIdx.x;
  double q[kLmSums] = {0, 0, 0, 0, 0, 0};
  for (long long p = t; p < a.N; p += T) {
    double di[6], ex[3], g[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) di[k] = a.Dinv[6 * (size_t)p + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ex[k] = a.ex[3 * (size_t)p + k];
    sym3_apply(di, ex, g);
    q[0] += ex[0] * g[0] + ex[1] * g[1] + ex[2] * g[2];
    const double* dx = a.dx + 3 * (size_t)p;
    q[4] += dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2];
    const double sx = save_pts[p], sy = save_pts[(size_t)a.N + p], sz = save_pts[2 * (size_t)a.N + p];
    q[5] += sx * sx + sy * sy + sz * sz;
  }
  for (long long i = t; i < 7LL * a.V; i += T) {
    const double x = a.x[i];
    q[1] += x * a.b[i];
    q[2] += x * a.r[i];
    q[3] += x * x;
    q[5] += save_cams[i] * save_cams[i];
  }
#pragma unroll
  for (int k = 0; k < kLmSums; ++k) q[k] = group_sum<64>(q[k]);
  if ((threadIdx.x & 63) == 0) {
    double* dst = partial + kLmSums * (size_t)(t >> 6);
#pragma unroll
    for (int k = 0; k < kLmSums; ++k) dst[k] = q[k];
  }
}

// One wave: the wave totals in order, then the verdict (sfm_hip.h states the rule), the trial's row and the next lambda, nu
__global__ __launch_bounds__(64) void lm_decide_kernel(PcgDev a, LmDev* lm, const double* __restrict__ partial, int waves, LmRule o,
                                                       const int* __restrict__ cam_status) {
  const int lane = threadIdx.x;
  double s = 0.0;
  if (lane < kLmSums) {
    // eight loads in flight, the additions still in wave order: the sum's bits do not depend on the unrolling
    int w = 0;
    for (; w + 8 <= waves; w += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = partial[kLmSums * (size_t)(w + k) + lane];
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; w < waves; ++w) s += partial[kLmSums * (size_t)w + lane];
  }
  double q[kLmSums];
#pragma unroll
  for (int k = 0; k < kLmSums; ++k) q[k] = __shfl(s, k, 64);
  if (lane != 0) return;
  const PcgState* st = a.st;
  const double lambda = lm->lambda, F = lm->cost, Ft = lm->cost_trial;
  const double h2 = q[3] + q[4];
  const double predicted = q[0] + q[1] + q[2] + lambda * h2;
  const double step_norm = sqrt(h2), state_norm = sqrt(q[5]);
  const double rho = (F - Ft) / predicted;
  // (a trial camera that failed its checks is never accepted: the host restores the state and returns its code)
  const bool accepted = cam_status[0] == SFM_OK && predicted > 0.0 && isfinite(Ft) && rho > SFM_LM_MIN_GAIN;
  sfm_lm_trial row = lm->row;                                // (lambda, cost and grad_inf are in it already)
  row.cost_trial = Ft; row.predicted = predicted; row.rho = rho; row.step_norm = step_norm;
  row.cg_rel = st->rel; row.cg_iters = st->iters; row.cg_status = st->status; row.accepted = accepted ? 1 : 0;
  lm->row = row;
  if (accepted) {
    const double f = 2.0 * rho - 1.0;
    lm->lambda = fmax(o.lambda_min, lambda * fmax(1.0 / 3.0, 1.0 - f * f * f));
    lm->nu = 2.0;
    if (o.ftol > 0.0 && F - Ft <= o.ftol * F) lm->stop = SFM_LM_STOP_FTOL;
    else if (o.xtol > 0.0 && step_norm <= o.xtol * (state_norm + o.xtol)) lm->stop = SFM_LM_STOP_XTOL;
    lm->cost = Ft;
    lm->accepted_steps += 1;
  } else {
    const double nu = lm->nu;
    lm->lambda = lambda * nu;
    lm->nu = 2.0 * nu;
    if (lm->lambda > o.lambda_max) lm->stop = SFM_LM_STOP_LAMBDA_MAX;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// `group` = 0: the narrowest width that gives every observation of a mean track a lane
static int pcg_pick_group(int n_pts, long long M) {
  const long long mean = n_pts > 0 ? (M + n_pts - 1) / n_pts : 1;
  return kGroupWidths[narrowest_group([&](int w) { return w >= mean; })];
}

struct PcgWork {
  DevBuf<unsigned char> freec;
  DevBuf<int> row_cam;
  DevBuf<double> J, v, Dinv, ex, cost_pt, ws, Minv, vec, cost, save_cams, save_pts;
  DevBuf<PcgState> st;
};

// What one call of either entry point works with: the buffers, the kernels' argument and the launch widths.
struct PcgRun {
  PcgWork w;
  PcgDev a = {};
  int g = 0, max_cg = 0;
  unsigned row_grid = 0;
};

static void pcg_launch_linearize(sfm_ba_problem* p, const PcgDev& a, int g, int quirks) {
  dispatch_loss(p->loss_kind, [&](auto L) {
    constexpr int LOSS = decltype(L)::value;
    const LossArg<LOSS> la = loss_arg<LOSS>(p);
    dispatch_group<1>(g, [&](auto G) {
      constexpr int kG = decltype(G)::value;
      const long long threads = (long long)a.N * kG;
      pcg_linearize_kernel<kG, LOSS><<<(unsigned)((threads + 255) / 256), 256, 0, p->stream>>>(p->dev, p->cur, a, quirks, la);
    });
  });
}

static void pcg_launch_matvec_points(const PcgDev& a, int g, hipStream_t s) {
  dispatch_group<1>(g, [&](auto G) {
    constexpr int kG = decltype(G)::value;
    const long long threads = (long long)a.N * kG;
    pcg_matvec_points_kernel<kG><<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(a);
  });
}

template <bool KEEP_DX>
static void pcg_launch_backsub(const BaDev& d, const PcgDev& a, int g, hipStream_t s) {
  dispatch_group<1>(g, [&](auto G) {
    constexpr int kG = decltype(G)::value;
    const long long threads = (long long)a.N * kG;
    pcg_backsub_kernel<kG, KEEP_DX><<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(d, a);
  });
}

// the cost of the current state: per point into cost_pt [N], their sum into *out (both device memory)
static int ba_cost_enqueue(sfm_ba_problem* p, int g, double* cost_pt, double* out) {
  const BaDev& d = p->dev;
  dispatch_loss(p->loss_kind, [&](auto L) {
    constexpr int LOSS = decltype(L)::value;
    const LossArg<LOSS> la = loss_arg<LOSS>(p);
    dispatch_group<1>(g, [&](auto G) {
      constexpr int kG = decltype(G)::value;
      const long long threads = (long long)d.N * kG;
      ba_cost_kernel<kG, LOSS><<<(unsigned)((threads + 255) / 256), 256, 0, p->stream>>>(d, p->cur, la, cost_pt);
    });
  });
  ba_point_cost_reduce_kernel<<<1, 256, 0, p->stream>>>(d.N, cost_pt, nullptr, out);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// cameras and points to the save buffers (the state a failed call or a rejected trial goes back to), or back from them
static int pcg_copy_state(sfm_ba_problem* p, PcgRun& run, bool restore) {
  const BaDev& d = p->dev;
  hipStream_t s = p->stream;
  const size_t n = (size_t)d.N, nv = (size_t)d.V;
  double* sc = run.w.save_cams.p;
  double* sp = run.w.save_pts.p;
  if (!restore) {
    SFM_HIP(hipMemcpyAsync(sc, d.cams, sizeof(double) * 7 * nv, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(sp, d.px, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(sp + n, d.py, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(sp + 2 * n, d.pz, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  } else {
    SFM_HIP(hipMemcpyAsync(d.cams, sc, sizeof(double) * 7 * nv, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(d.px, sp, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(d.py, sp + n, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(d.pz, sp + 2 * n, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  }
  return SFM_OK;
}

// The work buffers of a call on a scene with observations, the mask, the state as it came in, the camera of every slice.
// `cost_slots`: linearisation costs the call keeps on the device.
static int pcg_setup(sfm_ba_problem* p, const unsigned char* cam_mask, int group, int max_cg, int cost_slots, PcgRun& run) {
  BaDev& d = p->dev;
  hipStream_t s = p->stream;
  const int V = d.V, N = d.N;
  SFM_TRY(ba_cam_list_ensure(p));
  const size_t n = (size_t)N, m = (size_t)d.M, nv = (size_t)V;
  const int rows = (int)cam_slice_rows(d.M, V);
  run.g = group ? group : pcg_pick_group(N, d.M);
  run.max_cg = max_cg;
  run.row_grid = (unsigned)((rows + 3) / 4);
  PcgWork& w = run.w;
  std::vector<unsigned char> h_free(nv, 1);              // the kernels' flags are 0 / 1 whatever the mask's non-zero values
  for (int c = 0; cam_mask != nullptr && c < V; ++c) h_free[c] = cam_mask[c] != 0;
  SFM_TRY(w.freec.upload(h_free.data(), nv, s));
  p->upload_bytes += V;
  SFM_TRY(w.row_cam.alloc((size_t)rows, s));
  SFM_TRY(w.J.alloc(kPcgJ * m, s)); SFM_TRY(w.v.alloc(2 * m, s));
  SFM_TRY(w.Dinv.alloc(6 * n, s)); SFM_TRY(w.ex.alloc(3 * n, s)); SFM_TRY(w.cost_pt.alloc(n, s));
  SFM_TRY(w.ws.alloc(kPcgBlockSums * (size_t)rows, s));
  SFM_TRY(w.Minv.alloc(49 * nv, s));
  SFM_TRY(w.vec.alloc(5 * 7 * nv, s));                   // b | x | r | z | p
  SFM_TRY(w.cost.alloc((size_t)cost_slots, s));
  SFM_TRY(w.save_cams.alloc(7 * nv, s)); SFM_TRY(w.save_pts.alloc(3 * n, s));
  SFM_TRY(w.st.alloc(1, s));
  // the state as it came in: a block that does not factor in a later outer iteration still leaves the state untouched
  SFM_TRY(pcg_copy_state(p, run, false));
  SFM_HIP(hipMemsetAsync(w.row_cam.p, 0xFF, sizeof(int) * (size_t)rows, s));
  PcgDev& a = run.a;
  a.V = V; a.N = N; a.M = d.M; a.rows = rows; a.lambda = 0.0;
  a.pt_ptr = d.pt_ptr; a.cam_idx = d.cam_idx; a.obs_pt = d.obs_pt; a.cam_ptr = p->cam_ptr; a.cam_obs = p->cam_obs;
  a.freec = w.freec.p; a.row_cam = w.row_cam.p;
  a.J = w.J.p; a.v = w.v.p; a.Dinv = w.Dinv.p; a.ex = w.ex.p; a.cost_pt = w.cost_pt.p; a.ws = w.ws.p; a.Minv = w.Minv.p;
  a.b = w.vec.p; a.x = a.b + 7 * nv; a.r = a.x + 7 * nv; a.z = a.r + 7 * nv; a.pv = a.z + 7 * nv;
  a.dx = nullptr;
  a.st = w.st.p;
  pcg_rows_kernel<<<(V + 255) / 256, 256, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// The first half of an outer iteration at run.a.lambda: the linearisation and its cost (to *cost_out, device), a mark, the
// diagonal blocks and the start of CG; a mark before and behind.
static int pcg_enqueue_system(sfm_ba_problem* p, PcgRun& run, int quirks, double cg_tol, double* cost_out, PhaseEvents& ev) {
  hipStream_t s = p->stream;
  const PcgDev& a = run.a;
  SFM_TRY(ev.mark(s));
  pcg_reset_kernel<<<1, 1, 0, s>>>(a, cg_tol * cg_tol, run.max_cg);
  pcg_launch_linearize(p, a, run.g, quirks);
  ba_point_cost_reduce_kernel<<<1, 256, 0, s>>>(a.N, a.cost_pt, nullptr, cost_out);      // (out[0] only: out[1] is the next iteration's)
  SFM_TRY(ev.mark(s));
  pcg_blocks_kernel<<<run.row_grid, 256, 0, s>>>(a);
  pcg_blocks_finish_kernel<<<a.V, 64, 0, s>>>(a);
  pcg_init_kernel<<<1, kPcgVecThreads, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  SFM_TRY(ev.mark(s));
  return SFM_OK;
}

// The CG loop: chunks of kPcgChunk iterations until the done flag is read as set; *hs is the state then.  *cam_ret: the
// cameras of the previous update failed their checks (the loop ends at once).
static int pcg_run_cg(sfm_ba_problem* p, PcgRun& run, const char* who, const char* when, PcgState* hs, int* cam_ret) {
  hipStream_t s = p->stream;
  const PcgDev& a = run.a;
  for (;;) {
    for (int k = 0; k < kPcgChunk; ++k) {
      pcg_launch_matvec_points(a, run.g, s);
      pcg_matvec_slices_kernel<<<run.row_grid, 256, 0, s>>>(a);
      pcg_update_kernel<<<1, kPcgVecThreads, 0, s>>>(a);
    }
    SFM_HIP(hipGetLastError());
    SFM_HIP(hipMemcpyAsync(hs, a.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    *cam_ret = ba_sync_cam_status(p, who, when);      // (the previous update's cameras)
    if (hs->done || *cam_ret != SFM_OK) return SFM_OK;
  }
}

// The second half: the points' back substitution and the camera update with its checks
template <bool KEEP_DX>
static int pcg_enqueue_step(sfm_ba_problem* p, PcgRun& run) {
  hipStream_t s = p->stream;
  pcg_launch_backsub<KEEP_DX>(p->dev, run.a, run.g, s);
  pcg_update_cams_kernel<<<(run.a.V + 63) / 64, 64, 0, s>>>(p->dev, p->cur, run.a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

static int pcg_max_cg(int cg_max_iters, int v_free) { return cg_max_iters > 0 ? cg_max_iters : std::min(7 * v_free, 1000); }

static int lm_options_check(const sfm_lm_options* o) {
  const char* who = "sfm_ba_minimize_pcg";
  if (o == nullptr) { set_error("%s: opt is null", who); return SFM_E_SHAPE; }
  if (!(std::isfinite(o->lambda_min) && std::isfinite(o->lambda0) && std::isfinite(o->lambda_max) && o->lambda_min > 0 &&
        o->lambda_min <= o->lambda0 && o->lambda0 <= o->lambda_max)) {
    set_error("%s: 0 < lambda_min <= lambda0 <= lambda_max, all finite, is required", who);
    return SFM_E_SHAPE;
  }
  if (!(o->ftol >= 0) || !(o->xtol >= 0) || !(o->gtol >= 0)) { set_error("%s: ftol, xtol and gtol must be >= 0", who); return SFM_E_SHAPE; }
  if (!(o->cg_tol > 0 && o->cg_tol < 1)) { set_error("%s: cg_tol must lie in (0, 1)", who); return SFM_E_SHAPE; }
  if (o->cg_max_iters < 0) { set_error("%s: cg_max_iters < 0", who); return SFM_E_SHAPE; }
  if (o->max_trials < 0) { set_error("%s: max_trials < 0", who); return SFM_E_SHAPE; }
  return group_width_check(who, o->group);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_ba_pcg_times(sfm_ba_problem* p, double* ms) {
  SFM_TRY(ba_check_handle(p));
  if (ms == nullptr) { set_error("sfm_ba_pcg_times: ms is null"); return SFM_E_SHAPE; }
  for (int k = 0; k < 5; ++k) ms[k] = p->pcg_ms[k];
  return SFM_OK;
}

int sfm_ba_iterate_pcg(sfm_ba_problem* p, double lambda, int iters, int quirks, const unsigned char* cam_mask, double cg_tol,
                       int cg_max_iters, int group, int* iters_done, double* cost, int* cg_iters, double* cg_rel, int* cg_status,
                       int* bad_camera) {
  SFM_TRY(ba_check_handle(p));
  if (iters < 0) { set_error("sfm_ba_iterate_pcg: iters < 0"); return SFM_E_SHAPE; }
  if (!(lambda >= 0) || !std::isfinite(lambda)) { set_error("sfm_ba_iterate_pcg: lambda must be finite and >= 0"); return SFM_E_SHAPE; }
  if (!(cg_tol > 0 && cg_tol < 1)) { set_error("sfm_ba_iterate_pcg: cg_tol must lie in (0, 1)"); return SFM_E_SHAPE; }
  if (cg_max_iters < 0) { set_error("sfm_ba_iterate_pcg: cg_max_iters < 0"); return SFM_E_SHAPE; }
  SFM_TRY(group_width_check("sfm_ba_iterate_pcg", group));
  SFM_TRY(ba_refuse_comm(p, "sfm_ba_iterate_pcg", "the points are sharded; the replicas would diverge"));
  const auto wall0 = std::chrono::steady_clock::now();
  if (iters_done) *iters_done = 0;
  if (iters == 0) return SFM_OK;
  BaDev& d = p->dev;
  const int V = d.V, N = d.N;
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  hipStream_t s = p->stream;
  SFM_TRY(ba_prepared_cameras(p, "sfm_ba_iterate_pcg"));
  int v_free = 0, first_free = -1;
  ba_free_cameras(cam_mask, V, &v_free, &first_free);
  for (int k = 0; k < 5; ++k) p->pcg_ms[k] = 0.f;
  p->pcg_held_points = 0;
  if (N == 0 || d.M == 0) {                              // nothing is observed: S = lambda I, rhs = 0, dp = 0
    if (v_free > 0 && !(lambda > 0)) {
      if (bad_camera) *bad_camera = first_free;
      set_error("sfm_ba_iterate_pcg: the diagonal block of camera %d does not factor (no observations, lambda = 0)", first_free);
      return SFM_E_SINGULAR;
    }
    for (int it = 0; it < iters; ++it) {
      if (cost) cost[it] = 0.0;
      if (cg_iters) cg_iters[it] = 0;
      if (cg_rel) cg_rel[it] = 0.0;
      if (cg_status) cg_status[it] = SFM_PCG_CONVERGED;
    }
    if (iters_done) *iters_done = iters;
    return SFM_OK;
  }
  PcgRun run;
  SFM_TRY(pcg_setup(p, cam_mask, group, pcg_max_cg(cg_max_iters, v_free), iters, run));
  PcgWork& w = run.w;
  run.a.lambda = lambda;
  // SFM_OPT_TIMING (any bit): hipEvents around the four parts of every outer iteration, read back by sfm_ba_pcg_times
  PhaseEvents ev(p->timing != 0);
  std::vector<int> h_cg((size_t)iters, 0), h_status((size_t)iters, 0);
  std::vector<double> h_rel((size_t)iters, 0.0);
  int done_iters = 0, ret = SFM_OK, bad_cam = -1, held_pts = 0;
  for (int it = 0; it < iters; ++it) {
    SFM_TRY(pcg_enqueue_system(p, run, quirks, cg_tol, w.cost.p + it, ev));
    PcgState hs = {};
    int cam_ret = SFM_OK;
    char when[48];
    std::snprintf(when, sizeof(when), " after iteration %d", it);
    SFM_TRY(pcg_run_cg(p, run, "sfm_ba_iterate_pcg", when, &hs, &cam_ret));
    SFM_TRY(ev.mark(s));
    if (cam_ret != SFM_OK) {                             // the previous update produced a camera that fails its checks
      ret = cam_ret;
      SFM_TRY(ev.mark(s));
      break;
    }
    if (hs.status == kPcgSingular) {
      bad_cam = hs.bad_cam;
      ret = SFM_E_SINGULAR;
      SFM_TRY(ev.mark(s));
      break;
    }
    held_pts = hs.bad_pts;
    h_cg[it] = hs.iters; h_rel[it] = hs.rel; h_status[it] = hs.status;
    done_iters = it + 1;
    if (hs.status == SFM_PCG_BREAKDOWN) {                // nothing of this outer iteration is applied
      SFM_TRY(ev.mark(s));
      break;
    }
    SFM_TRY(pcg_enqueue_step<false>(p, run));
    SFM_TRY(ev.mark(s));
  }
  if (ret == SFM_E_SINGULAR) {
    SFM_TRY(pcg_copy_state(p, run, true));
    if (done_iters > 0) p->prep_valid = false;           // (the first iteration wrote nothing: the prepared cameras still hold)
    SFM_TRY(stream_sync(s));
    if (bad_camera) *bad_camera = bad_cam;
    set_error("sfm_ba_iterate_pcg: the diagonal block of camera %d does not factor (hold it, or use lambda > 0)", bad_cam);
    return SFM_E_SINGULAR;
  }
  SFM_TRY(ba_state_changed(p));                          // new cameras and points
  if (cost && done_iters > 0) SFM_TRY(w.cost.download(cost, (size_t)done_iters, s));
  if (ret == SFM_OK) ret = ba_sync_cam_status(p, "sfm_ba_iterate_pcg", " after the last iteration");
  else SFM_TRY(stream_sync(s));                          // (its message stands)
  for (int it = 0; it < done_iters; ++it) {
    if (cg_iters) cg_iters[it] = h_cg[it];
    if (cg_rel) cg_rel[it] = h_rel[it];
    if (cg_status) cg_status[it] = h_status[it];
  }
  if (iters_done) *iters_done = done_iters;
  p->pcg_held_points = held_pts;
  for (int k = 0; k + 4 < ev.marks(); k += 5)             // five marks per outer iteration
    for (int q = 0; q < 4; ++q) p->pcg_ms[q] += ev.elapsed_ms(k + q);
  p->pcg_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  return ret;
}

int sfm_ba_cost(sfm_ba_problem* p, int quirks, int group, double* cost) {
  (void)quirks;                                          // no bit of it changes a residual
  SFM_TRY(ba_check_handle(p));
  if (cost == nullptr) { set_error("sfm_ba_cost: cost is null"); return SFM_E_SHAPE; }
  SFM_TRY(group_width_check("sfm_ba_cost", group));
  SFM_TRY(ba_refuse_comm(p, "sfm_ba_cost", "the points are sharded; the value would be this rank's share"));
  const BaDev& d = p->dev;
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  hipStream_t s = p->stream;
  SFM_TRY(ba_prepared_cameras(p, "sfm_ba_cost"));
  *cost = 0.0;
  if (d.N == 0 || d.M == 0) return SFM_OK;
  DevBuf<double> cost_pt, out;
  SFM_TRY(cost_pt.alloc((size_t)d.N, s));
  SFM_TRY(out.alloc(1, s));
  SFM_TRY(ba_cost_enqueue(p, group ? group : pcg_pick_group(d.N, d.M), cost_pt.p, out.p));
  SFM_TRY(out.download(cost, 1, s));
  return stream_sync(s);
}

int sfm_lm_options_default(sfm_lm_options* opt) {
  if (opt == nullptr) return 0;
  sfm_lm_options o = {};
  o.lambda0 = 5.0; o.lambda_min = 1e-8; o.lambda_max = 1e8;
  o.ftol = 1e-8; o.xtol = 0.0; o.gtol = 0.0;
  o.cg_tol = 1e-10; o.cg_max_iters = 0;
  o.max_trials = 50;
  o.quirks = SFM_QUIRKS_REFERENCE; o.group = 0;
  *opt = o;
  return (int)sizeof(sfm_lm_options);
}

int sfm_lm_trial_size(void) { return (int)sizeof(sfm_lm_trial); }

int sfm_ba_minimize_pcg(sfm_ba_problem* p, const sfm_lm_options* opt, const unsigned char* cam_mask, sfm_lm_trial* log,
                        int* trials_done, int* accepted_steps, int* stop_reason, double* lambda_out, double* cost_out,
                        int* bad_camera) {
  const char* who = "sfm_ba_minimize_pcg";
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(lm_options_check(opt));
  SFM_TRY(ba_refuse_comm(p, who, "the points are sharded; the replicas would diverge"));
  const auto wall0 = std::chrono::steady_clock::now();
  const sfm_lm_options o = *opt;
  if (trials_done) *trials_done = 0;
  if (accepted_steps) *accepted_steps = 0;
  if (stop_reason) *stop_reason = SFM_LM_STOP_MAX_TRIALS;
  if (lambda_out) *lambda_out = o.lambda0;
  if (cost_out) *cost_out = 0.0;
  if (bad_camera) *bad_camera = -1;
  BaDev& d = p->dev;
  const int V = d.V, N = d.N;
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  hipStream_t s = p->stream;
  SFM_TRY(ba_prepared_cameras(p, who));
  if (N == 0 || d.M == 0) return SFM_OK;                 // nothing is observed: the cost is 0 and there is no trial to make
  double F = 0.0;
  if (o.max_trials == 0) {
    SFM_TRY(sfm_ba_cost(p, o.quirks, o.group, &F));
    if (cost_out) *cost_out = F;
    return SFM_OK;
  }
  int v_free = 0, first_free = -1;
  ba_free_cameras(cam_mask, V, &v_free, &first_free);
  for (int k = 0; k < 5; ++k) p->pcg_ms[k] = 0.f;
  p->pcg_held_points = 0;
  PcgRun run;
  SFM_TRY(pcg_setup(p, cam_mask, o.group, pcg_max_cg(o.cg_max_iters, v_free), 1, run));
  PcgWork& w = run.w;
  PcgDev& a = run.a;
  const size_t n = (size_t)N, nv = (size_t)V;
  const int waves = std::min(kLmMaxWaves, (int)((std::max<long long>(N, 7LL * V) + 255) / 256) * 4);
  DevBuf<double> dx, partial;
  DevBuf<CamPrep> save_prep;
  DevBuf<LmDev> lmb;
  SFM_TRY(dx.alloc(3 * n, s));
  SFM_TRY(partial.alloc(kLmSums * (size_t)waves, s));
  SFM_TRY(save_prep.alloc(nv, s));
  SFM_TRY(lmb.alloc(1, s));
  SFM_HIP(hipMemsetAsync(dx.p, 0, sizeof(double) * 3 * n, s));      // (a point without observations is never written)
  a.dx = dx.p;
  LmDev* lm = lmb.p;
  const LmRule rule = {o.lambda_min, o.lambda_max, o.ftol, o.xtol, o.gtol};
  const int cur = p->cur;
  const unsigned grad_grid = (unsigned)std::min<long long>(256, (std::max<long long>(3LL * N, 7LL * V) + 255) / 256);
  lm_begin_kernel<<<1, 1, 0, s>>>(lm, o.lambda0);
  SFM_TRY(ba_cost_enqueue(p, run.g, a.cost_pt, &lm->cost));
  PhaseEvents ev(false);
  std::vector<sfm_lm_trial> rows;
  LmDev h = {};
  h.lambda = o.lambda0; h.stop = -1;
  int stop = SFM_LM_STOP_MAX_TRIALS, ret = SFM_OK, bad_cam = -1, held_pts = 0;
  bool moved = false;                                    // a trial state was written (whether it stood or not)
  for (int trial = 0; trial < o.max_trials; ++trial) {
    a.lambda = h.lambda;
    SFM_TRY(pcg_enqueue_system(p, run, o.quirks, o.cg_tol, w.cost.p, ev));
    lm_grad_kernel<<<grad_grid, 256, 0, s>>>(a, lm);
    lm_gtol_kernel<<<1, 1, 0, s>>>(a, lm, o.gtol);
    PcgState hs = {};
    int cam_ret = SFM_OK;
    char when[48];
    std::snprintf(when, sizeof(when), " before trial %d", trial);
    SFM_TRY(pcg_run_cg(p, run, who, when, &hs, &cam_ret));
    if (cam_ret != SFM_OK) { ret = cam_ret; break; }     // (cannot arise: every trial's cameras are checked below)
    if (hs.status == kPcgSingular) { bad_cam = hs.bad_cam; stop = SFM_LM_STOP_SINGULAR; break; }
    if (hs.status == SFM_PCG_BREAKDOWN) { stop = SFM_LM_STOP_BREAKDOWN; break; }
    held_pts = hs.bad_pts;
    if (hs.status == kPcgGtol) {                         // the row holds lambda, the cost and grad_inf
      SFM_HIP(hipMemcpyAsync(&h, lm, sizeof(h), hipMemcpyDeviceToHost, s));
      SFM_TRY(stream_sync(s));
      rows.push_back(h.row);
      stop = SFM_LM_STOP_GTOL;
      break;
    }
    // the state the trial starts from, its prepared cameras included; then the step, its cost and the verdict
    SFM_TRY(pcg_copy_state(p, run, false));
    SFM_HIP(hipMemcpyAsync(save_prep.p, d.prep[cur], sizeof(CamPrep) * nv, hipMemcpyDeviceToDevice, s));
    SFM_TRY(pcg_enqueue_step<true>(p, run));
    moved = true;
    SFM_TRY(ba_cost_enqueue(p, run.g, a.cost_pt, &lm->cost_trial));
    lm_sums_kernel<<<waves / 4, 256, 0, s>>>(a, w.save_cams.p, w.save_pts.p, partial.p);
    lm_decide_kernel<<<1, 64, 0, s>>>(a, lm, partial.p, waves, rule, d.status);
    SFM_HIP(hipGetLastError());
    SFM_HIP(hipMemcpyAsync(&h, lm, sizeof(h), hipMemcpyDeviceToHost, s));
    std::snprintf(when, sizeof(when), " in trial %d", trial);
    cam_ret = ba_sync_cam_status(p, who, when);
    if (cam_ret != SFM_OK || !h.row.accepted) {
      SFM_TRY(pcg_copy_state(p, run, true));
      SFM_HIP(hipMemcpyAsync(d.prep[cur], save_prep.p, sizeof(CamPrep) * nv, hipMemcpyDeviceToDevice, s));
    }
    if (cam_ret != SFM_OK) {                             // a trial camera failed its checks: the restored state is valid again
      SFM_HIP(hipMemsetAsync(d.status, 0, 2 * sizeof(int), s));
      ret = cam_ret;
      break;
    }
    rows.push_back(h.row);
    if (h.stop >= 0) { stop = h.stop; break; }
  }
  if (moved) SFM_TRY(ba_state_changed(p));               // as after sfm_ba_iterate_pcg
  // what the device carries: the cost of the state that stands (a refused trial leaves it at the last accepted one) and
  // the damping of the next trial
  LmDev last = {};
  SFM_HIP(hipMemcpyAsync(&last, lm, sizeof(last), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  for (size_t i = 0; log != nullptr && i < rows.size(); ++i) log[i] = rows[i];
  if (trials_done) *trials_done = (int)rows.size();
  if (accepted_steps) *accepted_steps = last.accepted_steps;
  if (stop_reason) *stop_reason = stop;
  if (lambda_out) *lambda_out = last.lambda;
  if (cost_out) *cost_out = last.cost;
  if (bad_camera) *bad_camera = bad_cam;
  p->pcg_held_points = held_pts;
  p->pcg_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  return ret;
}

}  // extern "C"
