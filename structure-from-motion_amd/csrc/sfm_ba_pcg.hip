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

// pts += D^-1 (ex - sum_o W_o^T dp_c)
template <int G>
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

static void pcg_launch_backsub(const BaDev& d, const PcgDev& a, int g, hipStream_t s) {
  dispatch_group<1>(g, [&](auto G) {
    constexpr int kG = decltype(G)::value;
    const long long threads = (long long)a.N * kG;
    pcg_backsub_kernel<kG><<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(d, a);
  });
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
  const int max_cg = cg_max_iters > 0 ? cg_max_iters : std::min(7 * v_free, 1000);
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
  SFM_TRY(ba_cam_list_ensure(p));
  const size_t n = (size_t)N, m = (size_t)d.M, nv = (size_t)V;
  const int rows = (int)cam_slice_rows(d.M, V);
  const int g = group ? group : pcg_pick_group(N, d.M);
  PcgWork w;
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
  SFM_TRY(w.cost.alloc((size_t)iters, s));
  SFM_TRY(w.save_cams.alloc(7 * nv, s)); SFM_TRY(w.save_pts.alloc(3 * n, s));
  SFM_TRY(w.st.alloc(1, s));
  // the state as it came in: a block that does not factor in a later outer iteration still leaves the state untouched
  SFM_HIP(hipMemcpyAsync(w.save_cams.p, d.cams, sizeof(double) * 7 * nv, hipMemcpyDeviceToDevice, s));
  SFM_HIP(hipMemcpyAsync(w.save_pts.p, d.px, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  SFM_HIP(hipMemcpyAsync(w.save_pts.p + n, d.py, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  SFM_HIP(hipMemcpyAsync(w.save_pts.p + 2 * n, d.pz, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  SFM_HIP(hipMemsetAsync(w.row_cam.p, 0xFF, sizeof(int) * (size_t)rows, s));
  PcgDev a = {};
  a.V = V; a.N = N; a.M = d.M; a.rows = rows; a.lambda = lambda;
  a.pt_ptr = d.pt_ptr; a.cam_idx = d.cam_idx; a.obs_pt = d.obs_pt; a.cam_ptr = p->cam_ptr; a.cam_obs = p->cam_obs;
  a.freec = w.freec.p; a.row_cam = w.row_cam.p;
  a.J = w.J.p; a.v = w.v.p; a.Dinv = w.Dinv.p; a.ex = w.ex.p; a.cost_pt = w.cost_pt.p; a.ws = w.ws.p; a.Minv = w.Minv.p;
  a.b = w.vec.p; a.x = a.b + 7 * nv; a.r = a.x + 7 * nv; a.z = a.r + 7 * nv; a.pv = a.z + 7 * nv;
  a.st = w.st.p;
  pcg_rows_kernel<<<(V + 255) / 256, 256, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  // SFM_OPT_TIMING (any bit): hipEvents around the four parts of every outer iteration, read back by sfm_ba_pcg_times
  PhaseEvents ev(p->timing != 0);
  const unsigned row_grid = (unsigned)((rows + 3) / 4);
  const int cur = p->cur;
  std::vector<int> h_cg((size_t)iters, 0), h_status((size_t)iters, 0);
  std::vector<double> h_rel((size_t)iters, 0.0);
  int done_iters = 0, ret = SFM_OK, bad_cam = -1, held_pts = 0;
  for (int it = 0; it < iters; ++it) {
    SFM_TRY(ev.mark(s));
    pcg_reset_kernel<<<1, 1, 0, s>>>(a, cg_tol * cg_tol, max_cg);
    pcg_launch_linearize(p, a, g, quirks);
    ba_point_cost_reduce_kernel<<<1, 256, 0, s>>>(N, a.cost_pt, nullptr, w.cost.p + it);      // (out[0] only: out[1] is the next iteration's)
    SFM_TRY(ev.mark(s));
    pcg_blocks_kernel<<<row_grid, 256, 0, s>>>(a);
    pcg_blocks_finish_kernel<<<V, 64, 0, s>>>(a);
    pcg_init_kernel<<<1, kPcgVecThreads, 0, s>>>(a);
    SFM_HIP(hipGetLastError());
    SFM_TRY(ev.mark(s));
    PcgState hs = {};
    int cam_ret = SFM_OK;
    char when[48];
    std::snprintf(when, sizeof(when), " after iteration %d", it);
    for (;;) {
      for (int k = 0; k < kPcgChunk; ++k) {
        pcg_launch_matvec_points(a, g, s);
        pcg_matvec_slices_kernel<<<row_grid, 256, 0, s>>>(a);
        pcg_update_kernel<<<1, kPcgVecThreads, 0, s>>>(a);
      }
      SFM_HIP(hipGetLastError());
      SFM_HIP(hipMemcpyAsync(&hs, a.st, sizeof(hs), hipMemcpyDeviceToHost, s));
      cam_ret = ba_sync_cam_status(p, "sfm_ba_iterate_pcg", when);      // (the previous update's cameras)
      if (hs.done || cam_ret != SFM_OK) break;
    }
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
    pcg_launch_backsub(d, a, g, s);
    pcg_update_cams_kernel<<<(V + 63) / 64, 64, 0, s>>>(d, cur, a);
    SFM_HIP(hipGetLastError());
    SFM_TRY(ev.mark(s));
  }
  if (ret == SFM_E_SINGULAR) {
    SFM_HIP(hipMemcpyAsync(d.cams, w.save_cams.p, sizeof(double) * 7 * nv, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(d.px, w.save_pts.p, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(d.py, w.save_pts.p + n, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(d.pz, w.save_pts.p + 2 * n, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
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

}  // extern "C"
