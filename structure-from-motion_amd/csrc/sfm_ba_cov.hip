// sfm_ba_cov.hip — covariance of the resident bundle-adjustment scene: per-camera and per-point blocks
// (sfm_ba_covariance; gfx950).
//
// With H = J^T J + lambda I = [A B; B^T D] at the current state (the weighted blocks under a loss), cameras with
// cam_mask[c] == 0 held (no unknowns: their rows and columns leave the system):
//   Sigma_cc = inv(S_ff),  S = A - B D^-1 B^T                                       (7x7 diagonal blocks returned)
//   Sigma_pp = D_p^-1 + sum_{o, o' in track(p)} Y_o^T Sigma_{c(o) c(o')} Y_o',  Y_o = W_o D_p^-1        (3x3 per point)
// The call is self-contained: it reads the state, the prepared cameras and the CSR, and works in buffers of its own --
// nothing an iteration owns (red, Z, Zd, lin_ws, xinv, flow) is touched, so an iteration after it launches what it would
// have launched without it.
//
//   cov_rows            free / held / padding rows of the P' x P' system (P' = 7V rounded up to 64): the identity's
//   cov_point_terms     one thread per point: D_p^-1, and per observation W_o, Y_o; the point's cost share
//   cov_build_s         one workgroup per block (c, c') of S, c' <= c: the points both cameras see, in ascending order
//   cov_chol_diag / _panel / _update   right-looking blocked Cholesky, 64 x 64 blocks, three launches per block column
//   cov_trinv_row       X = L^-1, one launch per block row
//   cov_product         Sigma = X^T X, both triangles, held and padding rows zeroed
//   cov_points<G>       the hot path: G lanes per point (tracks up to 64), cov_points_block beyond
//   ba_point_cost_reduce  cost and observed-point count, one workgroup, fixed order (sfm_ba_terms.h)
//
// Fixed summation order everywhere, no floating-point atomic: every element of S, L, X and Sigma is summed by one thread
// in ascending k; a point's six sums are the leaves of ONE balanced binary tree over 64 row slots whatever the group
// width (cov_points) -- so two calls return the same bits, and a point's bits do not depend on `group`.
#include <algorithm>
#include <vector>

#include "sfm_ba.h"
#include "sfm_ba_terms.h"

namespace sfm {

constexpr int kCovNB = 64;            // block size of the dense inverse
constexpr int kCovKC = 16;            // k-chunk of the tile products
constexpr int kCovGroupMax = 64;      // longest track a lane group takes; beyond it one workgroup per point
constexpr int kCovPtBlock = 128;      // threads per workgroup of cov_points
constexpr int kCovSlots = 2;          // observations per lane whose Y is staged in LDS (a track of up to 2 G)

// ---------------------------------------------------------------------------------------------
// rows of the system
// ---------------------------------------------------------------------------------------------
__global__ void cov_rows_kernel(int P, int Pp, const unsigned char* __restrict__ mask, unsigned char* __restrict__ rowfree,
                                double* __restrict__ S) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Pp) return;
  const bool fr = r < P && (mask == nullptr || mask[r / 7] != 0);
  rowfree[r] = fr ? 1 : 0;
  if (!fr) S[(size_t)r * Pp + r] = 1.0;      // S was cleared: a held or padding row is the identity's
}

__global__ void cov_diag_kernel(int Pp, const double* __restrict__ S, double* __restrict__ diag0) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < Pp) diag0[r] = S[(size_t)r * Pp + r];
}

// ---------------------------------------------------------------------------------------------
// per point: D^-1 (packed xx, xy, xz, yy, yz, zz), W_o = Jp^T Jx and Y_o = W_o D^-1 ([7][3], element 3 i + k)
// pt_status: SFM_COV_PT_EMPTY, SFM_COV_PT_SINGULAR (D is not positive definite: D^-1, W and Y are written as zeros, and
// cov_build_s leaves the point's observations out of U as well)
// ---------------------------------------------------------------------------------------------
template <int LOSS>
__global__ void cov_point_terms_kernel(BaDev d, int cur, double lambda, int quirks, LossArg<LOSS> la, double* __restrict__ Dinv,
                                       double* __restrict__ W, double* __restrict__ Y, double* __restrict__ cost_pt,
                                       int* __restrict__ pt_status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= d.N) return;
  const int beg = d.pt_ptr[p], end = d.pt_ptr[p + 1];
  const double X0 = d.px[p], X1 = d.py[p], X2 = d.pz[p];
  double v[6] = {0, 0, 0, 0, 0, 0}, cost = 0;
  for (int o = beg; o < end; ++o) {
    CamPrep c;
    load_cam(c, d.prep[cur] + d.cam_idx[o]);
    double r[2], Jp[14], Jx[6], rho = 0;
    obs_terms_loss<LOSS>(c, X0, X1, X2, d.u[o], d.v[o], quirks, la, r, Jp, Jx, rho);
    if constexpr (LOSS == SFM_LOSS_NONE) rho = r[0] * r[0] + r[1] * r[1];
    cost += rho;
    v[0] += Jx[0] * Jx[0] + Jx[3] * Jx[3];
    v[1] += Jx[0] * Jx[1] + Jx[3] * Jx[4];
    v[2] += Jx[0] * Jx[2] + Jx[3] * Jx[5];
    v[3] += Jx[1] * Jx[1] + Jx[4] * Jx[4];
    v[4] += Jx[1] * Jx[2] + Jx[4] * Jx[5];
    v[5] += Jx[2] * Jx[2] + Jx[5] * Jx[5];
  }
  cost_pt[p] = cost;
  // Cholesky of D = V + lambda I and D^-1 = L^-T L^-1
  const double a00 = v[0] + lambda, a10 = v[1], a20 = v[2], a11 = v[3] + lambda, a21 = v[4], a22 = v[5] + lambda;
  int st = end == beg ? SFM_COV_PT_EMPTY : 0;
  double di[6] = {0, 0, 0, 0, 0, 0};
  bool ok = end > beg && a00 > 0.0;
  if (ok) {
    const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
    const double d1 = a11 - l10 * l10;
    ok = d1 > 0.0;
    if (ok) {
      const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
      const double d2 = a22 - l20 * l20 - l21 * l21;
      ok = d2 > kPtPivotTol * a22;
      if (ok) {
        const double l22 = sqrt(d2);
        const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
        const double i10 = -l10 * i00 * i11;
        const double i21 = -l21 * i11 * i22;
        const double li[6] = {i00, i10, i11, -(l20 * i00 + l21 * i10) * i22, i21, i22};
        sym3_from_li(li, di);
      }
    }
  }
  if (!ok && end > beg) st |= SFM_COV_PT_SINGULAR;
  ok = sym3_finite_or_zero(ok, di);
#pragma unroll
  for (int k = 0; k < 6; ++k) Dinv[6 * (size_t)p + k] = di[k];
  pt_status[p] = st;
  for (int o = beg; o < end; ++o) {
    CamPrep c;
    load_cam(c, d.prep[cur] + d.cam_idx[o]);
    double r[2], Jp[14], Jx[6], rho = 0;
    obs_terms_loss<LOSS>(c, X0, X1, X2, d.u[o], d.v[o], quirks, la, r, Jp, Jx, rho);
    double* w = W + 21 * (size_t)o;
    double* y = Y + 21 * (size_t)o;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      double wi[3], yi[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) wi[k] = ok ? Jp[i] * Jx[k] + Jp[7 + i] * Jx[3 + k] : 0.0;
      sym3_apply(di, wi, yi);
#pragma unroll
      for (int k = 0; k < 3; ++k) { w[3 * i + k] = wi[k]; y[3 * i + k] = yi[k]; }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// S, one workgroup per block (c, c2), c2 <= c, of two free cameras:  [c == c2] (U_c + lambda I) - sum_p Y_{p,c} W_{p,c2}^T
// over the points both see.  Thread t takes entries t, t + 256, ... of camera c's list (ascending point), finds the
// point's observation in c2 by bisection of its track (sorted by camera) and keeps its own 49 sums; the 256 partial
// blocks go through a wave tree and the four wave totals are added in order.
// ---------------------------------------------------------------------------------------------
template <int LOSS>
__global__ __launch_bounds__(256) void cov_build_s_kernel(BaDev d, int cur, double lambda, int quirks, LossArg<LOSS> la,
                                                          const int* __restrict__ cam_ptr, const int* __restrict__ cam_obs,
                                                          const unsigned char* __restrict__ mask, const double* __restrict__ W,
                                                          const double* __restrict__ Y, const int* __restrict__ pt_status,
                                                          double* __restrict__ S, int Pp) {
  __shared__ double part[4][49];
  const int tid = threadIdx.x;
  // workgroup b = block (c, c2) of the lower triangle, row-major: c (c + 1) / 2 + c2
  int c = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((long long)c * (c + 1) / 2 > (long long)blockIdx.x) --c;
  while ((long long)(c + 1) * (c + 2) / 2 <= (long long)blockIdx.x) ++c;
  const int c2 = (int)((long long)blockIdx.x - (long long)c * (c + 1) / 2);
  if (mask != nullptr && (mask[c] == 0 || mask[c2] == 0)) return;
  double acc[49];
#pragma unroll
  for (int k = 0; k < 49; ++k) acc[k] = 0;
  CamPrep cp;
  if (c2 == c) load_cam(cp, d.prep[cur] + c);
  for (int e = cam_ptr[c] + tid; e < cam_ptr[c + 1]; e += 256) {
    const int o = cam_obs[e];
    int o2 = o;
    if (c2 != c) {
      int lo = d.pt_ptr[d.obs_pt[o]], hi = o;                // c2 < c: its observation, if any, lies in [first of the track, o)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d.cam_idx[mid] < c2) lo = mid + 1; else hi = mid;
      }
      if (lo >= o || d.cam_idx[lo] != c2) continue;
      o2 = lo;
    }
    double y[21], w[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) { y[k] = Y[21 * (size_t)o + k]; w[k] = W[21 * (size_t)o2 + k]; }
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 7; ++j) acc[7 * i + j] -= y[3 * i] * w[3 * j] + y[3 * i + 1] * w[3 * j + 1] + y[3 * i + 2] * w[3 * j + 2];
    // A point whose D_p is singular (SFM_COV_PT_SINGULAR; W and Y are zero) is left out of S altogether, U included: for one
    // observation Jx (Jx^T Jx + lambda I)^-1 Jx^T -> I_2 as lambda -> 0, so Jp^T (I - ...) Jp -> 0, the observation says
    // nothing about its camera.  Keeping its Jp^T Jp would treat the point as a known constant.
    if (c2 == c && !(pt_status[d.obs_pt[o]] & SFM_COV_PT_SINGULAR)) {
      const int p = d.obs_pt[o];
      double r[2], Jp[14], Jx[6], rho = 0;
      obs_terms_loss<LOSS>(cp, d.px[p], d.py[p], d.pz[p], d.u[o], d.v[o], quirks, la, r, Jp, Jx, rho);
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) acc[7 * i + j] += Jp[i] * Jp[j] + Jp[7 + i] * Jp[7 + j];
    }
  }
#pragma unroll
  for (int k = 0; k < 49; ++k) acc[k] = group_sum<64>(acc[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 49; ++k) part[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < 49) {
    const int i = tid / 7, j = tid % 7;
    double v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (c2 == c && i == j) v += lambda;
    S[(size_t)(7 * c + i) * Pp + 7 * c2 + j] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Dense FP64 inverse of the P' x P' SPD system (lower triangle, row-major, pitch P'), 64 x 64 blocks, 256 threads,
// a 4 x 4 micro-tile per thread; every sum runs over ascending k in one thread.
// ---------------------------------------------------------------------------------------------
// acc[i][j] += sum_{k in [k0, k1)} a(4 ty + i, k) b(k, 4 tx + j); k1 - k0 a multiple of kCovKC
template <class FA, class FB>
__device__ __forceinline__ void cov_tile_mm(double (&acc)[4][4], int k0, int k1, FA a, FB b, double (*As)[kCovNB + 1],
                                            double (*Bs)[kCovNB + 1]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int kb = k0; kb < k1; kb += kCovKC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, kk = idx & (kCovKC - 1), rc = idx >> 4;
      As[kk][rc] = a(rc, kb + kk);
      Bs[kk][rc] = b(kb + kk, rc);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kCovKC; ++kk) {
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { av[q] = As[kk][4 * ty + q]; bv[q] = Bs[kk][4 * tx + q]; }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[q][s] += av[q] * bv[s];
    }
  }
}

// Block column k, first half (one workgroup): the diagonal block A[k][k] = L L^T in LDS, then L^-1 by forward substitution;
// both are stored.  A pivot that is not above tol x its original diagonal entry counts as non-positive: the first such row
// goes to status[0..1] (code 1, row), the pivot is replaced by 1 and the factorisation runs to its end (the host
// discards the result).
__global__ __launch_bounds__(256) void cov_chol_diag_kernel(double* __restrict__ S, int Pp, int k, const double* __restrict__ diag0,
                                                            double tol, double* __restrict__ dinv, int* __restrict__ status) {
  __shared__ double Ls[kCovNB][kCovNB + 1];      // L in the lower triangle; L^-1 (r >= c) transposed above it, at [c][r + 1]
  const int tid = threadIdx.x;
  double* Akk = S + ((size_t)k * kCovNB) * Pp + (size_t)k * kCovNB;
  for (int idx = tid; idx < kCovNB * kCovNB; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    if (c <= r) Ls[r][c] = Akk[(size_t)r * Pp + c];
  }
  __syncthreads();
  const int ur = tid >> 2, uq = tid & 3;          // trailing update: row ur, columns uq, uq + 4, ...
#pragma unroll 1
  for (int j = 0; j < kCovNB; ++j) {
    double piv = Ls[j][j];                                  // (every thread reads it before anyone scales the column)
    const bool bad = !(piv > tol * diag0[k * kCovNB + j]);
    if (bad) {
      piv = 1.0;
      if (tid == 0 && status[0] == 0) { status[0] = 1; status[1] = k * kCovNB + j; }
    }
    const double il = 1.0 / sqrt(piv);
    __syncthreads();
    if (tid < kCovNB) {
      if (tid == j) Ls[j][j] = piv * il;
      else if (tid > j) Ls[tid][j] *= il;
    }
    __syncthreads();
    if (ur > j) {
      const double lr = Ls[ur][j];
#pragma unroll 1
      for (int c = j + 1 + uq; c <= ur; c += 4) Ls[ur][c] -= lr * Ls[c][j];
    }
    __syncthreads();
  }
  if (tid < kCovNB) {                                       // column tid of L^-1 by forward substitution
    const int c = tid;
#pragma unroll 1
    for (int r = c; r < kCovNB; ++r) {
      double s = r == c ? 1.0 : 0.0;
#pragma unroll 1
      for (int m = c; m < r; ++m) s -= Ls[r][m] * Ls[c][m + 1];
      Ls[c][r + 1] = s / Ls[r][r];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < kCovNB * kCovNB; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    if (c <= r) Akk[(size_t)r * Pp + c] = Ls[r][c];
    dinv[(size_t)k * kCovNB * kCovNB + idx] = c <= r ? Ls[c][r + 1] : 0.0;
  }
}

// ... second half: workgroup b stores the panel block L[k + 1 + b][k] = A[k + 1 + b][k] L_kk^-T
__global__ __launch_bounds__(256) void cov_chol_panel_kernel(double* __restrict__ S, int Pp, int k, const double* __restrict__ dinv) {
  __shared__ double As[kCovKC][kCovNB + 1];
  __shared__ double Bs[kCovKC][kCovNB + 1];
  const int tid = threadIdx.x;
  const double* Li = dinv + (size_t)k * kCovNB * kCovNB;
  double* Aik = S + ((size_t)(k + 1 + blockIdx.x) * kCovNB) * Pp + (size_t)k * kCovNB;
  double acc[4][4] = {};
  cov_tile_mm(acc, 0, kCovNB, [&](int r, int m) { return Aik[(size_t)r * Pp + m]; }, [&](int m, int c) { return Li[c * kCovNB + m]; }, As, Bs);
  __syncthreads();                                          // every read of A[i][k] is done
  const int tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) Aik[(size_t)(4 * ty + q) * Pp + 4 * tx + s] = acc[q][s];
}

// A[i][j] -= L[i][k] L[j][k]^T for k < j <= i: workgroup t = tile t of the trailing lower triangle, row-major
__global__ __launch_bounds__(256) void cov_chol_update_kernel(double* __restrict__ S, int Pp, int k) {
  __shared__ double As[kCovKC][kCovNB + 1];
  __shared__ double Bs[kCovKC][kCovNB + 1];
  int ti = 0, t = blockIdx.x;
  while (t > ti) { t -= ti + 1; ++ti; }
  const int i = k + 1 + ti, j = k + 1 + t;
  const double* Lik = S + ((size_t)i * kCovNB) * Pp + (size_t)k * kCovNB;
  const double* Ljk = S + ((size_t)j * kCovNB) * Pp + (size_t)k * kCovNB;
  double acc[4][4] = {};
  cov_tile_mm(acc, 0, kCovNB, [&](int r, int m) { return Lik[(size_t)r * Pp + m]; }, [&](int m, int c) { return Ljk[(size_t)c * Pp + m]; }, As, Bs);
  double* Aij = S + ((size_t)i * kCovNB) * Pp + (size_t)j * kCovNB;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) Aij[(size_t)(4 * ty + q) * Pp + 4 * tx + s] -= acc[q][s];
}

// Block row i of X = L^-1: X[i][i] = L_ii^-1, X[i][j] = -L_ii^-1 sum_{k = j .. i-1} L[i][k] X[k][j] for j < i (workgroup j)
__global__ __launch_bounds__(256) void cov_trinv_row_kernel(const double* __restrict__ L, double* __restrict__ X, int Pp, int i,
                                                            const double* __restrict__ dinv) {
  __shared__ double T[kCovNB][kCovNB + 1];
  __shared__ double As[kCovKC][kCovNB + 1];
  __shared__ double Bs[kCovKC][kCovNB + 1];
  const int j = blockIdx.x, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const double* Di = dinv + (size_t)i * kCovNB * kCovNB;
  double* Xij = X + ((size_t)i * kCovNB) * Pp + (size_t)j * kCovNB;
  if (j == i) {
    for (int idx = tid; idx < kCovNB * kCovNB; idx += 256) Xij[(size_t)(idx >> 6) * Pp + (idx & 63)] = Di[idx];
    return;
  }
  const double* Li = L + ((size_t)i * kCovNB) * Pp;
  const double* Xj = X + (size_t)j * kCovNB;
  double acc[4][4] = {};
  cov_tile_mm(acc, j * kCovNB, i * kCovNB, [&](int r, int m) { return Li[(size_t)r * Pp + m]; },
              [&](int m, int c) { return Xj[(size_t)m * Pp + c]; }, As, Bs);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) T[4 * ty + q][4 * tx + s] = acc[q][s];
  double out[4][4] = {};
  cov_tile_mm(out, 0, kCovNB, [&](int r, int m) { return Di[r * kCovNB + m]; }, [&](int m, int c) { return T[m][c]; }, As, Bs);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) Xij[(size_t)(4 * ty + q) * Pp + 4 * tx + s] = -out[q][s];
}

// Sigma[i][j] = sum_{k >= i} X[k][i]^T X[k][j] for j <= i, written to both triangles; a row or column that is not free is zero
__global__ __launch_bounds__(256) void cov_product_kernel(const double* __restrict__ X, double* __restrict__ Sg, int Pp, int nb,
                                                          const unsigned char* __restrict__ rowfree) {
  __shared__ double As[kCovKC][kCovNB + 1];
  __shared__ double Bs[kCovKC][kCovNB + 1];
  int i = 0, t = blockIdx.x;
  while (t > i) { t -= i + 1; ++i; }
  const int j = t;
  const double* Xi = X + (size_t)i * kCovNB;
  const double* Xj = X + (size_t)j * kCovNB;
  double acc[4][4] = {};
  cov_tile_mm(acc, i * kCovNB, nb * kCovNB, [&](int r, int m) { return Xi[(size_t)m * Pp + r]; },
              [&](int m, int c) { return Xj[(size_t)m * Pp + c]; }, As, Bs);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int r = i * kCovNB + 4 * ty + q, c = j * kCovNB + 4 * tx + s;
      if (i == j && c > r) continue;                       // the diagonal tile's upper half is its lower half mirrored
      const double val = (rowfree[r] && rowfree[c]) ? acc[q][s] : 0.0;
      Sg[(size_t)r * Pp + c] = val;
      Sg[(size_t)c * Pp + r] = val;
    }
}

__global__ void cov_cam_blocks_kernel(int V, int Pp, const double* __restrict__ Sg, double* __restrict__ cam_cov) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 49 * V) return;
  const int c = t / 49, ij = t % 49;
  cam_cov[t] = Sg[(size_t)(7 * c + ij / 7) * Pp + 7 * c + ij % 7];
}

// ---------------------------------------------------------------------------------------------
// The point kernel.  Row j of a track (j = 0 .. deg-1) is
//   x_j = sym( Y_j^T ( 2 sum_{i < j} Sigma_{c_j c_i} Y_i + Sigma_{c_j c_j} Y_j ) )       (the pairs i <= j, by symmetry)
// summed over i in ascending order by ONE lane, and Sigma_pp = D^-1 + sum_j x_j.  The rows sit in slots: slot 2 m holds
// row m, slot 2 m + 1 row deg-1-m (if that is a different row), so that two neighbouring slots always cost deg + 1 pairs.
// The slots are the leaves of a balanced binary tree whose inner nodes add their two children.
// ---------------------------------------------------------------------------------------------
struct CovPtArgs {
  int N, Pp;
  const int* pt_ptr;
  const int* cam_idx;
  const double* Y;        // [M][21]
  const double* Dinv;     // [N][6]
  const double* Sg;       // [Pp][Pp]
  double* pt_cov;         // [N][6]
};

__device__ __forceinline__ int cov_slot_row(int slot, int deg) {      // -1: the slot is empty
  const int m = slot >> 1;
  if (!(slot & 1)) return 2 * m < deg ? m : -1;
  return deg - 1 - m > m ? deg - 1 - m : -1;
}

// LDSY: the track's Y blocks are in `ys` ([deg][21]); else they are read from global memory
template <bool LDSY>
__device__ __forceinline__ void cov_row(const CovPtArgs& a, int beg, int j, const double* ys, double (&x)[6]) {
  const double* yg = a.Y + 21 * (size_t)beg;
  const int cj = a.cam_idx[beg + j];
  const double* srow = a.Sg + (size_t)(7 * cj) * a.Pp;
  double R[7][3] = {};
  for (int i = 0; i <= j; ++i) {
    const int ci = a.cam_idx[beg + i];
    double y[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) y[k] = LDSY ? ys[21 * i + k] : yg[21 * (size_t)i + k];
    if (i == j) {
#pragma unroll
      for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) R[r][k] *= 2.0;
    }
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const double* sg = srow + (size_t)r * a.Pp + 7 * ci;
#pragma unroll
      for (int b = 0; b < 7; ++b) {
        const double s = sg[b];
#pragma unroll
        for (int k = 0; k < 3; ++k) R[r][k] += s * y[3 * b + k];
      }
    }
    if (i == j) {                                           // y is Y_j: A = Y_j^T R, x = sym(A)
      double A[3][3] = {};
#pragma unroll
      for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int l = 0; l < 3; ++l) A[k][l] += y[3 * r + k] * R[r][l];
      x[0] = A[0][0]; x[1] = 0.5 * (A[0][1] + A[1][0]); x[2] = 0.5 * (A[0][2] + A[2][0]);
      x[3] = A[1][1]; x[4] = 0.5 * (A[1][2] + A[2][1]); x[5] = A[2][2];
    }
  }
}

template <int G>
__global__ __launch_bounds__(kCovPtBlock) void cov_points_kernel(CovPtArgs a) {
  constexpr int kCap = kCovSlots * G;
  constexpr int kLevels = 6;                                 // 64 slots at the most
  __shared__ double ytile[kCovPtBlock * kCovSlots * 21];
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)(t / G), lane = (int)(threadIdx.x % G);
  if (p >= a.N) return;                                      // whole groups leave together
  const int beg = a.pt_ptr[p], deg = a.pt_ptr[p + 1] - beg;
  if (deg > kCovGroupMax) return;                            // cov_points_block's
  double* ys = ytile + (size_t)(threadIdx.x - lane) * kCovSlots * 21;
  const bool staged = deg <= kCap;
  if (staged) {
    const double* yg = a.Y + 21 * (size_t)beg;
    for (int k = lane; k < 21 * deg; k += G) ys[k] = yg[k];
  }
  group_lds_sync();
  // The tree has S = the used slots rounded up to a power of two leaves (the empty ones are zeros, and x + 0 = x, so
  // any larger tree gives the same bits).  A lane takes a contiguous, aligned run of K = S / G slots (one slot when
  // S < G: the lanes beyond S hold zeros) and folds it with a binary counter: level l holds the sum of 2^l slots.
  const int n_slots = deg + (deg & 1);
  int S = 2;
  while (S < n_slots) S <<= 1;
  const int K = S > G ? S / G : 1;
  const int s_end = max(0, min(K, n_slots - lane * K));
  double stack[kLevels + 1][6] = {};
  double carry[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
  for (int s = 0; s < s_end; ++s) {
    const int row = cov_slot_row(lane * K + s, deg);
#pragma unroll
    for (int k = 0; k < 6; ++k) carry[k] = 0;
    if (row >= 0) {
      if (staged) cov_row<true>(a, beg, row, ys, carry);
      else cov_row<false>(a, beg, row, ys, carry);
    }
    bool active = true;
#pragma unroll
    for (int l = 0; l < kLevels; ++l) {
      const bool bit = (s >> l) & 1;
      if (active && bit) {
#pragma unroll
        for (int k = 0; k < 6; ++k) carry[k] = stack[l][k] + carry[k];
      } else if (active) {
#pragma unroll
        for (int k = 0; k < 6; ++k) stack[l][k] = carry[k];
        active = false;
      }
    }
  }
  // a full run ends with every level merged into carry; a run cut short by the end of the track folds what the counter
  // holds, lowest level first -- what running on over zero slots would give
  if (s_end < K) {
#pragma unroll
    for (int k = 0; k < 6; ++k) carry[k] = 0;
#pragma unroll
    for (int l = 0; l < kLevels; ++l) {
      if ((s_end >> l) & 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) carry[k] = stack[l][k] + carry[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) carry[k] = group_sum<G>(carry[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.pt_cov[6 * (size_t)p + k] = a.Dinv[6 * (size_t)p + k] + carry[k];
  }
}

// Tracks beyond kCovGroupMax, one workgroup of 256 per point: thread t adds slots t, t + 256, ... in ascending order, the
// 256 partial sums go through a wave tree and four wave totals are added in order.
__global__ __launch_bounds__(256) void cov_points_block_kernel(CovPtArgs a) {
  __shared__ double part[4][6];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int beg = a.pt_ptr[p], deg = a.pt_ptr[p + 1] - beg;
  if (deg <= kCovGroupMax) return;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int s = tid; s < deg + 1; s += 256) {
    const int row = cov_slot_row(s, deg);
    if (row < 0) continue;
    double x[6];
    cov_row<false>(a, beg, row, nullptr, x);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += x[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = group_sum<64>(acc[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) part[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < 6) a.pt_cov[6 * (size_t)p + tid] = a.Dinv[6 * (size_t)p + tid] + (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
}

// The group width `group` = 0 stands for: the narrowest that gives a mean track one slot pair per lane, widened while the
// scene would otherwise leave the device short of waves.
static int cov_pick_group(int n_pts, long long M, int max_track) {
  const long long mean = n_pts > 0 ? (M + n_pts - 1) / n_pts : 1;
  const int top = std::min(max_track, kCovGroupMax);
  const int i = narrowest_group([&](int w) { return 2 * w >= std::min<long long>(mean + 1, top + 1); });
  return kGroupWidths[widen_for_waves(i, n_pts, top + 1)];
}

template <int G>
static void launch_cov_points(const CovPtArgs& a, hipStream_t s) {
  const long long threads = (long long)a.N * G;
  cov_points_kernel<G><<<dim3((unsigned)((threads + kCovPtBlock - 1) / kCovPtBlock)), dim3(kCovPtBlock), 0, s>>>(a);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct CovWork {
  DevBuf<unsigned char> mask, rowfree;
  DevBuf<double> Dinv, W, Y, cost_pt, red, S, X, dinv, diag0, cam_cov, pt_cov;
  DevBuf<int> pt_status, status;
};

// the per-point terms and the cost (a mark of `ev` behind them), then S if it is wanted
static int cov_enqueue_terms(sfm_ba_problem* p, double lambda, int quirks, int loss_kind, CovWork& w, int Pp, bool want_s,
                             PhaseEvents& ev) {
  return dispatch_loss(loss_kind, [&](auto L) -> int {
    constexpr int LOSS = decltype(L)::value;
    const BaDev& d = p->dev;
    hipStream_t s = p->stream;
    const LossArg<LOSS> la = loss_arg<LOSS>(p);
    cov_point_terms_kernel<LOSS><<<(d.N + 127) / 128, 128, 0, s>>>(d, p->cur, lambda, quirks, la, w.Dinv.p, w.W.p, w.Y.p, w.cost_pt.p,
                                                                   w.pt_status.p);
    ba_point_cost_reduce_kernel<<<1, 256, 0, s>>>(d.N, w.cost_pt.p, d.pt_ptr, w.red.p);
    SFM_TRY(ev.mark(s));
    if (want_s)
      cov_build_s_kernel<LOSS><<<(unsigned)((long long)d.V * (d.V + 1) / 2), 256, 0, s>>>(d, p->cur, lambda, quirks, la, p->cam_ptr, p->cam_obs,
                                                                                      w.mask.p, w.W.p, w.Y.p, w.pt_status.p, w.S.p, Pp);
    SFM_HIP(hipGetLastError());
    return SFM_OK;
  });
}

// S (in w.S, cleared, rows set) -> Sigma in w.S; *fail_row >= 0: the first row whose pivot was not positive
static int cov_enqueue_inverse(hipStream_t s, CovWork& w, int Pp, int* fail_row) {
  const int nb = Pp / kCovNB;
  SFM_TRY(w.X.alloc((size_t)Pp * Pp, s));
  SFM_TRY(w.dinv.alloc((size_t)nb * kCovNB * kCovNB, s));
  SFM_TRY(w.diag0.alloc((size_t)Pp, s));
  SFM_TRY(w.status.alloc(2, s));
  SFM_HIP(hipMemsetAsync(w.status.p, 0, 2 * sizeof(int), s));
  SFM_HIP(hipMemsetAsync(w.X.p, 0, sizeof(double) * (size_t)Pp * Pp, s));
  cov_diag_kernel<<<(Pp + 255) / 256, 256, 0, s>>>(Pp, w.S.p, w.diag0.p);
  // A pivot of a singular direction is rounding noise amplified by the pivots before it: measured on the test scenes,
  // |noise| <= 7e-11 of the row's diagonal entry, while the smallest pivot of a system that does have an inverse
  // (two cameras held, or lambda >= 1e-6) is 4e-5 of it.  Below 1e-9 fewer than seven digits of the inverse would be left.
  const double tol = 1e-9;
  for (int k = 0; k < nb; ++k) {
    cov_chol_diag_kernel<<<1, 256, 0, s>>>(w.S.p, Pp, k, w.diag0.p, tol, w.dinv.p, w.status.p);
    const int n = nb - k - 1;
    if (n > 0) cov_chol_panel_kernel<<<n, 256, 0, s>>>(w.S.p, Pp, k, w.dinv.p);
    if (n > 0) cov_chol_update_kernel<<<n * (n + 1) / 2, 256, 0, s>>>(w.S.p, Pp, k);
  }
  SFM_HIP(hipGetLastError());
  int st[2] = {0, 0};
  SFM_HIP(hipMemcpyAsync(st, w.status.p, sizeof(st), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  *fail_row = st[0] != 0 ? st[1] : -1;
  if (st[0] != 0) return SFM_OK;
  for (int i = 0; i < nb; ++i) cov_trinv_row_kernel<<<i + 1, 256, 0, s>>>(w.S.p, w.X.p, Pp, i, w.dinv.p);
  cov_product_kernel<<<nb * (nb + 1) / 2, 256, 0, s>>>(w.X.p, w.S.p, Pp, nb, w.rowfree.p);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_ba_covariance_plan(int n_cams, int* block, int* n_blocks, int* n_launches, int* group_max_track) {
  if (n_cams < 1) { set_error("sfm_ba_covariance_plan: n_cams < 1"); return SFM_E_SHAPE; }
  const int nb = (7 * n_cams + kCovNB - 1) / kCovNB;
  if (block) *block = kCovNB;
  if (n_blocks) *n_blocks = nb;
  if (n_launches) *n_launches = 4 * nb - 1;      // nb diagonal blocks, nb - 1 panels and updates, nb rows of X, the product
  if (group_max_track) *group_max_track = kCovGroupMax;
  return SFM_OK;
}

int sfm_ba_covariance_times(sfm_ba_problem* p, double* ms) {
  SFM_TRY(ba_check_handle(p));
  if (ms == nullptr) { set_error("sfm_ba_covariance_times: ms is null"); return SFM_E_SHAPE; }
  for (int k = 0; k < 4; ++k) ms[k] = p->cov_ms[k];
  return SFM_OK;
}

int sfm_ba_covariance(sfm_ba_problem* p, double lambda, int quirks, int use_loss, const unsigned char* cam_mask, int group,
                      double* cam_cov, double* pt_cov, int* cam_status, int* pt_status, double* sigma0_sq) {
  SFM_TRY(ba_check_handle(p));
  if (!(lambda >= 0)) { set_error("sfm_ba_covariance: lambda must be >= 0"); return SFM_E_SHAPE; }
  if (use_loss != 0 && use_loss != 1) { set_error("sfm_ba_covariance: use_loss must be 0 or 1"); return SFM_E_SHAPE; }
  SFM_TRY(group_width_check("sfm_ba_covariance", group));
  SFM_TRY(ba_refuse_comm(p, "sfm_ba_covariance", "the points are sharded; Sigma_ff needs the all-reduced S"));
  const BaDev& d = p->dev;
  const int V = d.V, N = d.N;
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  hipStream_t s = p->stream;
  SFM_TRY(ba_prepared_cameras(p, "sfm_ba_covariance"));
  int v_free = 0, first_free = -1;
  ba_free_cameras(cam_mask, V, &v_free, &first_free);
  if (cam_status)
    for (int c = 0; c < V; ++c) cam_status[c] = (cam_mask && cam_mask[c] == 0) ? SFM_COV_CAM_HELD : 0;
  if (N == 0 || d.M == 0) {                              // nothing is observed: S_ff = lambda I, every point is empty
    if (v_free > 0 && !(lambda > 0)) {
      if (cam_status) cam_status[first_free] |= SFM_COV_CAM_PIVOT;
      set_error("sfm_ba_covariance: the free cameras' system is not positive definite at camera %d (no observations, lambda = 0)", first_free);
      return SFM_E_SINGULAR;
    }
    if (cam_cov) {
      std::fill(cam_cov, cam_cov + 49 * (size_t)V, 0.0);
      for (int c = 0; c < V; ++c)
        if (cam_mask == nullptr || cam_mask[c] != 0)
          for (int i = 0; i < 7; ++i) cam_cov[49 * (size_t)c + 8 * i] = 1.0 / lambda;
    }
    if (pt_cov) std::fill(pt_cov, pt_cov + 6 * (size_t)N, 0.0);
    if (pt_status) std::fill(pt_status, pt_status + N, (int)SFM_COV_PT_EMPTY);
    if (sigma0_sq) *sigma0_sq = 0.0;
    return stream_sync(s);
  }
  const bool want_sigma = v_free > 0;                    // every camera held: Sigma_pp = D^-1, no system to invert
  const int P = 7 * V, Pp = (P + kCovNB - 1) / kCovNB * kCovNB;
  const size_t n = (size_t)N, m = (size_t)d.M;
  CovWork w;
  // SFM_OPT_TIMING (any bit): marks around the four phases, read back by sfm_ba_covariance_times
  PhaseEvents ev(p->timing != 0);
  for (int k = 0; k < 4; ++k) p->cov_ms[k] = 0.f;
  if (cam_mask) {
    SFM_TRY(w.mask.upload(cam_mask, (size_t)V, s));
    p->upload_bytes += V;
  }
  SFM_TRY(w.Dinv.alloc(6 * n, s)); SFM_TRY(w.W.alloc(21 * m, s)); SFM_TRY(w.Y.alloc(21 * m, s));
  SFM_TRY(w.cost_pt.alloc(n, s)); SFM_TRY(w.pt_status.alloc(n, s)); SFM_TRY(w.red.alloc(2, s));
  SFM_TRY(w.pt_cov.alloc(6 * n, s));
  if (want_sigma) {
    SFM_TRY(ba_cam_list_ensure(p));
    SFM_TRY(w.S.alloc((size_t)Pp * Pp, s));
    SFM_TRY(w.rowfree.alloc((size_t)Pp, s));
    SFM_HIP(hipMemsetAsync(w.S.p, 0, sizeof(double) * (size_t)Pp * Pp, s));
    cov_rows_kernel<<<(Pp + 255) / 256, 256, 0, s>>>(P, Pp, w.mask.p, w.rowfree.p, w.S.p);
  }
  SFM_HIP(hipMemsetAsync(w.red.p, 0, 2 * sizeof(double), s));
  SFM_TRY(ev.mark(s));
  SFM_TRY(cov_enqueue_terms(p, lambda, quirks, use_loss ? p->loss_kind : SFM_LOSS_NONE, w, Pp, want_sigma, ev));
  int fail_row = -1;
  SFM_TRY(ev.mark(s));
  if (want_sigma) SFM_TRY(cov_enqueue_inverse(s, w, Pp, &fail_row));
  SFM_TRY(ev.mark(s));
  if (fail_row >= 0) {
    SFM_TRY(stream_sync(s));
    const int cam = std::min(fail_row / 7, V - 1);
    if (cam_status) cam_status[cam] |= SFM_COV_CAM_PIVOT;
    set_error("sfm_ba_covariance: the free cameras' system is not positive definite at camera %d "
              "(hold at least two cameras, or use lambda > 0)", cam);
    return SFM_E_SINGULAR;
  }
  if (pt_cov != nullptr) {
    if (want_sigma) {
      CovPtArgs a = {};
      a.N = N; a.Pp = Pp; a.pt_ptr = d.pt_ptr; a.cam_idx = d.cam_idx; a.Y = w.Y.p; a.Dinv = w.Dinv.p; a.Sg = w.S.p; a.pt_cov = w.pt_cov.p;
      const int g = group ? group : cov_pick_group(N, d.M, p->max_track);
      dispatch_group<1>(g, [&](auto G) { launch_cov_points<decltype(G)::value>(a, s); });
      if (p->max_track > kCovGroupMax) cov_points_block_kernel<<<N, 256, 0, s>>>(a);
      SFM_HIP(hipGetLastError());
      SFM_TRY(ev.mark(s));
      SFM_TRY(w.pt_cov.download(pt_cov, 6 * n, s));
    } else {
      SFM_TRY(w.Dinv.download(pt_cov, 6 * n, s));
    }
  }
  if (cam_cov != nullptr) {
    if (want_sigma) {
      SFM_TRY(w.cam_cov.alloc(49 * (size_t)V, s));
      cov_cam_blocks_kernel<<<(49 * V + 255) / 256, 256, 0, s>>>(V, Pp, w.S.p, w.cam_cov.p);
      SFM_HIP(hipGetLastError());
      SFM_TRY(w.cam_cov.download(cam_cov, 49 * (size_t)V, s));
    } else {
      std::fill(cam_cov, cam_cov + 49 * (size_t)V, 0.0);
    }
  }
  if (pt_status != nullptr) SFM_TRY(w.pt_status.download(pt_status, n, s));
  double red[2] = {0, 0};
  SFM_TRY(w.red.download(red, 2, s));
  SFM_TRY(stream_sync(s));
  for (int k = 0; k < 4; ++k) p->cov_ms[k] = ev.elapsed_ms(k);      // (the points' phase has its closing mark only when it ran)
  if (sigma0_sq) {
    const double dof = 2.0 * (double)d.M - 7.0 * v_free - 3.0 * red[1];
    *sigma0_sq = dof > 0 ? red[0] / dof : 0.0;
  }
  return SFM_OK;
}

}  // extern "C"
