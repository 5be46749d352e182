// sfm_eight_point.h -- the eight-point solve of one wave, shared by fund_eight_point_kernel (sfm_epipolar.hip) and the
// robust two-view geometry (sfm_twoview.hip): the null vector of a design matrix held as rows-in-lanes by the
// wave-cooperative one-sided Jacobi, and the rank-2 projection of the 3x3 matrix with matrix_rank's test.  What follows
// the projected matrix (the division by f[2][2] there, de-normalisation and scaling here) stays with the caller.
//
// Compiled with the compiler's default contraction: include it BEFORE sfm_obs_test.h.
#pragma once

#include "sfm_common.h"

namespace sfm {

// 3x3 SVD pieces: columns of B become sigma_c u_c, V the right singular vectors; ord[] sorts sigma descending.
// B is first scaled by the power of two that brings max|B| into [1, 2): exact, so the result is that of 2^e B, whose
// Jacobi sums al, be and al*be cannot overflow (they did from max|B| ~ 2^255) or lose bits to underflow (below ~2^-511).
// sigma and the columns of B come out scaled by 2^e; every caller uses sigma only in ratios or as B / sigma.
__device__ inline void svd3(double (&B)[3][3], double (&V)[3][3], double (&sig)[3], int (&ord)[3]) {
  double mx = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) mx = fmax(mx, fabs(B[i][j]));        // fmax skips NaN, which stays NaN below
  if (mx > 0.0 && mx <= 1.7976931348623157e308) {
    const int e = -ilogb(mx);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) B[i][j] = ldexp(B[i][j], e);
  }
  jacobi_right_vectors<3>(B, V, 40);
  for (int c = 0; c < 3; ++c) sig[c] = sqrt(B[0][c] * B[0][c] + B[1][c] * B[1][c] + B[2][c] * B[2][c]);
  ord[0] = 0; ord[1] = 1; ord[2] = 2;
  for (int i = 0; i < 2; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (sig[ord[j]] > sig[ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
}

// The design row of one normalised match p = (x1, y1, x2, y2): epipolar_processor.py:156-171.
__device__ __forceinline__ void eight_point_row(const double* p, double (&row)[9]) {
  const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
  row[0] = x1 * x2; row[1] = y1 * x2; row[2] = x2;
  row[3] = x1 * y2; row[4] = y1 * y2; row[5] = y2;
  row[6] = x1;      row[7] = y1;      row[8] = 1.0;
}

// Lanes 0..8 hold the rows of a matrix of nine columns (the 8x9 design matrix and a zero row, or a symmetric 9x9 moment
// matrix; lanes 9..15 zero rows), lanes 16..24 the identity, every other lane zeros.  After jacobi_rows_wave the null
// vector is the column of V whose B V column has the smallest norm; every lane gets it as f (row-major 3x3).
__device__ __forceinline__ void eight_point_null_vector(double (&row)[9], int lane, double (&f)[9]) {
  jacobi_rows_wave<9>(row, lane, 40);
  int best = 0;
  double bn = 0;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const double nn = wave_lane0(group_sum<16>(lane < 16 ? row[c] * row[c] : 0.0));
    if (c == 0 || nn < bn) { bn = nn; best = c; }
  }
  double mine = 0.0;
#pragma unroll
  for (int c = 0; c < 9; ++c) mine = (c == best) ? row[c] : mine;
#pragma unroll
  for (int k = 0; k < 9; ++k) {                                  // f_ = reshape(null vector, (3, 3))
    const int lo = __builtin_amdgcn_readlane(__double2loint(mine), 16 + k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(mine), 16 + k);
    f[k] = __hiloint2double(hi, lo);
  }
}

// One lane: f2 = u diag(s0, s1, 0) v^T of f (epipolar:181-188); SFM_E_RANK if f2 is not of rank 2.
__device__ __forceinline__ int eight_point_project(const double (&f)[9], double (&f2)[9]) {
  double B[3][3], V3[3][3], sig[3];
  int ord[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i][j] = f[3 * i + j];
  svd3(B, V3, sig, ord);
  // matrix_rank tolerance: sigma_max * max(M, N) * eps (numpy.linalg.matrix_rank)
  const double tol = sig[ord[0]] * 3.0 * 2.220446049250313e-16;
  int st = (sig[ord[1]] > tol) ? SFM_OK : SFM_E_RANK;
  if (!(sig[ord[0]] == sig[ord[0]])) st = SFM_E_RANK;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)       // u diag(s0, s1, 0) v^T = sum over the two largest of (sigma u)_i v_j
      f2[3 * i + j] = B[i][ord[0]] * V3[j][ord[0]] + B[i][ord[1]] * V3[j][ord[1]];
  return st;
}

}  // namespace sfm
