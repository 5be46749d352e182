// sfm_dlt.h — the per-thread DLT solver shared by the rectangular (sfm_core.hip) and the ragged-track
// (sfm_tri_tracks.hip) linear triangulation: streaming Givens QR of the rows into a 4x4 upper-triangular R, then a
// one-sided Jacobi SVD of R in registers; the column of smallest norm gives the null vector.
#pragma once

#include "sfm_common.h"

namespace sfm {

__device__ __forceinline__ void dlt_add_row(double (&R)[4][4], double r0, double r1, double r2, double r3) {
  double row[4] = {r0, r1, r2, r3};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double a = R[i][i], b = row[i];
    if (b != 0.0) {
      const double h = sqrt(a * a + b * b);
      const double c = a / h, s = b / h;
#pragma unroll
      for (int k = i; k < 4; ++k) {
        const double x = R[i][k], y = row[k];
        R[i][k] = c * x + s * y;
        row[k] = -s * x + c * y;
      }
    }
  }
}

__device__ __forceinline__ void dlt_null_vector(double (&B)[4][4], double* x_out) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double al = 0, be = 0, ga = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { al += B[k][p] * B[k][p]; be += B[k][q] * B[k][q]; ga += B[k][p] * B[k][q]; }
        if (fabs(ga) > 1e-17 * sqrt(al * be) && ga != 0.0) {
          rotated = true;
          const double ze = (be - al) / (2.0 * ga);
          const double t = (ze == 0.0) ? 1.0 : copysign(1.0, ze) / (fabs(ze) + sqrt(1.0 + ze * ze));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double bp = B[k][p], bq = B[k][q];
            B[k][p] = c * bp - s * bq; B[k][q] = s * bp + c * bq;
            const double vp = V[k][p], vq = V[k][q];
            V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
  double best = 0;
  double v[4] = {0, 0, 0, 1};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) n += B[k][c] * B[k][c];
    if (c == 0 || n < best) {
      best = n;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = V[k][c];
    }
  }
  x_out[0] = v[0] / v[3]; x_out[1] = v[1] / v[3]; x_out[2] = v[2] / v[3]; x_out[3] = v[3] / v[3];   // tri:152
}

}  // namespace sfm
