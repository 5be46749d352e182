// sfm_five_point.h -- the minimal solver of the robust essential matrix (sfm_essential.hip; the rule is in sfm_hip.h, block
// "robust essential matrix", step 5): the essential matrices of five matches given as rays, ONE function for the
// hypothesis kernel and for the host (sfm_essential_solve).
//
// All state of a solve lives in a FivePointWork (LDS on the device, the stack on the host) and the work is written as
// loops over ROWS, intervals or roots that a lane group shares: `for (i = g.first(); i < n; i += g.step())`, and g.sync()
// where the next loop reads what this one wrote.  On the device a group is 16 lanes of a workgroup of 64 (first = lane
// & 15, step = 16, sync = the workgroup barrier: every group of the workgroup passes the same syncs, none sits in a
// data-dependent branch); on the host first = 0, step = 1 and sync does nothing.  No value crosses a sync in a register
// and every element is computed by one lane with the same operations in the same order, so host and device agree bit
// for bit.  The stages:
//   null     the four-dimensional null space of the 5x9 matrix of b (x) a by Gauss-Jordan elimination with full
//            pivoting (a lane per row; the pivot search is repeated by every lane)
//   cubics   the ten cubic equations det E = 0, 2 E E^T E - tr(E E^T) E = 0 of E = x N0 + y N1 + z N2 + N3 as a 10x20
//            coefficient matrix (a lane per equation), columns ordered x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy |
//            xz^2 xz x yz^2 yz y z^3 z^2 z 1
//   elim     Gauss-Jordan on the left ten columns with partial pivoting (a lane per row, the pivot row read by all)
//   poly     rows x^2z - z x^2, y^2z - z y^2, xyz - z xy give a 3x3 matrix B(z) with B (x, y, 1)^T = 0, entries of degree
//            3, 3, 4; det B is the degree-10 polynomial in z
//   roots    its real roots by the derivative chain: the roots of p^(k+1) separate those of p^(k); a lane per
//            interval, a sign test, 64 bisections and two guarded Newton steps; ten levels
//   finish   a lane per root: (x, y) from the null vector of B(z), kFpPolish Gauss-Newton steps of (x, y, z) on the ten cubics
//            as first written, E scaled to the canonical form, the solutions ranked by E[0]
// A degenerate sample makes a pivot zero or the leading coefficient vanish: what follows is not finite and is left out.
//
// Compiled WITHOUT automatic contraction, the FMAs spelled out: include it after sfm_obs_test.h.
#pragma once

#include "sfm_obs_test.h"

namespace sfm {

constexpr int kFpMaxSol = 10;
constexpr int kFpPolish = 2;          // Gauss-Newton steps on every root (four were tried on the host: no better in the worst case)

struct FivePointWork {
  double a[5][2], b[5][2];      // in: the rays (a0, a1, 1), (b0, b1, 1) of the five matches
  double A[5][9];               // null: the design matrix, reduced in place
  int prow[5], pcol[5];         // null: pivot row and column of every step
  double N[4][9];               // the basis N0 .. N3
  double M0[10][20];            // cubics: the equations as first written (kept for the polish)
  double M[10][20];             // elim: reduced in place
  int rowof[10];                // elim: the row that holds the pivot of column k
  double B[3][3][5];            // poly: B[row][x, y, 1][power of z]
  double d[11][11];             // roots: d[k][j] the coefficient of z^j of the k-th derivative
  double crit[11];              // roots: the roots of the level above, ascending
  double found[11];             // roots: the root of interval i of this level, NaN if there is none
  double bound;                 // roots: all real roots lie in (-bound, bound)
  double sol[kFpMaxSol][9];     // finish: the canonical E of root r
  double key[kFpMaxSol];        // finish: its E[0], NaN if the root gave no finite E
  double E[kFpMaxSol][9];       // out: the solutions by ascending key
  int n;                        // out: their number
};

struct FpHostGroup {
  __host__ __device__ int first() const { return 0; }
  __host__ __device__ int step() const { return 1; }
  __host__ __device__ void sync() const {}
};

// ---- the monomials of a cubic in (x, y, z): the column of x^nx y^ny z^nz, and of a product of three of (x, y, z, 1) ----
__host__ __device__ constexpr int fp_col(int nx, int ny, int nz) {
  return nx == 3 ? 0 : ny == 3 ? 1 : (nx == 2 && ny == 1) ? 2 : (nx == 1 && ny == 2) ? 3 : (nx == 2 && nz == 1) ? 4 : nx == 2 ? 5
       : (ny == 2 && nz == 1) ? 6 : ny == 2 ? 7 : (nx == 1 && ny == 1 && nz == 1) ? 8 : (nx == 1 && ny == 1) ? 9
       : (nx == 1 && nz == 2) ? 10 : (nx == 1 && nz == 1) ? 11 : nx == 1 ? 12 : (ny == 1 && nz == 2) ? 13 : (ny == 1 && nz == 1) ? 14
       : ny == 1 ? 15 : nz == 3 ? 16 : nz == 2 ? 17 : nz == 1 ? 18 : 19;
}
__host__ __device__ constexpr int fp_col3(int u, int v, int w) {       // variables 0 x, 1 y, 2 z, 3 the constant
  return fp_col((u == 0) + (v == 0) + (w == 0), (u == 1) + (v == 1) + (w == 1), (u == 2) + (v == 2) + (w == 2));
}
// a product of two of them: the pair (u <= v) in the order 00 01 02 03 11 12 13 22 23 33
__host__ __device__ constexpr int fp_pair(int u, int v) {
  return u <= v ? (u * 4 - u * (u - 1) / 2 + (v - u)) : (v * 4 - v * (v - 1) / 2 + (u - v));
}
__host__ __device__ constexpr int fp_pair_u(int q) { return q < 4 ? 0 : q < 7 ? 1 : q < 9 ? 2 : 3; }
__host__ __device__ constexpr int fp_pair_v(int q) { return q < 4 ? q : q < 7 ? q - 3 : q < 9 ? q - 5 : 3; }

// q += l * m (two linear forms), q += s q2, c += q * l
__host__ __device__ inline void fp_mul11(const double* l, const double* m, double* q) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) q[fp_pair(u, v)] = __builtin_fma(l[u], m[v], q[fp_pair(u, v)]);
}
__host__ __device__ inline void fp_mul21(const double* q, const double* l, double* c) {
#pragma unroll
  for (int p = 0; p < 10; ++p)
#pragma unroll
    for (int w = 0; w < 4; ++w) c[fp_col3(fp_pair_u(p), fp_pair_v(p), w)] = __builtin_fma(q[p], l[w], c[fp_col3(fp_pair_u(p), fp_pair_v(p), w)]);
}
__host__ __device__ inline void fp_entry(const FivePointWork& w, int e, double* l) {
#pragma unroll
  for (int v = 0; v < 4; ++v) l[v] = w.N[v][e];
}

// Equation q of the ten: q < 9 entry (q / 3, q % 3) of 2 E E^T E - tr(E E^T) E, q = 9 the determinant.
__host__ __device__ inline void fp_cubic(const FivePointWork& w, int q, double* c) {
#pragma unroll
  for (int k = 0; k < 20; ++k) c[k] = 0.0;
  double l0[4], l1[4], l2[4];
  if (q == 9) {
    for (int t = 0; t < 3; ++t) {                          // e_0t (e_1u e_2v - e_1v e_2u), (t, u, v) cyclic
      const int u = (t + 1) % 3, v = (t + 2) % 3;
      double m[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) m[k] = 0.0;
      fp_entry(w, 3 + u, l0); fp_entry(w, 6 + v, l1);
      fp_mul11(l0, l1, m);
      fp_entry(w, 3 + v, l0); fp_entry(w, 6 + u, l1);
#pragma unroll
      for (int k = 0; k < 4; ++k) l0[k] = -l0[k];
      fp_mul11(l0, l1, m);
      fp_entry(w, t, l2);
      fp_mul21(m, l2, c);
    }
    return;
  }
  const int i = q / 3, j = q % 3;
  double tr[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) tr[k] = 0.0;
  for (int e = 0; e < 9; ++e) { fp_entry(w, e, l0); fp_mul11(l0, l0, tr); }
  for (int k = 0; k < 3; ++k) {                            // (2 (E E^T)_ik - [i = k] tr) e_kj
    double m[10];
#pragma unroll
    for (int p = 0; p < 10; ++p) m[p] = 0.0;
    for (int s = 0; s < 3; ++s) { fp_entry(w, 3 * i + s, l0); fp_entry(w, 3 * k + s, l1); fp_mul11(l0, l1, m); }
    const double on = (i == k) ? 1.0 : 0.0;
#pragma unroll
    for (int p = 0; p < 10; ++p) m[p] = __builtin_fma(-on, tr[p], 2.0 * m[p]);
    fp_entry(w, 3 * k + j, l2);
    fp_mul21(m, l2, c);
  }
}

// The value of the 20 monomials at (x, y, z) in column order.
__host__ __device__ inline void fp_monomials(double x, double y, double z, double* m) {
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y;
  m[0] = xx * x; m[1] = yy * y; m[2] = xx * y; m[3] = x * yy; m[4] = xx * z; m[5] = xx; m[6] = yy * z; m[7] = yy; m[8] = xy * z; m[9] = xy;
  m[10] = x * zz; m[11] = x * z; m[12] = x; m[13] = y * zz; m[14] = y * z; m[15] = y; m[16] = zz * z; m[17] = zz; m[18] = z; m[19] = 1.0;
}

// c0 + c1 z + ... + c_deg z^deg
__host__ __device__ inline double fp_horner(const double* c, int deg, double z) {
  double v = c[deg];
  for (int k = deg - 1; k >= 0; --k) v = __builtin_fma(v, z, c[k]);
  return v;
}

// out (degree da + db) += s a b
__host__ __device__ inline void fp_poly_mac(const double* a, int da, const double* b, int db, double s, double* out) {
  for (int i = 0; i <= da; ++i)
    for (int j = 0; j <= db; ++j) out[i + j] = __builtin_fma(s * a[i], b[j], out[i + j]);
}

// g scaled to Frobenius norm 1 with its entry of largest magnitude (the first of them) positive; false if g is not
// finite or zero.  (canon9 of sfm_match_norm.h, for host and device.)
__host__ __device__ inline bool fp_canon9(double* g) {
  double ss = 0, big = -1.0, sign = 1.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double v = g[k];
    ss = __builtin_fma(v, v, ss);
    const bool larger = __builtin_fabs(v) > big;
    sign = larger ? (v < 0.0 ? -1.0 : 1.0) : sign;
    big = larger ? __builtin_fabs(v) : big;
  }
  const double nrm = sign * __builtin_sqrt(ss);
#pragma unroll
  for (int k = 0; k < 9; ++k) g[k] = g[k] / nrm;
  return ss > 0.0 && __builtin_isfinite(ss);
}

// One Gauss-Newton step of (x, y, z) on the ten cubics M0; the step is left out if it is not finite.
__host__ __device__ inline void fp_polish(const FivePointWork& w, double& x, double& y, double& z) {
  double m[20], gx[20], gy[20], gz[20];
  fp_monomials(x, y, z, m);
#pragma unroll
  for (int k = 0; k < 20; ++k) { gx[k] = 0.0; gy[k] = 0.0; gz[k] = 0.0; }
  const double xx = x * x, yy = y * y, zz = z * z;
  gx[0] = 3.0 * xx; gx[2] = 2.0 * (x * y); gx[3] = yy; gx[4] = 2.0 * (x * z); gx[5] = 2.0 * x; gx[8] = y * z; gx[9] = y;
  gx[10] = zz; gx[11] = z; gx[12] = 1.0;
  gy[1] = 3.0 * yy; gy[2] = xx; gy[3] = 2.0 * (x * y); gy[6] = 2.0 * (y * z); gy[7] = 2.0 * y; gy[8] = x * z; gy[9] = x;
  gy[13] = zz; gy[14] = z; gy[15] = 1.0;
  gz[4] = xx; gz[6] = yy; gz[8] = x * y; gz[10] = 2.0 * (x * z); gz[11] = x; gz[13] = 2.0 * (y * z); gz[14] = y;
  gz[16] = 3.0 * zz; gz[17] = 2.0 * z; gz[18] = 1.0;
  double s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0, r0 = 0, r1 = 0, r2 = 0;
#pragma unroll 1
  for (int i = 0; i < 10; ++i) {
    double f = 0, jx = 0, jy = 0, jz = 0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
      const double c = w.M0[i][k];
      f = __builtin_fma(c, m[k], f); jx = __builtin_fma(c, gx[k], jx); jy = __builtin_fma(c, gy[k], jy); jz = __builtin_fma(c, gz[k], jz);
    }
    s00 = __builtin_fma(jx, jx, s00); s01 = __builtin_fma(jx, jy, s01); s02 = __builtin_fma(jx, jz, s02);
    s11 = __builtin_fma(jy, jy, s11); s12 = __builtin_fma(jy, jz, s12); s22 = __builtin_fma(jz, jz, s22);
    r0 = __builtin_fma(jx, f, r0); r1 = __builtin_fma(jy, f, r1); r2 = __builtin_fma(jz, f, r2);
  }
  // the step solves S d = r by the adjugate of the symmetric S
  const double c00 = __builtin_fma(s11, s22, -(s12 * s12)), c01 = __builtin_fma(s02, s12, -(s01 * s22)), c02 = __builtin_fma(s01, s12, -(s02 * s11));
  const double c11 = __builtin_fma(s00, s22, -(s02 * s02)), c12 = __builtin_fma(s01, s02, -(s00 * s12)), c22 = __builtin_fma(s00, s11, -(s01 * s01));
  const double det = __builtin_fma(s00, c00, __builtin_fma(s01, c01, s02 * c02));
  const double dx = __builtin_fma(c00, r0, __builtin_fma(c01, r1, c02 * r2)) / det;
  const double dy = __builtin_fma(c01, r0, __builtin_fma(c11, r1, c12 * r2)) / det;
  const double dz = __builtin_fma(c02, r0, __builtin_fma(c12, r1, c22 * r2)) / det;
  const bool ok = ((dx + dy + dz) * 0.0) == 0.0;
  x = ok ? x - dx : x; y = ok ? y - dy : y; z = ok ? z - dz : z;
}

// The solver.  In: w.a, w.b (written before a sync).  Out: w.E[0 .. w.n - 1], valid after the call's last sync.
template <class Group>
__host__ __device__ inline void five_point_solve(const Group& g, FivePointWork& w) {
  const int first = g.first(), step = g.step();
  // ---- null ----
  for (int r = first; r < 5; r += step) {
    const double b[3] = {w.b[r][0], w.b[r][1], 1.0}, a[3] = {w.a[r][0], w.a[r][1], 1.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) w.A[r][3 * i + j] = b[i] * a[j];
  }
  g.sync();
  for (int k = 0; k < 5; ++k) {
    // every lane repeats the search: the largest magnitude among the rows and columns not yet used, the first of them
    unsigned used_r = 0, used_c = 0;
    for (int q = 0; q < k; ++q) { used_r |= 1u << w.prow[q]; used_c |= 1u << w.pcol[q]; }
    int pr = 0, pc = 0;
    double big = -1.0;
    for (int r = 0; r < 5; ++r)
      for (int c = 0; c < 9; ++c) {
        const double v = __builtin_fabs(w.A[r][c]);
        const bool take = !(used_r >> r & 1) && !(used_c >> c & 1) && (v > big || big < 0.0);
        if (take) { big = v; pr = r; pc = c; }
      }
    g.sync();                                              // the search has read what the writes below change
    for (int r = first; r < 5; r += step) {
      if (r == pr) { w.prow[k] = pr; w.pcol[k] = pc; continue; }
      const double f = w.A[r][pc] / w.A[pr][pc];
      for (int c = 0; c < 9; ++c) w.A[r][c] = (c == pc) ? 0.0 : __builtin_fma(-f, w.A[pr][c], w.A[r][c]);
    }
    g.sync();
  }
  for (int v = first; v < 4; v += step) {                  // the v-th free column, ascending
    unsigned used_c = 0;
    for (int q = 0; q < 5; ++q) used_c |= 1u << w.pcol[q];
    int fc = 0, seen = 0;
    for (int c = 0; c < 9; ++c)
      if (!(used_c >> c & 1)) { if (seen == v) fc = c; ++seen; }
    for (int c = 0; c < 9; ++c) w.N[v][c] = (c == fc) ? 1.0 : 0.0;
    for (int q = 0; q < 5; ++q) w.N[v][w.pcol[q]] = -(w.A[w.prow[q]][fc] / w.A[w.prow[q]][w.pcol[q]]);
  }
  g.sync();
  // ---- cubics ----
  for (int q = first; q < 10; q += step) {
    double c[20];
    fp_cubic(w, q, c);
    double big = 0.0;
#pragma unroll
    for (int k = 0; k < 20; ++k) big = __builtin_fmax(big, __builtin_fabs(c[k]));
    const double s = 1.0 / big;                            // every equation at the same scale; a zero equation ends as NaN
#pragma unroll
    for (int k = 0; k < 20; ++k) { w.M0[q][k] = c[k] * s; w.M[q][k] = c[k] * s; }
  }
  g.sync();
  // ---- elim ----
  for (int k = 0; k < 10; ++k) {
    unsigned used = 0;
    for (int q = 0; q < k; ++q) used |= 1u << w.rowof[q];
    int pr = 0;
    double big = -1.0;
    for (int r = 0; r < 10; ++r) {
      const double v = __builtin_fabs(w.M[r][k]);
      const bool take = !(used >> r & 1) && (v > big || big < 0.0);
      if (take) { big = v; pr = r; }
    }
    g.sync();
    for (int r = first; r < 10; r += step) {
      if (r == pr) { w.rowof[k] = pr; continue; }
      const double f = w.M[r][k] / w.M[pr][k];
      w.M[r][k] = 0.0;
      for (int c = k + 1; c < 20; ++c) w.M[r][c] = __builtin_fma(-f, w.M[pr][c], w.M[r][c]);
    }
    g.sync();
  }
  // ---- poly ----
  for (int t = first; t < 3; t += step) {                  // row t: column 4 + 2 t minus z times column 5 + 2 t
    const int re = w.rowof[4 + 2 * t], rf = w.rowof[5 + 2 * t];
    const double ie = 1.0 / w.M[re][4 + 2 * t], jf = 1.0 / w.M[rf][5 + 2 * t];
    for (int v = 0; v < 3; ++v) {
      const int c0 = 10 + 3 * v, len = v == 2 ? 4 : 3;     // x: columns 10 .. 12, y: 13 .. 15, 1: 16 .. 19, highest power first
      for (int p = 0; p < 5; ++p) w.B[t][v][p] = 0.0;
      for (int q = 0; q < len; ++q) {
        const int pw = len - 1 - q;
        w.B[t][v][pw] += w.M[re][c0 + q] * ie;
        w.B[t][v][pw + 1] -= w.M[rf][c0 + q] * jf;
      }
    }
  }
  g.sync();
  for (int t = first; t < 1; t += step) {
    double* p = w.d[0];
    for (int k = 0; k < 11; ++k) p[k] = 0.0;
    for (int r = 0; r < 3; ++r) {                          // det B along its last column
      const int u = (r + 1) % 3, v = (r + 2) % 3;
      double* minor = w.found;                             // seven coefficients; found[] is free until the roots
      for (int k = 0; k < 7; ++k) minor[k] = 0.0;
      fp_poly_mac(w.B[u][0], 3, w.B[v][1], 3, 1.0, minor);
      fp_poly_mac(w.B[u][1], 3, w.B[v][0], 3, -1.0, minor);
      fp_poly_mac(minor, 6, w.B[r][2], 4, 1.0, p);
    }
    for (int k = 1; k < 11; ++k)
      for (int j = 0; j + k < 11; ++j) w.d[k][j] = w.d[k - 1][j + 1] * (double)(j + 1);
    double big = 0.0;
    for (int k = 0; k < 10; ++k) big = __builtin_fmax(big, __builtin_fabs(p[k] / p[10]));
    w.bound = 1.0 + big;                                   // Cauchy; NaN if a coefficient is
  }
  g.sync();
  // ---- roots ----
  for (int level = 9; level >= 0; --level) {
    const int deg = 10 - level;
    for (int i = first; i < deg; i += step) {
      // the ascending roots of the level above that are there: at most deg - 1 of them, in crit[0 ..]
      int m = 0;
      if (level < 9)
        for (int q = 0; q < deg - 1; ++q) m += (w.crit[q] == w.crit[q]);
      double root = __builtin_nan("");
      if (i <= m && w.bound < 1e300) {
        double lo = i == 0 ? -w.bound : w.crit[i - 1], hi = i == m ? w.bound : w.crit[i];
        const double* c = w.d[level];
        const bool neg = fp_horner(c, deg, lo) < 0.0;
        if (neg != (fp_horner(c, deg, hi) < 0.0)) {
          for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
            if ((fp_horner(c, deg, mid) < 0.0) == neg) lo = mid; else hi = mid;
          }
          root = 0.5 * (lo + hi);
          for (int it = 0; it < 2; ++it) {
            const double nx = root - fp_horner(c, deg, root) / fp_horner(w.d[level + 1], deg - 1, root);
            root = (nx >= lo && nx <= hi) ? nx : root;
          }
        }
      }
      w.found[i] = root;
    }
    g.sync();
    for (int i = first; i < 11; i += step) {               // compaction: found[] is ascending where it holds a root
      if (i >= deg) continue;
      int before = 0, total = 0;
      for (int q = 0; q < deg; ++q) { const int has = (w.found[q] == w.found[q]); before += (q < i) ? has : 0; total += has; }
      // crit is read by nobody in this phase; slot `before` is written by the one interval that has that many before it
      if (w.found[i] == w.found[i]) w.crit[before] = w.found[i];
      if (i == 0)
        for (int q = total; q < 11; ++q) w.crit[q] = __builtin_nan("");
    }
    g.sync();
  }
  // ---- finish: crit[] holds the real roots of the polynomial ----
  for (int r = first; r < kFpMaxSol; r += step) {
    double z = w.crit[r], E[9];
    double key = __builtin_nan("");
    if (z == z) {
      double row[3][3];
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int v = 0; v < 3; ++v) row[t][v] = fp_horner(w.B[t][v], v == 2 ? 4 : 3, z);
      double best[3] = {0, 0, 0}, big = -1.0;
#pragma unroll
      for (int t = 0; t < 3; ++t) {                        // the cross product of two rows with the largest norm
        const int u = (t + 1) % 3, v = (t + 2) % 3;
        double c[3];
        c[0] = __builtin_fma(row[u][1], row[v][2], -(row[u][2] * row[v][1]));
        c[1] = __builtin_fma(row[u][2], row[v][0], -(row[u][0] * row[v][2]));
        c[2] = __builtin_fma(row[u][0], row[v][1], -(row[u][1] * row[v][0]));
        const double nn = __builtin_fma(c[2], c[2], __builtin_fma(c[1], c[1], c[0] * c[0]));
        if (nn > big) { big = nn; best[0] = c[0]; best[1] = c[1]; best[2] = c[2]; }
      }
      double x = best[0] / best[2], y = best[1] / best[2];
      for (int it = 0; it < kFpPolish; ++it) fp_polish(w, x, y, z);
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = __builtin_fma(x, w.N[0][k], __builtin_fma(y, w.N[1][k], __builtin_fma(z, w.N[2][k], w.N[3][k])));
      if (fp_canon9(E)) {
        double probe = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) probe += E[k] * 0.0;
        if (probe == 0.0) key = E[0];
      }
    }
    w.key[r] = key;
#pragma unroll
    for (int k = 0; k < 9; ++k) w.sol[r][k] = (key == key) ? E[k] : 0.0;
  }
  g.sync();
  for (int r = first; r < kFpMaxSol; r += step) {          // rank sort by (key, r)
    int rank = 0, total = 0;
    const double mine = w.key[r];
    for (int q = 0; q < kFpMaxSol; ++q) {
      const double other = w.key[q];
      const bool has = other == other;
      total += has;
      rank += (has && (other < mine || (other == mine && q < r))) ? 1 : 0;
    }
    if (mine == mine)
      for (int k = 0; k < 9; ++k) w.E[rank][k] = w.sol[r][k];
    if (r == 0) w.n = total;
  }
  g.sync();
}

}  // namespace sfm
