// sfm_obs_test.h -- the reprojection test of one observation, once: the residual of a projected point s against the key
// (u, v), its scaled square, the inlier predicate.  Whoever judges an observation (sfm_ba_screen, the robust triangulation
// and resection, the residuals of the ragged-track kernels) projects by its own data layout (track_project for a 3x4 P,
// rs_project_pose for [m | t], obs_project_cam for a prepared camera) and continues here: resect then screen, retriangulate
// then cull, free and resident form agree on every decision because they execute the same function.  Below it the test
// of one match against a fundamental matrix (the squared Sampson distance), which every stage of the robust two-view
// geometry calls in the same way, and the test of one match against a homography and its inverse (the transfer error in
// each image), which every stage of the robust homography calls, and the test of one match against a relative pose (in
// front of both cameras, with parallax), which every stage of the relative pose of a verified pair calls, and the model
// of a pose with the signed Sampson residual of one match and its Jacobian row, which the passes and the judge of the
// refinement of a relative pose call, and the test of one 3D-3D correspondence against a similarity, which every stage of
// the robust similarity calls.
//
// Compiled WITHOUT automatic contraction, the FMAs spelled out.  The pragma is lexical and stays in force for the rest of
// the translation unit: include this header outside any namespace and AFTER all code that keeps the compiler's default
// contraction (sfm_ba_terms.h, sfm_cam_fit.h, tri_tracks_linear_kernel) -- a later `contract(on)` is not that default.
#pragma once

#include "sfm_common.h"

#pragma clang fp contract(off)

namespace sfm {

// s = [R^T | t] (X, 1) of a prepared camera, in track_project's operation order
__device__ __forceinline__ void obs_project_cam(const CamPrep& c, double X, double Y, double Z, double* s) {
#pragma unroll
  for (int r = 0; r < 3; ++r) s[r] = __builtin_fma(c.R[6 + r], Z, __builtin_fma(c.R[3 + r], Y, c.R[r] * X)) + c.t[r];
}

__device__ __forceinline__ double obs_inv_depth(const double* s) { return rcp_nr(s[2]); }

// (eu, ev) = s[0:2] / s[2] - (u, v)
__device__ __forceinline__ void obs_residual(const double* s, double u, double v, double& eu, double& ev) {
  const double iz = obs_inv_depth(s);
  eu = __builtin_fma(s[0], iz, -u);
  ev = __builtin_fma(s[1], iz, -v);
}

__device__ __forceinline__ double obs_err2(const double* s, double u, double v, double scale) {
  double eu, ev;
  obs_residual(s, u, v, eu, ev);
  return (scale * scale) * __builtin_fma(ev, ev, eu * eu);
}

// in front of the camera, finite, within the bound; no short circuit: a branch per observation would serialise a walk
__device__ __forceinline__ bool obs_passes(const double* s, double err2, double max_err2) {
  return (s[2] > 0.0) & isfinite(err2) & (err2 <= max_err2);
}

// The test of one MATCH (x_l, y_l) <-> (x_r, y_r) against a fundamental matrix F (row-major, pixel coordinates): with
// a = F (x_l, y_l, 1)^T, b = F^T (x_r, y_r, 1)^T and e = (x_r, y_r, 1) . a, the squared Sampson distance
// d2 = e^2 / (a0^2 + a1^2 + b0^2 + b1^2) in pixels squared; an inlier iff d2 is finite and d2 <= max_err2.  Every stage
// of the robust two-view geometry (sample gate, score, refit, judge) calls this one function; no branch.
__host__ __device__ inline bool twoview_inlier(const double* F, double xl, double yl, double xr, double yr, double max_err2) {
  const double a0 = __builtin_fma(F[0], xl, __builtin_fma(F[1], yl, F[2]));
  const double a1 = __builtin_fma(F[3], xl, __builtin_fma(F[4], yl, F[5]));
  const double a2 = __builtin_fma(F[6], xl, __builtin_fma(F[7], yl, F[8]));
  const double b0 = __builtin_fma(F[0], xr, __builtin_fma(F[3], yr, F[6]));
  const double b1 = __builtin_fma(F[1], xr, __builtin_fma(F[4], yr, F[7]));
  const double e = __builtin_fma(xr, a0, __builtin_fma(yr, a1, a2));
  const double den = __builtin_fma(a0, a0, a1 * a1) + __builtin_fma(b0, b0, b1 * b1);
  const double d2 = (e * e) / den;
  return (bool)((int)(__builtin_isfinite(d2) != 0) & (int)(d2 <= max_err2));
}

// One half of the test of a match against a homography: A (row-major 3x3) maps p to (u, v, w); the transfer error
// against q, times w^2, is compared with max_err2 w^2 -- no division.  True iff the error is finite, w^2 > 0 and it is
// within the bound.
__host__ __device__ inline bool homography_half(const double* A, double px, double py, double qx, double qy, double max_err2) {
  const double u = __builtin_fma(A[0], px, __builtin_fma(A[1], py, A[2]));
  const double v = __builtin_fma(A[3], px, __builtin_fma(A[4], py, A[5]));
  const double w = __builtin_fma(A[6], px, __builtin_fma(A[7], py, A[8]));
  const double eu = __builtin_fma(-qx, w, u), ev = __builtin_fma(-qy, w, v);
  const double lhs = __builtin_fma(eu, eu, ev * ev), rhs = max_err2 * (w * w);
  return (bool)((int)(__builtin_isfinite(lhs) != 0) & (int)(w * w > 0.0) & (int)(lhs <= rhs));
}

// The test of one MATCH (x_l, y_l) <-> (x_r, y_r) against a model HG = (H, G) of 18 doubles, H mapping left to right and
// G right to left (pixel coordinates): an inlier iff the transfer error in each image is at most max_err2 pixels squared.
// Every stage of the robust homography (sample gate, score, refit, judge) calls this one function; no branch.
__host__ __device__ inline bool homography_inlier(const double* HG, double xl, double yl, double xr, double yr, double max_err2) {
  return (bool)((int)homography_half(HG, xl, yl, xr, yr, max_err2) & (int)homography_half(HG + 9, xr, yr, xl, yl, max_err2));
}

// G = adj H by cofactors, not scaled (H G = det H . I): the right-to-left half of a model (H, G) for a caller that
// has H alone (guided matching).  Each cofactor is fma(a, b, -(c * d)) in the operand order written here.
__host__ __device__ inline void homography_adjugate(const double* H, double* G) {
  G[0] = __builtin_fma(H[4], H[8], -(H[5] * H[7]));
  G[1] = __builtin_fma(H[2], H[7], -(H[1] * H[8]));
  G[2] = __builtin_fma(H[1], H[5], -(H[2] * H[4]));
  G[3] = __builtin_fma(H[5], H[6], -(H[3] * H[8]));
  G[4] = __builtin_fma(H[0], H[8], -(H[2] * H[6]));
  G[5] = __builtin_fma(H[2], H[3], -(H[0] * H[5]));
  G[6] = __builtin_fma(H[3], H[7], -(H[4] * H[6]));
  G[7] = __builtin_fma(H[1], H[6], -(H[0] * H[7]));
  G[8] = __builtin_fma(H[0], H[4], -(H[1] * H[3]));
}

// The test of one CORRESPONDENCE a <-> b between two 3D frames against a similarity b ~ s A a + t.  A model under test is
// 12 doubles (Mx, t): Mx row-major with Mx[i][j] = s * A[i][j] (one rounding each), then t.  e = b - (Mx a + t), the squared
// length of e in the units of the b frame; an inlier iff it is finite and <= max_err2.  The back-transfer error times s^2
// is the same quantity: one half suffices.  Every stage of the robust similarity (sample gate, score, refit, judge) and
// the alignment of a resident scene call this one function; no branch.
__host__ __device__ inline bool similarity_inlier(const double* Mt, double ax, double ay, double az, double bx, double by, double bz,
                                                  double max_err2) {
  const double e0 = bx - __builtin_fma(Mt[0], ax, __builtin_fma(Mt[1], ay, __builtin_fma(Mt[2], az, Mt[9])));
  const double e1 = by - __builtin_fma(Mt[3], ax, __builtin_fma(Mt[4], ay, __builtin_fma(Mt[5], az, Mt[10])));
  const double e2 = bz - __builtin_fma(Mt[6], ax, __builtin_fma(Mt[7], ay, __builtin_fma(Mt[8], az, Mt[11])));
  const double lhs = __builtin_fma(e0, e0, __builtin_fma(e1, e1, e2 * e2));
  return (bool)((int)(__builtin_isfinite(lhs) != 0) & (int)(lhs <= max_err2));
}

// P = Rel R, both row-major: P[a][b] = fma(Rel[a][0], R[0][b], fma(Rel[a][1], R[1][b], Rel[a][2] * R[2][b])).  The step forward
// along an edge of a view graph (R_j = Rel R_i) and the first half of its test.
__host__ __device__ inline void rotation_forward(const double* Rel, const double* R, double* P) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      P[3 * a + b] = __builtin_fma(Rel[3 * a], R[b], __builtin_fma(Rel[3 * a + 1], R[3 + b], Rel[3 * a + 2] * R[6 + b]));
}

// Q = Rel^T R: Q[a][b] = fma(Rel[0][a], R[0][b], fma(Rel[1][a], R[1][b], Rel[2][a] * R[2][b])).  The step backward along an
// edge (R_i = Rel^T R_j).
__host__ __device__ inline void rotation_backward(const double* Rel, const double* R, double* Q) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      Q[3 * a + b] = __builtin_fma(Rel[a], R[b], __builtin_fma(Rel[3 + a], R[3 + b], Rel[6 + a] * R[6 + b]));
}

// The test of one EDGE (i, j, Rel) of a view graph against the rotations R_i, R_j of its ends: with P = Rel R_i
// (rotation_forward), lhs = trace(R_j^T P) = sum_ab P[a][b] R_j[a][b], started as P[0] * R_j[0] and continued as
// lhs = fma(P[k], R_j[k], lhs) for k = 1 .. 8 in row-major order; 1 + 2 cos of the residual angle.  An inlier iff lhs is
// finite and lhs >= thr, thr = fma(2, cos_max, 1) formed once by the caller.  No division, no acos.  Every stage of the
// rotation averaging (score, refit, judge) and sfm_rotation_edge_test call this one function; no branch.
__host__ __device__ inline bool rotation_edge_inlier(const double* Ri, const double* Rj, const double* Rel, double thr, double* lhs_out) {
  double P[9];
  rotation_forward(Rel, Ri, P);
  double lhs = P[0] * Rj[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) lhs = __builtin_fma(P[k], Rj[k], lhs);
  *lhs_out = lhs;
  return (bool)((int)(__builtin_isfinite(lhs) != 0) & (int)(lhs >= thr));
}

// The test of one EDGE (i, j) of a view graph with the world direction d from c_i to c_j against the positions c_i, c_j of
// its ends: v = c_j - c_i, dv = fma(d0, v0, fma(d1, v1, d2 * v2)), n2 = fma(v0, v0, fma(v1, v1, v2 * v2)).  An inlier iff dv
// and n2 are finite, dv > 0 and dv * dv >= cc * n2, cc = cos_max * cos_max formed once by the caller.  No division, no
// square root, no acos.  Every stage of the translation averaging (rounds, polish, outputs) and
// sfm_translation_edge_test call this one function; no branch.
__host__ __device__ inline bool translation_edge_inlier(const double* d, const double* ci, const double* cj, double cc, double* dv_out,
                                                        double* n2_out) {
  const double v0 = cj[0] - ci[0], v1 = cj[1] - ci[1], v2 = cj[2] - ci[2];
  const double dv = __builtin_fma(d[0], v0, __builtin_fma(d[1], v1, d[2] * v2));
  const double n2 = __builtin_fma(v0, v0, __builtin_fma(v1, v1, v2 * v2));
  *dv_out = dv;
  *n2_out = n2;
  return (bool)((int)(__builtin_isfinite(dv) != 0) & (int)(__builtin_isfinite(n2) != 0) & (int)(dv > 0.0) & (int)(dv * dv >= cc * n2));
}

// The terms of the test of one MATCH against a relative pose (R, t), X_right = R X_left + t: the rays (a0, a1, 1) of the
// left key and (b0, b1, 1) of the right key in normalised coordinates, a' = R a, p = a'.a', q = b.b, r = a'.b,
// d = p q - r r, and the numerators m1, m2 of the depths along a' and b of the midpoint of the two rays, both over d.
struct PoseTerms { double ap[3], p, q, r, d, m1, m2; };

__host__ __device__ inline PoseTerms pose_terms(const double* R, const double* t, double a0, double a1, double b0, double b1) {
  PoseTerms w;
  w.ap[0] = __builtin_fma(R[0], a0, __builtin_fma(R[1], a1, R[2]));
  w.ap[1] = __builtin_fma(R[3], a0, __builtin_fma(R[4], a1, R[5]));
  w.ap[2] = __builtin_fma(R[6], a0, __builtin_fma(R[7], a1, R[8]));
  w.p = __builtin_fma(w.ap[0], w.ap[0], __builtin_fma(w.ap[1], w.ap[1], w.ap[2] * w.ap[2]));
  w.q = __builtin_fma(b0, b0, __builtin_fma(b1, b1, 1.0));
  w.r = __builtin_fma(w.ap[0], b0, __builtin_fma(w.ap[1], b1, w.ap[2]));
  w.d = __builtin_fma(w.p, w.q, -(w.r * w.r));
  const double bt = __builtin_fma(b0, t[0], __builtin_fma(b1, t[1], t[2]));
  const double at = __builtin_fma(w.ap[0], t[0], __builtin_fma(w.ap[1], t[1], w.ap[2] * t[2]));
  w.m1 = __builtin_fma(w.r, bt, -(w.q * at));
  w.m2 = __builtin_fma(w.p, bt, -(w.r * at));
  return w;
}

// The test of one MATCH against a relative pose: IN FRONT of both cameras (the return value) iff d, m1, m2 are finite and
// d > 0, m1 > 0, m2 > 0 -- no division; *parallax iff in front and not (r > 0 and r r > cos2_min p q), cos2_min the
// squared cosine of the minimum triangulation angle.  Every stage of the relative pose of a verified pair (score, judge)
// and sfm_twoview_pose_test call this one function; no branch.
__host__ __device__ inline bool pose_front(const double* R, const double* t, double a0, double a1, double b0, double b1,
                                           double cos2_min, bool* parallax) {
  const PoseTerms w = pose_terms(R, t, a0, a1, b0, b1);
  const int finite = (int)(__builtin_isfinite(w.d) != 0) & (int)(__builtin_isfinite(w.m1) != 0) & (int)(__builtin_isfinite(w.m2) != 0);
  const int front = finite & (int)(w.d > 0.0) & (int)(w.m1 > 0.0) & (int)(w.m2 > 0.0);
  const int narrow = (int)(w.r > 0.0) & (int)(w.r * w.r > cos2_min * (w.p * w.q));
  *parallax = (bool)(front & (narrow ^ 1));
  return (bool)front;
}

// The model of a relative pose (R, t) for its refinement (sfm_twoview_refine): F = K_r^-T [t]x R K_l^-1 in pixels, not
// scaled, and its five derivatives dF[j] at the origin of the chart (w0, w1, w2, d0, d1) of the pose:
// R(w) = exp([w]x) R, t(d) = (t + d0 b1 + d1 b2) / |.| with b1 = (t x e_k) / |t x e_k|, k the index of the smallest |t_k|
// (the lowest on a tie), and b2 = t x b1.  54 doubles; b1 and b2 are kept for the step.
struct RefineModel { double F[9], dF[5][9], b1[3], b2[3]; };

// out = [v]x M, both row-major.
__host__ __device__ inline void refine_cross_mat(const double* v, const double* M, double* out) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[c] = __builtin_fma(v[1], M[6 + c], -(v[2] * M[3 + c]));
    out[3 + c] = __builtin_fma(v[2], M[c], -(v[0] * M[6 + c]));
    out[6 + c] = __builtin_fma(v[0], M[3 + c], -(v[1] * M[c]));
  }
}

// F = K_r^-T E K_l^-1 by substitution through the upper triangular intrinsics (K[8] = 1): K_r^T Y = E column by column from
// the top, then F K_l = Y row by row from the left; the four divisions by the focal lengths are taken once, as reciprocals.
__host__ __device__ inline void refine_to_pixels(const double* Kl, const double* Kr, const double* E, double* F) {
  const double ir0 = 1.0 / Kr[0], ir4 = 1.0 / Kr[4], il0 = 1.0 / Kl[0], il4 = 1.0 / Kl[4];
  double Y[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    Y[c] = E[c] * ir0;
    Y[3 + c] = __builtin_fma(-Kr[1], Y[c], E[3 + c]) * ir4;
    Y[6 + c] = __builtin_fma(-Kr[5], Y[3 + c], __builtin_fma(-Kr[2], Y[c], E[6 + c]));
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    F[3 * r] = Y[3 * r] * il0;
    F[3 * r + 1] = __builtin_fma(-F[3 * r], Kl[1], Y[3 * r + 1]) * il4;
    F[3 * r + 2] = __builtin_fma(-F[3 * r + 1], Kl[5], __builtin_fma(-F[3 * r], Kl[2], Y[3 * r + 2]));
  }
}

// The basis (b1, b2) of the tangent plane of the unit sphere at t.
__host__ __device__ inline void refine_basis(const double* t, double* b1, double* b2) {
  int k = 0;
  double least = __builtin_fabs(t[0]);
#pragma unroll
  for (int i = 1; i < 3; ++i) {
    const bool less = __builtin_fabs(t[i]) < least;
    k = less ? i : k;
    least = less ? __builtin_fabs(t[i]) : least;
  }
  const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
  double c[3];
  c[0] = __builtin_fma(t[1], ek[2], -(t[2] * ek[1]));
  c[1] = __builtin_fma(t[2], ek[0], -(t[0] * ek[2]));
  c[2] = __builtin_fma(t[0], ek[1], -(t[1] * ek[0]));
  const double nrm = __builtin_sqrt(__builtin_fma(c[2], c[2], __builtin_fma(c[1], c[1], c[0] * c[0])));
#pragma unroll
  for (int i = 0; i < 3; ++i) b1[i] = c[i] / nrm;
  b2[0] = __builtin_fma(t[1], b1[2], -(t[2] * b1[1]));
  b2[1] = __builtin_fma(t[2], b1[0], -(t[0] * b1[2]));
  b2[2] = __builtin_fma(t[0], b1[1], -(t[1] * b1[0]));
}

// One of the six matrices of the model: part 0 is F, part 1 + j is dF[j].  The parts do not depend on each other (six
// lanes form them side by side); part 0 also leaves b1 and b2.
__host__ __device__ inline void refine_model_part(const double* R, const double* t, const double* Kl, const double* Kr, int part,
                                                  RefineModel& m) {
  double b1[3], b2[3], E[9], G[9];
  refine_basis(t, b1, b2);
  if (part == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { m.b1[i] = b1[i]; m.b2[i] = b2[i]; }
    refine_cross_mat(t, R, E);
  } else if (part <= 3) {
    const int j = part - 1;
    const double ej[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    refine_cross_mat(ej, R, G);
    refine_cross_mat(t, G, E);
  } else {
    refine_cross_mat(part == 4 ? b1 : b2, R, E);
  }
  refine_to_pixels(Kl, Kr, E, part == 0 ? m.F : m.dF[part - 1]);
}

__host__ __device__ inline void refine_model(const double* R, const double* t, const double* Kl, const double* Kr, RefineModel& m) {
  for (int part = 0; part < 6; ++part) refine_model_part(R, t, Kl, Kr, part, m);
}

// The residual of one MATCH against the model of a pose and its Jacobian row: with x = (x_l, y_l, 1), y = (x_r, y_r, 1),
// a = F x, b = F^T y, e = y . a and s = a0^2 + a1^2 + b0^2 + b1^2 the signed Sampson distance r = e / sqrt(s) in pixels,
// and J[j] = (y . dF_j x) / sqrt(s) - (e / s^(3/2)) (a0 da0 + a1 da1 + b0 db0 + b1 db1), da = dF_j x, db = dF_j^T y.  J may be
// null.  The pass and the judge of sfm_twoview_refine and sfm_twoview_refine_test call this one function; no branch on the
// data.
__host__ __device__ inline double refine_residual(const double* F, const double (*dF)[9], double xl, double yl, double xr, double yr,
                                                  double* J) {
  const double a0 = __builtin_fma(F[0], xl, __builtin_fma(F[1], yl, F[2]));
  const double a1 = __builtin_fma(F[3], xl, __builtin_fma(F[4], yl, F[5]));
  const double a2 = __builtin_fma(F[6], xl, __builtin_fma(F[7], yl, F[8]));
  const double b0 = __builtin_fma(F[0], xr, __builtin_fma(F[3], yr, F[6]));
  const double b1 = __builtin_fma(F[1], xr, __builtin_fma(F[4], yr, F[7]));
  const double e = __builtin_fma(xr, a0, __builtin_fma(yr, a1, a2));
  const double s = __builtin_fma(a0, a0, a1 * a1) + __builtin_fma(b0, b0, b1 * b1);
  const double root = __builtin_sqrt(s);
  const double r = e / root;
  if (J) {
    const double inv = 1.0 / root, q = r / s;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const double* D = dF[j];
      const double da0 = __builtin_fma(D[0], xl, __builtin_fma(D[1], yl, D[2]));
      const double da1 = __builtin_fma(D[3], xl, __builtin_fma(D[4], yl, D[5]));
      const double da2 = __builtin_fma(D[6], xl, __builtin_fma(D[7], yl, D[8]));
      const double db0 = __builtin_fma(D[0], xr, __builtin_fma(D[3], yr, D[6]));
      const double db1 = __builtin_fma(D[1], xr, __builtin_fma(D[4], yr, D[7]));
      const double de = __builtin_fma(xr, da0, __builtin_fma(yr, da1, da2));
      const double g = __builtin_fma(a0, da0, __builtin_fma(a1, da1, __builtin_fma(b0, db0, b1 * db1)));
      J[j] = __builtin_fma(-q, g, de * inv);
    }
  }
  return r;
}

}  // namespace sfm
