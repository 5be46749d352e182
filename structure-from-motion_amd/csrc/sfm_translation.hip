// sfm_translation.hip — translation averaging: view positions from the directions of a view graph, rotations known (gfx950).
//
// From the unit translations on the edges of a view graph, some of them wrong, and the absolute rotations of its views, one
// position per view and the verdict on every edge.  The rule is stated in sfm_hip.h, block "translation averaging".  One
// graph per call; the stages:
//   adjacency  the view-major list of the 2 E edge ends (view_adjacency of sfm_view_graph.h)
//   verify     the _dev form only: the lowest view whose non-zero R fails verify_rotation (check_rotations_dev)
//   direct     a lane per edge: d_e = -R_j^T t_e normalised, the used flag, the weights and lengths of round 0
//   conn       one workgroup: breadth-first levels (graph_levels) from root over the edges that take part (w_e > 0) or over
//              a byte mask
//   solve      the hot path, one workgroup per solve: the diagonal blocks, their inverses and the right-hand side per view
//              over its adjacency, block-Jacobi CG with q = A p formed on the fly from d_e and w_e (nothing of size E x 9 is
//              stored), every dot product by block_dot, the convergence test; then the edge pass:
//              the verdicts, the count, the cost, the weights and lengths of the next solve, and for the polish the stand
//              decision, all on the device
//   output     one workgroup: the outputs
// No floating-point value is accumulated with an atomic; the counts are integers.
#include <cmath>

#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_view_graph.h"

namespace sfm {

constexpr int kTrBlock = 1024;               // the one workgroup of solve and output
constexpr int kTrConnThreads = 256;

// state words of a call on the device
enum { kTsNoModel = 0, kTsCount = 1, kTsFlags = 2, kTsWords = 3 };
enum { kTrRound = 0, kTrLastRound = 1, kTrPolish = 2 };

struct TrArgs {
  int V, E, root;
  const int* edges;             // [E][2] = (i, j); read as the 2 E keys of the adjacency
  const double* R;              // [V][9]
  const double* t;              // [E][3]
  const unsigned char* edge_mask;      // [E] or null
  const int* adj_ptr;           // [V + 1]
  const int* adj;               // [2 E] entries x = 2 e + dir of every view, ascending
  double cc, sigma2, mu, om;    // cos_max^2, 2 - 2 cos_max, mu, 1 - mu
  int rounds, polish, cg_max;
  double cg_tol2;
  int* st;                      // [kTsWords]
  unsigned char* used;          // [E]
  double* d;                    // [E][3]
  double* w;                    // [E] weights of the next solve
  double* l;                    // [E] target lengths of the next solve
  unsigned char* mask;          // [E] inliers of the standing model
  unsigned char* mask_try;      // [E] inliers of the polish
  int* reach;                   // [V] depth from root over the used edges (-1: unreached)
  int* conn;                    // [V] depth from root over the edges of the next solve, then over the final inliers
  double* C;                    // [V][3] the standing positions
  double* vec;                  // [6][3 V]: b, x, r, p, q, z
  double* dinv;                 // [V][6] inverse diagonal blocks (00 01 02 11 12 22); zeros for a view that is not free
  double* C_out;                // [V][3]
  unsigned char* edge_inlier;   // [E] or null
  double* edge_cos;             // [E] or null
  double* edge_len;             // [E] or null
  int* view_status;             // [V] or null
  int* n_inliers;               // [1] or null
  int* status;                  // [1] or null
  unsigned long long* summary;  // [6] or null
  double* log;                  // [rounds + 2][4] or null
};

// ---------------------------------------------------------------------------------------------
// direct: step 1, and the weights and lengths of round 0
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transavg_direct_kernel(TrArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  const int i = a.edges[2 * e], j = a.edges[2 * e + 1];
  double Ri[9], Rj[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { Ri[k] = a.R[(size_t)i * 9 + k]; Rj[k] = a.R[(size_t)j * 9 + k]; }
  const double t0 = a.t[3 * e], t1 = a.t[3 * e + 1], t2 = a.t[3 * e + 2];
  const double tt = __builtin_fma(t0, t0, __builtin_fma(t1, t1, t2 * t2));
  double u[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) u[c] = -__builtin_fma(Rj[c], t0, __builtin_fma(Rj[3 + c], t1, Rj[6 + c] * t2));
  const double m = __builtin_fma(u[0], u[0], __builtin_fma(u[1], u[1], u[2] * u[2])), len = sqrt(m);
  const bool used = (a.edge_mask == nullptr || a.edge_mask[e] != 0) && has_rotation(Ri) && has_rotation(Rj) &&
                    __builtin_isfinite(tt) && tt > 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.d[3 * e + c] = used ? u[c] / len : 0.0;
  a.used[e] = used ? 1 : 0;
  a.w[e] = used ? 1.0 : 0.0;
  a.l[e] = 1.0;
  a.mask[e] = 0;
}

// ---------------------------------------------------------------------------------------------
// conn: the views joined to root over the edges with w_e > 0 (w != null) or with a non-zero byte (mask)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrConnThreads) void transavg_conn_kernel(TrArgs a, const double* w, const unsigned char* mask, int* depth,
                                                                       int flag_root) {
  if (a.st[kTsNoModel]) return;
  const bool any = graph_levels<kTrConnThreads>(a.V, a.root, depth, [&](int v, int lev) {
    bool hit = false;
    for (int k = a.adj_ptr[v]; k < a.adj_ptr[v + 1] && !hit; ++k) {
      const int x = a.adj[k], e = x >> 1;
      if (w ? !(w[e] > 0.0) : !mask[e]) continue;
      hit = depth[a.edges[x ^ 1]] == lev - 1;
    }
    return hit;
  });
  if (flag_root && !any && threadIdx.x == 0) a.st[kTsNoModel] = 1;      // root has no used edge (or no rotation: then none of its edges is used)
}

// ---------------------------------------------------------------------------------------------
// solve: one solve of the rule and the edge pass after it, one workgroup
// ---------------------------------------------------------------------------------------------
// z = B_e y = w (y - (1 - mu) d (d . y)), added onto acc
__device__ __forceinline__ void tr_edge_block(const double* d, double w, double om, double y0, double y1, double y2, double* acc) {
  const double g = om * __builtin_fma(d[0], y0, __builtin_fma(d[1], y1, d[2] * y2));
  acc[0] += w * __builtin_fma(-g, d[0], y0);
  acc[1] += w * __builtin_fma(-g, d[1], y1);
  acc[2] += w * __builtin_fma(-g, d[2], y2);
}

// (A u)_v of a free view over its adjacency in adjacency order; u holds zeros (or held positions) on views that are not free
__device__ __forceinline__ void tr_apply(const TrArgs& a, const double* u, int v, double* out) {
  out[0] = 0.0; out[1] = 0.0; out[2] = 0.0;
  const double u0 = u[3 * (size_t)v], u1 = u[3 * (size_t)v + 1], u2 = u[3 * (size_t)v + 2];
  for (int k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
    const int x = a.adj[k], e = x >> 1;
    const double w = a.w[e];
    if (!(w > 0.0)) continue;
    const int o = a.edges[x ^ 1];
    const double d[3] = {a.d[3 * (size_t)e], a.d[3 * (size_t)e + 1], a.d[3 * (size_t)e + 2]};
    tr_edge_block(d, w, a.om, u0 - u[3 * (size_t)o], u1 - u[3 * (size_t)o + 1], u2 - u[3 * (size_t)o + 2], out);
  }
}

__global__ __launch_bounds__(kTrBlock) void transavg_solve_kernel(TrArgs a, int row, int mode) {
  __shared__ double red[kTrBlock / 64];
  __shared__ double total;
  __shared__ int lds_total;
  if (a.st[kTsNoModel]) return;
  const int tid = threadIdx.x, V = a.V;
  const size_t n3 = (size_t)3 * V;
  double *vb = a.vec, *vx = a.vec + n3, *vr = a.vec + 2 * n3, *vp = a.vec + 3 * n3, *vq = a.vec + 4 * n3, *vz = a.vec + 5 * n3;
  for (size_t k = tid; k < n3; k += kTrBlock) vx[k] = a.C[k];
  __syncthreads();
  // per free view, over its adjacency in adjacency order: the diagonal block and its inverse, the right-hand side, r = b - A x
  for (int v = tid; v < V; v += kTrBlock) {
    double b[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, inv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.conn[v] > 0) {
      double D00 = 0.0, D01 = 0.0, D02 = 0.0, D11 = 0.0, D12 = 0.0, D22 = 0.0;
      for (int k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
        const int x = a.adj[k], e = x >> 1;
        const double w = a.w[e];
        if (!(w > 0.0)) continue;
        const double d0 = a.d[3 * (size_t)e], d1 = a.d[3 * (size_t)e + 1], d2 = a.d[3 * (size_t)e + 2];
        D00 += w * __builtin_fma(-a.om, d0 * d0, 1.0); D01 += w * __builtin_fma(-a.om, d0 * d1, 0.0); D02 += w * __builtin_fma(-a.om, d0 * d2, 0.0);
        D11 += w * __builtin_fma(-a.om, d1 * d1, 1.0); D12 += w * __builtin_fma(-a.om, d1 * d2, 0.0); D22 += w * __builtin_fma(-a.om, d2 * d2, 1.0);
        const double h = ((w * a.mu) * a.l[e]) * ((x & 1) ? 1.0 : -1.0);
        b[0] += h * d0; b[1] += h * d1; b[2] += h * d2;
      }
      const double c00 = D11 * D22 - D12 * D12, c01 = D02 * D12 - D01 * D22, c02 = D01 * D12 - D02 * D11;
      const double c11 = D00 * D22 - D02 * D02, c12 = D01 * D02 - D00 * D12, c22 = D00 * D11 - D01 * D01;
      const double det = __builtin_fma(D00, c00, __builtin_fma(D01, c01, D02 * c02));
      inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det; inv[3] = c11 / det; inv[4] = c12 / det; inv[5] = c22 / det;
      double ax[3];
      tr_apply(a, vx, v, ax);
      r[0] = b[0] - ax[0]; r[1] = b[1] - ax[1]; r[2] = b[2] - ax[2];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) a.dinv[6 * (size_t)v + c] = inv[c];
    const double z[3] = {__builtin_fma(inv[0], r[0], __builtin_fma(inv[1], r[1], inv[2] * r[2])),
                         __builtin_fma(inv[1], r[0], __builtin_fma(inv[3], r[1], inv[4] * r[2])),
                         __builtin_fma(inv[2], r[0], __builtin_fma(inv[4], r[1], inv[5] * r[2]))};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t k = 3 * (size_t)v + c;
      vb[k] = b[c]; vr[k] = r[c]; vz[k] = z[c]; vp[k] = z[c];
    }
  }
  __syncthreads();
  auto dot3 = [&](const double* x, const double* y, int v) {
    return __builtin_fma(x[3 * (size_t)v + 2], y[3 * (size_t)v + 2], __builtin_fma(x[3 * (size_t)v + 1], y[3 * (size_t)v + 1], x[3 * (size_t)v] * y[3 * (size_t)v]));
  };
  const double bb = block_dot<kTrBlock>(V, [&](int v) { return dot3(vb, vb, v); }, red, &total);
  const double rr0 = block_dot<kTrBlock>(V, [&](int v) { return dot3(vr, vr, v); }, red, &total);
  double rz = block_dot<kTrBlock>(V, [&](int v) { return dot3(vr, vz, v); }, red, &total);
  bool done = rr0 <= a.cg_tol2 * bb;
  int iters = 0;
  for (int it = 0; it < a.cg_max && !done; ++it) {
    // q = A p: a view that is not free carries p = 0
    for (int v = tid; v < V; v += kTrBlock) {
      double q[3] = {0.0, 0.0, 0.0};
      if (a.conn[v] > 0) tr_apply(a, vp, v, q);
#pragma unroll
      for (int c = 0; c < 3; ++c) vq[3 * (size_t)v + c] = q[c];
    }
    __syncthreads();
    const double pq = block_dot<kTrBlock>(V, [&](int v) { return dot3(vp, vq, v); }, red, &total);
    const double alpha = rz / pq;
    for (int v = tid; v < V; v += kTrBlock) {
      const double* inv = a.dinv + 6 * (size_t)v;
      double r[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t k = 3 * (size_t)v + c;
        vx[k] = __builtin_fma(alpha, vp[k], vx[k]);
        r[c] = __builtin_fma(-alpha, vq[k], vr[k]);
        vr[k] = r[c];
      }
      vz[3 * (size_t)v] = __builtin_fma(inv[0], r[0], __builtin_fma(inv[1], r[1], inv[2] * r[2]));
      vz[3 * (size_t)v + 1] = __builtin_fma(inv[1], r[0], __builtin_fma(inv[3], r[1], inv[4] * r[2]));
      vz[3 * (size_t)v + 2] = __builtin_fma(inv[2], r[0], __builtin_fma(inv[4], r[1], inv[5] * r[2]));
    }
    __syncthreads();
    ++iters;
    const double rr = block_dot<kTrBlock>(V, [&](int v) { return dot3(vr, vr, v); }, red, &total);
    if (rr <= a.cg_tol2 * bb) { done = true; break; }
    const double rz_new = block_dot<kTrBlock>(V, [&](int v) { return dot3(vr, vz, v); }, red, &total);
    const double beta = rz_new / rz;
    rz = rz_new;
    for (size_t k = tid; k < n3; k += kTrBlock) vp[k] = __builtin_fma(beta, vp[k], vz[k]);
    __syncthreads();
  }
  if (!done && tid == 0) atomicOr(&a.st[kTsFlags], SFM_TRANSAVG_CG_LIMIT);
  // every free position finite?  Round 0 without: no model.  A polish without: it does not stand.
  int bad = 0;
  for (int v = tid; v < V; v += kTrBlock) {
    if (!(a.conn[v] > 0)) continue;
    const double probe = vx[3 * (size_t)v] * 0.0 + vx[3 * (size_t)v + 1] * 0.0 + vx[3 * (size_t)v + 2] * 0.0;
    bad |= probe == 0.0 ? 0 : 1;
  }
  bad = __syncthreads_or(bad);
  if (row == 0 && bad) { if (tid == 0) a.st[kTsNoModel] = 1; return; }
  // the edge pass over the positions of this solve: verdict, cost under the weights of this solve, the next weights and lengths
  unsigned char* verdict = mode == kTrPolish ? a.mask_try : a.mask;
  int mine = 0;
  const double cost = block_dot<kTrBlock>(a.E, [&](int e) {
    if (!a.used[e]) { verdict[e] = 0; return 0.0; }
    const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
    const double d[3] = {a.d[3 * (size_t)e], a.d[3 * (size_t)e + 1], a.d[3 * (size_t)e + 2]};
    double dv, n2;
    const bool in = translation_edge_inlier(d, vx + 3 * (size_t)i, vx + 3 * (size_t)j, a.cc, &dv, &n2);
    verdict[e] = in ? 1 : 0;
    mine += in;
    const double w = a.w[e], gap = dv - a.l[e];
    const double term = w > 0.0 ? w * ((n2 - dv * dv) + a.mu * (gap * gap)) : 0.0;
    if (mode != kTrPolish) {
      double w_next;
      if (mode == kTrLastRound) {
        w_next = in ? 1.0 : 0.0;
      } else {
        const double s2 = (__builtin_isfinite(n2) && n2 > 0.0) ? 2.0 - 2.0 * (dv / sqrt(n2)) : 2.0;
        w_next = 1.0 / (1.0 + s2 / a.sigma2);
      }
      a.w[e] = w_next;
      a.l[e] = dv > 0.0 ? dv : 1.0;
    }
    return term;
  }, red, &total);
  const int count = block_sum_int(mine, &lds_total);
  const bool stands = mode != kTrPolish || (!bad && count >= a.st[kTsCount]);
  __syncthreads();                                           // every thread has read the standing count
  if (stands) {
    for (size_t k = tid; k < n3; k += kTrBlock) a.C[k] = vx[k];
    if (mode == kTrPolish)
      for (int e = tid; e < a.E; e += kTrBlock) a.mask[e] = a.mask_try[e];
  }
  if (tid != 0) return;
  if (stands) a.st[kTsCount] = count; else atomicOr(&a.st[kTsFlags], SFM_TRANSAVG_KEPT_ROUNDS);
  if (a.log) {
    double* lg = a.log + 4 * (size_t)row;
    lg[0] = (double)count; lg[1] = (double)iters; lg[2] = stands ? 1.0 : 0.0; lg[3] = cost;
  }
}

// ---------------------------------------------------------------------------------------------
// output: step 6
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrBlock) void transavg_output_kernel(TrArgs a) {
  __shared__ int lds_sums[6];
  const int tid = threadIdx.x;
  const bool model = a.st[kTsNoModel] == 0;
  const double nan = __builtin_nan("");
  int n_in = 0, n_out = 0, n_pos = 0, n_norot = 0, n_unreached = 0, n_held = 0;
  for (int e = tid; e < a.E; e += kTrBlock) {
    const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
    const bool used = a.used[e] != 0;
    const double d[3] = {a.d[3 * (size_t)e], a.d[3 * (size_t)e + 1], a.d[3 * (size_t)e + 2]};
    double dv, n2, ci[3], cj[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { ci[c] = model ? a.C[3 * (size_t)i + c] : 0.0; cj[c] = model ? a.C[3 * (size_t)j + c] : 0.0; }
    const bool in = translation_edge_inlier(d, ci, cj, a.cc, &dv, &n2) && used && model;
    if (a.edge_inlier) a.edge_inlier[e] = in ? 1 : 0;
    if (a.edge_cos) a.edge_cos[e] = (used && __builtin_isfinite(n2) && n2 > 0.0) ? dv / sqrt(n2) : nan;
    if (a.edge_len) a.edge_len[e] = used ? dv : nan;
    n_in += in;
    n_out += used && !in;
  }
  for (int v = tid; v < a.V; v += kTrBlock) {
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R[(size_t)v * 9 + k];
    const bool norot = !has_rotation(R), unreached = a.reach[v] < 0, has = model && !unreached, held = !(model && a.conn[v] >= 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.C_out[3 * (size_t)v + c] = has ? a.C[3 * (size_t)v + c] : 0.0;
    if (a.view_status)
      a.view_status[v] = (norot ? SFM_TRANSAVG_NO_ROTATION : 0) | (unreached ? SFM_TRANSAVG_UNREACHED : 0) | (held ? SFM_TRANSAVG_HELD : 0);
    n_pos += has; n_norot += norot; n_unreached += unreached; n_held += held;
  }
  int n[6] = {n_pos, n_norot, n_unreached, n_held, n_in, n_out};       // the order of the summary
  block_sums(n, lds_sums);
  if (tid != 0) return;
  if (a.n_inliers) *a.n_inliers = n[4];
  if (a.status) *a.status = model ? a.st[kTsFlags] : SFM_TRANSAVG_NO_MODEL;
  if (a.summary) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.summary[k] = n[k];
  }
  if (a.log && !model)
    for (int k = 0; k < 4 * (a.rounds + 2); ++k) a.log[k] = 0.0;
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int tr_check(const char* who, int V, long long E, const int* edges, const double* R, const double* t, int root,
                    double cos_max, double mu, int rounds, int polish, double cg_tol, int cg_max, const void* C_out) {
  if (V < 2 || E < 1 || E >= (1LL << 30)) { set_error("%s: bad sizes V=%d E=%lld (V >= 2, 1 <= E < 2^30)", who, V, E); return SFM_E_SHAPE; }
  if (edges == nullptr || R == nullptr || t == nullptr || C_out == nullptr) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  if (root < 0 || root >= V) { set_error("%s: root = %d must be in 0 .. %d", who, root, V - 1); return SFM_E_SHAPE; }
  if (!(cos_max > 0.0 && cos_max <= 1.0)) { set_error("%s: cos_max = %g must be in (0, 1]", who, cos_max); return SFM_E_SHAPE; }
  if (!(mu >= 0.0 && mu <= 1.0)) { set_error("%s: mu = %g must be in (0, 1] (0 = 0.01)", who, mu); return SFM_E_SHAPE; }
  if (rounds < 0) { set_error("%s: rounds = %d must be >= 0", who, rounds); return SFM_E_SHAPE; }
  if (polish != 0 && polish != 1) { set_error("%s: polish = %d must be 0 or 1", who, polish); return SFM_E_SHAPE; }
  if (!(cg_tol > 0.0 && cg_tol < 1.0)) { set_error("%s: cg_tol = %g must be in (0, 1)", who, cg_tol); return SFM_E_SHAPE; }
  if (cg_max < 1) { set_error("%s: cg_max = %d must be >= 1", who, cg_max); return SFM_E_SHAPE; }
  return view_graph_check_edges(who, V, E, edges);
}

struct TrWork {
  DevBuf<int> adj_ptr, adj, st, reach, conn;
  DevBuf<double> d, w, l, C, vec, dinv;
  DevBuf<unsigned char> used, mask, mask_try;
};

// The arguments of the kernels, but for the work buffers: the inputs and outputs of either form, on the device.
static TrArgs tr_args(int V, long long E, const int* d_edges, const double* d_R, const double* d_t, const unsigned char* d_edge_mask, int root,
                      double cos_max, double mu, int rounds, int polish, double cg_tol, int cg_max, double* C_out, unsigned char* edge_inlier,
                      double* edge_cos, double* edge_len, int* view_status, int* n_inliers, int* status, int64_t* summary, double* log) {
  TrArgs a = {};
  a.V = V; a.E = (int)E; a.root = root; a.edges = d_edges; a.R = d_R; a.t = d_t; a.edge_mask = d_edge_mask;
  if (mu == 0.0) mu = 0.01;
  a.cc = cos_max * cos_max; a.sigma2 = 2.0 - 2.0 * cos_max; a.mu = mu; a.om = 1.0 - mu;
  a.rounds = rounds; a.polish = polish; a.cg_max = cg_max; a.cg_tol2 = cg_tol * cg_tol;
  a.C_out = C_out; a.edge_inlier = edge_inlier; a.edge_cos = edge_cos; a.edge_len = edge_len; a.view_status = view_status;
  a.n_inliers = n_inliers; a.status = status; a.summary = reinterpret_cast<unsigned long long*>(summary); a.log = log;
  return a;
}

// The one body of both forms: checked arguments and device pointers in, everything enqueued on s.
static int tr_run(TrArgs a, TrWork& w, hipStream_t s) {
  const int V = a.V, E = a.E;
  SFM_TRY(w.st.alloc(kTsWords, s));
  const int st0[kTsWords] = {0, 0, 0};
  SFM_HIP(hipMemcpyAsync(w.st.p, st0, sizeof(st0), hipMemcpyHostToDevice, s));
  a.st = w.st.p;
  SFM_TRY(view_adjacency(V, E, a.edges, w.adj_ptr, w.adj, s));
  a.adj_ptr = w.adj_ptr.p; a.adj = w.adj.p;
  SFM_TRY(w.reach.alloc(V, s)); SFM_TRY(w.conn.alloc(V, s)); SFM_TRY(w.used.alloc(E, s)); SFM_TRY(w.mask.alloc(E, s)); SFM_TRY(w.mask_try.alloc(E, s));
  SFM_TRY(w.d.alloc((size_t)3 * E, s)); SFM_TRY(w.w.alloc(E, s)); SFM_TRY(w.l.alloc(E, s));
  SFM_TRY(w.C.alloc((size_t)3 * V, s)); SFM_TRY(w.vec.alloc((size_t)18 * V, s)); SFM_TRY(w.dinv.alloc((size_t)6 * V, s));
  a.reach = w.reach.p; a.conn = w.conn.p; a.used = w.used.p; a.mask = w.mask.p; a.mask_try = w.mask_try.p;
  a.d = w.d.p; a.w = w.w.p; a.l = w.l.p; a.C = w.C.p; a.vec = w.vec.p; a.dinv = w.dinv.p;
  SFM_HIP(hipMemsetAsync(a.C, 0, sizeof(double) * 3 * (size_t)V, s));
  SFM_HIP(hipMemsetAsync(a.reach, 0xFF, sizeof(int) * (size_t)V, s));
  SFM_HIP(hipMemsetAsync(a.conn, 0xFF, sizeof(int) * (size_t)V, s));
  if (a.log) SFM_HIP(hipMemsetAsync(a.log, 0, sizeof(double) * 4 * (size_t)(a.rounds + 2), s));
  transavg_direct_kernel<<<(unsigned)((E + 255) / 256), 256, 0, s>>>(a);
  // what the used edges reach from root; a root without a used edge has no model
  transavg_conn_kernel<<<1, kTrConnThreads, 0, s>>>(a, a.w, nullptr, a.reach, 1);
  for (int r = 0; r <= a.rounds; ++r) {
    transavg_conn_kernel<<<1, kTrConnThreads, 0, s>>>(a, a.w, nullptr, a.conn, 0);
    transavg_solve_kernel<<<1, kTrBlock, 0, s>>>(a, r, r == a.rounds ? kTrLastRound : kTrRound);
  }
  if (a.polish) {
    transavg_conn_kernel<<<1, kTrConnThreads, 0, s>>>(a, a.w, nullptr, a.conn, 0);
    transavg_solve_kernel<<<1, kTrBlock, 0, s>>>(a, a.rounds + 1, kTrPolish);
  }
  transavg_conn_kernel<<<1, kTrConnThreads, 0, s>>>(a, nullptr, a.mask, a.conn, 0);
  transavg_output_kernel<<<1, kTrBlock, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_translation_edge_test(const double* d, const double* ci, const double* cj, double cos_max, double* dv_out, double* n2_out) {
  if (d == nullptr || ci == nullptr || cj == nullptr) return 0;
  double dv, n2;
  const bool in = translation_edge_inlier(d, ci, cj, cos_max * cos_max, &dv, &n2);
  if (dv_out) *dv_out = dv;
  if (n2_out) *n2_out = n2;
  return in ? 1 : 0;
}

int sfm_translation_average_dev(int V, int64_t E, const int* edges, const double* d_R, const double* d_t, const unsigned char* d_edge_mask,
                                int root, double cos_max, double mu, int rounds, int polish, double cg_tol, int cg_max, double* d_C_out,
                                unsigned char* d_edge_inlier, double* d_edge_cos, double* d_edge_len, int* d_view_status, int* d_n_inliers,
                                int* d_status, int64_t* d_summary, double* d_log, void* hip_stream) {
  const char* who = "sfm_translation_average_dev";
  SFM_TRY(tr_check(who, V, E, edges, d_R, d_t, root, cos_max, mu, rounds, polish, cg_tol, cg_max, d_C_out));
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  SFM_TRY(check_rotations_dev(who, "R of view %lld", V, d_R, true, s));
  DevBuf<int> dE;                       // the checked host copy: no kernel indexes with a value that was not looked at
  SFM_TRY(dE.upload(edges, 2 * (size_t)E, s));
  const TrArgs a = tr_args(V, E, dE.p, d_R, d_t, d_edge_mask, root, cos_max, mu, rounds, polish, cg_tol, cg_max, d_C_out, d_edge_inlier,
                           d_edge_cos, d_edge_len, d_view_status, d_n_inliers, d_status, d_summary, d_log);
  TrWork w;
  SFM_TRY(tr_run(a, w, s));
  return stream_sync(s);
}

int sfm_translation_average(int V, int64_t E, const int* edges, const double* R, const double* t, const unsigned char* edge_mask, int root,
                            double cos_max, double mu, int rounds, int polish, double cg_tol, int cg_max, double* C_out,
                            unsigned char* edge_inlier, double* edge_cos, double* edge_len, int* view_status, int* n_inliers, int* status,
                            int64_t* summary, double* log) {
  const char* who = "sfm_translation_average";
  SFM_TRY(tr_check(who, V, E, edges, R, t, root, cos_max, mu, rounds, polish, cg_tol, cg_max, C_out));
  SFM_TRY(check_rotations_host(who, "R of view %lld", V, R, true));
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)V, m = (size_t)E;
  DevBuf<int> dE;
  DevBuf<double> dR, dT;
  DevBuf<unsigned char> dMask;
  HostOut<double> oC, oCos, oLen, oLog;
  HostOut<unsigned char> oIn;
  HostOut<int> oView, oN, oStatus;
  HostOut<int64_t> oSum;
  TrWork w;
  SFM_TRY(dE.upload(edges, 2 * m, s)); SFM_TRY(dR.upload(R, 9 * v, s)); SFM_TRY(dT.upload(t, 3 * m, s));
  SFM_TRY(dMask.upload_if(edge_mask, m, s));
  SFM_TRY(oC.want(C_out, 3 * v, s)); SFM_TRY(oCos.want(edge_cos, m, s)); SFM_TRY(oLen.want(edge_len, m, s)); SFM_TRY(oIn.want(edge_inlier, m, s));
  SFM_TRY(oView.want(view_status, v, s)); SFM_TRY(oN.want(n_inliers, 1, s)); SFM_TRY(oStatus.want(status, 1, s));
  SFM_TRY(oSum.want(summary, 6, s)); SFM_TRY(oLog.want(log, 4 * (size_t)(rounds + 2), s));
  const TrArgs a = tr_args(V, E, dE.p, dR.p, dT.p, dMask.p, root, cos_max, mu, rounds, polish, cg_tol, cg_max, oC.dev(), oIn.dev(),
                           oCos.dev(), oLen.dev(), oView.dev(), oN.dev(), oStatus.dev(), oSum.dev(), oLog.dev());
  SFM_TRY(tr_run(a, w, s));
  SFM_TRY(oC.fetch(s)); SFM_TRY(oCos.fetch(s)); SFM_TRY(oLen.fetch(s)); SFM_TRY(oIn.fetch(s)); SFM_TRY(oView.fetch(s));
  SFM_TRY(oN.fetch(s)); SFM_TRY(oStatus.fetch(s)); SFM_TRY(oSum.fetch(s)); SFM_TRY(oLog.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
