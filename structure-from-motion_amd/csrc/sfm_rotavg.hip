// sfm_rotavg.hip — rotation averaging: spanning-tree hypotheses of a view graph, inlier refit on the Lie algebra (gfx950).
//
// The seventh robust estimator.  From the relative rotations on the edges of a view graph, some of them wrong, one absolute
// rotation per view and the verdict on every edge.  The rule is stated in sfm_hip.h, block "rotation averaging".  One
// graph per call; the stages:
//   adjacency  the view-major list of the 2 E edge ends (view_adjacency of sfm_view_graph.h)
//   tree       a workgroup per hypothesis: breadth-first levels (graph_levels), a lane per view scanning its own adjacency
//              for neighbours of the previous depth, the smallest (key, e) as parent edge, the rotation formed from the
//              parent's; depths in LDS up to kRotLdsViews views, in global memory beyond.  With an edge mask and no
//              rotations the same kernel gives the connectivity of the refit and of the judge
//   score      the hot path: grid = (blocks of 1 024 edges, slices of the batch's hypotheses); Rel_e and the two indices of
//              four edges per lane stay in registers, the two rotations are gathered, ballots are counted and one integer
//              atomicAdd per workgroup and hypothesis goes out
//   adopt      one workgroup per batch: wave_arg_best over the batch, carried across batches by (count, h); the winner's
//              rotations leave the work buffer through the gauge
//   step       one workgroup per Gauss-Newton step: the logs per edge, the right-hand side and q = L p per view in adjacency
//              order, every dot product by block_dot, Jacobi-preconditioned CG, the exponential update
//   accept     one workgroup per round: the count over all edges, the stand/stop decision, taken on the device
//   judge      the outputs
// No floating-point value is accumulated with an atomic; the counts are integers.
#include <climits>
#include <cmath>
#include <vector>

#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_view_graph.h"

namespace sfm {

constexpr int kRotLdsViews = 4096;            // depths of a tree live in LDS up to here (16 KiB)
constexpr int kRotTreeThreads = 256;
constexpr int kRotScoreThreads = 256, kRotScorePer = 4, kRotScoreEdges = kRotScoreThreads * kRotScorePer;
constexpr int kRotScoreSlices = 64;           // grid.y of the score: hypotheses h = y, y + 64, ... of the batch
constexpr int kRotBlock = 1024;               // the one workgroup of step, accept and judge
constexpr long long kRotWorkCap = 256LL << 20;      // the rotations of a batch of hypotheses stay below this many bytes

// state words of a call on the device
enum { kStCount = 0, kStHyp = 1, kStStopped = 2, kStStood = 3, kStFlags = 4, kStWords = 5 };

struct RotArgs {
  int V, E, root;
  const int* edges;             // [E][2] = (i, j); read as the 2 E keys of the adjacency
  const double* rel;            // [E][9]
  const int* adj_ptr;           // [V + 1]
  const int* adj;               // [2 E] entries x = 2 e + dir of every view, ascending
  double thr;                   // fma(2, cos_max, 1)
  int iters, steps, cg_max;
  double cg_tol2;
  int* st;                      // [kStWords]
  double* R_cur;                // [V][9] the standing model
  double* R_try;                // [V][9] the model of the round
  unsigned char* mask;          // [E] inliers of the standing model
  unsigned char* mask_try;      // [E]
  int* reach;                   // [V] depth from root in the input graph (-1: unreached)
  int* conn;                    // [V] depth from root through the inliers of the standing model (-1: held)
  double* d;                    // [E][3] logs of a step
  double* vec;                  // [6][3 V]: b, x, r, p, q, 1 / degree (one per view, in the first V of its block)
  double* R_out;                // [V][9]
  unsigned char* edge_inlier;   // [E] or null
  double* edge_cos;             // [E] or null
  int* view_status;             // [V] or null
  int* n_inliers;               // [1] or null
  int* best_hyp;                // [1] or null
  int* status;                  // [1] or null
  unsigned long long* summary;  // [6] or null
};

__host__ __device__ inline unsigned long long rot_key(int h, unsigned e) {
  return splitmix64_mix(((unsigned long long)(unsigned)h << 32) | (unsigned long long)e);
}
__host__ __device__ inline int rot_tree_root(int h, int V, int root) { return h == 0 ? root : (int)(rot_key(h, 0xFFFFFFFFu) % (unsigned long long)V); }

__device__ __forceinline__ bool rot_finite9(const double* R) {
  double probe = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) probe += R[k] * 0.0;
  return probe == 0.0;
}

// ---------------------------------------------------------------------------------------------
// tree: hypotheses (rot != null: rotations [nb][V][9], ok [nb]) or connectivity (mask, depth_out)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRotTreeThreads) void rotavg_tree_kernel(RotArgs a, int h0, const unsigned char* mask, const int* gate, int* depth_glob,
                                                                      double* rot, unsigned char* ok, int* depth_out) {
  __shared__ int lds_depth[kRotLdsViews];
  if (gate && (gate[kStStopped] || gate[kStHyp] < 0)) return;      // a connectivity of the refit after the rounds have stopped
  const int tid = threadIdx.x, b = blockIdx.x, h = h0 + b, V = a.V;
  int* depth = V <= kRotLdsViews ? lds_depth : depth_glob + (size_t)b * V;
  double* R = rot ? rot + (size_t)b * V * 9 : nullptr;
  const int r0 = rot_tree_root(h, V, a.root);
  const double nan = __builtin_nan("");
  if (R)
    for (int v = tid; v < V; v += kRotTreeThreads) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[(size_t)v * 9 + k] = v == r0 ? ((k & 3) == 0 ? 1.0 : 0.0) : nan;
    }
  int bad = 0;
  const bool any = graph_levels<kRotTreeThreads>(V, r0, depth, [&](int v, int d) {
    unsigned long long best_key = 0;
    int best_x = -1, best_o = -1;
    for (int k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
      const int x = a.adj[k], e = x >> 1;
      if (mask && !mask[e]) continue;
      const int o = a.edges[x ^ 1];
      if (depth[o] != d - 1) continue;
      const unsigned long long key = h == 0 ? (unsigned long long)e : rot_key(h, (unsigned)e);
      if (best_x < 0 || key < best_key) { best_key = key; best_x = x; best_o = o; }      // ascending e: the first of equal keys stays
    }
    if (best_x < 0) return false;
    if (R) {
      double Rp[9], Rel[9], Rv[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) { Rp[k] = R[(size_t)best_o * 9 + k]; Rel[k] = a.rel[(size_t)(best_x >> 1) * 9 + k]; }
      if (best_x & 1) rotation_forward(Rel, Rp, Rv); else rotation_backward(Rel, Rp, Rv);
#pragma unroll
      for (int k = 0; k < 9; ++k) R[(size_t)v * 9 + k] = Rv[k];
      bad |= rot_finite9(Rv) ? 0 : 1;
    }
    return true;
  });
  bad = __syncthreads_or(bad);
  if (ok && tid == 0) ok[b] = (any && depth[a.root] >= 0 && !bad) ? 1 : 0;
  if (depth_out)
    for (int v = tid; v < V; v += kRotTreeThreads) depth_out[v] = depth[v];
}

// ---------------------------------------------------------------------------------------------
// score: the hot path
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRotScoreThreads) void rotavg_score_kernel(RotArgs a, int nb, const double* rot, const unsigned char* ok, int* counts) {
  __shared__ int wg_cnt[2];
  const int tid = threadIdx.x;
  double Rel[kRotScorePer][9];
  int vi[kRotScorePer], vj[kRotScorePer];
  bool live[kRotScorePer];
#pragma unroll
  for (int k = 0; k < kRotScorePer; ++k) {
    const long long e = (long long)blockIdx.x * kRotScoreEdges + k * kRotScoreThreads + tid;
    live[k] = e < a.E;
    const size_t ee = live[k] ? (size_t)e : 0;
    vi[k] = a.edges[2 * ee]; vj[k] = a.edges[2 * ee + 1];
#pragma unroll
    for (int q = 0; q < 9; ++q) Rel[k][q] = a.rel[9 * ee + q];
  }
  if (tid < 2) wg_cnt[tid] = 0;
  __syncthreads();
  int turn = 0;
  for (int hh = blockIdx.y; hh < nb; hh += gridDim.y) {
    if (!ok[hh]) continue;                                   // the same for the whole workgroup
    const double* R = rot + (size_t)hh * a.V * 9;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kRotScorePer; ++k) {
      double Ri[9], Rj[9], lhs;
#pragma unroll
      for (int q = 0; q < 9; ++q) { Ri[q] = R[(size_t)vi[k] * 9 + q]; Rj[q] = R[(size_t)vj[k] * 9 + q]; }
      const bool in = rotation_edge_inlier(Ri, Rj, Rel[k], a.thr, &lhs) & live[k];
      cnt += __popcll(__ballot(in));
    }
    int* slot = &wg_cnt[turn & 1];
    if ((tid & 63) == 0 && cnt) atomicAdd(slot, cnt);
    __syncthreads();
    // the slot is used again two turns on, after the next turn's barrier: thread 0 has emptied it by then
    if (tid == 0) { const int c = *slot; *slot = 0; if (c) atomicAdd(&counts[hh], c); }
    ++turn;
  }
}

// ---------------------------------------------------------------------------------------------
// adopt: the winner of a batch against the winner so far; its rotations through the gauge
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRotTreeThreads) void rotavg_adopt_kernel(RotArgs a, int h0, int nb, const double* rot, const unsigned char* ok, const int* counts) {
  __shared__ int take;
  const int tid = threadIdx.x;
  if (tid < 64) {
    int best_cnt, best_i;
    wave_arg_best(tid, nb, [&](int i) { return ok[i] != 0; }, [&](int i) { return counts[i]; }, best_cnt, best_i);
    if (tid == 0) {
      // batches come in ascending h: only a larger count replaces the winner so far
      const bool won = best_cnt >= 0 && best_cnt > a.st[kStCount];
      if (won) { a.st[kStCount] = best_cnt; a.st[kStHyp] = h0 + best_i; }
      take = won ? best_i : -1;
    }
  }
  __syncthreads();
  if (take < 0) return;
  const double* R = rot + (size_t)take * a.V * 9;
  double Rr[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rr[k] = R[(size_t)a.root * 9 + k];
  for (int v = tid; v < a.V; v += kRotTreeThreads) {
    double Rv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rv[k] = R[(size_t)v * 9 + k];
    // the gauge: G = R_v R_root^T, G[r][c] = fma(R_v[r][0], R_root[c][0], fma(R_v[r][1], R_root[c][1], R_v[r][2] * R_root[c][2]));
    // the root itself takes the identity
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double g = __builtin_fma(Rv[3 * r], Rr[3 * c], __builtin_fma(Rv[3 * r + 1], Rr[3 * c + 1], Rv[3 * r + 2] * Rr[3 * c + 2]));
        a.R_cur[(size_t)v * 9 + 3 * r + c] = v == a.root ? (r == c ? 1.0 : 0.0) : g;
      }
  }
}

// The inliers of the winner: the set S of the first round and, with iters = 0, of the judge.
__global__ __launch_bounds__(256) void rotavg_mask_kernel(RotArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  double Ri[9], Rj[9], Rel[9], lhs;
  const int i = a.edges[2 * e], j = a.edges[2 * e + 1];
#pragma unroll
  for (int k = 0; k < 9; ++k) { Ri[k] = a.R_cur[(size_t)i * 9 + k]; Rj[k] = a.R_cur[(size_t)j * 9 + k]; Rel[k] = a.rel[(size_t)e * 9 + k]; }
  a.mask[e] = (a.st[kStHyp] >= 0 && rotation_edge_inlier(Ri, Rj, Rel, a.thr, &lhs)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void rotavg_copy_kernel(RotArgs a) {      // R_try <- R_cur at the start of a round
  if (a.st[kStStopped] || a.st[kStHyp] < 0) return;
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k < (size_t)a.V * 9) a.R_try[k] = a.R_cur[k];
}

// ---------------------------------------------------------------------------------------------
// step: one Gauss-Newton step of a round, one workgroup
// ---------------------------------------------------------------------------------------------
// log of a rotation M whose angle is below a quarter turn (cos_max > 0): v = (M - M^T)^vee / 2 = sin(theta) axis,
// c = (trace - 1) / 2, theta = atan2(|v|, c), log = (theta / |v|) v with the series 1 + s^2 / 6 + 3 s^4 / 40 below |v| = 1e-4.
__device__ inline void rot_log(const double* M, double* w) {
  const double v0 = 0.5 * (M[7] - M[5]), v1 = 0.5 * (M[2] - M[6]), v2 = 0.5 * (M[3] - M[1]);
  const double c = 0.5 * ((M[0] + M[4] + M[8]) - 1.0);
  const double s2 = __builtin_fma(v0, v0, __builtin_fma(v1, v1, v2 * v2)), s = sqrt(s2);
  const double f = s < 1e-4 ? 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0)) : atan2(s, c) / s;
  w[0] = f * v0; w[1] = f * v1; w[2] = f * v2;
}

// R <- R exp([w]x): exp = I + A [w]x + B [w]x^2, A = sin(t) / t, B = (1 - cos t) / t^2, their series below t = 1e-4.
__device__ inline void rot_apply_exp(double* R, const double* w) {
  const double t2 = __builtin_fma(w[0], w[0], __builtin_fma(w[1], w[1], w[2] * w[2])), t = sqrt(t2);
  const double A = t < 1e-4 ? 1.0 - t2 / 6.0 : sin(t) / t, B = t < 1e-4 ? 0.5 - t2 / 24.0 : (1.0 - cos(t)) / t2;
  double X[9];
  X[0] = 1.0 - B * (w[1] * w[1] + w[2] * w[2]); X[1] = B * (w[0] * w[1]) - A * w[2];       X[2] = B * (w[0] * w[2]) + A * w[1];
  X[3] = B * (w[0] * w[1]) + A * w[2];       X[4] = 1.0 - B * (w[0] * w[0] + w[2] * w[2]); X[5] = B * (w[1] * w[2]) - A * w[0];
  X[6] = B * (w[0] * w[2]) - A * w[1];       X[7] = B * (w[1] * w[2]) + A * w[0];       X[8] = 1.0 - B * (w[0] * w[0] + w[1] * w[1]);
  double out[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * r + c] = __builtin_fma(R[3 * r], X[c], __builtin_fma(R[3 * r + 1], X[3 + c], R[3 * r + 2] * X[6 + c]));
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = out[k];
}

__global__ __launch_bounds__(kRotBlock) void rotavg_step_kernel(RotArgs a) {
  __shared__ double red[kRotBlock / 64];
  __shared__ double total;
  if (a.st[kStStopped] || a.st[kStHyp] < 0) return;
  const int tid = threadIdx.x, V = a.V;
  const size_t n3 = (size_t)3 * V;
  double *vb = a.vec, *vx = a.vec + n3, *vr = a.vec + 2 * n3, *vp = a.vec + 3 * n3, *vq = a.vec + 4 * n3, *vinv = a.vec + 5 * n3;
  // the logs d_e = log(R_j^T Rel_e R_i) of the edges of S (an end of such an edge is connected iff the other is)
  for (int e = tid; e < a.E; e += kRotBlock) {
    double w[3] = {0.0, 0.0, 0.0};
    const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
    if (a.mask[e] && a.conn[i] >= 0) {
      double Ri[9], Rj[9], Rel[9], P[9], M[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) { Ri[k] = a.R_try[(size_t)i * 9 + k]; Rj[k] = a.R_try[(size_t)j * 9 + k]; Rel[k] = a.rel[(size_t)e * 9 + k]; }
      rotation_forward(Rel, Ri, P);
      rotation_backward(Rj, P, M);
      rot_log(M, w);
    }
    a.d[3 * (size_t)e] = w[0]; a.d[3 * (size_t)e + 1] = w[1]; a.d[3 * (size_t)e + 2] = w[2];
  }
  __syncthreads();
  // per view, over its adjacency in adjacency order: the degree in S and b_v = sum (v is j ? d_e : -d_e)
  for (int v = tid; v < V; v += kRotBlock) {
    double b[3] = {0.0, 0.0, 0.0}, inv = 0.0;
    if (a.conn[v] >= 0 && v != a.root) {
      int deg = 0;
      for (int k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
        const int x = a.adj[k], e = x >> 1;
        if (!a.mask[e]) continue;
        ++deg;
        const double sg = (x & 1) ? 1.0 : -1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] += sg * a.d[3 * (size_t)e + c];
      }
      inv = 1.0 / (double)deg;                               // connected through S and not the root: deg >= 1
    }
    vinv[v] = inv;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      vb[3 * (size_t)v + c] = b[c]; vx[3 * (size_t)v + c] = 0.0; vr[3 * (size_t)v + c] = b[c]; vp[3 * (size_t)v + c] = inv * b[c];
    }
  }
  __syncthreads();
  auto dot3 = [&](const double* x, const double* y, int v) {
    return __builtin_fma(x[3 * (size_t)v + 2], y[3 * (size_t)v + 2], __builtin_fma(x[3 * (size_t)v + 1], y[3 * (size_t)v + 1], x[3 * (size_t)v] * y[3 * (size_t)v]));
  };
  const double bb = block_dot<kRotBlock>(V, [&](int v) { return dot3(vb, vb, v); }, red, &total);
  double rz = block_dot<kRotBlock>(V, [&](int v) { return dot3(vr, vp, v); }, red, &total);      // p = z at the start
  bool done = !(bb > 0.0);                                   // nothing to move (or NaN: the round will not stand)
  for (int it = 0; it < a.cg_max && !done; ++it) {
    // q = L p: a held view and the root carry p = 0
    for (int v = tid; v < V; v += kRotBlock) {
      double q[3] = {0.0, 0.0, 0.0};
      if (vinv[v] > 0.0) {
        int deg = 0;
        double nb[3] = {0.0, 0.0, 0.0};
        for (int k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
          const int x = a.adj[k];
          if (!a.mask[x >> 1]) continue;
          ++deg;
          const int o = a.edges[x ^ 1];
#pragma unroll
          for (int c = 0; c < 3; ++c) nb[c] += vp[3 * (size_t)o + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = (double)deg * vp[3 * (size_t)v + c] - nb[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) vq[3 * (size_t)v + c] = q[c];
    }
    __syncthreads();
    const double pq = block_dot<kRotBlock>(V, [&](int v) { return dot3(vp, vq, v); }, red, &total);
    const double alpha = rz / pq;
    for (int v = tid; v < V; v += kRotBlock) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t k = 3 * (size_t)v + c;
        vx[k] = __builtin_fma(alpha, vp[k], vx[k]);
        vr[k] = __builtin_fma(-alpha, vq[k], vr[k]);
      }
    }
    __syncthreads();
    const double rr = block_dot<kRotBlock>(V, [&](int v) { return dot3(vr, vr, v); }, red, &total);
    if (rr <= a.cg_tol2 * bb) { done = true; break; }
    const double rz_new = block_dot<kRotBlock>(V, [&](int v) { return vinv[v] * dot3(vr, vr, v); }, red, &total);
    const double beta = rz_new / rz;
    rz = rz_new;
    for (int v = tid; v < V; v += kRotBlock) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t k = 3 * (size_t)v + c;
        vp[k] = __builtin_fma(beta, vp[k], vinv[v] * vr[k]);
      }
    }
    __syncthreads();
  }
  if (!done && tid == 0) atomicOr(&a.st[kStFlags], SFM_ROTAVG_CG_LIMIT);
  for (int v = tid; v < V; v += kRotBlock) {
    if (!(vinv[v] > 0.0)) continue;
    double R[9];
    const double w[3] = {vx[3 * (size_t)v], vx[3 * (size_t)v + 1], vx[3 * (size_t)v + 2]};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R_try[(size_t)v * 9 + k];
    rot_apply_exp(R, w);
#pragma unroll
    for (int k = 0; k < 9; ++k) a.R_try[(size_t)v * 9 + k] = R[k];
  }
}

// ---------------------------------------------------------------------------------------------
// accept: the round stands iff every moved rotation is finite and the count over all E does not fall
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRotBlock) void rotavg_accept_kernel(RotArgs a) {
  __shared__ int lds_total;
  if (a.st[kStStopped] || a.st[kStHyp] < 0) return;
  const int tid = threadIdx.x;
  int mine = 0, bad = 0;
  for (int e = tid; e < a.E; e += kRotBlock) {
    double Ri[9], Rj[9], Rel[9], lhs;
    const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ri[k] = a.R_try[(size_t)i * 9 + k]; Rj[k] = a.R_try[(size_t)j * 9 + k]; Rel[k] = a.rel[(size_t)e * 9 + k]; }
    const bool in = rotation_edge_inlier(Ri, Rj, Rel, a.thr, &lhs);
    a.mask_try[e] = in ? 1 : 0;
    mine += in;
  }
  for (int v = tid; v < a.V; v += kRotBlock) {
    if (a.conn[v] < 0) continue;
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.R_try[(size_t)v * 9 + k];
    bad |= rot_finite9(R) ? 0 : 1;
  }
  const int count = block_sum_int(mine, &lds_total);
  bad = __syncthreads_or(bad);
  const bool stands = !bad && count >= a.st[kStCount];
  __syncthreads();                                           // every thread has read the standing count
  if (!stands) { if (tid == 0) a.st[kStStopped] = 1; return; }
  for (size_t k = tid; k < (size_t)a.V * 9; k += kRotBlock) a.R_cur[k] = a.R_try[k];
  for (int e = tid; e < a.E; e += kRotBlock) a.mask[e] = a.mask_try[e];
  if (tid == 0) { a.st[kStCount] = count; a.st[kStStood] += 1; }
}

// ---------------------------------------------------------------------------------------------
// judge: the outputs
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRotBlock) void rotavg_judge_kernel(RotArgs a) {
  __shared__ int lds_sums[5];
  const int tid = threadIdx.x;
  const bool model = a.st[kStHyp] >= 0;
  const double nan = __builtin_nan("");
  int n_in = 0, n_out = 0, n_rot = 0, n_unreached = 0, n_held = 0;
  for (int e = tid; e < a.E; e += kRotBlock) {
    double Ri[9], Rj[9], Rel[9], lhs;
    const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ri[k] = a.R_cur[(size_t)i * 9 + k]; Rj[k] = a.R_cur[(size_t)j * 9 + k]; Rel[k] = a.rel[(size_t)e * 9 + k]; }
    const bool both = model && a.reach[i] >= 0 && a.reach[j] >= 0;
    const bool in = rotation_edge_inlier(Ri, Rj, Rel, a.thr, &lhs) && both;
    if (a.edge_inlier) a.edge_inlier[e] = in ? 1 : 0;
    if (a.edge_cos) a.edge_cos[e] = both ? (lhs - 1.0) / 2.0 : nan;
    n_in += in;
    n_out += both && !in;
  }
  for (int v = tid; v < a.V; v += kRotBlock) {
    const bool has = model && a.reach[v] >= 0, held = !(model && a.conn[v] >= 0);
#pragma unroll
    for (int k = 0; k < 9; ++k) a.R_out[(size_t)v * 9 + k] = has ? a.R_cur[(size_t)v * 9 + k] : 0.0;
    if (a.view_status) a.view_status[v] = (a.reach[v] < 0 ? SFM_ROTAVG_UNREACHED : 0) | (held ? SFM_ROTAVG_HELD : 0);
    n_rot += has; n_unreached += a.reach[v] < 0; n_held += held;
  }
  int n[5] = {n_rot, n_unreached, n_held, n_in, n_out};       // the order of the summary
  block_sums(n, lds_sums);
  if (tid != 0) return;
  const int stood = a.st[kStStood];
  const int flags = model ? ((a.iters > 0 && stood == 0 ? SFM_ROTAVG_KEPT_HYPOTHESIS : 0) | a.st[kStFlags]) : SFM_ROTAVG_NO_MODEL;
  if (a.n_inliers) *a.n_inliers = n[3];
  if (a.best_hyp) *a.best_hyp = model ? a.st[kStHyp] : -1;
  if (a.status) *a.status = flags;
  if (a.summary) {
#pragma unroll
    for (int k = 0; k < 5; ++k) a.summary[k] = n[k];
    a.summary[5] = stood;
  }
}

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static long long g_rot_work_cap = kRotWorkCap;

// Hypotheses per batch: as many as keep [batch][V][9] doubles within the cap, at least one.
static void rot_plan(int V, int H, int* batch, int* n_batches) {
  const long long per = (long long)V * 9 * (long long)sizeof(double);
  long long b = g_rot_work_cap / per;
  b = b < 1 ? 1 : (b > H ? H : b);
  *batch = (int)b;
  *n_batches = (int)((H + b - 1) / b);
}

static int rot_check(const char* who, int V, long long E, const int* edges, const double* rel, int root, double cos_max,
                     int max_hyp, int iters, int steps, double cg_tol, int cg_max, const void* R_out) {
  if (V < 2 || E < 1 || E >= (1LL << 31)) { set_error("%s: bad sizes V=%d E=%lld (V >= 2, 1 <= E < 2^31)", who, V, E); return SFM_E_SHAPE; }
  if (E > INT_MAX / 2) { set_error("%s: E=%lld edges are beyond the workspace", who, E); return SFM_E_SHAPE; }
  if (edges == nullptr || rel == nullptr || R_out == nullptr) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  if (root < 0 || root >= V) { set_error("%s: root = %d must be in 0 .. %d", who, root, V - 1); return SFM_E_SHAPE; }
  if (!(cos_max > 0.0 && cos_max <= 1.0)) { set_error("%s: cos_max = %g must be in (0, 1]", who, cos_max); return SFM_E_SHAPE; }
  if (max_hyp < 0 || max_hyp > kHypMax) { set_error("%s: max_hyp = %d must be in 1 .. %d (0 = %d)", who, max_hyp, kHypMax, kHypDefault); return SFM_E_SHAPE; }
  if (iters < 0) { set_error("%s: iters = %d must be >= 0", who, iters); return SFM_E_SHAPE; }
  if (steps < 1) { set_error("%s: steps = %d must be >= 1", who, steps); return SFM_E_SHAPE; }
  if (!(cg_tol > 0.0 && cg_tol < 1.0)) { set_error("%s: cg_tol = %g must be in (0, 1)", who, cg_tol); return SFM_E_SHAPE; }
  if (cg_max < 1) { set_error("%s: cg_max = %d must be >= 1", who, cg_max); return SFM_E_SHAPE; }
  return view_graph_check_edges(who, V, E, edges);
}

// The breadth-first tree of hypothesis h on the host (the rule's step 2, without rotations).
static void rot_tree_host(int V, long long E, const int* edges, int h, int root, int* parent, int* depth) {
  std::vector<int> ptr((size_t)V + 1, 0), adj((size_t)2 * E), fill;
  for (long long x = 0; x < 2 * E; ++x) ++ptr[(size_t)edges[x] + 1];
  for (int v = 0; v < V; ++v) ptr[v + 1] += ptr[v];
  fill.assign(ptr.begin(), ptr.end() - 1);
  for (long long x = 0; x < 2 * E; ++x) adj[(size_t)fill[edges[x]]++] = (int)x;
  for (int v = 0; v < V; ++v) { parent[v] = -1; depth[v] = -1; }
  depth[rot_tree_root(h, V, root)] = 0;
  for (int d = 1; d < V; ++d) {
    std::vector<int> took;
    for (int v = 0; v < V; ++v) {
      if (depth[v] != -1) continue;
      unsigned long long best_key = 0;
      int best_e = -1;
      for (int k = ptr[v]; k < ptr[v + 1]; ++k) {
        const int x = adj[(size_t)k], e = x >> 1;
        if (depth[edges[x ^ 1]] != d - 1) continue;
        const unsigned long long key = h == 0 ? (unsigned long long)e : rot_key(h, (unsigned)e);
        if (best_e < 0 || key < best_key) { best_key = key; best_e = e; }
      }
      if (best_e >= 0) { parent[v] = best_e; took.push_back(v); }
    }
    if (took.empty()) break;
    for (int v : took) depth[v] = d;
  }
}

struct RotWork {
  DevBuf<int> adj_ptr, adj, st, reach, conn, counts, depth_glob;
  DevBuf<double> rot, R_cur, R_try, d, vec;
  DevBuf<unsigned char> ok, mask, mask_try;
};

// The arguments of the kernels, but for the work buffers: the inputs and outputs of either form, on the device.
static RotArgs rot_args(int V, long long E, const int* d_edges, const double* d_rel, int root, double cos_max, int iters, int steps,
                        double cg_tol, int cg_max, double* R_out, unsigned char* edge_inlier, double* edge_cos, int* view_status,
                        int* n_inliers, int* best_hyp, int* status, int64_t* summary) {
  RotArgs a = {};
  a.V = V; a.E = (int)E; a.root = root; a.edges = d_edges; a.rel = d_rel; a.thr = __builtin_fma(2.0, cos_max, 1.0);
  a.iters = iters; a.steps = steps; a.cg_max = cg_max; a.cg_tol2 = cg_tol * cg_tol;
  a.R_out = R_out; a.edge_inlier = edge_inlier; a.edge_cos = edge_cos; a.view_status = view_status;
  a.n_inliers = n_inliers; a.best_hyp = best_hyp; a.status = status; a.summary = reinterpret_cast<unsigned long long*>(summary);
  return a;
}

// The one body of both forms: checked arguments and device pointers in, everything enqueued on s.
static int rot_run(RotArgs a, int max_hyp, RotWork& w, hipStream_t s) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  const int V = a.V, E = a.E;
  int batch, n_batches;
  rot_plan(V, max_hyp, &batch, &n_batches);
  SFM_TRY(w.st.alloc(kStWords, s));
  const int st0[kStWords] = {-1, -1, 0, 0, 0};
  SFM_HIP(hipMemcpyAsync(w.st.p, st0, sizeof(st0), hipMemcpyHostToDevice, s));
  a.st = w.st.p;
  SFM_TRY(view_adjacency(V, E, a.edges, w.adj_ptr, w.adj, s));
  a.adj_ptr = w.adj_ptr.p; a.adj = w.adj.p;
  SFM_TRY(w.reach.alloc(V, s)); SFM_TRY(w.conn.alloc(V, s)); SFM_TRY(w.counts.alloc(batch, s)); SFM_TRY(w.ok.alloc(batch, s));
  SFM_TRY(w.rot.alloc((size_t)batch * V * 9, s)); SFM_TRY(w.R_cur.alloc((size_t)V * 9, s)); SFM_TRY(w.R_try.alloc((size_t)V * 9, s));
  SFM_TRY(w.mask.alloc(E, s)); SFM_TRY(w.mask_try.alloc(E, s)); SFM_TRY(w.d.alloc((size_t)3 * E, s)); SFM_TRY(w.vec.alloc((size_t)18 * V, s));
  if (V > kRotLdsViews) SFM_TRY(w.depth_glob.alloc((size_t)batch * V, s));
  a.R_cur = w.R_cur.p; a.R_try = w.R_try.p; a.mask = w.mask.p; a.mask_try = w.mask_try.p; a.reach = w.reach.p; a.conn = w.conn.p;
  a.d = w.d.p; a.vec = w.vec.p;
  SFM_HIP(hipMemsetAsync(a.R_cur, 0, sizeof(double) * 9 * (size_t)V, s));
  // what the input graph reaches from root
  rotavg_tree_kernel<<<1, kRotTreeThreads, 0, s>>>(a, 0, nullptr, nullptr, w.depth_glob.p, nullptr, nullptr, a.reach);
  const unsigned edge_blocks = (unsigned)((E + kRotScoreEdges - 1) / kRotScoreEdges);
  for (int k = 0; k < n_batches; ++k) {
    const int h0 = k * batch, nb = std::min(batch, max_hyp - h0);
    SFM_HIP(hipMemsetAsync(w.counts.p, 0, sizeof(int) * (size_t)nb, s));
    rotavg_tree_kernel<<<nb, kRotTreeThreads, 0, s>>>(a, h0, nullptr, nullptr, w.depth_glob.p, w.rot.p, w.ok.p, nullptr);
    rotavg_score_kernel<<<dim3(edge_blocks, (unsigned)std::min(nb, kRotScoreSlices)), kRotScoreThreads, 0, s>>>(a, nb, w.rot.p, w.ok.p, w.counts.p);
    rotavg_adopt_kernel<<<1, kRotTreeThreads, 0, s>>>(a, h0, nb, w.rot.p, w.ok.p, w.counts.p);
  }
  rotavg_mask_kernel<<<(unsigned)((E + 255) / 256), 256, 0, s>>>(a);
  // the gate of this first connectivity is open even without a model: conn then holds the root alone (no edge is in the mask)
  rotavg_tree_kernel<<<1, kRotTreeThreads, 0, s>>>(a, 0, a.mask, nullptr, w.depth_glob.p, nullptr, nullptr, a.conn);
  for (int it = 0; it < a.iters; ++it) {
    rotavg_copy_kernel<<<(unsigned)((9 * (size_t)V + 255) / 256), 256, 0, s>>>(a);
    for (int k = 0; k < a.steps; ++k) rotavg_step_kernel<<<1, kRotBlock, 0, s>>>(a);
    rotavg_accept_kernel<<<1, kRotBlock, 0, s>>>(a);
    rotavg_tree_kernel<<<1, kRotTreeThreads, 0, s>>>(a, 0, a.mask, a.st, w.depth_glob.p, nullptr, nullptr, a.conn);
  }
  rotavg_judge_kernel<<<1, kRotBlock, 0, s>>>(a);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_rotation_edge_test(const double* Ri, const double* Rj, const double* Rel, double cos_max, double* lhs_out) {
  if (Ri == nullptr || Rj == nullptr || Rel == nullptr) return 0;
  double lhs;
  const bool in = rotation_edge_inlier(Ri, Rj, Rel, __builtin_fma(2.0, cos_max, 1.0), &lhs);
  if (lhs_out) *lhs_out = lhs;
  return in ? 1 : 0;
}

int sfm_rotation_tree(int V, int64_t E, const int* edges, int root, int max_hyp, int h, int* parent_edge_out, int* depth_out) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (V < 2 || E < 1 || E > INT_MAX / 2 || edges == nullptr || root < 0 || root >= V || max_hyp < 1 || max_hyp > kHypMax) return 0;
  for (int64_t e = 0; e < E; ++e)
    if (!view_graph_edge_ok(V, edges[2 * e], edges[2 * e + 1])) return 0;
  if (h >= 0 && h < max_hyp && parent_edge_out != nullptr && depth_out != nullptr) rot_tree_host(V, E, edges, h, root, parent_edge_out, depth_out);
  return max_hyp;
}

int sfm_rotation_plan(int V, int max_hyp, int64_t cap_bytes, int* batch, int* n_batches) {
  if (max_hyp == 0) max_hyp = kHypDefault;
  if (V < 2 || max_hyp < 1 || max_hyp > kHypMax || cap_bytes < 0 || batch == nullptr || n_batches == nullptr) return SFM_E_SHAPE;
  g_rot_work_cap = cap_bytes ? cap_bytes : kRotWorkCap;
  rot_plan(V, max_hyp, batch, n_batches);
  return SFM_OK;
}

int sfm_rotation_average_dev(int V, int64_t E, const int* edges, const double* d_rel, int root, double cos_max,
                             int max_hyp, int iters, int steps, double cg_tol, int cg_max, double* d_R_out,
                             unsigned char* d_edge_inlier, double* d_edge_cos, int* d_view_status, int* d_n_inliers, int* d_best_hyp,
                             int* d_status, int64_t* d_summary, void* hip_stream) {
  const char* who = "sfm_rotation_average_dev";
  SFM_TRY(rot_check(who, V, E, edges, d_rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max, d_R_out));
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  SFM_TRY(check_rotations_dev(who, "Rel of edge %lld", E, d_rel, false, s));
  DevBuf<int> dE;                       // the checked host copy: no kernel indexes with a value that was not looked at
  SFM_TRY(dE.upload(edges, 2 * (size_t)E, s));
  const RotArgs a = rot_args(V, E, dE.p, d_rel, root, cos_max, iters, steps, cg_tol, cg_max, d_R_out, d_edge_inlier, d_edge_cos,
                             d_view_status, d_n_inliers, d_best_hyp, d_status, d_summary);
  RotWork w;
  SFM_TRY(rot_run(a, max_hyp, w, s));
  return stream_sync(s);
}

int sfm_rotation_average(int V, int64_t E, const int* edges, const double* rel, int root, double cos_max, int max_hyp, int iters,
                         int steps, double cg_tol, int cg_max, double* R_out, unsigned char* edge_inlier, double* edge_cos,
                         int* view_status, int* n_inliers, int* best_hyp, int* status, int64_t* summary) {
  const char* who = "sfm_rotation_average";
  SFM_TRY(rot_check(who, V, E, edges, rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max, R_out));
  SFM_TRY(check_rotations_host(who, "Rel of edge %lld", E, rel, false));
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t v = (size_t)V, m = (size_t)E;
  DevBuf<int> dE;
  DevBuf<double> dRel;
  HostOut<double> oR, oCos;
  HostOut<unsigned char> oIn;
  HostOut<int> oView, oN, oBest, oStatus;
  HostOut<int64_t> oSum;
  RotWork w;
  SFM_TRY(dE.upload(edges, 2 * m, s));
  SFM_TRY(dRel.upload(rel, 9 * m, s));
  SFM_TRY(oR.want(R_out, 9 * v, s)); SFM_TRY(oCos.want(edge_cos, m, s)); SFM_TRY(oIn.want(edge_inlier, m, s));
  SFM_TRY(oView.want(view_status, v, s)); SFM_TRY(oN.want(n_inliers, 1, s)); SFM_TRY(oBest.want(best_hyp, 1, s));
  SFM_TRY(oStatus.want(status, 1, s)); SFM_TRY(oSum.want(summary, 6, s));
  const RotArgs a = rot_args(V, E, dE.p, dRel.p, root, cos_max, iters, steps, cg_tol, cg_max, oR.dev(), oIn.dev(), oCos.dev(), oView.dev(),
                             oN.dev(), oBest.dev(), oStatus.dev(), oSum.dev());
  SFM_TRY(rot_run(a, max_hyp, w, s));
  SFM_TRY(oR.fetch(s)); SFM_TRY(oCos.fetch(s)); SFM_TRY(oIn.fetch(s)); SFM_TRY(oView.fetch(s)); SFM_TRY(oN.fetch(s));
  SFM_TRY(oBest.fetch(s)); SFM_TRY(oStatus.fetch(s)); SFM_TRY(oSum.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
