// sfm_view_graph.h -- what the operations on a view graph share (sfm_rotavg.hip, sfm_translation.hip, sfm_triplets.hip):
// the check of the edge list, the check that matrices are rotations (host and device), the view-major adjacency, the
// slice-ordered sum of the two conjugate-gradient solvers, and the breadth-first levels from a root.  DESIGN.md, "Shared
// primitives", states what each piece guarantees.
//
// Include it after sfm_obs_test.h, where contraction is off.  Nothing here multiplies and then adds: the only floating-point
// operation is the addition of block_dot, so no bit of it would change under another contraction mode, and nothing may be
// added here whose bits would.
#pragma once

#include <climits>
#include <cstdio>

#include "sfm_robust.h"

namespace sfm {

// ---- the edge list: E pairs (i, j) on the host ----
inline bool view_graph_edge_ok(int V, int i, int j) { return i >= 0 && i < V && j >= 0 && j < V && i != j; }

inline int view_graph_check_edges(const char* who, int V, long long E, const int* edges) {
  if (edges == nullptr) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  for (long long e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (!view_graph_edge_ok(V, i, j)) { set_error("%s: edge %lld = (%d, %d) must join two different views in 0 .. %d", who, e, i, j, V - 1); return SFM_E_SHAPE; }
  }
  return SFM_OK;
}

// ---- n matrices of nine doubles that must pass verify_rotation; with skip_zero nine zeros stand for "no rotation" ----
SFM_HD bool has_rotation(const double* R) {
  bool any = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) any |= R[k] != 0.0;
  return any;
}

// `what` names the item, a format for its index: "Rel of edge %lld", "R of view %lld"
inline int rotation_refused(const char* who, const char* what, long long k) {
  char item[64];
  std::snprintf(item, sizeof(item), what, k);
  set_error("%s: %s is not a rotation", who, item);
  return SFM_E_BAD_ROTATION;
}

inline int check_rotations_host(const char* who, const char* what, long long n, const double* R, bool skip_zero) {
  for (long long k = 0; k < n; ++k)
    if ((!skip_zero || has_rotation(R + 9 * k)) && !verify_rotation(R + 9 * k)) return rotation_refused(who, what, k);
  return SFM_OK;
}

static __global__ __launch_bounds__(256) void view_graph_verify_kernel(int n, const double* R, int skip_zero, int* lowest) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double M[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) M[q] = R[(size_t)k * 9 + q];
  if ((!skip_zero || has_rotation(M)) && !verify_rotation(M)) atomicMin(lowest, (int)k);
}

// The same on the device (n < 2^31): the lowest failing index through one word of the pool.  Waits for s.
inline int check_rotations_dev(const char* who, const char* what, long long n, const double* d_R, bool skip_zero, hipStream_t s) {
  DevBuf<int> lowest;
  int k = INT_MAX;
  SFM_TRY(lowest.upload(&k, 1, s));
  view_graph_verify_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((int)n, d_R, skip_zero ? 1 : 0, lowest.p);
  SFM_TRY(lowest.download(&k, 1, s));
  SFM_HIP(hipStreamSynchronize(s));
  return k == INT_MAX ? SFM_OK : rotation_refused(who, what, k);
}

// ---- the view-major adjacency: entry x = 2 e + dir (dir = 1 where the view is the edge's j) of every view, ascending ----
// The key-major list of sfm_common.h over the 2 E index pairs as they lie in memory, stable in edge order.
inline int view_adjacency(int V, int E, const int* d_edges, DevBuf<int>& adj_ptr, DevBuf<int>& adj, hipStream_t s) {
  SFM_TRY(adj_ptr.alloc((size_t)V + 1, s));
  SFM_TRY(adj.alloc((size_t)2 * E, s));
  return key_major_list(2LL * E, V, d_edges, adj_ptr.p, adj.p, s);
}

// ---- the workgroup's sum of one value per item, in an order that depends on n alone ----
// Chunks of BLOCK items in ascending order; inside a chunk a wave's 64 items are summed in the wave (group_sum<64>'s fixed
// order) and the slices are then added in slice order by thread 0.  val(k) is called once for every k < n.  Every thread
// returns the total.  red holds BLOCK / 64 doubles.  The barriers also order the caller's global-memory vectors between
// the phases of a CG: what was stored before the call is visible to every thread after it.
template <int BLOCK, class Val>
__device__ __forceinline__ double block_dot(int n, Val val, double* red, double* total) {
  const int tid = threadIdx.x;
  double run = 0.0;
  for (int base = 0; base < n; base += BLOCK) {
    const int k = base + tid;
    const double s = group_sum<64>(k < n ? val(k) : 0.0);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      const int slices = (min(n - base, BLOCK) + 63) / 64;
      for (int q = 0; q < slices; ++q) run += red[q];
    }
    __syncthreads();                                           // red is free for the next chunk
  }
  if (tid == 0) *total = run;
  __syncthreads();
  const double t = *total;
  __syncthreads();                                             // total is free for the next call
  return t;
}

// ---- breadth-first levels from root, one workgroup of THREADS ----
// depth[v] becomes the level of v (0: root, -1: not joined).  visit(v, lev) is called for every view without a depth and
// scans its adjacency for a neighbour o with depth[o] == lev - 1; it returns true when v joins level lev.  A view that takes
// its depth in this very level holds -1 or lev while others look at it, never lev - 1: visit may read depth[] without a
// barrier inside a level.  Returns whether any level was added: false means that root has no live edge.
template <int THREADS, class Visit>
__device__ __forceinline__ bool graph_levels(int V, int root, int* depth, Visit visit) {
  const int tid = threadIdx.x;
  for (int v = tid; v < V; v += THREADS) depth[v] = v == root ? 0 : -1;
  __syncthreads();
  bool any = false;
  for (int lev = 1; lev < V; ++lev) {              // a level adds at least one view, so V - 1 levels at the most
    int added = 0;
    for (int v = tid; v < V; v += THREADS) {
      if (depth[v] != -1 || !visit(v, lev)) continue;
      depth[v] = lev;
      added = 1;
    }
    if (!__syncthreads_or(added)) break;
    any = true;
  }
  return any;
}

}  // namespace sfm
