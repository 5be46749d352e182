// sfm_triplets.hip — view triplets: the cycle-consistency filter of a view graph (gfx950).
//
// Around every triangle of the view graph the three relative rotations must compose to the identity; an edge that lies in
// no consistent triangle is dropped before the rotation averaging sees it.  The rule is stated in sfm_hip.h, block "view
// triplets".  One graph per call; the stages:
//   adjacency  the view-major list of the 2 E edge ends ordered by (view, neighbour, edge): two passes of the key-major
//              list of sfm_common.h (a stable counting sort), least-significant key first -- keys = the other end, then
//              keys = the own end gathered through the first pass's list -- and a gather of (neighbour, entry) per slot
//   enumerate  the hot path: a group of G lanes per edge.  The lanes stride over the SHORTER adjacency of the edge's two
//              ends; a lane looks its neighbour up in the longer one by binary search and walks the run of parallel
//              edges there.  Every edge enumerates ALL its triplets (three times the tests, no atomic at all): the two
//              counts live in registers and are folded over the group; lane 0 stores them and the verdict
//   summary    integer sums over the edges (64-bit integer atomics: order-independent)
//   scan       the exclusive prefix sum of the verdicts (sfm_scan.h: one workgroup, or device-wide from 2^14 edges on)
//              scatters the kept edge numbers and writes the summary
// No floating-point value is accumulated at all; a triplet is always tested in its canonical a < b < c order, so its bits
// do not depend on the edge, lane or group width that finds it.
#include <climits>
#include <cmath>

#include "sfm_obs_test.h"      // contraction is off from here on
#include "sfm_view_graph.h"
#include "sfm_scan.h"

namespace sfm {

constexpr int kTriThreads = 256;
constexpr int kTriScanCrossover = 1 << 14;      // the device-wide scan from this many edges on

typedef unsigned long long u64;

// state words of a call on the device (64-bit counters)
enum { kTsTri = 0, kTsOk, kTsTested, kTsKept, kTsDropped, kTsUntested, kTsMasked, kTsLargest, kTsNKept, kTsWords };

struct TriArgs {
  int V, E;
  const int* edges;             // [E][2] = (i, j); read as the 2 E keys of the adjacency
  const double* rel;            // [E][9]
  const unsigned char* mask;    // [E] or null
  const int* adj_ptr;           // [V + 1]
  const int* adj_nb;            // [2 E] the neighbour of every slot, ascending inside a view
  const int* adj_x;             // [2 E] the entry x = 2 e + dir of every slot, ascending inside a neighbour
  double thr;                   // fma(2, cos_loop, 1)
  long long min_ok, min_pct;
  int keep_untested;
  u64* st;                      // [kTsWords]
  unsigned char* keep;          // [E] (the caller's edge_keep or a work buffer)
  long long* n_tri;             // [E] (likewise)
  long long* n_ok;              // [E] (likewise)
  int* kept_idx;                // [E] or null
  long long* summary;           // [8] or null
};

// M_e, frame lo -> frame hi: Rel_e as it is where i_e < j_e, its transpose (a copy of entries) otherwise
__device__ __forceinline__ void tri_oriented(const TriArgs& a, int e, double* M) {
  const bool tr = a.edges[2 * (size_t)e] > a.edges[2 * (size_t)e + 1];
  double R[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = a.rel[9 * (size_t)e + k];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[3 * r + c] = tr ? R[3 * c + r] : R[3 * r + c];
}

// ---------------------------------------------------------------------------------------------
// adjacency: the keys of the two passes and the gather
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void triplets_other_end_kernel(TriArgs a, int* key) {
  const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
  if (x < 2LL * a.E) key[x] = a.edges[x ^ 1];
}

__global__ __launch_bounds__(256) void triplets_own_end_kernel(TriArgs a, const int* by_nb, int* key) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < 2LL * a.E) key[k] = a.edges[by_nb[k]];
}

__global__ __launch_bounds__(256) void triplets_adjacency_kernel(TriArgs a, const int* by_nb, const int* by_view, int* adj_nb, int* adj_x) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= 2LL * a.E) return;
  const int x = by_nb[by_view[m]];
  adj_x[m] = x;
  adj_nb[m] = a.edges[x ^ 1];
}

// ---------------------------------------------------------------------------------------------
// enumerate: the hot path
// ---------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kTriThreads) void triplets_enumerate_kernel(TriArgs a) {
  constexpr int kPer = kTriThreads / G;                       // edges of a workgroup per turn
  const int lane = threadIdx.x & (G - 1);
  const long long step = (long long)gridDim.x * kPer;
  // the turns are the same for every lane of a wave: the fold below needs them all
  for (long long base = (long long)blockIdx.x * kPer; base < a.E; base += step) {
    const long long el = base + threadIdx.x / G;
    const bool live = el < a.E;
    const int e = live ? (int)el : 0;
    const bool masked = a.mask != nullptr && a.mask[e] == 0;
    long long nt = 0, nk = 0;
    if (live && !masked) {
      const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      double Me[9];
      tri_oriented(a, e, Me);
      const int l0 = a.adj_ptr[lo], l1 = a.adj_ptr[lo + 1], h0 = a.adj_ptr[hi], h1 = a.adj_ptr[hi + 1];
      const bool lo_short = l1 - l0 <= h1 - h0;
      const int s0 = lo_short ? l0 : h0, s1 = lo_short ? l1 : h1, t0 = lo_short ? h0 : l0, t1 = lo_short ? h1 : l1;
      for (int k = s0 + lane; k < s1; k += G) {              // a hub's adjacency is strided
        const int w = a.adj_nb[k];
        if (w == lo || w == hi) continue;
        const int es = a.adj_x[k] >> 1;
        if (a.mask != nullptr && a.mask[es] == 0) continue;
        int L = t0, R = t1;                                   // the first slot of the longer adjacency with neighbour >= w
        while (L < R) {
          const int mid = L + ((R - L) >> 1);
          if (a.adj_nb[mid] < w) L = mid + 1; else R = mid;
        }
        if (L >= t1 || a.adj_nb[L] != w) continue;
        double Ms[9];
        tri_oriented(a, es, Ms);
        const bool c0 = w < lo, c2 = w > hi;                  // (a, b, c) = (w, lo, hi) | (lo, w, hi) | (lo, hi, w)
        for (int q = L; q < t1 && a.adj_nb[q] == w; ++q) {    // every parallel edge is a triplet of its own
          const int et = a.adj_x[q] >> 1;
          if (a.mask != nullptr && a.mask[et] == 0) continue;
          double Mt[9], Mab[9], Mbc[9], Mac[9], lhs;
          tri_oriented(a, et, Mt);
#pragma unroll
          for (int n = 0; n < 9; ++n) {
            const double F = lo_short ? Ms[n] : Mt[n];        // the edge between lo and w
            const double H = lo_short ? Mt[n] : Ms[n];        // the edge between hi and w
            Mab[n] = c2 ? Me[n] : F;
            Mbc[n] = c0 ? Me[n] : H;
            Mac[n] = c0 ? H : (c2 ? F : Me[n]);
          }
          nk += rotation_edge_inlier(Mab, Mac, Mbc, a.thr, &lhs) ? 1 : 0;
          nt += 1;
        }
      }
    }
    nt = group_sum<G>(nt);
    nk = group_sum<G>(nk);
    if (live && lane == 0) {
      a.n_tri[e] = nt;
      a.n_ok[e] = nk;
      const bool keep = masked ? false : (nt == 0 ? a.keep_untested != 0 : (nk >= a.min_ok && 100 * nk >= a.min_pct * nt));
      a.keep[e] = keep ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// summary: integer sums over the edges
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void triplets_summary_kernel(TriArgs a) {
  long long v[7] = {0, 0, 0, 0, 0, 0, 0}, largest = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < a.E; e += (long long)gridDim.x * 256) {
    const bool masked = a.mask != nullptr && a.mask[e] == 0;
    const long long nt = a.n_tri[e];
    const bool keep = a.keep[e] != 0, tested = !masked && nt > 0;
    v[0] += nt; v[1] += a.n_ok[e]; v[2] += tested; v[3] += keep; v[4] += tested && !keep; v[5] += !masked && nt == 0; v[6] += masked;
    largest = nt > largest ? nt : largest;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = group_sum<64>(v[k]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const long long o = __shfl_xor(largest, off, 64); largest = o > largest ? o : largest; }
  if ((threadIdx.x & 63) != 0) return;
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (v[k]) atomicAdd(&a.st[kTsTri + k], (u64)v[k]);
  if (largest) atomicMax(&a.st[kTsLargest], (u64)largest);
}

// the prefix sum over the verdicts: kept_idx, the count the host reads, and the summary
struct TriScanKept {
  TriArgs a;
  __device__ int n() const { return a.E; }
  __device__ void load(int e, int (&v)[1]) const { v[0] = a.keep[e] ? 1 : 0; }
  __device__ void store(int e, const int (&p)[1]) const {
    if (a.kept_idx != nullptr && a.keep[e]) a.kept_idx[p[0]] = e;
  }
  __device__ void total(const int (&t)[1]) const {
    a.st[kTsNKept] = (u64)t[0];
    if (a.summary == nullptr) return;
    // every triplet was counted once by each of its three edges
    a.summary[0] = (long long)(a.st[kTsTri] / 3); a.summary[1] = (long long)(a.st[kTsOk] / 3);
#pragma unroll
    for (int k = 2; k < 8; ++k) a.summary[k] = (long long)a.st[kTsTri + k];
  }
};

#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int tri_check(const char* who, int V, long long E, const int* edges, const double* rel, double cos_loop, int min_ok, int min_pct,
                     int keep_untested, int group) {
  if (V < 3 || E < 1 || E >= (1LL << 30)) { set_error("%s: bad sizes V=%d E=%lld (V >= 3, 1 <= E < 2^30)", who, V, E); return SFM_E_SHAPE; }
  if (edges == nullptr || rel == nullptr) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  if (!(cos_loop > 0.0 && cos_loop <= 1.0)) { set_error("%s: cos_loop = %g must be in (0, 1]", who, cos_loop); return SFM_E_SHAPE; }
  if (min_ok < 0) { set_error("%s: min_ok = %d must be >= 1 (0 = 1)", who, min_ok); return SFM_E_SHAPE; }
  if (min_pct < 0 || min_pct > 100) { set_error("%s: min_pct = %d must be in 0 .. 100", who, min_pct); return SFM_E_SHAPE; }
  if (keep_untested != 0 && keep_untested != 1) { set_error("%s: keep_untested = %d must be 0 or 1", who, keep_untested); return SFM_E_SHAPE; }
  SFM_TRY(group_width_check(who, group));
  return view_graph_check_edges(who, V, E, edges);
}

// `group` = 0: the narrowest width that covers the mean adjacency, wider while the device would be short of waves
static int tri_auto_group(int V, long long E) {
  const long long mean = (2 * E + V - 1) / V;
  const int i = narrowest_group([&](int g) { return g >= mean; });
  return kGroupWidths[widen_for_waves(i, (int)E, 64)];
}

// The arguments of the kernels, but for the work buffers: the inputs and outputs of either form, on the device.
static TriArgs tri_args(int V, long long E, const int* d_edges, const double* d_rel, const unsigned char* d_edge_mask, double cos_loop,
                        int min_ok, int min_pct, int keep_untested, unsigned char* edge_keep, int64_t* n_tri, int64_t* n_ok, int* kept_idx,
                        int64_t* summary) {
  TriArgs a = {};
  a.V = V; a.E = (int)E; a.edges = d_edges; a.rel = d_rel; a.mask = d_edge_mask; a.thr = __builtin_fma(2.0, cos_loop, 1.0);
  a.min_ok = min_ok == 0 ? 1 : min_ok; a.min_pct = min_pct; a.keep_untested = keep_untested;
  a.keep = edge_keep; a.n_tri = reinterpret_cast<long long*>(n_tri); a.n_ok = reinterpret_cast<long long*>(n_ok);
  a.kept_idx = kept_idx; a.summary = reinterpret_cast<long long*>(summary);
  return a;
}

// The one body of both forms: checked arguments and device pointers in, everything enqueued on s; *n_kept is read at the end.
static int tri_run(TriArgs a, int group, int* n_kept, hipStream_t s) {
  const int V = a.V, E = a.E;
  const size_t ends = 2 * (size_t)E;
  DevBuf<u64> st;
  DevBuf<int> adj_ptr, adj_nb, adj_x, key, by_nb, nb_ptr, by_view, tiles;
  DevBuf<unsigned char> keep;
  DevBuf<long long> n_tri, n_ok;
  SFM_TRY(st.alloc(kTsWords, s));
  const u64 st0[kTsWords] = {};
  SFM_HIP(hipMemcpyAsync(st.p, st0, sizeof(st0), hipMemcpyHostToDevice, s));
  a.st = st.p;
  const unsigned edge_blocks = (unsigned)((E + 255) / 256), end_blocks = (unsigned)((ends + 255) / 256);
  if (a.keep == nullptr) { SFM_TRY(keep.alloc(E, s)); a.keep = keep.p; }
  if (a.n_tri == nullptr) { SFM_TRY(n_tri.alloc(E, s)); a.n_tri = n_tri.p; }
  if (a.n_ok == nullptr) { SFM_TRY(n_ok.alloc(E, s)); a.n_ok = n_ok.p; }
  SFM_TRY(adj_ptr.alloc((size_t)V + 1, s)); SFM_TRY(nb_ptr.alloc((size_t)V + 1, s));
  SFM_TRY(adj_nb.alloc(ends, s)); SFM_TRY(adj_x.alloc(ends, s)); SFM_TRY(key.alloc(ends, s));
  SFM_TRY(by_nb.alloc(ends, s)); SFM_TRY(by_view.alloc(ends, s));
  // sorted adjacency: by neighbour first, then (stable) by view
  triplets_other_end_kernel<<<end_blocks, 256, 0, s>>>(a, key.p);
  SFM_TRY(key_major_list(2LL * E, V, key.p, nb_ptr.p, by_nb.p, s));
  triplets_own_end_kernel<<<end_blocks, 256, 0, s>>>(a, by_nb.p, key.p);
  SFM_TRY(key_major_list(2LL * E, V, key.p, adj_ptr.p, by_view.p, s));
  triplets_adjacency_kernel<<<end_blocks, 256, 0, s>>>(a, by_nb.p, by_view.p, adj_nb.p, adj_x.p);
  a.adj_ptr = adj_ptr.p; a.adj_nb = adj_nb.p; a.adj_x = adj_x.p;
  if (group == 0) group = tri_auto_group(V, E);
  const long long want = ((long long)E * group + kTriThreads - 1) / kTriThreads, cap = 64LL * plan_cus();
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  dispatch_group<1>(group, [&](auto g) { triplets_enumerate_kernel<decltype(g)::value><<<grid, kTriThreads, 0, s>>>(a); });
  const long long sum_cap = 4LL * plan_cus();
  triplets_summary_kernel<<<(unsigned)(edge_blocks < sum_cap ? edge_blocks : sum_cap), 256, 0, s>>>(a);
  const int n_tiles = (E + kScanBlock - 1) / kScanBlock;
  SFM_TRY(tiles.alloc(2 * (size_t)n_tiles + 2, s));
  exclusive_scan_launch<1>(TriScanKept{a}, E < kTriScanCrossover, tiles.p, n_tiles, s);
  SFM_HIP(hipGetLastError());
  if (n_kept != nullptr) {
    u64 count = 0;
    SFM_HIP(hipMemcpyAsync(&count, st.p + kTsNKept, sizeof(count), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    *n_kept = (int)count;
  }
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_view_triplet_test(const double* Mab, const double* Mbc, const double* Mac, double cos_loop, double* lhs_out) {
  if (Mab == nullptr || Mbc == nullptr || Mac == nullptr) return 0;
  double lhs;
  const bool ok = rotation_edge_inlier(Mab, Mac, Mbc, __builtin_fma(2.0, cos_loop, 1.0), &lhs);
  if (lhs_out) *lhs_out = lhs;
  return ok ? 1 : 0;
}

int sfm_view_triplets_dev(int V, int64_t E, const int* edges, const double* d_rel, const unsigned char* d_edge_mask, double cos_loop,
                          int min_ok, int min_pct, int keep_untested, int group, unsigned char* d_edge_keep, int64_t* d_n_tri,
                          int64_t* d_n_ok, int* d_kept_idx, int64_t* d_summary, int* n_kept, void* hip_stream) {
  const char* who = "sfm_view_triplets_dev";
  SFM_TRY(tri_check(who, V, E, edges, d_rel, cos_loop, min_ok, min_pct, keep_untested, group));
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  SFM_TRY(check_rotations_dev(who, "Rel of edge %lld", E, d_rel, false, s));
  DevBuf<int> dE;                       // the checked host copy: no kernel indexes with a value that was not looked at
  SFM_TRY(dE.upload(edges, 2 * (size_t)E, s));
  const TriArgs a = tri_args(V, E, dE.p, d_rel, d_edge_mask, cos_loop, min_ok, min_pct, keep_untested, d_edge_keep, d_n_tri, d_n_ok,
                             d_kept_idx, d_summary);
  SFM_TRY(tri_run(a, group, n_kept, s));
  return stream_sync(s);
}

int sfm_view_triplets(int V, int64_t E, const int* edges, const double* rel, const unsigned char* edge_mask, double cos_loop, int min_ok,
                      int min_pct, int keep_untested, int group, unsigned char* edge_keep, int64_t* n_tri, int64_t* n_ok, int* kept_idx,
                      int64_t* summary, int* n_kept) {
  const char* who = "sfm_view_triplets";
  SFM_TRY(tri_check(who, V, E, edges, rel, cos_loop, min_ok, min_pct, keep_untested, group));
  SFM_TRY(check_rotations_host(who, "Rel of edge %lld", E, rel, false));
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t m = (size_t)E;
  DevBuf<int> dE;
  DevBuf<double> dRel;
  DevBuf<unsigned char> dMask;
  HostOut<unsigned char> oKeep;
  HostOut<int64_t> oTri, oOk, oSum;
  HostOut<int> oIdx;
  SFM_TRY(dE.upload(edges, 2 * m, s));
  SFM_TRY(dRel.upload(rel, 9 * m, s));
  SFM_TRY(dMask.upload_if(edge_mask, m, s));
  SFM_TRY(oKeep.want(edge_keep, m, s)); SFM_TRY(oTri.want(n_tri, m, s)); SFM_TRY(oOk.want(n_ok, m, s));
  SFM_TRY(oIdx.want(kept_idx, m, s)); SFM_TRY(oSum.want(summary, 8, s));
  const TriArgs a = tri_args(V, E, dE.p, dRel.p, dMask.p, cos_loop, min_ok, min_pct, keep_untested, oKeep.dev(), oTri.dev(), oOk.dev(),
                             oIdx.dev(), oSum.dev());
  int count = 0;
  SFM_TRY(tri_run(a, group, &count, s));
  // only the first `count` entries of kept_idx were written: the rest of the caller's array stays as it was
  SFM_TRY(oKeep.fetch(s)); SFM_TRY(oTri.fetch(s)); SFM_TRY(oOk.fetch(s)); SFM_TRY(oSum.fetch(s));
  if (kept_idx != nullptr && count > 0) SFM_TRY(oIdx.buf.download(kept_idx, (size_t)count, s));
  if (n_kept != nullptr) *n_kept = count;
  return stream_sync(s);
}

}  // extern "C"
