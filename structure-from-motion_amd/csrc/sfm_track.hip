// sfm_track.hip — the key tracks of KeyTracker (key_tracker.py:14-59, 132-181, 213-317) resident on the device: per
// view the key coordinates and the KeyTrack.table, filled straight from the neighbour arrays sfm_match_dev leaves on
// the device.  Everything here is an integer or a copied coordinate, so the results equal the host path
// (structure-from-motion_amd/matching.py) exactly; the one floating-point decision is the ratio test, a correctly
// rounded fp64 division of two widened float32 values, as Python computes it.
//
// track_dedup_kernel: ONE workgroup of 1024 threads per reference view walks the new view's queries in chunks of 1024:
//   1. filter     keep(q) by mode; position in the filtered list = running base + wave offsets (__ballot + popcount
//                 inside a wave, 16 wave totals through LDS): the list keeps query order;
//   2. first(t)   atomicMin of the list position on a per-train-index array;
//   3. rank(t)    the same ordered compaction over the flags "position == first(train)";
//   4. cand(t)    atomicMax of the positions i > first(t) with dist[i] < dist[rank(t)] (quirk Q14: the threshold is the
//                 filtered list's element at position rank(t));
//   5. kept[rank(t)] = cand(t) if there is one, else first(t).
// Only integer atomics whose result does not depend on their order, so the output is independent of scheduling.
// The order of the filtered list is what makes a single workgroup per reference view the natural shape; the lists
// are a few thousand entries and a view is matched against at most a few dozen others, so the kernel is latency-bound
// (five passes separated by workgroup barriers), not throughput-bound.
//
// sfm_obs_build: the bundle adjustment's observation list (observations.build_observations: the loop of
// ba_processor.py:304-310 over KeyTracker.is_visible, key_tracker.py:198-204, quirk Q3) from the self rows table[v][v, :]
// and per-view tables of normalised key coordinates the host uploaded (inv(K) @ [u, v, 1] is a BLAS product on the host;
// the device only gathers its results):
//   mark    one thread per key: id = table[v][v, k]; for 0 <= id < n_pts atomicMin(min_key[v][id], k), atomicMax(max_key[v][id], k)
//   count   one thread per point: the views with max_key > 0 (np.any tests the index VALUES: a point whose only key is 0
//           is invisible)
//   scan    one workgroup: pt_ptr = exclusive scan of the counts
//   fill    one thread per point, views ascending: camera v, key min_key (key_idx[0][0]: index 0 included when another
//           matching index is non-zero) and the normalised coordinates of that key
// Integer atomics only, each independent of the order it is applied in; no floating-point arithmetic at all.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <vector>

#include "sfm_common.h"
#include "sfm_scan.h"
#include "sfm_track_link.h"

// the ratio test must be the plain division followed by the comparison
#pragma clang fp contract(off)

namespace {

constexpr int TB = sfm::kScanBlock; // threads of the single-workgroup kernels
constexpr int WAVES = TB / 64;
constexpr int ROWS_SPARE = 16;      // rows a table is allocated with beyond what it needs
constexpr double RATIO = 0.7;       // key_tracker.py:10

struct ViewDesc {                   // one view as the kernels see it
  int* table;                       // [rows_cap][n] int32, -1 filled
  const double* x;                  // [n]
  const double* y;                  // [n]
  int n;                            // keys
  int key_off;                      // sum of the key counts of the views before it (offset into per-train scratch)
  const double* nu;                 // [n] normalised coordinates (sfm_obs_set_normalised), NULL until they are set
  const double* nv;
};

// Position of this thread's element among the kept elements of the workgroup's current chunk, and their number.
// Every thread of the workgroup calls it.
__device__ __forceinline__ int chunk_offset(bool keep, int* wave_cnt, int& total) {
  const unsigned long long b = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int within = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();                  // the previous chunk's totals have been read
  if (lane == 0) wave_cnt[wave] = __popcll(b);
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int c = wave_cnt[w];
    before += w < wave ? c : 0;
    tot += c;
  }
  total = tot;
  return before + within;
}

// first[] and cand[] are written by device-scope atomics: read them at the same scope, past the vector L1
__device__ __forceinline__ int load_dev(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// info per reference view: {status, first offending query, filtered length, kept length}
__global__ __launch_bounds__(TB) void track_dedup_kernel(const ViewDesc* __restrict__ views, int nq, int mode,
                                                         const int* __restrict__ best_idx, const float* __restrict__ best_dist,
                                                         const int* __restrict__ second_idx, const float* __restrict__ second_dist,
                                                         const uint8_t* __restrict__ mutual, int* __restrict__ fq_all,
                                                         int* __restrict__ ft_all, float* __restrict__ fd_all, int* __restrict__ kq_all,
                                                         int* __restrict__ kt_all, int* __restrict__ tr_first, int* __restrict__ tr_rank,
                                                         int* __restrict__ tr_cand, int* __restrict__ info) {
  __shared__ int wave_cnt[WAVES];
  __shared__ int bad_key;           // min over the offending queries of (query << 2 | kind)
  const int r = blockIdx.x, tid = threadIdx.x;
  const ViewDesc ref = views[r];
  const int nt = ref.n;
  const size_t o = (size_t)r * nq;
  int* fq = fq_all + o; int* ft = ft_all + o; float* fd = fd_all + o;
  int* kq = kq_all + o; int* kt = kt_all + o;
  int* first = tr_first + ref.key_off; int* rank = tr_rank + ref.key_off; int* cand = tr_cand + ref.key_off;
  if (tid == 0) bad_key = INT_MAX;
  for (int t = tid; t < nt; t += TB) { first[t] = INT_MAX; cand[t] = -1; }
  __syncthreads();

  // 1. filter
  int m = 0;
  for (int base = 0; base < nq; base += TB) {
    const int q = base + tid;
    bool keep = false;
    int t = -1;
    float d = 0.f;
    if (q < nq) {
      t = best_idx[o + q];
      d = best_dist[o + q];
      if (mode == SFM_MATCH_MUTUAL) {
        keep = mutual[o + q] != 0 && t >= 0;
      } else if (mode == SFM_MATCH_KNN2) {
        const float d1 = second_dist[o + q];
        if (second_idx[o + q] < 0) atomicMin(&bad_key, (q << 2) | 0);
        else if (d1 == 0.f) atomicMin(&bad_key, (q << 2) | 1);
        else keep = (double)d / (double)d1 < RATIO;
      } else {
        keep = t >= 0;
      }
      if (keep && (t < 0 || t >= nt)) { atomicMin(&bad_key, (q << 2) | 2); keep = false; }
    }
    int total;
    const int pos = m + chunk_offset(keep, wave_cnt, total);
    if (keep) { fq[pos] = q; ft[pos] = t; fd[pos] = d; }
    m += total;
  }
  __syncthreads();                  // the list is written, bad_key is final
  const int bad = bad_key;
  if (bad != INT_MAX) {
    if (tid == 0) {
      const int kind = bad & 3;
      info[4 * r + 0] = kind == 0 ? SFM_TRACK_NO_SECOND : (kind == 1 ? SFM_TRACK_ZERO_SECOND : SFM_TRACK_BAD_TRAIN);
      info[4 * r + 1] = bad >> 2;
      info[4 * r + 2] = 0;
      info[4 * r + 3] = 0;
    }
    return;
  }

  // 2. first appearance of every train index
  for (int i = tid; i < m; i += TB) atomicMin(&first[ft[i]], i);
  __syncthreads();

  // 3. rank of the first appearances
  int u = 0;
  for (int base = 0; base < m; base += TB) {
    const int i = base + tid;
    int t = 0;
    bool is_first = false;
    if (i < m) { t = ft[i]; is_first = load_dev(&first[t]) == i; }
    int total;
    const int pos = u + chunk_offset(is_first, wave_cnt, total);
    if (is_first) rank[t] = pos;
    u += total;
  }
  __syncthreads();

  // 4. the last later match of t that beats the filtered list's element at rank(t)
  for (int i = tid; i < m; i += TB) {
    const int t = ft[i];
    if (i > load_dev(&first[t]) && fd[i] < fd[rank[t]]) atomicMax(&cand[t], i);
  }
  __syncthreads();

  // 5. one entry per distinct train index, at its rank
  for (int i = tid; i < m; i += TB) {
    const int t = ft[i];
    if (load_dev(&first[t]) == i) {
      const int c = load_dev(&cand[t]);
      kq[rank[t]] = fq[c >= 0 ? c : i];
      kt[rank[t]] = t;
    }
  }
  if (tid == 0) {
    info[4 * r + 0] = SFM_TRACK_OK;
    info[4 * r + 1] = -1;
    info[4 * r + 2] = m;
    info[4 * r + 3] = u;
  }
}

// table[ref][new_view, t] = q and table[new_view][ref, q] = t over the first `limit` kept entries (limit < 0: all) of the
// reference views ref0 + blockIdx.y.  chained: a view writes only if no view up to it has a status.
__global__ __launch_bounds__(256) void track_write_kernel(const ViewDesc* __restrict__ views, int new_view, int nq, int ref0, int limit,
                                                          int chained, const int* __restrict__ kq_all, const int* __restrict__ kt_all,
                                                          const int* __restrict__ info) {
  const int r = ref0 + blockIdx.y;
  for (int j = chained ? 0 : r; j <= r; ++j)
    if (info[4 * j] != SFM_TRACK_OK) return;
  int n = info[4 * r + 3];
  if (limit >= 0 && limit < n) n = limit;
  const ViewDesc ref = views[r], nv = views[new_view];
  const int* kq = kq_all + (size_t)r * nq;
  const int* kt = kt_all + (size_t)r * nq;
  int* ref_row = ref.table + (size_t)new_view * ref.n;
  int* new_row = nv.table + (size_t)r * nv.n;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const int q = kq[j], t = kt[j];             // t < ref.n was checked by the filter, q < nq = nv.n by construction
    ref_row[t] = q;
    new_row[q] = t;
  }
}

// generate_matched_pairs: one workgroup; a counting pass, then the ordered writes packed for the count.
__global__ __launch_bounds__(TB) void track_pairs_kernel(const ViewDesc* __restrict__ views, int ref, int que, int* __restrict__ count,
                                                         int* __restrict__ r_idx, int* __restrict__ q_idx, double* __restrict__ ref_pts,
                                                         double* __restrict__ que_pts) {
  __shared__ int wave_cnt[WAVES];
  __shared__ int flag;
  const int tid = threadIdx.x;
  const ViewDesc rv = views[ref], qv = views[que];
  const int* row = rv.table + (size_t)que * rv.n;
  if (tid == 0) flag = 0;
  int n = 0;
  for (int base = 0; base < rv.n; base += TB) {
    const int k = base + tid;
    int total;
    chunk_offset(k < rv.n && row[k] > 0, wave_cnt, total);
    n += total;
  }
  int at = 0;
  for (int base = 0; base < rv.n; base += TB) {
    const int k = base + tid;
    const int q = k < rv.n ? row[k] : -1;
    const bool keep = q > 0;
    int total;
    const int pos = at + chunk_offset(keep, wave_cnt, total);
    if (keep) {
      r_idx[pos] = k;
      q_idx[pos] = q;
      ref_pts[pos] = rv.x[k];
      ref_pts[n + pos] = rv.y[k];
      ref_pts[2 * (size_t)n + pos] = 1.0;
      const bool ok = q < qv.n;
      if (!ok) flag = 1;
      que_pts[pos] = ok ? qv.x[q] : NAN;
      que_pts[n + pos] = ok ? qv.y[q] : NAN;
      que_pts[2 * (size_t)n + pos] = 1.0;
    }
    at += total;
  }
  __syncthreads();
  if (tid == 0) { count[0] = n; count[1] = flag; }
}

// extract_constructed_points (want_used) / extract_unconstructed_points of the view's own row.
__global__ __launch_bounds__(TB) void track_usage_list_kernel(const ViewDesc* __restrict__ views, int view, int want_used,
                                                              int* __restrict__ count, int* __restrict__ keys, int* __restrict__ tri) {
  __shared__ int wave_cnt[WAVES];
  const int tid = threadIdx.x;
  const ViewDesc v = views[view];
  const int* row = v.table + (size_t)view * v.n;
  int at = 0;
  for (int base = 0; base < v.n; base += TB) {
    const int k = base + tid;
    const int val = k < v.n ? row[k] : -1;
    const bool keep = k < v.n && (want_used ? val != -1 : val == -1);
    int total;
    const int pos = at + chunk_offset(keep, wave_cnt, total);
    if (keep) { keys[pos] = k; tri[pos] = val; }
    at += total;
  }
  if (tid == 0) count[0] = at;
}

// update_usage, duplicates resolved as NumPy's fancy assignment does: the last entry of a key wins.
__global__ void track_usage_last_kernel(int n, const int* __restrict__ keys, int* __restrict__ last) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicMax(&last[keys[i]], i);
}
__global__ void track_usage_write_kernel(const ViewDesc* __restrict__ views, int view, int n, const int* __restrict__ keys,
                                         const int* __restrict__ tri, int* __restrict__ last) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = keys[i];
  if (load_dev(&last[k]) != i) return;
  const ViewDesc v = views[view];
  v.table[(size_t)view * v.n + k] = tri[i];
  last[k] = -1;                     // only the winner of a key resets it: the scratch is all -1 again afterwards
}

// set_pairs: row que of table[ref] and row ref of table[que] to -1, then the pairs (the host has checked the indices:
// in range, none repeated on either side, so every write has its own cell).
__global__ void track_pairs_clear_kernel(const ViewDesc* __restrict__ views, int ref, int que) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const ViewDesc r = views[ref], q = views[que];
  if (i < r.n) r.table[(size_t)que * r.n + i] = -1;
  if (i < q.n) q.table[(size_t)ref * q.n + i] = -1;
}
__global__ void track_pairs_write_kernel(const ViewDesc* __restrict__ views, int ref, int que, int n, const int* __restrict__ r_idx,
                                         const int* __restrict__ q_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ViewDesc r = views[ref], q = views[que];
  r.table[(size_t)que * r.n + r_idx[i]] = q_idx[i];
  q.table[(size_t)ref * q.n + q_idx[i]] = r_idx[i];
}

// ---- observation list ------------------------------------------------------------------------------------------
__global__ void obs_init_kernel(size_t cells, int* __restrict__ min_key, int* __restrict__ max_key) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < cells) { min_key[i] = INT_MAX; max_key[i] = -1; }
}

// grid (key chunks, views)
__global__ void obs_mark_kernel(const ViewDesc* __restrict__ views, int n_pts, int* __restrict__ min_key, int* __restrict__ max_key) {
  const int v = blockIdx.y;
  const ViewDesc w = views[v];
  const int* row = w.table + (size_t)v * w.n;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < w.n; k += gridDim.x * blockDim.x) {
    const int id = row[k];
    if (id >= 0 && id < n_pts) {
      atomicMin(&min_key[(size_t)v * n_pts + id], k);
      atomicMax(&max_key[(size_t)v * n_pts + id], k);
    }
  }
}

__global__ void obs_count_kernel(int n_views, int n_pts, const int* __restrict__ max_key, int* __restrict__ cnt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  int c = 0;
  for (int v = 0; v < n_views; ++v) c += max_key[(size_t)v * n_pts + p] > 0;
  cnt[p] = c;
}

// ptr = exclusive prefix sum of cnt, ptr[n] = the total (one workgroup)
__global__ __launch_bounds__(TB) void obs_scan_kernel(int n, const int* __restrict__ cnt, int* __restrict__ ptr) {
  sfm::block_exclusive_scan<1>(
      n, [&](int q, int (&a)[1]) { a[0] = cnt[q]; }, [&](int q, const int (&e)[1]) { ptr[q] = e[0]; },
      [&](const int (&t)[1]) { ptr[n] = t[0]; });
}

__global__ void obs_fill_kernel(const ViewDesc* __restrict__ views, int n_views, int n_pts, const int* __restrict__ min_key,
                                const int* __restrict__ max_key, const int* __restrict__ ptr, int* __restrict__ cam_idx,
                                int* __restrict__ key_idx, double* __restrict__ u, double* __restrict__ v_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  int w = ptr[p];
  for (int v = 0; v < n_views; ++v) {
    if (max_key[(size_t)v * n_pts + p] <= 0) continue;
    const int k = min_key[(size_t)v * n_pts + p];          // 0 <= k < views[v].n: a key index the mark kernel wrote
    cam_idx[w] = v;
    key_idx[w] = k;
    u[w] = views[v].nu[k];
    v_out[w] = views[v].nv[k];
    ++w;
  }
}

struct View {
  int n = 0, rows = 0, rows_cap = 0, key_off = 0;
  int* table = nullptr;
  double* xy = nullptr;             // x[n] then y[n]
  double* norm = nullptr;           // u[n] then v[n]: normalised coordinates, NULL until sfm_obs_set_normalised
};

// grow-only device buffer owned by the store
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(size_t want, int fill = -1) {
    if (want <= bytes && p) return SFM_OK;
    if (p) SFM_HIP(hipFree(p));     // hipFree waits for the device
    p = nullptr; bytes = 0;
    const size_t cap = want < 4096 ? 4096 : want + want / 2;
    SFM_HIP(hipMalloc(&p, cap));
    if (fill >= 0) SFM_HIP(hipMemset(p, fill, cap));
    bytes = cap;
    return SFM_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

}  // namespace

struct sfm_track_store {
  std::vector<View> views;
  ViewDesc* d_views = nullptr;      // [views_cap]
  int views_cap = 0;
  int total_keys = 0;
  Scratch lists;                    // fq, ft, fd, kq, kt: [n_refs][nq] each
  Scratch train;                    // first, rank, cand: [total keys of the reference views] each
  Scratch info;                     // [n_refs][4]
  Scratch usage_last;               // [max keys] ints, all -1 between calls
  Scratch staging;                  // host-form inputs and outputs
  Scratch neighbours;               // sfm_track_match_views: the five [n_refs][nq] arrays of sfm_match_dev
  int last_new = -1, last_refs = 0, last_nq = 0;   // what the kept lists in `lists` belong to
  // the observation list of the last sfm_obs_build
  Scratch obs_keys;                 // min_key, max_key: [n_views][n_pts] each, then cnt[n_pts]
  Scratch obs_ptr;                  // pt_ptr[n_pts + 1]
  Scratch obs_idx;                  // cam_idx[cap], key_idx[cap]
  Scratch obs_uv;                   // u[cap], v[cap]
  int obs_views = -1, obs_pts = 0, obs_cap = 0;      // obs_views < 0: no list
  long long obs_m = 0;
  hipStream_t pending = nullptr;    // the stream of the last enqueue that has not been waited for
  bool has_pending = false;
  int64_t upload_bytes = 0, download_bytes = 0;
};

using namespace sfm;

namespace {

inline hipStream_t pick(void* hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx().stream; }

// An enqueuing entry point notes its stream; a blocking one settles it before it touches what the kernels read or
// write.  Only one stream is remembered: an enqueue on another stream first waits for the one before it.
int note_stream(sfm_track_store* s, hipStream_t st) {
  if (s->has_pending && s->pending != st) SFM_HIP(hipStreamSynchronize(s->pending));
  s->pending = st; s->has_pending = true;
  return SFM_OK;
}

int settle(sfm_track_store* s) {
  if (s->has_pending) SFM_HIP(hipStreamSynchronize(s->pending));
  s->has_pending = false;
  return SFM_OK;
}

// device allocations of an entry point that has not committed them to the store yet
struct Uncommitted {
  std::vector<void*> ptrs;
  ~Uncommitted() { for (void* p : ptrs) (void)hipFree(p); }
  int alloc(void** out, size_t bytes) {
    SFM_HIP(hipMalloc(out, bytes));
    ptrs.push_back(*out);
    return SFM_OK;
  }
  void commit() { ptrs.clear(); }
};

inline int* list_ptr(const sfm_track_store* s, int which) {      // 0 fq, 1 ft, 2 fd, 3 kq, 4 kt
  return static_cast<int*>(s->lists.p) + (size_t)which * s->last_refs * (s->last_nq > 0 ? s->last_nq : 1);
}

inline ViewDesc desc_of(const View& w) {
  return ViewDesc{w.table, w.xy, w.xy + w.n, w.n, w.key_off, w.norm, w.norm ? w.norm + w.n : nullptr};
}

// 2 V n_pts ints of min_key / max_key scratch at the most (1 GiB); beyond it sfm_obs_build returns SFM_E_SHAPE
constexpr size_t OBS_SCRATCH_CAP = (size_t)1 << 28;

int table_alloc(Uncommitted& mem, View& w, int rows_cap) {
  const size_t bytes = sizeof(int) * (size_t)rows_cap * (w.n > 0 ? w.n : 1);
  SFM_TRY(mem.alloc(reinterpret_cast<void**>(&w.table), bytes));
  SFM_HIP(hipMemset(w.table, 0xFF, bytes));                    // every int -1
  w.rows_cap = rows_cap;
  return SFM_OK;
}

int valid_view(const sfm_track_store* s, int view, const char* who) {
  if (view < 0 || view >= (int)s->views.size()) { set_error("%s: view %d of %d", who, view, (int)s->views.size()); return SFM_E_SHAPE; }
  return SFM_OK;
}

int run_dedup(sfm_track_store* s, int new_view, int n_refs, int mode, const int* bi, const float* bd, const int* si, const float* sd,
              const uint8_t* mu, hipStream_t st) {
  SFM_TRY(valid_view(s, new_view, "sfm_track_extend"));
  if (n_refs < 0 || n_refs > new_view) { set_error("sfm_track_extend: %d reference views for view %d", n_refs, new_view); return SFM_E_SHAPE; }
  if (mode != SFM_MATCH_KNN2 && mode != SFM_MATCH_NN1 && mode != SFM_MATCH_MUTUAL) { set_error("sfm_track_extend: unknown mode %d", mode); return SFM_E_SHAPE; }
  const View& nv = s->views[new_view];
  const int nq = nv.n;
  if ((size_t)nq >= (1u << 29)) { set_error("sfm_track_extend: %d queries", nq); return SFM_E_SHAPE; }
  if (nv.rows < n_refs) { set_error("sfm_track_extend: the new view's table has %d rows for %d reference views", nv.rows, n_refs); return SFM_E_SHAPE; }
  for (int r = 0; r < n_refs; ++r)
    if (s->views[r].rows <= new_view) { set_error("sfm_track_extend: table %d has no row %d", r, new_view); return SFM_E_SHAPE; }
  if (n_refs > 0 && nq > 0) {
    const bool need2 = mode == SFM_MATCH_KNN2, needm = mode == SFM_MATCH_MUTUAL;
    if (!bi || !bd || (need2 && (!si || !sd)) || (needm && !mu)) { set_error("sfm_track_extend: a neighbour array of mode %d is NULL", mode); return SFM_E_SHAPE; }
  }
  s->last_new = new_view; s->last_refs = n_refs; s->last_nq = nq;
  if (n_refs == 0) return SFM_OK;
  SFM_TRY(note_stream(s, st));
  const size_t cells = (size_t)n_refs * (nq > 0 ? nq : 1);
  SFM_TRY(s->lists.reserve(5 * cells * sizeof(int)));
  SFM_TRY(s->train.reserve(3 * sizeof(int) * (size_t)(s->total_keys > 0 ? s->total_keys : 1)));
  SFM_TRY(s->info.reserve(4 * sizeof(int) * (size_t)n_refs));
  int* tr = static_cast<int*>(s->train.p);
  const size_t tk = (size_t)(s->total_keys > 0 ? s->total_keys : 1);
  track_dedup_kernel<<<n_refs, TB, 0, st>>>(s->d_views, nq, mode, bi, bd, si, sd, mu, list_ptr(s, 0), list_ptr(s, 1),
                                            reinterpret_cast<float*>(list_ptr(s, 2)), list_ptr(s, 3), list_ptr(s, 4), tr, tr + tk, tr + 2 * tk,
                                            static_cast<int*>(s->info.p));
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

int run_write(sfm_track_store* s, int ref0, int n_refs, int limit, int chained, hipStream_t st) {
  if (n_refs <= 0 || s->last_nq <= 0) return SFM_OK;
  SFM_TRY(note_stream(s, st));
  const int bx = (s->last_nq + 255) / 256 < 64 ? (s->last_nq + 255) / 256 : 64;
  track_write_kernel<<<dim3((unsigned)bx, (unsigned)n_refs), 256, 0, st>>>(s->d_views, s->last_new, s->last_nq, ref0, limit, chained,
                                                                          list_ptr(s, 3), list_ptr(s, 4), static_cast<int*>(s->info.p));
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// blocking: the list track_usage_list_kernel left in staging as {count, a[cap], b[cap]}
int fetch_list(sfm_track_store* s, hipStream_t st, int cap, int* n, int* a, int* b) {
  int* base = static_cast<int*>(s->staging.p);
  int cnt = 0;
  SFM_HIP(hipMemcpyAsync(&cnt, base, sizeof(cnt), hipMemcpyDeviceToHost, st));
  SFM_TRY(stream_sync(st));
  s->download_bytes += (int64_t)sizeof(cnt);
  if (cnt > 0) {
    if (a) { SFM_HIP(hipMemcpyAsync(a, base + 1, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, st)); s->download_bytes += 4ll * cnt; }
    if (b) { SFM_HIP(hipMemcpyAsync(b, base + 1 + cap, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, st)); s->download_bytes += 4ll * cnt; }
    SFM_TRY(stream_sync(st));
  }
  *n = cnt;
  return SFM_OK;
}

int usage_list(sfm_track_store* s, int view, int want_used, int* n, int* keys, int* tri) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (!n) { set_error("sfm_track usage list: n is NULL"); return SFM_E_SHAPE; }
  SFM_TRY(valid_view(s, view, "sfm_track usage list"));
  const View& w = s->views[view];
  if (w.rows <= view) { set_error("sfm_track usage list: table %d has no row %d", view, view); return SFM_E_SHAPE; }
  *n = 0;
  if (w.n == 0) return SFM_OK;
  hipStream_t st = ctx().stream;
  SFM_TRY(settle(s));
  SFM_TRY(s->staging.reserve(sizeof(int) * (1 + 2 * (size_t)w.n)));
  int* base = static_cast<int*>(s->staging.p);
  track_usage_list_kernel<<<1, TB, 0, st>>>(s->d_views, view, want_used, base, base + 1, base + 1 + w.n);
  SFM_HIP(hipGetLastError());
  return fetch_list(s, st, w.n, n, keys, tri);
}

}  // namespace

extern "C" {

int sfm_track_create(sfm_track_store** out) {
  SFM_TRY(ensure_init());
  if (!out) { set_error("sfm_track_create: out is NULL"); return SFM_E_SHAPE; }
  *out = new sfm_track_store();
  return SFM_OK;
}

int sfm_track_destroy(sfm_track_store* s) {
  if (!s) return SFM_E_HANDLE;
  (void)settle(s);
  (void)hipStreamSynchronize(ctx().stream);
  for (View& w : s->views) {
    if (w.table) (void)hipFree(w.table);
    if (w.xy) (void)hipFree(w.xy);
    if (w.norm) (void)hipFree(w.norm);
  }
  if (s->d_views) (void)hipFree(s->d_views);
  s->obs_keys.release(); s->obs_ptr.release(); s->obs_idx.release(); s->obs_uv.release();
  s->lists.release(); s->train.release(); s->info.release(); s->usage_last.release(); s->staging.release(); s->neighbours.release();
  delete s;
  return SFM_OK;
}

int sfm_track_info(const sfm_track_store* s, int what, int view, int64_t* value) {
  if (!s) return SFM_E_HANDLE;
  if (!value) return SFM_E_SHAPE;
  switch (what) {
    case SFM_TRACK_INFO_N_VIEWS: *value = (int64_t)s->views.size(); return SFM_OK;
    case SFM_TRACK_INFO_UPLOAD_BYTES: *value = s->upload_bytes; return SFM_OK;
    case SFM_TRACK_INFO_DOWNLOAD_BYTES: *value = s->download_bytes; return SFM_OK;
    case SFM_TRACK_INFO_OBS_VIEWS: *value = s->obs_views; return SFM_OK;
    case SFM_TRACK_INFO_OBS_PTS: *value = s->obs_views < 0 ? 0 : s->obs_pts; return SFM_OK;
    case SFM_TRACK_INFO_N_OBS: *value = s->obs_views < 0 ? 0 : s->obs_m; return SFM_OK;
    case SFM_TRACK_INFO_N_KEYS:
    case SFM_TRACK_INFO_N_ROWS:
      SFM_TRY(valid_view(s, view, "sfm_track_info"));
      *value = what == SFM_TRACK_INFO_N_KEYS ? s->views[view].n : s->views[view].rows;
      return SFM_OK;
    default: set_error("sfm_track_info: unknown item %d", what); return SFM_E_SHAPE;
  }
}

int sfm_track_add_view(sfm_track_store* s, int n, const double* x, const double* y, int* view_out) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (n < 0 || (n > 0 && (!x || !y))) { set_error("sfm_track_add_view: bad sizes n=%d", n); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));                                 // tables and the descriptor array may be replaced below
  SFM_TRY(stream_sync(ctx().stream));
  const int v = (int)s->views.size();
  // Everything that can fail comes first and touches nothing the store owns; a failure frees it and leaves the store as
  // it was.  The store changes only after the last of it.
  Uncommitted mem;
  const int cap = v + 1 > s->views_cap ? (s->views_cap ? 2 * s->views_cap : 32) : s->views_cap;
  ViewDesc* d_views = s->d_views;
  if (cap != s->views_cap) SFM_TRY(mem.alloc(reinterpret_cast<void**>(&d_views), sizeof(ViewDesc) * (size_t)cap));
  // one more row for every existing table (key_tracker.py:236-237): already -1, only a table out of spare rows moves
  std::vector<View> next(s->views);
  for (View& w : next) {
    if (w.rows == w.rows_cap) {
      const int* old = w.table;
      SFM_TRY(table_alloc(mem, w, 2 * w.rows_cap));
      if (w.n) SFM_HIP(hipMemcpy(w.table, old, sizeof(int) * (size_t)w.rows * w.n, hipMemcpyDeviceToDevice));
    }
    ++w.rows;
  }
  View w;
  w.n = n; w.rows = v + 1; w.key_off = s->total_keys;
  SFM_TRY(mem.alloc(reinterpret_cast<void**>(&w.xy), sizeof(double) * 2 * (size_t)(n > 0 ? n : 1)));
  if (n) {
    SFM_HIP(hipMemcpy(w.xy, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    SFM_HIP(hipMemcpy(w.xy + n, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  }
  SFM_TRY(table_alloc(mem, w, v + 1 + ROWS_SPARE));
  next.push_back(w);
  std::vector<ViewDesc> descs;
  for (const View& e : next) descs.push_back(desc_of(e));
  // one copy, the last thing that can fail: a new array takes every view, the old one the views from the first table
  // that moved on
  int lo = d_views != s->d_views ? 0 : v;
  for (int i = v - 1; i >= 0; --i)
    if (next[i].table != s->views[i].table) lo = i < lo ? i : lo;
  SFM_HIP(hipMemcpy(d_views + lo, descs.data() + lo, sizeof(ViewDesc) * (size_t)(v + 1 - lo), hipMemcpyHostToDevice));
  // commit: nothing below fails
  mem.commit();
  for (int i = 0; i < v; ++i)
    if (next[i].table != s->views[i].table) (void)hipFree(s->views[i].table);
  if (d_views != s->d_views && s->d_views) (void)hipFree(s->d_views);
  s->d_views = d_views; s->views_cap = cap;
  s->views.swap(next);
  s->total_keys += n;
  s->upload_bytes += 16ll * n;
  if (view_out) *view_out = v;
  return SFM_OK;
}

int sfm_track_drop_last_view(sfm_track_store* s) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (s->views.empty()) { set_error("sfm_track_drop_last_view: the store has no view"); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));
  SFM_TRY(stream_sync(ctx().stream));
  View& w = s->views.back();
  s->total_keys -= w.n;
  if (w.table) (void)hipFree(w.table);
  if (w.xy) (void)hipFree(w.xy);
  if (w.norm) (void)hipFree(w.norm);
  s->views.pop_back();
  s->last_new = -1; s->last_refs = 0; s->last_nq = 0;
  return SFM_OK;
}

int sfm_track_match_dedup_dev(sfm_track_store* s, int new_view, int n_refs, int mode, const int* d_best_idx, const float* d_best_dist,
                              const int* d_second_idx, const float* d_second_dist, const uint8_t* d_mutual, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  return run_dedup(s, new_view, n_refs, mode, d_best_idx, d_best_dist, d_second_idx, d_second_dist, d_mutual, pick(hip_stream));
}

int sfm_track_extend_dev(sfm_track_store* s, int new_view, int n_refs, int mode, const int* d_best_idx, const float* d_best_dist,
                         const int* d_second_idx, const float* d_second_dist, const uint8_t* d_mutual, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  hipStream_t st = pick(hip_stream);
  SFM_TRY(run_dedup(s, new_view, n_refs, mode, d_best_idx, d_best_dist, d_second_idx, d_second_dist, d_mutual, st));
  return run_write(s, 0, n_refs, -1, 1, st);
}

int sfm_track_match_views(sfm_track_store* s, int new_view, sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, int mode,
                          int write, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!s || !query) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, new_view, "sfm_track_match_views"));
  int64_t qn = 0;
  SFM_TRY(sfm_desc_info(query, SFM_DESC_INFO_N, &qn));
  const int nq = s->views[new_view].n;
  if (qn != nq) { set_error("sfm_track_match_views: %d descriptors for a view of %d keys", (int)qn, nq); return SFM_E_SHAPE; }
  if (n_refs < 0 || n_refs > new_view) { set_error("sfm_track_match_views: %d reference views for view %d", n_refs, new_view); return SFM_E_SHAPE; }
  hipStream_t st = pick(hip_stream);
  const size_t cells = (size_t)(n_refs > 0 ? n_refs : 1) * (nq > 0 ? nq : 1);
  SFM_TRY(s->neighbours.reserve(cells * 17));
  int* bi = static_cast<int*>(s->neighbours.p);
  float* bd = reinterpret_cast<float*>(bi + cells);
  int* si = bi + 2 * cells;
  float* sd = reinterpret_cast<float*>(bi + 3 * cells);
  uint8_t* mu = reinterpret_cast<uint8_t*>(bi + 4 * cells);
  SFM_TRY(note_stream(s, st));                        // an earlier dedup on another stream may still read `neighbours`
  SFM_TRY(sfm_match_dev(query, n_refs, refs, mode, bi, bd, si, sd, mu, st));
  SFM_TRY(run_dedup(s, new_view, n_refs, mode, bi, bd, si, sd, mu, st));
  return write ? run_write(s, 0, n_refs, -1, 1, st) : SFM_OK;
}

int sfm_track_extend_status(sfm_track_store* s, int n_refs, int* status, int* first_bad, int* n_kept) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (n_refs != s->last_refs) { set_error("sfm_track_extend_status: %d reference views, the last extend had %d", n_refs, s->last_refs); return SFM_E_SHAPE; }
  if (n_refs == 0) return SFM_OK;
  std::vector<int> h(4 * (size_t)n_refs);
  SFM_TRY(settle(s));                                 // the extend may have run on a caller's stream
  SFM_HIP(hipMemcpy(h.data(), s->info.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
  s->download_bytes += (int64_t)(sizeof(int) * h.size());
  for (int r = 0; r < n_refs; ++r) {
    if (status) status[r] = h[4 * r];
    if (first_bad) first_bad[r] = h[4 * r + 1];
    if (n_kept) n_kept[r] = h[4 * r + 3];
  }
  return SFM_OK;
}

int sfm_track_kept_copy(sfm_track_store* s, int ref, int* q, int* t) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (ref < 0 || ref >= s->last_refs) { set_error("sfm_track_kept_copy: reference view %d of %d", ref, s->last_refs); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));
  int h[4];
  SFM_HIP(hipMemcpy(h, static_cast<int*>(s->info.p) + 4 * ref, sizeof(h), hipMemcpyDeviceToHost));
  s->download_bytes += (int64_t)sizeof(h);
  const int n = h[3];
  if (n <= 0) return SFM_OK;
  const size_t o = (size_t)ref * s->last_nq;
  if (q) { SFM_HIP(hipMemcpy(q, list_ptr(s, 3) + o, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost)); s->download_bytes += 4ll * n; }
  if (t) { SFM_HIP(hipMemcpy(t, list_ptr(s, 4) + o, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost)); s->download_bytes += 4ll * n; }
  return SFM_OK;
}

int sfm_track_write_kept(sfm_track_store* s, int ref, int n, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (ref < 0 || ref >= s->last_refs) { set_error("sfm_track_write_kept: reference view %d of %d", ref, s->last_refs); return SFM_E_SHAPE; }
  return run_write(s, ref, 1, n, 0, pick(hip_stream));
}

int sfm_track_pairs_dev(sfm_track_store* s, int ref, int que, int* d_count, int* d_r_idx, int* d_q_idx, double* d_ref_pts,
                        double* d_que_pts, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, ref, "sfm_track_pairs"));
  SFM_TRY(valid_view(s, que, "sfm_track_pairs"));
  if (s->views[ref].rows <= que) { set_error("sfm_track_pairs: table %d has no row %d", ref, que); return SFM_E_SHAPE; }
  if (!d_count || !d_r_idx || !d_q_idx || !d_ref_pts || !d_que_pts) { set_error("sfm_track_pairs: an output is NULL"); return SFM_E_SHAPE; }
  hipStream_t st = pick(hip_stream);
  SFM_TRY(note_stream(s, st));
  track_pairs_kernel<<<1, TB, 0, st>>>(s->d_views, ref, que, d_count, d_r_idx, d_q_idx, d_ref_pts, d_que_pts);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

int sfm_track_pairs(sfm_track_store* s, int ref, int que, int* n, int* r_idx, int* q_idx, double* ref_pts, double* que_pts) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (!n) { set_error("sfm_track_pairs: n is NULL"); return SFM_E_SHAPE; }
  SFM_TRY(valid_view(s, ref, "sfm_track_pairs"));
  const size_t cap = (size_t)(s->views[ref].n > 0 ? s->views[ref].n : 1);
  // staging: ref_pts[3 cap], que_pts[3 cap] doubles, then count[2], r_idx[cap], q_idx[cap] ints
  SFM_TRY(s->staging.reserve(6 * cap * sizeof(double) + (2 + 2 * cap) * sizeof(int)));
  double* d_ref = static_cast<double*>(s->staging.p);
  double* d_que = d_ref + 3 * cap;
  int* d_cnt = reinterpret_cast<int*>(d_que + 3 * cap);
  hipStream_t st = ctx().stream;
  SFM_TRY(sfm_track_pairs_dev(s, ref, que, d_cnt, d_cnt + 2, d_cnt + 2 + cap, d_ref, d_que, st));
  int cnt[2] = {0, 0};
  SFM_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
  SFM_TRY(stream_sync(st));
  s->has_pending = false;                             // pairs_dev noted st, and st has just been waited for
  s->download_bytes += (int64_t)sizeof(cnt);
  *n = cnt[0];
  if (cnt[1]) { set_error("sfm_track_pairs: table %d row %d names a key the view %d does not have", ref, que, que); return SFM_E_SHAPE; }
  if (cnt[0] > 0) {
    const size_t c = (size_t)cnt[0];
    if (r_idx) { SFM_HIP(hipMemcpyAsync(r_idx, d_cnt + 2, 4 * c, hipMemcpyDeviceToHost, st)); s->download_bytes += 4ll * cnt[0]; }
    if (q_idx) { SFM_HIP(hipMemcpyAsync(q_idx, d_cnt + 2 + cap, 4 * c, hipMemcpyDeviceToHost, st)); s->download_bytes += 4ll * cnt[0]; }
    if (ref_pts) { SFM_HIP(hipMemcpyAsync(ref_pts, d_ref, 24 * c, hipMemcpyDeviceToHost, st)); s->download_bytes += 24ll * cnt[0]; }
    if (que_pts) { SFM_HIP(hipMemcpyAsync(que_pts, d_que, 24 * c, hipMemcpyDeviceToHost, st)); s->download_bytes += 24ll * cnt[0]; }
    SFM_TRY(stream_sync(st));
  }
  return SFM_OK;
}

int sfm_track_update_usage(sfm_track_store* s, int view, int n, const int* keys, const int* tri) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, view, "sfm_track_update_usage"));
  const View& w = s->views[view];
  if (n < 0 || (n > 0 && (!keys || !tri))) { set_error("sfm_track_update_usage: bad sizes n=%d", n); return SFM_E_SHAPE; }
  if (w.rows <= view) { set_error("sfm_track_update_usage: table %d has no row %d", view, view); return SFM_E_SHAPE; }
  for (int i = 0; i < n; ++i)
    if (keys[i] < 0 || keys[i] >= w.n) { set_error("sfm_track_update_usage: key %d of a view with %d keys", keys[i], w.n); return SFM_E_SHAPE; }
  if (n == 0) return SFM_OK;
  hipStream_t st = ctx().stream;
  SFM_TRY(settle(s));
  SFM_TRY(s->usage_last.reserve(sizeof(int) * (size_t)w.n, 0xFF));
  DevBuf<int> dk, dt;
  SFM_TRY(dk.upload(keys, (size_t)n, st));
  SFM_TRY(dt.upload(tri, (size_t)n, st));
  s->upload_bytes += 8ll * n;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  int* last = static_cast<int*>(s->usage_last.p);
  track_usage_last_kernel<<<blocks, 256, 0, st>>>(n, dk.p, last);
  track_usage_write_kernel<<<blocks, 256, 0, st>>>(s->d_views, view, n, dk.p, dt.p, last);
  SFM_HIP(hipGetLastError());
  return stream_sync(st);
}

int sfm_match_guided_track(sfm_track_store* s, int que_view, sfm_desc_set* query, int n_refs, const int* ref_views,
                           sfm_desc_set* const* refs, const int* kind, const double* model, double max_err2, int* d_best_idx,
                           float* d_best_dist, int* d_second_idx, float* d_second_dist, uint8_t* d_mutual, int* d_n_admitted,
                           void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!s || !query) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, que_view, "sfm_match_guided_track"));
  if (n_refs < 0 || (n_refs > 0 && (!ref_views || !refs))) { set_error("sfm_match_guided_track: bad reference list"); return SFM_E_SHAPE; }
  int64_t cnt = 0;
  SFM_TRY(sfm_desc_info(query, SFM_DESC_INFO_N, &cnt));
  const View& qv = s->views[que_view];
  if (cnt != qv.n) { set_error("sfm_match_guided_track: %d descriptors for a view of %d keys", (int)cnt, qv.n); return SFM_E_SHAPE; }
  std::vector<const double*> rx((size_t)n_refs), ry((size_t)n_refs);
  for (int r = 0; r < n_refs; ++r) {
    SFM_TRY(valid_view(s, ref_views[r], "sfm_match_guided_track"));
    if (!refs[r]) return SFM_E_HANDLE;
    const View& w = s->views[ref_views[r]];
    SFM_TRY(sfm_desc_info(refs[r], SFM_DESC_INFO_N, &cnt));
    if (cnt != w.n) { set_error("sfm_match_guided_track: %d descriptors for view %d of %d keys", (int)cnt, ref_views[r], w.n); return SFM_E_SHAPE; }
    rx[r] = w.xy;
    ry[r] = w.xy + w.n;
  }
  hipStream_t st = pick(hip_stream);
  SFM_TRY(note_stream(s, st));
  return sfm_match_guided_dev(query, qv.xy, qv.xy + qv.n, n_refs, refs, rx.data(), ry.data(), kind, model, max_err2, d_best_idx,
                              d_best_dist, d_second_idx, d_second_dist, d_mutual, d_n_admitted, st);
}

int sfm_match_guided_set_pairs(sfm_track_store* s, int ref, int que, int n, const int* r_idx, const int* q_idx) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, ref, "sfm_match_guided_set_pairs"));
  SFM_TRY(valid_view(s, que, "sfm_match_guided_set_pairs"));
  if (ref == que) { set_error("sfm_match_guided_set_pairs: view %d against itself", ref); return SFM_E_SHAPE; }
  const View& rv = s->views[ref];
  const View& qv = s->views[que];
  if (rv.rows <= que || qv.rows <= ref) { set_error("sfm_match_guided_set_pairs: tables %d and %d have no rows for each other", ref, que); return SFM_E_SHAPE; }
  if (n < 0 || (n > 0 && (!r_idx || !q_idx))) { set_error("sfm_match_guided_set_pairs: bad sizes n=%d", n); return SFM_E_SHAPE; }
  std::vector<char> seen_r((size_t)rv.n, 0), seen_q((size_t)qv.n, 0);
  for (int i = 0; i < n; ++i) {
    if (r_idx[i] < 0 || r_idx[i] >= rv.n || q_idx[i] < 0 || q_idx[i] >= qv.n) {
      set_error("sfm_match_guided_set_pairs: pair %d (%d, %d) outside views of %d and %d keys", i, r_idx[i], q_idx[i], rv.n, qv.n);
      return SFM_E_SHAPE;
    }
    if (seen_r[r_idx[i]] || seen_q[q_idx[i]]) { set_error("sfm_match_guided_set_pairs: pair %d (%d, %d) repeats a key", i, r_idx[i], q_idx[i]); return SFM_E_SHAPE; }
    seen_r[r_idx[i]] = seen_q[q_idx[i]] = 1;
  }
  hipStream_t st = ctx().stream;
  SFM_TRY(settle(s));
  DevBuf<int> dr, dq;
  SFM_TRY(dr.upload(r_idx, (size_t)n, st));
  SFM_TRY(dq.upload(q_idx, (size_t)n, st));
  s->upload_bytes += 8ll * n;
  const int widest = rv.n > qv.n ? rv.n : qv.n;
  if (widest > 0) track_pairs_clear_kernel<<<(unsigned)((widest + 255) / 256), 256, 0, st>>>(s->d_views, ref, que);
  if (n > 0) track_pairs_write_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(s->d_views, ref, que, n, dr.p, dq.p);
  SFM_HIP(hipGetLastError());
  return stream_sync(st);
}

int sfm_track_constructed(sfm_track_store* s, int view, int* n, int* keys, int* tri) { return usage_list(s, view, 1, n, keys, tri); }

int sfm_track_unconstructed(sfm_track_store* s, int view, int* n, int* keys) { return usage_list(s, view, 0, n, keys, nullptr); }

int sfm_track_copy_table(sfm_track_store* s, int view, int* out) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, view, "sfm_track_copy_table"));
  const View& w = s->views[view];
  const size_t bytes = sizeof(int) * (size_t)w.rows * w.n;
  if (bytes == 0) return SFM_OK;
  if (!out) { set_error("sfm_track_copy_table: out is NULL"); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));
  SFM_HIP(hipMemcpy(out, w.table, bytes, hipMemcpyDeviceToHost));
  s->download_bytes += (int64_t)bytes;
  return SFM_OK;
}

int sfm_track_copy_row(sfm_track_store* s, int view, int row, int* out) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, view, "sfm_track_copy_row"));
  const View& w = s->views[view];
  if (row < 0 || row >= w.rows) { set_error("sfm_track_copy_row: row %d of %d", row, w.rows); return SFM_E_SHAPE; }
  if (w.n == 0) return SFM_OK;
  if (!out) { set_error("sfm_track_copy_row: out is NULL"); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));
  SFM_HIP(hipMemcpy(out, w.table + (size_t)row * w.n, sizeof(int) * (size_t)w.n, hipMemcpyDeviceToHost));
  s->download_bytes += 4ll * w.n;
  return SFM_OK;
}

int sfm_obs_set_normalised(sfm_track_store* s, int view, int n, const double* u, const double* v) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  SFM_TRY(valid_view(s, view, "sfm_obs_set_normalised"));
  View& w = s->views[view];
  if (n != w.n || (n > 0 && (!u || !v))) { set_error("sfm_obs_set_normalised: %d coordinates for a view of %d keys", n, w.n); return SFM_E_SHAPE; }
  if (n == 0) return SFM_OK;
  SFM_TRY(settle(s));                                 // no kernel reads the table that is replaced
  SFM_TRY(stream_sync(ctx().stream));
  if (!w.norm) {
    Uncommitted mem;
    double* norm = nullptr;
    SFM_TRY(mem.alloc(reinterpret_cast<void**>(&norm), sizeof(double) * 2 * (size_t)n));
    View next = w;
    next.norm = norm;
    const ViewDesc d = desc_of(next);
    SFM_HIP(hipMemcpy(s->d_views + view, &d, sizeof(d), hipMemcpyHostToDevice));
    mem.commit();
    w.norm = norm;
  }
  SFM_HIP(hipMemcpy(w.norm, u, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  SFM_HIP(hipMemcpy(w.norm + n, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  s->upload_bytes += 16ll * n;
  return SFM_OK;
}

int sfm_obs_build(sfm_track_store* s, int n_views, int n_pts, int64_t* n_obs) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (n_views < 0 || n_views > (int)s->views.size() || n_pts < 0) {
    set_error("sfm_obs_build: %d views of %d, %d points", n_views, (int)s->views.size(), n_pts);
    return SFM_E_SHAPE;
  }
  const size_t cells = (size_t)n_views * (size_t)n_pts;
  if (2 * cells > OBS_SCRATCH_CAP) {
    set_error("sfm_obs_build: %d views x %d points need more than %zu ints of scratch", n_views, n_pts, OBS_SCRATCH_CAP);
    return SFM_E_SHAPE;
  }
  long long keys = 0;                                 // an observation has a key of its own: M <= the keys of the views
  int max_n = 0;
  for (int v = 0; v < n_views; ++v) {
    const View& w = s->views[v];
    if (w.n > 0 && !w.norm) { set_error("sfm_obs_build: view %d has no normalised coordinates", v); return SFM_E_SHAPE; }
    if (w.rows <= v) { set_error("sfm_obs_build: table %d has no row %d", v, v); return SFM_E_SHAPE; }
    keys += w.n;
    max_n = w.n > max_n ? w.n : max_n;
  }
  const size_t cap = (size_t)(keys < (long long)cells ? keys : (long long)cells);
  if (cap > 0x7fffffffull) { set_error("sfm_obs_build: too many observations"); return SFM_E_SHAPE; }
  hipStream_t st = ctx().stream;
  SFM_TRY(settle(s));
  s->obs_views = -1;
  SFM_TRY(s->obs_keys.reserve(sizeof(int) * (2 * cells + (size_t)n_pts + 1)));
  SFM_TRY(s->obs_ptr.reserve(sizeof(int) * ((size_t)n_pts + 1)));
  SFM_TRY(s->obs_idx.reserve(sizeof(int) * 2 * (cap + 1)));
  SFM_TRY(s->obs_uv.reserve(sizeof(double) * 2 * (cap + 1)));
  int* min_key = static_cast<int*>(s->obs_keys.p);
  int* max_key = min_key + cells;
  int* cnt = max_key + cells;
  int* ptr = static_cast<int*>(s->obs_ptr.p);
  int* cam = static_cast<int*>(s->obs_idx.p);
  double* u = static_cast<double*>(s->obs_uv.p);
  if (cells > 0) {
    obs_init_kernel<<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(cells, min_key, max_key);
    if (max_n > 0) {
      const int bx = (max_n + 255) / 256 < 64 ? (max_n + 255) / 256 : 64;
      obs_mark_kernel<<<dim3((unsigned)bx, (unsigned)n_views), 256, 0, st>>>(s->d_views, n_pts, min_key, max_key);
    }
  }
  if (n_pts > 0) obs_count_kernel<<<(n_pts + 255) / 256, 256, 0, st>>>(n_views, n_pts, max_key, cnt);
  obs_scan_kernel<<<1, TB, 0, st>>>(n_pts, cnt, ptr);
  if (cells > 0) obs_fill_kernel<<<(n_pts + 255) / 256, 256, 0, st>>>(s->d_views, n_views, n_pts, min_key, max_key, ptr, cam, cam + cap + 1, u, u + cap + 1);
  SFM_HIP(hipGetLastError());
  int m = 0;
  SFM_HIP(hipMemcpyAsync(&m, ptr + n_pts, sizeof(m), hipMemcpyDeviceToHost, st));
  SFM_TRY(stream_sync(st));                           // (the count is the call's result, not data of the store: not in download_bytes)
  s->obs_views = n_views; s->obs_pts = n_pts; s->obs_cap = (int)cap; s->obs_m = m;
  if (n_obs) *n_obs = m;
  return SFM_OK;
}

int sfm_obs_copy(sfm_track_store* s, int* pt_ptr, int* cam_idx, int* key_idx, double* uv) {
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  if (s->obs_views < 0) { set_error("sfm_obs_copy: no observation list has been built"); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));
  const size_t m = (size_t)s->obs_m, cap1 = (size_t)s->obs_cap + 1;
  const int* cam = static_cast<const int*>(s->obs_idx.p);
  const double* u = static_cast<const double*>(s->obs_uv.p);
  if (pt_ptr) { SFM_HIP(hipMemcpy(pt_ptr, s->obs_ptr.p, sizeof(int) * ((size_t)s->obs_pts + 1), hipMemcpyDeviceToHost)); s->download_bytes += 4ll * (s->obs_pts + 1); }
  if (m == 0) return SFM_OK;
  if (cam_idx) { SFM_HIP(hipMemcpy(cam_idx, cam, sizeof(int) * m, hipMemcpyDeviceToHost)); s->download_bytes += 4ll * (int64_t)m; }
  if (key_idx) { SFM_HIP(hipMemcpy(key_idx, cam + cap1, sizeof(int) * m, hipMemcpyDeviceToHost)); s->download_bytes += 4ll * (int64_t)m; }
  if (uv) {
    SFM_HIP(hipMemcpy(uv, u, sizeof(double) * m, hipMemcpyDeviceToHost));
    SFM_HIP(hipMemcpy(uv + m, u + cap1, sizeof(double) * m, hipMemcpyDeviceToHost));
    s->download_bytes += 16ll * (int64_t)m;
  }
  return SFM_OK;
}

// The store form of the track linking (sfm_hip.h, block "track linking"): the matches of pair p are the entries q > 0 of
// table[ref][que, :], read where they lie; the result becomes the store's observation list.
int sfm_link_tracks_views(sfm_track_store* s, int P, const int* pairs, const unsigned char* key_mask, int min_len, int* d_key_track,
                         int64_t* summary) {
  const char* who = "sfm_link_tracks_views";
  SFM_TRY(ensure_init());
  if (!s) return SFM_E_HANDLE;
  const int V = (int)s->views.size();
  if (P < 0 || (P > 0 && !pairs)) { set_error("%s: %d pairs", who, P); return SFM_E_SHAPE; }
  std::vector<int> key_ptr((size_t)V + 1, 0);
  for (int v = 0; v < V; ++v) key_ptr[v + 1] = key_ptr[v] + s->views[v].n;
  std::vector<int64_t> pair_ptr((size_t)P + 1, 0);
  std::vector<const int*> rows((size_t)(P > 0 ? P : 1), nullptr);
  std::vector<const double*> nu((size_t)(V > 0 ? V : 1), nullptr), nv((size_t)(V > 0 ? V : 1), nullptr);
  for (int p = 0; p < P; ++p) {
    const int ref = pairs[2 * p], que = pairs[2 * p + 1];
    SFM_TRY(valid_view(s, ref, who));
    SFM_TRY(valid_view(s, que, who));
    const View& r = s->views[ref];
    if (r.rows <= que) { set_error("%s: table %d has no row %d", who, ref, que); return SFM_E_SHAPE; }
    for (int v : {ref, que})
      if (s->views[v].n > 0 && !s->views[v].norm) { set_error("%s: view %d has no normalised coordinates", who, v); return SFM_E_SHAPE; }
    pair_ptr[p + 1] = pair_ptr[p] + r.n;
    rows[p] = r.table + (size_t)que * r.n;
  }
  SFM_TRY(track_link_check(who, V, key_ptr.data(), P, pairs, pair_ptr.data(), min_len, 0, 0));
  for (int v = 0; v < V; ++v) { nu[v] = s->views[v].norm; nv[v] = s->views[v].norm ? s->views[v].norm + s->views[v].n : nullptr; }
  const size_t cap = (size_t)key_ptr[V], M = (size_t)pair_ptr[P];
  hipStream_t st = ctx().stream;
  SFM_TRY(settle(s));
  s->obs_views = -1;
  SFM_TRY(s->obs_ptr.reserve(sizeof(int) * (cap / 2 + 2)));
  SFM_TRY(s->obs_idx.reserve(sizeof(int) * 2 * (cap + 1)));
  SFM_TRY(s->obs_uv.reserve(sizeof(double) * 2 * (cap + 1)));
  DevBuf<unsigned char> d_mask;
  DevBuf<int64_t> d_summary;
  if (key_mask) { SFM_TRY(d_mask.upload(key_mask, M, st)); s->upload_bytes += (int64_t)M; }
  SFM_TRY(d_summary.alloc(8, st));
  int* cam = static_cast<int*>(s->obs_idx.p);
  double* u = static_cast<double*>(s->obs_uv.p);
  LinkProblem q;
  q.V = V; q.P = P; q.min_len = min_len; q.key_ptr = key_ptr.data(); q.pair_views = pairs; q.pair_ptr = pair_ptr.data();
  q.rows = rows.data(); q.d_mask = d_mask.p;
  q.d_key_track = d_key_track; q.d_pt_ptr = static_cast<int*>(s->obs_ptr.p); q.d_cam_idx = cam; q.d_key_idx = cam + cap + 1;
  q.d_summary = d_summary.p; q.view_nu = nu.data(); q.view_nv = nv.data(); q.d_u = u; q.d_v = u + cap + 1;
  int n_tracks = 0;
  int64_t n_obs = 0;
  SFM_TRY(track_link_run(who, q, &n_tracks, &n_obs, st));
  if (summary) { SFM_TRY(d_summary.download(summary, 8, st)); SFM_TRY(stream_sync(st)); }
  s->obs_views = V; s->obs_pts = n_tracks; s->obs_cap = (int)cap; s->obs_m = n_obs;
  return SFM_OK;
}

}  // extern "C"

namespace sfm {

int track_observations(sfm_track_store* s, const char* who, TrackObservations* out) {
  if (!s) { set_error("%s: the track store is NULL", who); return SFM_E_HANDLE; }
  if (s->obs_views < 0) { set_error("%s: the store has no observation list (sfm_obs_build)", who); return SFM_E_SHAPE; }
  SFM_TRY(settle(s));
  const int* cam = static_cast<const int*>(s->obs_idx.p);
  const double* u = static_cast<const double*>(s->obs_uv.p);
  *out = TrackObservations{s->obs_views, s->obs_pts, s->obs_m, static_cast<const int*>(s->obs_ptr.p), cam, u, u + (size_t)s->obs_cap + 1};
  return SFM_OK;
}

}  // namespace sfm
