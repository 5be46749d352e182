// sfm_track_link.hip — multi-view tracks from verified pairwise matches: connected components of the match graph over
// (view, key) nodes, judged and written as a (point, view)-sorted CSR (gfx950).
//
// The rule is stated in sfm_hip.h, block "track linking".  Everything is an integer; the stages of a call:
//   verify   the lowest match whose key index lies outside its view (atomicMin), read by the host before anything else runs
//   init     parent[g] = g, sizes and counters zero
//   union    the used matches dealt over a grid: a lock-free union-find that hooks the root with the LARGER id under the
//            root with the smaller one by atomicCAS (retry on failure), path halving on the way.  A root is never hooked
//            under a larger id, so parent[x] <= x throughout and the root of a component is its minimum.
//   flatten  label[g] = find(g), size[label] += 1 (integer atomicAdd, the lanes of a wave that share a root adding once)
//   scan A   over the roots in id order: the components of at least two keys are numbered, their member ranges laid out
//   fill     members scattered through a per-component cursor: arrival order, not yet deterministic (a component of
//            more than V keys is left out: it is a conflict by counting)
//   order    a group of 1-64 lanes per component of up to 64 members: the rank of every member among the ids of its
//            component, and the conflict test.  Members ascend by id, and ids ascend by view, so the successor of a member
//            is its neighbour: the component is in conflict iff some member's view range holds another member.  Components
//            beyond 64 members go to a list and get one workgroup each (members in LDS up to 1 024, read from memory
//            beyond).  A component of more than V keys is a conflict by counting and is not ordered.
//   scan B   over the components: the kept ones are numbered, pt_ptr is the scan of their sizes
//   gather   a lane per key: key_track, and for a member of a kept component its place pt_ptr[track] + rank
// No workgroup waits for another one anywhere in this file: every loop is a CAS retry or a walk towards a root, and both
// make progress on their own.  Every atomic is an integer one whose result does not depend on the order of arrival, and
// the one arrival-ordered array (members) is only ever read as a set.
#include <climits>
#include <vector>

#include "sfm_scan.h"
#include "sfm_track_link.h"

namespace sfm {

constexpr int kLkThreads = 256;
constexpr int kLkBigLds = 1024;            // members a workgroup of the big pass holds in LDS
constexpr int kLkScanCrossover = 1 << 14;  // auto: the device-wide scan from this many elements on (measured: DESIGN.md section 39)

// state words of a call on the device (64-bit each)
enum { kLsBad = 0, kLsUsed, kLsComps, kLsMembers, kLsBig, kLsConflict, kLsShort, kLsLongest, kLsLargest, kLsTracks, kLsObs, kLsWords };

typedef unsigned long long u64;

struct LkArgs {
  int V, P, K, min_len;
  long long M;
  const int* key_ptr;            // [V + 1]
  const long long* pair_ptr;     // [P + 1]
  const int4* pair_info;         // [P]: key_ptr of the first view, of the second, key count of the first, of the second
  const int* a;                  // [M] or null (rows)
  const int* b;
  const int* const* rows;        // [P] or null
  const unsigned char* mask;     // [M] or null
  u64* st;                       // [kLsWords]
  int* parent;                   // [K]
  int* label;                    // [K]
  int* size;                     // [K] on the roots
  int* cursor;                   // [K] on the roots of at least two keys
  int* root_comp;                // [K] on the same: the component number
  int* members;                  // [K] by component, arrival order inside
  int* rank;                     // [K] of a member among its component's ids
  int* comp_ptr;                 // [K / 2 + 1] first member
  int* comp_size;                // [K / 2 + 1]
  int* comp_kept;                // [K / 2 + 1] size if kept, else 0
  int* comp_track;               // [K / 2 + 1] track number, -2 short, -3 conflict
  int* comp_off;                 // [K / 2 + 1] pt_ptr of a kept component
  int* big;                      // [K / 65 + 1] components of more than 64 members
  int* key_track; int* pt_ptr; int* cam_idx; int* key_idx; long long* summary; int* label_out;
  const double* const* view_nu; const double* const* view_nv; double* u; double* v;
};

__device__ __forceinline__ int lk_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lk_store(int* p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the last p with ptr[p] <= m (ptr[0] <= m < ptr[n])
__device__ __forceinline__ int lk_pair_of(const long long* ptr, int n, long long m) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= m) lo = mid; else hi = mid;
  }
  return lo;
}

// the view of global key g: the last v with key_ptr[v] <= g (a view without keys is never the last one)
__device__ __forceinline__ int lk_view_of(const int* key_ptr, int V, int g) {
  int lo = 0, hi = V;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (key_ptr[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// match m as (pair, a, b, is a match at all)
__device__ __forceinline__ bool lk_match(const LkArgs& x, long long m, int* p_out, int* a_out, int* b_out) {
  const int p = lk_pair_of(x.pair_ptr, x.P, m);
  *p_out = p;
  if (x.rows) {
    const int r = (int)(m - x.pair_ptr[p]), q = x.rows[p][r];
    *a_out = r; *b_out = q;
    return q > 0;
  }
  *a_out = x.a[m]; *b_out = x.b[m];
  return true;
}

__global__ __launch_bounds__(kLkThreads) void link_verify_kernel(LkArgs x) {
  const long long step = (long long)gridDim.x * kLkThreads;
  for (long long m = (long long)blockIdx.x * kLkThreads + threadIdx.x; m < x.M; m += step) {
    int p, a, b;
    if (!lk_match(x, m, &p, &a, &b)) continue;
    const int4 info = x.pair_info[p];
    if (a < 0 || a >= info.z || b < 0 || b >= info.w) atomicMin(&x.st[kLsBad], (u64)m);
  }
}

__global__ __launch_bounds__(kLkThreads) void link_init_kernel(LkArgs x) {
  const int g = blockIdx.x * kLkThreads + threadIdx.x;
  if (g < x.K) { x.parent[g] = g; x.size[g] = 0; }
}

// Walk to the root, halving the path: parent[x] = parent[parent[x]] names an ancestor whatever other lanes do meanwhile
// (links are only ever added at roots, and a key that has a parent never becomes a root again).
__device__ __forceinline__ int lk_find(int* parent, int x) {
  for (;;) {
    const int p = lk_load(parent + x);
    if (p == x) return x;
    const int gp = lk_load(parent + p);
    if (gp == p) return p;
    lk_store(parent + x, gp);
    x = gp;
  }
}

__global__ __launch_bounds__(kLkThreads) void link_union_kernel(LkArgs x) {
  __shared__ int lds_used;
  if (threadIdx.x == 0) lds_used = 0;
  __syncthreads();
  int used = 0;
  const long long step = (long long)gridDim.x * kLkThreads;
  for (long long m = (long long)blockIdx.x * kLkThreads + threadIdx.x; m < x.M; m += step) {
    int p, a, b;
    if (!lk_match(x, m, &p, &a, &b)) continue;
    if (x.mask && x.mask[m] == 0) continue;
    ++used;
    const int4 info = x.pair_info[p];
    int ga = info.x + a, gb = info.y + b;
    for (;;) {                                   // a failed CAS means another lane hooked that root: progress either way
      ga = lk_find(x.parent, ga);
      gb = lk_find(x.parent, gb);
      if (ga == gb) break;
      const int hi = ga > gb ? ga : gb, lo = ga > gb ? gb : ga;
      if (atomicCAS(x.parent + hi, hi, lo) == hi) break;
      ga = hi; gb = lo;
    }
  }
  used = group_sum<64>(used);
  if ((threadIdx.x & 63) == 0 && used) atomicAdd(&lds_used, used);
  __syncthreads();
  if (threadIdx.x == 0 && lds_used) atomicAdd(&x.st[kLsUsed], (u64)lds_used);
}

__global__ __launch_bounds__(kLkThreads) void link_flatten_kernel(LkArgs x) {
  const int g = blockIdx.x * kLkThreads + threadIdx.x;
  if (g >= x.K) return;
  const int r = lk_find(x.parent, g);
  x.label[g] = r;
  // One component can hold most of the keys (a few per cent of false matches join everything), and that many atomics on one
  // word queue up at a single L2 channel (11 ns each, measured: DESIGN.md section 39).  The lanes of a wave that name the
  // root of the wave's first lane therefore add once, together; then the same among the lanes that are left (the first lane
  // need not be of the large component); whoever is left after that adds for itself.
  bool done = false;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (done) continue;
    const int first = __builtin_amdgcn_readfirstlane(r);
    const unsigned long long same = __ballot(r == first);
    if (r != first) continue;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(x.size + r, __popcll(same));
    done = true;
  }
  if (!done) atomicAdd(x.size + r, 1);
}

// scan A: the roots of at least two keys, in id order
struct LkScanRoots {
  LkArgs x;
  __device__ int n() const { return x.K; }
  __device__ void load(int g, int (&a)[2]) const {
    const bool root = x.label[g] == g && x.size[g] >= 2;
    a[0] = root ? 1 : 0; a[1] = root ? x.size[g] : 0;
  }
  __device__ void store(int g, const int (&e)[2]) const {
    if (!(x.label[g] == g && x.size[g] >= 2)) return;
    x.root_comp[g] = e[0]; x.cursor[g] = e[1];
    x.comp_ptr[e[0]] = e[1]; x.comp_size[e[0]] = x.size[g];
  }
  __device__ void total(const int (&t)[2]) const { x.st[kLsComps] = (u64)t[0]; x.st[kLsMembers] = (u64)t[1]; }
};

__global__ __launch_bounds__(kLkThreads) void link_fill_kernel(LkArgs x) {
  const int g = blockIdx.x * kLkThreads + threadIdx.x;
  if (g >= x.K) return;
  const int r = x.label[g], s = x.size[r];
  if (s < 2 || s > x.V) return;                // beyond V keys: a conflict by counting, which nothing orders or reads
  x.members[atomicAdd(x.cursor + r, 1)] = g;
}

// The verdict on a component, by one lane: what scan B reads, and the lane's share of the counters.
__device__ __forceinline__ void lk_judge(const LkArgs& x, int c, int s, bool conflict, int* n_conf, int* n_short, int* longest) {
  const bool is_short = !conflict && s < x.min_len, kept = !conflict && !is_short;
  x.comp_kept[c] = kept ? s : 0;
  x.comp_track[c] = conflict ? -3 : (is_short ? -2 : 0);
  *n_conf += conflict; *n_short += is_short;
  if (kept && s > *longest) *longest = s;
}

// The rank of member `me` among the s ids at mem[0 .. s), and whether its view's id range [lo, hi) holds another of them.
__device__ __forceinline__ int lk_rank(const int* mem, int s, int me, int lo, int hi, bool* conflict) {
  int r = 0;
  bool c = false;
  for (int j = 0; j < s; ++j) {
    const int y = mem[j];
    r += y < me;
    c |= y != me && y >= lo && y < hi;
  }
  *conflict |= c;
  return r;
}

template <int G>
__global__ __launch_bounds__(kLkThreads) void link_order_kernel(LkArgs x) {
  constexpr int kPerBlock = kLkThreads / G;
  const int n_comp = (int)x.st[kLsComps], gl = threadIdx.x % G;
  int n_conf = 0, n_short = 0, longest = 0, largest = 0;
  for (long long base = (long long)blockIdx.x * kPerBlock; base < n_comp; base += (long long)gridDim.x * kPerBlock) {      // block-uniform trip count
    const long long c = base + threadIdx.x / G;
    const int s = c < n_comp ? x.comp_size[c] : 0;
    if (s == 0) continue;
    if (gl == 0 && s > largest) largest = s;
    if (s > 64) {
      if (gl == 0) x.big[atomicAdd(&x.st[kLsBig], 1ull)] = (int)c;
      continue;
    }
    bool conflict = s > x.V;
    if (!conflict) {
      const int* mem = x.members + x.comp_ptr[c];
      for (int i = gl; i < s; i += G) {
        const int me = mem[i], v = lk_view_of(x.key_ptr, x.V, me);
        x.rank[me] = lk_rank(mem, s, me, x.key_ptr[v], x.key_ptr[v + 1], &conflict);
      }
      conflict = group_sum<G>(conflict ? 1 : 0) > 0;
    }
    if (gl == 0) lk_judge(x, (int)c, s, conflict, &n_conf, &n_short, &longest);
  }
  // one atomic per wave and counter
  n_conf = group_sum<64>(n_conf); n_short = group_sum<64>(n_short);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { longest = max(longest, __shfl_xor(longest, off, 64)); largest = max(largest, __shfl_xor(largest, off, 64)); }
  if ((threadIdx.x & 63) != 0) return;
  if (n_conf) atomicAdd(&x.st[kLsConflict], (u64)n_conf);
  if (n_short) atomicAdd(&x.st[kLsShort], (u64)n_short);
  if (longest) atomicMax(&x.st[kLsLongest], (u64)longest);
  if (largest) atomicMax(&x.st[kLsLargest], (u64)largest);
}

// one workgroup per component of more than 64 members
__global__ __launch_bounds__(kLkThreads) void link_order_big_kernel(LkArgs x) {
  __shared__ int lds_mem[kLkBigLds];
  const int n_big = (int)x.st[kLsBig], tid = threadIdx.x;
  for (int k = blockIdx.x; k < n_big; k += gridDim.x) {
    const int c = x.big[k], s = x.comp_size[c];
    bool conflict = s > x.V;
    if (!conflict) {
      const int* mem = x.members + x.comp_ptr[c];
      const bool in_lds = s <= kLkBigLds;
      __syncthreads();                           // the previous component's members have been read
      if (in_lds) {
        for (int i = tid; i < s; i += kLkThreads) lds_mem[i] = mem[i];
        __syncthreads();
      }
      for (int i = tid; i < s; i += kLkThreads) {
        const int me = mem[i], v = lk_view_of(x.key_ptr, x.V, me);
        const int lo = x.key_ptr[v], hi = x.key_ptr[v + 1];
        x.rank[me] = in_lds ? lk_rank(lds_mem, s, me, lo, hi, &conflict) : lk_rank(mem, s, me, lo, hi, &conflict);
      }
      conflict = __syncthreads_or(conflict ? 1 : 0) != 0;
    }
    if (tid == 0) {
      int n_conf = 0, n_short = 0, longest = 0;
      lk_judge(x, c, s, conflict, &n_conf, &n_short, &longest);
      if (n_conf) atomicAdd(&x.st[kLsConflict], 1ull);
      if (n_short) atomicAdd(&x.st[kLsShort], 1ull);
      if (longest) atomicMax(&x.st[kLsLongest], (u64)longest);
    }
  }
}

// scan B: the kept components, in label order
struct LkScanKept {
  LkArgs x;
  __device__ int n() const { return (int)x.st[kLsComps]; }
  __device__ void load(int c, int (&a)[2]) const {
    const int s = x.comp_kept[c];
    a[0] = s > 0 ? 1 : 0; a[1] = s;
  }
  __device__ void store(int c, const int (&e)[2]) const {
    if (x.comp_kept[c] <= 0) return;
    x.comp_track[c] = e[0]; x.comp_off[c] = e[1];
    if (x.pt_ptr) x.pt_ptr[e[0]] = e[1];
  }
  __device__ void total(const int (&t)[2]) const {
    x.st[kLsTracks] = (u64)t[0]; x.st[kLsObs] = (u64)t[1];
    if (x.pt_ptr) x.pt_ptr[t[0]] = t[1];
    if (x.summary) {
      x.summary[0] = (long long)x.st[kLsUsed]; x.summary[1] = (long long)x.st[kLsComps]; x.summary[2] = t[0];
      x.summary[3] = (long long)x.st[kLsConflict]; x.summary[4] = (long long)x.st[kLsShort]; x.summary[5] = t[1];
      x.summary[6] = (long long)x.st[kLsLongest]; x.summary[7] = (long long)x.st[kLsLargest];
    }
  }
};

__global__ __launch_bounds__(kLkThreads) void link_gather_kernel(LkArgs x) {
  const int g = blockIdx.x * kLkThreads + threadIdx.x;
  if (g >= x.K) return;
  const int r = x.label[g];
  if (x.label_out) x.label_out[g] = r;
  int track = -1;
  if (x.size[r] >= 2) {
    const int c = x.root_comp[r];
    track = x.comp_track[c];
    if (track >= 0 && (x.cam_idx || x.key_idx || x.u)) {
      const int o = x.comp_off[c] + x.rank[g], v = lk_view_of(x.key_ptr, x.V, g), k = g - x.key_ptr[v];
      if (x.cam_idx) x.cam_idx[o] = v;
      if (x.key_idx) x.key_idx[o] = k;
      if (x.u) { x.u[o] = x.view_nu[v][k]; x.v[o] = x.view_nv[v][k]; }
    }
  }
  if (x.key_track) x.key_track[g] = track;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct LkPlan { int union_grid, group, order_grid, big_grid, scan_keys, tiles_keys, scan_comps, tiles_comps; };

static LkPlan lk_plan(int V, long long K, long long M, int group, int scan) {
  LkPlan p;
  const int cus = plan_cus();
  const long long want = (M + kLkThreads - 1) / kLkThreads, cap = 16LL * cus;
  p.union_grid = (int)(want < 1 ? 1 : (want < cap ? want : cap));
  const long long comps = K / 2;
  if (group == 0) {
    const int typical = V < 8 ? V : 8;           // tracks of a handful of views are the common case
    const int i = narrowest_group([&](int g) { return g >= typical; });
    group = kGroupWidths[widen_for_waves(i, (int)(comps > INT_MAX ? INT_MAX : comps), 64)];
  }
  p.group = group;
  const long long blocks = (comps * group + kLkThreads - 1) / kLkThreads, ocap = 32LL * cus;
  p.order_grid = (int)(blocks < 1 ? 1 : (blocks < ocap ? blocks : ocap));
  const long long nbig = K / 65;
  p.big_grid = (int)(nbig < 1 ? 1 : (nbig < 4LL * cus ? nbig : 4LL * cus));
  auto route = [&](long long n, int* r, int* tiles) {
    *tiles = (int)((n + kScanBlock - 1) / kScanBlock);
    if (*tiles < 1) *tiles = 1;
    *r = scan == 0 ? (n >= kLkScanCrossover ? 2 : 1) : scan;
    if (*tiles <= 1) *r = 1;
  };
  route(K, &p.scan_keys, &p.tiles_keys);
  route(comps, &p.scan_comps, &p.tiles_comps);
  return p;
}

int track_link_check(const char* who, int V, const int* key_ptr, int P, const int* pair_views, const int64_t* pair_ptr, int min_len,
                     int group, int scan) {
  if (V < 0 || P < 0) { set_error("%s: bad sizes V=%d P=%d", who, V, P); return SFM_E_SHAPE; }
  if (key_ptr == nullptr || pair_ptr == nullptr || (P > 0 && pair_views == nullptr)) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  if (min_len < 2) { set_error("%s: min_len = %d must be >= 2", who, min_len); return SFM_E_SHAPE; }
  SFM_TRY(group_width_check(who, group));
  if (scan < 0 || scan > 2) { set_error("%s: scan = %d must be 0 (automatic), 1 (one workgroup) or 2 (device-wide)", who, scan); return SFM_E_SHAPE; }
  if (key_ptr[0] != 0) { set_error("%s: key_ptr[0] = %d must be 0", who, key_ptr[0]); return SFM_E_SHAPE; }
  for (int v = 0; v < V; ++v)
    if (key_ptr[v + 1] < key_ptr[v]) { set_error("%s: key_ptr decreases at view %d", who, v); return SFM_E_SHAPE; }
  if (pair_ptr[0] != 0) { set_error("%s: pair_ptr[0] = %lld must be 0", who, (long long)pair_ptr[0]); return SFM_E_SHAPE; }
  for (int p = 0; p < P; ++p) {
    const int i = pair_views[2 * p], j = pair_views[2 * p + 1];
    if (i < 0 || i >= V || j < 0 || j >= V || i == j) { set_error("%s: pair %d = (%d, %d) must join two different views in 0 .. %d", who, p, i, j, V - 1); return SFM_E_SHAPE; }
    if (pair_ptr[p + 1] < pair_ptr[p]) { set_error("%s: pair_ptr decreases at pair %d", who, p); return SFM_E_SHAPE; }
  }
  return SFM_OK;
}

int track_link_run(const char* who, const LinkProblem& q, int* n_tracks, int64_t* n_obs, hipStream_t s) {
  const int V = q.V, P = q.P, K = q.key_ptr[V];
  const long long M = q.pair_ptr[P];
  const LkPlan plan = lk_plan(V, K, M, q.group, q.scan);
  const size_t comps = (size_t)K / 2 + 1;
  // the checked host arrays, as the kernels read them
  std::vector<long long> h_ptr((size_t)P + 1);
  std::vector<int4> h_info((size_t)(P > 0 ? P : 1));
  for (int p = 0; p <= P; ++p) h_ptr[p] = q.pair_ptr[p];
  for (int p = 0; p < P; ++p) {
    const int i = q.pair_views[2 * p], j = q.pair_views[2 * p + 1];
    h_info[p] = make_int4(q.key_ptr[i], q.key_ptr[j], q.key_ptr[i + 1] - q.key_ptr[i], q.key_ptr[j + 1] - q.key_ptr[j]);
  }
  DevBuf<int> d_key_ptr, parent, label, size, cursor, root_comp, members, rank, comp_ptr, comp_size, comp_kept, comp_track, comp_off, big, tiles;
  DevBuf<long long> d_pair_ptr;
  DevBuf<int4> d_info;
  DevBuf<const int*> d_rows;
  DevBuf<const double*> d_nu, d_nv;
  DevBuf<u64> st;
  SFM_TRY(d_key_ptr.upload(q.key_ptr, (size_t)V + 1, s));
  SFM_TRY(d_pair_ptr.upload(h_ptr.data(), (size_t)P + 1, s));
  SFM_TRY(d_info.upload(h_info.data(), (size_t)P, s));
  if (q.rows) SFM_TRY(d_rows.upload(q.rows, (size_t)P, s));
  if (q.d_u) { SFM_TRY(d_nu.upload(q.view_nu, (size_t)V, s)); SFM_TRY(d_nv.upload(q.view_nv, (size_t)V, s)); }
  SFM_TRY(st.alloc(kLsWords, s));
  u64 st0[kLsWords] = {};
  st0[kLsBad] = ULLONG_MAX;
  SFM_HIP(hipMemcpyAsync(st.p, st0, sizeof(st0), hipMemcpyHostToDevice, s));
  LkArgs x = {};
  x.V = V; x.P = P; x.K = K; x.min_len = q.min_len; x.M = M;
  x.key_ptr = d_key_ptr.p; x.pair_ptr = d_pair_ptr.p; x.pair_info = d_info.p;
  x.a = q.d_a; x.b = q.d_b; x.rows = q.rows ? d_rows.p : nullptr; x.mask = q.d_mask; x.st = st.p;
  if (M > 0) {
    link_verify_kernel<<<(unsigned)plan.union_grid, kLkThreads, 0, s>>>(x);
    u64 bad = 0;
    SFM_HIP(hipMemcpyAsync(&bad, st.p + kLsBad, sizeof(bad), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    if (bad != ULLONG_MAX) {
      set_error("%s: match %lld names a key outside its view", who, (long long)bad);
      return SFM_E_SHAPE;
    }
  }
  const size_t k = (size_t)K;
  SFM_TRY(parent.alloc(k, s)); SFM_TRY(label.alloc(k, s)); SFM_TRY(size.alloc(k, s)); SFM_TRY(cursor.alloc(k, s));
  SFM_TRY(root_comp.alloc(k, s)); SFM_TRY(members.alloc(k, s)); SFM_TRY(rank.alloc(k, s));
  SFM_TRY(comp_ptr.alloc(comps, s)); SFM_TRY(comp_size.alloc(comps, s)); SFM_TRY(comp_kept.alloc(comps, s));
  SFM_TRY(comp_track.alloc(comps, s)); SFM_TRY(comp_off.alloc(comps, s)); SFM_TRY(big.alloc(k / 65 + 1, s));
  SFM_TRY(tiles.alloc(3 * (size_t)plan.tiles_keys + 3, s));
  x.parent = parent.p; x.label = label.p; x.size = size.p; x.cursor = cursor.p; x.root_comp = root_comp.p; x.members = members.p;
  x.rank = rank.p; x.comp_ptr = comp_ptr.p; x.comp_size = comp_size.p; x.comp_kept = comp_kept.p; x.comp_track = comp_track.p;
  x.comp_off = comp_off.p; x.big = big.p;
  x.key_track = q.d_key_track; x.pt_ptr = q.d_pt_ptr; x.cam_idx = q.d_cam_idx; x.key_idx = q.d_key_idx;
  x.summary = reinterpret_cast<long long*>(q.d_summary); x.label_out = q.d_label;
  x.view_nu = d_nu.p; x.view_nv = d_nv.p; x.u = q.d_u; x.v = q.d_v;
  const unsigned key_grid = (unsigned)((k + kLkThreads - 1) / kLkThreads);
  if (K > 0) {
    link_init_kernel<<<key_grid, kLkThreads, 0, s>>>(x);
    if (M > 0) link_union_kernel<<<(unsigned)plan.union_grid, kLkThreads, 0, s>>>(x);
    link_flatten_kernel<<<key_grid, kLkThreads, 0, s>>>(x);
  }
  exclusive_scan_launch<2>(LkScanRoots{x}, plan.scan_keys == 1, tiles.p, plan.tiles_keys, s);
  if (K > 0) {
    link_fill_kernel<<<key_grid, kLkThreads, 0, s>>>(x);
    dispatch_group<1>(plan.group, [&](auto g) { link_order_kernel<decltype(g)::value><<<(unsigned)plan.order_grid, kLkThreads, 0, s>>>(x); });
    link_order_big_kernel<<<(unsigned)plan.big_grid, kLkThreads, 0, s>>>(x);
  }
  exclusive_scan_launch<2>(LkScanKept{x}, plan.scan_comps == 1, tiles.p, plan.tiles_comps, s);
  if (K > 0) link_gather_kernel<<<key_grid, kLkThreads, 0, s>>>(x);
  SFM_HIP(hipGetLastError());
  u64 counts[2] = {0, 0};
  SFM_HIP(hipMemcpyAsync(counts, st.p + kLsTracks, sizeof(counts), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  if (n_tracks) *n_tracks = (int)counts[0];
  if (n_obs) *n_obs = (int64_t)counts[1];
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_link_tracks_plan(int V, int64_t K, int64_t M, int group, int scan, int* plan) {
  const char* who = "sfm_link_tracks_plan";
  if (plan == nullptr) { set_error("%s: plan is NULL", who); return SFM_E_SHAPE; }
  if (V < 0 || K < 0 || K > INT_MAX || M < 0) { set_error("%s: bad sizes V=%d K=%lld M=%lld", who, V, (long long)K, (long long)M); return SFM_E_SHAPE; }
  SFM_TRY(group_width_check(who, group));
  if (scan < 0 || scan > 2) { set_error("%s: scan = %d must be 0, 1 or 2", who, scan); return SFM_E_SHAPE; }
  const LkPlan p = lk_plan(V, K, M, group, scan);
  plan[0] = p.union_grid; plan[1] = p.group; plan[2] = p.order_grid; plan[3] = p.big_grid;
  plan[4] = p.scan_keys; plan[5] = p.tiles_keys; plan[6] = p.scan_comps; plan[7] = p.tiles_comps;
  return SFM_OK;
}

int sfm_link_tracks_dev(int V, const int* key_ptr, int P, const int* pair_views, const int64_t* pair_ptr, const int* d_a, const int* d_b,
                       const unsigned char* d_mask, int min_len, int group, int scan, int* d_key_track, int* d_pt_ptr, int* d_cam_idx,
                       int* d_key_idx, int64_t* d_summary, int* d_label_out, int* n_tracks, int64_t* n_obs, void* hip_stream) {
  const char* who = "sfm_link_tracks_dev";
  SFM_TRY(track_link_check(who, V, key_ptr, P, pair_views, pair_ptr, min_len, group, scan));
  if (pair_ptr[P] > 0 && (d_a == nullptr || d_b == nullptr)) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  LinkProblem q;
  q.V = V; q.P = P; q.min_len = min_len; q.group = group; q.scan = scan; q.key_ptr = key_ptr; q.pair_views = pair_views; q.pair_ptr = pair_ptr;
  q.d_a = d_a; q.d_b = d_b; q.d_mask = d_mask;
  q.d_key_track = d_key_track; q.d_pt_ptr = d_pt_ptr; q.d_cam_idx = d_cam_idx; q.d_key_idx = d_key_idx; q.d_summary = d_summary; q.d_label = d_label_out;
  return track_link_run(who, q, n_tracks, n_obs, s);
}

int sfm_link_tracks(int V, const int* key_ptr, int P, const int* pair_views, const int64_t* pair_ptr, const int* a, const int* b,
                   const unsigned char* mask, int min_len, int group, int scan, int* key_track, int* pt_ptr, int* cam_idx, int* key_idx,
                   int64_t* summary, int* label_out) {
  const char* who = "sfm_link_tracks";
  SFM_TRY(track_link_check(who, V, key_ptr, P, pair_views, pair_ptr, min_len, group, scan));
  const long long M = pair_ptr[P];
  if (M > 0 && (a == nullptr || b == nullptr)) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  for (int p = 0; p < P; ++p) {
    const int i = pair_views[2 * p], j = pair_views[2 * p + 1], na = key_ptr[i + 1] - key_ptr[i], nb = key_ptr[j + 1] - key_ptr[j];
    for (long long m = pair_ptr[p]; m < pair_ptr[p + 1]; ++m)
      if (a[m] < 0 || a[m] >= na || b[m] < 0 || b[m] >= nb) { set_error("%s: match %lld names a key outside its view", who, m); return SFM_E_SHAPE; }
  }
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t K = (size_t)key_ptr[V];
  DevBuf<int> dA, dB;
  DevBuf<unsigned char> dMask;
  HostOut<int> oTrack, oPtr, oCam, oKey, oLabel;
  HostOut<int64_t> oSum;
  SFM_TRY(dA.upload(a, (size_t)M, s)); SFM_TRY(dB.upload(b, (size_t)M, s)); SFM_TRY(dMask.upload_if(mask, (size_t)M, s));
  SFM_TRY(oTrack.want(key_track, K, s)); SFM_TRY(oPtr.want(pt_ptr, K / 2 + 2, s)); SFM_TRY(oCam.want(cam_idx, K, s));
  SFM_TRY(oKey.want(key_idx, K, s)); SFM_TRY(oLabel.want(label_out, K, s)); SFM_TRY(oSum.want(summary, 8, s));
  LinkProblem q;
  q.V = V; q.P = P; q.min_len = min_len; q.group = group; q.scan = scan; q.key_ptr = key_ptr; q.pair_views = pair_views; q.pair_ptr = pair_ptr;
  q.d_a = dA.p; q.d_b = dB.p; q.d_mask = dMask.p;
  q.d_key_track = oTrack.dev(); q.d_pt_ptr = oPtr.dev(); q.d_cam_idx = oCam.dev(); q.d_key_idx = oKey.dev(); q.d_summary = oSum.dev(); q.d_label = oLabel.dev();
  int n_tracks = 0;
  int64_t n_obs = 0;
  SFM_TRY(track_link_run(who, q, &n_tracks, &n_obs, s));
  // only what the rule defines comes down: pt_ptr[0 .. n_tracks], the first n_obs entries of cam_idx and key_idx
  if (pt_ptr) SFM_HIP(hipMemcpyAsync(pt_ptr, oPtr.dev(), sizeof(int) * ((size_t)n_tracks + 1), hipMemcpyDeviceToHost, s));
  if (cam_idx && n_obs) SFM_HIP(hipMemcpyAsync(cam_idx, oCam.dev(), sizeof(int) * (size_t)n_obs, hipMemcpyDeviceToHost, s));
  if (key_idx && n_obs) SFM_HIP(hipMemcpyAsync(key_idx, oKey.dev(), sizeof(int) * (size_t)n_obs, hipMemcpyDeviceToHost, s));
  SFM_TRY(oTrack.fetch(s)); SFM_TRY(oLabel.fetch(s)); SFM_TRY(oSum.fetch(s));
  return stream_sync(s);
}

}  // extern "C"
