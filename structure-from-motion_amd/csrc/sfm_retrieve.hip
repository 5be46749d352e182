// sfm_retrieve.hip — view pairs: which pairs of views to match, from one short descriptor per view (gfx950).
//
// The rule is stated in sfm_hip.h, block "view pairs".  Three operations share this file:
//   vocabulary   sfm_vocab_train: K words from the resident exact L2 sets by `iters` rounds of integer k-means
//   describe     sfm_view_describe: one VLAD descriptor per view (int8, power-normalised by an integer square root)
//   pairs        sfm_view_pairs: the V x V scores, the k best partners of every view, the sorted list of pairs
// and these stages:
//   assign       hot path 1 (training and describing): a tile of 128 rows against all K words, v_mfma_f32_16x16x32_bf16 on
//                the sets' resident bf16 rows and integer norms, exactly the arithmetic of the matcher's exact path; a lane
//                keeps ONE running best per row as the key (s << 32 | w), s itself (no sqrt canonicalisation: the order is
//                (s, w), not (float distance, index)); the 16 lanes of a row fold at the end
//   accumulate   int32 sums of x per (group, word, dimension) and the word counts; a group is a view (describing) or the
//                whole training set.  Per workgroup in LDS where (K D + K) * 4 bytes fit in 64 KiB, by global int32
//                atomics otherwise.  Integer addition is associative: neither the route nor the arrival order shows
//   update       c = floor((2 S + n) / (2 n)) per word (training)       quantise   r = S - n c, q, norm2 per view (describing)
//   dot          hot path 2: V x V dot products of the int8 descriptors by v_mfma_i32_16x16x64_i8, a wave per 32 x 32 tile,
//                in strips of rows into a bounded work buffer (or into `dot` where the caller asks for it)
//   select       a wave per view: k rounds of "the least (score key, index) above the last one taken"
//   pairs        the reverse neighbour lists by the key-major list; per view a count of its listed partners b > a, the
//                shared prefix sum, a fill in order; a wave per listed pair recomputes its dot product for pair_score
// No floating-point value is summed or used in an atomic anywhere; the only floating-point results are scores, each a
// function of three integers.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "sfm_common.h"
#include "sfm_desc.h"
#include "sfm_hyp_number.h"
#include "sfm_scan.h"

#pragma clang fp contract(off)

namespace sfm {

constexpr int kRetrMaxWords = 1024, kRetrMaxLen = 131072, kRetrMaxDim = 256, kRetrMaxViews = 65536, kRetrMaxK = 64, kRetrMaxIters = 64;
constexpr long long kRetrMaxViewKeys = 1LL << 22, kRetrCapDefault = 1LL << 20, kRetrCapMax = 1LL << 22;
constexpr int kRetrTileRows = 128;              // rows of an assignment workgroup: 4 waves x 2 strips x 16
constexpr int kRetrChunkRows = 1024;            // rows of an accumulation workgroup
constexpr int kRetrLdsBytes = 64 * 1024;        // the LDS route of the accumulation up to here
constexpr long long kRetrStripInts = 1LL << 26; // the work buffer of the dot products (256 MiB)
constexpr long long kRetrSumInts = 1LL << 26;   // the sums of one batch of views (256 MiB)

typedef unsigned long long u64;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;

// The score of a pair: a product, a square root and a division, each correctly rounded (contraction is off in this file and
// there is nothing to contract).  The same function on the host (sfm_view_score) and in the kernels.
__host__ __device__ inline double view_score(int dot, long long na, long long nb) {
  const double p = (double)na * (double)nb;
  return (double)dot / sqrt(p);
}

// A double's bits in an unsigned order, and back.
__host__ __device__ inline u64 f64_order(double v) {
  u64 u;
  memcpy(&u, &v, 8);
  return (u >> 63) ? ~u : (u | (1ULL << 63));
}
__host__ __device__ inline double f64_unorder(u64 o) {
  const u64 u = (o >> 63) ? (o & ~(1ULL << 63)) : ~o;
  double v;
  memcpy(&v, &u, 8);
  return v;
}

// floor(t N / T) for t < T <= N, split as ransac_pair_number splits its product
__host__ __device__ inline long long retr_spread(long long t, long long N, long long T) { return T == N ? t : t * (N / T) + t * (N % T) / T; }

// The rows of a job: the concatenation of n_sets exact sets, all N rows (T == N) or T of them, evenly spaced.
struct RowSrc {
  const long long* off;             // [n_sets + 1] first row of every set in the concatenation
  const uint16_t* const* bf;        // [n_sets]
  const int* const* norm;           // [n_sets]
  int n_sets, dp;
  long long N, T;
};

// job row t -> (set, row inside it): the first set whose end lies past the row (empty sets are stepped over)
__device__ __forceinline__ void retr_locate(const RowSrc& R, long long t, int* set, int* loc) {
  const long long g = retr_spread(t, R.N, R.T);
  int lo = 0, hi = R.n_sets - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (R.off[mid + 1] <= g) lo = mid + 1; else hi = mid;
  }
  *set = lo;
  *loc = (int)(g - R.off[lo]);
}

__device__ __forceinline__ int bf16_int(uint16_t v) { return (int)__uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint16_t int_bf16(int v) { return (uint16_t)(__float_as_uint((float)v) >> 16); }      // exact below 2^8

__device__ __forceinline__ u64 retr_shfl_xor_u64(u64 v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}

// ---------------------------------------------------------------------------------------------
// assign: hot path 1
// ---------------------------------------------------------------------------------------------
// Operand and result maps as in match_l2_mfma_kernel: A lane l = row (l & 15), k = 8 (l >> 4) .. + 7 of each 32-wide step;
// B the same of a word; C[row 4 h + r][col l & 15].  Rows past T are zero rows and store nothing; words past K (the image
// of the words is padded to a multiple of 128 rows) are not selected.
template <int KS>
__global__ __launch_bounds__(256) void retr_assign_kernel(RowSrc R, const uint16_t* __restrict__ voc_bf, const int* __restrict__ voc_norm,
                                                          int K, int* __restrict__ assign, uint32_t* __restrict__ dist) {
  constexpr int DP = KS * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, h = lane >> 4;
  const long long t0 = (long long)blockIdx.x * kRetrTileRows + wave * 32;
  bf16x8 a[2][KS];
  int own_norm[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long t = t0 + 16 * s + r16;
    own_norm[s] = 0;
    if (t < R.T) {
      int set, loc;
      retr_locate(R, t, &set, &loc);
      const uint16_t* row = R.bf[set] + (size_t)loc * DP;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a[s][ks] = *reinterpret_cast<const bf16x8*>(row + ks * 32 + 8 * h);
      own_norm[s] = R.norm[set][loc];
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a[s][ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  int qn[2][4];
  u64 best[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      qn[s][r] = __shfl(own_norm[s], 4 * h + r, 64);      // the norm of row 4 h + r sits with the lanes that loaded it
      best[s][r] = ~0ULL;
    }
  for (int w0 = 0; w0 < K; w0 += 16) {
    const int col = w0 + r16;
    const bool valid = col < K;
    bf16x8 b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const bf16x8*>(voc_bf + (size_t)col * DP + ks * 32 + 8 * h);
    const int tn = valid ? voc_norm[col] : 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s][ks], b[ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t sv = (uint32_t)(qn[s][r] + tn - 2 * (int)acc[r]);
        const u64 key = ((u64)sv << 32) | (uint32_t)col;
        if (valid && key < best[s][r]) best[s][r] = key;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u64 k = best[s][r];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        const u64 o = retr_shfl_xor_u64(k, m);
        k = o < k ? o : k;
      }
      const long long t = t0 + 16 * s + 4 * h + r;
      if (r16 == 0 && t < R.T) {
        assign[t] = (int)(uint32_t)k;
        dist[t] = (uint32_t)(k >> 32);
      }
    }
}

// ---------------------------------------------------------------------------------------------
// accumulate: S[group][w][d] += x[d], cnt[group][w] += 1 over the rows of a chunk (one group per chunk); inertia += s
// ---------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(256) void retr_accum_kernel(RowSrc R, const int4* __restrict__ chunks, const int* __restrict__ assign,
                                                         const uint32_t* __restrict__ dist, int K, int D, int* __restrict__ S,
                                                         int* __restrict__ cnt, u64* __restrict__ inertia) {
  extern __shared__ int retr_lds[];                       // LDS route: [K D] sums, [K] counts
  const int4 ch = chunks[blockIdx.x];                     // {group inside the batch, first row, end row, -}
  const int d = threadIdx.x, KD = K * D;                  // a thread per padded dimension, one row at a time
  int* sums = LDS ? retr_lds : S + (size_t)ch.x * KD;
  int* counts = LDS ? retr_lds + KD : cnt + (size_t)ch.x * K;
  if (LDS) {
    for (int i = threadIdx.x; i < KD + K; i += blockDim.x) retr_lds[i] = 0;
    __syncthreads();
  }
  u64 inert = 0;
  for (int t = ch.y; t < ch.z; ++t) {
    const int w = assign[t];
    int set, loc;
    retr_locate(R, t, &set, &loc);
    if (d < D) {
      const int x = bf16_int(R.bf[set][(size_t)loc * R.dp + d]);
      if (x != 0) atomicAdd(&sums[w * D + d], x);
    }
    if (d == 0) {
      atomicAdd(&counts[w], 1);
      inert += dist[t];
    }
  }
  if (LDS) {
    __syncthreads();
    int* gs = S + (size_t)ch.x * KD;
    int* gc = cnt + (size_t)ch.x * K;
    for (int i = threadIdx.x; i < KD; i += blockDim.x)
      if (retr_lds[i] != 0) atomicAdd(&gs[i], retr_lds[i]);
    for (int i = threadIdx.x; i < K; i += blockDim.x)
      if (retr_lds[KD + i] != 0) atomicAdd(&gc[i], retr_lds[KD + i]);
  }
  if (d == 0 && inertia != nullptr && inert != 0) atomicAdd(inertia, inert);
}

// ---------------------------------------------------------------------------------------------
// training: the start words, and the update of a round
// ---------------------------------------------------------------------------------------------
// word w = row rows[w] of the concatenation: a copy of its bf16 image, its norm and its bytes
__global__ __launch_bounds__(256) void retr_words_init_kernel(RowSrc R, const long long* __restrict__ rows, int D, uint16_t* __restrict__ voc_bf,
                                                              int* __restrict__ voc_norm, uint8_t* __restrict__ words) {
  const int w = blockIdx.x;
  RowSrc all = R;
  all.T = R.N;                                            // rows[] numbers the concatenation
  int set, loc;
  retr_locate(all, rows[w], &set, &loc);
  for (int d = threadIdx.x; d < R.dp; d += blockDim.x) {
    const uint16_t v = R.bf[set][(size_t)loc * R.dp + d];
    voc_bf[(size_t)w * R.dp + d] = v;
    if (d < D) words[(size_t)w * D + d] = (uint8_t)bf16_int(v);
  }
  if (threadIdx.x == 0) voc_norm[w] = R.norm[set][loc];
}

// One word per workgroup.  log3 = the round's row of the log on the device: [1] += 1 for a word without a row, [2] += 1
// for a word whose bytes change.  apply = 0 (the last row): nothing is written but the count of empty words.
__global__ __launch_bounds__(256) void retr_words_update_kernel(int D, int dp, const int* __restrict__ S, const int* __restrict__ cnt,
                                                                uint16_t* __restrict__ voc_bf, int* __restrict__ voc_norm,
                                                                uint8_t* __restrict__ words, u64* __restrict__ log3, int apply) {
  __shared__ int red[256];
  const int w = blockIdx.x, tid = threadIdx.x;
  const long long n = cnt[w];
  int changed = 0, nrm = 0;
  if (apply && n > 0)
    for (int d = tid; d < D; d += 256) {
      const int old = bf16_int(voc_bf[(size_t)w * dp + d]);
      const int nv = (int)((2LL * S[(size_t)w * D + d] + n) / (2 * n));
      changed |= nv != old;
      voc_bf[(size_t)w * dp + d] = int_bf16(nv);
      words[(size_t)w * D + d] = (uint8_t)nv;
      nrm += nv * nv;
    }
  const int any = __syncthreads_or(changed);
  red[tid] = nrm;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid != 0) return;
  if (apply && n > 0) voc_norm[w] = red[0];
  if (n == 0) atomicAdd(&log3[1], 1ULL);
  if (any) atomicAdd(&log3[2], 1ULL);
}

// ---------------------------------------------------------------------------------------------
// describing: r = S - n c, q = sgn(r) min(isqrt |r|, 127), norm2 = sum q^2; one view per workgroup
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int retr_isqrt(uint32_t v) {
  uint32_t s = (uint32_t)sqrt((double)v);
  while ((u64)s * s > v) --s;
  while ((u64)(s + 1) * (s + 1) <= v) ++s;
  return (int)s;
}

__global__ __launch_bounds__(256) void retr_quantise_kernel(int K, int D, int dp, const int* __restrict__ S, const int* __restrict__ cnt,
                                                            const uint16_t* __restrict__ voc_bf, int8_t* __restrict__ desc,
                                                            long long* __restrict__ norm2, int* __restrict__ word_count,
                                                            int* __restrict__ residual) {
  __shared__ int red[256];
  const int v = blockIdx.x, tid = threadIdx.x, KD = K * D;
  const int* s = S + (size_t)v * KD;
  const int* c = cnt + (size_t)v * K;
  int acc = 0;
  for (int i = tid; i < KD; i += 256) {
    const int w = i / D, d = i - w * D;
    const int r = s[i] - c[w] * bf16_int(voc_bf[(size_t)w * dp + d]);
    const int m = retr_isqrt((uint32_t)(r < 0 ? -r : r));
    const int q = (r < 0 ? -1 : 1) * (m < 127 ? m : 127);
    if (desc) desc[(size_t)v * KD + i] = (int8_t)q;
    if (residual) residual[(size_t)v * KD + i] = r;
    acc += q * q;
  }
  if (word_count)
    for (int w = tid; w < K; w += 256) word_count[(size_t)v * K + w] = c[w];
  red[tid] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0 && norm2) norm2[v] = red[0];
}

// ---------------------------------------------------------------------------------------------
// dot: hot path 2
// ---------------------------------------------------------------------------------------------
// A workgroup = 2 x 2 waves over a 64 x 64 tile of (row view, column view); a wave holds four 16 x 16 accumulators.  Both
// operands are plain 16-byte loads of the [view][stride] image: lane l takes bytes 16 (l >> 4) .. + 15 of each 64-wide k
// step of view (l & 15), as the A operand for the rows and as the B operand for the columns.  A and B use the same (lane,
// byte) -> k map, whatever it is, so the sum over k is the dot product; C[row 4 h + r][col l & 15] as for every 16 x 16
// shape.  Views past V - 1 are read as view V - 1 and not stored.
__global__ __launch_bounds__(256) void retr_dot_kernel(const int8_t* __restrict__ desc, int V, int stride, int r0, int r1, int* __restrict__ out,
                                                       long long ld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, h = lane >> 4;
  const int rowbase = r0 + blockIdx.y * 64 + (wave >> 1) * 32, colbase = blockIdx.x * 64 + (wave & 1) * 32;
  const int8_t* pa[2];
  const int8_t* pb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int ra = rowbase + 16 * s + r16, cb = colbase + 16 * s + r16;
    pa[s] = desc + (size_t)(ra < V ? ra : V - 1) * stride + 16 * h;
    pb[s] = desc + (size_t)(cb < V ? cb : V - 1) * stride + 16 * h;
  }
  i32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = i32x4{0, 0, 0, 0};
  for (int k0 = 0; k0 < stride; k0 += 64) {
    i32x4 a[2], b[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      a[s] = *reinterpret_cast<const i32x4*>(pa[s] + k0);
      b[s] = *reinterpret_cast<const i32x4*>(pb[s] + k0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rowbase + 16 * i + 4 * h + r, col = colbase + 16 * j + r16;
        if (row < r1 && col < V) out[(size_t)(row - r0) * ld + col] = acc[i][j][r];
      }
}

// ---------------------------------------------------------------------------------------------
// select: the k neighbours of a view, a wave per view.  The order is (score descending, b ascending) = ascending in
// (~order(score), b); round j takes the least pair above the one round j - 1 took.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retr_select_kernel(const int* __restrict__ dots, long long ld, int r0, int r1, int V,
                                                          const long long* __restrict__ norm2, int k, double min_score,
                                                          int* __restrict__ nbr, double* __restrict__ nbr_score) {
  const int lane = threadIdx.x & 63;
  const int a = r0 + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= r1) return;                                    // wave-uniform
  const long long na = norm2[a];
  const int* row = dots + (size_t)(a - r0) * ld;
  u64 last_key = 0;
  int last_b = -1;
  bool have = false, dry = na <= 0;
  for (int j = 0; j < k; ++j) {
    u64 bk = ~0ULL;
    int bb = INT_MAX;
    if (!dry)
      for (int b = lane; b < V; b += 64) {
        if (b == a) continue;
        const long long nb = norm2[b];
        if (nb <= 0) continue;
        const double sc = view_score(row[b], na, nb);
        if (!(sc >= min_score)) continue;
        const u64 key = ~f64_order(sc);
        if (have && !(key > last_key || (key == last_key && b > last_b))) continue;
        if (key < bk || (key == bk && b < bb)) { bk = key; bb = b; }
      }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const u64 ok = retr_shfl_xor_u64(bk, m);
      const int ob = __shfl_xor(bb, m, 64);
      if (ok < bk || (ok == bk && ob < bb)) { bk = ok; bb = ob; }
    }
    dry = dry || bb == INT_MAX;
    if (lane == 0) {
      nbr[(size_t)a * k + j] = dry ? -1 : bb;
      nbr_score[(size_t)a * k + j] = dry ? -INFINITY : f64_unorder(~bk);
    }
    last_key = bk; last_b = bb; have = true;
  }
}

// ---------------------------------------------------------------------------------------------
// pairs
// ---------------------------------------------------------------------------------------------
struct PairArgs {
  int V, k, mutual, sequential;
  long long cap;
  const int* nbr;               // [V][k]
  const int* rev_ptr;           // [V + 2]: the slots m = b k + j with nbr[m] = a, ascending; key V holds the missing entries
  const int* rev_list;          // [V k]
  int* cnt;                     // [V]
  int* start;                   // [V]
  int* pairs;                   // [cap][2] or null
  int* how;                     // [cap] or null
  u64* total;                   // [1]
};

__global__ __launch_bounds__(256) void retr_rev_key_kernel(int V, long long M, const int* __restrict__ nbr, int* __restrict__ key) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m < M) key[m] = nbr[m] < 0 ? V : nbr[m];
}

// The listed partners b > a of view a in ascending order: a merge of its own neighbours (the least one above the last b, by
// a scan of k entries), of the views that list it (a sorted list) and of the sequential range.
template <bool FILL>
__global__ __launch_bounds__(256) void retr_pairs_kernel(PairArgs P) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= P.V) return;
  const int* f = P.nbr + (size_t)a * P.k;
  int rp = P.rev_ptr[a];
  const int rend = P.rev_ptr[a + 1];
  while (rp < rend && P.rev_list[rp] / P.k <= a) ++rp;
  const long long seq_hi = (long long)a + P.sequential < P.V - 1 ? (long long)a + P.sequential : P.V - 1;
  const long long base = FILL ? P.start[a] : 0;
  int cur = a, count = 0;
  for (;;) {
    int nf = INT_MAX;
    for (int j = 0; j < P.k; ++j) {
      const int v = f[j];
      if (v > cur && v < nf) nf = v;
    }
    const int nr = rp < rend ? P.rev_list[rp] / P.k : INT_MAX;
    const int ns = cur + 1 <= seq_hi ? cur + 1 : INT_MAX;
    const int b = nf < nr ? (nf < ns ? nf : ns) : (nr < ns ? nr : ns);
    if (b == INT_MAX) break;
    const int how = (b == nf ? 1 : 0) | (b == nr ? 2 : 0) | (b == ns ? 4 : 0);
    if (b == nr) ++rp;
    cur = b;
    const bool listed = (how & 4) != 0 || (P.mutual ? (how & 3) == 3 : (how & 3) != 0);
    if (!listed) continue;
    if (FILL && base + count < P.cap) {
      if (P.pairs) { P.pairs[2 * (base + count)] = a; P.pairs[2 * (base + count) + 1] = b; }
      if (P.how) P.how[base + count] = how;
    }
    ++count;
  }
  if (!FILL) P.cnt[a] = count;
}

struct PairScan {
  PairArgs P;
  __device__ int n() const { return P.V; }
  __device__ void load(int a, int (&v)[1]) const { v[0] = P.cnt[a]; }
  __device__ void store(int a, const int (&p)[1]) const { P.start[a] = p[0]; }
  __device__ void total(const int (&t)[1]) const { P.total[0] = (u64)t[0]; }
};

// pair_score: a wave per written pair; the dot product again, four bytes per lane and step, in integers
__global__ __launch_bounds__(256) void retr_pair_score_kernel(const int8_t* __restrict__ desc, int stride, const long long* __restrict__ norm2,
                                                              const int* __restrict__ pairs, long long n, double* __restrict__ pair_score) {
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n) return;
  const int lane = threadIdx.x & 63;
  const int a = pairs[2 * p], b = pairs[2 * p + 1];
  const long long na = norm2[a], nb = norm2[b];
  const int* xa = reinterpret_cast<const int*>(desc + (size_t)a * stride);
  const int* xb = reinterpret_cast<const int*>(desc + (size_t)b * stride);
  int acc = 0;
  for (int i = lane; i < stride / 4; i += 64) {
    const int u = xa[i], v = xb[i];
#pragma unroll
    for (int s = 0; s < 32; s += 8) acc += (int)(int8_t)(u >> s) * (int)(int8_t)(v >> s);
  }
  acc = group_sum<64>(acc);
  if (lane == 0) pair_score[p] = (na > 0 && nb > 0) ? view_score(acc, na, nb) : -INFINITY;
}

// ---------------------------------------------------------------------------------------------
// host side: the argument rules (no device), then the bodies
// ---------------------------------------------------------------------------------------------
// The sets of a call: exact L2 sets of one dimension; *D their dimension, *N their rows, max_n the most one set may hold.
static int retr_check_sets(const char* who, const char* what, int n_sets, sfm_desc_set* const* sets, int* D, long long* N) {
  if (n_sets < 1 || n_sets > kRetrMaxViews) { set_error("%s: %d %ss (1 .. %d)", who, n_sets, what, kRetrMaxViews); return SFM_E_SHAPE; }
  if (sets == nullptr) { set_error("%s: null list of %ss", who, what); return SFM_E_SHAPE; }
  long long total = 0;
  for (int i = 0; i < n_sets; ++i) {
    const sfm_desc_set* s = sets[i];
    if (s == nullptr) { set_error("%s: %s %d is null", who, what, i); return SFM_E_SHAPE; }
    if (s->metric != SFM_MATCH_L2 || s->kind != kDescKindExact) {
      set_error("%s: %s %d is not an exact L2 set (Hamming and non-integer float sets are not described)", who, what, i);
      return SFM_E_SHAPE;
    }
    if (i == 0) *D = s->dim;
    if (s->dim != *D) { set_error("%s: %s %d has dim %d, %s 0 has %d", who, what, i, s->dim, what, *D); return SFM_E_SHAPE; }
    if (s->n > kRetrMaxViewKeys) { set_error("%s: %s %d has %d keys (at most 2^22)", who, what, i, s->n); return SFM_E_SHAPE; }
    total += s->n;
  }
  *N = total;
  return SFM_OK;
}

static int retr_check_words(const char* who, int K, int D) {
  if (K < 1 || K > kRetrMaxWords) { set_error("%s: K = %d words (1 .. %d)", who, K, kRetrMaxWords); return SFM_E_SHAPE; }
  if (D < 1 || D > kRetrMaxDim) { set_error("%s: dim %d (1 .. %d)", who, D, kRetrMaxDim); return SFM_E_SHAPE; }
  if ((long long)K * D > kRetrMaxLen) { set_error("%s: K * D = %lld exceeds %d", who, (long long)K * D, kRetrMaxLen); return SFM_E_SHAPE; }
  return SFM_OK;
}

static int retr_check_train(const char* who, int K, int iters, long long train_cap) {
  if (K < 1 || K > kRetrMaxWords) { set_error("%s: K = %d words (1 .. %d)", who, K, kRetrMaxWords); return SFM_E_SHAPE; }
  if (iters < 0 || iters > kRetrMaxIters) { set_error("%s: iters = %d (0 .. %d)", who, iters, kRetrMaxIters); return SFM_E_SHAPE; }
  if (train_cap < 0 || train_cap > kRetrCapMax) { set_error("%s: train_cap = %lld (0 = 2^20, at most 2^22)", who, train_cap); return SFM_E_SHAPE; }
  return SFM_OK;
}

static long long retr_train_rows(long long N, long long train_cap) {
  const long long cap = train_cap == 0 ? kRetrCapDefault : train_cap;
  return N <= cap ? N : cap;
}

// the start rows, as rows of the concatenation
static void retr_init_rows(long long N, long long T, int K, uint64_t seed, long long* rows) {
  for (int w = 0; w < K; ++w) {
    const long long lo = (long long)w * T / K, hi = (long long)(w + 1) * T / K;
    const u64 z = splitmix64_mix((u64)seed * (u64)K + (u64)w);
    rows[w] = retr_spread(lo + (long long)(z % (u64)(hi - lo)), N, T);
  }
}

static int retr_check_pairs(const char* who, int V, int len, const void* desc, const void* norm2, int k, double min_score, int mutual,
                            int sequential, long long cap, const void* pairs, const void* how, const void* pair_score) {
  if (V < 1 || V > kRetrMaxViews) { set_error("%s: V = %d views (1 .. %d)", who, V, kRetrMaxViews); return SFM_E_SHAPE; }
  if (len < 1 || len > kRetrMaxLen) { set_error("%s: len = %d (1 .. %d)", who, len, kRetrMaxLen); return SFM_E_SHAPE; }
  if (desc == nullptr || norm2 == nullptr) { set_error("%s: null desc or norm2", who); return SFM_E_SHAPE; }
  if (k < 1 || k > kRetrMaxK) { set_error("%s: k = %d neighbours (1 .. %d)", who, k, kRetrMaxK); return SFM_E_SHAPE; }
  if (min_score != min_score) { set_error("%s: min_score is NaN", who); return SFM_E_SHAPE; }
  if (mutual != 0 && mutual != 1) { set_error("%s: mutual = %d must be 0 or 1", who, mutual); return SFM_E_SHAPE; }
  if (sequential < 0) { set_error("%s: sequential = %d must be >= 0", who, sequential); return SFM_E_SHAPE; }
  if (cap < 0) { set_error("%s: cap = %lld must be >= 0", who, cap); return SFM_E_SHAPE; }
  if (cap > 0 && pairs == nullptr && (how != nullptr || pair_score != nullptr)) { set_error("%s: how or pair_score without pairs", who); return SFM_E_SHAPE; }
  const long long seq = sequential < V ? sequential : V;
  if ((long long)V * (2LL * k + seq) >= (1LL << 31)) { set_error("%s: V (2 k + sequential) reaches 2^31 pairs", who); return SFM_E_SHAPE; }
  return SFM_OK;
}

// The rows of a list of sets on the device.
struct RowTables {
  DevBuf<long long> off;
  DevBuf<const uint16_t*> bf;
  DevBuf<const int*> norm;
  int upload(int n_sets, sfm_desc_set* const* sets, hipStream_t s) {
    std::vector<long long> o((size_t)n_sets + 1, 0);
    std::vector<const uint16_t*> b(n_sets);
    std::vector<const int*> n(n_sets);
    for (int i = 0; i < n_sets; ++i) { o[i + 1] = o[i] + sets[i]->n; b[i] = sets[i]->bf; n[i] = sets[i]->norm; }
    SFM_TRY(off.upload(o.data(), o.size(), s));
    SFM_TRY(bf.upload(b.data(), b.size(), s));
    SFM_TRY(norm.upload(n.data(), n.size(), s));
    SFM_HIP(hipStreamSynchronize(s));                      // the host vectors die with this frame
    return SFM_OK;
  }
};

static void retr_assign_launch(const RowSrc& R, const uint16_t* voc_bf, const int* voc_norm, int K, int* assign, uint32_t* dist, hipStream_t s) {
  if (R.T == 0) return;
  const unsigned grid = (unsigned)((R.T + kRetrTileRows - 1) / kRetrTileRows);
  if (R.dp == 128) retr_assign_kernel<4><<<grid, 256, 0, s>>>(R, voc_bf, voc_norm, K, assign, dist);
  else retr_assign_kernel<8><<<grid, 256, 0, s>>>(R, voc_bf, voc_norm, K, assign, dist);
}

static void retr_accum_launch(const RowSrc& R, const int4* chunks, int n_chunks, const int* assign, const uint32_t* dist, int K, int D, int* S,
                              int* cnt, u64* inertia, hipStream_t s) {
  if (n_chunks == 0) return;
  const size_t bytes = ((size_t)K * D + K) * sizeof(int);
  if (bytes <= (size_t)kRetrLdsBytes) retr_accum_kernel<true><<<(unsigned)n_chunks, R.dp, bytes, s>>>(R, chunks, assign, dist, K, D, S, cnt, inertia);
  else retr_accum_kernel<false><<<(unsigned)n_chunks, R.dp, 0, s>>>(R, chunks, assign, dist, K, D, S, cnt, inertia);
}

static int retr_train_run(int n_sets, sfm_desc_set* const* sets, int K, int D, long long N, long long T, int iters, uint64_t seed,
                          uint8_t* words_out, int64_t* log, hipStream_t s) {
  const int dp = sets[0]->dp, KD = K * D, K_pad = (K + 127) / 128 * 128;
  RowTables rt;
  SFM_TRY(rt.upload(n_sets, sets, s));
  const RowSrc R{rt.off.p, rt.bf.p, rt.norm.p, n_sets, dp, N, T};
  std::vector<long long> rows(K);
  retr_init_rows(N, T, K, seed, rows.data());
  std::vector<int4> chunks;
  for (long long t = 0; t < T; t += kRetrChunkRows) chunks.push_back(make_int4(0, (int)t, (int)(t + kRetrChunkRows < T ? t + kRetrChunkRows : T), 0));
  DevBuf<long long> d_rows;
  DevBuf<int4> d_chunks;
  DevBuf<uint16_t> voc_bf;
  DevBuf<int> voc_norm, assign, S, cnt;
  DevBuf<uint32_t> dist;
  DevBuf<uint8_t> words;
  DevBuf<u64> d_log;
  SFM_TRY(d_rows.upload(rows.data(), rows.size(), s));
  SFM_TRY(d_chunks.upload(chunks.data(), chunks.size(), s));
  SFM_TRY(voc_bf.alloc((size_t)K_pad * dp, s)); SFM_TRY(voc_norm.alloc(K_pad, s)); SFM_TRY(words.alloc(KD, s));
  SFM_TRY(assign.alloc((size_t)T, s)); SFM_TRY(dist.alloc((size_t)T, s)); SFM_TRY(S.alloc(KD, s)); SFM_TRY(cnt.alloc(K, s));
  SFM_TRY(d_log.alloc(3 * ((size_t)iters + 1), s));
  SFM_HIP(hipMemsetAsync(voc_bf.p, 0, sizeof(uint16_t) * (size_t)K_pad * dp, s));
  SFM_HIP(hipMemsetAsync(voc_norm.p, 0, sizeof(int) * (size_t)K_pad, s));
  SFM_HIP(hipMemsetAsync(d_log.p, 0, sizeof(u64) * 3 * ((size_t)iters + 1), s));
  retr_words_init_kernel<<<K, 256, 0, s>>>(R, d_rows.p, D, voc_bf.p, voc_norm.p, words.p);
  for (int round = 0; round <= iters; ++round) {
    retr_assign_launch(R, voc_bf.p, voc_norm.p, K, assign.p, dist.p, s);
    SFM_HIP(hipMemsetAsync(S.p, 0, sizeof(int) * (size_t)KD, s));
    SFM_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int) * (size_t)K, s));
    retr_accum_launch(R, d_chunks.p, (int)chunks.size(), assign.p, dist.p, K, D, S.p, cnt.p, d_log.p + 3 * round, s);
    retr_words_update_kernel<<<K, 256, 0, s>>>(D, dp, S.p, cnt.p, voc_bf.p, voc_norm.p, words.p, d_log.p + 3 * round, round < iters ? 1 : 0);
  }
  SFM_HIP(hipGetLastError());
  std::vector<u64> h_log(3 * ((size_t)iters + 1));
  SFM_HIP(hipMemcpyAsync(words_out, words.p, (size_t)KD, hipMemcpyDeviceToHost, s));
  SFM_HIP(hipMemcpyAsync(h_log.data(), d_log.p, sizeof(u64) * h_log.size(), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  if (log != nullptr)
    for (size_t i = 0; i < h_log.size(); ++i) log[i] = (int64_t)h_log[i];
  return SFM_OK;
}

// Describing; device outputs, any of them null.  Enqueues on s and waits (its work buffers go back to the pool).
static int retr_describe_run(sfm_desc_set* vocab, int V, sfm_desc_set* const* views, int D, long long N, int8_t* d_desc, long long* d_norm2,
                             int* d_word_count, int* d_assign, int* d_residual, hipStream_t s) {
  const int K = vocab->n, dp = vocab->dp, KD = K * D;
  RowTables rt;
  SFM_TRY(rt.upload(V, views, s));
  const RowSrc R{rt.off.p, rt.bf.p, rt.norm.p, V, dp, N, N};
  DevBuf<int> assign, S, cnt;
  DevBuf<uint32_t> dist;
  if (d_assign == nullptr) { SFM_TRY(assign.alloc((size_t)N, s)); d_assign = assign.p; }
  SFM_TRY(dist.alloc((size_t)N, s));
  retr_assign_launch(R, vocab->bf, vocab->norm, K, d_assign, dist.p, s);
  SFM_HIP(hipGetLastError());
  if (d_desc == nullptr && d_norm2 == nullptr && d_word_count == nullptr && d_residual == nullptr) return stream_sync(s);
  // batches of views whose sums fit the work buffer; the chunks of a view do not leave it
  const int batch = (int)std::max<long long>(1, std::min<long long>(V, kRetrSumInts / KD));
  SFM_TRY(S.alloc((size_t)batch * KD, s)); SFM_TRY(cnt.alloc((size_t)batch * K, s));
  std::vector<int4> chunks;
  std::vector<int> first_chunk;
  long long off = 0;
  for (int v = 0; v < V; ++v) {
    if (v % batch == 0) first_chunk.push_back((int)chunks.size());
    for (long long t = 0; t < views[v]->n; t += kRetrChunkRows)
      chunks.push_back(make_int4(v % batch, (int)(off + t), (int)(off + (t + kRetrChunkRows < views[v]->n ? t + kRetrChunkRows : views[v]->n)), 0));
    off += views[v]->n;
  }
  first_chunk.push_back((int)chunks.size());
  DevBuf<int4> d_chunks;
  SFM_TRY(d_chunks.upload(chunks.data(), chunks.size(), s));
  for (int v0 = 0, bi = 0; v0 < V; v0 += batch, ++bi) {
    const int nv = v0 + batch < V ? batch : V - v0;
    SFM_HIP(hipMemsetAsync(S.p, 0, sizeof(int) * (size_t)nv * KD, s));
    SFM_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int) * (size_t)nv * K, s));
    retr_accum_launch(R, d_chunks.p + first_chunk[bi], first_chunk[bi + 1] - first_chunk[bi], d_assign, dist.p, K, D, S.p, cnt.p, nullptr, s);
    retr_quantise_kernel<<<nv, 256, 0, s>>>(K, D, dp, S.p, cnt.p, vocab->bf, d_desc ? d_desc + (size_t)v0 * KD : nullptr,
                                             d_norm2 ? d_norm2 + v0 : nullptr, d_word_count ? d_word_count + (size_t)v0 * K : nullptr,
                                             d_residual ? d_residual + (size_t)v0 * KD : nullptr);
  }
  SFM_HIP(hipGetLastError());
  return stream_sync(s);
}

static int retr_describe_check(const char* who, sfm_desc_set* vocab, int n_views, sfm_desc_set* const* views, int* D, long long* N) {
  if (vocab == nullptr) { set_error("%s: the vocabulary is null", who); return SFM_E_SHAPE; }
  sfm_desc_set* const one[1] = {vocab};
  int Dv = 0;
  long long Kv = 0;
  SFM_TRY(retr_check_sets(who, "vocabulary", 1, one, &Dv, &Kv));
  SFM_TRY(retr_check_words(who, (int)std::min<long long>(Kv, INT_MAX), Dv));
  SFM_TRY(retr_check_sets(who, "view", n_views, views, D, N));
  if (*D != Dv) { set_error("%s: the views have dim %d, the vocabulary %d", who, *D, Dv); return SFM_E_SHAPE; }
  if (*N >= (1LL << 31)) { set_error("%s: %lld keys in all (fewer than 2^31)", who, *N); return SFM_E_SHAPE; }
  return SFM_OK;
}

// Pairs; device arrays, *n_pairs on the host.  Waits for s.
static int retr_pairs_run(int V, int len, const int8_t* d_desc, const long long* d_norm2, int k, double min_score, int mutual, int sequential,
                          long long cap, int* d_nbr, double* d_nbr_score, int* d_pairs, int* d_how, double* d_pair_score, int* d_dot,
                          int64_t* n_pairs, hipStream_t s) {
  // the image the kernels read: rows of a multiple of 64 bytes at 16-byte aligned addresses, zero padded
  const int stride = (len + 63) / 64 * 64;
  DevBuf<int8_t> padded;
  if (stride != len || (reinterpret_cast<uintptr_t>(d_desc) & 15) != 0) {
    SFM_TRY(padded.alloc((size_t)V * stride, s));
    SFM_HIP(hipMemsetAsync(padded.p, 0, (size_t)V * stride, s));
    SFM_HIP(hipMemcpy2DAsync(padded.p, stride, d_desc, len, len, V, hipMemcpyDeviceToDevice, s));
    d_desc = padded.p;
  }
  DevBuf<int> nbr, strip, key, rev_ptr, rev_list, cnt, start, tiles;
  DevBuf<double> nbr_score;
  DevBuf<u64> total;
  if (d_nbr == nullptr) { SFM_TRY(nbr.alloc((size_t)V * k, s)); d_nbr = nbr.p; }
  if (d_nbr_score == nullptr) { SFM_TRY(nbr_score.alloc((size_t)V * k, s)); d_nbr_score = nbr_score.p; }
  long long strip_rows = V;
  if (d_dot == nullptr) {
    strip_rows = std::max<long long>(64, kRetrStripInts / V / 64 * 64);
    strip_rows = std::min<long long>(strip_rows, (V + 63) / 64 * 64);
    SFM_TRY(strip.alloc((size_t)strip_rows * V, s));
  }
  for (long long r0 = 0; r0 < V; r0 += strip_rows) {
    const int r1 = (int)std::min<long long>(V, r0 + strip_rows);
    int* out = d_dot ? d_dot : strip.p;
    const dim3 grid((unsigned)((V + 63) / 64), (unsigned)((r1 - r0 + 63) / 64));
    retr_dot_kernel<<<grid, 256, 0, s>>>(d_desc, V, stride, (int)r0, r1, out, V);
    retr_select_kernel<<<(unsigned)((r1 - r0 + 3) / 4), 256, 0, s>>>(out, V, (int)r0, r1, V, d_norm2, k, min_score, d_nbr, d_nbr_score);
  }
  SFM_HIP(hipGetLastError());
  // the reverse lists: the slots of nbr by the view they name (missing entries under the extra key V)
  const long long M = (long long)V * k;
  SFM_TRY(key.alloc((size_t)M, s)); SFM_TRY(rev_ptr.alloc((size_t)V + 2, s)); SFM_TRY(rev_list.alloc((size_t)M, s));
  SFM_TRY(cnt.alloc(V, s)); SFM_TRY(start.alloc(V, s)); SFM_TRY(total.alloc(1, s));
  retr_rev_key_kernel<<<(unsigned)((M + 255) / 256), 256, 0, s>>>(V, M, d_nbr, key.p);
  SFM_TRY(key_major_list(M, V + 1, key.p, rev_ptr.p, rev_list.p, s));
  PairArgs P{V, k, mutual, sequential, d_pairs ? cap : 0, d_nbr, rev_ptr.p, rev_list.p, cnt.p, start.p, d_pairs, d_how, total.p};
  const unsigned view_blocks = (unsigned)((V + 255) / 256);
  retr_pairs_kernel<false><<<view_blocks, 256, 0, s>>>(P);
  const int n_tiles = (V + kScanBlock - 1) / kScanBlock;
  SFM_TRY(tiles.alloc(2 * (size_t)n_tiles + 2, s));
  exclusive_scan_launch<1>(PairScan{P}, true, tiles.p, n_tiles, s);
  retr_pairs_kernel<true><<<view_blocks, 256, 0, s>>>(P);
  SFM_HIP(hipGetLastError());
  u64 count = 0;
  SFM_HIP(hipMemcpyAsync(&count, total.p, sizeof(count), hipMemcpyDeviceToHost, s));
  SFM_HIP(hipStreamSynchronize(s));
  const long long written = std::min<long long>((long long)count, P.cap);
  if (d_pair_score != nullptr && d_pairs != nullptr && written > 0)
    retr_pair_score_kernel<<<(unsigned)((written + 3) / 4), 256, 0, s>>>(d_desc, stride, d_norm2, d_pairs, written, d_pair_score);
  SFM_HIP(hipGetLastError());
  if (n_pairs != nullptr) *n_pairs = (int64_t)count;
  return stream_sync(s);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_view_score(int dot, int64_t norm2_a, int64_t norm2_b, double* score_out) {
  if (score_out == nullptr) { set_error("sfm_view_score: null score_out"); return SFM_E_SHAPE; }
  *score_out = view_score(dot, norm2_a, norm2_b);
  return SFM_OK;
}

int sfm_vocab_init_rows(int64_t N, int K, uint64_t seed, int64_t train_cap, int64_t* rows_out) {
  const char* who = "sfm_vocab_init_rows";
  SFM_TRY(retr_check_train(who, K, 0, train_cap));
  if (rows_out == nullptr) { set_error("%s: null rows_out", who); return SFM_E_SHAPE; }
  if (N < 0 || N > (long long)kRetrMaxViews * kRetrMaxViewKeys) { set_error("%s: N = %lld rows", who, (long long)N); return SFM_E_SHAPE; }
  const long long T = retr_train_rows(N, train_cap);
  if (T < K) { set_error("%s: T = %lld training rows for K = %d words", who, T, K); return SFM_E_SHAPE; }
  std::vector<long long> rows(K);
  retr_init_rows(N, T, K, seed, rows.data());
  for (int w = 0; w < K; ++w) rows_out[w] = rows[w];
  return SFM_OK;
}

int sfm_vocab_train(int n_sets, sfm_desc_set* const* sets, int K, int iters, uint64_t seed, int64_t train_cap, uint8_t* words_out, int64_t* log) {
  const char* who = "sfm_vocab_train";
  SFM_TRY(retr_check_train(who, K, iters, train_cap));
  if (words_out == nullptr) { set_error("%s: null words_out", who); return SFM_E_SHAPE; }
  int D = 0;
  long long N = 0;
  SFM_TRY(retr_check_sets(who, "set", n_sets, sets, &D, &N));
  SFM_TRY(retr_check_words(who, K, D));
  const long long T = retr_train_rows(N, train_cap);
  if (T < K) { set_error("%s: T = %lld training rows for K = %d words", who, T, K); return SFM_E_SHAPE; }
  SFM_TRY(ensure_init());
  return retr_train_run(n_sets, sets, K, D, N, T, iters, seed, words_out, log, ctx().stream);
}

int sfm_view_describe_dev(sfm_desc_set* vocab, int n_views, sfm_desc_set* const* views, int8_t* d_desc, int64_t* d_norm2, int* d_word_count,
                          int* d_assign, int* d_residual, void* hip_stream) {
  int D = 0;
  long long N = 0;
  SFM_TRY(retr_describe_check("sfm_view_describe_dev", vocab, n_views, views, &D, &N));
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  return retr_describe_run(vocab, n_views, views, D, N, d_desc, reinterpret_cast<long long*>(d_norm2), d_word_count, d_assign, d_residual, s);
}

int sfm_view_describe(sfm_desc_set* vocab, int n_views, sfm_desc_set* const* views, int8_t* desc, int64_t* norm2, int* word_count, int* assign,
                      int* residual) {
  int D = 0;
  long long N = 0;
  SFM_TRY(retr_describe_check("sfm_view_describe", vocab, n_views, views, &D, &N));
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t V = (size_t)n_views, K = (size_t)vocab->n, KD = K * D;
  HostOut<int8_t> oDesc;
  HostOut<int64_t> oNorm;
  HostOut<int> oCount, oAssign, oRes;
  SFM_TRY(oDesc.want(desc, V * KD, s)); SFM_TRY(oNorm.want(norm2, V, s)); SFM_TRY(oCount.want(word_count, V * K, s));
  SFM_TRY(oAssign.want(assign, (size_t)N, s)); SFM_TRY(oRes.want(residual, V * KD, s));
  SFM_TRY(retr_describe_run(vocab, n_views, views, D, N, oDesc.dev(), reinterpret_cast<long long*>(oNorm.dev()), oCount.dev(), oAssign.dev(),
                            oRes.dev(), s));
  SFM_TRY(oDesc.fetch(s)); SFM_TRY(oNorm.fetch(s)); SFM_TRY(oCount.fetch(s)); SFM_TRY(oAssign.fetch(s)); SFM_TRY(oRes.fetch(s));
  return stream_sync(s);
}

int sfm_view_pairs_dev(int V, int len, const int8_t* d_desc, const int64_t* d_norm2, int k, double min_score, int mutual, int sequential,
                       int64_t cap, int* d_nbr, double* d_nbr_score, int* d_pairs, int* d_how, double* d_pair_score, int* d_dot,
                       int64_t* n_pairs, void* hip_stream) {
  SFM_TRY(retr_check_pairs("sfm_view_pairs_dev", V, len, d_desc, d_norm2, k, min_score, mutual, sequential, cap, d_pairs, d_how, d_pair_score));
  SFM_TRY(ensure_init());
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  return retr_pairs_run(V, len, d_desc, reinterpret_cast<const long long*>(d_norm2), k, min_score, mutual, sequential, cap, d_nbr, d_nbr_score,
                        d_pairs, d_how, d_pair_score, d_dot, n_pairs, s);
}

int sfm_view_pairs(int V, int len, const int8_t* desc, const int64_t* norm2, int k, double min_score, int mutual, int sequential, int64_t cap,
                   int* nbr, double* nbr_score, int* pairs, int* how, double* pair_score, int* dot, int64_t* n_pairs) {
  SFM_TRY(retr_check_pairs("sfm_view_pairs", V, len, desc, norm2, k, min_score, mutual, sequential, cap, pairs, how, pair_score));
  SFM_TRY(ensure_init());
  hipStream_t s = ctx().stream;
  const size_t nv = (size_t)V, n_cap = (size_t)cap;
  DevBuf<int8_t> dDesc;
  DevBuf<int64_t> dNorm;
  HostOut<int> oNbr, oPairs, oHow, oDot;
  HostOut<double> oNbrScore, oPairScore;
  SFM_TRY(dDesc.upload(desc, nv * len, s)); SFM_TRY(dNorm.upload(norm2, nv, s));
  SFM_TRY(oNbr.want(nbr, nv * k, s)); SFM_TRY(oNbrScore.want(nbr_score, nv * k, s)); SFM_TRY(oDot.want(dot, nv * nv, s));
  if (cap > 0) { SFM_TRY(oPairs.want(pairs, 2 * n_cap, s)); SFM_TRY(oHow.want(how, n_cap, s)); SFM_TRY(oPairScore.want(pair_score, n_cap, s)); }
  int64_t count = 0;
  SFM_TRY(retr_pairs_run(V, len, dDesc.p, reinterpret_cast<const long long*>(dNorm.p), k, min_score, mutual, sequential, cap, oNbr.dev(),
                         oNbrScore.dev(), oPairs.dev(), oHow.dev(), oPairScore.dev(), oDot.dev(), &count, s));
  SFM_TRY(oNbr.fetch(s)); SFM_TRY(oNbrScore.fetch(s)); SFM_TRY(oDot.fetch(s));
  // only the rows that were written come back: the rest of the caller's arrays stays as it was
  const size_t written = (size_t)std::min<long long>(count, cap);
  if (written > 0) {
    if (pairs) SFM_TRY(oPairs.buf.download(pairs, 2 * written, s));
    if (how) SFM_TRY(oHow.buf.download(how, written, s));
    if (pair_score) SFM_TRY(oPairScore.buf.download(pair_score, written, s));
  }
  if (n_pairs != nullptr) *n_pairs = count;
  return stream_sync(s);
}

}  // extern "C"
