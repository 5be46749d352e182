// sfm_match.hip — brute-force descriptor matching of KeyTracker.__extend_list (key_tracker.py:248-262): the new
// view's descriptors against every resident earlier view in ONE launch, per (reference view, query) the best two
// train indices by the contract's order (distance, train index), and the column-wise best query for cross-check.
//
// Three distance kernels share one selection:
//  * exact L2 (the hot path): integer descriptors in [0, 255] are exact in bf16 and every partial dot product stays
//    below 2^24, so v_mfma_f32_16x16x32_bf16 with f32 accumulation returns a . b exactly in any order; the squared
//    distance s = |a|^2 + |b|^2 - 2 a . b is then an exact int32;
//  * Hamming: v_xor + v_bcnt over uint32 words (rows zero-padded to whole words);
//  * general L2: fp32 sum of (a - b)^2 for float data that is not integer-valued (correct, not tuned).
// Selection keys are 64-bit (value << 32 | index): one unsigned compare orders by (value, index), so ties go to the
// lower index.  For exact L2 the value is s mapped to the SMALLEST integer with the same float32(sqrt(s)) (identity
// below 2^22, where sqrt is injective on the integers at float precision; a rarely taken branch above), so that two s
// whose rounded distances tie compare by index, as the contract's (d, index) order requires.  Hamming values are the
// popcounts themselves; general L2 values are the bits of the float32 distance (non-negative floats order as integers).
//
// The train axis is cut into chunks of CHUNK columns (a device table of (reference, first, last) rows over all
// reference views); each workgroup takes one query tile against one chunk and leaves its partial top-2 per query in a
// scratch buffer, which match_merge_kernel folds per (reference, query).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "sfm_common.h"

namespace {

constexpr int CHUNK = 1024;         // train columns per workgroup
constexpr int ROW_PAD = 128;        // rows of every set are padded to a multiple of this (query tile of the MFMA kernel)
constexpr int MFMA_ROWS = 128;      // query rows per workgroup of the MFMA kernel: 4 waves x 2 strips x 16
constexpr int SIMT_ROWS = 256;      // query rows per workgroup of the thread-per-query kernels
constexpr uint64_t NO_KEY = ~0ull;
constexpr uint32_t CANON_FROM = 1u << 22;
constexpr int MAX_L2_DIM = 256;     // exact path: 256 * 255^2 < 2^24; general path: registers per query row
constexpr int MAX_HAMMING_WORDS = 64;

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

enum Kind : int { KIND_EXACT = 0, KIND_HAMMING = 1, KIND_FLOAT = 2 };

struct RefSeg {                     // one reference view as the kernels see it
  const uint16_t* bf;               // exact L2: [n_pad][dp] bf16
  const int* norm;                  // exact L2: [n] |b|^2
  const float* f32;                 // general L2: [n_pad][dp]
  const uint32_t* words;            // Hamming: [n_pad][dp] uint32 words
  int n;
  int stride;                       // elements per row of the image the kernel reads
};

// float32(sqrt(s)), correctly rounded, for an integer s < 2^32: the double square root rounded to float can sit on
// the wrong side of a float midpoint only through double rounding; the midpoints m have 25 significant bits, so m^2
// is exact in double and the comparison with s settles it (m^2 is never an integer here: m = odd * 2^-e, e >= 1).
__host__ __device__ inline float sqrt_int_rn(uint32_t s) {
  if (s == 0) return 0.0f;
  float d = (float)sqrt((double)s);
  uint32_t bits;
  memcpy(&bits, &d, 4);
  float pred, succ;
  uint32_t pb = bits - 1, sb = bits + 1;
  memcpy(&pred, &pb, 4);
  memcpy(&succ, &sb, 4);
  const double ds = (double)s;
  const double mlo = 0.5 * ((double)pred + (double)d), mhi = 0.5 * ((double)d + (double)succ);
  if (ds < mlo * mlo) return pred;
  if (ds > mhi * mhi) return succ;
  return d;
}

// The smallest integer with the same float32(sqrt(.)) as s.
__host__ __device__ inline uint32_t canon_s(uint32_t s) {
  const float d = sqrt_int_rn(s);
  uint32_t bits;
  memcpy(&bits, &d, 4);
  uint32_t pb = bits - 1;
  float pred;
  memcpy(&pred, &pb, 4);
  const double m = 0.5 * ((double)pred + (double)d);
  return (uint32_t)floor(m * m) + 1u;
}

__device__ __forceinline__ void top2_insert(uint64_t& k1, uint64_t& k2, uint64_t k) {
  if (k < k1) { k2 = k1; k1 = k; }
  else if (k < k2) k2 = k;
}

__device__ __forceinline__ void top2_merge(uint64_t& k1, uint64_t& k2, uint64_t b1, uint64_t b2) {
  if (b1 < k1) { k2 = k1 < b2 ? k1 : b2; k1 = b1; }
  else if (b1 < k2) k2 = b1;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- exact L2: MFMA 16x16x32 bf16 ---------------------------------------------------------------------------------
// Workgroup = 4 waves over 128 query rows (each wave two 16-row strips) against one chunk of one reference view.
// Per 16-column train tile a lane holds, for each strip, C[row 4h + r][col l & 15] (r = 0..3, h = l >> 4): the dot
// products of 8 query rows with ONE train column; it keeps a running top-2 for those 8 rows and the 16 lanes of a
// row group fold theirs at the end.  A operand: lane l holds query row (l & 15), k = 8h .. 8h + 7 of each 32-wide k
// step; B operand: train row (l & 15), same k -- both plain 16-byte row loads of the [row][k] images.
template <int KS, bool MUTUAL>
__global__ __launch_bounds__(256) void match_l2_mfma_kernel(const uint16_t* __restrict__ q_bf, const int* __restrict__ q_norm, int nq,
                                                            const RefSeg* __restrict__ segs, const int4* __restrict__ chunks,
                                                            uint64_t* __restrict__ partial, int nq_pad,
                                                            uint64_t* const* __restrict__ colbest) {
  constexpr int DP = KS * 32;
  __shared__ uint64_t col_lds[MUTUAL ? CHUNK : 1];
  const int4 ch = chunks[blockIdx.y];                 // {ref, first, last}
  const RefSeg seg = segs[ch.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, h = lane >> 4;
  const int q0 = blockIdx.x * MFMA_ROWS + wave * 32;
  if (MUTUAL) {
    for (int i = threadIdx.x; i < CHUNK; i += 256) col_lds[i] = NO_KEY;
    __syncthreads();
  }
  bf16x8 a[2][KS];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      a[s][ks] = *reinterpret_cast<const bf16x8*>(q_bf + (size_t)(q0 + 16 * s + r16) * DP + ks * 32 + 8 * h);
  int qn[2][4];
  uint64_t k1[2][4], k2[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 16 * s + 4 * h + r;
      qn[s][r] = q < nq ? q_norm[q] : 0;
      k1[s][r] = k2[s][r] = NO_KEY;
    }
  for (int t = ch.y; t < ch.z; t += 16) {
    const int col = t + r16;                          // < n_pad: the rows of the image are padded to 128
    bf16x8 b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const bf16x8*>(seg.bf + (size_t)col * DP + ks * 32 + 8 * h);
    const bool valid = col < ch.z;
    const int tn = valid ? seg.norm[col] : 0;
    uint64_t cbest = NO_KEY;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s][ks], b[ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uint32_t sv = (uint32_t)(qn[s][r] + tn - 2 * (int)acc[r]);
        if (sv >= CANON_FROM) sv = canon_s(sv);
        if (valid) top2_insert(k1[s][r], k2[s][r], ((uint64_t)sv << 32) | (uint32_t)col);
        const int q = q0 + 16 * s + 4 * h + r;
        if (MUTUAL && valid && q < nq) cbest = min_u64(cbest, ((uint64_t)sv << 32) | (uint32_t)q);
      }
    }
    if (MUTUAL) {
      cbest = min_u64(cbest, shfl_xor_u64(cbest, 16));
      cbest = min_u64(cbest, shfl_xor_u64(cbest, 32));
      if (h == 0 && valid) atomicMin(reinterpret_cast<unsigned long long*>(&col_lds[col - ch.y]), (unsigned long long)cbest);
    }
  }
  // fold the 16 lanes of a row group (lanes that differ in bits 0..3)
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        const uint64_t b1 = shfl_xor_u64(k1[s][r], m), b2 = shfl_xor_u64(k2[s][r], m);
        top2_merge(k1[s][r], k2[s][r], b1, b2);
      }
      const int q = q0 + 16 * s + 4 * h + r;
      if (r16 == 0 && q < nq) {
        uint64_t* out = partial + 2 * ((size_t)blockIdx.y * nq_pad + q);
        out[0] = k1[s][r];
        out[1] = k2[s][r];
      }
    }
  if (MUTUAL) {
    __syncthreads();
    uint64_t* cb = colbest[ch.x];
    for (int i = threadIdx.x; i < ch.z - ch.y; i += 256)
      if (col_lds[i] != NO_KEY) atomicMin(reinterpret_cast<unsigned long long*>(&cb[ch.y + i]), (unsigned long long)col_lds[i]);
  }
}

// ---- Hamming and general L2: one thread per query row ----------------------------------------------------------
// The train row is the same address for every lane of the workgroup (a broadcast load); the query row sits in
// registers (MAXW words / floats, the first W of them used).
template <int KIND, int MAXW, bool MUTUAL>
__global__ __launch_bounds__(256) void match_simt_kernel(const void* __restrict__ q_rows, int nq, int w, const RefSeg* __restrict__ segs,
                                                         const int4* __restrict__ chunks, uint64_t* __restrict__ partial, int nq_pad,
                                                         uint64_t* const* __restrict__ colbest) {
  __shared__ uint64_t col_lds[MUTUAL ? CHUNK : 1];
  const int4 ch = chunks[blockIdx.y];
  const RefSeg seg = segs[ch.x];
  const int q = blockIdx.x * SIMT_ROWS + threadIdx.x;    // < nq_pad: rows are padded to 128, tiles of 256 may pass it
  const bool live = q < nq;
  if (MUTUAL) {
    for (int i = threadIdx.x; i < CHUNK; i += 256) col_lds[i] = NO_KEY;
    __syncthreads();
  }
  uint32_t qv[MAXW];
  const uint32_t* qsrc = reinterpret_cast<const uint32_t*>(q_rows) + (size_t)(live ? q : 0) * w;
#pragma unroll
  for (int i = 0; i < MAXW; ++i) qv[i] = i < w ? qsrc[i] : 0u;
  uint64_t k1 = NO_KEY, k2 = NO_KEY;
  const uint32_t* base = KIND == KIND_HAMMING ? seg.words : reinterpret_cast<const uint32_t*>(seg.f32);
  for (int t = ch.y; t < ch.z; ++t) {
    const uint32_t* trow = base + (size_t)t * w;
    uint32_t v;
    if (KIND == KIND_HAMMING) {
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < MAXW; ++i)
        if (i < w) c += __builtin_popcount(qv[i] ^ trow[i]);
      v = c;
    } else {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < MAXW; ++i)
        if (i < w) {
          const float e = __uint_as_float(qv[i]) - __uint_as_float(trow[i]);
          acc = __builtin_fmaf(e, e, acc);
        }
      // sqrtf, not __fsqrt_rn: HIP maps the latter to the bare v_sqrt_f32 (1 ulp), sqrtf is correctly rounded
      v = __float_as_uint(sqrtf(acc));
    }
    const uint64_t key = ((uint64_t)v << 32) | (uint32_t)t;
    if (live) top2_insert(k1, k2, key);
    if (MUTUAL) {
      uint64_t cb = live ? (((uint64_t)v << 32) | (uint32_t)q) : NO_KEY;
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) cb = min_u64(cb, shfl_xor_u64(cb, m));
      if ((threadIdx.x & 63) == 0 && cb != NO_KEY) atomicMin(reinterpret_cast<unsigned long long*>(&col_lds[t - ch.y]), (unsigned long long)cb);
    }
  }
  if (live) {
    uint64_t* out = partial + 2 * ((size_t)blockIdx.y * nq_pad + q);
    out[0] = k1;
    out[1] = k2;
  }
  if (MUTUAL) {
    __syncthreads();
    uint64_t* cb = colbest[ch.x];
    for (int i = threadIdx.x; i < ch.z - ch.y; i += 256)
      if (col_lds[i] != NO_KEY) atomicMin(reinterpret_cast<unsigned long long*>(&cb[ch.y + i]), (unsigned long long)col_lds[i]);
  }
}

__device__ __forceinline__ float key_distance(int kind, uint64_t key) {
  const uint32_t v = (uint32_t)(key >> 32);
  if (kind == KIND_EXACT) return sqrt_int_rn(v);
  if (kind == KIND_HAMMING) return (float)v;
  return __uint_as_float(v);
}

// Per (reference, query): fold the partial top-2 of the reference's chunks; the mutual flag from the column bests.
__global__ void match_merge_kernel(int kind, int nq, int n_refs, const int* __restrict__ ref_chunk0, const uint64_t* __restrict__ partial,
                                   int nq_pad, uint64_t* const* __restrict__ colbest, int* __restrict__ best_idx, float* __restrict__ best_dist,
                                   int* __restrict__ second_idx, float* __restrict__ second_dist, uint8_t* __restrict__ mutual) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (q >= nq || r >= n_refs) return;
  uint64_t k1 = NO_KEY, k2 = NO_KEY;
  for (int c = ref_chunk0[r]; c < ref_chunk0[r + 1]; ++c) {
    const uint64_t* p = partial + 2 * ((size_t)c * nq_pad + q);
    top2_merge(k1, k2, p[0], p[1]);
  }
  const size_t o = (size_t)r * nq + q;
  const int j1 = k1 == NO_KEY ? -1 : (int)(uint32_t)k1, j2 = k2 == NO_KEY ? -1 : (int)(uint32_t)k2;
  if (best_idx) best_idx[o] = j1;
  if (best_dist) best_dist[o] = j1 < 0 ? INFINITY : key_distance(kind, k1);
  if (second_idx) second_idx[o] = j2;
  if (second_dist) second_dist[o] = j2 < 0 ? INFINITY : key_distance(kind, k2);
  if (mutual) mutual[o] = (colbest && j1 >= 0 && (uint32_t)colbest[r][j1] == (uint32_t)q) ? 1 : 0;
}

__global__ void fill_u64_kernel(uint64_t* p, size_t n, uint64_t v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// Conversion of an uploaded set: exact L2 -> bf16 [n_pad][dp] + int norms; general L2 -> f32 [n_pad][dp];
// Hamming -> the bytes zero-padded to dp uint32 words per row.  Padding rows / columns are zero.
__global__ void desc_convert_kernel(int kind, int n, int n_pad, int dim, int dp, int is_u8, const void* __restrict__ raw,
                                    uint16_t* __restrict__ bf, int* __restrict__ norm, float* __restrict__ f32, uint32_t* __restrict__ words) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const uint8_t* u8 = reinterpret_cast<const uint8_t*>(raw) + (size_t)row * dim;
  const float* fp = reinterpret_cast<const float*>(raw) + (size_t)row * dim;
  if (kind == KIND_HAMMING) {
    for (int wi = tid; wi < dp; wi += blockDim.x) {
      uint32_t v = 0;
      if (row < n)
        for (int b = 0; b < 4; ++b) {
          const int k = 4 * wi + b;
          if (k < dim) v |= (uint32_t)u8[k] << (8 * b);
        }
      words[(size_t)row * dp + wi] = v;
    }
    return;
  }
  __shared__ int red[256];
  int acc = 0;
  for (int k = tid; k < dp; k += blockDim.x) {
    float v = 0.f;
    if (row < n && k < dim) v = is_u8 ? (float)u8[k] : fp[k];
    if (kind == KIND_EXACT) {
      bf[(size_t)row * dp + k] = (uint16_t)(__float_as_uint(v) >> 16);   // exact: integers below 2^8 have <= 8 significant bits
      acc += (int)v * (int)v;
    } else {
      f32[(size_t)row * dp + k] = v;
    }
  }
  if (kind != KIND_EXACT) return;
  red[tid] = acc;
  __syncthreads();
  for (int st = blockDim.x / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0 && row < n) norm[row] = red[0];
}

}  // namespace

struct sfm_desc_set {
  int metric, n, dim, dtype, kind, n_pad, dp;
  uint16_t* bf = nullptr;
  int* norm = nullptr;
  float* f32 = nullptr;
  uint32_t* words = nullptr;
  int64_t upload_bytes = 0;
};

namespace {

int set_kind(const sfm_desc_set* s, bool all_exact) {
  if (s->metric == SFM_MATCH_HAMMING) return KIND_HAMMING;
  return all_exact ? KIND_EXACT : KIND_FLOAT;
}

// An exact set matched together with a non-exact one (general L2) needs an f32 image of row stride dim, like the
// non-exact sets have; it is made once, on demand, from the bf16 image (whose values are exact).
__global__ void bf16_to_f32_kernel(int n_pad, int dim, int dp, const uint16_t* __restrict__ bf, float* __restrict__ f32) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n_pad * dim) return;
  const size_t row = i / dim, k = i % dim;
  f32[i] = __uint_as_float((uint32_t)bf[row * dp + k] << 16);
}

int ensure_f32(sfm_desc_set* s, hipStream_t st) {
  if (s->f32) return SFM_OK;
  const size_t cnt = (size_t)s->n_pad * s->dim;
  SFM_HIP(hipMalloc(reinterpret_cast<void**>(&s->f32), cnt * sizeof(float) + 16));
  bf16_to_f32_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, st>>>(s->n_pad, s->dim, s->dp, s->bf, s->f32);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace

using namespace sfm;

extern "C" {

int sfm_desc_create(int metric, int n, int dim, int dtype, const void* data, sfm_desc_set** out) {
  SFM_TRY(ensure_init());
  if (!out) { set_error("sfm_desc_create: out is NULL"); return SFM_E_SHAPE; }
  *out = nullptr;
  if (metric != SFM_MATCH_L2 && metric != SFM_MATCH_HAMMING) { set_error("sfm_desc_create: unknown metric %d", metric); return SFM_E_SHAPE; }
  if (dtype != SFM_DESC_U8 && dtype != SFM_DESC_F32) { set_error("sfm_desc_create: unknown dtype %d", dtype); return SFM_E_SHAPE; }
  if (metric == SFM_MATCH_HAMMING && dtype != SFM_DESC_U8) { set_error("sfm_desc_create: Hamming needs uint8 rows"); return SFM_E_SHAPE; }
  if (n < 0 || dim < 1 || (n > 0 && !data)) { set_error("sfm_desc_create: bad sizes n=%d dim=%d", n, dim); return SFM_E_SHAPE; }
  if (metric == SFM_MATCH_L2 && dim > MAX_L2_DIM) { set_error("sfm_desc_create: L2 dim %d > %d", dim, MAX_L2_DIM); return SFM_E_SHAPE; }
  if (metric == SFM_MATCH_HAMMING && dim > 4 * MAX_HAMMING_WORDS) {
    set_error("sfm_desc_create: Hamming row of %d bytes > %d", dim, 4 * MAX_HAMMING_WORDS);
    return SFM_E_SHAPE;
  }
  bool exact = metric == SFM_MATCH_L2;
  if (exact && dtype == SFM_DESC_F32) {            // integer-valued in [0, 255]?
    const float* f = static_cast<const float*>(data);
    for (size_t i = 0, cnt = (size_t)n * dim; i < cnt && exact; ++i)
      exact = f[i] >= 0.f && f[i] <= 255.f && f[i] == floorf(f[i]);
  }
  sfm_desc_set* s = new sfm_desc_set();
  s->metric = metric; s->n = n; s->dim = dim; s->dtype = dtype;
  s->kind = metric == SFM_MATCH_HAMMING ? KIND_HAMMING : (exact ? KIND_EXACT : KIND_FLOAT);
  s->n_pad = ((n + ROW_PAD - 1) / ROW_PAD) * ROW_PAD;
  if (s->n_pad == 0) s->n_pad = ROW_PAD;
  s->dp = s->kind == KIND_HAMMING ? (dim + 3) / 4 : (s->kind == KIND_EXACT ? (dim <= 128 ? 128 : 256) : dim);
  hipStream_t st = ctx().stream;
  const size_t raw_bytes = (size_t)n * dim * (dtype == SFM_DESC_U8 ? 1 : 4);
  const size_t cells = (size_t)s->n_pad * s->dp;
  int rc = SFM_OK;
  void* d_raw = nullptr;
  hipError_t e = hipSuccess;
  if (s->kind == KIND_EXACT) {
    e = hipMalloc(reinterpret_cast<void**>(&s->bf), cells * 2 + 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->norm), sizeof(int) * (size_t)s->n_pad);
  } else if (s->kind == KIND_FLOAT) {
    e = hipMalloc(reinterpret_cast<void**>(&s->f32), cells * 4 + 16);
  } else {
    e = hipMalloc(reinterpret_cast<void**>(&s->words), cells * 4 + 16);
  }
  if (e == hipSuccess && raw_bytes) e = hipMalloc(&d_raw, raw_bytes);
  if (e == hipSuccess && raw_bytes) e = hipMemcpyAsync(d_raw, data, raw_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    desc_convert_kernel<<<s->n_pad, 256, 0, st>>>(s->kind, n, s->n_pad, dim, s->dp, dtype == SFM_DESC_U8, d_raw, s->bf, s->norm, s->f32, s->words);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (d_raw) (void)hipFree(d_raw);
  if (e != hipSuccess) {
    rc = hip_fail(e, "sfm_desc_create", __LINE__);
    sfm_desc_destroy(s);
    return rc;
  }
  s->upload_bytes = (int64_t)raw_bytes;
  *out = s;
  return SFM_OK;
}

int sfm_desc_destroy(sfm_desc_set* s) {
  if (!s) return SFM_E_HANDLE;
  if (s->bf) (void)hipFree(s->bf);
  if (s->norm) (void)hipFree(s->norm);
  if (s->f32) (void)hipFree(s->f32);
  if (s->words) (void)hipFree(s->words);
  delete s;
  return SFM_OK;
}

int sfm_desc_info(const sfm_desc_set* s, int what, int64_t* value) {
  if (!s) return SFM_E_HANDLE;
  if (!value) return SFM_E_SHAPE;
  switch (what) {
    case SFM_DESC_INFO_N: *value = s->n; return SFM_OK;
    case SFM_DESC_INFO_DIM: *value = s->dim; return SFM_OK;
    case SFM_DESC_INFO_EXACT: *value = s->kind == KIND_EXACT; return SFM_OK;
    case SFM_DESC_INFO_UPLOAD_BYTES: *value = s->upload_bytes; return SFM_OK;
    default: set_error("sfm_desc_info: unknown item %d", what); return SFM_E_SHAPE;
  }
}

int sfm_match_dev(sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, int mode, int* d_best_idx, float* d_best_dist,
                  int* d_second_idx, float* d_second_dist, uint8_t* d_mutual, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!query) return SFM_E_HANDLE;
  if (n_refs < 0 || (n_refs > 0 && !refs)) { set_error("sfm_match: bad reference list"); return SFM_E_SHAPE; }
  if (mode != SFM_MATCH_KNN2 && mode != SFM_MATCH_NN1 && mode != SFM_MATCH_MUTUAL) { set_error("sfm_match: unknown mode %d", mode); return SFM_E_SHAPE; }
  bool all_exact = query->kind == KIND_EXACT;
  for (int r = 0; r < n_refs; ++r) {
    if (!refs[r]) return SFM_E_HANDLE;
    if (refs[r]->metric != query->metric) { set_error("sfm_match: reference %d has another metric", r); return SFM_E_SHAPE; }
    if (refs[r]->dim != query->dim) { set_error("sfm_match: reference %d has dim %d, the query %d", r, refs[r]->dim, query->dim); return SFM_E_SHAPE; }
    if (refs[r]->n < 1) { set_error("sfm_match: reference %d has no descriptors", r); return SFM_E_SHAPE; }
    all_exact = all_exact && refs[r]->kind == KIND_EXACT;
  }
  const int nq = query->n;
  if (nq == 0 || n_refs == 0) return SFM_OK;
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx().stream;
  const int kind = set_kind(query, all_exact);
  if (kind == KIND_FLOAT) {
    SFM_TRY(ensure_f32(query, st));
    for (int r = 0; r < n_refs; ++r) SFM_TRY(ensure_f32(refs[r], st));
  }
  std::vector<RefSeg> segs(n_refs);
  std::vector<int4> chunks;
  std::vector<int> chunk0(n_refs + 1, 0);
  for (int r = 0; r < n_refs; ++r) {
    const sfm_desc_set* s = refs[r];
    segs[r] = RefSeg{s->bf, s->norm, s->f32, s->words, s->n, kind == KIND_FLOAT ? s->dim : s->dp};
    chunk0[r] = (int)chunks.size();
    for (int t = 0; t < s->n; t += CHUNK) chunks.push_back(make_int4(r, t, t + CHUNK < s->n ? t + CHUNK : s->n, 0));
  }
  chunk0[n_refs] = (int)chunks.size();
  const int n_chunks = (int)chunks.size();
  const size_t nq_pad = (size_t)query->n_pad;
  DevBuf<RefSeg> d_segs;
  DevBuf<int4> d_chunks;
  DevBuf<int> d_chunk0;
  DevBuf<uint64_t> d_partial, d_col;
  DevBuf<uint64_t*> d_colptr;
  SFM_TRY(d_segs.upload(segs.data(), segs.size(), st));
  SFM_TRY(d_chunks.upload(chunks.data(), chunks.size(), st));
  SFM_TRY(d_chunk0.upload(chunk0.data(), chunk0.size(), st));
  SFM_TRY(d_partial.alloc(2 * (size_t)n_chunks * nq_pad, st));
  const bool mutual = mode == SFM_MATCH_MUTUAL;
  uint64_t** colptr = nullptr;
  if (mutual) {
    size_t total = 0;
    for (int r = 0; r < n_refs; ++r) total += (size_t)refs[r]->n;
    SFM_TRY(d_col.alloc(total, st));
    fill_u64_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(d_col.p, total, NO_KEY);
    std::vector<uint64_t*> ptrs(n_refs);
    size_t off = 0;
    for (int r = 0; r < n_refs; ++r) { ptrs[r] = d_col.p + off; off += (size_t)refs[r]->n; }
    SFM_TRY(d_colptr.upload(ptrs.data(), ptrs.size(), st));
    colptr = d_colptr.p;
  }
  if (kind == KIND_EXACT) {
    const dim3 grid((unsigned)(nq_pad / MFMA_ROWS), (unsigned)n_chunks);
    if (query->dp == 128) {
      if (mutual) match_l2_mfma_kernel<4, true><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, d_segs.p, d_chunks.p, d_partial.p, (int)nq_pad, colptr);
      else match_l2_mfma_kernel<4, false><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, d_segs.p, d_chunks.p, d_partial.p, (int)nq_pad, colptr);
    } else {
      if (mutual) match_l2_mfma_kernel<8, true><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, d_segs.p, d_chunks.p, d_partial.p, (int)nq_pad, colptr);
      else match_l2_mfma_kernel<8, false><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, d_segs.p, d_chunks.p, d_partial.p, (int)nq_pad, colptr);
    }
  } else {
    const dim3 grid((unsigned)((nq + SIMT_ROWS - 1) / SIMT_ROWS), (unsigned)n_chunks);
    const int w = kind == KIND_HAMMING ? query->dp : query->dim;      // uint32 words / floats per row
    const void* qrows = kind == KIND_HAMMING ? static_cast<const void*>(query->words) : static_cast<const void*>(query->f32);
#define SFM_SIMT(K, W)                                                                                                            \
  do {                                                                                                                            \
    if (mutual) match_simt_kernel<K, W, true><<<grid, 256, 0, st>>>(qrows, nq, w, d_segs.p, d_chunks.p, d_partial.p, (int)nq_pad, colptr); \
    else match_simt_kernel<K, W, false><<<grid, 256, 0, st>>>(qrows, nq, w, d_segs.p, d_chunks.p, d_partial.p, (int)nq_pad, colptr);      \
  } while (0)
    if (kind == KIND_HAMMING) {
      if (w <= 8) SFM_SIMT(KIND_HAMMING, 8);
      else if (w <= 16) SFM_SIMT(KIND_HAMMING, 16);
      else SFM_SIMT(KIND_HAMMING, MAX_HAMMING_WORDS);
    } else {
      if (w <= 32) SFM_SIMT(KIND_FLOAT, 32);
      else if (w <= 128) SFM_SIMT(KIND_FLOAT, 128);
      else SFM_SIMT(KIND_FLOAT, MAX_L2_DIM);
    }
#undef SFM_SIMT
  }
  SFM_HIP(hipGetLastError());
  match_merge_kernel<<<dim3((unsigned)((nq + 255) / 256), (unsigned)n_refs), 256, 0, st>>>(
      kind, nq, n_refs, d_chunk0.p, d_partial.p, (int)nq_pad, colptr, d_best_idx, d_best_dist, d_second_idx, d_second_dist,
      mutual ? d_mutual : nullptr);
  SFM_HIP(hipGetLastError());
  if (!mutual && d_mutual) SFM_HIP(hipMemsetAsync(d_mutual, 0, (size_t)n_refs * nq, st));
  return SFM_OK;
}

int sfm_match(sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, int mode, int* best_idx, float* best_dist,
              int* second_idx, float* second_dist, uint8_t* mutual) {
  SFM_TRY(ensure_init());
  if (!query) return SFM_E_HANDLE;
  const size_t pairs = (size_t)(n_refs > 0 ? n_refs : 0) * (size_t)query->n;
  hipStream_t st = ctx().stream;
  HostOut<int> obi, osi;
  HostOut<float> obd, osd;
  HostOut<uint8_t> om;
  SFM_TRY(obi.want(best_idx, pairs, st)); SFM_TRY(obd.want(best_dist, pairs, st)); SFM_TRY(osi.want(second_idx, pairs, st));
  SFM_TRY(osd.want(second_dist, pairs, st)); SFM_TRY(om.want(mutual, pairs, st));
  SFM_TRY(sfm_match_dev(query, n_refs, refs, mode, obi.dev(), obd.dev(), osi.dev(), osd.dev(), om.dev(), st));
  SFM_TRY(obi.fetch(st)); SFM_TRY(obd.fetch(st)); SFM_TRY(osi.fetch(st)); SFM_TRY(osd.fetch(st)); SFM_TRY(om.fetch(st));
  return stream_sync(st);
}

}  // extern "C"
