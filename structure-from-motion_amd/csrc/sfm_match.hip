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
//
// Guided matching (sfm_match_guided*): the same kernels with a compile-time gate, the inlier test of a verified
// two-view model (twoview_inlier / homography_inlier of sfm_obs_test.h) on the key coordinates of the pair.  A
// workgroup works on one chunk of one reference view, so the model is workgroup-uniform (scalar loads); the selection
// and the column-best update take `valid && admitted`, nothing else changes.  The test is called as the one function
// it is: what depends on one key only is loop-invariant and the compiler hoists it, contraction is off in the
// function, so the decisions are its decisions.  One launch per gate present in the call, over that gate's chunks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "sfm_common.h"
#include "sfm_desc.h"

namespace {

constexpr int CHUNK = 1024;        // train columns per workgroup
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

struct GateRef {                    // one gated reference view: its key coordinates and its model
  const double* x;                  // [n]
  const double* y;                  // [n]
  double m[18];                     // fundamental: F in m[0..8]; homography: (H, adj H)
};

// What a gated kernel gets beside the ungated arguments; the ungated instantiation gets the empty GateArgs<0>.
template <int GATE>
struct GateArgs {
  const double* qx;                 // [nq] query key coordinates
  const double* qy;
  const GateRef* refs;              // [n_refs]
  double max_err2;
  int* n_adm;                       // [chunks of this launch][nq_pad] admitted train keys per query, or NULL
};
template <>
struct GateArgs<SFM_GUIDE_NONE> {};

// the reference key (xt, yt) is left, the query key (xq, yq) right; defined below the kernels, past the contraction
// pragma of sfm_obs_test.h
template <int GATE>
__device__ __forceinline__ bool gate_admits(const double* m, double xt, double yt, double xq, double yq, double max_err2);

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
template <int KS, bool MUTUAL, int GATE>
__global__ __launch_bounds__(256) void match_l2_mfma_kernel(const uint16_t* __restrict__ q_bf, const int* __restrict__ q_norm, int nq,
                                                            const RefSeg* __restrict__ segs, const int4* __restrict__ chunks,
                                                            uint64_t* __restrict__ partial, int nq_pad,
                                                            uint64_t* const* __restrict__ colbest, const GateArgs<GATE> gate) {
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
  // gate: the lane's eight query keys in registers, the model at a workgroup-uniform address, the train key per tile
  double gqx[2][4], gqy[2][4];
  int n_adm[2][4];
  const GateRef* gref = nullptr;
  if constexpr (GATE != SFM_GUIDE_NONE) {
    gref = gate.refs + ch.x;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + 16 * s + 4 * h + r;
        gqx[s][r] = q < nq ? gate.qx[q] : 0.0;
        gqy[s][r] = q < nq ? gate.qy[q] : 0.0;
        n_adm[s][r] = 0;
      }
  }
  for (int t = ch.y; t < ch.z; t += 16) {
    const int col = t + r16;                          // < n_pad: the rows of the image are padded to 128
    const bool valid = col < ch.z;
    bool adm[2][4];
    if constexpr (GATE != SFM_GUIDE_NONE) {
      // gate first.  Under a homography a tile none of whose 32 x 16 pairs is admitted -- nearly every tile -- has
      // nothing to select and no column best to offer, so the wave leaves out its loads and MFMAs (wave-uniform; no
      // result changes; measured -23 %).  Under a fundamental matrix no tile is empty (2 % of the pairs are admitted)
      // and the branch cost 3 %: it is compiled out.
      const double gtx = valid ? gref->x[col] : 0.0, gty = valid ? gref->y[col] : 0.0;
      bool any = false;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          adm[s][r] = valid && gate_admits<GATE>(gref->m, gtx, gty, gqx[s][r], gqy[s][r], gate.max_err2);
          n_adm[s][r] += adm[s][r] ? 1 : 0;
          any = any || adm[s][r];
        }
      if constexpr (GATE == SFM_GUIDE_HOMOGRAPHY) {
        if (__ballot(any) == 0) continue;
      }
    }
    bf16x8 b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const bf16x8*>(seg.bf + (size_t)col * DP + ks * 32 + 8 * h);
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
        bool ok = valid;
        if constexpr (GATE != SFM_GUIDE_NONE) ok = adm[s][r];
        if (ok) top2_insert(k1[s][r], k2[s][r], ((uint64_t)sv << 32) | (uint32_t)col);
        const int q = q0 + 16 * s + 4 * h + r;
        if (MUTUAL && ok && q < nq) cbest = min_u64(cbest, ((uint64_t)sv << 32) | (uint32_t)q);
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
      if constexpr (GATE != SFM_GUIDE_NONE) {
        if (gate.n_adm) {                             // kernel argument: uniform
          int c = n_adm[s][r];
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) c += __shfl_xor(c, m, 64);
          if (r16 == 0 && q < nq) gate.n_adm[(size_t)blockIdx.y * nq_pad + q] = c;
        }
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
template <int KIND, int MAXW, bool MUTUAL, int GATE>
__global__ __launch_bounds__(256) void match_simt_kernel(const void* __restrict__ q_rows, int nq, int w, const RefSeg* __restrict__ segs,
                                                         const int4* __restrict__ chunks, uint64_t* __restrict__ partial, int nq_pad,
                                                         uint64_t* const* __restrict__ colbest, const GateArgs<GATE> gate) {
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
  double gqx = 0.0, gqy = 0.0;
  int n_adm = 0;
  const GateRef* gref = nullptr;
  if constexpr (GATE != SFM_GUIDE_NONE) {
    gref = gate.refs + ch.x;
    gqx = live ? gate.qx[q] : 0.0;
    gqy = live ? gate.qy[q] : 0.0;
  }
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
    bool ok = live;
    if constexpr (GATE != SFM_GUIDE_NONE) {             // the train key is the same address for every lane
      ok = live && gate_admits<GATE>(gref->m, gref->x[t], gref->y[t], gqx, gqy, gate.max_err2);
      n_adm += ok ? 1 : 0;
    }
    if (ok) top2_insert(k1, k2, key);
    if (MUTUAL) {
      uint64_t cb = ok ? (((uint64_t)v << 32) | (uint32_t)q) : NO_KEY;
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) cb = min_u64(cb, shfl_xor_u64(cb, m));
      if ((threadIdx.x & 63) == 0 && cb != NO_KEY) atomicMin(reinterpret_cast<unsigned long long*>(&col_lds[t - ch.y]), (unsigned long long)cb);
    }
  }
  if (live) {
    uint64_t* out = partial + 2 * ((size_t)blockIdx.y * nq_pad + q);
    out[0] = k1;
    out[1] = k2;
    if constexpr (GATE != SFM_GUIDE_NONE) {
      if (gate.n_adm) gate.n_adm[(size_t)blockIdx.y * nq_pad + q] = n_adm;
    }
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

// Per (reference, query): fold the partial top-2 of the reference's chunks; the mutual flag from the column bests;
// the number of admitted train keys (an ungated reference admits all of its keys).  ref_rows[r] = {first chunk, end
// chunk, gate, keys}.
__global__ void match_merge_kernel(int kind, int nq, int n_refs, const int4* __restrict__ ref_rows, const uint64_t* __restrict__ partial,
                                   int nq_pad, uint64_t* const* __restrict__ colbest, const int* __restrict__ adm_partial,
                                   int* __restrict__ best_idx, float* __restrict__ best_dist, int* __restrict__ second_idx,
                                   float* __restrict__ second_dist, uint8_t* __restrict__ mutual, int* __restrict__ n_admitted) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (q >= nq || r >= n_refs) return;
  const int4 row = ref_rows[r];
  uint64_t k1 = NO_KEY, k2 = NO_KEY;
  int adm = 0;
  for (int c = row.x; c < row.y; ++c) {
    const uint64_t* p = partial + 2 * ((size_t)c * nq_pad + q);
    top2_merge(k1, k2, p[0], p[1]);
    if (n_admitted && row.z != SFM_GUIDE_NONE) adm += adm_partial[(size_t)c * nq_pad + q];
  }
  const size_t o = (size_t)r * nq + q;
  if (n_admitted) n_admitted[o] = row.z != SFM_GUIDE_NONE ? adm : row.w;
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

// Below the kernels, which keep the compiler's default contraction: the header switches it off for the rest of the file.
#include "sfm_obs_test.h"

namespace {

template <>
__device__ __forceinline__ bool gate_admits<SFM_GUIDE_FUNDAMENTAL>(const double* m, double xt, double yt, double xq, double yq, double max_err2) {
  return sfm::twoview_inlier(m, xt, yt, xq, yq, max_err2);
}

template <>
__device__ __forceinline__ bool gate_admits<SFM_GUIDE_HOMOGRAPHY>(const double* m, double xt, double yt, double xq, double yq, double max_err2) {
  return sfm::homography_inlier(m, xt, yt, xq, yq, max_err2);
}

}  // namespace

namespace {

static_assert(KIND_EXACT == sfm::kDescKindExact && KIND_HAMMING == sfm::kDescKindHamming && KIND_FLOAT == sfm::kDescKindFloat,
              "sfm_desc.h names the kinds for the other readers of a set");

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

}  // extern "C"

namespace {

// The gate of a guided call as the host frame sees it: DEVICE coordinate arrays, HOST kinds and models.
struct Guide {
  const double* d_qx;
  const double* d_qy;
  const double* const* d_rx;        // host array [n_refs] of device pointers
  const double* const* d_ry;
  const int* kind;                  // [n_refs]
  const double* model;              // [n_refs][9]
  double max_err2;
};

// What the launches of one call share.
struct MatchLaunch {
  const sfm_desc_set* query;
  int kind, nq;
  bool mutual;
  size_t nq_pad;
  const RefSeg* segs;
  const int4* chunks;
  uint64_t* partial;
  uint64_t* const* colptr;
  const double* qx;
  const double* qy;
  const GateRef* grefs;
  double max_err2;
  int* adm;
  hipStream_t st;
};

// One launch over the chunks [first, first + count) of the call's table: those of the references of one gate.
template <int GATE>
void launch_chunks(const MatchLaunch& L, int first, int count) {
  if (count == 0) return;
  GateArgs<GATE> gate;
  if constexpr (GATE != SFM_GUIDE_NONE) gate = GateArgs<GATE>{L.qx, L.qy, L.grefs, L.max_err2, L.adm ? L.adm + (size_t)first * L.nq_pad : nullptr};
  const int4* chunks = L.chunks + first;
  uint64_t* partial = L.partial + 2 * (size_t)first * L.nq_pad;
  const sfm_desc_set* query = L.query;
  const int nq = L.nq, nq_pad = (int)L.nq_pad;
  hipStream_t st = L.st;
  if (L.kind == KIND_EXACT) {
    const dim3 grid((unsigned)(L.nq_pad / MFMA_ROWS), (unsigned)count);
    if (query->dp == 128) {
      if (L.mutual) match_l2_mfma_kernel<4, true, GATE><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, L.segs, chunks, partial, nq_pad, L.colptr, gate);
      else match_l2_mfma_kernel<4, false, GATE><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, L.segs, chunks, partial, nq_pad, L.colptr, gate);
    } else {
      if (L.mutual) match_l2_mfma_kernel<8, true, GATE><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, L.segs, chunks, partial, nq_pad, L.colptr, gate);
      else match_l2_mfma_kernel<8, false, GATE><<<grid, 256, 0, st>>>(query->bf, query->norm, nq, L.segs, chunks, partial, nq_pad, L.colptr, gate);
    }
    return;
  }
  const dim3 grid((unsigned)((nq + SIMT_ROWS - 1) / SIMT_ROWS), (unsigned)count);
  const int w = L.kind == KIND_HAMMING ? query->dp : query->dim;      // uint32 words / floats per row
  const void* qrows = L.kind == KIND_HAMMING ? static_cast<const void*>(query->words) : static_cast<const void*>(query->f32);
#define SFM_SIMT(K, W)                                                                                                              \
  do {                                                                                                                              \
    if (L.mutual) match_simt_kernel<K, W, true, GATE><<<grid, 256, 0, st>>>(qrows, nq, w, L.segs, chunks, partial, nq_pad, L.colptr, gate); \
    else match_simt_kernel<K, W, false, GATE><<<grid, 256, 0, st>>>(qrows, nq, w, L.segs, chunks, partial, nq_pad, L.colptr, gate);        \
  } while (0)
  if (L.kind == KIND_HAMMING) {
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

inline int gate_of(const Guide* g, int r) { return g ? g->kind[r] : SFM_GUIDE_NONE; }

// The checks of a gate that need no device and no handle; `who` names the entry point in the message.
int check_guide(const char* who, int n_refs, const int* kind, const double* model, double max_err2) {
  if (n_refs < 0) { set_error("%s: bad reference list", who); return SFM_E_SHAPE; }
  if (!(max_err2 >= 0.0)) { set_error("%s: max_err2 %g is negative or NaN", who, max_err2); return SFM_E_SHAPE; }
  if (n_refs > 0 && (!kind || !model)) { set_error("%s: kind or model is NULL", who); return SFM_E_SHAPE; }
  for (int r = 0; r < n_refs; ++r) {
    if (kind[r] != SFM_GUIDE_NONE && kind[r] != SFM_GUIDE_FUNDAMENTAL && kind[r] != SFM_GUIDE_HOMOGRAPHY) {
      set_error("%s: reference %d has the unknown gate %d", who, r, kind[r]);
      return SFM_E_SHAPE;
    }
    if (kind[r] == SFM_GUIDE_NONE) continue;
    for (int i = 0; i < 9; ++i)
      if (!std::isfinite(model[9 * (size_t)r + i])) { set_error("%s: the model of reference %d is not finite", who, r); return SFM_E_SHAPE; }
  }
  return SFM_OK;
}

// The sets of one call fit together; *all_exact (may be NULL): every one of them takes the exact path.
int check_sets(const char* who, const sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, bool* all_exact) {
  if (n_refs < 0 || (n_refs > 0 && !refs)) { set_error("%s: bad reference list", who); return SFM_E_SHAPE; }
  bool exact = query->kind == KIND_EXACT;
  for (int r = 0; r < n_refs; ++r) {
    if (!refs[r]) return SFM_E_HANDLE;
    if (refs[r]->metric != query->metric) { set_error("%s: reference %d has another metric", who, r); return SFM_E_SHAPE; }
    if (refs[r]->dim != query->dim) { set_error("%s: reference %d has dim %d, the query %d", who, r, refs[r]->dim, query->dim); return SFM_E_SHAPE; }
    if (refs[r]->n < 1) { set_error("%s: reference %d has no descriptors", who, r); return SFM_E_SHAPE; }
    exact = exact && refs[r]->kind == KIND_EXACT;
  }
  if (all_exact) *all_exact = exact;
  return SFM_OK;
}

// sfm_match_dev (guide == NULL: no gate, no admission counts) and sfm_match_guided_dev.  Every check comes before the
// first enqueue.
int match_run(const char* who, sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, bool mutual, const Guide* guide,
              int* d_best_idx, float* d_best_dist, int* d_second_idx, float* d_second_dist, uint8_t* d_mutual, int* d_n_admitted,
              hipStream_t st) {
  bool all_exact = false;
  SFM_TRY(check_sets(who, query, n_refs, refs, &all_exact));
  const int nq = query->n;
  bool gated = false;
  for (int r = 0; r < n_refs; ++r) gated = gated || gate_of(guide, r) != SFM_GUIDE_NONE;
  if (gated && nq > 0) {
    if (!guide->d_qx || !guide->d_qy || !guide->d_rx || !guide->d_ry) { set_error("%s: a coordinate array is NULL", who); return SFM_E_SHAPE; }
    for (int r = 0; r < n_refs; ++r)
      if (gate_of(guide, r) != SFM_GUIDE_NONE && (!guide->d_rx[r] || !guide->d_ry[r])) {
        set_error("%s: reference %d has a gate and no coordinates", who, r);
        return SFM_E_SHAPE;
      }
  }
  if (nq == 0 || n_refs == 0) return SFM_OK;
  const int kind = set_kind(query, all_exact);
  if (kind == KIND_FLOAT) {
    SFM_TRY(ensure_f32(query, st));
    for (int r = 0; r < n_refs; ++r) SFM_TRY(ensure_f32(refs[r], st));
  }
  // the chunk table, the chunks of the references of one gate next to each other: one launch per gate present
  std::vector<RefSeg> segs(n_refs);
  std::vector<GateRef> grefs(gated ? n_refs : 0);
  std::vector<int4> chunks, ref_rows(n_refs);
  int gate_first[4] = {0, 0, 0, 0};
  for (int g = SFM_GUIDE_NONE; g <= SFM_GUIDE_HOMOGRAPHY; ++g) {
    gate_first[g] = (int)chunks.size();
    for (int r = 0; r < n_refs; ++r) {
      if (gate_of(guide, r) != g) continue;
      const sfm_desc_set* s = refs[r];
      segs[r] = RefSeg{s->bf, s->norm, s->f32, s->words, s->n, kind == KIND_FLOAT ? s->dim : s->dp};
      ref_rows[r].x = (int)chunks.size();
      for (int t = 0; t < s->n; t += CHUNK) chunks.push_back(make_int4(r, t, t + CHUNK < s->n ? t + CHUNK : s->n, 0));
      ref_rows[r].y = (int)chunks.size();
      ref_rows[r].z = g;
      ref_rows[r].w = s->n;
      if (!gated) continue;
      GateRef& gr = grefs[r];
      memset(&gr, 0, sizeof(gr));
      if (g == SFM_GUIDE_NONE) continue;
      gr.x = guide->d_rx[r];
      gr.y = guide->d_ry[r];
      for (int i = 0; i < 9; ++i) gr.m[i] = guide->model[9 * (size_t)r + i];
      if (g == SFM_GUIDE_HOMOGRAPHY) homography_adjugate(gr.m, gr.m + 9);
    }
  }
  gate_first[3] = (int)chunks.size();
  const int n_chunks = (int)chunks.size();
  const size_t nq_pad = (size_t)query->n_pad;
  DevBuf<RefSeg> d_segs;
  DevBuf<GateRef> d_grefs;
  DevBuf<int4> d_chunks, d_ref_rows;
  DevBuf<uint64_t> d_partial, d_col;
  DevBuf<uint64_t*> d_colptr;
  DevBuf<int> d_adm;
  SFM_TRY(d_segs.upload(segs.data(), segs.size(), st));
  SFM_TRY(d_chunks.upload(chunks.data(), chunks.size(), st));
  SFM_TRY(d_ref_rows.upload(ref_rows.data(), ref_rows.size(), st));
  SFM_TRY(d_partial.alloc(2 * (size_t)n_chunks * nq_pad, st));
  if (gated) SFM_TRY(d_grefs.upload(grefs.data(), grefs.size(), st));
  if (gated && d_n_admitted) SFM_TRY(d_adm.alloc((size_t)n_chunks * nq_pad, st));
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
  const MatchLaunch L{query, kind, nq, mutual, nq_pad, d_segs.p, d_chunks.p, d_partial.p, colptr, guide ? guide->d_qx : nullptr,
                      guide ? guide->d_qy : nullptr, d_grefs.p, guide ? guide->max_err2 : 0.0, d_adm.p, st};
  launch_chunks<SFM_GUIDE_NONE>(L, gate_first[0], gate_first[1] - gate_first[0]);
  launch_chunks<SFM_GUIDE_FUNDAMENTAL>(L, gate_first[1], gate_first[2] - gate_first[1]);
  launch_chunks<SFM_GUIDE_HOMOGRAPHY>(L, gate_first[2], gate_first[3] - gate_first[2]);
  SFM_HIP(hipGetLastError());
  match_merge_kernel<<<dim3((unsigned)((nq + 255) / 256), (unsigned)n_refs), 256, 0, st>>>(
      kind, nq, n_refs, d_ref_rows.p, d_partial.p, (int)nq_pad, colptr, d_adm.p, d_best_idx, d_best_dist, d_second_idx, d_second_dist,
      mutual ? d_mutual : nullptr, d_n_admitted);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace

extern "C" {

int sfm_match_dev(sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, int mode, int* d_best_idx, float* d_best_dist,
                  int* d_second_idx, float* d_second_dist, uint8_t* d_mutual, void* hip_stream) {
  SFM_TRY(ensure_init());
  if (!query) return SFM_E_HANDLE;
  if (n_refs < 0 || (n_refs > 0 && !refs)) { set_error("sfm_match: bad reference list"); return SFM_E_SHAPE; }
  if (mode != SFM_MATCH_KNN2 && mode != SFM_MATCH_NN1 && mode != SFM_MATCH_MUTUAL) { set_error("sfm_match: unknown mode %d", mode); return SFM_E_SHAPE; }
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx().stream;
  const bool mutual = mode == SFM_MATCH_MUTUAL;
  SFM_TRY(match_run("sfm_match", query, n_refs, refs, mutual, nullptr, d_best_idx, d_best_dist, d_second_idx, d_second_dist, d_mutual,
                    nullptr, st));
  if (!mutual && d_mutual && query->n > 0 && n_refs > 0) SFM_HIP(hipMemsetAsync(d_mutual, 0, (size_t)n_refs * query->n, st));
  return SFM_OK;
}

int sfm_match_guided_dev(sfm_desc_set* query, const double* d_qx, const double* d_qy, int n_refs, sfm_desc_set* const* refs,
                         const double* const* d_rx, const double* const* d_ry, const int* kind, const double* model, double max_err2,
                         int* d_best_idx, float* d_best_dist, int* d_second_idx, float* d_second_dist, uint8_t* d_mutual,
                         int* d_n_admitted, void* hip_stream) {
  if (!query) return SFM_E_HANDLE;
  SFM_TRY(check_guide("sfm_match_guided", n_refs, kind, model, max_err2));
  SFM_TRY(ensure_init());
  const Guide guide{d_qx, d_qy, d_rx, d_ry, kind, model, max_err2};
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx().stream;
  return match_run("sfm_match_guided", query, n_refs, refs, d_mutual != nullptr, &guide, d_best_idx, d_best_dist, d_second_idx,
                   d_second_dist, d_mutual, d_n_admitted, st);
}

int sfm_match_guided(sfm_desc_set* query, const double* qx, const double* qy, int n_refs, sfm_desc_set* const* refs,
                     const double* const* rx, const double* const* ry, const int* kind, const double* model, double max_err2,
                     int* best_idx, float* best_dist, int* second_idx, float* second_dist, uint8_t* mutual, int* n_admitted) {
  if (!query) return SFM_E_HANDLE;
  SFM_TRY(check_guide("sfm_match_guided", n_refs, kind, model, max_err2));
  SFM_TRY(ensure_init());
  SFM_TRY(check_sets("sfm_match_guided", query, n_refs, refs, nullptr));
  hipStream_t st = ctx().stream;
  // the coordinates of the query and of every gated reference go up; an ungated reference needs none
  const size_t nq = (size_t)query->n;
  bool gated = false;
  for (int r = 0; r < n_refs; ++r) gated = gated || kind[r] != SFM_GUIDE_NONE;
  DevBuf<double> d_q;
  std::vector<DevBuf<double>> d_r(n_refs);
  std::vector<const double*> prx(n_refs, nullptr), pry(n_refs, nullptr);
  if (gated && nq > 0) {
    if (!qx || !qy || !rx || !ry) { set_error("sfm_match_guided: a coordinate array is NULL"); return SFM_E_SHAPE; }
    for (int r = 0; r < n_refs; ++r) {
      if (kind[r] != SFM_GUIDE_NONE && (!rx[r] || !ry[r])) { set_error("sfm_match_guided: reference %d has a gate and no coordinates", r); return SFM_E_SHAPE; }
    }
    SFM_TRY(d_q.alloc(2 * nq, st));
    SFM_HIP(hipMemcpyAsync(d_q.p, qx, nq * sizeof(double), hipMemcpyHostToDevice, st));
    SFM_HIP(hipMemcpyAsync(d_q.p + nq, qy, nq * sizeof(double), hipMemcpyHostToDevice, st));
    for (int r = 0; r < n_refs; ++r) {
      if (kind[r] == SFM_GUIDE_NONE) continue;
      const size_t n = (size_t)refs[r]->n;
      SFM_TRY(d_r[r].alloc(2 * n, st));
      SFM_HIP(hipMemcpyAsync(d_r[r].p, rx[r], n * sizeof(double), hipMemcpyHostToDevice, st));
      SFM_HIP(hipMemcpyAsync(d_r[r].p + n, ry[r], n * sizeof(double), hipMemcpyHostToDevice, st));
      prx[r] = d_r[r].p;
      pry[r] = d_r[r].p + n;
    }
  }
  const size_t pairs = (size_t)(n_refs > 0 ? n_refs : 0) * nq;
  HostOut<int> obi, osi, oad;
  HostOut<float> obd, osd;
  HostOut<uint8_t> om;
  SFM_TRY(obi.want(best_idx, pairs, st)); SFM_TRY(obd.want(best_dist, pairs, st)); SFM_TRY(osi.want(second_idx, pairs, st));
  SFM_TRY(osd.want(second_dist, pairs, st)); SFM_TRY(om.want(mutual, pairs, st)); SFM_TRY(oad.want(n_admitted, pairs, st));
  const Guide guide{d_q.p, d_q.p ? d_q.p + nq : nullptr, prx.data(), pry.data(), kind, model, max_err2};
  SFM_TRY(match_run("sfm_match_guided", query, n_refs, refs, mutual != nullptr, &guide, obi.dev(), obd.dev(), osi.dev(), osd.dev(),
                    om.dev(), oad.dev(), st));
  SFM_TRY(obi.fetch(st)); SFM_TRY(obd.fetch(st)); SFM_TRY(osi.fetch(st)); SFM_TRY(osd.fetch(st)); SFM_TRY(om.fetch(st));
  SFM_TRY(oad.fetch(st));
  return stream_sync(st);
}

int sfm_homography_adjugate(const double H[9], double G[9]) {
  if (!H || !G) { set_error("sfm_homography_adjugate: NULL argument"); return SFM_E_SHAPE; }
  homography_adjugate(H, G);
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
