// sfm_scan.h — the one-workgroup exclusive prefix sum every "count, scan, fill" chain of the library runs through
// ("Shared primitives").
#pragma once

#include <hip/hip_runtime.h>

namespace sfm {

constexpr int kScanBlock = 1024;      // threads of the workgroup that calls block_exclusive_scan

// Exclusive prefix sums of K integer sequences of length n in one pass, by ONE workgroup of kScanBlock threads: an
// inclusive scan inside a wave (__shfl_up), the wave totals through LDS, a running total carried from chunk to chunk.
//   load(q, int (&a)[K])           the K elements at q, called for q < n (a comes in as zeros)
//   store(q, const int (&e)[K])    the exclusive prefixes at q, called for q < n
//   total(const int (&t)[K])       the K totals, called by thread 0 after the last chunk
template <int K, class Load, class Store, class Total>
__device__ __forceinline__ void block_exclusive_scan(int n, Load load, Store store, Total total) {
  constexpr int kWaves = kScanBlock / 64;
  __shared__ int wsum[K][kWaves];
  __shared__ int carry[K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < K) carry[tid] = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kScanBlock) {
    const int q = base + tid;
    int a[K], s[K], o[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0;
    if (q < n) load(q, a);
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = a[k];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {             // inclusive scan inside the wave
      int t[K];
#pragma unroll
      for (int k = 0; k < K; ++k) t[k] = __shfl_up(s[k], off, 64);
      if (lane >= off) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += t[k];
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < K; ++k) wsum[k][wave] = s[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = carry[k];
    for (int w = 0; w < wave; ++w) {
#pragma unroll
      for (int k = 0; k < K; ++k) o[k] += wsum[k][w];
    }
    if (q < n) {
      int e[K];
#pragma unroll
      for (int k = 0; k < K; ++k) e[k] = o[k] + s[k] - a[k];
      store(q, e);
    }
    __syncthreads();
    if (tid == kScanBlock - 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) carry[k] = o[k] + s[k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    int t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = carry[k];
    total(t);
  }
}

}  // namespace sfm
