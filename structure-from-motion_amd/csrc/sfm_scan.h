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

// ---- the device-wide form: three launches, no workgroup waits for another one ----
// The one-workgroup scan walks n / kScanBlock dependent chunks; past some n (DESIGN.md section 39 holds the measured
// crossover) it pays to cut the sequence into tiles of kScanBlock elements, one workgroup each:
//   device_scan_tiles_kernel   tile totals -> tile_tot[k][tile]
//   device_scan_totals_kernel  ONE workgroup: exclusive scan of the tile totals in place, the K grand totals behind them
//   device_scan_apply_kernel   every tile scans itself again and stores with its tile's offset added
// Op is a small struct passed by value: n() the length (it may read device memory), load / store / total as above.
// `tiles` covers the host's bound on n(); a tile past n() has nothing to do.  Integer sums: the bits equal the
// one-workgroup route's.
template <int K, class Op>
__global__ __launch_bounds__(kScanBlock) void block_scan_kernel(Op op) {
  block_exclusive_scan<K>(
      op.n(), [&](int q, int (&a)[K]) { op.load(q, a); }, [&](int q, const int (&e)[K]) { op.store(q, e); },
      [&](const int (&t)[K]) { op.total(t); });
}

template <int K, class Op>
__global__ __launch_bounds__(kScanBlock) void device_scan_tiles_kernel(Op op, int* tile_tot, int tiles) {
  const long long base = (long long)blockIdx.x * kScanBlock, left = (long long)op.n() - base;
  const int n = left <= 0 ? 0 : (left < kScanBlock ? (int)left : kScanBlock);
  block_exclusive_scan<K>(
      n, [&](int q, int (&a)[K]) { op.load((int)base + q, a); }, [&](int, const int (&)[K]) {},
      [&](const int (&t)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) tile_tot[(size_t)k * tiles + blockIdx.x] = t[k];
      });
}

template <int K>
__global__ __launch_bounds__(kScanBlock) void device_scan_totals_kernel(int* tile_tot, int tiles) {
  block_exclusive_scan<K>(
      tiles,
      [&](int q, int (&a)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = tile_tot[(size_t)k * tiles + q];
      },
      [&](int q, const int (&e)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) tile_tot[(size_t)k * tiles + q] = e[k];
      },
      [&](const int (&t)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) tile_tot[(size_t)K * tiles + k] = t[k];
      });
}

template <int K, class Op>
__global__ __launch_bounds__(kScanBlock) void device_scan_apply_kernel(Op op, const int* tile_tot, int tiles) {
  const long long base = (long long)blockIdx.x * kScanBlock, left = (long long)op.n() - base;
  const int n = left <= 0 ? 0 : (left < kScanBlock ? (int)left : kScanBlock);
  int off[K];
#pragma unroll
  for (int k = 0; k < K; ++k) off[k] = tile_tot[(size_t)k * tiles + blockIdx.x];
  block_exclusive_scan<K>(
      n, [&](int q, int (&a)[K]) { op.load((int)base + q, a); },
      [&](int q, const int (&e)[K]) {
        int f[K];
#pragma unroll
        for (int k = 0; k < K; ++k) f[k] = e[k] + off[k];
        op.store((int)base + q, f);
      },
      [&](const int (&)[K]) {
        if (blockIdx.x != 0) return;
        int t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] = tile_tot[(size_t)K * tiles + k];
        op.total(t);
      });
}

// Host side: tile_tot holds (K + 1) * tiles ints (K <= tiles).  one_block picks the one-workgroup route.
template <int K, class Op>
inline void exclusive_scan_launch(Op op, bool one_block, int* tile_tot, int tiles, hipStream_t s) {
  if (one_block || tiles <= 1) {
    block_scan_kernel<K, Op><<<1, kScanBlock, 0, s>>>(op);
    return;
  }
  device_scan_tiles_kernel<K, Op><<<(unsigned)tiles, kScanBlock, 0, s>>>(op, tile_tot, tiles);
  device_scan_totals_kernel<K><<<1, kScanBlock, 0, s>>>(tile_tot, tiles);
  device_scan_apply_kernel<K, Op><<<(unsigned)tiles, kScanBlock, 0, s>>>(op, tile_tot, tiles);
}

}  // namespace sfm
