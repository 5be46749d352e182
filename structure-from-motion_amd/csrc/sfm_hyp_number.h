// sfm_hyp_number.h -- the numbering of the hypotheses of the robust operations (host and device): the pairs of a track
// (sfm_tri_ransac.hip) and the triples of a camera's observations (sfm_resect.hip), both in lexicographic order, all of
// them up to max_hyp, else evenly spaced.  No random number anywhere.  The floating-point estimates below only seed integer
// searches that end at the exact answer, so the results do not depend on how the including file contracts them.
// The eight-match samples of the robust two-view geometry (sfm_twoview.hip), the four-match samples of the robust
// homography (sfm_homography.hip), the five-match samples of the robust essential matrix (sfm_essential.hip) and the
// three-correspondence samples of the robust similarity (sfm_similarity.hip) are drawn by a stratified integer sampler.
#pragma once

#include <cmath>

#include "sfm_common.h"

namespace sfm {

constexpr int kHypMax = 65536, kHypDefault = 128;      // the bound on max_hyp, and what max_hyp = 0 stands for

// Hypotheses of a track or camera with `total` pairs or triples: all of them up to max_hyp.
__host__ __device__ inline int hyp_count(long long total, int max_hyp) { return total < (long long)max_hyp ? (int)total : max_hyp; }

__host__ __device__ inline long long ransac_pair_count(int n) { return (long long)n * (n - 1) / 2; }

// Pair number of hypothesis h: h itself while every pair is a hypothesis, else floor(h P / max_hyp) -- split as
// h (P / max_hyp) + floor(h (P % max_hyp) / max_hyp), which is the same integer and stays below 2^63.
__host__ __device__ inline long long ransac_pair_number(long long P, int max_hyp, int h) {
  if (P <= max_hyp) return h;
  return (long long)h * (P / max_hyp) + (long long)h * (P % max_hyp) / max_hyp;
}

// Pair k of the n (n - 1) / 2 pairs (i < j) in lexicographic order: r (2 n - r - 1) / 2 pairs precede row r.  The square
// root gives the row to within a few units (its argument exceeds 2^53 for long tracks); the two loops make it exact.
__host__ __device__ inline void ransac_pair_of(int n, long long k, int* i, int* j) {
  const double b = 2.0 * n - 1.0;
  long long r = (long long)((b - sqrt(fmax(b * b - 8.0 * (double)k, 0.0))) * 0.5);
  r = r < 0 ? 0 : (r > n - 2 ? n - 2 : r);
  while (r > 0 && r * (2LL * n - r - 1) / 2 > k) --r;
  while (r < n - 2 && (r + 1) * (2LL * n - r - 2) / 2 <= k) ++r;
  *i = (int)r;
  *j = (int)(r + 1 + (k - r * (2LL * n - r - 1) / 2));
}

// ---- triples: n <= 2^20, so that T = n (n - 1) (n - 2) / 6 and the product before the division stay below 2^63 ----
constexpr int kTripleMaxObs = 1 << 20;
__host__ __device__ inline long long triple_count(long long n) { return n * (n - 1) * (n - 2) / 6; }

// Triple k of the T triples (i < j < l) in lexicographic order: T - C(n - i, 3) triples precede first index i, and inside
// it the pairs (j, l) of the n - i - 1 later observations follow in ransac_pair_of's order.  The cube root gives n - i to
// within a few units; the two loops make it exact.
__host__ __device__ inline void triple_of(int n, long long k, int* i, int* j, int* l) {
  const long long T = triple_count(n), rem = T - k;                  // triples from k on: C(n - i, 3) >= rem > C(n - i - 1, 3)
  long long m = (long long)cbrt(6.0 * (double)rem) + 1;
  m = m < 3 ? 3 : (m > n ? n : m);
  while (m > 3 && triple_count(m - 1) >= rem) --m;
  while (m < n && triple_count(m) < rem) ++m;
  const int first = (int)(n - m);
  int r, s;
  ransac_pair_of((int)(m - 1), k - (T - triple_count(m)), &r, &s);
  *i = first;
  *j = first + 1 + r;
  *l = first + 1 + s;
}

// ---- eight-index samples of a set of matches (sfm_twoview.hip): C(n, 8) passes 2^63 near n = 2 000, so the 8-subsets are
// not numbered; a stratified integer sampler takes their place.  Stratum k of a set of n >= 9 matches is
// floor(k n / 8) .. floor((k + 1) n / 8) - 1 (never empty); hypothesis h takes from it the match
// lo_k + mix(8 h + k) mod (hi_k - lo_k), mix being the splitmix64 finaliser: no state, no floating point, eight distinct
// ascending indices.
__host__ __device__ inline unsigned long long splitmix64_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

__host__ __device__ inline int twoview_sample_index(int n, int h, int k) {
  const long long lo = (long long)k * n / 8, hi = (long long)(k + 1) * n / 8;
  return (int)(lo + (long long)(splitmix64_mix(8ULL * (unsigned long long)h + (unsigned long long)k) % (unsigned long long)(hi - lo)));
}

// ---- four-index samples of a set of n >= 5 matches (sfm_homography.hip): the same sampler over quarters, stratum k being
// floor(k n / 4) .. floor((k + 1) n / 4) - 1 (never empty) and hypothesis h taking lo_k + mix(4 h + k) mod (hi_k - lo_k).
__host__ __device__ inline int homography_sample_index(int n, int h, int k) {
  const long long lo = (long long)k * n / 4, hi = (long long)(k + 1) * n / 4;
  return (int)(lo + (long long)(splitmix64_mix(4ULL * (unsigned long long)h + (unsigned long long)k) % (unsigned long long)(hi - lo)));
}

// ---- five-index samples of a set of n >= 6 matches (sfm_essential.hip): the same sampler over fifths, stratum k being
// floor(k n / 5) .. floor((k + 1) n / 5) - 1 (never empty) and hypothesis h taking lo_k + mix(5 h + k) mod (hi_k - lo_k).
__host__ __device__ inline int essential_sample_index(int n, int h, int k) {
  const long long lo = (long long)k * n / 5, hi = (long long)(k + 1) * n / 5;
  return (int)(lo + (long long)(splitmix64_mix(5ULL * (unsigned long long)h + (unsigned long long)k) % (unsigned long long)(hi - lo)));
}

// ---- three-index samples of a set of n >= 4 correspondences (sfm_similarity.hip): the same sampler over thirds, stratum k
// being floor(k n / 3) .. floor((k + 1) n / 3) - 1 (never empty) and hypothesis h taking lo_k + mix(3 h + k) mod (hi_k - lo_k).
__host__ __device__ inline int similarity_sample_index(int n, int h, int k) {
  const long long lo = (long long)k * n / 3, hi = (long long)(k + 1) * n / 3;
  return (int)(lo + (long long)(splitmix64_mix(3ULL * (unsigned long long)h + (unsigned long long)k) % (unsigned long long)(hi - lo)));
}

}  // namespace sfm
