// host_check_retrieve.hip -- a stand-alone program around the host code of the view-pair selection that needs no device: the
// score of a pair (sfm_view_score), the start rows of the vocabulary (sfm_vocab_init_rows) and the argument path of
// sfm_vocab_train, sfm_view_describe(_dev) and sfm_view_pairs(_dev) up to, but not past, the first call that wants a GPU.
// The descriptor sets it hands over are structs with no device memory behind them: every call is refused, or stops at the
// search for a device, before one of their pointers is read.  Meant to be built with the host sanitizers and run on a
// machine without a GPU (the device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_retrieve.hip $(make -s print-srcs) -ldl -o /tmp/host_check_retrieve
//   /tmp/host_check_retrieve
// Exit status 0 and "host_check_retrieve: ok" when every check holds and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sfm_hip.h"
#include "../structure-from-motion_amd/csrc/sfm_desc.h"

static int failures = 0;

#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static unsigned long long mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

static sfm_desc_set fake(int n, int dim, int metric = SFM_MATCH_L2, int kind = sfm::kDescKindExact) {
  sfm_desc_set s;
  s.metric = metric; s.n = n; s.dim = dim; s.dtype = SFM_DESC_U8; s.kind = kind;
  s.n_pad = n > 0 ? (n + 127) / 128 * 128 : 128;
  s.dp = dim <= 128 ? 128 : 256;
  return s;
}

static bool says(const char* word) { return std::strstr(sfm_last_error(), word) != nullptr; }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  EXPECT(sfm_version() >= 112);

  // ---- the score: dot / sqrt(na nb) in three operations
  {
    double s = -9;
    EXPECT(sfm_view_score(7, 49, 1, &s) == SFM_OK && s == 1.0);
    EXPECT(sfm_view_score(-7, 7, 7, &s) == SFM_OK && s == -1.0);
    EXPECT(sfm_view_score(0, 3, 5, &s) == SFM_OK && s == 0.0 && !std::signbit(s));
    const int64_t big = 127LL * 127 * 131072;
    EXPECT(sfm_view_score((int)big, big, big, &s) == SFM_OK && s == 1.0);
    EXPECT(sfm_view_score(-(int)big, big, big, &s) == SFM_OK && s == -1.0);
    for (int dot = -40; dot <= 40; dot += 7)
      for (int64_t na = 1; na < 2000; na += 131)
        for (int64_t nb = 3; nb < (1LL << 31); nb = nb * 37 + 1) {
          const double p = (double)na * (double)nb;
          const double want = (double)dot / std::sqrt(p);
          EXPECT(sfm_view_score(dot, na, nb, &s) == SFM_OK && std::memcmp(&s, &want, 8) == 0);
        }
    EXPECT(sfm_view_score(1, 1, 1, nullptr) == SFM_E_SHAPE);
  }

  // ---- the start rows: stratified, distinct, ascending; the capped form maps training rows to rows of the concatenation
  {
    std::vector<int64_t> rows(1024, -7);
    const long long Ns[] = {1, 17, 1000, 2500, (1LL << 20) + 3, (1LL << 38)};
    for (long long N : Ns)
      for (int K : {1, 2, 15, 17, 1024})
        for (long long cap : {0LL, 1000LL, 1LL << 22})
          for (unsigned long long seed : {0ULL, 1ULL, 1ULL << 63, ~0ULL}) {
            const long long limit = cap == 0 ? (1LL << 20) : cap, T = N <= limit ? N : limit;
            std::fill(rows.begin(), rows.end(), -7);
            const int rc = sfm_vocab_init_rows(N, K, seed, cap, rows.data());
            if (T < K) { EXPECT(rc == SFM_E_SHAPE && rows[0] == -7); continue; }
            EXPECT(rc == SFM_OK);
            for (int w = 0; w < K; ++w) {
              const long long lo = (long long)w * T / K, hi = (long long)(w + 1) * T / K;
              const long long t = lo + (long long)(mix(seed * (unsigned long long)K + (unsigned long long)w) % (unsigned long long)(hi - lo));
              const long long g = T == N ? t : (long long)((__int128)t * N / T);
              EXPECT(rows[w] == g && g >= 0 && g < N && (w == 0 || rows[w] > rows[w - 1]));
            }
            EXPECT(K == 1024 || rows[K] == -7);
          }
    EXPECT(sfm_vocab_init_rows(100, 0, 1, 0, rows.data()) == SFM_E_SHAPE && sfm_vocab_init_rows(100, 1025, 1, 0, rows.data()) == SFM_E_SHAPE);
    EXPECT(sfm_vocab_init_rows(100, 4, 1, -1, rows.data()) == SFM_E_SHAPE && sfm_vocab_init_rows(100, 4, 1, (1LL << 22) + 1, rows.data()) == SFM_E_SHAPE);
    EXPECT(sfm_vocab_init_rows(-1, 4, 1, 0, rows.data()) == SFM_E_SHAPE && sfm_vocab_init_rows(100, 4, 1, 0, nullptr) == SFM_E_SHAPE);
  }

  // ---- training: the argument path
  sfm_desc_set a = fake(300, 128), empty = fake(0, 128), b = fake(200, 128), ham = fake(50, 128, SFM_MATCH_HAMMING, sfm::kDescKindHamming);
  sfm_desc_set flt = fake(50, 128, SFM_MATCH_L2, sfm::kDescKindFloat), narrow = fake(50, 64), wide = fake(2000, 256), huge = fake((1 << 22) + 1, 128);
  std::vector<uint8_t> words(1024 * 256, 7);
  std::vector<int64_t> log(3 * 66, -7);
  auto train = [&](std::vector<sfm_desc_set*> sets, int K, int iters, long long cap) {
    return sfm_vocab_train((int)sets.size(), sets.data(), K, iters, 1, cap, words.data(), log.data());
  };
  EXPECT(train({&a, &empty, &b}, 0, 4, 0) == SFM_E_SHAPE && says("K = 0"));
  EXPECT(train({&a, &empty, &b}, 1025, 4, 0) == SFM_E_SHAPE && says("K = 1025"));
  EXPECT(train({&a}, 8, -1, 0) == SFM_E_SHAPE && train({&a}, 8, 65, 0) == SFM_E_SHAPE && says("iters"));
  EXPECT(train({&a}, 8, 4, -1) == SFM_E_SHAPE && train({&a}, 8, 4, (1LL << 22) + 1) == SFM_E_SHAPE && says("train_cap"));
  EXPECT(train({}, 8, 4, 0) == SFM_E_SHAPE && says("0 sets"));
  EXPECT(sfm_vocab_train(2, nullptr, 8, 4, 1, 0, words.data(), log.data()) == SFM_E_SHAPE && says("null"));
  EXPECT(train({&a, nullptr}, 8, 4, 0) == SFM_E_SHAPE && says("set 1 is null"));
  EXPECT(train({&a, &ham}, 8, 4, 0) == SFM_E_SHAPE && says("set 1 is not an exact L2 set"));
  EXPECT(train({&flt, &a}, 8, 4, 0) == SFM_E_SHAPE && says("set 0 is not an exact L2 set"));
  EXPECT(train({&a, &narrow}, 8, 4, 0) == SFM_E_SHAPE && says("set 1 has dim 64"));
  EXPECT(train({&wide}, 513, 4, 0) == SFM_E_SHAPE && says("K * D = 131328"));
  EXPECT(train({&huge}, 8, 4, 0) == SFM_E_SHAPE && says("at most 2^22"));
  EXPECT(train({&a, &empty, &b}, 501, 4, 0) == SFM_E_SHAPE && says("T = 500 training rows for K = 501"));
  EXPECT(train({&a, &empty, &b}, 300, 4, 299) == SFM_E_SHAPE && says("T = 299"));
  {
    sfm_desc_set* one[1] = {&a};
    EXPECT(sfm_vocab_train(1, one, 8, 4, 1, 0, nullptr, log.data()) == SFM_E_SHAPE && says("words_out"));
  }

  // ---- describing: the argument path, both forms
  sfm_desc_set voc = fake(64, 128), voc0 = fake(0, 128), voc_big = fake(1025, 8), voc_len = fake(1024, 129);
  std::vector<int8_t> desc(2 * 64 * 128, 7);
  std::vector<int64_t> norm2(2, -7);
  auto describe = [&](sfm_desc_set* v, std::vector<sfm_desc_set*> views) {
    const int h = sfm_view_describe(v, (int)views.size(), views.data(), desc.data(), norm2.data(), nullptr, nullptr, nullptr);
    const int d = sfm_view_describe_dev(v, (int)views.size(), views.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return h == SFM_E_SHAPE && d == SFM_E_SHAPE;
  };
  EXPECT(describe(nullptr, {&a}) && says("vocabulary is null"));
  EXPECT(describe(&ham, {&a}) && says("vocabulary 0 is not an exact L2 set"));
  EXPECT(describe(&voc0, {&a}) && says("K = 0"));
  EXPECT(describe(&voc_big, {&a}) && says("K = 1025"));
  EXPECT(describe(&voc_len, {&a}) && says("K * D = 132096"));
  EXPECT(describe(&voc, {}) && says("0 views"));
  EXPECT(describe(&voc, {&a, &flt}) && says("view 1 is not an exact L2 set"));
  EXPECT(describe(&voc, {&a, &narrow}) && says("view 1 has dim 64"));
  EXPECT(describe(&voc, {&narrow}) && says("the views have dim 64, the vocabulary 128"));
  EXPECT(describe(&voc, {&a, nullptr}) && says("view 1 is null"));

  // ---- pairs: the argument path, both forms
  const int V = 5, len = 16, k = 2;
  std::vector<int8_t> pd(V * len, 1);
  std::vector<int64_t> pn(V, len);
  std::vector<int> nbr(V * 64, -7), pairs(2 * 10, -7), how(10, -7);
  std::vector<double> nbr_score(V * 64, -7.0), pair_score(10, -7.0);
  int64_t n_pairs = -7;
  auto both = [&](int v, int l, const int8_t* d, const int64_t* n, int kk, double ms, int mu, int sq, long long cap) {
    const int h = sfm_view_pairs(v, l, d, n, kk, ms, mu, sq, cap, nbr.data(), nbr_score.data(), pairs.data(), how.data(), pair_score.data(), nullptr, &n_pairs);
    const int dv = sfm_view_pairs_dev(v, l, d, n, kk, ms, mu, sq, cap, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_pairs, nullptr);
    return h == SFM_E_SHAPE && dv == SFM_E_SHAPE;
  };
  EXPECT(both(0, len, pd.data(), pn.data(), k, -inf, 0, 0, 10) && says("V = 0"));
  EXPECT(both(65537, len, pd.data(), pn.data(), k, -inf, 0, 0, 10) && says("V = 65537"));
  EXPECT(both(V, 0, pd.data(), pn.data(), k, -inf, 0, 0, 10) && both(V, 131073, pd.data(), pn.data(), k, -inf, 0, 0, 10) && says("len = 131073"));
  EXPECT(both(V, len, nullptr, pn.data(), k, -inf, 0, 0, 10) && both(V, len, pd.data(), nullptr, k, -inf, 0, 0, 10) && says("null"));
  EXPECT(both(V, len, pd.data(), pn.data(), 0, -inf, 0, 0, 10) && says("k = 0"));
  EXPECT(both(V, len, pd.data(), pn.data(), 65, -inf, 0, 0, 10) && says("k = 65"));
  EXPECT(both(V, len, pd.data(), pn.data(), k, nan, 0, 0, 10) && says("NaN"));
  EXPECT(both(V, len, pd.data(), pn.data(), k, 0.0, 2, 0, 10) && both(V, len, pd.data(), pn.data(), k, 0.0, -1, 0, 10) && says("mutual"));
  EXPECT(both(V, len, pd.data(), pn.data(), k, 0.0, 0, -1, 10) && says("sequential"));
  EXPECT(both(V, len, pd.data(), pn.data(), k, 0.0, 0, 0, -1) && says("cap"));
  EXPECT(both(65536, len, pd.data(), pn.data(), 64, 0.0, 0, 65536, 0) && says("2^31 pairs"));
  EXPECT(sfm_view_pairs(V, len, pd.data(), pn.data(), k, 0.0, 0, 0, 10, nullptr, nullptr, nullptr, how.data(), nullptr, nullptr, &n_pairs) == SFM_E_SHAPE &&
         says("without pairs"));

  if (sfm_init(0) == SFM_OK) {
    std::printf("host_check_retrieve: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  // valid arguments: every call goes on to look for a device and fails there, with nothing written
  const int rc_train = train({&a, &empty, &b}, 8, 4, 0);
  EXPECT(rc_train != SFM_E_SHAPE && rc_train != SFM_OK);
  {
    sfm_desc_set* views[2] = {&a, &empty};
    const int rc = sfm_view_describe(&voc, 2, views, desc.data(), norm2.data(), nullptr, nullptr, nullptr);
    EXPECT(rc != SFM_E_SHAPE && rc != SFM_OK);
  }
  const int rc_pairs = sfm_view_pairs(V, len, pd.data(), pn.data(), k, -inf, 1, 2, 10, nbr.data(), nbr_score.data(), pairs.data(), how.data(),
                                      pair_score.data(), nullptr, &n_pairs);
  EXPECT(rc_pairs != SFM_E_SHAPE && rc_pairs != SFM_OK);
  for (uint8_t v : words) EXPECT(v == 7);
  for (int64_t v : log) EXPECT(v == -7);
  for (int8_t v : desc) EXPECT(v == 7);
  for (int64_t v : norm2) EXPECT(v == -7);
  for (int v : nbr) EXPECT(v == -7);
  for (int v : pairs) EXPECT(v == -7);
  for (int v : how) EXPECT(v == -7);
  for (double v : nbr_score) EXPECT(v == -7.0);
  for (double v : pair_score) EXPECT(v == -7.0);
  EXPECT(n_pairs == -7);
  if (failures == 0) std::printf("host_check_retrieve: ok (without a device the valid calls returned %d, %d)\n", rc_train, rc_pairs);
  return failures == 0 ? 0 : 1;
}
