// host_check_track_link.hip -- a stand-alone program around the host code of the track linking that needs no device: the
// argument rules of sfm_link_tracks / sfm_link_tracks_dev (up to, but not past, the first call that wants a GPU), the match
// check the host form does on the host, and the launch plan (sfm_link_tracks_plan) under sfm_set_cu_limit.  The store form
// (sfm_link_tracks_views) needs a store, and a store needs a device: only its null handle is looked at here.
// Meant to be built with the host sanitizers and run on a machine without a GPU (the device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_track_link.hip $(make -s print-srcs) -ldl -o /tmp/host_check_track_link
//   /tmp/host_check_track_link
// Exit status 0 and "host_check_track_link: ok" when every check holds and the sanitizers stay silent.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/sfm_hip.h"

static int failures = 0;

#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

int main() {
  // three views of 4, 3 and 5 keys; pairs (0, 1), (2, 1), (0, 2) with 2, 1 and 2 matches
  const int V = 3, P = 3;
  const int key_ptr[V + 1] = {0, 4, 7, 12};
  const int pairs[2 * P] = {0, 1, 2, 1, 0, 2};
  const int64_t pair_ptr[P + 1] = {0, 2, 3, 5};
  const int a[5] = {0, 3, 4, 1, 2}, b[5] = {1, 2, 0, 4, 3};
  const unsigned char mask[5] = {1, 0, 1, 1, 1};
  const int K = 12;
  std::vector<int> key_track(K, -7), pt_ptr(K / 2 + 2, -7), cam_idx(K, -7), key_idx(K, -7), label(K, -7);
  int64_t summary[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
  int n_tracks = -7;
  int64_t n_obs = -7;
  auto host = [&](int v, const int* kp, int p, const int* pv, const int64_t* pp, const int* aa, const int* bb, int min_len, int group, int scan) {
    return sfm_link_tracks(v, kp, p, pv, pp, aa, bb, mask, min_len, group, scan, key_track.data(), pt_ptr.data(), cam_idx.data(), key_idx.data(),
                          summary, label.data());
  };
  auto dev = [&](int v, const int* kp, int p, const int* pv, const int64_t* pp, const int* aa, const int* bb, int min_len, int group, int scan) {
    return sfm_link_tracks_dev(v, kp, p, pv, pp, aa, bb, nullptr, min_len, group, scan, key_track.data(), pt_ptr.data(), cam_idx.data(),
                              key_idx.data(), summary, label.data(), &n_tracks, &n_obs, nullptr);
  };
#define BOTH_REFUSE(word, ...)                                                                   \
  do {                                                                                           \
    EXPECT(host(__VA_ARGS__) == SFM_E_SHAPE && std::strstr(sfm_last_error(), word) != nullptr);  \
    EXPECT(dev(__VA_ARGS__) == SFM_E_SHAPE && std::strstr(sfm_last_error(), word) != nullptr);   \
  } while (0)
  BOTH_REFUSE("sizes", -1, key_ptr, P, pairs, pair_ptr, a, b, 2, 0, 0);
  BOTH_REFUSE("sizes", V, key_ptr, -1, pairs, pair_ptr, a, b, 2, 0, 0);
  BOTH_REFUSE("null", V, nullptr, P, pairs, pair_ptr, a, b, 2, 0, 0);
  BOTH_REFUSE("null", V, key_ptr, P, nullptr, pair_ptr, a, b, 2, 0, 0);
  BOTH_REFUSE("null", V, key_ptr, P, pairs, nullptr, a, b, 2, 0, 0);
  BOTH_REFUSE("null", V, key_ptr, P, pairs, pair_ptr, nullptr, b, 2, 0, 0);
  BOTH_REFUSE("null", V, key_ptr, P, pairs, pair_ptr, a, nullptr, 2, 0, 0);
  for (int min_len : {1, 0, -3}) BOTH_REFUSE("min_len", V, key_ptr, P, pairs, pair_ptr, a, b, min_len, 0, 0);
  for (int group : {-1, 2, 3, 48, 128}) BOTH_REFUSE("group", V, key_ptr, P, pairs, pair_ptr, a, b, 2, group, 0);
  for (int scan : {-1, 3}) BOTH_REFUSE("scan", V, key_ptr, P, pairs, pair_ptr, a, b, 2, 0, scan);
  {
    const int from_one[V + 1] = {1, 4, 7, 12}, down[V + 1] = {0, 4, 3, 12};
    BOTH_REFUSE("key_ptr[0]", V, from_one, P, pairs, pair_ptr, a, b, 2, 0, 0);
    BOTH_REFUSE("decreases at view 1", V, down, P, pairs, pair_ptr, a, b, 2, 0, 0);
    const int far[2 * P] = {0, 1, 2, 3, 0, 2}, neg[2 * P] = {0, 1, 2, 1, -1, 2}, self[2 * P] = {1, 1, 2, 1, 0, 2};
    BOTH_REFUSE("pair 1 ", V, key_ptr, P, far, pair_ptr, a, b, 2, 0, 0);
    BOTH_REFUSE("pair 2 ", V, key_ptr, P, neg, pair_ptr, a, b, 2, 0, 0);
    BOTH_REFUSE("pair 0 ", V, key_ptr, P, self, pair_ptr, a, b, 2, 0, 0);
    const int64_t ptr_from_one[P + 1] = {1, 2, 3, 5}, ptr_down[P + 1] = {0, 3, 2, 5};
    BOTH_REFUSE("pair_ptr[0]", V, key_ptr, P, pairs, ptr_from_one, a, b, 2, 0, 0);
    BOTH_REFUSE("decreases at pair 1", V, key_ptr, P, pairs, ptr_down, a, b, 2, 0, 0);
  }
  // a key index out of its view's range: the host form finds the lowest such match on the host, masked or not
  {
    const int a1[5] = {0, 4, 4, 1, 2}, a2[5] = {0, 3, 5, 1, 9}, b3[5] = {1, 2, 0, 5, 3}, b4[5] = {1, 2, 0, 4, -1};
    EXPECT(host(V, key_ptr, P, pairs, pair_ptr, a1, b, 2, 0, 0) == SFM_E_SHAPE && std::strstr(sfm_last_error(), "match 1 ") != nullptr);
    EXPECT(host(V, key_ptr, P, pairs, pair_ptr, a2, b, 2, 0, 0) == SFM_E_SHAPE && std::strstr(sfm_last_error(), "match 2 ") != nullptr);
    EXPECT(host(V, key_ptr, P, pairs, pair_ptr, a, b3, 2, 0, 0) == SFM_E_SHAPE && std::strstr(sfm_last_error(), "match 3 ") != nullptr);
    EXPECT(host(V, key_ptr, P, pairs, pair_ptr, a, b4, 2, 0, 0) == SFM_E_SHAPE && std::strstr(sfm_last_error(), "match 4 ") != nullptr);
  }
  EXPECT(sfm_link_tracks_views(nullptr, 0, nullptr, nullptr, 2, nullptr, summary) != SFM_OK);

  // ---- the plan
  int plan[8], again[8];
  EXPECT(sfm_link_tracks_plan(1000, 8000000, 40000000, 0, 0, plan) == SFM_OK);
  int cus = 0, eff = 0;
  EXPECT(sfm_cu_count(&cus, &eff) == SFM_OK && cus == eff);
  EXPECT(plan[0] == 16 * cus && plan[2] == 32 * cus && plan[3] == 4 * cus && plan[4] == 2 && plan[5] == 7813 && plan[6] == 2 && plan[7] == 3907);
  for (int limit : {1, 32}) {
    EXPECT(sfm_set_cu_limit(limit) == SFM_OK);
    EXPECT(sfm_link_tracks_plan(1000, 8000000, 40000000, 0, 0, again) == SFM_OK);
    EXPECT(again[0] == 16 * limit && again[2] == 32 * limit && again[3] == 4 * limit);
    for (int k = 4; k < 8; ++k) EXPECT(again[k] == plan[k]);
  }
  EXPECT(sfm_set_cu_limit(0) == SFM_OK);
  EXPECT(sfm_link_tracks_plan(1000, 8000000, 40000000, 0, 0, again) == SFM_OK && std::memcmp(plan, again, sizeof(plan)) == 0);
  EXPECT(sfm_link_tracks_plan(0, 0, 0, 0, 0, again) == SFM_OK && again[0] == 1 && again[2] == 1 && again[3] == 1 && again[4] == 1 && again[5] == 1);
  EXPECT(sfm_link_tracks_plan(10, 5000, 100, 16, 2, again) == SFM_OK && again[1] == 16 && again[4] == 2 && again[5] == 5 && again[6] == 2 && again[7] == 3);
  EXPECT(sfm_link_tracks_plan(10, 5000, 100, 0, 1, again) == SFM_OK && again[4] == 1 && again[6] == 1);
  EXPECT(sfm_link_tracks_plan(10, 2147483647LL, 100, 0, 0, again) == SFM_OK && again[5] == 2097152);
  EXPECT(sfm_link_tracks_plan(10, 2147483648LL, 100, 0, 0, again) == SFM_E_SHAPE);
  EXPECT(sfm_link_tracks_plan(10, -1, 100, 0, 0, again) == SFM_E_SHAPE && sfm_link_tracks_plan(10, 10, -1, 0, 0, again) == SFM_E_SHAPE);
  EXPECT(sfm_link_tracks_plan(-1, 10, 1, 0, 0, again) == SFM_E_SHAPE && sfm_link_tracks_plan(10, 10, 1, 5, 0, again) == SFM_E_SHAPE);
  EXPECT(sfm_link_tracks_plan(10, 10, 1, 0, 3, again) == SFM_E_SHAPE && sfm_link_tracks_plan(10, 10, 1, 0, 0, nullptr) == SFM_E_SHAPE);

  if (sfm_init(0) == SFM_OK) {
    std::printf("host_check_track_link: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  const int rc = host(V, key_ptr, P, pairs, pair_ptr, a, b, 2, 0, 0);          // valid arguments: the call goes on to look for a device
  EXPECT(rc != SFM_E_SHAPE && rc != SFM_OK);
  const int rc_dev = dev(V, key_ptr, P, pairs, pair_ptr, a, b, 3, 64, 2);
  EXPECT(rc_dev != SFM_E_SHAPE && rc_dev != SFM_OK);
  const int64_t no_ptr[1] = {0};
  const int rc_empty = dev(0, key_ptr, 0, nullptr, no_ptr, nullptr, nullptr, 2, 0, 0);      // K = 0, P = 0: valid
  EXPECT(rc_empty != SFM_E_SHAPE && rc_empty != SFM_OK);
  for (int v : key_track) EXPECT(v == -7);                                     // no output was touched anywhere above
  for (int v : pt_ptr) EXPECT(v == -7);
  for (int v : cam_idx) EXPECT(v == -7);
  for (int v : key_idx) EXPECT(v == -7);
  for (int v : label) EXPECT(v == -7);
  for (int64_t v : summary) EXPECT(v == -7);
  EXPECT(n_tracks == -7 && n_obs == -7);
  if (failures == 0) std::printf("host_check_track_link: ok (without a device the valid call returned %d)\n", rc);
  return failures == 0 ? 0 : 1;
}
