// host_check_similarity.hip -- a stand-alone program around the host code of the robust similarity that needs no device:
// the sampler (sfm_similarity_sample) and the argument path of sfm_similarity_ransac / sfm_similarity_ransac_dev up to, but
// not past, the first call that wants a GPU.
// Meant to be built with the host sanitizers and run on a machine without a GPU (the device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_similarity.hip $(make -s print-srcs) -ldl -o /tmp/host_check_similarity
//   /tmp/host_check_similarity
// Exit status 0 and "host_check_similarity: ok" when every check holds and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  // ---- the sampler: three ascending distinct indices, one per third, for every small n and across a workgroup boundary
  std::vector<int> sizes;
  for (int n = 4; n <= 70; ++n) sizes.push_back(n);
  for (int n : {1023, 1024, 1025, 2049, 1 << 20}) sizes.push_back(n);
  for (int n : sizes)
    for (int h : {0, 1, 2, 63, 64, 127, 999}) {
      int idx[3] = {-1, -1, -1};
      EXPECT(sfm_similarity_sample(n, 1000, h, idx) == 1000);
      for (int k = 0; k < 3; ++k) EXPECT(idx[k] >= (long long)k * n / 3 && idx[k] < (long long)(k + 1) * n / 3);
      EXPECT(idx[0] < idx[1] && idx[1] < idx[2]);
      int again[3] = {-1, -1, -1};
      EXPECT(sfm_similarity_sample(n, 1000, h, again) == 1000 && std::memcmp(idx, again, sizeof(idx)) == 0);
    }
  {
    int idx[3] = {-7, -7, -7};
    EXPECT(sfm_similarity_sample(3, 128, 0, idx) == 0 && sfm_similarity_sample(64, 65537, 0, idx) == 0 && sfm_similarity_sample(64, -1, 0, idx) == 0);
    EXPECT(sfm_similarity_sample(0, 128, 0, idx) == 0 && sfm_similarity_sample(-5, 128, 0, idx) == 0);
    EXPECT(sfm_similarity_sample(64, 0, 128, idx) == 128 && sfm_similarity_sample(64, 0, -1, idx) == 128 && idx[0] == -7 && idx[2] == -7);
    EXPECT(sfm_similarity_sample(64, 0, 127, nullptr) == 128 && sfm_similarity_sample(64, 65536, 65535, idx) == 65536 && idx[0] >= 0);
  }

  // ---- the argument path: these answers come before the library looks for a device
  const int set_ptr[3] = {0, 6, 12};
  std::vector<double> xyz(36, 1.0), sim(26, 7.0);
  std::vector<unsigned char> inl(12, 9);
  int small[6] = {-5, -5, -5, -5, -5, -5};
  int64_t summary[6] = {-1, -1, -1, -1, -1, -1};
  auto host = [&](int n_sets, const int* ptr, long long M, double err2, int hyp, int iters, int flags) {
    return sfm_similarity_ransac(n_sets, ptr, M, xyz.data(), xyz.data(), err2, hyp, iters, flags, sim.data(), inl.data(), small, small + 2,
                                 small + 4, summary);
  };
  auto dev = [&](int n_sets, const int* ptr, long long M, double err2, int hyp, int iters, int flags) {
    return sfm_similarity_ransac_dev(n_sets, ptr, M, xyz.data(), xyz.data(), err2, hyp, iters, flags, sim.data(), nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr);
  };
  for (double e2 : {nan, -1.0, -inf})
    EXPECT(host(2, set_ptr, 12, e2, 128, 2, 0) == SFM_E_SHAPE && dev(2, set_ptr, 12, e2, 128, 2, 0) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "max_err2") != nullptr);
  for (int hyp : {-1, 65537})
    EXPECT(host(2, set_ptr, 12, 4, hyp, 2, 0) == SFM_E_SHAPE && dev(2, set_ptr, 12, 4, hyp, 2, 0) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "max_hyp") != nullptr);
  EXPECT(host(2, set_ptr, 12, 4, 128, -1, 0) == SFM_E_SHAPE && dev(2, set_ptr, 12, 4, 128, -1, 0) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "iters") != nullptr);
  for (int flags : {2, 3, -1, 1 << 30})
    EXPECT(host(2, set_ptr, 12, 4, 128, 2, flags) == SFM_E_SHAPE && dev(2, set_ptr, 12, 4, 128, 2, flags) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "flags") != nullptr);
  const int bad_a[3] = {1, 6, 12}, bad_b[3] = {0, 7, 6}, bad_c[3] = {0, 6, 11};
  EXPECT(host(2, bad_a, 12, 4, 128, 2, 0) == SFM_E_SHAPE && host(2, bad_b, 6, 4, 128, 2, 0) == SFM_E_SHAPE);
  EXPECT(host(2, bad_c, 12, 4, 128, 2, 0) == SFM_E_SHAPE && dev(2, nullptr, 12, 4, 128, 2, 0) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "set_ptr") != nullptr);
  EXPECT(host(2, set_ptr, -1, 4, 128, 2, 0) == SFM_E_SHAPE && host(-1, set_ptr, 12, 4, 128, 2, 0) == SFM_E_SHAPE);
  EXPECT(host(0, nullptr, 0, 4, 128, 2, 0) == SFM_E_SHAPE);                  // even an empty call needs its offsets
  EXPECT(sfm_similarity_ransac(2, set_ptr, 12, xyz.data(), xyz.data(), 4, 128, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr) == SFM_E_SHAPE);                     // sim_out is not optional
  EXPECT(sfm_similarity_ransac(2, set_ptr, 12, nullptr, xyz.data(), 4, 128, 2, 0, sim.data(), nullptr, nullptr, nullptr, nullptr,
                               nullptr) == SFM_E_SHAPE);
  EXPECT(sfm_similarity_ransac_dev(2, set_ptr, 12, xyz.data(), nullptr, 4, 128, 2, 0, sim.data(), nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "null") != nullptr);
  if (sfm_init(0) == SFM_OK) {
    std::printf("host_check_similarity: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  const int rc = host(2, set_ptr, 12, 4, 128, 2, SFM_SIMILARITY_RIGID);      // valid arguments: the call goes on to look for a device
  EXPECT(rc != SFM_E_SHAPE && rc != SFM_OK);
  const int rc_dev = dev(2, set_ptr, 12, 0, 1, 0, 0);
  EXPECT(rc_dev != SFM_E_SHAPE && rc_dev != SFM_OK);
  for (double v : sim) EXPECT(v == 7.0);                                     // no output was touched anywhere above
  for (unsigned char v : inl) EXPECT(v == 9);
  for (int v : small) EXPECT(v == -5);
  for (int64_t v : summary) EXPECT(v == -1);
  if (failures == 0) std::printf("host_check_similarity: ok (without a device the valid call returned %d)\n", rc);
  return failures == 0 ? 0 : 1;
}
