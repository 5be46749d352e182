// host_check_match_guided.hip -- a stand-alone program around the host code of guided matching that needs no device: the
// adjugate helper and the argument path of sfm_match_guided / sfm_match_guided_dev up to the first call that wants a GPU.
// Meant to be built with the host sanitizers and run on a machine without a GPU (the device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_match_guided.hip $(make -s print-srcs) -ldl -o /tmp/host_check_match_guided
//   /tmp/host_check_match_guided
// Exit status 0 and "host_check_match_guided: ok" when every check holds and the sanitizers stay silent.
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
  // ---- the adjugate: H adj(H) = det(H) I, not scaled, NULL arguments refused
  const double H[9] = {1.02, 0.03, -4.0, -0.02, 0.98, 7.5, 1e-5, -2e-5, 1.0};
  double G[9];
  EXPECT(sfm_homography_adjugate(H, G) == SFM_OK);
  const double det = H[0] * G[0] + H[1] * G[3] + H[2] * G[6];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += H[3 * i + k] * G[3 * k + j];
      EXPECT(std::fabs(s - (i == j ? det : 0.0)) < 1e-12);
    }
  const double I3[9] = {2, 0, 0, 0, 2, 0, 0, 0, 2};
  EXPECT(sfm_homography_adjugate(I3, G) == SFM_OK && G[0] == 4.0 && G[4] == 4.0 && G[8] == 4.0 && G[1] == 0.0);
  EXPECT(sfm_homography_adjugate(nullptr, G) == SFM_E_SHAPE);
  EXPECT(sfm_homography_adjugate(H, nullptr) == SFM_E_SHAPE);

  // ---- the argument path: these answers come before the library looks for a device
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  sfm_desc_set* fake = reinterpret_cast<sfm_desc_set*>(&failures);      // never dereferenced on these paths
  sfm_desc_set* refs[2] = {fake, fake};
  std::vector<double> xs(4, 1.0);
  const double* rx[2] = {xs.data(), xs.data()};
  int kind[2] = {SFM_GUIDE_FUNDAMENTAL, SFM_GUIDE_HOMOGRAPHY};
  double model[18];
  for (int i = 0; i < 18; ++i) model[i] = 0.1 * (i + 1);
  int best[8];
  std::memset(best, 0x55, sizeof(best));
  auto host = [&](double e2) {
    return sfm_match_guided(fake, xs.data(), xs.data(), 2, refs, rx, rx, kind, model, e2, best, nullptr, nullptr, nullptr, nullptr, nullptr);
  };
  auto dev = [&](double e2) {
    return sfm_match_guided_dev(fake, nullptr, nullptr, 2, refs, rx, rx, kind, model, e2, best, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr);
  };
  EXPECT(sfm_match_guided(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 4.0, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr) == SFM_E_HANDLE);
  EXPECT(host(nan) == SFM_E_SHAPE && dev(nan) == SFM_E_SHAPE);
  EXPECT(host(-1.0) == SFM_E_SHAPE && dev(-inf) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "max_err2") != nullptr);
  kind[1] = 3;
  EXPECT(host(4.0) == SFM_E_SHAPE && dev(4.0) == SFM_E_SHAPE);
  kind[1] = -1;
  EXPECT(host(4.0) == SFM_E_SHAPE);
  kind[1] = SFM_GUIDE_HOMOGRAPHY;
  model[17] = nan;
  EXPECT(host(4.0) == SFM_E_SHAPE && dev(4.0) == SFM_E_SHAPE);
  model[17] = 1.0;
  model[3] = inf;
  EXPECT(host(4.0) == SFM_E_SHAPE);
  EXPECT(std::strstr(sfm_last_error(), "not finite") != nullptr);
  model[3] = 0.4;
  EXPECT(sfm_match_guided(fake, xs.data(), xs.data(), -1, refs, rx, rx, kind, model, 4.0, best, nullptr, nullptr, nullptr, nullptr,
                          nullptr) == SFM_E_SHAPE);
  EXPECT(sfm_match_guided(fake, xs.data(), xs.data(), 2, refs, rx, rx, nullptr, model, 4.0, best, nullptr, nullptr, nullptr, nullptr,
                          nullptr) == SFM_E_SHAPE);
  // a non-finite model of an UNGATED reference is not an error of the argument path: the call goes on to look for a device
  kind[0] = SFM_GUIDE_NONE;
  model[0] = nan;
  if (sfm_init(0) == SFM_OK) {                                            // with a device the fake handle would be read
    std::printf("host_check_match_guided: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  const int rc = host(4.0);
  EXPECT(rc != SFM_E_SHAPE && rc != SFM_OK);                              // no device here: SFM_E_NO_DEVICE or SFM_E_HIP
  for (int i = 0; i < 8; ++i) EXPECT(best[i] == 0x55555555);              // no output was touched anywhere above
  if (failures == 0) std::printf("host_check_match_guided: ok (without a device the valid call returned %d)\n", rc);
  return failures == 0 ? 0 : 1;
}
