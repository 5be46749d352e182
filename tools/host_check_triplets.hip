// host_check_triplets.hip -- a stand-alone program around the host code of the view-triplet filter that needs no device: the
// test of a triplet (sfm_view_triplet_test) and the argument path of sfm_view_triplets / sfm_view_triplets_dev up to, but not
// past, the first call that wants a GPU.  Meant to be built with the host sanitizers and run on a machine without a GPU (the
// device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_triplets.hip $(make -s print-srcs) -ldl -o /tmp/host_check_triplets
//   /tmp/host_check_triplets
// Exit status 0 and "host_check_triplets: ok" when every check holds and the sanitizers stay silent.
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
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  EXPECT(sfm_version() >= 111);

  // ---- the test of a triplet: lhs = trace(M_ac^T M_bc M_ab)
  {
    double lhs = -1;
    EXPECT(sfm_view_triplet_test(eye, eye, eye, 1.0, &lhs) == 1 && lhs == 3.0);
    EXPECT(sfm_view_triplet_test(eye, eye, eye, 1.0, nullptr) == 1);
    const double c = std::cos(0.2), s = std::sin(0.2), c2 = std::cos(0.4), s2 = std::sin(0.4);
    const double rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, rz2[9] = {c2, -s2, 0, s2, c2, 0, 0, 0, 1};
    EXPECT(sfm_view_triplet_test(rz, rz, rz2, 1.0 - 1e-15, &lhs) == 1 && std::fabs(lhs - 3.0) < 1e-15);      // M_ac = M_bc M_ab
    EXPECT(sfm_view_triplet_test(rz, eye, eye, std::cos(0.19), &lhs) == 0 && std::fabs(lhs - (1 + 2 * c)) < 1e-15);
    EXPECT(sfm_view_triplet_test(rz, eye, eye, std::cos(0.21), &lhs) == 1);
    EXPECT(sfm_view_triplet_test(eye, rz, eye, std::cos(0.19), &lhs) == 0 && sfm_view_triplet_test(eye, eye, rz, std::cos(0.19), &lhs) == 0);
    double lhs_edge = -2;
    EXPECT(sfm_rotation_edge_test(rz, rz2, rz, 0.9, &lhs_edge) == sfm_view_triplet_test(rz, rz, rz2, 0.9, &lhs) && lhs == lhs_edge);
    double bad[9];
    std::memcpy(bad, eye, sizeof(bad));
    bad[4] = nan;
    EXPECT(sfm_view_triplet_test(bad, eye, eye, 0.5, &lhs) == 0 && std::isnan(lhs));
    bad[4] = inf;
    EXPECT(sfm_view_triplet_test(eye, bad, eye, 0.5, &lhs) == 0 && sfm_view_triplet_test(eye, eye, bad, 0.5, &lhs) == 0);
    EXPECT(sfm_view_triplet_test(nullptr, eye, eye, 0.5, &lhs) == 0 && sfm_view_triplet_test(eye, nullptr, eye, 0.5, &lhs) == 0);
    EXPECT(sfm_view_triplet_test(eye, eye, nullptr, 0.5, &lhs) == 0);
  }

  // ---- the argument path: these answers come before the library looks for a device
  const int V = 4, E = 5;
  const int edges[2 * E] = {0, 1, 1, 2, 2, 3, 3, 0, 0, 2};
  std::vector<double> rel(9 * E);
  for (int e = 0; e < E; ++e) std::memcpy(&rel[9 * e], eye, sizeof(eye));
  std::vector<unsigned char> keep(E, 9), mask(E, 1);
  std::vector<int64_t> n_tri(E, -1), n_ok(E, -1);
  std::vector<int> kept(E, -5);
  int64_t summary[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  int n_kept = -5;
  auto host = [&](int v, long long e, const int* ed, const double* rl, double cl, int mo, int mp, int ku, int g) {
    return sfm_view_triplets(v, e, ed, rl, mask.data(), cl, mo, mp, ku, g, keep.data(), n_tri.data(), n_ok.data(), kept.data(), summary, &n_kept);
  };
  auto dev = [&](int v, long long e, const int* ed, const double* rl, double cl, int mo, int mp, int ku, int g) {
    return sfm_view_triplets_dev(v, e, ed, rl, nullptr, cl, mo, mp, ku, g, nullptr, nullptr, nullptr, nullptr, nullptr, &n_kept, nullptr);
  };
#define BOTH_REFUSE(...) EXPECT(host(__VA_ARGS__) == SFM_E_SHAPE && dev(__VA_ARGS__) == SFM_E_SHAPE)
  BOTH_REFUSE(2, E, edges, rel.data(), 0.99, 1, 0, 0, 0);
  BOTH_REFUSE(V, 0, edges, rel.data(), 0.99, 1, 0, 0, 0);
  BOTH_REFUSE(V, 1LL << 30, edges, rel.data(), 0.99, 1, 0, 0, 0);
  BOTH_REFUSE(V, 1LL << 40, edges, rel.data(), 0.99, 1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "E=") != nullptr);
  for (double cl : {nan, 0.0, -0.5, 1.0000001, inf}) BOTH_REFUSE(V, E, edges, rel.data(), cl, 1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "cos_loop") != nullptr);
  BOTH_REFUSE(V, E, edges, rel.data(), 0.99, -1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "min_ok") != nullptr);
  for (int mp : {-1, 101}) BOTH_REFUSE(V, E, edges, rel.data(), 0.99, 1, mp, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "min_pct") != nullptr);
  for (int ku : {-1, 2}) BOTH_REFUSE(V, E, edges, rel.data(), 0.99, 1, 0, ku, 0);
  EXPECT(std::strstr(sfm_last_error(), "keep_untested") != nullptr);
  for (int g : {-1, 2, 3, 12, 128}) BOTH_REFUSE(V, E, edges, rel.data(), 0.99, 1, 0, 0, g);
  EXPECT(std::strstr(sfm_last_error(), "group") != nullptr);
  const int loop[2 * E] = {0, 1, 1, 2, 2, 2, 3, 0, 0, 2}, far[2 * E] = {0, 1, 1, 2, 2, 3, 3, 0, 0, 4}, neg[2 * E] = {0, -1, 1, 2, 2, 3, 3, 0, 0, 2};
  BOTH_REFUSE(V, E, loop, rel.data(), 0.99, 1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "edge 2 ") != nullptr);
  BOTH_REFUSE(V, E, far, rel.data(), 0.99, 1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "edge 4 ") != nullptr);
  BOTH_REFUSE(V, E, neg, rel.data(), 0.99, 1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "edge 0 ") != nullptr);
  BOTH_REFUSE(V, E, nullptr, rel.data(), 0.99, 1, 0, 0, 0);
  BOTH_REFUSE(V, E, edges, nullptr, 0.99, 1, 0, 0, 0);
  EXPECT(std::strstr(sfm_last_error(), "null") != nullptr);
  {
    std::vector<double> stretched(rel);
    stretched[9 * 3 + 4] = 1.5;
    stretched[9 * 1 + 0] = 1.2;
    EXPECT(host(V, E, edges, stretched.data(), 0.99, 1, 0, 0, 0) == SFM_E_BAD_ROTATION);
    EXPECT(std::strstr(sfm_last_error(), "edge 1 ") != nullptr);                       // the lowest such edge
  }
  if (sfm_init(0) == SFM_OK) {
    std::printf("host_check_triplets: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  const int rc = host(V, E, edges, rel.data(), 0.99, 0, 100, 1, 64);                    // valid arguments: the call goes on to look for a device
  EXPECT(rc != SFM_E_SHAPE && rc != SFM_E_BAD_ROTATION && rc != SFM_OK);
  const int rc_dev = dev(V, E, edges, rel.data(), 1.0, 1, 0, 0, 1);
  EXPECT(rc_dev != SFM_E_SHAPE && rc_dev != SFM_OK);
  for (unsigned char v : keep) EXPECT(v == 9);                                          // no output was touched anywhere above
  for (int64_t v : n_tri) EXPECT(v == -1);
  for (int64_t v : n_ok) EXPECT(v == -1);
  for (int v : kept) EXPECT(v == -5);
  for (int64_t v : summary) EXPECT(v == -1);
  EXPECT(n_kept == -5);
  if (failures == 0) std::printf("host_check_triplets: ok (without a device the valid call returned %d)\n", rc);
  return failures == 0 ? 0 : 1;
}
