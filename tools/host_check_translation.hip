// host_check_translation.hip -- a stand-alone program around the host code of the translation averaging that needs no device:
// the test of an edge (sfm_translation_edge_test) and the argument path of sfm_translation_average /
// sfm_translation_average_dev up to, but not past, the first call that wants a GPU.
// Meant to be built with the host sanitizers and run on a machine without a GPU (the device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_translation.hip $(make -s print-srcs) -ldl -o /tmp/host_check_translation
//   /tmp/host_check_translation
// Exit status 0 and "host_check_translation: ok" when every check holds and the sanitizers stay silent.
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

  // ---- the test of an edge
  {
    const double x[3] = {1, 0, 0}, o[3] = {0, 0, 0};
    double dv = -1, n2 = -1;
    const double along[3] = {5, 0, 0}, across[3] = {0, 2, 0}, back[3] = {-1, 0, 0}, v345[3] = {4, 3, 0};
    EXPECT(sfm_translation_edge_test(x, o, along, 1.0, &dv, &n2) == 1 && dv == 5.0 && n2 == 25.0);      // exactly at cos_max = 1
    EXPECT(sfm_translation_edge_test(x, o, along, 1.0, nullptr, nullptr) == 1);
    EXPECT(sfm_translation_edge_test(x, o, across, 0.5, &dv, &n2) == 0 && dv == 0.0 && n2 == 4.0);      // dv = 0
    EXPECT(sfm_translation_edge_test(x, o, o, 0.5, &dv, &n2) == 0 && dv == 0.0 && n2 == 0.0);           // n2 = 0
    EXPECT(sfm_translation_edge_test(x, o, back, 0.5, &dv, &n2) == 0 && dv == -1.0);                    // the wrong way
    for (double cm : {0.8, std::nextafter(0.8, 0.0), std::nextafter(0.8, 1.0), 0.8 - 1e-6, 0.8 + 1e-6}) {
      const int in = sfm_translation_edge_test(x, o, v345, cm, &dv, &n2);
      EXPECT(dv == 4.0 && n2 == 25.0 && in == (dv * dv >= (cm * cm) * n2 ? 1 : 0));
    }
    EXPECT(sfm_translation_edge_test(x, o, v345, 0.8 - 1e-6, &dv, &n2) == 1 && sfm_translation_edge_test(x, o, v345, 0.8 + 1e-6, &dv, &n2) == 0);
    const double bad[3] = {nan, 0, 0}, far[3] = {inf, 0, 0}, huge[3] = {1e200, 1e200, 0};
    EXPECT(sfm_translation_edge_test(x, o, bad, 0.5, &dv, &n2) == 0 && std::isnan(dv));
    EXPECT(sfm_translation_edge_test(bad, o, along, 0.5, &dv, &n2) == 0);
    EXPECT(sfm_translation_edge_test(x, bad, along, 0.5, &dv, &n2) == 0);
    EXPECT(sfm_translation_edge_test(x, o, far, 0.5, &dv, &n2) == 0);
    EXPECT(sfm_translation_edge_test(x, o, huge, 0.5, &dv, &n2) == 0 && std::isinf(n2));
    EXPECT(sfm_translation_edge_test(nullptr, o, along, 0.5, &dv, &n2) == 0 && sfm_translation_edge_test(x, nullptr, along, 0.5, &dv, &n2) == 0);
    EXPECT(sfm_translation_edge_test(x, o, nullptr, 0.5, &dv, &n2) == 0);
  }

  // ---- the argument path: these answers come before the library looks for a device
  const int V = 4, E = 5, rounds = 2;
  const int edges[2 * E] = {0, 1, 1, 2, 2, 3, 3, 0, 0, 2};
  std::vector<double> R(9 * V), t(3 * E, 0.5), C(3 * V, 7.0), cosv(E, 7.0), lenv(E, 7.0), log(4 * (rounds + 2), 7.0);
  for (int v = 0; v < V; ++v) std::memcpy(&R[9 * v], eye, sizeof(eye));
  std::vector<unsigned char> inl(E, 9), mask(E, 1);
  int view[V] = {-5, -5, -5, -5}, small[2] = {-5, -5};
  int64_t summary[6] = {-1, -1, -1, -1, -1, -1};
  auto host = [&](int v, long long e, const int* ed, const double* r, const double* tt, int root, double cm, double mu, int rd, int pol, double tol,
                  int cgm) {
    return sfm_translation_average(v, e, ed, r, tt, mask.data(), root, cm, mu, rd, pol, tol, cgm, C.data(), inl.data(), cosv.data(), lenv.data(),
                                   view, small, small + 1, summary, log.data());
  };
  auto dev = [&](int v, long long e, const int* ed, const double* r, const double* tt, int root, double cm, double mu, int rd, int pol, double tol,
                 int cgm) {
    return sfm_translation_average_dev(v, e, ed, r, tt, nullptr, root, cm, mu, rd, pol, tol, cgm, C.data(), nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, nullptr);
  };
#define BOTH_REFUSE(...) EXPECT(host(__VA_ARGS__) == SFM_E_SHAPE && dev(__VA_ARGS__) == SFM_E_SHAPE)
  BOTH_REFUSE(1, E, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  BOTH_REFUSE(V, 0, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  BOTH_REFUSE(V, 1LL << 30, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  BOTH_REFUSE(V, 1LL << 31, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "E=") != nullptr);
  BOTH_REFUSE(V, E, edges, R.data(), t.data(), -1, 0.99, 0.01, rounds, 1, 1e-12, 100);
  BOTH_REFUSE(V, E, edges, R.data(), t.data(), V, 0.99, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "root") != nullptr);
  for (double cm : {nan, 0.0, -0.5, 1.0000001, inf}) BOTH_REFUSE(V, E, edges, R.data(), t.data(), 0, cm, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "cos_max") != nullptr);
  for (double mu : {nan, -0.01, 1.0000001, inf}) BOTH_REFUSE(V, E, edges, R.data(), t.data(), 0, 0.99, mu, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "mu") != nullptr);
  BOTH_REFUSE(V, E, edges, R.data(), t.data(), 0, 0.99, 0.01, -1, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "rounds") != nullptr);
  for (int pol : {-1, 2}) BOTH_REFUSE(V, E, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, pol, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "polish") != nullptr);
  for (double tol : {nan, 0.0, 1.0, -1e-3}) BOTH_REFUSE(V, E, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, tol, 100);
  EXPECT(std::strstr(sfm_last_error(), "cg_tol") != nullptr);
  BOTH_REFUSE(V, E, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 0);
  EXPECT(std::strstr(sfm_last_error(), "cg_max") != nullptr);
  const int loop[2 * E] = {0, 1, 1, 2, 2, 2, 3, 0, 0, 2}, far[2 * E] = {0, 1, 1, 2, 2, 3, 3, 0, 0, 4}, neg[2 * E] = {0, -1, 1, 2, 2, 3, 3, 0, 0, 2};
  BOTH_REFUSE(V, E, loop, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "edge 2 ") != nullptr);
  BOTH_REFUSE(V, E, far, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "edge 4 ") != nullptr);
  BOTH_REFUSE(V, E, neg, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "edge 0 ") != nullptr);
  BOTH_REFUSE(V, E, nullptr, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  BOTH_REFUSE(V, E, edges, nullptr, t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  BOTH_REFUSE(V, E, edges, R.data(), nullptr, 0, 0.99, 0.01, rounds, 1, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "null") != nullptr);
  EXPECT(sfm_translation_average(V, E, edges, R.data(), t.data(), nullptr, 0, 0.99, 0.01, rounds, 1, 1e-12, 100, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr) == SFM_E_SHAPE);            // C_out is not optional
  {
    std::vector<double> stretched(R);
    stretched[9 * 3 + 4] = 1.5;
    stretched[9 * 2 + 0] = 1.2;
    for (int k = 0; k < 9; ++k) stretched[9 * 1 + k] = 0.0;                             // nine zeros: no rotation, no error
    EXPECT(host(V, E, edges, stretched.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100) == SFM_E_BAD_ROTATION);
    EXPECT(std::strstr(sfm_last_error(), "view 2 ") != nullptr);                        // the lowest such view
  }
  if (sfm_init(0) == SFM_OK) {
    std::printf("host_check_translation: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  const int rc = host(V, E, edges, R.data(), t.data(), 0, 0.99, 0.01, rounds, 1, 1e-12, 100);      // valid arguments: the call goes on to look for a device
  EXPECT(rc != SFM_E_SHAPE && rc != SFM_E_BAD_ROTATION && rc != SFM_OK);
  const int rc_dev = dev(V, E, edges, R.data(), t.data(), 3, 1.0, 0.0, 0, 0, 0.5, 1);
  EXPECT(rc_dev != SFM_E_SHAPE && rc_dev != SFM_OK);
  for (double v : C) EXPECT(v == 7.0);                                                 // no output was touched anywhere above
  for (double v : cosv) EXPECT(v == 7.0);
  for (double v : lenv) EXPECT(v == 7.0);
  for (double v : log) EXPECT(v == 7.0);
  for (unsigned char v : inl) EXPECT(v == 9);
  for (int v : view) EXPECT(v == -5);
  for (int v : small) EXPECT(v == -5);
  for (int64_t v : summary) EXPECT(v == -1);
  if (failures == 0) std::printf("host_check_translation: ok (without a device the valid call returned %d)\n", rc);
  return failures == 0 ? 0 : 1;
}
