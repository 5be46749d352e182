// host_check_rotavg.hip -- a stand-alone program around the host code of the rotation averaging that needs no device: the
// spanning trees (sfm_rotation_tree), the test of an edge (sfm_rotation_edge_test), the batch plan (sfm_rotation_plan) and the
// argument path of sfm_rotation_average / sfm_rotation_average_dev up to, but not past, the first call that wants a GPU.
// Meant to be built with the host sanitizers and run on a machine without a GPU (the device code is not instrumented):
//   cd structure-from-motion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -munsafe-fp-atomics -Xarch_host -fsanitize=address,undefined \
//         ../../tools/host_check_rotavg.hip $(make -s print-srcs) -ldl -o /tmp/host_check_rotavg
//   /tmp/host_check_rotavg
// Exit status 0 and "host_check_rotavg: ok" when every check holds and the sanitizers stay silent.
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

  // ---- a ring of V views with chords: edge e = (e % V, (e + 1 + e / V) % V), orientations alternating
  for (int V : {2, 3, 5, 64, 65, 257, 5000}) {
    const int E = V == 2 ? 3 : 2 * V + 1;
    std::vector<int> edges(2 * (size_t)E);
    for (int e = 0; e < E; ++e) {
      int a = e % V, b = (a + 1 + e / V) % V;
      if (a == b) b = (a + 1) % V;
      edges[2 * e] = (e & 1) ? b : a;
      edges[2 * e + 1] = (e & 1) ? a : b;
    }
    std::vector<int> parent(V), depth(V), again_p(V), again_d(V);
    for (int h : {0, 1, 63, 127, 65535}) {
      const int root = V / 2;
      EXPECT(sfm_rotation_tree(V, E, edges.data(), root, 65536, h, parent.data(), depth.data()) == 65536);
      int roots = 0;
      for (int v = 0; v < V; ++v) {
        EXPECT(depth[v] >= 0);                                            // a ring is connected
        if (depth[v] == 0) { ++roots; EXPECT(parent[v] == -1); continue; }
        EXPECT(parent[v] >= 0 && parent[v] < E);
        const int i = edges[2 * parent[v]], j = edges[2 * parent[v] + 1], other = i == v ? j : i;
        EXPECT((i == v || j == v) && depth[other] == depth[v] - 1);
      }
      EXPECT(roots == 1 && (h != 0 || depth[root] == 0));
      EXPECT(sfm_rotation_tree(V, E, edges.data(), root, 65536, h, again_p.data(), again_d.data()) == 65536);
      EXPECT(parent == again_p && depth == again_d);
    }
    int mark[2] = {-7, -7};
    EXPECT(sfm_rotation_tree(V, E, edges.data(), 0, 0, 128, mark, mark + 1) == 128 && mark[0] == -7 && mark[1] == -7);
    EXPECT(sfm_rotation_tree(V, E, edges.data(), 0, 0, -1, mark, mark + 1) == 128 && mark[0] == -7);
    EXPECT(sfm_rotation_tree(V, E, edges.data(), 0, 16, 3, nullptr, nullptr) == 16);
    EXPECT(sfm_rotation_tree(V, E, edges.data(), V, 16, 0, parent.data(), depth.data()) == 0);
    EXPECT(sfm_rotation_tree(V, E, edges.data(), -1, 16, 0, parent.data(), depth.data()) == 0);
    EXPECT(sfm_rotation_tree(V, E, nullptr, 0, 16, 0, parent.data(), depth.data()) == 0);
    EXPECT(sfm_rotation_tree(V, 0, edges.data(), 0, 16, 0, parent.data(), depth.data()) == 0);
    EXPECT(sfm_rotation_tree(V, E, edges.data(), 0, 65537, 0, parent.data(), depth.data()) == 0);
    EXPECT(sfm_rotation_tree(1, E, edges.data(), 0, 16, 0, parent.data(), depth.data()) == 0);
  }
  {
    // two components and a view without an edge: the tree of h = 0 stops at the component of its root
    const int edges[] = {0, 1, 2, 1, 3, 4};
    int parent[6], depth[6];
    EXPECT(sfm_rotation_tree(6, 3, edges, 0, 4, 0, parent, depth) == 4);
    EXPECT(depth[0] == 0 && depth[1] == 1 && depth[2] == 2 && depth[3] == -1 && depth[4] == -1 && depth[5] == -1);
    EXPECT(parent[1] == 0 && parent[2] == 1 && parent[3] == -1 && parent[5] == -1);
    const int loop[] = {0, 1, 2, 2};
    EXPECT(sfm_rotation_tree(6, 2, loop, 0, 4, 0, parent, depth) == 0);
    const int far[] = {0, 6};
    EXPECT(sfm_rotation_tree(6, 1, far, 0, 4, 0, parent, depth) == 0);
  }

  // ---- the test of an edge
  {
    double lhs = -1;
    EXPECT(sfm_rotation_edge_test(eye, eye, eye, 1.0, &lhs) == 1 && lhs == 3.0);
    EXPECT(sfm_rotation_edge_test(eye, eye, eye, 1.0, nullptr) == 1);
    const double c = std::cos(0.2), s = std::sin(0.2);
    const double rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    EXPECT(sfm_rotation_edge_test(eye, rz, rz, 1.0, &lhs) == 1 && std::fabs(lhs - 3.0) < 1e-15);        // R_j = Rel R_i
    EXPECT(sfm_rotation_edge_test(eye, eye, rz, std::cos(0.19), &lhs) == 0 && std::fabs(lhs - (1 + 2 * c)) < 1e-15);
    EXPECT(sfm_rotation_edge_test(eye, eye, rz, std::cos(0.21), &lhs) == 1);
    double bad[9];
    std::memcpy(bad, eye, sizeof(bad));
    bad[4] = nan;
    EXPECT(sfm_rotation_edge_test(bad, eye, eye, 0.5, &lhs) == 0 && std::isnan(lhs));
    bad[4] = inf;
    EXPECT(sfm_rotation_edge_test(eye, eye, bad, 0.5, &lhs) == 0);
    EXPECT(sfm_rotation_edge_test(nullptr, eye, eye, 0.5, &lhs) == 0);
  }

  // ---- the batch plan
  {
    int batch = -1, n = -1;
    EXPECT(sfm_rotation_plan(12, 0, 0, &batch, &n) == SFM_OK && batch == 128 && n == 1);
    EXPECT(sfm_rotation_plan(12, 256, 24 * 12 * 72, &batch, &n) == SFM_OK && batch == 24 && n == 11);
    EXPECT(sfm_rotation_plan(1000, 128, 1, &batch, &n) == SFM_OK && batch == 1 && n == 128);            // never below one
    EXPECT(sfm_rotation_plan(1000, 65536, 0, &batch, &n) == SFM_OK && batch == 3728 && n == 18);
    EXPECT((long long)batch * 1000 * 72 <= (256LL << 20) && (long long)(batch + 1) * 1000 * 72 > (256LL << 20));
    EXPECT(sfm_rotation_plan(1, 16, 0, &batch, &n) == SFM_E_SHAPE && sfm_rotation_plan(12, -1, 0, &batch, &n) == SFM_E_SHAPE);
    EXPECT(sfm_rotation_plan(12, 65537, 0, &batch, &n) == SFM_E_SHAPE && sfm_rotation_plan(12, 16, -1, &batch, &n) == SFM_E_SHAPE);
    EXPECT(sfm_rotation_plan(12, 16, 0, nullptr, &n) == SFM_E_SHAPE && sfm_rotation_plan(12, 16, 0, &batch, nullptr) == SFM_E_SHAPE);
  }

  // ---- the argument path: these answers come before the library looks for a device
  const int V = 4, E = 5;
  const int edges[2 * E] = {0, 1, 1, 2, 2, 3, 3, 0, 0, 2};
  std::vector<double> rel(9 * E), R(9 * V, 7.0), cosv(E, 7.0);
  for (int e = 0; e < E; ++e) std::memcpy(&rel[9 * e], eye, sizeof(eye));
  std::vector<unsigned char> inl(E, 9);
  int view[V] = {-5, -5, -5, -5}, small[3] = {-5, -5, -5};
  int64_t summary[6] = {-1, -1, -1, -1, -1, -1};
  auto host = [&](int v, long long e, const int* ed, const double* rl, int root, double cm, int hyp, int iters, int steps, double tol, int cgm) {
    return sfm_rotation_average(v, e, ed, rl, root, cm, hyp, iters, steps, tol, cgm, R.data(), inl.data(), cosv.data(), view, small,
                                small + 1, small + 2, summary);
  };
  auto dev = [&](int v, long long e, const int* ed, const double* rl, int root, double cm, int hyp, int iters, int steps, double tol, int cgm) {
    return sfm_rotation_average_dev(v, e, ed, rl, root, cm, hyp, iters, steps, tol, cgm, R.data(), nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr);
  };
#define BOTH_REFUSE(...) EXPECT(host(__VA_ARGS__) == SFM_E_SHAPE && dev(__VA_ARGS__) == SFM_E_SHAPE)
  BOTH_REFUSE(1, E, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  BOTH_REFUSE(V, 0, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  BOTH_REFUSE(V, 1LL << 31, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  BOTH_REFUSE(V, 1LL << 30, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "E=") != nullptr);
  BOTH_REFUSE(V, E, edges, rel.data(), -1, 0.99, 16, 2, 2, 1e-12, 100);
  BOTH_REFUSE(V, E, edges, rel.data(), V, 0.99, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "root") != nullptr);
  for (double cm : {nan, 0.0, -0.5, 1.0000001, inf}) BOTH_REFUSE(V, E, edges, rel.data(), 0, cm, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "cos_max") != nullptr);
  for (int hyp : {-1, 65537}) BOTH_REFUSE(V, E, edges, rel.data(), 0, 0.99, hyp, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "max_hyp") != nullptr);
  BOTH_REFUSE(V, E, edges, rel.data(), 0, 0.99, 16, -1, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "iters") != nullptr);
  BOTH_REFUSE(V, E, edges, rel.data(), 0, 0.99, 16, 2, 0, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "steps") != nullptr);
  for (double tol : {nan, 0.0, 1.0, -1e-3}) BOTH_REFUSE(V, E, edges, rel.data(), 0, 0.99, 16, 2, 2, tol, 100);
  EXPECT(std::strstr(sfm_last_error(), "cg_tol") != nullptr);
  BOTH_REFUSE(V, E, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 0);
  EXPECT(std::strstr(sfm_last_error(), "cg_max") != nullptr);
  const int loop[2 * E] = {0, 1, 1, 2, 2, 2, 3, 0, 0, 2}, far[2 * E] = {0, 1, 1, 2, 2, 3, 3, 0, 0, 4}, neg[2 * E] = {0, -1, 1, 2, 2, 3, 3, 0, 0, 2};
  BOTH_REFUSE(V, E, loop, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "edge 2 ") != nullptr);
  BOTH_REFUSE(V, E, far, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "edge 4 ") != nullptr);
  BOTH_REFUSE(V, E, neg, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "edge 0 ") != nullptr);
  BOTH_REFUSE(V, E, nullptr, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);
  BOTH_REFUSE(V, E, edges, nullptr, 0, 0.99, 16, 2, 2, 1e-12, 100);
  EXPECT(std::strstr(sfm_last_error(), "null") != nullptr);
  EXPECT(sfm_rotation_average(V, E, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr) == SFM_E_SHAPE);                       // R_out is not optional
  {
    std::vector<double> stretched(rel);
    stretched[9 * 3 + 4] = 1.5;
    stretched[9 * 1 + 0] = 1.2;
    EXPECT(host(V, E, edges, stretched.data(), 0, 0.99, 16, 2, 2, 1e-12, 100) == SFM_E_BAD_ROTATION);
    EXPECT(std::strstr(sfm_last_error(), "edge 1 ") != nullptr);                       // the lowest such edge
  }
  if (sfm_init(0) == SFM_OK) {
    std::printf("host_check_rotavg: a device is present, the no-device path is not exercised\n");
    return failures == 0 ? 0 : 1;
  }
  const int rc = host(V, E, edges, rel.data(), 0, 0.99, 16, 2, 2, 1e-12, 100);          // valid arguments: the call goes on to look for a device
  EXPECT(rc != SFM_E_SHAPE && rc != SFM_E_BAD_ROTATION && rc != SFM_OK);
  const int rc_dev = dev(V, E, edges, rel.data(), 3, 1.0, 0, 0, 1, 0.5, 1);
  EXPECT(rc_dev != SFM_E_SHAPE && rc_dev != SFM_OK);
  for (double v : R) EXPECT(v == 7.0);                                                 // no output was touched anywhere above
  for (double v : cosv) EXPECT(v == 7.0);
  for (unsigned char v : inl) EXPECT(v == 9);
  for (int v : view) EXPECT(v == -5);
  for (int v : small) EXPECT(v == -5);
  for (int64_t v : summary) EXPECT(v == -1);
  if (failures == 0) std::printf("host_check_rotavg: ok (without a device the valid call returned %d)\n", rc);
  return failures == 0 ? 0 : 1;
}
