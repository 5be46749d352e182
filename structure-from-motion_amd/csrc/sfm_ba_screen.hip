// sfm_ba_screen.hip — screening and culling of the observations of a resident bundle-adjustment scene (gfx950).
//
// After an adjustment, every observation of the resident CSR is judged at the current state -- reprojection error,
// depth -- and every point by what is left of its track -- number of surviving observations, widest angle between two
// of their rays (sfm_hip.h, block "screening").  The residuals are the linearisation's: the projection is
// [R(q)^T | t] of the prepared cameras in track_project's operation order and the residual is track_residual's
// (sfm_obs_test.h), so the sum of err2 over a track is sfm_ba_refine_points' cost row 0 of that point.
//   screen   a group of G lanes owns a point, lane l takes observations l, l + G, ... in track order; one lane
//            evaluates an observation and writes err2 / depth / flags, the group counts the survivors and takes the
//            minimum of r_i . r_j over the surviving pairs with the rays staged in LDS
//   scan     one workgroup: exclusive scan of the per-point kept counts -> new pt_ptr, M' (read back by the host)
//   scatter  per point: the kept (cam_idx, u, v) in their old order at the new offsets
// No floating-point value is summed across lanes: err2 and depth come from one lane, min_cos is a minimum of products
// that commute, the counts are integers -- the outputs do not depend on G, on the other points or on timing.
#include <cmath>

#include "sfm_ba.h"
#include "sfm_scan.h"
#include "sfm_obs_test.h"      // contraction is off from here on

namespace sfm {

constexpr int kScrSlots = 6;        // rays per lane of the LDS tile: a track of up to 6 G observations is staged once
constexpr int kScrBlock = 256;

struct ScreenArgs {
  int N;
  const int* pt_ptr;
  const int* cam_idx;
  const double* u;
  const double* v;
  const CamPrep* prep;
  const double* px;
  const double* py;
  const double* pz;
  const double* cam_scale;      // [V] or null (= 1)
  double max_err2, cos_min_angle;
  int min_obs;
  double* err2;                 // [M]
  double* depth;                // [M]
  unsigned char* obs_flags;     // [M]
  double* min_cos;              // [N]
  int* pt_flags;                // [N]
  int* keep;                    // [N] observations the point keeps (0 for a dropped point)
  unsigned long long* summary;  // [8]; slots 2..7 are counted here, 0 and 1 by the scan
};

// Everything below is compiled WITHOUT automatic contraction (sfm_obs_test.h) and spells its FMAs out: every instantiation
// executes the same operations per observation.
struct ScreenObs { double err2, depth, r[3]; int flags; };

// One observation: obs_project_cam and obs_err2 (sfm_obs_test.h), the flags that say why it does not pass, the unit ray
// from the point to the camera centre.  r[0] is NaN for an observation that does not survive.
__device__ __forceinline__ void screen_obs(const CamPrep& c, double scale, double ku, double kv, double x0, double x1, double x2,
                                           double max_err2, ScreenObs& e) {
  double s[3];
  obs_project_cam(c, x0, x1, x2, s);
  e.err2 = obs_err2(s, ku, kv, scale);
  e.depth = s[2];
  e.flags = !isfinite(e.err2) ? SFM_OBS_NONFINITE : (e.err2 > max_err2 ? SFM_OBS_HIGH_ERROR : 0);
  if (s[2] <= 0.0) e.flags |= SFM_OBS_BEHIND;
  const double d0 = c.C[0] - x0, d1 = c.C[1] - x1, d2 = c.C[2] - x2;
  const double inv = rsqrt_nr(__builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0)));
  e.r[0] = e.flags ? __builtin_nan("") : d0 * inv;
  e.r[1] = d1 * inv;
  e.r[2] = d2 * inv;
}

// A track of up to kScrSlots * G observations has its rays staged by the evaluation pass itself and every lane reads
// its own rays back from the tile.  A longer one is staged tile by tile, and a lane forms the rays of its own
// observations again for every tile (the fallback: any length, nothing held per observation).
template <int G>
__global__ __launch_bounds__(kScrBlock) void ba_screen_kernel(ScreenArgs a) {
  constexpr int kCap = kScrSlots * G;
  __shared__ double tile_all[kScrBlock * kScrSlots * 3];
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)(t / G), lane = (int)(threadIdx.x % G);
  if (p >= a.N) return;                   // whole groups leave together
  double* tile = tile_all + (size_t)(threadIdx.x - lane) * kScrSlots * 3;      // kCap rays of this group
  const int beg = a.pt_ptr[p], end = a.pt_ptr[p + 1];
  const double x0 = a.px[p], x1 = a.py[p], x2 = a.pz[p];
  const bool one = end - beg <= kCap;
  ScreenObs e;

  int nk = 0, n_high = 0, n_behind = 0, n_nonfinite = 0;
  for (int o = beg + lane; o < end; o += G) {
    const int c = a.cam_idx[o];
    screen_obs(a.prep[c], a.cam_scale ? a.cam_scale[c] : 1.0, a.u[o], a.v[o], x0, x1, x2, a.max_err2, e);
    a.err2[o] = e.err2;
    a.depth[o] = e.depth;
    a.obs_flags[o] = (unsigned char)e.flags;
    nk += e.flags == 0;
    n_high += (e.flags & SFM_OBS_HIGH_ERROR) != 0;
    n_behind += (e.flags & SFM_OBS_BEHIND) != 0;
    n_nonfinite += (e.flags & SFM_OBS_NONFINITE) != 0;
    if (one) {
      double* w = tile + 3 * (o - beg);
      w[0] = e.r[0]; w[1] = e.r[1]; w[2] = e.r[2];
    }
  }
  nk = group_sum<G>(nk);
  group_lds_sync();

  double mc = 1.0;
  if (nk >= 2) {
    for (int tb = beg; tb < end; tb += kCap) {
      const int te = min(end, tb + kCap);
      if (!one) {
        for (int o = tb + lane; o < te; o += G) {
          const int c = a.cam_idx[o];
          screen_obs(a.prep[c], a.cam_scale ? a.cam_scale[c] : 1.0, a.u[o], a.v[o], x0, x1, x2, a.max_err2, e);
          double* w = tile + 3 * (o - tb);
          w[0] = e.r[0]; w[1] = e.r[1]; w[2] = e.r[2];
        }
        group_lds_sync();
      }
      for (int i = beg + lane; i < end; i += G) {
        double r0, r1, r2;
        if (one) {
          const double* w = tile + 3 * (i - beg);
          r0 = w[0]; r1 = w[1]; r2 = w[2];
        } else {
          const int c = a.cam_idx[i];
          screen_obs(a.prep[c], a.cam_scale ? a.cam_scale[c] : 1.0, a.u[i], a.v[i], x0, x1, x2, a.max_err2, e);
          r0 = e.r[0]; r1 = e.r[1]; r2 = e.r[2];
        }
        if (r0 != r0) continue;
        for (int j = tb; j < te; ++j) {
          const double* w = tile + 3 * (j - tb);
          const double q0 = w[0];
          if (j == i || q0 != q0) continue;
          mc = fmin(mc, __builtin_fma(r2, w[2], __builtin_fma(r1, w[1], r0 * q0)));
        }
      }
      if (!one) group_lds_sync();
    }
  }
  mc = group_min<G>(mc);

  int pf = 0;
  if (end == beg) {
    pf = SFM_PT_EMPTY;
  } else {
    if (nk < a.min_obs) pf |= SFM_PT_TOO_FEW;
    if (nk >= 2 && a.cos_min_angle < 1.0 && mc > a.cos_min_angle) pf |= SFM_PT_LOW_ANGLE;
  }
  const bool dropped = (pf & (SFM_PT_TOO_FEW | SFM_PT_LOW_ANGLE)) != 0;
  if (dropped) {
    for (int o = beg + lane; o < end; o += G)      // the lane's own stores, read back
      if (a.obs_flags[o] == 0) a.obs_flags[o] = SFM_OBS_POINT;
  }
  n_high = group_sum<G>(n_high);
  n_behind = group_sum<G>(n_behind);
  n_nonfinite = group_sum<G>(n_nonfinite);
  if (lane != 0) return;
  a.min_cos[p] = mc;
  a.pt_flags[p] = pf;
  a.keep[p] = dropped ? 0 : nk;
  if (n_high) atomicAdd(&a.summary[2], (unsigned long long)n_high);
  if (n_behind) atomicAdd(&a.summary[3], (unsigned long long)n_behind);
  if (n_nonfinite) atomicAdd(&a.summary[4], (unsigned long long)n_nonfinite);
  if (dropped && nk) atomicAdd(&a.summary[5], (unsigned long long)nk);
  if (pf & SFM_PT_TOO_FEW) atomicAdd(&a.summary[6], 1ULL);
  if (pf & SFM_PT_LOW_ANGLE) atomicAdd(&a.summary[7], 1ULL);
}

#pragma clang fp contract(on)

// Exclusive prefix sum of the kept counts (one workgroup); summary[0] = observations before, summary[1] = observations kept.
__global__ __launch_bounds__(kScanBlock) void ba_cull_scan_kernel(int N, const int* __restrict__ old_ptr, const int* __restrict__ keep,
                                                                  int* __restrict__ new_ptr, unsigned long long* __restrict__ summary) {
  block_exclusive_scan<1>(
      N, [&](int q, int (&a)[1]) { a[0] = keep[q]; }, [&](int q, const int (&e)[1]) { new_ptr[q] = e[0]; },
      [&](const int (&t)[1]) {
        new_ptr[N] = t[0];
        summary[0] = (unsigned long long)old_ptr[N];
        summary[1] = (unsigned long long)t[0];
      });
}

// One thread per point: the observations whose flags are clear, in their old order, to the new offsets.
__global__ void ba_cull_scatter_kernel(int N, const int* __restrict__ old_ptr, const int* __restrict__ old_cam,
                                       const double* __restrict__ old_u, const double* __restrict__ old_v,
                                       const unsigned char* __restrict__ obs_flags, const int* __restrict__ new_ptr,
                                       int* __restrict__ pt_ptr2, int* __restrict__ cam2, double* __restrict__ u2,
                                       double* __restrict__ v2) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  int w = new_ptr[p];
  const int we = new_ptr[p + 1];
  pt_ptr2[p] = w;
  if (p == N - 1) pt_ptr2[N] = we;
  for (int o = old_ptr[p]; o < old_ptr[p + 1] && w < we; ++o) {
    if (obs_flags[o] != 0) continue;
    cam2[w] = old_cam[o]; u2[w] = old_u[o]; v2[w] = old_v[o];
    ++w;
  }
}

template <int G>
static void launch_screen(const ScreenArgs& a, hipStream_t s) {
  const long long threads = (long long)a.N * G;
  ba_screen_kernel<G><<<dim3((unsigned)((threads + kScrBlock - 1) / kScrBlock)), dim3(kScrBlock), 0, s>>>(a);
}

int ba_screen_check_args(const char* who, double max_err2, double cos_min_angle, int min_obs, int group) {
  if (!(max_err2 >= 0.0)) { set_error("%s: max_err2 = %g must be >= 0 (+inf switches the test off)", who, max_err2); return SFM_E_SHAPE; }
  if (!(cos_min_angle >= -1.0)) { set_error("%s: cos_min_angle = %g must be >= -1 (>= 1 switches the test off)", who, cos_min_angle); return SFM_E_SHAPE; }
  if (min_obs < 0) { set_error("%s: min_obs = %d must be >= 0", who, min_obs); return SFM_E_SHAPE; }
  return group_width_check(who, group);
}

// Screen p's scene at its current state: enqueue, download what the caller asked for, wait.  The per-observation flags
// and the scanned offsets stay in w for a cull to scatter by; w.kept = M'.
int ba_screen_run(sfm_ba_problem* p, const char* who, double max_err2, double cos_min_angle, int min_obs, int group,
                  const double* cam_scale, double* err2, double* depth, unsigned char* obs_flags, double* min_cos,
                  int* pt_flags, int64_t* summary, ScreenWork& w) {
  SFM_TRY(ba_screen_check_args(who, max_err2, cos_min_angle, min_obs, group));
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  const BaDev& d = p->dev;
  hipStream_t s = p->stream;
  w.kept = d.M;
  if (summary) for (int k = 0; k < 8; ++k) summary[k] = 0;
  if (d.N == 0) return SFM_OK;
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));       // the expanded cameras the linearisation reads
  const size_t n = (size_t)d.N, m = (size_t)d.M;
  SFM_TRY(w.scale.upload_if(cam_scale, (size_t)d.V, s));
  if (cam_scale) p->upload_bytes += (long long)(sizeof(double) * d.V);
  SFM_TRY(w.err2.want(err2, m, s, true)); SFM_TRY(w.depth.want(depth, m, s, true)); SFM_TRY(w.flags.want(obs_flags, m, s, true));
  SFM_TRY(w.min_cos.want(min_cos, n, s, true)); SFM_TRY(w.pt_flags.want(pt_flags, n, s, true)); SFM_TRY(w.keep.alloc(n, s));
  SFM_TRY(w.new_ptr.alloc(n + 1, s)); SFM_TRY(w.summary.alloc(8, s));
  SFM_HIP(hipMemsetAsync(w.summary.p, 0, 8 * sizeof(unsigned long long), s));
  ScreenArgs a = {};
  a.N = d.N;
  a.pt_ptr = d.pt_ptr; a.cam_idx = d.cam_idx; a.u = d.u; a.v = d.v;
  a.prep = d.prep[p->cur];
  a.px = d.px; a.py = d.py; a.pz = d.pz;
  a.cam_scale = w.scale.p;
  a.max_err2 = max_err2; a.cos_min_angle = cos_min_angle; a.min_obs = min_obs;
  a.err2 = w.err2.dev(); a.depth = w.depth.dev(); a.obs_flags = w.flags.dev();
  a.min_cos = w.min_cos.dev(); a.pt_flags = w.pt_flags.dev(); a.keep = w.keep.p;
  a.summary = w.summary.p;
  dispatch_group<1>(group ? group : sfm_tri_tracks_auto_group(d.N, d.M, p->max_track),
                    [&](auto G) { launch_screen<decltype(G)::value>(a, s); });
  SFM_HIP(hipGetLastError());
  ba_cull_scan_kernel<<<1, kScanBlock, 0, s>>>(d.N, d.pt_ptr, w.keep.p, w.new_ptr.p, w.summary.p);
  SFM_HIP(hipGetLastError());
  unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  SFM_HIP(hipMemcpyAsync(sum, w.summary.p, sizeof(sum), hipMemcpyDeviceToHost, s));
  SFM_TRY(w.err2.fetch(s)); SFM_TRY(w.depth.fetch(s)); SFM_TRY(w.flags.fetch(s));
  SFM_TRY(w.min_cos.fetch(s)); SFM_TRY(w.pt_flags.fetch(s));
  SFM_TRY(ba_sync_cam_status(p, who, ""));
  if (summary) for (int k = 0; k < 8; ++k) summary[k] = (int64_t)sum[k];
  w.kept = (long long)sum[1];
  return SFM_OK;
}

// Fill of the culled scene e from d: the kept observations and the new pt_ptr.
int ba_cull_enqueue_scatter(const BaDev& d, const BaDev& e, const ScreenWork& w, hipStream_t s) {
  if (d.N <= 0) return SFM_OK;
  ba_cull_scatter_kernel<<<(d.N + 255) / 256, 256, 0, s>>>(d.N, d.pt_ptr, d.cam_idx, d.u, d.v, w.flags.dev(), w.new_ptr.p,
                                                           e.pt_ptr, e.cam_idx, e.u, e.v);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_ba_screen(sfm_ba_problem* p, double max_err2, double cos_min_angle, int min_obs, int group, const double* cam_scale,
                  double* err2, double* depth, unsigned char* obs_flags, double* min_cos, int* pt_flags, int64_t* summary) {
  SFM_TRY(ba_check_handle(p));
  ScreenWork w;
  return ba_screen_run(p, "sfm_ba_screen", max_err2, cos_min_angle, min_obs, group, cam_scale, err2, depth, obs_flags,
                       min_cos, pt_flags, summary, w);
}

}  // extern "C"
