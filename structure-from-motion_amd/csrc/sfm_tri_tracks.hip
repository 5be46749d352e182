// sfm_tri_tracks.hip — triangulation and structure-only refinement over RAGGED multi-view tracks (gfx950).
//
// The rectangular kernels of sfm_core.hip take uv[n_views][2][m]: every point seen in every view.  Here a point owns
// a CSR row of observations (pt_ptr / cam_idx / u / v, the layout of the resident bundle-adjustment scene and of
// sfm_obs_build) and is solved from exactly those:
//   linear     TriangulationProcessor.linear_triangulate (triangulation_processor.py:91-157) over the point's views,
//   nonlinear  TriangulationProcessor.nonlinear_triangulate (triangulation_processor.py:160-234) over the point's
//              views = the point half of BaProcessor.__execute_bundle_adjustment with delta_p = 0
//              (ba_processor.py:333, 355-359, 405):  X -= inv(sum Jx^T Jx + lambda I) sum Jx^T (f - b).
// A group of G lanes owns a point; lane l takes observations l, l + G, ... in track order, the nine normal-equation
// sums go through group_sum<G>, every lane of the group then holds the same bits and solves the 3x3 redundantly.
// No atomics, no LDS accumulation: a point's result is a function of its track, its input and G alone.
#include <climits>

#include "sfm_ba.h"
#include "sfm_dlt.h"

namespace sfm {

// first failure of the CSR check: info[0] = code, info[1] = index, info[2] = longest track
enum { kTrkPtr0 = 1, kTrkMonotone = 2, kTrkEnd = 3, kTrkCam = 4 };

__global__ void tracks_check_kernel(int n_pts, int n_views, long long M, const int* __restrict__ pt_ptr,
                                    const int* __restrict__ cam_idx, int* __restrict__ info) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  if (p == 0 && pt_ptr[0] != 0) report_status(info, kTrkPtr0, 0);
  if (p == n_pts - 1 && pt_ptr[n_pts] != M) report_status(info, kTrkEnd, n_pts);
  const int beg = pt_ptr[p], end = pt_ptr[p + 1];
  if (beg < 0 || end < beg || end > M) { report_status(info, kTrkMonotone, p); return; }
  for (int o = beg; o < end; ++o) {
    const int c = cam_idx[o];
    if (c < 0 || c >= n_views) { report_status(info, kTrkCam, o); break; }
  }
  atomicMax(&info[2], end - beg);
}

// [R^T | t] of every prepared camera as a row-major 3x4 projection (ba_processor.py:328)
__global__ void tracks_proj_from_prep_kernel(int V, const CamPrep* __restrict__ prep, double* __restrict__ projs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 12 * V) return;
  const CamPrep& c = prep[i / 12];
  const int r = (i % 12) / 4, k = i % 4;
  projs[i] = k < 3 ? c.R[3 * k + r] : c.t[r];
}

struct TrackArgs {
  TrackView t;
  double lambda;
  int iters;
  double* cost;             // [2][n_pts] or null
  int* status;              // [n_pts] or null
  int status_or;            // 1: OR into what the linear pass left in status, 0: overwrite
  int proj_in_lds;          // re-reading variant: stage the projections in LDS
};

// ---------------------------------------------------------------------------------------------
// Linear pass: one thread per point, the track's rows streamed through the Givens QR in the row order of
// tri_linear_kernel (per observation the u-row, then the v-row).  (Compiled with the default contraction, as
// tri_linear_kernel is: the same expressions give the same instructions.)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tri_tracks_linear_kernel(TrackArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.t.n_pts) return;
  const int beg = a.t.pt_ptr[p], end = a.t.pt_ptr[p + 1];
  double x[4] = {0, 0, 0, 1};
  if (a.t.xin[0]) {
    x[0] = a.t.xin[0][p]; x[1] = a.t.xin[1][p]; x[2] = a.t.xin[2][p];
    x[3] = a.t.xin[3] ? a.t.xin[3][p] : 1.0;
  }
  int flags = 0;
  if (end - beg < 2) {
    flags = SFM_TRACK_TOO_FEW;
  } else {
    double R[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int o = beg; o < end; ++o) {
      const double* P = a.t.projs + 12 * (size_t)a.t.cam_idx[o];
      const double u = a.t.u[o], w = a.t.v[o];
      dlt_add_row(R, u * P[8] - P[0], u * P[9] - P[1], u * P[10] - P[2], u * P[11] - P[3]);    // tri:145
      dlt_add_row(R, w * P[8] - P[4], w * P[9] - P[5], w * P[10] - P[6], w * P[11] - P[7]);    // tri:146
    }
    double y[4];
    dlt_null_vector(R, y);
    if (isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]) && isfinite(y[3])) {
      x[0] = y[0]; x[1] = y[1]; x[2] = y[2]; x[3] = y[3];
    } else {
      flags = SFM_TRACK_NONFINITE;
    }
  }
  a.t.xout[0][p] = x[0]; a.t.xout[1][p] = x[1]; a.t.xout[2][p] = x[2];
  if (a.t.xout[3]) a.t.xout[3][p] = x[3];
  if (a.status) a.status[p] = flags;
}

// ---------------------------------------------------------------------------------------------
// Nonlinear pass.  Everything below is compiled WITHOUT automatic contraction and spells its FMAs out: the cached and
// the re-reading instantiations then execute the same operations per observation, so a point's bits do not depend on
// which of them the longest track of a call selects.
// ---------------------------------------------------------------------------------------------
}  // namespace sfm

#include "sfm_track_obs.h"      // contraction is off from here on

namespace sfm {

constexpr int kTrkLdsViews = 512;     // projections staged in LDS by the re-reading variant up to here (48 KB)

// NC > 0: every lane keeps its (up to NC = 2, 4 or 6) observations -- u, v and the twelve projection entries -- in registers
// for all iterations; the host selects the smallest NC with G * NC >= the longest track of the call.  (A slot is skipped
// by a branch: computing every slot and selecting at the accumulation, to let the scheduler interleave the slots of a
// lane, measured 20 % slower.)  NC == 0: any length, observations
// re-read per iteration, projections from LDS (or through L2 beyond kTrkLdsViews cameras).
template <int G, int NC>
__global__ __launch_bounds__(256) void tri_tracks_nonlinear_kernel(TrackArgs a) {
  extern __shared__ double lds_proj[];
  if (NC == 0 && a.proj_in_lds) {
    for (int i = threadIdx.x; i < a.t.n_views * 12; i += blockDim.x) lds_proj[i] = a.t.projs[i];
    __syncthreads();
  }
  const double* P_all = (NC == 0 && a.proj_in_lds) ? lds_proj : a.t.projs;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)(t / G), lane = (int)(threadIdx.x % G);
  if (p >= a.t.n_pts) return;               // whole groups leave together
  const int beg = a.t.pt_ptr[p], end = a.t.pt_ptr[p + 1];
  const double in0 = a.t.xin[0][p], in1 = a.t.xin[1][p], in2 = a.t.xin[2][p];
  const double x3 = a.t.xin[3] ? a.t.xin[3][p] : 1.0;
  double x0 = in0, x1 = in1, x2 = in2;
  const bool eval = a.cost != nullptr || a.status != nullptr;
  double cost0 = 0, cost1 = 0, behind = 0;
  int flags = 0;

  constexpr int NR = NC > 0 ? NC : 1;
  double ku[NR], kv[NR], kP[NR][12];
  if (NC > 0) {
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int o = beg + lane + k * G;
      ku[k] = 0; kv[k] = 0;
#pragma unroll
      for (int i = 0; i < 12; ++i) kP[k][i] = 0;
      if (o < end) {
        ku[k] = a.t.u[o]; kv[k] = a.t.v[o];
        const double* P = a.t.projs + 12 * (size_t)a.t.cam_idx[o];
#pragma unroll
        for (int i = 0; i < 12; ++i) kP[k][i] = P[i];
      }
    }
  }

  if (end > beg) {
    for (int it = 0;; ++it) {
      const bool last = it >= a.iters;
      if (last && !eval) break;
      TrackSums S = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      double nb = 0;
      if (NC > 0) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
          if (beg + lane + k * G < end) {
            if (last) track_residual(kP[k], ku[k], kv[k], x0, x1, x2, x3, S.c, nb);
            else track_view(kP[k], ku[k], kv[k], x0, x1, x2, x3, S);
          }
        }
      } else {
        for (int o = beg + lane; o < end; o += G) {
          const double* P = P_all + 12 * (size_t)a.t.cam_idx[o];
          if (last) track_residual(P, a.t.u[o], a.t.v[o], x0, x1, x2, x3, S.c, nb);
          else track_view(P, a.t.u[o], a.t.v[o], x0, x1, x2, x3, S);
        }
      }
      if (last) {
        cost1 = group_sum<G>(S.c);
        behind = group_sum<G>(nb);
        if (it == 0) cost0 = cost1;
        break;
      }
      if (it == 0 && eval) cost0 = group_sum<G>(S.c);
      const double a00 = group_sum<G>(S.a00) + a.lambda, a10 = group_sum<G>(S.a10), a11 = group_sum<G>(S.a11) + a.lambda;
      const double a20 = group_sum<G>(S.a20), a21 = group_sum<G>(S.a21), a22 = group_sum<G>(S.a22) + a.lambda;
      const double b0 = group_sum<G>(S.b0), b1 = group_sum<G>(S.b1), b2 = group_sum<G>(S.b2);
      double d0, d1, d2;
      if (!track_solve3(a00, a10, a11, a20, a21, a22, b0, b1, b2, d0, d1, d2)) {      // the same bits on every lane of the group
        flags |= SFM_TRACK_NONFINITE;
        x0 = in0; x1 = in1; x2 = in2;
        it = a.iters - 1;                  // straight to the evaluation of the point as it came in
        continue;
      }
      x0 -= d0; x1 -= d1; x2 -= d2;
    }
    if (eval && !(isfinite(cost0) && isfinite(cost1))) flags |= SFM_TRACK_NONFINITE;
    if (behind > 0.0) flags |= SFM_TRACK_BEHIND;
  }

  if (lane != 0) return;
  a.t.xout[0][p] = x0; a.t.xout[1][p] = x1; a.t.xout[2][p] = x2;
  if (a.t.xout[3]) a.t.xout[3][p] = x3;
  if (a.cost) { a.cost[p] = cost0; a.cost[(size_t)a.t.n_pts + p] = cost1; }
  if (a.status) a.status[p] = a.status_or ? (a.status[p] | flags) : flags;
}

template <int G>
static void launch_tracks_g(const TrackArgs& a, int nc, hipStream_t s) {
  const long long threads = (long long)a.t.n_pts * G;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (nc == 2) tri_tracks_nonlinear_kernel<G, 2><<<grid, block, 0, s>>>(a);
  else if (nc == 4) tri_tracks_nonlinear_kernel<G, 4><<<grid, block, 0, s>>>(a);
  else if (nc == 6) tri_tracks_nonlinear_kernel<G, 6><<<grid, block, 0, s>>>(a);
  else tri_tracks_nonlinear_kernel<G, 0><<<grid, block, a.proj_in_lds ? sizeof(double) * 12 * (size_t)a.t.n_views : 0, s>>>(a);
}

// Automatic group width from n_pts, M and the longest track: the narrowest group whose lanes can
// keep the longest track in registers (6 observations each), widened while the call is too small to give every SIMD
// two waves and the wider group is still no wider than the longest track.
static int tracks_pick_group(int n_pts, long long M, int max_track) {
  (void)M;
  const int i = narrowest_group([&](int w) { return 6 * w >= max_track; });
  return kGroupWidths[widen_for_waves(i, n_pts, max_track)];
}

// Enqueue the requested passes on s.  The CSR has been validated; max_track is its longest track.
static int tracks_enqueue(TrackArgs a, int mode, int group, long long M, int max_track, hipStream_t s) {
  if (a.t.n_pts <= 0) return SFM_OK;
  if (mode & SFM_TRACKS_LINEAR) {
    tri_tracks_linear_kernel<<<(a.t.n_pts + 255) / 256, 256, 0, s>>>(a);
    SFM_HIP(hipGetLastError());
    for (int r = 0; r < 4; ++r) a.t.xin[r] = a.t.xout[r];      // the nonlinear pass starts from the DLT result
    a.status_or = 1;
  }
  if (mode & SFM_TRACKS_NONLINEAR) {
    const int g = group ? group : tracks_pick_group(a.t.n_pts, M, max_track);
    const int nc = max_track <= 2 * g ? 2 : (max_track <= 4 * g ? 4 : (max_track <= 6 * g ? 6 : 0));
    a.proj_in_lds = a.t.n_views <= kTrkLdsViews;
    dispatch_group<1>(g, [&](auto G) { launch_tracks_g<decltype(G)::value>(a, nc, s); });
    SFM_HIP(hipGetLastError());
  }
  return SFM_OK;
}

static int tracks_check_args(const char* who, int n_pts, int n_views, long long M, int mode, int iters, int group) {
  if (n_pts < 0 || n_views < 1 || M < 0 || M > INT_MAX || iters < 0) {
    set_error("%s: bad sizes n_pts=%d n_views=%d M=%lld iters=%d", who, n_pts, n_views, M, iters);
    return SFM_E_SHAPE;
  }
  if (mode < 1 || mode > (SFM_TRACKS_LINEAR | SFM_TRACKS_NONLINEAR)) { set_error("%s: bad mode %d", who, mode); return SFM_E_SHAPE; }
  return group_width_check(who, group);
}

// Validate the CSR on the device (the way ba_structure_kernel does) and wait for the verdict.
int tracks_validate(const char* who, int n_pts, int n_views, long long M, const int* d_pt_ptr, const int* d_cam_idx,
                    int* max_track, hipStream_t s) {
  DevBuf<int> dInfo;
  SFM_TRY(dInfo.alloc(4, s));
  SFM_HIP(hipMemsetAsync(dInfo.p, 0, 4 * sizeof(int), s));
  tracks_check_kernel<<<(n_pts + 255) / 256, 256, 0, s>>>(n_pts, n_views, M, d_pt_ptr, d_cam_idx, dInfo.p);
  SFM_HIP(hipGetLastError());
  int info[4] = {0, 0, 0, 0};
  SFM_TRY(dInfo.download(info, 4, s));
  SFM_TRY(stream_sync(s));
  *max_track = info[2];
  switch (info[0]) {
    case 0: return SFM_OK;
    case kTrkPtr0: set_error("%s: pt_ptr[0] is not 0", who); break;
    case kTrkMonotone: set_error("%s: pt_ptr not monotone at point %d", who, info[1]); break;
    case kTrkEnd: set_error("%s: pt_ptr[%d] is not M = %lld", who, info[1], M); break;
    default: set_error("%s: cam_idx[%d] out of range", who, info[1]); break;
  }
  return SFM_E_SHAPE;
}

TrackView track_view_free(int n_pts, int n_views, long long M, const int* pt_ptr, const int* cam_idx, const double* uv,
                          const double* projs, const double* X_init, double* X_out) {
  TrackView t = {n_pts, n_views, pt_ptr, cam_idx, uv, uv + M, projs, {}, {}};
  for (int r = 0; r < 4; ++r) {
    t.xin[r] = X_init ? X_init + (size_t)r * n_pts : nullptr;
    t.xout[r] = X_out + (size_t)r * n_pts;
  }
  return t;
}

int track_view_resident(sfm_ba_problem* p, DevBuf<double>& projs, TrackView* out) {
  const BaDev& d = p->dev;
  SFM_TRY(projs.alloc(12 * (size_t)d.V, p->stream));
  tracks_proj_from_prep_kernel<<<(12 * d.V + 255) / 256, 256, 0, p->stream>>>(d.V, d.prep[p->cur], projs.p);
  SFM_HIP(hipGetLastError());
  *out = TrackView{d.N, d.V, d.pt_ptr, d.cam_idx, d.u, d.v, projs.p, {d.px, d.py, d.pz, nullptr}, {d.px, d.py, d.pz, nullptr}};
  return SFM_OK;
}

int tracks_check_ptrs(const char* who, const char* what, long long M, const void* pt_ptr, const void* cam_idx, const void* uv,
                      const void* projs, const void* X_out) {
  if (pt_ptr && projs && X_out && (M == 0 || (cam_idx && uv))) return SFM_OK;
  set_error("%s: %s", who, what);
  return SFM_E_SHAPE;
}

// The checks of both free forms, in their order; their pointers are the host's or the device's.
static int tracks_check_free(const char* who, const char* null_what, int n_pts, int n_views, long long M, const void* pt_ptr,
                             const void* cam_idx, const void* uv, const void* projs, int mode, int iters, int group,
                             const void* X_init, const void* X_out) {
  SFM_TRY(tracks_check_args(who, n_pts, n_views, M, mode, iters, group));
  if (n_pts == 0) return SFM_OK;
  if (!(mode & SFM_TRACKS_LINEAR) && X_init == nullptr) { set_error("%s: X_init is required without SFM_TRACKS_LINEAR", who); return SFM_E_SHAPE; }
  return tracks_check_ptrs(who, null_what, M, pt_ptr, cam_idx, uv, projs, X_out);
}

// The one body of sfm_tri_tracks and sfm_tri_tracks_dev: checked arguments and device pointers in (n_pts > 0), the
// kernels enqueued on s out.
static int tracks_run(const char* who, int n_pts, int n_views, long long M, const int* d_pt_ptr, const int* d_cam_idx,
                      const double* d_uv, const double* d_projs, int mode, double lambda, int iters, int group,
                      const double* d_X_init, double* d_X_out, double* d_cost, int* d_status, hipStream_t s) {
  int max_track = 0;
  SFM_TRY(tracks_validate(who, n_pts, n_views, M, d_pt_ptr, d_cam_idx, &max_track, s));
  TrackArgs a = {};
  a.t = track_view_free(n_pts, n_views, M, d_pt_ptr, d_cam_idx, d_uv, d_projs, d_X_init, d_X_out);
  a.lambda = lambda; a.iters = iters;
  a.cost = d_cost; a.status = d_status;
  return tracks_enqueue(a, mode, group, M, max_track, s);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_tri_tracks_auto_group(int n_pts, int64_t M, int max_track) { return tracks_pick_group(n_pts, M, max_track); }

int sfm_tri_tracks_dev(int n_pts, int n_views, int64_t M, const int* d_pt_ptr, const int* d_cam_idx, const double* d_uv,
                       const double* d_projs, int mode, double lambda, int iters, int group, const double* d_X_init,
                       double* d_X_out, double* d_cost, int* d_status, void* hip_stream) {
  const char* who = "sfm_tri_tracks_dev";
  SFM_TRY(ensure_init());
  SFM_TRY(tracks_check_free(who, "null device pointer", n_pts, n_views, M, d_pt_ptr, d_cam_idx, d_uv, d_projs, mode, iters, group,
                            d_X_init, d_X_out));
  if (n_pts == 0) return SFM_OK;
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().stream;
  return tracks_run(who, n_pts, n_views, M, d_pt_ptr, d_cam_idx, d_uv, d_projs, mode, lambda, iters, group, d_X_init, d_X_out,
                    d_cost, d_status, s);
}

int sfm_tri_tracks(int n_pts, int n_views, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv,
                   const double* projs, int mode, double lambda, int iters, int group, const double* X_init, double* X_out,
                   double* cost, int* status) {
  const char* who = "sfm_tri_tracks";
  SFM_TRY(ensure_init());
  SFM_TRY(tracks_check_free(who, "null pointer", n_pts, n_views, M, pt_ptr, cam_idx, uv, projs, mode, iters, group, X_init, X_out));
  if (n_pts == 0) return SFM_OK;
  hipStream_t s = ctx().stream;
  const size_t n = (size_t)n_pts;
  DevBuf<int> dPtr, dCam;
  DevBuf<double> dUV, dP, dX;
  HostOut<double> oX, oCost;
  HostOut<int> oStatus;
  SFM_TRY(dPtr.upload(pt_ptr, n + 1, s));
  SFM_TRY(dCam.upload(cam_idx, (size_t)M, s));
  SFM_TRY(dUV.upload(uv, 2 * (size_t)M, s));
  SFM_TRY(dP.upload(projs, 12 * (size_t)n_views, s));
  SFM_TRY(dX.upload_if(X_init, 4 * n, s));
  SFM_TRY(oX.want(X_out, 4 * n, s)); SFM_TRY(oCost.want(cost, 2 * n, s)); SFM_TRY(oStatus.want(status, n, s));
  SFM_TRY(tracks_run(who, n_pts, n_views, M, dPtr.p, dCam.p, dUV.p, dP.p, mode, lambda, iters, group, dX.p, oX.dev(),
                     oCost.dev(), oStatus.dev(), s));
  SFM_TRY(oX.fetch(s)); SFM_TRY(oCost.fetch(s)); SFM_TRY(oStatus.fetch(s));
  return stream_sync(s);
}

int sfm_ba_refine_points(sfm_ba_problem* p, int mode, double lambda, int iters, int group, double* cost, int* status) {
  SFM_TRY(ba_check_handle(p));
  BaDev& d = p->dev;
  SFM_TRY(tracks_check_args("sfm_ba_refine_points", d.N, d.V > 0 ? d.V : 1, d.M, mode, iters, group));
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  if (d.N == 0 || d.M == 0) return SFM_OK;
  hipStream_t s = p->stream;
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));       // the expanded cameras the linearisation reads
  DevBuf<double> dP;
  HostOut<double> oCost;
  HostOut<int> oStatus;
  TrackArgs a = {};
  SFM_TRY(track_view_resident(p, dP, &a.t));
  SFM_TRY(oCost.want(cost, 2 * (size_t)d.N, s)); SFM_TRY(oStatus.want(status, (size_t)d.N, s));
  a.lambda = lambda; a.iters = iters;
  a.cost = oCost.dev(); a.status = oStatus.dev();
  SFM_TRY(tracks_enqueue(a, mode, group, d.M, p->max_track, s));
  SFM_TRY(ba_reset_stats(p));                            // new points, as after sfm_ba_set_points
  SFM_TRY(oCost.fetch(s)); SFM_TRY(oStatus.fetch(s));
  return ba_sync_cam_status(p, "sfm_ba_refine_points", "");
}

}  // extern "C"
