// sfm_ba_motion.hip — motion-only refinement of the resident scene: every camera from its own observations, points held
// (sfm_ba_refine_cameras; gfx950).
//
// The camera half of a bundle-adjustment iteration (ba_processor.py:382-392) with the point blocks dropped: per camera
//   U = sum Jp^T Jp (7x7),  g = sum Jp^T r,  dp = (U + lambda I)^-1 g,  cam += dp,  q /= |q|,  R(q), checks, q^ = q(R(q))
// over the camera's observations, r and Jp exactly those of ba_linearize (obs_terms_loss, sfm_ba_terms.h), optionally
// reweighted by the handle's robust loss.  Nothing couples two cameras, so there is no Schur complement and no reduced solve.
//
//   ba_cam_list_ensure     the scene's camera-major list (BaScene::cam_ptr, cam_obs; sfm_ba_host.hip), shared with the
//                          row-panel Schur product: ascending observation (= ascending point) inside a camera
//   ba_motion_resident<T>  one workgroup per camera of up to 256 (T = 64) or 1 024 (T = 256) observations: the observations
//                          stay in registers, all iterations run in one launch, every thread solves the same 7x7;
//                          STREAM: up to 16 384 observations, read again in every pass, 1 024 at a time
//   ba_motion_partial      cameras beyond 16 384 observations, one launch per pass: a workgroup sums 1 024 consecutive
//                          observations into 16 slice vectors
//   ba_motion_finish       ... and one wave per such camera adds the slice vectors in order, solves, updates, prepares
//
// Fixed summation order: a lane accumulates four consecutive observations, a 16-lane row folds to the 36 sums
// (U lower 28 | g 7 | cost) of a SLICE of 64 consecutive observations, slices are added in ascending order.  Which kernel
// a camera takes depends on its own observation count only (sfm_ba_refine_cameras_plan), so its result bits do not depend
// on the other cameras, the mask, the grid or timing.  There is no floating-point atomic in this file.
#include <algorithm>
#include <vector>

#include "sfm_ba.h"
#include "sfm_cam_fit.h"

namespace sfm {

constexpr int kMoWaveObs = 256;      // size class 1: one wave
constexpr int kMoBlockObs = 1024;    // size class 2: four waves; the larger classes work through 1 024 observations at a time
constexpr int kMoStreamObs = 16384;  // size class 3: one workgroup streams the camera's observations in every pass; beyond it
                                     // (class 4) a pass is spread over one workgroup per 1 024 observations and a second launch
constexpr int kMoDone = 1 << 30;     // internal status bit of the multi-launch path: the camera needs no further pass

// ---------------------------------------------------------------------------------------------
// The iteration
// ---------------------------------------------------------------------------------------------
struct MoArgs {
  CamObsView w;                 // the scene's camera-major list
  const unsigned char* mask;    // [V] or null
  double* cams;                 // [V][7]
  CamPrep* prep;                // [V] the prepared cameras of the current state
  double lambda;
  int iters, quirks;
  double* cost;                 // [2][V]
  int* status;                  // [V]
};

// One workgroup per camera of n_lo .. n_hi observations (the other size classes' launches skip it).  THREADS = 64 serves
// up to 256 observations, THREADS = 256 up to 1 024: a lane's four consecutive observations and their points stay in
// registers over all iterations.  STREAM (THREADS = 256): the camera is worked through in blocks of 1 024 observations,
// read again in every pass (they stay in L2), the 36 running totals carried from block to block by the threads that add
// the row partials -- the slices are still added in ascending order.  Pass `it` linearises at the current camera; pass 0
// yields cost row 0, the pass after the last update yields cost row 1 and SFM_CAM_BEHIND.  A held or empty camera stops
// after pass 0.
template <int THREADS, bool STREAM, int LOSS>
__global__ __launch_bounds__(THREADS) void ba_motion_resident_kernel(MoArgs a, int n_lo, int n_hi, LossArg<LOSS> la) {
  static_assert(!STREAM || THREADS * kMoPerLane == kMoBlockObs, "a streamed block is one round of the workgroup");
  constexpr int ROWS = THREADS / 16;
  __shared__ double red[ROWS][kMoSums];
  __shared__ double sums[kMoSums];
  const int cam = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  if (n < n_lo || n > n_hi) return;
  const bool held = a.mask != nullptr && a.mask[cam] == 0;
  const int my_iters = (held || n == 0) ? 0 : a.iters;
  MoObs ob[kMoPerLane];
  if (!STREAM) {
#pragma unroll
    for (int k = 0; k < kMoPerLane; ++k)
      if (kMoPerLane * tid + k < n) cam_obs_load(a.w, cam, base + kMoPerLane * tid + k, ob[k]);
  }
  const int n_blocks = STREAM ? (n + kMoBlockObs - 1) / kMoBlockObs : 1;
  int own[3];
  mo_fold_own(lane, own);
  CamPrep c;
  load_cam(c, a.prep + cam);
  double params[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) params[k] = a.cams[7 * (size_t)cam + k];
  int flags = (held ? SFM_CAM_HELD : 0) | (n == 0 ? SFM_CAM_EMPTY : 0);
  double cost0 = 0, cost1 = 0;
  for (int it = 0;; ++it) {
    int behind = 0, any_behind = 0;
    double run = 0;                                           // threads 0 .. 35: the running total of their sum
    for (int blk = 0; blk < n_blocks; ++blk) {
      double acc[kMoSums];
#pragma unroll
      for (int k = 0; k < kMoSums; ++k) acc[k] = 0;
#pragma unroll
      for (int k = 0; k < kMoPerLane; ++k) {
        const int i = blk * kMoBlockObs + kMoPerLane * tid + k;
        if (i < n) {
          if (STREAM) cam_obs_load(a.w, cam, base + i, ob[k]);
          mo_accumulate<LOSS>(c, ob[k], a.quirks, la, acc, behind);
        }
      }
      mo_fold_row(acc, own, lane, red[tid >> 4]);
      const bool last = blk == n_blocks - 1;                  // (uniform over the workgroup)
      if (last) any_behind = __syncthreads_or(behind);
      else __syncthreads();
      if (tid < kMoSums) {
        double t = blk == 0 ? red[0][tid] : run + red[0][tid];
#pragma unroll
        for (int w = 1; w < ROWS; ++w) t += red[w][tid];      // slice order; the rows beyond the camera's slices hold zeros
        run = t;
        if (last) sums[tid] = t;
      }
      __syncthreads();                                        // sums complete / red free for the next block
    }
    // from here on every thread holds the same values: the branches are uniform
    const double chk = mo_finite_probe(sums, kMoSums);
    if (it == 0) cost0 = sums[35];
    if (!(chk == 0.0)) { flags |= SFM_CAM_NONFINITE; cost1 = cost0; break; }
    if (it == my_iters) {
      cost1 = sums[35];
      if (any_behind) flags |= SFM_CAM_BEHIND;
      break;
    }
    if (!mo_step(sums, a.lambda, params, c)) { flags |= SFM_CAM_NONFINITE; cost1 = cost0; break; }
    // (the next pass writes red after this pass' last read of it, and sums only behind its first barrier)
  }
  if (tid == 0) {
    if (my_iters > 0 && !(flags & SFM_CAM_NONFINITE)) {
#pragma unroll
      for (int k = 0; k < 7; ++k) a.cams[7 * (size_t)cam + k] = params[k];
    }
    a.cost[cam] = cost0;
    a.cost[(size_t)a.w.V + cam] = cost1;
    a.status[cam] = flags;
  }
}

// Cameras of more than n_min observations, one pass: workgroup (camera, block) sums observations [1024 block, +1024) of the
// camera's list at the prepared camera into one 36-vector per slice.
template <int LOSS>
__global__ __launch_bounds__(256) void ba_motion_partial_kernel(MoArgs a, int n_min, double* __restrict__ ws,
                                                                int* __restrict__ behind_flag, LossArg<LOSS> la) {
  __shared__ double red[16][kMoSums];
  const int cam = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  if (n <= n_min || (long long)blk * kMoBlockObs >= n) return;
  if (a.status[cam] & kMoDone) return;
  int own[3];
  mo_fold_own(lane, own);
  CamPrep c;
  load_cam(c, a.prep + cam);
  double acc[kMoSums];
#pragma unroll
  for (int k = 0; k < kMoSums; ++k) acc[k] = 0;
  int behind = 0;
#pragma unroll
  for (int k = 0; k < kMoPerLane; ++k) {
    const int i = blk * kMoBlockObs + kMoPerLane * tid + k;
    if (i < n) {
      MoObs ob;
      cam_obs_load(a.w, cam, base + i, ob);
      mo_accumulate<LOSS>(c, ob, a.quirks, la, acc, behind);
    }
  }
  mo_fold_row(acc, own, lane, red[tid >> 4]);
  const int any_behind = __syncthreads_or(behind);
  if (any_behind && tid == 0) atomicOr(&behind_flag[cam], 1);
  const int n_slices = cam_slice_count(n);
  const int rows = min(16, n_slices - blk * 16);
  double* dst = ws + (cam_slice_first_row(base, cam) + (size_t)blk * 16) * kMoSums;
  const double* src = &red[0][0];
  for (int i = tid; i < rows * kMoSums; i += 256) dst[i] = src[i];
}

// ... and its second half, one wave per camera: the slice vectors added in slice order, then what ba_motion_resident does
// with the sums of pass `it`.  The camera and its prepared form travel through a.cams / a.prep between the passes;
// cams_in restores a camera that turns non-finite.
__global__ __launch_bounds__(64) void ba_motion_finish_kernel(MoArgs a, int n_min, const double* __restrict__ ws,
                                                              int* __restrict__ behind_flag, const double* __restrict__ cams_in, int it) {
  __shared__ double sums[kMoSums];
  const int cam = blockIdx.x, tid = threadIdx.x;
  const int base = a.w.ptr[cam], n = a.w.ptr[cam + 1] - base;
  if (n <= n_min) return;
  if (a.status[cam] & kMoDone) return;
  const int n_slices = cam_slice_count(n);
  if (tid < kMoSums) {
    const double* part = ws + cam_slice_first_row(base, cam) * kMoSums + tid;
    double t = part[0];
    for (int s = 1; s < n_slices; ++s) t += part[(size_t)s * kMoSums];
    sums[tid] = t;
  }
  __syncthreads();
  const bool held = a.mask != nullptr && a.mask[cam] == 0;
  const int my_iters = held ? 0 : a.iters;
  const int flags = held ? SFM_CAM_HELD : 0;
  const double chk = mo_finite_probe(sums, kMoSums);
  const double cost0 = it == 0 ? sums[35] : a.cost[cam];
  bool ok = chk == 0.0;
  if (ok && it == my_iters) {
    if (tid == 0) {
      if (it == 0) a.cost[cam] = cost0;
      a.cost[(size_t)a.w.V + cam] = sums[35];
      a.status[cam] = flags | (behind_flag[cam] ? SFM_CAM_BEHIND : 0) | kMoDone;
      behind_flag[cam] = 0;
    }
    return;
  }
  double params[7];
  CamPrep c;
  if (ok) {
#pragma unroll
    for (int k = 0; k < 7; ++k) params[k] = a.cams[7 * (size_t)cam + k];
    ok = mo_step(sums, a.lambda, params, c);
  }
  if (tid != 0) return;
  behind_flag[cam] = 0;
  if (it == 0) a.cost[cam] = cost0;
  if (ok) {
#pragma unroll
    for (int k = 0; k < 7; ++k) a.cams[7 * (size_t)cam + k] = params[k];
    a.prep[cam] = c;
  } else {
    for (int k = 0; k < 7; ++k) a.cams[7 * (size_t)cam + k] = cams_in[7 * (size_t)cam + k];
    a.cost[(size_t)a.w.V + cam] = cost0;
    a.status[cam] = flags | SFM_CAM_NONFINITE | kMoDone;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int mo_size_class(long long n) {
  return n <= 0 ? 0 : (n <= kMoWaveObs ? 1 : (n <= kMoBlockObs ? 2 : (n <= kMoStreamObs ? 3 : 4)));
}

// SFM_OPT_DEBUG bit 32768 (measurement only): cameras of size class 3 take class 4's launches
static int mo_enqueue(sfm_ba_problem* p, const MoArgs& a, int loss_kind, const int (&n_class)[5], int max_obs, DevBuf<double>& ws,
                      DevBuf<int>& behind, DevBuf<double>& cams_in) {
  return dispatch_loss(loss_kind, [&](auto L) -> int {
    constexpr int LOSS = decltype(L)::value;
    const BaDev& d = p->dev;
    hipStream_t s = p->stream;
    const LossArg<LOSS> la = loss_arg<LOSS>(p);
    const bool stream3 = !(p->debug & 32768);
    const int n_min = stream3 ? kMoStreamObs : kMoBlockObs;      // the multi-launch path takes the cameras beyond it
    if (n_class[0] + n_class[1] > 0)
      ba_motion_resident_kernel<64, false, LOSS><<<d.V, 64, 0, s>>>(a, 0, kMoWaveObs, la);
    if (n_class[2] > 0)
      ba_motion_resident_kernel<256, false, LOSS><<<d.V, 256, 0, s>>>(a, kMoWaveObs + 1, kMoBlockObs, la);
    if (n_class[3] > 0 && stream3)
      ba_motion_resident_kernel<256, true, LOSS><<<d.V, 256, 0, s>>>(a, kMoBlockObs + 1, kMoStreamObs, la);
    if (n_class[4] > 0 || (n_class[3] > 0 && !stream3)) {
      SFM_TRY(ws.alloc(cam_slice_rows(d.M, d.V) * kMoSums, s));
      SFM_TRY(behind.alloc((size_t)d.V, s));
      SFM_TRY(cams_in.alloc(7 * (size_t)d.V, s));
      SFM_HIP(hipMemsetAsync(behind.p, 0, sizeof(int) * (size_t)d.V, s));
      SFM_HIP(hipMemcpyAsync(cams_in.p, d.cams, sizeof(double) * 7 * d.V, hipMemcpyDeviceToDevice, s));
      const dim3 grid((unsigned)d.V, (unsigned)((max_obs + kMoBlockObs - 1) / kMoBlockObs));
      for (int it = 0; it <= a.iters; ++it) {
        ba_motion_partial_kernel<LOSS><<<grid, 256, 0, s>>>(a, n_min, ws.p, behind.p, la);
        ba_motion_finish_kernel<<<d.V, 64, 0, s>>>(a, n_min, ws.p, behind.p, cams_in.p, it);
      }
    }
    SFM_HIP(hipGetLastError());
    return SFM_OK;
  });
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_ba_refine_cameras_plan(int64_t n_obs, int* n_slices, int* slice_obs, int* size_class) {
  if (n_obs < 0) { set_error("sfm_ba_refine_cameras_plan: n_obs < 0"); return SFM_E_SHAPE; }
  if (n_slices) *n_slices = (int)cam_slice_count(n_obs);
  if (slice_obs) *slice_obs = kCamSlice;
  if (size_class) *size_class = mo_size_class(n_obs);
  return SFM_OK;
}

int sfm_ba_refine_cameras(sfm_ba_problem* p, double lambda, int iters, int quirks, int use_loss, const unsigned char* cam_mask,
                          double* cost, int* status) {
  SFM_TRY(ba_check_handle(p));
  if (iters < 0) { set_error("sfm_ba_refine_cameras: iters < 0"); return SFM_E_SHAPE; }
  if (!(lambda >= 0)) { set_error("sfm_ba_refine_cameras: lambda must be >= 0"); return SFM_E_SHAPE; }
  if (use_loss != 0 && use_loss != 1) { set_error("sfm_ba_refine_cameras: use_loss must be 0 or 1"); return SFM_E_SHAPE; }
  SFM_TRY(ba_refuse_comm(p, "sfm_ba_refine_cameras", "the points are sharded; the replicas would diverge"));
  BaDev& d = p->dev;
  const int V = d.V;
  SFM_TRY(ba_flush(p));                                  // a deferred back substitution still owes the points its update
  if (d.N == 0 || d.M == 0) {                            // nothing to fit: every camera is empty
    for (int c = 0; c < V; ++c) {
      if (cost) cost[c] = cost[(size_t)V + c] = 0.0;
      if (status) status[c] = SFM_CAM_EMPTY | ((cam_mask && cam_mask[c] == 0) ? SFM_CAM_HELD : 0);
    }
    return SFM_OK;
  }
  hipStream_t s = p->stream;
  SFM_TRY(ba_prepared_cameras(p, "sfm_ba_refine_cameras"));
  SFM_TRY(ba_cam_list_ensure(p));
  int n_class[5] = {0, 0, 0, 0, 0}, max_obs = 0;
  for (int c = 0; c < V; ++c) {
    const int n = p->h_cam_ptr[c + 1] - p->h_cam_ptr[c];
    ++n_class[mo_size_class(n)];
    max_obs = std::max(max_obs, n);
  }
  if ((max_obs + kMoBlockObs - 1) / kMoBlockObs > 65535) {
    set_error("sfm_ba_refine_cameras: a camera of %d observations is beyond the launch grid", max_obs);
    return SFM_E_SHAPE;
  }
  DevBuf<unsigned char> dmask;
  DevBuf<double> ws, cams_in;
  DevBuf<int> behind;
  HostOut<double> ocost;      // the kernels carry both through their iterations, wanted or not
  HostOut<int> ostat;
  SFM_TRY(dmask.upload_if(cam_mask, (size_t)V, s));
  if (cam_mask) p->upload_bytes += V;
  SFM_TRY(ocost.want(cost, 2 * (size_t)V, s, true));
  SFM_TRY(ostat.want(status, (size_t)V, s, true));
  SFM_HIP(hipMemsetAsync(ostat.dev(), 0, sizeof(int) * (size_t)V, s));
  MoArgs a = {};
  a.w = cam_obs_view_resident(p, nullptr); a.mask = dmask.p; a.cams = d.cams; a.prep = d.prep[p->cur];
  a.lambda = lambda; a.iters = iters; a.quirks = quirks;
  a.cost = ocost.dev(); a.status = ostat.dev();
  SFM_TRY(mo_enqueue(p, a, use_loss ? p->loss_kind : SFM_LOSS_NONE, n_class, max_obs, ws, behind, cams_in));
  SFM_TRY(ba_state_changed(p));                          // new cameras
  SFM_TRY(ocost.fetch(s));
  SFM_TRY(ostat.fetch(s));
  SFM_TRY(stream_sync(s));
  if (status)
    for (int c = 0; c < V; ++c) status[c] &= ~kMoDone;
  return SFM_OK;
}

}  // extern "C"
