// sfm_ba_host.hip — the device-resident bundle-adjustment problem object behind the C-ABI (gfx950).
//
// Host side of BaProcessor.__execute_bundle_adjustment (ba_processor.py:274-439) and of its caller, the
// per-view loop of BaProcessor.process (ba_processor.py:137-267): create / destroy, state upload and
// download, growing a resident scene in place (sfm_ba_append), the multi-GPU split, parity hooks.
//
// Everything that scales with the scene is built ON THE DEVICE: the host uploads the caller's CSR as it is
// (one copy per array) and ba_structure_kernel validates it, derives obs_pt, the per-point 18-camera block
// offsets of the sparse Schur product and the longest track (and, on first use, the ba_cam_list_* chain the
// camera-major list of the row-panel product and the motion-only refinement); sfm_ba_append uploads only the NEW cameras,
// points and observations and merges them into the (point, camera)-sorted list with a count / scan /
// bucket / merge kernel chain.  The host never loops over observations.
#include <algorithm>
#include <vector>

#include "sfm_ba.h"
#include "sfm_ba_terms.h"
#include "sfm_scan.h"

namespace sfm {

// ---------------------------------------------------------------------------------------------
// Structure check + derived index arrays, one thread per point.
// sinfo[0] = first failure code (1 pt_ptr not monotone, 2 camera out of range, 3 cameras of a track not strictly
// increasing), sinfo[1] = its index (point, observation, point), sinfo[2] = longest track.
// ---------------------------------------------------------------------------------------------
__global__ void ba_structure_kernel(int V, int N, long long M, const int* __restrict__ pt_ptr,
                                    const int* __restrict__ cam_idx, int* __restrict__ obs_pt,
                                    int* __restrict__ blk_ptr, int nblk, int* __restrict__ sinfo) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int beg = pt_ptr[p], end = pt_ptr[p + 1];
  int* row = blk_ptr + (size_t)p * (nblk + 1);
  if (beg < 0 || end < beg || end > M) {
    report_status(sinfo, 1, p);
    for (int b = 0; b <= nblk; ++b) row[b] = 0;
    return;
  }
  int prev = -1, b = 0;
  for (int o = beg; o < end; ++o) {
    const int c = cam_idx[o];
    if (c < 0 || c >= V) { report_status(sinfo, 2, o); continue; }
    if (c <= prev) report_status(sinfo, 3, p);
    prev = c;
    obs_pt[o] = p;
    while (b < nblk && c >= b * kSchurCB) row[b++] = o;      // first observation whose camera is >= 18 b
  }
  while (b <= nblk) row[b++] = end;
  atomicMax(&sinfo[2], end - beg);
}

// ---------------------------------------------------------------------------------------------
// The camera-major observation list (cam_ptr, cam_obs), once per scene.  The resident observations are sorted by
// (point, camera), so ascending observation index inside a camera IS ascending point: the order is fixed.
//   count       per observation: counts per (chunk of observations, camera)
//   chunk_scan  per camera: a scan over its chunks
//   ptr_scan    one workgroup: a scan over the cameras
//   fill        one wave per chunk hands out the slots in observation order
// ---------------------------------------------------------------------------------------------
__global__ void ba_cam_list_count_kernel(long long M, int V, int chunk_obs, const int* __restrict__ cam_idx, int* __restrict__ table) {
  const long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (o >= M) return;
  atomicAdd(&table[(size_t)(o / chunk_obs) * V + cam_idx[o]], 1);      // integer: the counts do not depend on the order
}

// per camera: counts of its chunks -> their exclusive prefix (the chunk's first slot inside the camera), and the total
__global__ void ba_cam_list_chunk_scan_kernel(int V, int nchunks, int* __restrict__ table, int* __restrict__ cnt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= V) return;
  int off = 0;
  for (int k = 0; k < nchunks; ++k) {
    const int t = table[(size_t)k * V + c];
    table[(size_t)k * V + c] = off;
    off += t;
  }
  cnt[c] = off;
}

__global__ __launch_bounds__(kScanBlock) void ba_cam_list_ptr_scan_kernel(int V, const int* __restrict__ cnt, int* __restrict__ ptr) {
  block_exclusive_scan<1>(
      V, [&](int q, int (&a)[1]) { a[0] = cnt[q]; }, [&](int q, const int (&e)[1]) { ptr[q] = e[0]; },
      [&](const int (&t)[1]) { ptr[V] = t[0]; });
}

// One wave per chunk, 64 observations at a time: a lane's slot is the chunk's running offset of its camera (fetched and
// advanced by the first lane of that camera, the only writer of the chunk's table row) plus the number of lower lanes with
// the same camera.
__global__ __launch_bounds__(64) void ba_cam_list_fill_kernel(long long M, int V, int chunk_obs, const int* __restrict__ cam_idx,
                                                              const int* __restrict__ ptr, int* __restrict__ table, int* __restrict__ list) {
  const int lane = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * chunk_obs, o1 = min(M, o0 + chunk_obs);
  int* row = table + (size_t)blockIdx.x * V;
  for (long long ob = o0; ob < o1; ob += 64) {
    const long long o = ob + lane;
    const bool live = o < o1;
    const int c = live ? cam_idx[o] : -1 - lane;          // idle lanes: cameras of their own
    int rank = 0, total = 0, lead = lane;
    for (int j = 63; j >= 0; --j) {
      const int cj = __shfl(c, j, 64);
      if (cj == c) { ++total; lead = j; if (j < lane) ++rank; }
    }
    int first = 0;
    if (live && rank == 0) first = atomicAdd(&row[c], total);
    first = __shfl(first, lead, 64);
    if (live) list[ptr[c] + first + rank] = (int)o;
  }
}

// ---------------------------------------------------------------------------------------------
// sfm_ba_append on the device.  New observation k = (obs_cam[k], obs_pt[k], u_new[k], v_new[k]).
//   count   per new observation: range check, cnt[point]++
//   scan    one workgroup: new_ptr = exclusive scan of (old track length + cnt), nstart = exclusive scan of cnt
//   bucket  per new observation: its slot in its point's bucket (order inside a bucket is fixed by the merge's sort)
//   merge   per point: sort the bucket by camera, merge with the old (sorted) track -> cam2 / u2 / v2
// Duplicates (a pair already present) survive the merge as equal neighbours and are caught by
// ba_structure_kernel's strictly-increasing check.
// ---------------------------------------------------------------------------------------------
__global__ void ba_append_count_kernel(long long n, int V2, int N2, const int* __restrict__ obs_cam,
                                       const int* __restrict__ obs_pt, int* __restrict__ cnt, int* __restrict__ sinfo) {
  const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int c = obs_cam[k], q = obs_pt[k];
  if (c < 0 || c >= V2 || q < 0 || q >= N2) { report_status(sinfo, 4, (int)k); return; }
  atomicAdd(&cnt[q], 1);
}

// exclusive prefix sums of two integer sequences in one pass (one workgroup): old track length + cnt, and cnt
__global__ __launch_bounds__(kScanBlock) void ba_append_scan_kernel(int N, int N2, const int* __restrict__ old_ptr,
                                                                    const int* __restrict__ cnt, int* __restrict__ new_ptr,
                                                                    int* __restrict__ nstart) {
  block_exclusive_scan<2>(
      N2,
      [&](int q, int (&a)[2]) {
        a[1] = cnt[q];
        a[0] = a[1] + (q < N ? old_ptr[q + 1] - old_ptr[q] : 0);
      },
      [&](int q, const int (&e)[2]) { new_ptr[q] = e[0]; nstart[q] = e[1]; },
      [&](const int (&t)[2]) { new_ptr[N2] = t[0]; nstart[N2] = t[1]; });
}

__global__ void ba_append_bucket_kernel(long long n, const int* __restrict__ obs_pt, const int* __restrict__ nstart,
                                        int* __restrict__ fill, int* __restrict__ norder) {
  const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int q = obs_pt[k];
  norder[nstart[q] + atomicAdd(&fill[q], 1)] = (int)k;
}

__global__ void ba_append_merge_kernel(int N, int N2, const int* __restrict__ old_ptr, const int* __restrict__ old_cam,
                                       const double* __restrict__ old_u, const double* __restrict__ old_v,
                                       const int* __restrict__ new_ptr, const int* __restrict__ nstart,
                                       int* __restrict__ norder, const int* __restrict__ obs_cam,
                                       const double* __restrict__ u_new, const double* __restrict__ v_new,
                                       int* __restrict__ cam2, double* __restrict__ u2, double* __restrict__ v2) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= N2) return;
  const int nb = nstart[q], ne = nstart[q + 1];
  for (int i = nb + 1; i < ne; ++i) {                 // insertion sort of the (short) bucket by camera
    const int k = norder[i], c = obs_cam[k];
    int j = i - 1;
    while (j >= nb && obs_cam[norder[j]] > c) { norder[j + 1] = norder[j]; --j; }
    norder[j + 1] = k;
  }
  int o = q < N ? old_ptr[q] : 0;
  const int oe = q < N ? old_ptr[q + 1] : 0;
  int i = nb, w = new_ptr[q];
  while (o < oe || i < ne) {
    const int co = o < oe ? old_cam[o] : 0x7fffffff;
    const int cn = i < ne ? obs_cam[norder[i]] : 0x7fffffff;
    if (co <= cn) { cam2[w] = co; u2[w] = old_u[o]; v2[w] = old_v[o]; ++o; }
    else { const int k = norder[i]; cam2[w] = cn; u2[w] = u_new[k]; v2[w] = v_new[k]; ++i; }
    ++w;
  }
}

// sfm_ba_sync_tracks: is every resident track a subsequence of the track the store built for the same point, with the same
// bits in u and v?  One thread per resident point walks both camera-sorted tracks; the first point that fails goes
// into *first_bad by an unsigned atomicMin (the word starts as all ones).
__global__ void ba_tracks_compare_kernel(int N, const int* __restrict__ old_ptr, const int* __restrict__ old_cam,
                                         const double* __restrict__ old_u, const double* __restrict__ old_v,
                                         const int* __restrict__ new_ptr, const int* __restrict__ new_cam,
                                         const double* __restrict__ new_u, const double* __restrict__ new_v,
                                         unsigned* __restrict__ first_bad) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  int i = new_ptr[p];
  const int ne = new_ptr[p + 1];
  bool ok = true;
  for (int o = old_ptr[p]; o < old_ptr[p + 1] && ok; ++o) {
    const int c = old_cam[o];
    while (i < ne && new_cam[i] < c) ++i;
    ok = i < ne && new_cam[i] == c && __double_as_longlong(new_u[i]) == __double_as_longlong(old_u[o]) &&
         __double_as_longlong(new_v[i]) == __double_as_longlong(old_v[o]);
    ++i;
  }
  if (!ok) atomicMin(first_bad, (unsigned)p);
}

// The reference packs every camera anew at the start of each BA call: q = convert_rotation_to_quaternion(view.rot)
// (ba_processor.py:285-288), and view.rot is R(q) of the previous call's result (ba:412) -- so the quaternion a call starts
// from is q(R(q_prev)), not q_prev.  For cameras the caller did not touch, that round trip is done here, on the device, from
// the R(q) and canonical q the camera expansion holds: nothing crosses PCIe.
__global__ void ba_rederive_quat_kernel(int first, int count, const CamPrep* __restrict__ prep, double* __restrict__ cams) {
  const int c = first + blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= first + count) return;
  for (int k = 0; k < 4; ++k) cams[7 * c + 3 + k] = prep[c].q[k];
}

// The scene moved by a similarity X' = s A X + t (sfm_ba_transform, sfm_ba_align): sim = (s, A row-major, t) in device
// memory, so that a model an estimator left there is applied without coming down.  `gate`, if not null, is that
// estimator's status word: without a model (bit 1 or 2) both kernels do nothing.
constexpr unsigned long long kTransformClean = ~0ULL;
__device__ __forceinline__ bool ba_transform_gated(const int* gate) { return gate != nullptr && (*gate & 3) != 0; }

__device__ __forceinline__ void ba_transform_point(const double* sim, double x, double y, double z, double* out) {
  const double s = sim[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = s * (sim[1 + 3 * i] * x + sim[2 + 3 * i] * y + sim[3 + 3 * i] * z) + sim[10 + i];
}

// First the cameras, into work[V][7]: C' = s A C + t, q' = q(A R(q)).  A camera whose quaternion fails leaves
// (camera << 3 | -status) in *fail, the lowest camera winning.
__global__ void ba_transform_cams_kernel(int V, const double* __restrict__ cams, const double* __restrict__ sim,
                                         const int* __restrict__ gate, double* __restrict__ work, unsigned long long* fail) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= V || ba_transform_gated(gate)) return;
  double R[9], AR[9], q[4] = {0, 0, 0, 0}, C[3];
  quat_to_rot(cams + 7 * c + 3, R);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) AR[3 * i + j] = sim[1 + 3 * i] * R[j] + sim[2 + 3 * i] * R[3 + j] + sim[3 + 3 * i] * R[6 + j];
  const int st = rot_to_quat(AR, q);
  ba_transform_point(sim, cams[7 * c], cams[7 * c + 1], cams[7 * c + 2], C);
  if (st != SFM_OK) atomicMin(fail, ((unsigned long long)c << 3) | (unsigned long long)(-st));
#pragma unroll
  for (int k = 0; k < 3; ++k) work[7 * c + k] = C[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) work[7 * c + 3 + k] = q[k];
}

// Then, if every camera passed, the commit: the cameras from the work buffer and the points by the formula.
__global__ void ba_transform_commit_kernel(int V, int N, const double* __restrict__ work, const double* __restrict__ sim,
                                           const int* __restrict__ gate, const unsigned long long* __restrict__ fail,
                                           double* __restrict__ cams, double* __restrict__ px, double* __restrict__ py,
                                           double* __restrict__ pz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (*fail != kTransformClean || ba_transform_gated(gate)) return;
  if (i < 7 * V) cams[i] = work[i];
  if (i < N) {
    double X[3];
    ba_transform_point(sim, px[i], py[i], pz[i], X);
    px[i] = X[0]; py[i] = X[1]; pz[i] = X[2];
  }
}

// Enqueue both on p->stream; *fail_word (device) is left for the caller to read behind them.
static int ba_enqueue_transform(sfm_ba_problem* p, const double* d_sim, const int* d_gate, DevBuf<double>& work,
                                DevBuf<unsigned long long>& fail) {
  BaDev& d = p->dev;
  hipStream_t s = p->stream;
  SFM_TRY(work.alloc(7 * (size_t)d.V, s));
  SFM_TRY(fail.alloc(1, s));
  SFM_HIP(hipMemsetAsync(fail.p, 0xFF, sizeof(unsigned long long), s));
  const int span = std::max(7 * d.V, d.N);
  if (d.V > 0) ba_transform_cams_kernel<<<(d.V + 63) / 64, 64, 0, s>>>(d.V, d.cams, d_sim, d_gate, work.p, fail.p);
  if (span > 0) ba_transform_commit_kernel<<<(span + 255) / 256, 256, 0, s>>>(d.V, d.N, work.p, d_sim, d_gate, fail.p, d.cams, d.px, d.py, d.pz);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// The word the transform left, downloaded and the stream waited for: a failed camera is the call's error.
static int ba_transform_verdict(sfm_ba_problem* p, const char* who, const DevBuf<unsigned long long>& fail) {
  unsigned long long word = kTransformClean;
  SFM_TRY(fail.download(&word, 1, p->stream));
  SFM_TRY(stream_sync(p->stream));
  if (word == kTransformClean) return SFM_OK;
  const int st = -(int)(word & 7);
  set_error("%s: camera %d has no quaternion after the transform (status %d); the scene is unchanged", who, (int)(word >> 3), st);
  return st;
}

__global__ void ba_gather_rot_kernel(int V, const CamPrep* __restrict__ prep, double* __restrict__ rots) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * V) return;
  rots[i] = prep[i / 9].R[i % 9];
}

// cost (and, with pt_ptr, the observed-point count) of a per-point linearisation: sfm_ba_terms.h
__global__ __launch_bounds__(256) void ba_point_cost_reduce_kernel(int N, const double* __restrict__ cost_pt, const int* __restrict__ pt_ptr,
                                                                   double* __restrict__ out) {
  __shared__ double sc[256];
  __shared__ int sn[256];
  const int t = threadIdx.x;
  double c = 0;
  int n = 0;
  for (int p = t; p < N; p += 256) {
    c += cost_pt[p];
    if (pt_ptr != nullptr) n += pt_ptr[p + 1] > pt_ptr[p];
  }
  sc[t] = c; sn[t] = n;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) { sc[t] += sc[t + s]; sn[t] += sn[t + s]; }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = sc[0];
    if (pt_ptr != nullptr) out[1] = (double)sn[0];
  }
}

int ba_check_handle(const sfm_ba_problem* p) {
  if (p == nullptr || p->magic != kBaMagic) {
    set_error("invalid bundle-adjustment problem handle");
    return SFM_E_HANDLE;
  }
  return SFM_OK;
}

int ba_refuse_comm(const sfm_ba_problem* p, const char* who, const char* why) {
  if (p->comm == nullptr) return SFM_OK;
  set_error("%s: not with a communicator attached (%s)", who, why);
  return SFM_E_SHAPE;
}

int ba_sync_cam_status(sfm_ba_problem* p, const char* who, const char* when) {
  int st[2] = {0, 0};
  SFM_HIP(hipMemcpyAsync(st, p->dev.status, sizeof(st), hipMemcpyDeviceToHost, p->stream));
  SFM_TRY(stream_sync(p->stream));
  if (st[0] != SFM_OK) set_error("%s: camera %d is invalid%s (status %d)", who, st[1], when, st[0]);
  return st[0];
}

int ba_prepared_cameras(sfm_ba_problem* p, const char* who) {
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));
  return ba_sync_cam_status(p, who, "");
}

void ba_free_cameras(const unsigned char* cam_mask, int V, int* v_free, int* first_free) {
  *v_free = 0;
  *first_free = -1;
  for (int c = 0; c < V; ++c) {
    if (cam_mask != nullptr && cam_mask[c] == 0) continue;
    if (*v_free == 0) *first_free = c;
    ++*v_free;
  }
}

static const char* status_name(int st) {
  switch (st) {
    case SFM_E_BAD_ROTATION: return "invalid rotation matrix";
    case SFM_E_QW_ZERO: return "quaternion qw ~ 0";
    case SFM_E_SQRT_DOMAIN: return "1 + trace(R) < 0";
    default: return "unknown";
  }
}

// Enqueue the structure kernel (all index arrays of sc.dev must be on the device already).
int ba_enqueue_structure(BaScene& sc, hipStream_t s) {
  const BaDev& d = sc.dev;
  SFM_HIP(hipMemsetAsync(d.sinfo, 0, 4 * sizeof(int), s));
  if (d.N > 0) {
    const int nblk = (d.V + kSchurCB - 1) / kSchurCB;
    ba_structure_kernel<<<(d.N + 255) / 256, 256, 0, s>>>(d.V, d.N, d.M, d.pt_ptr, d.cam_idx, d.obs_pt, sc.schur_blk_ptr, nblk, d.sinfo);
    SFM_HIP(hipGetLastError());
  }
  return SFM_OK;
}

// Wait for the structure kernel and turn its verdict into a status / message.  `who` names the entry point.
static int ba_finish_structure(BaScene& sc, hipStream_t s, const char* who) {
  int info[4] = {0, 0, 0, 0};
  SFM_HIP(hipMemcpyAsync(info, sc.dev.sinfo, sizeof(info), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  sc.max_track = info[2];
  switch (info[0]) {
    case 0: return SFM_OK;
    case 1: set_error("%s: pt_ptr not monotone at point %d", who, info[1]); break;
    case 2: set_error("%s: cam_idx[%d] out of range", who, info[1]); break;
    case 3: set_error("%s: observations of point %d are not sorted by strictly increasing camera "
                      "(a camera observes the point twice, or the point is already observed by it)", who, info[1]); break;
    default: set_error("%s: observation %d (camera, point) out of range", who, info[1]); break;
  }
  return SFM_E_SHAPE;
}

// The chain above for any list of M keys in 0 .. V - 1 on the device (the cameras of the scene's observations, the ends of
// the edges of a view graph): d_ptr[V + 1] and d_list[M], the entries of a key in ascending order.  Enqueued on s.
int key_major_list(long long M, int V, const int* d_key, int* d_ptr, int* d_list, hipStream_t s) {
  // at most 1 024 chunks of at least 1 024 entries: the count table stays within 1 024 V integers
  const int chunk_obs = (int)std::max<long long>(1024, ((M + 1023) / 1024 + 63) / 64 * 64);
  const int nchunks = (int)((M + chunk_obs - 1) / chunk_obs);
  DevBuf<int> table, cnt;
  SFM_TRY(table.alloc((size_t)nchunks * V, s));
  SFM_TRY(cnt.alloc((size_t)V, s));
  SFM_HIP(hipMemsetAsync(table.p, 0, sizeof(int) * (size_t)nchunks * V, s));
  ba_cam_list_count_kernel<<<(unsigned)((M + 255) / 256), 256, 0, s>>>(M, V, chunk_obs, d_key, table.p);
  ba_cam_list_chunk_scan_kernel<<<(V + 255) / 256, 256, 0, s>>>(V, nchunks, table.p, cnt.p);
  ba_cam_list_ptr_scan_kernel<<<1, kScanBlock, 0, s>>>(V, cnt.p, d_ptr);
  ba_cam_list_fill_kernel<<<nchunks, 64, 0, s>>>(M, V, chunk_obs, d_key, d_ptr, table.p, d_list);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

// The scene's camera-major list, built on first use by the row-panel product or the motion-only refinement (a grown or
// culled scene is a new BaScene and starts without one).  Needs M > 0; blocks once for the host copy of cam_ptr.
int ba_cam_list_ensure(sfm_ba_problem* p) {
  if (p->cam_list_built) return SFM_OK;
  const BaDev& d = p->dev;
  hipStream_t s = p->stream;
  const int V = d.V;
  const long long M = d.M;
  SFM_TRY(scene_alloc(*p, p->cam_ptr, (size_t)V + 1));
  SFM_TRY(scene_alloc(*p, p->cam_obs, (size_t)M));
  SFM_TRY(key_major_list(M, V, d.cam_idx, p->cam_ptr, p->cam_obs, s));
  p->h_cam_ptr.assign((size_t)V + 1, 0);
  SFM_HIP(hipMemcpyAsync(p->h_cam_ptr.data(), p->cam_ptr, sizeof(int) * ((size_t)V + 1), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  p->cam_list_built = true;
  return SFM_OK;
}

int scene_alloc_bytes(BaScene& sc, void** ptr, size_t bytes) {
  const hipError_t e = pool_alloc(ptr, std::max<size_t>(1, bytes));
  if (e != hipSuccess) return hip_fail(e, "hipMalloc of a scene buffer", __LINE__);
  sc.owned.push_back(*ptr);
  return SFM_OK;
}

// Give back everything the scene owns, once nothing on `stream` uses it any more, and leave a scene of defaults.  Not
// the scene's: the task tables of the data-flow solve (one per device for the life of the process) and a reduced
// buffer the caller bound.
static void ba_scene_free(BaScene& sc, hipStream_t stream) {
  if (!sc.owned.empty() && ctx().inited && stream) (void)hipStreamSynchronize(stream);      // (empty: a new handle's, nothing ran on it)
  for (void* q : sc.owned) pool_free(q);
  sc = BaScene();
}

// The buffers and plans of a scene of the given sizes (nothing uploaded, no structure yet); the caller frees it on failure.
static int ba_scene_alloc(BaScene& sc, int V, int N, long long M, hipStream_t stream) {
  sc.owned.reserve(40);
  BaDev& d = sc.dev;
  d.V = V; d.N = N; d.M = M; d.P = 7 * V;
  d.nbk = (d.P + kNB - 1) / kNB;
  const size_t lin_wgs = (size_t)kLinGridPerCu * plan_cus();
  SFM_TRY(scene_alloc(sc, d.pt_ptr, (size_t)N + 1));
  SFM_TRY(scene_alloc(sc, d.cam_idx, (size_t)M));
  SFM_TRY(scene_alloc(sc, d.obs_pt, (size_t)M));
  SFM_TRY(scene_alloc(sc, d.u, (size_t)M));
  SFM_TRY(scene_alloc(sc, d.v, (size_t)M));
  SFM_TRY(scene_alloc(sc, d.cams, (size_t)V * 7));
  SFM_TRY(scene_alloc(sc, d.px, (size_t)N)); SFM_TRY(scene_alloc(sc, d.py, (size_t)N)); SFM_TRY(scene_alloc(sc, d.pz, (size_t)N));
  SFM_TRY(scene_alloc(sc, d.prep[0], (size_t)V)); SFM_TRY(scene_alloc(sc, d.prep[1], (size_t)V));
  SFM_TRY(scene_alloc(sc, d.lin_ws, (sizeof(double) * V * 35 <= 64 * 1024) ? lin_wgs * V * 35 : 1));
  SFM_TRY(scene_alloc(sc, sc.own_red, red_size(d.nbk)));
  SFM_TRY(scene_alloc(sc, d.delta, (size_t)d.nbk * kNB));
  SFM_TRY(scene_alloc(sc, d.ldiag, (size_t)((d.P + 31) / 32) * 32 * 32));
  SFM_TRY(scene_alloc(sc, d.xinv, d.nbk <= kInvRowsMaxNbk ? red_rhs_off(d.nbk) : 1));      // beyond that the back substitution runs block row by block row
  SFM_TRY(scene_alloc(sc, d.sync_ctr, 1));
  SFM_TRY(scene_alloc(sc, d.status, 2));
  SFM_TRY(scene_alloc(sc, d.sinfo, 4));
  SFM_TRY(scene_alloc(sc, d.cost, kStatSlots));
  SFM_TRY(scene_alloc(sc, d.cost_ws, lin_wgs));
  SFM_TRY(scene_alloc(sc, d.iter_count, 1));
  d.red = sc.own_red;
  SFM_HIP(hipMemsetAsync(d.status, 0, 2 * sizeof(int), stream));
  SFM_HIP(hipMemsetAsync(d.cost, 0, kStatSlots * sizeof(double), stream));
  SFM_HIP(hipMemsetAsync(d.iter_count, 0, sizeof(int), stream));
  SFM_HIP(hipMemsetAsync(d.sync_ctr, 0, sizeof(int), stream));
  SFM_HIP(hipMemsetAsync(d.delta, 0, sizeof(double) * d.nbk * kNB, stream));
  SFM_TRY(ba_schur_plan(sc));
  return ba_flow_setup(sc, stream);
}

// A new state starts a new cost history (sfm_ba_get_stats).
int ba_reset_stats(sfm_ba_problem* p) {
  SFM_HIP(hipMemsetAsync(p->dev.cost, 0, kStatSlots * sizeof(double), p->stream));
  SFM_HIP(hipMemsetAsync(p->dev.iter_count, 0, sizeof(int), p->stream));
  return SFM_OK;
}

int ba_state_changed(sfm_ba_problem* p) {
  SFM_TRY(ba_reset_stats(p));
  p->prep_valid = false;
  return SFM_OK;
}

static int ba_upload(sfm_ba_problem* p, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return SFM_OK;
  SFM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, p->stream));
  p->upload_bytes += (long long)bytes;
  return SFM_OK;
}

// The two fields of the kernel argument that belong to the handle: after create, SFM_OPT_DEBUG and every adoption.
static void ba_mirror_handle(sfm_ba_problem* p) {
  p->dev.debug = p->debug;
  p->dev.stamps = p->stamps;
}

// Why the scene cannot run with a fixed summation order, or null: deterministic mode needs the atomic-free dense product
// (Zd resident) and the LDS camera accumulators of ba_linearize.
static const char* ba_deterministic_obstacle(const BaScene& sc) {
  if (!sc.schur_mfma_ok) return "deterministic mode needs the dense Schur product, which does not fit this scene";
  if (sizeof(double) * (size_t)sc.dev.V * 35 > 64 * 1024) return "deterministic mode supports at most 234 cameras";
  return nullptr;
}

// p takes over `sc`, a checked scene built on p's stream, and what it held before is freed: the handle keeps its
// identity, options, stream, counters and stamp buffer (sfm_ba_create*, sfm_ba_append, sfm_ba_sync_tracks).
static int ba_adopt_grown(sfm_ba_problem* p, BaScene& sc, int n_new_cams) {
  // an externally bound reduced buffer has the wrong size when cameras were added: the library's own buffer takes
  // over and the caller binds a new one (sfm_ba_reduced_buffer reports the new size); with the camera count
  // unchanged the binding survives
  double* const bound_red = (p->dev.red != p->own_red && n_new_cams == 0) ? p->dev.red : nullptr;
  ba_graph_drop(p);
  std::swap(static_cast<BaScene&>(*p), sc);
  ba_mirror_handle(p);
  // deterministic mode holds for the grown scene only while the dense product fits and the camera accumulators stay in
  // LDS (V <= 234): beyond that the handle falls back to the default path instead of mixing the two reduce kernels
  if (ba_deterministic_obstacle(*p)) p->deterministic = 0;
  if (bound_red) p->dev.red = bound_red;
  ba_scene_free(sc, p->stream);
  return SFM_OK;
}

// One growth: a scene of the given sizes on p's stream, `fill` enqueues its structure and state, the structure kernel
// checks it (synchronising: the caller's arrays are free again), and p adopts it.  On any failure the stream is drained, the
// new scene freed and p left as it was.  `fill` keeps its temporaries outside, so that they outlive the check.
template <typename Fill>
static int ba_grow(sfm_ba_problem* p, int V, int N, long long M, int n_new_cams, const char* who, Fill&& fill) {
  hipStream_t s = p->stream;
  BaScene sc;
  int st = ba_scene_alloc(sc, V, N, M, s);
  if (st == SFM_OK) st = fill(sc.dev);
  if (st == SFM_OK) st = ba_enqueue_structure(sc, s);
  if (st == SFM_OK) st = ba_finish_structure(sc, s, who);
  if (st != SFM_OK) { (void)hipStreamSynchronize(s); ba_scene_free(sc, s); return st; }
  return ba_adopt_grown(p, sc, n_new_cams);
}

// The store's list IS the (point, camera)-sorted list of a scene of its sizes: taken over device to device.
static int ba_fill_from_tracks(const BaDev& e, const TrackObservations& t, hipStream_t s) {
  const size_t m = (size_t)t.n_obs;
  SFM_HIP(hipMemcpyAsync(e.pt_ptr, t.pt_ptr, sizeof(int) * ((size_t)t.n_pts + 1), hipMemcpyDeviceToDevice, s));
  if (m > 0) {
    SFM_HIP(hipMemcpyAsync(e.cam_idx, t.cam_idx, sizeof(int) * m, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(e.u, t.u, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    SFM_HIP(hipMemcpyAsync(e.v, t.v, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
  }
  return SFM_OK;
}

// State of a grown scene e: p's cameras / points stay on the device, the new ones are uploaded behind them.
static int ba_carry_state(sfm_ba_problem* p, const BaDev& e, const double* cams_new, const double* pts_new) {
  const BaDev& d = p->dev;
  hipStream_t s = p->stream;
  const int n_new_cams = e.V - d.V, n_new_pts = e.N - d.N;
  SFM_HIP(hipMemcpyAsync(e.cams, d.cams, sizeof(double) * 7 * d.V, hipMemcpyDeviceToDevice, s));
  SFM_TRY(ba_upload(p, e.cams + 7 * (size_t)d.V, cams_new, sizeof(double) * 7 * n_new_cams));
  double* dst[3] = {e.px, e.py, e.pz};
  const double* old[3] = {d.px, d.py, d.pz};
  for (int k = 0; k < 3; ++k) {
    if (d.N > 0) SFM_HIP(hipMemcpyAsync(dst[k], old[k], sizeof(double) * d.N, hipMemcpyDeviceToDevice, s));
    SFM_TRY(ba_upload(p, dst[k] + d.N, pts_new + (size_t)k * n_new_pts, sizeof(double) * n_new_pts));
  }
  return SFM_OK;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_ba_create(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv_norm,
                  sfm_ba_problem** out) {
  SFM_TRY(ensure_init());
  if (out == nullptr) { set_error("sfm_ba_create: out is null"); return SFM_E_SHAPE; }
  *out = nullptr;
  if (V < 1 || N < 0 || M < 0 || M > 0x7fffffffLL) {
    set_error("sfm_ba_create: bad sizes V=%d N=%d M=%lld", V, N, (long long)M);
    return SFM_E_SHAPE;
  }
  if (N == 0 && M > 0) { set_error("sfm_ba_create: %lld observations but no point", (long long)M); return SFM_E_SHAPE; }
  if (M > 0 && uv_norm == nullptr) { set_error("sfm_ba_create: uv_norm is null"); return SFM_E_SHAPE; }
  if (N > 0 && (pt_ptr[0] != 0 || pt_ptr[N] != M)) { set_error("sfm_ba_create: pt_ptr must span [0, M]"); return SFM_E_SHAPE; }
  sfm_ba_problem* p = new sfm_ba_problem();
  ++ba_live_problems();      // (sfm_set_cu_limit is refused while one exists)
  p->stream = ctx().stream;
  const int zero_ptr = 0;
  const int st = ba_grow(p, V, N, M, 0, "sfm_ba_create", [&](const BaDev& d) -> int {
    SFM_TRY(N > 0 ? ba_upload(p, d.pt_ptr, pt_ptr, sizeof(int) * ((size_t)N + 1)) : ba_upload(p, d.pt_ptr, &zero_ptr, sizeof(int)));
    SFM_TRY(ba_upload(p, d.cam_idx, cam_idx, sizeof(int) * (size_t)M));
    SFM_TRY(ba_upload(p, d.u, uv_norm, sizeof(double) * (size_t)M));
    return ba_upload(p, d.v, uv_norm + M, sizeof(double) * (size_t)M);
  });
  if (st != SFM_OK) { sfm_ba_destroy(p); return st; }
  *out = p;
  return SFM_OK;
}

int sfm_ba_destroy(sfm_ba_problem* p) {
  if (p == nullptr) return SFM_OK;
  if (p->magic != kBaMagic) { set_error("sfm_ba_destroy: invalid handle"); return SFM_E_HANDLE; }
  ba_scene_free(*p, p->stream);      // waits for the stream before anything returns to the pool
  pool_free(p->stamps);
  ba_graph_drop(p);
  if (p->comm) { (void)comm_attach(p->comm, -1); p->comm = nullptr; }
  for (auto& t : p->timers)
    for (auto& e : t.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  p->magic = 0;
  delete p;
  --ba_live_problems();
  return SFM_OK;
}

int sfm_ba_set_stream(sfm_ba_problem* p, void* hip_stream) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  SFM_HIP(hipStreamSynchronize(p->stream));
  ba_graph_drop(p);
  p->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx().own;
  return SFM_OK;
}

int sfm_ba_set_option(sfm_ba_problem* p, int option, int value) {
  SFM_TRY(ba_check_handle(p));
  ba_graph_drop(p);       // every option changes what an iteration launches
  switch (option) {
    case SFM_OPT_GRAPH:
      p->use_graph = value != 0;
      return SFM_OK;
    case SFM_OPT_SCHUR:
      SFM_TRY(ba_flush(p));
      if (value < SFM_SCHUR_AUTO || value > SFM_SCHUR_ROWS) { set_error("bad schur mode %d", value); return SFM_E_SHAPE; }
      p->schur_mode = value;
      return SFM_OK;
    case SFM_OPT_DEBUG:
      SFM_TRY(ba_flush(p));
      p->debug = value;
      if ((value & 8) && p->stamps == nullptr) {
        SFM_HIP(pool_alloc(reinterpret_cast<void**>(&p->stamps), sizeof(unsigned long long) * 1024));
        SFM_HIP(hipMemset(p->stamps, 0, sizeof(unsigned long long) * 1024));
      }
      ba_mirror_handle(p);
      return SFM_OK;
    case SFM_OPT_TIMING:
      p->timing = value;   // bit k set = time kernel class k
      return SFM_OK;
    case SFM_OPT_TIMING_STRIDE:
      if (value < 1) { set_error("timing stride %d < 1", value); return SFM_E_SHAPE; }
      p->timing_stride = value;
      return SFM_OK;
    case SFM_OPT_DETERMINISTIC:
      SFM_TRY(ba_flush(p));
      if (const char* why = value != 0 ? ba_deterministic_obstacle(*p) : nullptr) { set_error("%s", why); return SFM_E_SHAPE; }
      p->deterministic = value != 0;
      return SFM_OK;
    default:
      set_error("unknown option %d", option);
      return SFM_E_SHAPE;
  }
}

int sfm_ba_info(sfm_ba_problem* p, int what, int64_t* value) {
  SFM_TRY(ba_check_handle(p));
  if (value == nullptr) { set_error("sfm_ba_info: value is null"); return SFM_E_SHAPE; }
  switch (what) {
    case SFM_INFO_SCHUR_KERNEL: {
      // the kernel the next iteration WILL launch: the row-panel product needs its camera-major list and work split,
      // which decide whether it can run at all -- build them now rather than answer "rows" and then launch "pairs"
      int choice = ba_schur_choice(p);
      if (choice == SFM_SCHUR_ROWS && p->dev.M > 0 && p->dev.N > 0) {
        if (!p->rows_built) SFM_TRY(ba_flush(p));
        SFM_TRY(ba_rows_ensure(p));
        if (!p->rows_ok) choice = SFM_SCHUR_PAIRS;
      }
      *value = choice;
      return SFM_OK;
    }
    case SFM_INFO_UPLOAD_BYTES: *value = p->upload_bytes; return SFM_OK;
    case SFM_INFO_N_CAMS: *value = p->dev.V; return SFM_OK;
    case SFM_INFO_N_PTS: *value = p->dev.N; return SFM_OK;
    case SFM_INFO_N_OBS: *value = p->dev.M; return SFM_OK;
    case SFM_INFO_MAX_TRACK: *value = p->max_track; return SFM_OK;
    case SFM_INFO_GRAPH_REPLAYS: *value = p->graph_replays; return SFM_OK;
    case SFM_INFO_REDUCE_IN_SOLVE: *value = p->last_reduce_deferred ? 1 : 0; return SFM_OK;
    case SFM_INFO_PCG_HELD_POINTS: *value = p->pcg_held_points; return SFM_OK;
    case SFM_INFO_SOLVE_PATH: *value = ba_solve_path(p); return SFM_OK;
    default: set_error("sfm_ba_info: unknown item %d", what); return SFM_E_SHAPE;
  }
}

int sfm_ba_flush(sfm_ba_problem* p) {
  SFM_TRY(ba_check_handle(p));
  return ba_flush(p);
}

int sfm_ba_set_cameras(sfm_ba_problem* p, const double* cams) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  BaDev& d = p->dev;
  SFM_TRY(ba_upload(p, d.cams, cams, sizeof(double) * 7 * d.V));
  SFM_HIP(hipMemsetAsync(d.status, 0, 2 * sizeof(int), p->stream));
  SFM_TRY(ba_reset_stats(p));
  SFM_TRY(stream_sync(p->stream));
  p->prep_valid = false;
  return SFM_OK;
}

int sfm_ba_set_points(sfm_ba_problem* p, int first, int count, const double* pts) {
  SFM_TRY(ba_check_handle(p));
  BaDev& d = p->dev;
  SFM_TRY(ba_flush(p));
  if (first < 0 || count < 0 || first + (long long)count > d.N) {
    set_error("sfm_ba_set_points: range [%d, %d) outside the %d points", first, first + count, d.N);
    return SFM_E_SHAPE;
  }
  SFM_TRY(ba_upload(p, d.px + first, pts, sizeof(double) * count));
  SFM_TRY(ba_upload(p, d.py + first, pts + count, sizeof(double) * count));
  SFM_TRY(ba_upload(p, d.pz + first, pts + 2 * (size_t)count, sizeof(double) * count));
  SFM_TRY(ba_reset_stats(p));
  SFM_TRY(stream_sync(p->stream));
  return SFM_OK;
}

int sfm_ba_set_state(sfm_ba_problem* p, const double* cams, const double* pts) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  BaDev& d = p->dev;
  SFM_TRY(ba_upload(p, d.cams, cams, sizeof(double) * 7 * d.V));
  if (d.N > 0) {
    SFM_TRY(ba_upload(p, d.px, pts, sizeof(double) * d.N));
    SFM_TRY(ba_upload(p, d.py, pts + d.N, sizeof(double) * d.N));
    SFM_TRY(ba_upload(p, d.pz, pts + 2 * (size_t)d.N, sizeof(double) * d.N));
  }
  SFM_HIP(hipMemsetAsync(d.status, 0, 2 * sizeof(int), p->stream));
  SFM_TRY(ba_reset_stats(p));
  SFM_TRY(stream_sync(p->stream));
  p->prep_valid = false;
  return SFM_OK;
}

int sfm_ba_transform(sfm_ba_problem* p, double s, const double A[9], const double t[3]) {
  const char* who = "sfm_ba_transform";
  SFM_TRY(ba_check_handle(p));
  if (A == nullptr || t == nullptr) { set_error("%s: null pointer", who); return SFM_E_SHAPE; }
  if (!(s > 0.0 && s <= 1.7976931348623157e308)) { set_error("%s: s = %g must be finite and > 0", who, s); return SFM_E_SHAPE; }
  double sim[13] = {s};
  bool finite = true;
  for (int k = 0; k < 9; ++k) { sim[1 + k] = A[k]; finite = finite && std::isfinite(A[k]); }
  for (int k = 0; k < 3; ++k) { sim[10 + k] = t[k]; finite = finite && std::isfinite(t[k]); }
  if (!finite) { set_error("%s: A and t must be finite", who); return SFM_E_SHAPE; }
  if (!verify_rotation(A)) { set_error("%s: A is not a rotation matrix", who); return SFM_E_BAD_ROTATION; }
  SFM_TRY(ba_refuse_comm(p, who, "the points are sharded; every rank would have to move its part by the same call"));
  SFM_TRY(ba_flush(p));
  DevBuf<double> d_sim, work;
  DevBuf<unsigned long long> fail;
  SFM_TRY(d_sim.upload(sim, 13, p->stream));
  p->upload_bytes += (long long)sizeof(sim);
  SFM_TRY(ba_enqueue_transform(p, d_sim.p, nullptr, work, fail));
  SFM_TRY(ba_transform_verdict(p, who, fail));
  return ba_state_changed(p);
}

int sfm_ba_align(sfm_ba_problem* p, int n, const int* point_idx, const double* target, double max_err2, int max_hyp, int iters,
                 int flags, int apply, double* sim_out, unsigned char* inlier, int* n_inliers, int* best_hyp, int* status) {
  const char* who = "sfm_ba_align";
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(similarity_check_options(who, max_err2, max_hyp, iters, flags));
  BaDev& d = p->dev;
  if (n < 0 || sim_out == nullptr || (n > 0 && (point_idx == nullptr || target == nullptr))) { set_error("%s: bad sizes or null pointer (n = %d)", who, n); return SFM_E_SHAPE; }
  for (int i = 0; i < n; ++i)
    if (point_idx[i] < 0 || point_idx[i] >= d.N) { set_error("%s: point_idx[%d] = %d is outside the %d points", who, i, point_idx[i], d.N); return SFM_E_SHAPE; }
  SFM_TRY(ba_refuse_comm(p, who, "the points are sharded; every rank would have to move its part by the same call"));
  SFM_TRY(ba_flush(p));
  if (n == 0) {
    std::fill(sim_out, sim_out + 13, 0.0);
    if (n_inliers) *n_inliers = 0;
    if (best_hyp) *best_hyp = -1;
    if (status) *status = SFM_SIMILARITY_TOO_FEW;
    return SFM_OK;
  }
  hipStream_t s = p->stream;
  const size_t m = (size_t)n;
  DevBuf<int> d_idx, d_small;                    // d_small: n_inliers, best_hyp, status
  DevBuf<double> d_src, d_dst, d_sim, work;
  DevBuf<unsigned char> d_inl;
  DevBuf<unsigned long long> fail;
  SFM_TRY(d_idx.upload(point_idx, m, s));
  SFM_TRY(d_dst.upload(target, 3 * m, s));
  p->upload_bytes += (long long)(sizeof(int) * m + sizeof(double) * 3 * m);
  SFM_TRY(d_src.alloc(4 * m, s)); SFM_TRY(d_sim.alloc(13, s)); SFM_TRY(d_small.alloc(3, s)); SFM_TRY(d_inl.alloc(m, s));
  SFM_TRY(sfm_gather_points_dev(n, d_idx.p, d.px, d.py, d.pz, d_src.p, s));      // rows X, Y, Z of [4][n]: src as [3][n]
  const int set_ptr[2] = {0, n};
  SFM_TRY(sfm_similarity_ransac_dev(1, set_ptr, n, d_src.p, d_dst.p, max_err2, max_hyp, iters, flags, d_sim.p, d_inl.p, d_small.p,
                                    d_small.p + 1, d_small.p + 2, nullptr, s));
  if (apply) SFM_TRY(ba_enqueue_transform(p, d_sim.p, d_small.p + 2, work, fail));
  int small[3] = {0, -1, 0};
  SFM_TRY(d_sim.download(sim_out, 13, s));
  SFM_TRY(d_small.download(small, 3, s));
  if (inlier) SFM_TRY(d_inl.download(inlier, m, s));
  const int verdict = apply ? ba_transform_verdict(p, who, fail) : stream_sync(s);
  if (n_inliers) *n_inliers = small[0];
  if (best_hyp) *best_hyp = small[1];
  if (status) *status = small[2];
  SFM_TRY(verdict);
  if (apply && !(small[2] & (SFM_SIMILARITY_TOO_FEW | SFM_SIMILARITY_NO_MODEL))) SFM_TRY(ba_state_changed(p));
  return SFM_OK;
}

int sfm_ba_set_loss(sfm_ba_problem* p, int kind, double delta) {
  SFM_TRY(ba_check_handle(p));
  if (kind != SFM_LOSS_NONE && kind != SFM_LOSS_HUBER && kind != SFM_LOSS_CAUCHY) { set_error("sfm_ba_set_loss: unknown loss %d", kind); return SFM_E_SHAPE; }
  if (kind != SFM_LOSS_NONE && !(delta > 0 && delta <= 1.7976931348623157e308)) { set_error("sfm_ba_set_loss: delta must be finite and > 0"); return SFM_E_SHAPE; }
  SFM_TRY(ba_flush(p));        // the pending step was solved for the old loss: its back substitution takes the old weights
  ba_graph_drop(p);            // the captured bodies hold the old instantiation and its delta
  SFM_TRY(ba_reset_stats(p));  // the cost changes meaning
  p->loss_kind = kind;
  if (kind != SFM_LOSS_NONE) p->loss_delta = delta;
  return SFM_OK;
}

int sfm_ba_get_loss(sfm_ba_problem* p, int* kind, double* delta) {
  SFM_TRY(ba_check_handle(p));
  if (kind) *kind = p->loss_kind;
  if (delta) *delta = p->loss_delta;
  return SFM_OK;
}

int sfm_ba_loss_terms(sfm_ba_problem* p, double* s, double* w, double* rho) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));
  const size_t m = (size_t)p->dev.M;
  if (m == 0) return stream_sync(p->stream);
  hipStream_t st = p->stream;
  HostOut<double> os, ow, orho;
  SFM_TRY(os.want(s, m, st)); SFM_TRY(ow.want(w, m, st)); SFM_TRY(orho.want(rho, m, st));
  ba_enqueue_loss_terms(p, p->quirks, os.dev(), ow.dev(), orho.dev());
  SFM_HIP(hipGetLastError());
  SFM_TRY(os.fetch(st)); SFM_TRY(ow.fetch(st)); SFM_TRY(orho.fetch(st));
  return stream_sync(st);
}

int sfm_ba_get_stats(sfm_ba_problem* p, double* cost, int max_iters, int* n_iters) {
  SFM_TRY(ba_check_handle(p));
  if (max_iters < 0 || (max_iters > 0 && cost == nullptr)) { set_error("sfm_ba_get_stats: bad output buffer"); return SFM_E_SHAPE; }
  int done = 0;
  SFM_HIP(hipMemcpyAsync(&done, p->dev.iter_count, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  SFM_TRY(stream_sync(p->stream));
  const int n = std::min(std::min(done, kStatSlots), max_iters);
  if (n > 0) SFM_HIP(hipMemcpyAsync(cost, p->dev.cost, sizeof(double) * n, hipMemcpyDeviceToHost, p->stream));
  SFM_TRY(stream_sync(p->stream));
  if (n_iters) *n_iters = n;
  return SFM_OK;
}

int sfm_ba_linearize_reduce(sfm_ba_problem* p, double lambda, int quirks) {
  SFM_TRY(ba_check_handle(p));
  return ba_enqueue_linearize_reduce(p, lambda, quirks);
}

int sfm_ba_solve_update(sfm_ba_problem* p, double lambda, int quirks) {
  SFM_TRY(ba_check_handle(p));
  return ba_enqueue_solve_update(p, lambda, quirks);
}

int sfm_ba_iterate(sfm_ba_problem* p, double lambda, int iters, int quirks) {
  SFM_TRY(ba_check_handle(p));
  if (iters < 0) { set_error("sfm_ba_iterate: iters < 0"); return SFM_E_SHAPE; }
  return ba_enqueue_iterations(p, lambda, iters, quirks);
}

int sfm_ba_get_state(sfm_ba_problem* p, double* cams, double* pts) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  hipStream_t s = p->stream;
  BaDev& d = p->dev;
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));     // validates the cameras even with zero iterations (ba:412)
  int st[2] = {0, 0};
  SFM_HIP(hipMemcpyAsync(cams, d.cams, sizeof(double) * 7 * d.V, hipMemcpyDeviceToHost, s));
  if (d.N > 0) {
    SFM_HIP(hipMemcpyAsync(pts, d.px, sizeof(double) * d.N, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(pts + d.N, d.py, sizeof(double) * d.N, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(pts + 2 * (size_t)d.N, d.pz, sizeof(double) * d.N, hipMemcpyDeviceToHost, s));
  }
  SFM_HIP(hipMemcpyAsync(st, d.status, sizeof(st), hipMemcpyDeviceToHost, s));
  SFM_TRY(stream_sync(s));
  if (st[0] != SFM_OK) {
    set_error("bundle adjustment: %s for camera %d", status_name(st[0]), st[1]);
    return st[0];
  }
  return SFM_OK;
}

int sfm_ba_rederive_quaternions(sfm_ba_problem* p, int first, int count) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  BaDev& d = p->dev;
  if (first < 0 || count < 0 || first + (long long)count > d.V) {
    set_error("sfm_ba_rederive_quaternions: range [%d, %d) outside the %d cameras", first, first + count, d.V);
    return SFM_E_SHAPE;
  }
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));      // R(q) and q(R(q)) of the resident cameras (validated: status)
  if (count > 0) {
    ba_rederive_quat_kernel<<<(count + 63) / 64, 64, 0, p->stream>>>(first, count, d.prep[p->cur], d.cams);
    SFM_HIP(hipGetLastError());
  }
  SFM_TRY(ba_reset_stats(p));
  p->prep_valid = false;          // R(q') differs from R(q) in the last bits: expand again before linearising
  return SFM_OK;
}

int sfm_ba_get_state_rot(sfm_ba_problem* p, double* cams, double* pts, double* rots) {
  SFM_TRY(ba_check_handle(p));
  if (rots == nullptr) return sfm_ba_get_state(p, cams, pts);
  SFM_TRY(ba_flush(p));
  if (!p->prep_valid) SFM_TRY(ba_enqueue_prep(p));
  BaDev& d = p->dev;
  DevBuf<double> dR;
  SFM_TRY(dR.alloc(9 * (size_t)d.V, p->stream));
  ba_gather_rot_kernel<<<(9 * d.V + 255) / 256, 256, 0, p->stream>>>(d.V, d.prep[p->cur], dR.p);
  SFM_HIP(hipGetLastError());
  SFM_TRY(dR.download(rots, 9 * (size_t)d.V, p->stream));
  return sfm_ba_get_state(p, cams, pts);      // synchronises, reports the first device-side failure
}

int sfm_ba_append(sfm_ba_problem* p, int n_new_cams, const double* cams_new, int n_new_pts, const double* pts_new,
                  int64_t n_new_obs, const int* obs_cam, const int* obs_pt, const double* uv_norm) {
  SFM_TRY(ba_check_handle(p));
  if (n_new_cams < 0 || n_new_pts < 0 || n_new_obs < 0) { set_error("sfm_ba_append: negative count"); return SFM_E_SHAPE; }
  SFM_TRY(ba_flush(p));
  BaDev& d = p->dev;
  const int V2 = d.V + n_new_cams, N2 = d.N + n_new_pts;
  const long long M2 = d.M + n_new_obs;
  if (M2 > 0x7fffffffLL) { set_error("sfm_ba_append: too many observations"); return SFM_E_SHAPE; }
  if (N2 == 0 && M2 > 0) { set_error("sfm_ba_append: observations but no point"); return SFM_E_SHAPE; }
  hipStream_t s = p->stream;
  DevBuf<int> dcam, dpt, cnt, nstart, fill, norder;
  DevBuf<double> duv;
  return ba_grow(p, V2, N2, M2, n_new_cams, "sfm_ba_append", [&](const BaDev& e) -> int {
    // only the NEW data crosses PCIe; it is accounted to the surviving handle
    const size_t n = (size_t)n_new_obs;
    SFM_TRY(dcam.upload(obs_cam, n, s)); SFM_TRY(dpt.upload(obs_pt, n, s)); SFM_TRY(duv.upload(uv_norm, 2 * n, s));
    p->upload_bytes += (long long)(n * (2 * sizeof(int) + 2 * sizeof(double)));
    SFM_TRY(cnt.alloc((size_t)N2 + 1, s)); SFM_TRY(nstart.alloc((size_t)N2 + 1, s));
    SFM_TRY(fill.alloc((size_t)N2 + 1, s)); SFM_TRY(norder.alloc(n, s));
    SFM_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)N2 + 1), s));
    SFM_HIP(hipMemsetAsync(fill.p, 0, sizeof(int) * ((size_t)N2 + 1), s));
    SFM_HIP(hipMemsetAsync(e.sinfo, 0, 4 * sizeof(int), s));
    if (n > 0) ba_append_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((long long)n, V2, N2, dcam.p, dpt.p, cnt.p, e.sinfo);
    {   // a bad (camera, point) index must stop the chain before the bucket kernel writes through it
      int info[4] = {0, 0, 0, 0};
      SFM_HIP(hipMemcpyAsync(info, e.sinfo, sizeof(info), hipMemcpyDeviceToHost, s));
      SFM_TRY(stream_sync(s));
      if (info[0] != 0) {
        set_error("sfm_ba_append: observation %d = (camera %d, point %d) out of range", info[1], obs_cam[info[1]], obs_pt[info[1]]);
        return SFM_E_SHAPE;
      }
    }
    ba_append_scan_kernel<<<1, kScanBlock, 0, s>>>(d.N, N2, d.pt_ptr, cnt.p, e.pt_ptr, nstart.p);
    if (n > 0) ba_append_bucket_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((long long)n, dpt.p, nstart.p, fill.p, norder.p);
    if (N2 > 0) ba_append_merge_kernel<<<(N2 + 255) / 256, 256, 0, s>>>(d.N, N2, d.pt_ptr, d.cam_idx, d.u, d.v, e.pt_ptr, nstart.p, norder.p,
                                                                        dcam.p, duv.p, duv.p + n, e.cam_idx, e.u, e.v);
    SFM_HIP(hipGetLastError());
    return ba_carry_state(p, e, cams_new, pts_new);
  });
}

// The shrinking twin of sfm_ba_append: screen (sfm_ba_screen.hip), and if anything fails, a scene of (V, N, M') filled on
// the device -- the kept observations scattered to their new offsets, cameras and points copied as they are.
int sfm_ba_cull(sfm_ba_problem* p, double max_err2, double cos_min_angle, int min_obs, int group, const double* cam_scale,
                double* err2, double* depth, unsigned char* obs_flags, double* min_cos, int* pt_flags, int64_t* summary) {
  SFM_TRY(ba_check_handle(p));
  ScreenWork w;
  SFM_TRY(ba_screen_run(p, "sfm_ba_cull", max_err2, cos_min_angle, min_obs, group, cam_scale, err2, depth, obs_flags, min_cos,
                        pt_flags, summary, w));
  const BaDev& d = p->dev;
  if (w.kept == d.M) return SFM_OK;      // nothing dropped: the scene, its cost history and its graphs stay
  hipStream_t s = p->stream;
  return ba_grow(p, d.V, d.N, w.kept, 0, "sfm_ba_cull", [&](const BaDev& e) -> int {
    SFM_TRY(ba_cull_enqueue_scatter(d, e, w, s));
    SFM_HIP(hipMemcpyAsync(e.cams, d.cams, sizeof(double) * 7 * d.V, hipMemcpyDeviceToDevice, s));
    double* dst[3] = {e.px, e.py, e.pz};
    const double* old[3] = {d.px, d.py, d.pz};
    for (int k = 0; k < 3; ++k) SFM_HIP(hipMemcpyAsync(dst[k], old[k], sizeof(double) * d.N, hipMemcpyDeviceToDevice, s));
    return SFM_OK;
  });
}

int sfm_ba_create_from_tracks(sfm_track_store* store, sfm_ba_problem** out) {
  SFM_TRY(ensure_init());
  if (out == nullptr) { set_error("sfm_ba_create_from_tracks: out is null"); return SFM_E_SHAPE; }
  *out = nullptr;
  TrackObservations t;
  SFM_TRY(track_observations(store, "sfm_ba_create_from_tracks", &t));      // waits for the store's pending work
  if (t.n_views < 1) { set_error("sfm_ba_create_from_tracks: the list was built for %d views", t.n_views); return SFM_E_SHAPE; }
  sfm_ba_problem* p = new sfm_ba_problem();
  ++ba_live_problems();      // (sfm_set_cu_limit is refused while one exists)
  p->stream = ctx().stream;
  // (the check synchronises: the store may build its next list)
  const int st = ba_grow(p, t.n_views, t.n_pts, t.n_obs, 0, "sfm_ba_create_from_tracks",
                         [&](const BaDev& d) -> int { return ba_fill_from_tracks(d, t, p->stream); });
  if (st != SFM_OK) { sfm_ba_destroy(p); return st; }
  *out = p;
  return SFM_OK;
}

int sfm_ba_sync_tracks(sfm_ba_problem* p, sfm_track_store* store, int n_new_cams, const double* cams_new, int n_new_pts,
                       const double* pts_new, int* action, int64_t* n_new_obs) {
  SFM_TRY(ba_check_handle(p));
  if (action == nullptr) { set_error("sfm_ba_sync_tracks: action is null"); return SFM_E_SHAPE; }
  if ((n_new_cams > 0 && cams_new == nullptr) || (n_new_pts > 0 && pts_new == nullptr)) { set_error("sfm_ba_sync_tracks: new cameras or points are null"); return SFM_E_SHAPE; }
  TrackObservations t;
  SFM_TRY(track_observations(store, "sfm_ba_sync_tracks", &t));             // waits for the store's pending work
  SFM_TRY(ba_flush(p));
  BaDev& d = p->dev;
  *action = SFM_SYNC_REPLACED;
  if (n_new_obs) *n_new_obs = 0;
  if (t.n_views < d.V || t.n_pts < d.N || n_new_cams != t.n_views - d.V || n_new_pts != t.n_pts - d.N) return SFM_OK;
  hipStream_t s = p->stream;
  if (d.N > 0) {
    DevBuf<unsigned> bad;
    SFM_TRY(bad.alloc(1, s));
    SFM_HIP(hipMemsetAsync(bad.p, 0xFF, sizeof(unsigned), s));
    ba_tracks_compare_kernel<<<(d.N + 255) / 256, 256, 0, s>>>(d.N, d.pt_ptr, d.cam_idx, d.u, d.v, t.pt_ptr, t.cam_idx, t.u, t.v, bad.p);
    SFM_HIP(hipGetLastError());
    unsigned first_bad = 0;
    SFM_HIP(hipMemcpyAsync(&first_bad, bad.p, sizeof(first_bad), hipMemcpyDeviceToHost, s));
    SFM_TRY(stream_sync(s));
    if (first_bad != 0xFFFFFFFFu) return SFM_OK;
  }
  // every resident track is part of its new track: with the same sizes all round nothing was added either
  if (t.n_views == d.V && t.n_pts == d.N && t.n_obs == d.M) { *action = SFM_SYNC_REUSE; return SFM_OK; }
  const long long M = d.M, uploaded = p->upload_bytes;
  // the store's list IS the merged (point, camera)-sorted list: adopt it
  const int st = ba_grow(p, t.n_views, t.n_pts, t.n_obs, n_new_cams, "sfm_ba_sync_tracks", [&](const BaDev& e) -> int {
    SFM_TRY(ba_fill_from_tracks(e, t, s));
    return ba_carry_state(p, e, cams_new, pts_new);
  });
  if (st != SFM_OK) { p->upload_bytes = uploaded; return st; }
  *action = SFM_SYNC_GROWN;
  if (n_new_obs) *n_new_obs = (int64_t)(t.n_obs - M);
  return SFM_OK;
}

int sfm_ba_get_structure(sfm_ba_problem* p, int* pt_ptr, int* cam_idx, double* uv_norm) {
  SFM_TRY(ba_check_handle(p));
  const BaDev& d = p->dev;
  hipStream_t s = p->stream;
  const size_t m = (size_t)d.M;
  if (pt_ptr) SFM_HIP(hipMemcpyAsync(pt_ptr, d.pt_ptr, sizeof(int) * ((size_t)d.N + 1), hipMemcpyDeviceToHost, s));
  if (cam_idx && m > 0) SFM_HIP(hipMemcpyAsync(cam_idx, d.cam_idx, sizeof(int) * m, hipMemcpyDeviceToHost, s));
  if (uv_norm && m > 0) {
    SFM_HIP(hipMemcpyAsync(uv_norm, d.u, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(uv_norm + m, d.v, sizeof(double) * m, hipMemcpyDeviceToHost, s));
  }
  return stream_sync(s);
}

int sfm_ba_points_ptr(sfm_ba_problem* p, void** d_px, void** d_py, void** d_pz, int* n_pts) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));           // the deferred back substitution still has to move the points
  if (d_px) *d_px = p->dev.px;
  if (d_py) *d_py = p->dev.py;
  if (d_pz) *d_pz = p->dev.pz;
  if (n_pts) *n_pts = p->dev.N;
  return SFM_OK;
}

int sfm_ba_stream(sfm_ba_problem* p, void** hip_stream) {
  SFM_TRY(ba_check_handle(p));
  if (hip_stream) *hip_stream = p->stream;
  return SFM_OK;
}

int sfm_ba_reduced_buffer(sfm_ba_problem* p, void** device_ptr, int64_t* n_doubles, int* ld) {
  SFM_TRY(ba_check_handle(p));
  if (device_ptr) *device_ptr = p->dev.red;
  if (n_doubles) *n_doubles = (int64_t)red_size(p->dev.nbk);
  if (ld) *ld = p->dev.nbk * kNB;
  return SFM_OK;
}

int sfm_ba_bind_reduced_buffer(sfm_ba_problem* p, void* device_ptr, int64_t n_doubles) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));           // the deferred kernel clears the buffer that is bound now
  const int64_t need = (int64_t)red_size(p->dev.nbk);
  ba_graph_drop(p);
  p->red_clean = false;
  if (device_ptr == nullptr) { p->dev.red = p->own_red; return SFM_OK; }
  if (n_doubles < need) { set_error("reduced buffer too small: %lld < %lld doubles", (long long)n_doubles, (long long)need); return SFM_E_SHAPE; }
  p->dev.red = static_cast<double*>(device_ptr);
  return SFM_OK;
}

int sfm_ba_set_comm(sfm_ba_problem* p, sfm_comm* comm) {
  SFM_TRY(ba_check_handle(p));
  SFM_TRY(ba_flush(p));
  ba_graph_drop(p);          // a captured iteration body has no collective in it
  SFM_TRY(comm_attach(comm, +1));
  if (p->comm) { SFM_HIP(hipStreamSynchronize(p->stream)); (void)comm_attach(p->comm, -1); }      // no collective of the old one in flight
  p->comm = comm;
  return SFM_OK;
}

int sfm_ba_kernel_time(sfm_ba_problem* p, int kernel_id, double* total_ms, int* launches) {
  SFM_TRY(ba_check_handle(p));
  if (kernel_id < 0 || kernel_id >= SFM_K_COUNT) { set_error("bad kernel id %d", kernel_id); return SFM_E_SHAPE; }
  SFM_HIP(hipStreamSynchronize(p->stream));
  KernelTimer& t = p->timers[kernel_id];
  double tot = 0;
  for (int i = 0; i < t.used; ++i) {
    float ms = 0;
    SFM_HIP(hipEventElapsedTime(&ms, t.ev[i].first, t.ev[i].second));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = t.used;
  return SFM_OK;
}

namespace sfm { __global__ void ba_noop_kernel() {} }

int sfm_ba_event_overhead(sfm_ba_problem* p, int n, double* avg_ms) {
  SFM_TRY(ba_check_handle(p));
  if (n < 1 || avg_ms == nullptr) { set_error("sfm_ba_event_overhead: bad arguments"); return SFM_E_SHAPE; }
  hipStream_t s = p->stream;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev((size_t)n);
  for (auto& e : ev) { SFM_HIP(hipEventCreate(&e.first)); SFM_HIP(hipEventCreate(&e.second)); }
  // the same pattern ba_tick brackets a kernel class with, around a kernel that does nothing, between other work
  for (auto& e : ev) {
    ba_noop_kernel<<<1, 64, 0, s>>>();
    SFM_HIP(hipEventRecord(e.first, s));
    ba_noop_kernel<<<1, 64, 0, s>>>();
    SFM_HIP(hipEventRecord(e.second, s));
    ba_noop_kernel<<<1, 64, 0, s>>>();
  }
  SFM_HIP(hipStreamSynchronize(s));
  double tot = 0;
  for (auto& e : ev) {
    float ms = 0;
    SFM_HIP(hipEventElapsedTime(&ms, e.first, e.second));
    tot += ms;
    (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
  }
  *avg_ms = tot / n;
  return SFM_OK;
}

int sfm_ba_debug_stamps(sfm_ba_problem* p, unsigned long long* out, int n) {
  SFM_TRY(ba_check_handle(p));
  if (p->stamps == nullptr || n < 0 || n > 1024) { set_error("debug stamps not enabled (SFM_OPT_DEBUG bit 8)"); return SFM_E_SHAPE; }
  SFM_HIP(hipStreamSynchronize(p->stream));
  SFM_HIP(hipMemcpy(out, p->stamps, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  return SFM_OK;
}

int sfm_ba_reset_timing(sfm_ba_problem* p) {
  SFM_TRY(ba_check_handle(p));
  SFM_HIP(hipStreamSynchronize(p->stream));
  for (auto& t : p->timers) { t.used = 0; t.calls = 0; t.open = false; }
  return SFM_OK;
}

int sfm_ba_solve(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv_norm, double* cams,
                 double* pts, double lambda, int iters, int quirks) {
  sfm_ba_problem* p = nullptr;
  SFM_TRY(sfm_ba_create(V, N, M, pt_ptr, cam_idx, uv_norm, &p));
  int st = sfm_ba_set_state(p, cams, pts);
  if (st == SFM_OK) st = sfm_ba_iterate(p, lambda, iters, quirks);
  if (st == SFM_OK) st = sfm_ba_get_state(p, cams, pts);
  sfm_ba_destroy(p);
  return st;
}

int sfm_ba_residual_jacobian(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv_norm,
                             const double* cams, const double* pts, int quirks, double* r, double* Jp, double* Jx) {
  sfm_ba_problem* p = nullptr;
  SFM_TRY(sfm_ba_create(V, N, M, pt_ptr, cam_idx, uv_norm, &p));
  auto run = [&]() -> int {
    SFM_TRY(sfm_ba_set_state(p, cams, pts));
    SFM_TRY(ba_enqueue_prep(p));
    if (M == 0) return SFM_OK;
    hipStream_t s = p->stream;
    DevBuf<double> dr, djp, djx;
    SFM_TRY(dr.alloc(2 * (size_t)M, s)); SFM_TRY(djp.alloc(14 * (size_t)M, s)); SFM_TRY(djx.alloc(6 * (size_t)M, s));
    ba_enqueue_residual_jacobian(p, quirks, dr.p, djp.p, djx.p);
    SFM_HIP(hipGetLastError());
    SFM_TRY(dr.download(r, 2 * (size_t)M, s)); SFM_TRY(djp.download(Jp, 14 * (size_t)M, s)); SFM_TRY(djx.download(Jx, 6 * (size_t)M, s));
    int st[2] = {0, 0};
    SFM_HIP(hipMemcpyAsync(st, p->dev.status, sizeof(st), hipMemcpyDeviceToHost, s));
    SFM_TRY(stream_sync(s));
    if (st[0] != SFM_OK) { set_error("bundle adjustment: %s for camera %d", status_name(st[0]), st[1]); return st[0]; }
    return SFM_OK;
  };
  const int st = run();
  sfm_ba_destroy(p);
  return st;
}

int sfm_ba_reduced_system(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv_norm,
                          const double* cams, const double* pts, double lambda, int quirks, int schur_mode, double* S,
                          double* rhs) {
  return sfm_ba_reduced_system_loss(V, N, M, pt_ptr, cam_idx, uv_norm, cams, pts, lambda, quirks, schur_mode, SFM_LOSS_NONE, 0.0, S, rhs);
}

int sfm_ba_reduced_system_loss(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx, const double* uv_norm,
                               const double* cams, const double* pts, double lambda, int quirks, int schur_mode,
                               int loss_kind, double loss_delta, double* S, double* rhs) {
  sfm_ba_problem* p = nullptr;
  SFM_TRY(sfm_ba_create(V, N, M, pt_ptr, cam_idx, uv_norm, &p));
  auto run = [&]() -> int {
    SFM_TRY(sfm_ba_set_option(p, SFM_OPT_SCHUR, schur_mode));
    SFM_TRY(sfm_ba_set_loss(p, loss_kind, loss_delta));
    SFM_TRY(sfm_ba_set_state(p, cams, pts));
    SFM_TRY(ba_enqueue_linearize_reduce(p, lambda, quirks));
    hipStream_t s = p->stream;
    const BaDev& d = p->dev;
    DevBuf<double> dS, drhs;
    SFM_TRY(dS.alloc((size_t)d.P * d.P, s)); SFM_TRY(drhs.alloc((size_t)d.P, s));
    ba_enqueue_symmetrize(p, lambda, dS.p, drhs.p);
    SFM_HIP(hipGetLastError());
    SFM_TRY(dS.download(S, (size_t)d.P * d.P, s));
    SFM_TRY(drhs.download(rhs, (size_t)d.P, s));
    int st[2] = {0, 0};
    SFM_HIP(hipMemcpyAsync(st, d.status, sizeof(st), hipMemcpyDeviceToHost, s));
    SFM_TRY(stream_sync(s));
    if (st[0] != SFM_OK) { set_error("bundle adjustment: %s for camera %d", status_name(st[0]), st[1]); return st[0]; }
    return SFM_OK;
  };
  const int st = run();
  sfm_ba_destroy(p);
  return st;
}

}  // extern "C"
