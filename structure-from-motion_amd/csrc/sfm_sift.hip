// sfm_sift.hip — SIFT keypoints and descriptors of ViewProcessor.__extract_keys (view_processor.py:199-202,
// cv.SIFT_create().detectAndCompute(img, None)), by the contract of INTEGRATION.md 'SIFT detection' and its NumPy
// statement tests/_sift_numpy.py.
//
// Launch sequence of one image:
//   sift_base_kernel       gray conversion + x2 bilinear upsampling (exact: every value is a multiple of 1/16)
//   sift_blur_row/col      separable Gaussian, row pass then column pass, taps summed from the leftmost one up
//   sift_down_kernel       first level of octave o > 0 = level L of octave o - 1, every other pixel
//   sift_dog_kernel        the L + 2 DoG levels of one octave
//   sift_extrema_kernel    26-neighbour extrema of layers 1..L + adjustLocalExtrema, appended by an integer atomic
//   sift_orient_kernel     one wave per refined keypoint: 36-bin histogram, smoothing, peaks
//   (host)                 stable sort + removeDuplicatedSorted + the firstOctave fixup over the oriented list
//   sift_descr_kernel      one wave per final keypoint: 4 x 4 x 8 histogram, normalisation, saturate_cast<uchar>
//
// Bit-exactness with the stand-in: contraction is off for the whole file, every division and square root is the
// correctly rounded one (hipcc's default), and transcendental functions run in double and are rounded to float, as
// the stand-in's precise mode does.  Histograms are summed in sample order by lanes that own their bins (no float
// atomics), so every result is the same from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "sfm_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int IMG_BORDER = 5;
constexpr int MAX_INTERP_STEPS = 5;
constexpr int ORI_BINS = 36;
constexpr int DESCR_W = 4;
constexpr int DESCR_BINS = 8;
constexpr int DESCR_LEN = DESCR_W * DESCR_W * DESCR_BINS;
constexpr int MAX_TAPS = 4095;
constexpr int PRE_CAPACITY0 = 1 << 16;
constexpr float FLT_EPS = 1.1920928955078125e-7f;

struct PreKp {                      // a refined keypoint before orientation (pyramid octave coordinates)
  float x, y, size, response;
  int octave;                       // packed cv2 field, before the firstOctave fixup
  int o, layer, r, c;
};

struct Level {                      // one Gaussian level as the orientation / descriptor kernels read it
  const float* p;
  int h, w;
};

struct DescIn {
  float ptx, pty, scl, ori;
  int level;
};

__host__ __device__ inline int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
  }
  return i;
}

__device__ inline float atan2_deg(float y, float x) {
  double d = atan2((double)y, (double)x) * (180.0 / 3.14159265358979323846);
  if (d < 0) d += 360.0;
  float f = (float)d;
  return f >= 360.0f ? 0.0f : f;
}

__device__ inline float exp_rn(float a) { return (float)exp((double)a); }

// ---- pyramid ----------------------------------------------------------------------------------------------------
__global__ void sift_base_kernel(const uint8_t* __restrict__ img, int h, int w, int ch, int64_t stride,
                                 float* __restrict__ base) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
  if (X >= 2 * w || Y >= 2 * h) return;
  auto gray = [&](int y, int x) -> float {
    const uint8_t* p = img + (int64_t)y * stride;
    if (ch == 1) return (float)p[x];
    const int b = p[3 * x], g = p[3 * x + 1], r = p[3 * x + 2];
    return (float)((1868 * b + 9617 * g + 4899 * r + 8192) >> 14);
  };
  const int i = Y >> 1, i2 = (Y & 1) ? min(i + 1, h - 1) : max(i - 1, 0);
  const int j = X >> 1, j2 = (X & 1) ? min(j + 1, w - 1) : max(j - 1, 0);
  const float a = 0.75f * gray(i, j) + 0.25f * gray(i, j2);
  const float b = 0.75f * gray(i2, j) + 0.25f * gray(i2, j2);
  base[(int64_t)Y * (2 * w) + X] = 0.75f * a + 0.25f * b;
}

__global__ void sift_blur_row_kernel(const float* __restrict__ src, float* __restrict__ dst, int h, int w,
                                     const float* __restrict__ wt, int ksize) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const int r = ksize / 2;
  const float* row = src + (int64_t)y * w;
  float acc = 0.0f;
  if (x >= r && x + r < w) {
    for (int t = 0; t < ksize; ++t) acc = t == 0 ? wt[0] * row[x - r] : acc + wt[t] * row[x + t - r];
  } else {
    for (int t = 0; t < ksize; ++t) {
      const float p = wt[t] * row[reflect101(x + t - r, w)];
      acc = t == 0 ? p : acc + p;
    }
  }
  dst[(int64_t)y * w + x] = acc;
}

__global__ void sift_blur_col_kernel(const float* __restrict__ src, float* __restrict__ dst, int h, int w,
                                     const float* __restrict__ wt, int ksize) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const int r = ksize / 2;
  float acc = 0.0f;
  for (int t = 0; t < ksize; ++t) {
    const float p = wt[t] * src[(int64_t)reflect101(y + t - r, h) * w + x];
    acc = t == 0 ? p : acc + p;
  }
  dst[(int64_t)y * w + x] = acc;
}

__global__ void sift_down_kernel(const float* __restrict__ src, int sw, float* __restrict__ dst, int h, int w) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  dst[(int64_t)y * w + x] = src[(int64_t)(2 * y) * sw + 2 * x];
}

__global__ void sift_dog_kernel(const float* __restrict__ g, float* __restrict__ d, int64_t plane, int levels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane * levels) return;
  d[i] = g[i + plane] - g[i];
}

// ---- extrema + adjustLocalExtrema ---------------------------------------------------------------------------------
struct Derivs {
  float dD[3], H[3][3], v, dxx, dyy, dxy;
};

__device__ inline void derivs(const float* dog, int64_t plane, int w, int lay, int r, int c, Derivs& o) {
  const float img_scale = 1.0f / 255.0f;
  const float deriv_scale = img_scale * 0.5f;
  const float cross_scale = img_scale * 0.25f;
  auto at = [&](int dl, int dr, int dc) { return dog[(int64_t)(lay + dl) * plane + (int64_t)(r + dr) * w + (c + dc)]; };
  o.dD[0] = (at(0, 0, 1) - at(0, 0, -1)) * deriv_scale;
  o.dD[1] = (at(0, 1, 0) - at(0, -1, 0)) * deriv_scale;
  o.dD[2] = (at(1, 0, 0) - at(-1, 0, 0)) * deriv_scale;
  o.v = at(0, 0, 0);
  const float v2 = o.v * 2.0f;
  const float dxx = (at(0, 0, 1) + at(0, 0, -1) - v2) * img_scale;
  const float dyy = (at(0, 1, 0) + at(0, -1, 0) - v2) * img_scale;
  const float dss = (at(1, 0, 0) + at(-1, 0, 0) - v2) * img_scale;
  const float dxy = (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1)) * cross_scale;
  const float dxs = (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1)) * cross_scale;
  const float dys = (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0)) * cross_scale;
  o.H[0][0] = dxx; o.H[0][1] = dxy; o.H[0][2] = dxs;
  o.H[1][0] = dxy; o.H[1][1] = dyy; o.H[1][2] = dys;
  o.H[2][0] = dxs; o.H[2][1] = dys; o.H[2][2] = dss;
  o.dxx = dxx; o.dyy = dyy; o.dxy = dxy;
}

__device__ inline void swap_rows(float (&a)[3][3], float (&b)[3], int r0, int r1) {
  for (int k = 0; k < 3; ++k) { const float t = a[r0][k]; a[r0][k] = a[r1][k]; a[r1][k] = t; }
  const float t = b[r0]; b[r0] = b[r1]; b[r1] = t;
}

// Gaussian elimination with partial pivoting, the operation sequence of _solve3 in the stand-in; a zero pivot gives 0
__device__ inline void solve3(float (&a)[3][3], float (&b)[3], float (&x)[3]) {
  int piv = 0;
  if (fabsf(a[1][0]) > fabsf(a[piv][0])) piv = 1;
  if (fabsf(a[2][0]) > fabsf(a[piv][0])) piv = 2;
  if (piv) swap_rows(a, b, 0, piv);
  x[0] = x[1] = x[2] = 0.0f;
  if (a[0][0] == 0.0f) return;
  for (int r = 1; r < 3; ++r) {
    const float f = a[r][0] / a[0][0];
    a[r][1] = a[r][1] - f * a[0][1];
    a[r][2] = a[r][2] - f * a[0][2];
    b[r] = b[r] - f * b[0];
  }
  if (fabsf(a[2][1]) > fabsf(a[1][1])) swap_rows(a, b, 1, 2);
  if (a[1][1] == 0.0f) return;
  const float f = a[2][1] / a[1][1];
  a[2][2] = a[2][2] - f * a[1][2];
  b[2] = b[2] - f * b[1];
  if (a[2][2] == 0.0f) return;
  const float x2 = b[2] / a[2][2];
  const float x1 = (b[1] - a[1][2] * x2) / a[1][1];
  const float x0 = ((b[0] - a[0][1] * x1) - a[0][2] * x2) / a[0][0];
  x[0] = x0; x[1] = x1; x[2] = x2;
}

// one thread per (layer 1..L, r, c) of the interior; dog holds the L + 2 levels of octave o back to back
__global__ void sift_extrema_kernel(const float* __restrict__ dog, int h, int w, int o, int L, float threshold,
                                    float contrast, float edge, float sigma, PreKp* __restrict__ out, int capacity,
                                    int* __restrict__ count) {
  const int c = IMG_BORDER + blockIdx.x * blockDim.x + threadIdx.x;
  const int r = IMG_BORDER + blockIdx.y;
  const int lay0 = 1 + blockIdx.z;
  if (c >= w - IMG_BORDER || r >= h - IMG_BORDER) return;
  const int64_t plane = (int64_t)h * w;
  const float* cur = dog + lay0 * plane;
  const float val = cur[(int64_t)r * w + c];
  if (!(fabsf(val) > threshold)) return;
  bool is_max = val > 0, is_min = val < 0;
  for (int dl = -1; dl <= 1; ++dl)
    for (int dr = -1; dr <= 1; ++dr)
      for (int dc = -1; dc <= 1; ++dc) {
        if (dl == 0 && dr == 0 && dc == 0) continue;
        const float nb = dog[(lay0 + dl) * plane + (int64_t)(r + dr) * w + (c + dc)];
        is_max = is_max && val >= nb;
        is_min = is_min && val <= nb;
      }
  if (!is_max && !is_min) return;

  int rr = r, cc = c, lay = lay0;
  float xc = 0, xr = 0, xi = 0;
  Derivs d;
  int i = 0;
  for (; i < MAX_INTERP_STEPS; ++i) {
    derivs(dog, plane, w, lay, rr, cc, d);
    float X[3];
    solve3(d.H, d.dD, X);
    xi = -X[2]; xr = -X[1]; xc = -X[0];
    if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
    const float big = (float)(2147483647 / 3);
    if (fabsf(xi) > big || fabsf(xr) > big || fabsf(xc) > big) return;
    cc += (int)rintf(xc);
    rr += (int)rintf(xr);
    lay += (int)rintf(xi);
    if (lay < 1 || lay > L || cc < IMG_BORDER || cc >= w - IMG_BORDER || rr < IMG_BORDER || rr >= h - IMG_BORDER) return;
  }
  if (i >= MAX_INTERP_STEPS) return;
  derivs(dog, plane, w, lay, rr, cc, d);
  const float t = d.dD[0] * xc + d.dD[1] * xr + d.dD[2] * xi;
  const float contr = d.v * (1.0f / 255.0f) + t * 0.5f;
  if (fabsf(contr) * (float)L - contrast < 0.0f) return;
  const float tr = d.dxx + d.dyy;
  const float det = d.dxx * d.dyy - d.dxy * d.dxy;
  if (det <= 0 || tr * tr * edge >= (edge + 1.0f) * (edge + 1.0f) * det) return;
  PreKp k;
  const float scale = (float)(1 << o);
  k.x = ((float)cc + xc) * scale;
  k.y = ((float)rr + xr) * scale;
  const float arg = ((float)lay + xi) / (float)L;
  k.size = sigma * (float)exp2((double)arg) * scale * 2.0f;
  k.response = fabsf(contr);
  k.octave = o + (lay << 8) + ((int)rint(((double)xi + 0.5) * 255) << 16);
  k.o = o; k.layer = lay; k.r = rr; k.c = cc;
  const int slot = atomicAdd(count, 1);
  if (slot < capacity) out[slot] = k;
}

// ---- orientation: one 64-lane block per refined keypoint ----------------------------------------------------------
__global__ __launch_bounds__(64) void sift_orient_kernel(const PreKp* __restrict__ pre, const Level* __restrict__ levels,
                                                         int L, float* __restrict__ angles) {
  __shared__ int s_bin[64];
  __shared__ float s_val[64];
  __shared__ float s_hist[ORI_BINS];
  __shared__ float s_sm[ORI_BINS];
  const int lane = threadIdx.x;
  const PreKp k = pre[blockIdx.x];
  const Level lv = levels[k.o * (L + 3) + k.layer];
  const float scl = k.size * 0.5f / (float)(1 << k.o);
  const int radius = (int)rintf(4.5f * scl);
  const float sig = 1.5f * scl;
  const float expf_scale = -1.0f / (2.0f * sig * sig);
  const int side = 2 * radius + 1;
  const int total = side * side;
  float own = 0.0f;                                  // lane < 36 owns bin `lane`
  for (int base = 0; base < total; base += 64) {
    const int s = base + lane;
    int bin = -1;
    float v = 0.0f;
    if (s < total) {
      const int i = s / side - radius, j = s % side - radius;
      const int y = k.r + i, x = k.c + j;
      if (y > 0 && y < lv.h - 1 && x > 0 && x < lv.w - 1) {
        const float* p = lv.p + (int64_t)y * lv.w + x;
        const float dx = p[1] - p[-1];
        const float dy = p[-lv.w] - p[lv.w];
        const float wgt = exp_rn((float)(i * i + j * j) * expf_scale);
        const float ori = atan2_deg(dy, dx);
        const float mag = sqrtf(dx * dx + dy * dy);
        bin = (int)rintf((36.0f / 360.0f) * ori);
        if (bin >= ORI_BINS) bin -= ORI_BINS;
        if (bin < 0) bin += ORI_BINS;
        v = wgt * mag;
      }
    }
    s_bin[lane] = bin;
    s_val[lane] = v;
    __syncthreads();
    if (lane < ORI_BINS)
      for (int t = 0; t < 64; ++t)
        if (s_bin[t] == lane) own = own + s_val[t];
    __syncthreads();
  }
  if (lane < ORI_BINS) s_hist[lane] = own;
  __syncthreads();
  if (lane < ORI_BINS) {
    auto th = [&](int q) { return s_hist[(q + ORI_BINS) % ORI_BINS]; };
    s_sm[lane] = (th(lane - 2) + th(lane + 2)) * (1.0f / 16.0f) + (th(lane - 1) + th(lane + 1)) * (4.0f / 16.0f) +
                 th(lane) * (6.0f / 16.0f);
  }
  __syncthreads();
  if (lane < ORI_BINS) {
    float omax = s_sm[0];
    for (int q = 1; q < ORI_BINS; ++q) omax = fmaxf(omax, s_sm[q]);
    const float mag_thr = omax * 0.8f;
    const int l = lane > 0 ? lane - 1 : ORI_BINS - 1, r2 = lane < ORI_BINS - 1 ? lane + 1 : 0;
    const float hj = s_sm[lane], hl = s_sm[l], hr = s_sm[r2];
    float angle = __builtin_nanf("");
    if (hj > hl && hj > hr && hj >= mag_thr) {
      float bin = (float)lane + 0.5f * (hl - hr) / (hl - 2.0f * hj + hr);
      bin = bin < 0 ? (float)ORI_BINS + bin : bin >= ORI_BINS ? bin - (float)ORI_BINS : bin;
      angle = 360.0f - (360.0f / ORI_BINS) * bin;
      if (fabsf(angle - 360.0f) < FLT_EPS) angle = 0.0f;
    }
    angles[(int64_t)blockIdx.x * ORI_BINS + lane] = angle;
  }
}

// ---- descriptor: one 64-lane block per final keypoint -------------------------------------------------------------
// Lane q < 36 owns spatial cell (q / 6, q % 6) of the (d + 2) x (d + 2) x (n + 2) histogram and its 10 orientation
// bins; every chunk of 64 samples is staged in LDS and each owner adds the contributions for its cell in sample order.
__global__ __launch_bounds__(64) void sift_descr_kernel(const DescIn* __restrict__ in, const Level* __restrict__ levels,
                                                        float* __restrict__ out) {
  constexpr int d = DESCR_W, n = DESCR_BINS;
  __shared__ int s_cell[64];
  __shared__ int s_o0[64];
  __shared__ float s_v[8][64];
  __shared__ float s_dst[DESCR_LEN];
  __shared__ float s_scale;
  const int lane = threadIdx.x;
  const DescIn k = in[blockIdx.x];
  const Level lv = levels[k.level];
  const int px = (int)rintf(k.ptx), py = (int)rintf(k.pty);
  float cos_t = (float)cos((double)(k.ori * (float)(3.14159265358979323846 / 180)));
  float sin_t = (float)sin((double)(k.ori * (float)(3.14159265358979323846 / 180)));
  const float bins_per_rad = (float)n / 360.0f;
  const float exp_scale = -1.0f / ((float)(d * d) * 0.5f);
  const float hist_width = 3.0f * k.scl;
  int radius = (int)rintf(hist_width * 1.4142135623730951f * (float)(d + 1) * 0.5f);
  radius = min(radius, (int)sqrt((double)lv.w * lv.w + (double)lv.h * lv.h));
  cos_t = cos_t / hist_width;
  sin_t = sin_t / hist_width;
  const int side = 2 * radius + 1;
  const int total = side * side;
  const int R = lane / (d + 2), C = lane % (d + 2);
  float hist[n + 2];
#pragma unroll
  for (int q = 0; q < n + 2; ++q) hist[q] = 0.0f;
  for (int base = 0; base < total; base += 64) {
    const int s = base + lane;
    int cell = -1, o0 = 0;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s < total) {
      const int i = s / side - radius, j = s % side - radius;
      const float c_rot = (float)j * cos_t - (float)i * sin_t;
      const float r_rot = (float)j * sin_t + (float)i * cos_t;
      float rbin = r_rot + (float)(d / 2) - 0.5f;
      float cbin = c_rot + (float)(d / 2) - 0.5f;
      const int rr = py + i, cc = px + j;
      if (rbin > -1 && rbin < d && cbin > -1 && cbin < d && rr > 0 && rr < lv.h - 1 && cc > 0 && cc < lv.w - 1) {
        const float* p = lv.p + (int64_t)rr * lv.w + cc;
        const float dx = p[1] - p[-1];
        const float dy = p[-lv.w] - p[lv.w];
        const float wgt = exp_rn((c_rot * c_rot + r_rot * r_rot) * exp_scale);
        const float ori = atan2_deg(dy, dx);
        float obin = (ori - k.ori) * bins_per_rad;
        const float mag = sqrtf(dx * dx + dy * dy) * wgt;
        const int r0 = (int)floorf(rbin), c0 = (int)floorf(cbin);
        o0 = (int)floorf(obin);
        rbin = rbin - (float)r0;
        cbin = cbin - (float)c0;
        obin = obin - (float)o0;
        if (o0 < 0) o0 += n;
        if (o0 >= n) o0 -= n;
        const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
        const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
        const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
        v[7] = v_rc11 * obin; v[6] = v_rc11 - v[7];
        v[5] = v_rc10 * obin; v[4] = v_rc10 - v[5];
        v[3] = v_rc01 * obin; v[2] = v_rc01 - v[3];
        v[1] = v_rc00 * obin; v[0] = v_rc00 - v[1];
        cell = (r0 + 1) * (d + 2) + (c0 + 1);
      }
    }
    s_cell[lane] = cell;
    s_o0[lane] = o0;
#pragma unroll
    for (int q = 0; q < 8; ++q) s_v[q][lane] = v[q];
    __syncthreads();
    if (lane < (d + 2) * (d + 2)) {
      for (int t = 0; t < 64; ++t) {
        const int ce = s_cell[t];
        if (ce < 0) continue;
        const int dr = R - ce / (d + 2), dc = C - ce % (d + 2);
        if (dr < 0 || dr > 1 || dc < 0 || dc > 1) continue;
        const int pair = 2 * (2 * dr + dc);         // (0,0) v000 v001, (0,1) v010 v011, (1,0) v100 v101, (1,1) v110 v111
        const float a = s_v[pair][t], b = s_v[pair + 1][t];
        const int oo = s_o0[t];
#pragma unroll
        for (int q = 0; q < n + 2; ++q) {
          if (q == oo) hist[q] = hist[q] + a;
          if (q == oo + 1) hist[q] = hist[q] + b;
        }
      }
    }
    __syncthreads();
  }
  if (R >= 1 && R <= d && C >= 1 && C <= d && lane < (d + 2) * (d + 2)) {
    hist[0] = hist[0] + hist[n];
    hist[1] = hist[1] + hist[n + 1];
#pragma unroll
    for (int q = 0; q < n; ++q) s_dst[((R - 1) * d + (C - 1)) * n + q] = hist[q];
  }
  __syncthreads();
  if (lane == 0) {
    float nrm2 = 0.0f;
    for (int q = 0; q < DESCR_LEN; ++q) nrm2 = nrm2 + s_dst[q] * s_dst[q];
    const float thr = sqrtf(nrm2) * 0.2f;
    nrm2 = 0.0f;
    for (int q = 0; q < DESCR_LEN; ++q) {
      const float val = fminf(s_dst[q], thr);
      s_dst[q] = val;
      nrm2 = nrm2 + val * val;
    }
    s_scale = 512.0f / fmaxf(sqrtf(nrm2), FLT_EPS);
  }
  __syncthreads();
  for (int q = lane; q < DESCR_LEN; q += 64) {
    const float r = rintf(s_dst[q] * s_scale);
    out[(int64_t)blockIdx.x * DESCR_LEN + q] = fminf(fmaxf(r, 0.0f), 255.0f);
  }
}

// ---- host helpers -----------------------------------------------------------------------------------------------
int gaussian_kernel(double sigma, std::vector<float>& w) {
  const int ksize = (int)std::nearbyint(sigma * 8 + 1) | 1;
  if (ksize < 1 || ksize > MAX_TAPS) return SFM_E_SHAPE;
  std::vector<double> t(ksize);
  double sum = 0;
  for (int i = 0; i < ksize; ++i) {
    const double x = i - (ksize - 1) * 0.5;
    t[i] = std::exp((-0.5 / (sigma * sigma)) * x * x);
    sum += t[i];
  }
  sum = 1.0 / sum;
  w.resize(ksize);
  for (int i = 0; i < ksize; ++i) w[i] = (float)(t[i] * sum);
  return SFM_OK;
}

int octave_count(int h, int w) {
  return (int)std::nearbyint(std::log2((double)std::min(2 * h, 2 * w)) - 2) + 1;
}

}  // namespace

struct sfm_sift_result {
  int n_layers = 3;
  int n_octaves = 0;
  std::vector<int> oct_h, oct_w;
  std::vector<int64_t> gauss_off, dog_off;          // float offsets of octave o's first level in `pyr`
  float* pyr = nullptr;                             // kept pyramid (SFM_SIFT keep_pyramid), else null
  std::vector<PreKp> pre;
  std::vector<float> x, y, size, angle, response, desc;
  std::vector<int> octave;
};

using namespace sfm;

namespace {

int launch_blur(const float* src, float* tmp, float* dst, int h, int w, const float* d_wt, int ksize, hipStream_t st) {
  const dim3 grid((unsigned)((w + 255) / 256), (unsigned)h);
  sift_blur_row_kernel<<<grid, 256, 0, st>>>(src, tmp, h, w, d_wt, ksize);
  sift_blur_col_kernel<<<grid, 256, 0, st>>>(tmp, dst, h, w, d_wt, ksize);
  SFM_HIP(hipGetLastError());
  return SFM_OK;
}

bool kp_less(const sfm_sift_result& r, int a, int b) {        // KeyPoint_LessThan (class_id is -1 for all)
  if (r.x[a] != r.x[b]) return r.x[a] < r.x[b];
  if (r.y[a] != r.y[b]) return r.y[a] < r.y[b];
  if (r.size[a] != r.size[b]) return r.size[a] > r.size[b];
  if (r.angle[a] != r.angle[b]) return r.angle[a] < r.angle[b];
  if (r.response[a] != r.response[b]) return r.response[a] > r.response[b];
  return r.octave[a] > r.octave[b];
}

int detect(const uint8_t* img, int h, int w, int ch, int64_t stride, const sfm_sift_params& prm, sfm_sift_result* res,
           hipStream_t st) {
  const int L = prm.n_octave_layers;
  res->n_layers = L;
  const int n_oct = octave_count(h, w);
  if (n_oct <= 0) return SFM_OK;
  res->n_octaves = n_oct;
  // level shapes and offsets: octave o holds L + 3 Gaussian levels, then L + 2 DoG levels
  int64_t total = 0;
  int oh = 2 * h, ow = 2 * w;
  for (int o = 0; o < n_oct; ++o) {
    if (o > 0) { oh /= 2; ow /= 2; }
    res->oct_h.push_back(oh);
    res->oct_w.push_back(ow);
    res->gauss_off.push_back(total);
    total += (int64_t)(L + 3) * oh * ow;
    res->dog_off.push_back(total);
    total += (int64_t)(L + 2) * oh * ow;
  }
  const int64_t plane0 = (int64_t)4 * h * w;
  // blur weights: the base blur, then sig[1..L+2]
  std::vector<std::vector<float>> wts(L + 3);
  const float s = (float)prm.sigma;
  const float sig_diff = sqrtf(std::max(s * s - 0.5f * 0.5f * 4.0f, 0.01f));
  SFM_TRY(gaussian_kernel((double)sig_diff, wts[0]));
  const double k = std::pow(2.0, 1.0 / L);
  for (int i = 1; i < L + 3; ++i) {
    const double prev = std::pow(k, (double)(i - 1)) * prm.sigma, tot = prev * k;
    if (gaussian_kernel(std::sqrt(tot * tot - prev * prev), wts[i]) != SFM_OK) {
      set_error("sfm_sift_detect: blur kernel of level %d has more than %d taps", i, MAX_TAPS);
      return SFM_E_SHAPE;
    }
  }
  std::vector<int> wt_off(L + 3), wt_len(L + 3);
  std::vector<float> wt_all;
  for (int i = 0; i < L + 3; ++i) { wt_off[i] = (int)wt_all.size(); wt_len[i] = (int)wts[i].size(); wt_all.insert(wt_all.end(), wts[i].begin(), wts[i].end()); }

  DevBuf<uint8_t> d_img;
  DevBuf<float> d_wt, d_tmp, d_base;
  float* pyr = nullptr;
  SFM_HIP(pool_alloc(reinterpret_cast<void**>(&pyr), (size_t)total * sizeof(float)));
  // an error return may leave kernels that write the pyramid in flight: drain the stream before the block goes back
  struct PyrGuard {
    float*& p; hipStream_t s; bool keep;
    ~PyrGuard() { if (!keep && p) { (void)hipStreamSynchronize(s); pool_free(p); } }
  } guard{pyr, st, false};
  SFM_TRY(d_img.upload(img, (size_t)stride * (h - 1) + (size_t)w * ch, st));
  SFM_TRY(d_wt.upload(wt_all.data(), wt_all.size(), st));
  SFM_TRY(d_tmp.alloc((size_t)plane0, st));
  SFM_TRY(d_base.alloc((size_t)plane0, st));
  {
    const dim3 grid((unsigned)((2 * w + 255) / 256), (unsigned)(2 * h));
    sift_base_kernel<<<grid, 256, 0, st>>>(d_img.p, h, w, ch, stride, d_base.p);
    SFM_HIP(hipGetLastError());
  }
  for (int o = 0; o < n_oct; ++o) {
    const int hh = res->oct_h[o], ww = res->oct_w[o];
    const int64_t plane = (int64_t)hh * ww;
    float* g = pyr + res->gauss_off[o];
    if (o == 0) {
      SFM_TRY(launch_blur(d_base.p, d_tmp.p, g, hh, ww, d_wt.p + wt_off[0], wt_len[0], st));
    } else {
      const float* src = pyr + res->gauss_off[o - 1] + (int64_t)L * res->oct_h[o - 1] * res->oct_w[o - 1];
      sift_down_kernel<<<dim3((unsigned)((ww + 255) / 256), (unsigned)hh), 256, 0, st>>>(src, res->oct_w[o - 1], g, hh, ww);
      SFM_HIP(hipGetLastError());
    }
    for (int i = 1; i < L + 3; ++i)
      SFM_TRY(launch_blur(g + (i - 1) * plane, d_tmp.p, g + i * plane, hh, ww, d_wt.p + wt_off[i], wt_len[i], st));
    const int64_t nd = plane * (L + 2);
    sift_dog_kernel<<<(unsigned)((nd + 255) / 256), 256, 0, st>>>(g, pyr + res->dog_off[o], plane, L + 2);
    SFM_HIP(hipGetLastError());
  }

  // extrema + refinement into an appended list; a list longer than the buffer is found again with a bigger one
  const float threshold = (float)std::floor(0.5 * prm.contrast_threshold / L * 255);
  int capacity = PRE_CAPACITY0;
  DevBuf<int> d_count;
  SFM_TRY(d_count.alloc(1, st));
  int n_pre = 0;
  DevBuf<PreKp> d_pre;
  for (int attempt = 0; attempt < 2; ++attempt) {
    SFM_TRY(d_pre.alloc((size_t)capacity, st));
    SFM_HIP(hipMemsetAsync(d_count.p, 0, sizeof(int), st));
    for (int o = 0; o < n_oct; ++o) {
      const int hh = res->oct_h[o], ww = res->oct_w[o];
      if (hh <= 2 * IMG_BORDER || ww <= 2 * IMG_BORDER) continue;
      const dim3 grid((unsigned)((ww - 2 * IMG_BORDER + 63) / 64), (unsigned)(hh - 2 * IMG_BORDER), (unsigned)L);
      sift_extrema_kernel<<<grid, 64, 0, st>>>(pyr + res->dog_off[o], hh, ww, o, L, threshold, (float)prm.contrast_threshold,
                                               (float)prm.edge_threshold, (float)prm.sigma, d_pre.p, capacity, d_count.p);
      SFM_HIP(hipGetLastError());
    }
    SFM_HIP(hipMemcpyAsync(&n_pre, d_count.p, sizeof(int), hipMemcpyDeviceToHost, st));
    SFM_TRY(stream_sync(st));
    if (n_pre <= capacity) break;
    capacity = n_pre;
    DevBuf<PreKp> fresh;
    std::swap(d_pre.p, fresh.p);                   // the old buffer goes back to the pool
  }
  if (n_pre > capacity) {                          // the count is deterministic, so the second pass fits; never read past it
    set_error("sfm_sift_detect: %d refined keypoints after resizing the list to %d", n_pre, capacity);
    return SFM_E_HIP;
  }
  res->pre.resize(n_pre);
  if (n_pre) SFM_TRY(d_pre.download(res->pre.data(), (size_t)n_pre, st));
  SFM_TRY(stream_sync(st));
  // the append order depends on the atomics: sort by the fields the contract defines (a fixed total order)
  std::sort(res->pre.begin(), res->pre.end(), [](const PreKp& a, const PreKp& b) {
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.size != b.size) return a.size > b.size;
    if (a.response != b.response) return a.response > b.response;
    return a.octave > b.octave;
  });

  std::vector<Level> levels((size_t)n_oct * (L + 3));
  for (int o = 0; o < n_oct; ++o)
    for (int i = 0; i < L + 3; ++i)
      levels[(size_t)o * (L + 3) + i] = Level{pyr + res->gauss_off[o] + (int64_t)i * res->oct_h[o] * res->oct_w[o], res->oct_h[o], res->oct_w[o]};
  DevBuf<Level> d_levels;
  SFM_TRY(d_levels.upload(levels.data(), levels.size(), st));

  std::vector<float> ang((size_t)n_pre * ORI_BINS);
  if (n_pre) {
    DevBuf<PreKp> d_sorted;
    DevBuf<float> d_ang;
    SFM_TRY(d_sorted.upload(res->pre.data(), (size_t)n_pre, st));
    SFM_TRY(d_ang.alloc(ang.size(), st));
    sift_orient_kernel<<<(unsigned)n_pre, 64, 0, st>>>(d_sorted.p, d_levels.p, L, d_ang.p);
    SFM_HIP(hipGetLastError());
    SFM_TRY(d_ang.download(ang.data(), ang.size(), st));
    SFM_TRY(stream_sync(st));
  }
  // the oriented list (keypoint-major, bin order), sorted, without duplicates, fixed up for firstOctave = -1
  sfm_sift_result all;
  for (int p = 0; p < n_pre; ++p)
    for (int j = 0; j < ORI_BINS; ++j) {
      const float a = ang[(size_t)p * ORI_BINS + j];
      if (a != a) continue;
      const PreKp& q = res->pre[p];
      all.x.push_back(q.x); all.y.push_back(q.y); all.size.push_back(q.size); all.angle.push_back(a);
      all.response.push_back(q.response); all.octave.push_back(q.octave);
    }
  std::vector<int> order(all.x.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return kp_less(all, a, b); });
  for (size_t t = 0; t < order.size(); ++t) {
    const int i = order[t];
    if (!res->x.empty() && all.x[i] * 0.5f == res->x.back() && all.y[i] * 0.5f == res->y.back() &&
        all.size[i] * 0.5f == res->size.back() && all.angle[i] == res->angle.back())
      continue;
    res->x.push_back(all.x[i] * 0.5f); res->y.push_back(all.y[i] * 0.5f); res->size.push_back(all.size[i] * 0.5f);
    res->angle.push_back(all.angle[i]); res->response.push_back(all.response[i]);
    res->octave.push_back((all.octave[i] & ~255) | ((all.octave[i] - 1) & 255));
  }
  const int n = (int)res->x.size();
  res->desc.assign((size_t)n * DESCR_LEN, 0.0f);
  if (n) {
    std::vector<DescIn> din(n);
    for (int i = 0; i < n; ++i) {                    // unpackOctave + calcDescriptors' scaling
      int oc = res->octave[i] & 255;
      oc = oc < 128 ? oc : (-128 | oc);
      const int layer = (res->octave[i] >> 8) & 255;
      const float scale = oc >= 0 ? 1.0f / (float)(1 << oc) : (float)(1 << -oc);
      float a = 360.0f - res->angle[i];
      if (std::fabs(a - 360.0f) < FLT_EPS) a = 0.0f;
      din[i] = DescIn{res->x[i] * scale, res->y[i] * scale, res->size[i] * scale * 0.5f, a, (oc + 1) * (L + 3) + layer};
    }
    DevBuf<DescIn> d_in;
    DevBuf<float> d_desc;
    SFM_TRY(d_in.upload(din.data(), din.size(), st));
    SFM_TRY(d_desc.alloc(res->desc.size(), st));
    sift_descr_kernel<<<(unsigned)n, 64, 0, st>>>(d_in.p, d_levels.p, d_desc.p);
    SFM_HIP(hipGetLastError());
    SFM_TRY(d_desc.download(res->desc.data(), res->desc.size(), st));
  }
  SFM_TRY(stream_sync(st));
  if (prm.keep_pyramid) { res->pyr = pyr; guard.keep = true; }
  return SFM_OK;
}

}  // namespace

extern "C" {

int sfm_sift_blur_kernel(double sigma, int capacity, float* weights, int* ksize) {
  if (!(sigma > 0) || !ksize) { set_error("sfm_sift_blur_kernel: bad sigma or null ksize"); return SFM_E_SHAPE; }
  std::vector<float> w;
  if (gaussian_kernel(sigma, w) != SFM_OK) { set_error("sfm_sift_blur_kernel: more than %d taps", MAX_TAPS); return SFM_E_SHAPE; }
  *ksize = (int)w.size();
  if (weights) std::memcpy(weights, w.data(), sizeof(float) * std::min<size_t>(w.size(), capacity > 0 ? capacity : 0));
  return SFM_OK;
}

int sfm_sift_detect(const uint8_t* img, int height, int width, int channels, int64_t row_stride_bytes,
                    const sfm_sift_params* params, sfm_sift_result** out) {
  if (!out) { set_error("sfm_sift_detect: out is NULL"); return SFM_E_SHAPE; }
  *out = nullptr;
  SFM_TRY(ensure_init());
  sfm_sift_params prm = {3, 0.04, 10.0, 1.6, 0, nullptr};
  if (params) prm = *params;
  if (!img || height < 1 || width < 1 || (channels != 1 && channels != 3) || row_stride_bytes < (int64_t)width * channels) {
    set_error("sfm_sift_detect: bad image (height %d, width %d, channels %d, row stride %lld)", height, width, channels,
              (long long)row_stride_bytes);
    return SFM_E_SHAPE;
  }
  if (height > (1 << 14) || width > (1 << 14)) { set_error("sfm_sift_detect: image larger than 16384 pixels a side"); return SFM_E_SHAPE; }
  if (prm.n_octave_layers < 1 || prm.n_octave_layers > 16 || !(prm.contrast_threshold >= 0) || !(prm.edge_threshold > 0) ||
      !(prm.sigma > 0) || !(prm.sigma < 64)) {
    set_error("sfm_sift_detect: bad parameters (layers %d, contrast %g, edge %g, sigma %g)", prm.n_octave_layers,
              prm.contrast_threshold, prm.edge_threshold, prm.sigma);
    return SFM_E_SHAPE;
  }
  hipStream_t st = prm.stream ? static_cast<hipStream_t>(prm.stream) : ctx().stream;
  sfm_sift_result* res = new sfm_sift_result();
  const int rc = detect(img, height, width, channels, row_stride_bytes, prm, res, st);
  if (rc != SFM_OK) { sfm_sift_result_destroy(res); return rc; }
  *out = res;
  return SFM_OK;
}

int sfm_sift_result_info(const sfm_sift_result* r, int what, int64_t* value) {
  if (!r) return SFM_E_HANDLE;
  if (!value) { set_error("sfm_sift_result_info: value is NULL"); return SFM_E_SHAPE; }
  switch (what) {
    case SFM_SIFT_INFO_N: *value = (int64_t)r->x.size(); return SFM_OK;
    case SFM_SIFT_INFO_N_OCTAVES: *value = r->n_octaves; return SFM_OK;
    case SFM_SIFT_INFO_N_PRE: *value = (int64_t)r->pre.size(); return SFM_OK;
    case SFM_SIFT_INFO_N_LAYERS: *value = r->n_layers; return SFM_OK;
    case SFM_SIFT_INFO_KEEPS_PYRAMID: *value = r->pyr != nullptr; return SFM_OK;
    default: set_error("sfm_sift_result_info: unknown item %d", what); return SFM_E_SHAPE;
  }
}

int sfm_sift_result_level_shape(const sfm_sift_result* r, int octave, int* height, int* width) {
  if (!r) return SFM_E_HANDLE;
  if (octave < 0 || octave >= r->n_octaves || !height || !width) { set_error("sfm_sift_result_level_shape: bad octave %d", octave); return SFM_E_SHAPE; }
  *height = r->oct_h[octave];
  *width = r->oct_w[octave];
  return SFM_OK;
}

int sfm_sift_result_copy(const sfm_sift_result* r, float* x, float* y, float* size, float* angle, float* response,
                         int32_t* octave, float* descriptors) {
  if (!r) return SFM_E_HANDLE;
  const size_t n = r->x.size();
  if (!n) return SFM_OK;
  if (x) std::memcpy(x, r->x.data(), n * sizeof(float));
  if (y) std::memcpy(y, r->y.data(), n * sizeof(float));
  if (size) std::memcpy(size, r->size.data(), n * sizeof(float));
  if (angle) std::memcpy(angle, r->angle.data(), n * sizeof(float));
  if (response) std::memcpy(response, r->response.data(), n * sizeof(float));
  if (octave) std::memcpy(octave, r->octave.data(), n * sizeof(int32_t));
  if (descriptors) std::memcpy(descriptors, r->desc.data(), r->desc.size() * sizeof(float));
  return SFM_OK;
}

int sfm_sift_result_copy_pre(const sfm_sift_result* r, float* x, float* y, float* size, float* response, int32_t* octave) {
  if (!r) return SFM_E_HANDLE;
  for (size_t i = 0; i < r->pre.size(); ++i) {
    const PreKp& k = r->pre[i];
    if (x) x[i] = k.x;
    if (y) y[i] = k.y;
    if (size) size[i] = k.size;
    if (response) response[i] = k.response;
    if (octave) octave[i] = k.octave;
  }
  return SFM_OK;
}

int sfm_sift_result_copy_level(const sfm_sift_result* r, int kind, int octave, int level, float* out) {
  if (!r) return SFM_E_HANDLE;
  if (!r->pyr) { set_error("sfm_sift_result_copy_level: the pyramid was not kept (keep_pyramid = 0)"); return SFM_E_SHAPE; }
  const int L = r->n_layers;
  const int n_lev = kind == SFM_SIFT_LEVEL_GAUSS ? L + 3 : L + 2;
  if ((kind != SFM_SIFT_LEVEL_GAUSS && kind != SFM_SIFT_LEVEL_DOG) || octave < 0 || octave >= r->n_octaves || level < 0 ||
      level >= n_lev || !out) {
    set_error("sfm_sift_result_copy_level: bad level (kind %d, octave %d, level %d)", kind, octave, level);
    return SFM_E_SHAPE;
  }
  const int64_t plane = (int64_t)r->oct_h[octave] * r->oct_w[octave];
  const int64_t off = (kind == SFM_SIFT_LEVEL_GAUSS ? r->gauss_off[octave] : r->dog_off[octave]) + level * plane;
  SFM_HIP(hipMemcpy(out, r->pyr + off, (size_t)plane * sizeof(float), hipMemcpyDeviceToHost));
  return SFM_OK;
}

int sfm_sift_result_destroy(sfm_sift_result* r) {
  if (!r) return SFM_E_HANDLE;
  if (r->pyr) pool_free(r->pyr);
  delete r;
  return SFM_OK;
}

}  // extern "C"
