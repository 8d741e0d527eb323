// Visualisation and training summaries on the GPU: what lets a person look at a run.
//   models/utils/flow_utils.py        make_color_wheel :14-42, compute_color :46-72, flow_to_image :74-100
//   models/adversarial_learner.py     collect_summaries :260-298 (flow images, the masked flow image, tf.summary.histogram of every
//                                     variable's gradient)
//   test_generator.py                 :93-117 (postprocess_image / postprocess_mask, cv2.addWeighted, cv2.resize to 384 x 640)
//                                     :101-106 once more at every frame's own size, without the resize and with the mask's contour, for a
//                                     ragged batch of untouched frames and final masks (overlay_native_ragged)
// The inputs already sit in plan buffers (image, flow, mask, pred, the flat gradient buffers); these kernels turn them into the uint8
// images and the bucket counts a writer stores, so that a summary step costs a few hundred microseconds of device time (profiles/NOTES.md) and two small copies.
// Written for exact agreement with the reference's arithmetic, not for a roofline.  Compiled with -ffp-contract=off (Makefile): the
// float32 radius u*u + v*v and every double expression below must round operation by operation like numpy.
#include <float.h>
#include <math.h>

#include "common.h"
#include "host_checks.h"
#include "rgb_groups.h"  // native_blend, rgb_group4: shared with instances.hip

namespace udet {

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce256(T v, T* sm /*[4]*/, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(sm[0], sm[1]), op(sm[2], sm[3]));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// flow_to_image
// ---------------------------------------------------------------------------------------------------------------------------------
// make_color_wheel (:14-42) divided by 255 (compute_color :64-65 divides on every use; the quotient is the same double): six ramps
// RY YG GC CB BM MR of 15, 6, 4, 11, 13, 6 entries, one channel at 255, one rising or falling as floor(255 i / len).  Built by the
// compiler: the table lives in constant memory, a dynamically indexed local array would live in scratch.
struct ColorWheel {
  double c[55][3];
};
constexpr ColorWheel make_color_wheel() {
  ColorWheel w{};
  const int len[6] = {15, 6, 4, 11, 13, 6}, full[6] = {0, 1, 1, 2, 2, 0}, ramp[6] = {1, 0, 2, 1, 0, 2};
  int col = 0;
  for (int s = 0; s < 6; ++s)
    for (int i = 0; i < len[s]; ++i, ++col) {
      const int r = 255 * i / len[s];
      for (int c = 0; c < 3; ++c) w.c[col][c] = 0.0;
      w.c[col][full[s]] = 255.0 / 255.0;
      w.c[col][ramp[s]] = (double)((s & 1) ? 255 - r : r) / 255.0;
    }
  return w;
}
__constant__ ColorWheel c_wheel = make_color_wheel();

#define FI_SPLIT 16  // workgroups (and partial maxima) per sample
// one flow sample as flow_to_image sees it (:85-89): a component beyond 1e7 zeroes both
__device__ __forceinline__ float2 flow_known(const float* __restrict__ flow, long i) {
  float2 v = *reinterpret_cast<const float2*>(flow + 2 * i);
  if (fabsf(v.x) > 1e7f || fabsf(v.y) > 1e7f) v = make_float2(0.f, 0.f);
  return v;
}
// stage 1: part[n][FI_SPLIT] = max over the workgroup's pixels of the float32 radius sqrtf(u*u + v*v), -1 (the reference's initial
// maxrad, :83) when it saw none.  sqrtf is correctly rounded and monotonic: the maximum of the roots is the root of the maximum.
// A NaN pixel is left out (see udet.h).
__global__ __launch_bounds__(256) void flow_maxrad_kernel(const float* __restrict__ flow, long HW, float* __restrict__ part) {
  __shared__ float sm[4];
  const int n = blockIdx.y;
  float m = -1.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)FI_SPLIT * 256) {
    const float2 v = flow_known(flow, n * HW + p);
    const float r2 = v.x * v.x + v.y * v.y;
    if (!isnan(r2)) m = fmaxf(m, r2);
  }
  m = block_reduce256(m, sm, [](float a, float b) { return fmaxf(a, b); });
  if (threadIdx.x == 0) part[n * FI_SPLIT + blockIdx.x] = m < 0.f ? -1.f : sqrtf(m);
}
// stage 2: compute_color (:46-72) of sample n divided by the running maximum over samples 0..n (:95-97), in double from the
// division on; optionally the object mask painted (127,127,127)
__global__ __launch_bounds__(256) void flow_colour_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                          const double* __restrict__ stats8, float threshold, int H, int W,
                                                          const float* __restrict__ part, unsigned char* __restrict__ rgb) {
  __shared__ float sm[4];
  const int n = blockIdx.y;
  const long HW = (long)H * W;
  float m = -1.f;
  for (int i = threadIdx.x; i < (n + 1) * FI_SPLIT; i += 256) m = fmaxf(m, part[i]);
  m = block_reduce256(m, sm, [](float a, float b) { return fmaxf(a, b); });
  const double den = (double)m + DBL_EPSILON;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  unsigned char* o = rgb + (n * HW + p) * 3;
  if (mask) {
    // disambiguate_forw_back (general_utils.py:100-109): the mask is complemented when it covers the image borders
    const bool flip = stats8[(long)n * 8] / (4.0 * W + 4.0 * H) >= 0.6;
    if ((mask[n * HW + p] > threshold) != flip) {
      o[0] = o[1] = o[2] = 127;
      return;
    }
  }
  const float2 v = flow_known(flow, n * HW + p);
  if (isnan(v.x) || isnan(v.y)) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const double u = (double)v.x / den, w = (double)v.y / den;
  const double rad = sqrt(u * u + w * w);
  const double a = atan2(-w, -u) / 3.141592653589793;
  const double fk = (a + 1.0) / 2.0 * 54.0 + 1.0;
  const int k0 = (int)floor(fk);
  const int k1 = k0 + 1 == 56 ? 1 : k0 + 1;
  const double f = fk - (double)k0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double col = (1.0 - f) * c_wheel.c[k0 - 1][c] + f * c_wheel.c[k1 - 1][c];
    col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
    o[c] = (unsigned char)(int)floor(255.0 * col);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// overlay_mask
// ---------------------------------------------------------------------------------------------------------------------------------
// OpenCV's 8-bit INTER_LINEAR coordinates along one axis: f = (d + 0.5) * in / out - 0.5 in float, taps (s, s + 1) clamped into the
// image with weight 0 on the clamped side, coefficients round(w * 2048)
__device__ __forceinline__ void linear_taps(int d, double scale, int in, int& i0, int& i1, int& c0, int& c1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= in - 1) { s = in - 1; f = 0.f; }
  i0 = s;
  i1 = min(s + 1, in - 1);
  c0 = (int)rintf((1.f - f) * 2048.f);
  c1 = (int)rintf(f * 2048.f);
}
// postprocess_image of one value, postprocess_mask's byte m of that channel, cv2.addWeighted(img, 0.5, mask, 0.4, 0)
__device__ __forceinline__ int overlay_blend(float x, int m) {
  const float t = fminf(fmaxf((x + 0.5f) * 255.f, 0.f), 255.f);
  const float b = (float)(int)t * 0.5f + (float)m * 0.4f;
  const int r = (int)rintf(b);
  return r < 0 ? 0 : (r > 255 ? 255 : r);
}
__global__ __launch_bounds__(256) void overlay_mask_kernel(const float* __restrict__ image, const float* __restrict__ mask,
                                                           const double* __restrict__ stats8, float threshold, int H, int W,
                                                           unsigned char* __restrict__ out, int OH, int OW, double sy, double sx) {
  const int n = blockIdx.y;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)OH * OW) return;
  const int dy = (int)(q / OW), dx = (int)(q - (long)dy * OW);
  const bool flip = stats8 && stats8[(long)n * 8] / (4.0 * W + 4.0 * H) >= 0.6;
  int y0, y1, b0, b1, x0, x1, a0, a1;
  linear_taps(dy, sy, H, y0, y1, b0, b1);
  linear_taps(dx, sx, W, x0, x1, a0, a1);
  const long base = (long)n * H * W;
  const long p00 = base + (long)y0 * W + x0, p01 = base + (long)y0 * W + x1, p10 = base + (long)y1 * W + x0, p11 = base + (long)y1 * W + x1;
  const int m00 = ((mask[p00] > threshold) != flip) ? 255 : 0, m01 = ((mask[p01] > threshold) != flip) ? 255 : 0;
  const int m10 = ((mask[p10] > threshold) != flip) ? 255 : 0, m11 = ((mask[p11] > threshold) != flip) ? 255 : 0;
  unsigned char* o = out + ((long)n * OH * OW + q) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int g = c == 1;  // the mask is painted into the middle channel only
    const int S0 = overlay_blend(image[p00 * 3 + c], g * m00) * a0 + overlay_blend(image[p01 * 3 + c], g * m01) * a1;
    const int S1 = overlay_blend(image[p10 * 3 + c], g * m10) * a0 + overlay_blend(image[p11 * 3 + c], g * m11) * a1;
    const int r = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    o[c] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// overlay_native_ragged
// ---------------------------------------------------------------------------------------------------------------------------------
// One workgroup owns a tile of ON_TH rows x ON_TW columns of one sample of the packed batch.
//   1. the foreground bits of the tile's rows plus `edge` rows above and below are packed into LDS, one __ballot per (row, word): a row
//      is 128 bits, bit p = column x0 - ON_LEFT + p; positions outside the frame are 1 (they never count as background);
//   2. the (2 edge + 1)^2 windowed minimum is two passes of ANDs on the packed words: a thread per row ANDs the row with its shifts
//      by 1 .. edge in both directions, then a thread per tile row ANDs 2 edge + 1 of those rows;
//   3. a thread takes four pixels of a row whose twelve colour bytes are three aligned 32-bit words: the row's groups start where the
//      element index offsets[i] + y W + x is a multiple of 4, so the tile's columns are [x0 - s, x0 + ON_TW - s) with s = (offsets[i] +
//      y W) mod 4 in that row (hence the ON_LEFT - edge = 4 spare columns, and a grid of ceil((max_w + 3) / ON_TW) tile columns).  A
//      group cut by a row end, and every group when image / out are not 4-byte aligned themselves, goes byte by byte.
#define ON_TH 32
#define ON_TW 64
#define ON_LEFT (4 + UDET_OVERLAY_MAX_EDGE)            // columns of the packed row in front of the tile's first
#define ON_ROWS (ON_TH + 2 * UDET_OVERLAY_MAX_EDGE)
static_assert(ON_LEFT + ON_TW + UDET_OVERLAY_MAX_EDGE <= 128, "a packed row is two 64-bit words");

// bits pos .. pos + 3 of the 128-bit row (lo, hi), 1 <= pos <= 124
__device__ __forceinline__ unsigned row_bits4(unsigned long long lo, unsigned long long hi, int pos) {
  return (unsigned)(pos < 64 ? (lo >> pos) | (hi << (64 - pos)) : hi >> (pos - 64)) & 15u;
}
__global__ __launch_bounds__(256) void overlay_native_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
                                                             const long long* __restrict__ offsets, const int* __restrict__ hw, int tiles_x,
                                                             float alpha, float beta, unsigned mask_rgb, int edge, unsigned edge_rgb,
                                                             unsigned char* __restrict__ out, int wide) {
  __shared__ unsigned long long F[ON_ROWS][2];  // foreground, row 0 = image row y0 - edge
  __shared__ unsigned long long Hm[ON_ROWS][2];  // its minimum over x - edge .. x + edge
  __shared__ unsigned long long E[ON_TH][2];     // the eroded mask of the tile's own rows
  const int n = blockIdx.y;
  const int H = hw[2 * n], W = hw[2 * n + 1];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * ON_TH, x0 = tx * ON_TW;
  if (y0 >= H || x0 - 3 >= W) return;  // beyond this sample's tiles (the whole workgroup: nothing below is reached)
  const long off = offsets[n];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int items = 2 * (ON_TH + 2 * edge);  // (row, word) pairs to pack

  // 1. pack: four (row, word) items per wave and round, the loads issued before the ballots.  Only the columns a contour of this tile
  // can depend on are read: [x0 - 3 - edge, x0 + ON_TW - 1 + edge] inside the frame.
  const int need_lo = max(x0 - 3 - edge, 0), need_hi = min(x0 + ON_TW - 1 + edge, W - 1);
  for (int it0 = wave; it0 < items; it0 += 16) {
    unsigned char v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + 4 * u;
      const int gy = y0 - edge + (it >> 1), gx = x0 - ON_LEFT + 64 * (it & 1) + lane;
      v[u] = 1;
      if (it < items && gy >= 0 && gy < H && gx >= need_lo && gx <= need_hi) v[u] = mask[off + (long)gy * W + gx];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + 4 * u;
      const unsigned long long b = __ballot(v[u] != 0);
      if (it < items && lane == 0) F[it >> 1][it & 1] = b;
    }
  }
  __syncthreads();

  // 2. the windowed minimum, separable; bits shifted in from beyond the 128 columns are 1 (no result that is used depends on them)
  if (edge > 0) {
    if ((int)threadIdx.x < ON_TH + 2 * edge) {
      const unsigned long long lo = F[threadIdx.x][0], hi = F[threadIdx.x][1];
      unsigned long long mlo = lo, mhi = hi;
      for (int d = 1; d <= edge; ++d) {
        mlo &= ((lo >> d) | (hi << (64 - d))) & ((lo << d) | (~0ull >> (64 - d)));
        mhi &= ((hi >> d) | (~0ull << (64 - d))) & ((hi << d) | (lo >> (64 - d)));
      }
      Hm[threadIdx.x][0] = mlo;
      Hm[threadIdx.x][1] = mhi;
    }
    __syncthreads();
    if (threadIdx.x < ON_TH) {
      unsigned long long mlo = ~0ull, mhi = ~0ull;
      for (int r = 0; r <= 2 * edge; ++r) {
        mlo &= Hm[threadIdx.x + r][0];
        mhi &= Hm[threadIdx.x + r][1];
      }
      E[threadIdx.x][0] = mlo;
      E[threadIdx.x][1] = mhi;
    }
    __syncthreads();
  }

  // 3. blend and contour: two groups of four pixels per thread, 16 groups (192 contiguous bytes) per row
  const float mb0 = (float)((mask_rgb >> 16) & 255u) * beta, mb1 = (float)((mask_rgb >> 8) & 255u) * beta, mb2 = (float)(mask_rgb & 255u) * beta;
  const unsigned e0 = (edge_rgb >> 16) & 255u, e1 = (edge_rgb >> 8) & 255u, e2 = edge_rgb & 255u;
  const int k = threadIdx.x & 15;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int ry = (threadIdx.x >> 4) + 16 * half, gy = y0 + ry;
    if (gy >= H) continue;
    const long b = off + (long)gy * W;  // element index of the row's first pixel
    const int s = (int)(b & 3);
    const int xf = x0 - s + 4 * k;      // the group's first pixel: b + xf is a multiple of 4
    if (xf + 3 < 0 || xf >= W) continue;
    const int pos = ON_LEFT - s + 4 * k;
    const unsigned fg = row_bits4(F[ry + edge][0], F[ry + edge][1], pos);
    const unsigned ct = edge > 0 ? fg & ~row_bits4(E[ry][0], E[ry][1], pos) : 0u;
    rgb_group4(image, out, b, xf, W, wide, [&](int j, int c, unsigned v) -> unsigned {
      const float mb = ((fg >> j) & 1u) ? (c == 0 ? mb0 : (c == 1 ? mb1 : mb2)) : 0.f;
      return ((ct >> j) & 1u) ? (c == 0 ? e0 : (c == 1 ? e1 : e2)) : native_blend(v, alpha, mb);
    });
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// grad_histogram
// ---------------------------------------------------------------------------------------------------------------------------------
#define GH_BUCKETS UDET_HISTOGRAM_BUCKETS
#define GH_SPLIT 128     // a segment is split over at most this many workgroups ...
#define GH_MIN_CHUNK 2048  // ... of at least this many elements each
__device__ __forceinline__ int gh_active(long len) {
  const long a = (len + GH_MIN_CHUNK - 1) / GH_MIN_CHUNK;
  return a < 1 ? 1 : (a > GH_SPLIT ? GH_SPLIT : (int)a);
}
// stage 1: workgroup (s, y) buckets its slice of segment s: limits in LDS, one binary search (upper_bound, compared in double) per
// element, counts privatised in LDS and flushed with integer atomics; min / max / sum / sum of squares of the slice go to
// part[s][y][4] (fixed order inside the workgroup: the sums do not depend on scheduling).
__global__ __launch_bounds__(256) void grad_hist_kernel(const float* __restrict__ g, const long long* __restrict__ seg_offsets,
                                                        const double* __restrict__ limits, unsigned* __restrict__ counts,
                                                        double* __restrict__ part) {
  __shared__ double lim[GH_BUCKETS];
  __shared__ unsigned cnt[GH_BUCKETS];
  __shared__ double sm[4];
  const int s = blockIdx.x, y = blockIdx.y;
  const long off = seg_offsets[s], len = seg_offsets[s + 1] - off;
  const int active = gh_active(len);
  if (y >= active) return;
  for (int i = threadIdx.x; i < GH_BUCKETS; i += 256) {
    lim[i] = limits[i];
    cnt[i] = 0u;
  }
  __syncthreads();
  const long b = len * y / active, e = len * (y + 1) / active;
  double mn = INFINITY, mx = -INFINITY, sum = 0.0, sq = 0.0;
  for (long i = b + threadIdx.x; i < e; i += 256) {
    const double x = (double)g[off + i];
    int lo = 0, hi = GH_BUCKETS;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lim[mid] > x) hi = mid; else lo = mid + 1;
    }
    atomicAdd(&cnt[lo < GH_BUCKETS ? lo : GH_BUCKETS - 1], 1u);  // +inf and NaN have no limit above them: last bucket
    mn = fmin(mn, x);
    mx = fmax(mx, x);
    sum += x;
    sq += x * x;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < GH_BUCKETS; i += 256)
    if (cnt[i]) atomicAdd(&counts[(long)s * GH_BUCKETS + i], cnt[i]);
  mn = block_reduce256(mn, sm, [](double p, double q) { return fmin(p, q); });
  mx = block_reduce256(mx, sm, [](double p, double q) { return fmax(p, q); });
  sum = block_reduce256(sum, sm, [](double p, double q) { return p + q; });
  sq = block_reduce256(sq, sm, [](double p, double q) { return p + q; });
  if (threadIdx.x == 0) {
    double* o = part + ((long)s * GH_SPLIT + y) * 4;
    o[0] = mn; o[1] = mx; o[2] = sum; o[3] = sq;
  }
}
// stage 2: stats[s] = {min, max, count, sum, sum of squares} from the segment's partials, in order
__global__ __launch_bounds__(256) void grad_hist_finish_kernel(const long long* __restrict__ seg_offsets, int nseg,
                                                               const double* __restrict__ part, double* __restrict__ stats) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nseg) return;
  const long len = seg_offsets[s + 1] - seg_offsets[s];
  const int active = gh_active(len);
  double mn = INFINITY, mx = -INFINITY, sum = 0.0, sq = 0.0;
  for (int y = 0; y < active; ++y) {
    const double* p = part + ((long)s * GH_SPLIT + y) * 4;
    mn = fmin(mn, p[0]);
    mx = fmax(mx, p[1]);
    sum += p[2];
    sq += p[3];
  }
  double* o = stats + (long)s * 5;
  o[0] = mn; o[1] = mx; o[2] = (double)len; o[3] = sum; o[4] = sq;
}

// TensorFlow's default histogram bucket limits (tensorflow/core/lib/histogram/histogram.cc, InitDefaultBucketsInner), built once
static const double* histogram_limits() {
  static const struct Table {
    double v[GH_BUCKETS];
    Table() {
      double pos[GH_BUCKETS / 2];
      int n = 0;
      for (double x = 1e-12; x < 1e20; x *= 1.1) pos[n++] = x;  // 774 values
      pos[n++] = DBL_MAX;
      for (int i = 0; i < n; ++i) {
        v[i] = -pos[n - 1 - i];
        v[n + 1 + i] = pos[i];
      }
      v[n] = 0.0;
    }
  } t;
  return t.v;
}
static const size_t kLimitBytes = (GH_BUCKETS * sizeof(double) + 255) / 256 * 256;

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_flow_to_image_workspace_bytes(int n) { return n < 1 ? 0 : (size_t)n * FI_SPLIT * sizeof(float); }
int udet_flow_to_image(const float* flow, const float* mask, const double* stats8, float threshold, int n, int h, int w,
                       unsigned char* rgb, void* workspace, size_t workspace_bytes, void* stream) {
  if (!flow || !rgb || n < 1 || n > 65535 || h < 1 || w < 1 || (mask != nullptr) != (stats8 != nullptr)) {
    set_error("flow_to_image: bad argument (mask and stats8 go together)");
    return UDET_ERR_ARG;
  }
  if (bad_workspace("flow_to_image", workspace, workspace_bytes, udet_flow_to_image_workspace_bytes(n), 4)) return UDET_ERR_ARG;
  const long HW = (long)h * w;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(flow_maxrad_kernel, dim3(FI_SPLIT, n), dim3(256), 0, (hipStream_t)stream, flow, HW, part);
  hipLaunchKernelGGL(flow_colour_kernel, dim3((unsigned)((HW + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, flow, mask, stats8,
                     threshold, h, w, part, rgb);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

int udet_overlay_mask(const float* image, const float* mask, const double* stats8, float threshold, int n, int h, int w,
                      unsigned char* out, int oh, int ow, void* stream) {
  if (!image || !mask || !out || n < 1 || n > 65535 || h < 1 || w < 1 || oh < 1 || ow < 1) {
    set_error("overlay_mask: bad argument");
    return UDET_ERR_ARG;
  }
  const long q = (long)oh * ow;
  hipLaunchKernelGGL(overlay_mask_kernel, dim3((unsigned)((q + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, image, mask, stats8,
                     threshold, h, w, out, oh, ow, (double)h / oh, (double)w / ow);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

int udet_overlay_native_ragged(const unsigned char* image_rgb, const unsigned char* mask, int n, const long long* offsets,
                               const int* hw, int max_h, int max_w, size_t total_pixels, float alpha, float beta,
                               unsigned mask_rgb, int edge, unsigned edge_rgb, unsigned char* out_rgb, void* stream) {
  if (bad_batch("overlay_native_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!image_rgb || !mask || !offsets || !hw || !out_rgb) {
    set_error("overlay_native_ragged: bad argument (non-null image_rgb, mask, offsets, hw and out_rgb)");
    return UDET_ERR_ARG;
  }
  if (edge < 0 || !(alpha >= 0.f) || !(beta >= 0.f) || isinf(alpha) || isinf(beta)) {
    set_error("overlay_native_ragged: edge %d >= 0 and finite alpha %g >= 0 and beta %g >= 0 are required", edge, alpha, beta);
    return UDET_ERR_ARG;
  }
  if (edge > UDET_OVERLAY_MAX_EDGE) {
    set_error("overlay_native_ragged: edge %d above UDET_OVERLAY_MAX_EDGE = %d", edge, UDET_OVERLAY_MAX_EDGE);
    return UDET_ERR_UNSUPPORTED;
  }
  // a row's groups of four pixels start up to three columns before the tile's first: ceil((max_w + 3) / ON_TW) tile columns
  const long tiles_x = ((long)max_w + 3 + ON_TW - 1) / ON_TW, tiles_y = ((long)max_h + ON_TH - 1) / ON_TH;
  if (tiles_x * tiles_y > (1L << 23)) {
    set_error("overlay_native_ragged: more than 2^23 tiles per sample");
    return UDET_ERR_SHAPE;
  }
  const int wide = ((reinterpret_cast<uintptr_t>(image_rgb) | reinterpret_cast<uintptr_t>(out_rgb)) & 3) == 0;
  hipLaunchKernelGGL(overlay_native_kernel, dim3((unsigned)(tiles_x * tiles_y), n), dim3(256), 0, (hipStream_t)stream, image_rgb, mask,
                     offsets, hw, (int)tiles_x, alpha, beta, mask_rgb, edge, edge_rgb, out_rgb, wide);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

int udet_histogram_limits(double* limits, int n) {
  if (!limits || n != GH_BUCKETS) { set_error("histogram_limits: the table has %d entries", GH_BUCKETS); return UDET_ERR_ARG; }
  const double* t = histogram_limits();
  for (int i = 0; i < n; ++i) limits[i] = t[i];
  return UDET_OK;
}
size_t udet_grad_histogram_workspace_bytes(int nseg) {
  return nseg < 1 ? 0 : kLimitBytes + (size_t)nseg * GH_SPLIT * 4 * sizeof(double);
}
int udet_grad_histogram(const float* g, const long long* seg_offsets, int nseg, double* stats, unsigned* counts, void* workspace,
                        size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!g || !seg_offsets || !stats || !counts || nseg < 1 || nseg > 65535) { set_error("grad_histogram: bad argument"); return UDET_ERR_ARG; }
  if (bad_workspace("grad_histogram", workspace, workspace_bytes, udet_grad_histogram_workspace_bytes(nseg), 8)) return UDET_ERR_ARG;
  double* limits = (double*)workspace;
  double* part = (double*)((char*)workspace + kLimitBytes);
  UDET_HIP(hipMemcpyAsync(limits, histogram_limits(), GH_BUCKETS * sizeof(double), hipMemcpyHostToDevice, s));
  UDET_HIP(hipMemsetAsync(counts, 0, (size_t)nseg * GH_BUCKETS * sizeof(unsigned), s));
  hipLaunchKernelGGL(grad_hist_kernel, dim3(nseg, GH_SPLIT), dim3(256), 0, s, g, seg_offsets, limits, counts, part);
  hipLaunchKernelGGL(grad_hist_finish_kernel, dim3((nseg + 255) / 256), dim3(256), 0, s, seg_offsets, nseg, part, stats);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
