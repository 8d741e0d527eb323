// The soft scores of the ensemble for a batch of frames: generate_soft_score_from_buffer.py buffer_to_soft_score :38-93 --
// sanity rule, rectify_pred_mask on every (shift, crop), the sum over the ensemble, min-max -- for n frames in four launches, what
// post_processing.soft_score does with about a hundred launches and a host round trip per frame, bit for bit:
//   1. soft_stats_kernel      per mask: the border mean (post_border_mean_kernel's loop and tree: the same double) by workgroup 0, the
//                             min / max of the mask's source window as SOFT_NB1 partial pairs by the others; zeroes the patch maximum
//   2. soft_resample_kernel   one 64 x 16 tile of a mask's patch per workgroup: pil_tile (pil_resample.h, the routine restore.hip runs)
//                             on the mask's source window; the bytes go to the workspace at their place on the canvas, their maximum by an
//                             integer atomicMax.  Every raw mask is resampled, whatever the sanity rule says: launch 3 chooses among the patches
//   3. soft_fuse_kernel       one thread per pixel: the sanity rule per (frame, shift, crop), term = vb / (maxb + 1e-6) + vf / (maxf + 1e-6)
//                             (identity row: s_b + s_f), score += term shift-major, crop-minor; the score into pred_mask, a (min, max)
//                             pair per workgroup into the workspace
//   4. soft_norm_kernel       the frame's pairs reduced by every workgroup, (score - min) / (max - min + 1e-6) in place
// No workgroup waits for another inside a launch; min, max and the integer atomicMax are exact in any order, every floating-point sum has
// a fixed order.  Every index comes from the geometry rows, which the caller validates on the host
// (post_processing.check_soft_score_tables).  Compiled with -ffp-contract=off (Makefile).
#include <math.h>

#include "common.h"
#include "host_checks.h"
#include "pil_resample.h"

namespace udet {

#define SOFT_NB1 8       // partial min / max pairs per mask
#define SOFT_GEOM UDET_SOFT_SCORE_GEOM
// a geometry row: mode (0 identity, 1 rectify) | source window sy0 sx0 sh sw | patch hh ww at y0 x0 | hk hb hks | vk vb vks | 0
enum { G_MODE, G_SY0, G_SX0, G_SH, G_SW, G_HH, G_WW, G_Y0, G_X0, G_HK, G_HB, G_HKS, G_VK, G_VB, G_VKS };
static_assert(G_VKS < SOFT_GEOM, "geometry row");

struct SoftArgs {
  const float* masks;  // [n][2][R][h][w], R = ns * nc rows (shift-major, crop-minor)
  const int* geom;     // [R][SOFT_GEOM]
  const int* coef;
  double* mean;        // [M] border means, M = n * 2 * R
  double* fpart;       // [n][nblk][2] (min, max) of the score per workgroup of launch 3
  float* wpart;        // [M][SOFT_NB1][2] (min, max) of the source window
  int* pmax;           // [M] the largest byte of the patch
  unsigned char* patch;  // [M][h][w]: the patch's bytes at their place on the canvas; the rest is never read
  double* pred;        // [n][h][w]
  double san_t;
  int n, R, h, w, nblk;
};

// launch 1: grid (1 + SOFT_NB1, M), 1024 threads
__global__ __launch_bounds__(1024) void soft_stats_kernel(SoftArgs a) {
  __shared__ double sm[1024];
  const int m = blockIdx.y, t = threadIdx.x, H = a.h, W = a.w;
  const unsigned hw = (unsigned)H * W;  // below 2^31: i + stride cannot wrap
  const float* __restrict__ p = a.masks + (size_t)m * hw;
  if (blockIdx.x == 0) {  // block-uniform
    // post_border_mean_kernel: thread t sums pixels t, t + 1024, ... in that order, then the halving tree over 1024 slots
    double acc = 0.0;
    for (unsigned i = t; i < hw; i += 1024) {
      const int y = i / W, x = i - y * W;
      const int cnt = (y < 2) + (y >= H - 2) + (x < 2) + (x >= W - 2);
      acc += (double)cnt * (double)p[i];
    }
    sm[t] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
      if (t < s) sm[t] = sm[t] + sm[t + s];
      __syncthreads();
    }
    if (t == 0) {
      a.mean[m] = sm[0] / (1.0 * (4.0 * W + 4.0 * H));
      a.pmax[m] = 0;
    }
    return;
  }
  const int* __restrict__ g = a.geom + (m % a.R) * SOFT_GEOM;
  float mn = INFINITY, mx = -INFINITY;
  if (g[G_MODE]) {
    const int sy0 = g[G_SY0], sx0 = g[G_SX0], sw = g[G_SW];
    const unsigned cnt = (unsigned)g[G_SH] * sw;
    for (unsigned k = (blockIdx.x - 1) * 1024 + t; k < cnt; k += SOFT_NB1 * 1024) {
      const unsigned r = k / sw, c = k - r * sw;
      const float v = p[(size_t)(sy0 + r) * W + sx0 + c];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  float* smf = reinterpret_cast<float*>(sm);
  if ((t & 63) == 0) {
    smf[t >> 6] = mn;
    smf[16 + (t >> 6)] = mx;
  }
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < 16; ++k) {
      mn = fminf(mn, smf[k]);
      mx = fmaxf(mx, smf[16 + k]);
    }
    float* o = a.wpart + ((size_t)m * SOFT_NB1 + (blockIdx.x - 1)) * 2;
    o[0] = mn;
    o[1] = mx;
  }
}

// launch 2: grid (tiles of the largest patch, M), 256 threads
__global__ __launch_bounds__(256) void soft_resample_kernel(SoftArgs a) {
  const int m = blockIdx.y, t = threadIdx.x, W = a.w;
  const int* __restrict__ g = a.geom + (m % a.R) * SOFT_GEOM;
  if (!g[G_MODE]) return;  // block-uniform: the identity row takes the raw masks
  const int hh = g[G_HH], ww = g[G_WW];
  const int tiles_x = (ww + PIL_TW - 1) / PIL_TW, tiles_y = (hh + PIL_TR - 1) / PIL_TR;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // block-uniform: the grid is sized for a patch that fills the canvas
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * PIL_TW + (t & (PIL_TW - 1)), y = ty * PIL_TR + (t >> 6);  // patch coordinates
  const bool in_x = x < ww;
  const int ya = ty * PIL_TR, yb = min(ya + PIL_TR, hh);  // patch rows [ya, yb) of this tile, ya < yb
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) live[j] = in_x && y + 4 * j < hh;
  double mn, scale;  // of the window: the partial pairs of launch 1
  pil_scale(a.wpart + (size_t)m * SOFT_NB1 * 2, SOFT_NB1, mn, scale);
  const float* __restrict__ win = a.masks + (size_t)m * a.h * W + (size_t)g[G_SY0] * W + g[G_SX0];
  const PilBytes b = pil_tile(win, W, pil_pass(a.coef, g[G_HK], g[G_HB], g[G_HKS]), pil_pass(a.coef, g[G_VK], g[G_VB], g[G_VKS]), mn, scale,
                              x, in_x, y, live, ya, yb);
  int best = 0;
  unsigned char* __restrict__ o = a.patch + (size_t)m * a.h * W + (size_t)g[G_Y0] * W + g[G_X0];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!live[j]) continue;  // x < ww and y < hh: inside the canvas by the validated row
    o[(size_t)(y + 4 * j) * W + x] = (unsigned char)b.v[j];
    best = max(best, b.v[j]);
  }
  pil_block_max(best, &a.pmax[m]);
}

// (min, max) over a workgroup of 256 threads; exact in any order
__device__ __forceinline__ void block_minmax_256(double& mn, double& mx, double* sm) {
  for (int o = 32; o > 0; o >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, o, 64));
    mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    sm[threadIdx.x >> 6] = mn;
    sm[4 + (threadIdx.x >> 6)] = mx;
  }
  __syncthreads();
  mn = fmin(fmin(sm[0], sm[1]), fmin(sm[2], sm[3]));
  mx = fmax(fmax(sm[4], sm[5]), fmax(sm[6], sm[7]));
}

// launch 3: grid (nblk, n), 256 threads, one pixel per thread
__global__ __launch_bounds__(256) void soft_fuse_kernel(SoftArgs a) {
  __shared__ double sm[8];
  const int f = blockIdx.y, R = a.R, W = a.w;
  const unsigned hw = (unsigned)a.h * W, i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < hw;
  const int y = i / W, x = i - y * W;
  double score = 0.0;
  for (int r = 0; r < R; ++r) {
    const int* __restrict__ g = a.geom + r * SOFT_GEOM;
    const size_t mb = (size_t)(2 * f) * R + r, mf = (size_t)(2 * f + 1) * R + r;  // the backward (-shift) and the forward run
    const bool bad_b = a.mean[mb] >= a.san_t, bad_f = a.mean[mf] >= a.san_t;
    const bool zero = bad_b && bad_f;          // both slots are zeros
    const size_t sb = bad_b ? mf : mb, sf = bad_f ? mb : mf;  // a bad run's slot takes its partner
    double term;
    if (!g[G_MODE]) {
      const double vb = (in && !zero) ? (double)a.masks[sb * hw + i] : 0.0;
      const double vf = (in && !zero) ? (double)a.masks[sf * hw + i] : 0.0;
      term = vb + vf;
    } else {
      const int py = y - g[G_Y0], px = x - g[G_X0];
      const bool use = in && !zero && py >= 0 && py < g[G_HH] && px >= 0 && px < g[G_WW];
      const double vb = use ? (double)a.patch[sb * hw + i] : 0.0;
      const double vf = use ? (double)a.patch[sf * hw + i] : 0.0;
      const double db = (zero ? 0.0 : (double)a.pmax[sb]) + 1e-6, df = (zero ? 0.0 : (double)a.pmax[sf]) + 1e-6;
      term = vb / db + vf / df;
    }
    score = r == 0 ? term : score + term;
  }
  if (in) a.pred[(size_t)f * hw + i] = score;
  double mn = in ? score : INFINITY, mx = in ? score : -INFINITY;
  block_minmax_256(mn, mx, sm);
  if (threadIdx.x == 0) {
    double* o = a.fpart + ((size_t)f * a.nblk + blockIdx.x) * 2;
    o[0] = mn;
    o[1] = mx;
  }
}

// launch 4: grid (nblk, n), 256 threads
__global__ __launch_bounds__(256) void soft_norm_kernel(SoftArgs a) {
  __shared__ double sm[8];
  const int f = blockIdx.y;
  const unsigned hw = (unsigned)a.h * a.w, i = blockIdx.x * 256 + threadIdx.x;
  const double* __restrict__ part = a.fpart + (size_t)f * a.nblk * 2;
  double mn = INFINITY, mx = -INFINITY;
  for (int k = threadIdx.x; k < a.nblk; k += 256) {
    mn = fmin(mn, part[2 * k]);
    mx = fmax(mx, part[2 * k + 1]);
  }
  block_minmax_256(mn, mx, sm);
  if (i < hw) {
    double* p = a.pred + (size_t)f * hw + i;
    *p = (*p - mn) / (mx - mn + 1e-6);
  }
}

// the workspace of n frames, section by section (every size a multiple of 8 bytes until the patches): mean | fpart | wpart | pmax | patch
static size_t soft_frame_bytes(int ns, int nc, int h, int w) {
  const size_t R = (size_t)ns * nc, hw = (size_t)h * w, nblk = (hw + 255) / 256;
  const size_t b = 2 * R * sizeof(double) + nblk * 2 * sizeof(double) + 2 * R * SOFT_NB1 * 2 * sizeof(float) + 2 * R * sizeof(int) + 2 * R * hw;
  return (b + 15) & ~(size_t)15;
}

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_post_soft_score_workspace_bytes(int n, int ns, int nc, int h, int w) {
  if (n < 1 || ns < 1 || nc < 1 || h < 1 || w < 1) return 0;
  return (size_t)n * soft_frame_bytes(ns, nc, h, w);
}

int udet_post_soft_score_batch(const float* masks, int n, int ns, int nc, int h, int w, const int* geom, const int* coef, double san_t,
                               double* pred_mask, void* workspace, size_t workspace_bytes, void* stream) {
  // (4 x 4 at least: the border strips of the sanity rule, as udet_post_border_mean; M masks are a grid dimension)
  if (n < 1 || ns < 1 || nc < 1 || h < 4 || w < 4 || (long)h * w > 0x7fffffffL || (long)n * 2 * ns * nc > 65535L) {
    set_error("post_soft_score_batch: bad argument (n = %d, ns = %d, nc = %d at least 1, frames of %d x %d at least 4 x 4 and below 2^31 pixels, "
              "n * 2 * ns * nc at most 65535)", n, ns, nc, h, w);
    return UDET_ERR_ARG;
  }
  if (!masks || !geom || !coef || !pred_mask || (reinterpret_cast<uintptr_t>(pred_mask) & 7)) {
    set_error("post_soft_score_batch: bad argument (non-null masks, geom, coef and pred_mask (8-byte aligned))");
    return UDET_ERR_ARG;
  }
  if (!isfinite(san_t)) {
    set_error("post_soft_score_batch: bad argument (san_t must be finite)");
    return UDET_ERR_ARG;
  }
  if (bad_workspace("post_soft_score_batch", workspace, workspace_bytes, udet_post_soft_score_workspace_bytes(n, ns, nc, h, w), 16))
    return UDET_ERR_ARG;
  const size_t R = (size_t)ns * nc, M = (size_t)n * 2 * R, hw = (size_t)h * w, nblk = (hw + 255) / 256;
  SoftArgs a;
  a.masks = masks; a.geom = geom; a.coef = coef;
  a.mean = (double*)workspace;
  a.fpart = a.mean + M;
  a.wpart = (float*)(a.fpart + (size_t)n * nblk * 2);
  a.pmax = (int*)(a.wpart + M * SOFT_NB1 * 2);
  a.patch = (unsigned char*)(a.pmax + M);
  a.pred = pred_mask;
  a.san_t = san_t;
  a.n = n; a.R = (int)R; a.h = h; a.w = w; a.nblk = (int)nblk;
  const size_t tiles = (size_t)((w + PIL_TW - 1) / PIL_TW) * ((h + PIL_TR - 1) / PIL_TR);
  hipStream_t s = (hipStream_t)stream;
  UDET_LAUNCH(soft_stats_kernel, dim3(1 + SOFT_NB1, (unsigned)M), dim3(1024), 0, s, a);
  UDET_LAUNCH(soft_resample_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(256), 0, s, a);
  UDET_LAUNCH(soft_fuse_kernel, dim3((unsigned)nblk, n), dim3(256), 0, s, a);
  UDET_LAUNCH(soft_norm_kernel, dim3((unsigned)nblk, n), dim3(256), 0, s, a);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
