// Native-resolution mask restore: n soft masks [n,mh,mw] float32 -> n uint8 frames of DIFFERENT sizes, packed.
//   post_processing/crf_refine.py:84-97 (run_crf_original_resolution) and post_processing/post_processing.py:32-46:
//   soft = imresize(soft, (int(0.9 H), int(0.9 W))); soft / (amax(soft) + 1e-8); pasted into zeros((H, W)).
// scipy.misc.imresize = bytescale over the whole mask + Pillow's 8-bit BILINEAR resampler (horizontal pass, uint8 intermediate,
// vertical pass), the arithmetic and the tile routine of pil_resample.h -- here batched, ragged and on many workgroups per sample, in
// at most three launches however many samples there are:
//   1. restore_minmax_kernel     per sample min / max of the mask: NB1 partial pairs per sample in the workspace; zeroes amax
//   2. restore_resample_kernel   one 64 x 16 tile of the sample's H x W frame per workgroup: pil_tile on the tile's part of the
//                                patch, the patch placed at (y0, x0), zeros around it; integer atomicMax of the patch's bytes into amax
//   3. restore_binary_kernel     (only with a binary output) byte / (amax + 1e-8) > threshold in float64 through a 256-entry table
// Every index comes from the per-sample tables, which the caller validates on the host (native_results.check_restore_tables).
#include <math.h>

#include "common.h"
#include "elementwise.h"
#include "pil_resample.h"

namespace udet {

#define RESTORE_NB1 32      // partial min / max pairs per sample
#define RESTORE_TAB 12      // int32 per sample: y0 x0 h w H W | hk hb hks | vk vb vks   (hk / vk < 0: that pass is skipped)

__global__ __launch_bounds__(256) void restore_minmax_kernel(const float* __restrict__ masks, int mhw, float* __restrict__ part,
                                                             int* __restrict__ amax) {
  __shared__ float smn[256], smx[256];
  const int i = blockIdx.y, t = threadIdx.x;
  const float* __restrict__ p = masks + (size_t)i * mhw;
  float mn = INFINITY, mx = -INFINITY;
  for (int k = blockIdx.x * 256 + t; k < mhw; k += RESTORE_NB1 * 256) {
    const float v = p[k];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  smn[t] = mn;
  smx[t] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      smn[t] = fminf(smn[t], smn[t + s]);
      smx[t] = fmaxf(smx[t], smx[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) {
    part[((size_t)i * RESTORE_NB1 + blockIdx.x) * 2] = smn[0];
    part[((size_t)i * RESTORE_NB1 + blockIdx.x) * 2 + 1] = smx[0];
    if (blockIdx.x == 0) amax[i] = 0;
  }
}

__global__ __launch_bounds__(256) void restore_resample_kernel(const float* __restrict__ masks, int mh, int mw,
                                                               const float* __restrict__ part, const long long* __restrict__ offsets,
                                                               const int* __restrict__ tab, const int* __restrict__ coef,
                                                               unsigned char* __restrict__ out, int* __restrict__ amax) {
  const int i = blockIdx.y, t = threadIdx.x;
  const int* __restrict__ d = tab + i * RESTORE_TAB;
  const int y0 = d[0], x0 = d[1], h = d[2], w = d[3], H = d[4], W = d[5];
  const int tiles_x = (W + PIL_TW - 1) / PIL_TW, tiles_y = (H + PIL_TR - 1) / PIL_TR;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // block-uniform: the grid is sized for the largest frame of the batch
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  // frame coordinates (X, Y), patch coordinates (x, y): negative above and left of the box
  const int X = tx * PIL_TW + (t & (PIL_TW - 1)), x = X - x0;
  const bool in_x = X < W && x >= 0 && x < w;
  const int Ya = ty * PIL_TR, Yb = min(Ya + PIL_TR, H), Y = Ya + (t >> 6), y = Y - y0;
  const int ya = max(Ya - y0, 0), yb = min(Yb - y0, h);  // patch rows [ya, yb) of this tile
  const bool tile_live = ya < yb && tx * PIL_TW < x0 + w && tx * PIL_TW + PIL_TW > x0;  // block-uniform
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) live[j] = in_x && Y + 4 * j < H && y + 4 * j >= 0 && y + 4 * j < h;
  PilBytes b = {{0, 0, 0, 0}};  // a tile outside the box: zeros
  if (tile_live) {
    double mn, scale;
    pil_scale(part + (size_t)i * RESTORE_NB1 * 2, RESTORE_NB1, mn, scale);
    b = pil_tile(masks + (size_t)i * mh * mw, mw, pil_pass(coef, d[6], d[7], d[8]), pil_pass(coef, d[9], d[10], d[11]), mn, scale, x, in_x,
                 y, live, ya, yb);
  }
  int best = 0;
  unsigned char* __restrict__ o = out + offsets[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (X >= W || Y + 4 * j >= H) continue;
    o[(size_t)(Y + 4 * j) * W + X] = (unsigned char)b.v[j];  // 0 where the row is not live: the strip around the box
    best = max(best, b.v[j]);
  }
  if (tile_live) pil_block_max(best, &amax[i]);
}

__global__ __launch_bounds__(256) void restore_binary_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                             const int* __restrict__ tab, const int* __restrict__ amax, double threshold,
                                                             unsigned char* __restrict__ binary) {
  __shared__ unsigned char lut[256];
  const int i = blockIdx.y, t = threadIdx.x;
  lut[t] = ((double)t / ((double)amax[i] + 1e-8) > threshold) ? 1 : 0;
  __syncthreads();
  const size_t total = (size_t)tab[i * RESTORE_TAB + 4] * tab[i * RESTORE_TAB + 5];
  const unsigned char* __restrict__ src = data + offsets[i];
  unsigned char* __restrict__ dst = binary + offsets[i];
  for (size_t k = (size_t)blockIdx.x * 256 + t; k < total; k += (size_t)gridDim.x * 256) dst[k] = lut[src[k]];
}

size_t restore_workspace_bytes(int n) { return (size_t)n * RESTORE_NB1 * 2 * sizeof(float); }

int launch_restore_masks_ragged(const float* masks, int n, int mh, int mw, const long long* offsets, const int* tab, const int* coef,
                                int max_h, int max_w, unsigned char* out, int* amax, unsigned char* binary, double threshold,
                                void* workspace, hipStream_t s) {
  float* part = (float*)workspace;
  const long tiles = (long)((max_w + PIL_TW - 1) / PIL_TW) * ((max_h + PIL_TR - 1) / PIL_TR);
  if (tiles > 0x7fffffffL) { set_error("restore_masks_ragged: frame too large"); return UDET_ERR_SHAPE; }
  hipLaunchKernelGGL(restore_minmax_kernel, dim3(RESTORE_NB1, n), dim3(256), 0, s, masks, mh * mw, part, amax);
  hipLaunchKernelGGL(restore_resample_kernel, dim3((unsigned)tiles, n), dim3(256), 0, s, masks, mh, mw, part, offsets, tab, coef, out, amax);
  if (binary) {
    const long nb = ((long)max_h * max_w + 256 * 16 - 1) / (256 * 16);
    hipLaunchKernelGGL(restore_binary_kernel, dim3((unsigned)(nb < 1 ? 1 : nb), n), dim3(256), 0, s, out, offsets, tab, amax, threshold, binary);
  }
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
