// Native-resolution mask restore: n soft masks [n,mh,mw] float32 -> n uint8 frames of DIFFERENT sizes, packed.
//   post_processing/crf_refine.py:84-97 (run_crf_original_resolution) and post_processing/post_processing.py:32-46:
//   soft = imresize(soft, (int(0.9 H), int(0.9 W))); soft / (amax(soft) + 1e-8); pasted into zeros((H, W)).
// scipy.misc.imresize = bytescale over the whole mask + Pillow's 8-bit BILINEAR resampler (horizontal pass, uint8 intermediate,
// vertical pass), the arithmetic of post_bytescale_kernel / post_resample_u8_kernel (postproc.hip) -- here batched, ragged and on
// many workgroups per sample, in at most three launches however many samples there are:
//   1. restore_minmax_kernel     per sample min / max of the mask: NB1 partial pairs per sample in the workspace; zeroes amax
//   2. restore_resample_kernel   one 64 x 16 tile of the sample's H x W frame per workgroup: bytescale on the fly, horizontal
//                                pass into an LDS strip (uint8, like Pillow's intermediate image), vertical pass out of it, the
//                                patch placed at (y0, x0), zeros around it; integer atomicMax of the patch's bytes into amax
//   3. restore_binary_kernel     (only with a binary output) byte / (amax + 1e-8) > threshold in float64 through a 256-entry table
// Integer work, bit-exact by construction; the only floating point is the bytescale (double, -ffp-contract=off in the Makefile).
// Every index comes from the per-sample tables, which the caller validates on the host (native_results.check_restore_tables).
#include <math.h>

#include "common.h"
#include "elementwise.h"

namespace udet {

#define RESTORE_NB1 32      // partial min / max pairs per sample
#define RESTORE_TW 64       // tile: 64 columns (one lane per column: rows are read and written in lane order)
#define RESTORE_TR 16       //       x 16 rows, four per thread
#define RESTORE_STRIP 64    // rows of the horizontal intermediate held in LDS at a time
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

// scipy.misc.bytescale of one value: the doubles of post_bytescale_kernel
__device__ __forceinline__ int restore_byte(float v, double mn, double scale) {
  double b = ((double)v - mn) * scale + 0.0;
  b = fmin(fmax(b, 0.0), 255.0) + 0.5;
  return (int)(unsigned char)b;
}

__global__ __launch_bounds__(256) void restore_resample_kernel(const float* __restrict__ masks, int mh, int mw,
                                                               const float* __restrict__ part, const long long* __restrict__ offsets,
                                                               const int* __restrict__ tab, const int* __restrict__ coef,
                                                               unsigned char* __restrict__ out, int* __restrict__ amax) {
  __shared__ unsigned char strip[RESTORE_STRIP * RESTORE_TW];
  __shared__ int smax[4];
  const int i = blockIdx.y, t = threadIdx.x;
  const int* __restrict__ d = tab + i * RESTORE_TAB;
  const int y0 = d[0], x0 = d[1], h = d[2], w = d[3], H = d[4], W = d[5];
  const int tiles_x = (W + RESTORE_TW - 1) / RESTORE_TW, tiles_y = (H + RESTORE_TR - 1) / RESTORE_TR;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // block-uniform: the grid is sized for the largest frame of the batch
  const int* __restrict__ hk = d[6] >= 0 ? coef + d[6] : nullptr;
  const int* __restrict__ hb = d[6] >= 0 ? coef + d[7] : nullptr;
  const int hks = d[8];
  const int* __restrict__ vk = d[9] >= 0 ? coef + d[9] : nullptr;
  const int* __restrict__ vb = d[9] >= 0 ? coef + d[10] : nullptr;
  const int vks = d[11];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int col = t & (RESTORE_TW - 1), X = tx * RESTORE_TW + col, x = X - x0;
  const bool in_x = X < W && x >= 0 && x < w;
  // patch rows of this tile
  const int Ya = ty * RESTORE_TR, Yb = min(Ya + RESTORE_TR, H);
  const int ya = max(Ya - y0, 0), yb = min(Yb - y0, h);  // [ya, yb)
  const bool tile_live = ya < yb && tx * RESTORE_TW < x0 + w && tx * RESTORE_TW + RESTORE_TW > x0;

  int ss[4], vlo[4], vn[4];
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int Y = Ya + (t >> 6) + 4 * j, y = Y - y0;
    live[j] = in_x && Y < H && y >= 0 && y < h;
    ss[j] = 1 << 21;
    vlo[j] = 0;
    vn[j] = 0;
    if (live[j]) {
      if (vb) { vlo[j] = vb[2 * y]; vn[j] = vb[2 * y + 1]; }
      else { vlo[j] = y; vn[j] = 1; }
    }
  }
  if (tile_live) {
    // bytescale constants of the sample: the partial pairs of launch 1
    float fmn = INFINITY, fmx = -INFINITY;
    for (int b = 0; b < RESTORE_NB1; ++b) {
      fmn = fminf(fmn, part[((size_t)i * RESTORE_NB1 + b) * 2]);
      fmx = fmaxf(fmx, part[((size_t)i * RESTORE_NB1 + b) * 2 + 1]);
    }
    const double mn = (double)fmn;
    double cscale = (double)fmx - mn;
    if (cscale == 0.0) cscale = 1.0;
    const double scale = 255.0 / cscale;
    const float* __restrict__ m = masks + (size_t)i * mh * mw;
    // mask rows the tile's patch rows read
    const int r0 = vb ? vb[2 * ya] : ya;
    const int r1 = vb ? vb[2 * (yb - 1)] + vb[2 * (yb - 1) + 1] : yb;
    int hlo = 0, hn = 0;
    if (in_x) {
      if (hb) { hlo = hb[2 * x]; hn = hb[2 * x + 1]; }
      else { hlo = x; hn = 1; }
    }
    for (int c0 = r0; c0 < r1; c0 += RESTORE_STRIP) {
      const int c1 = min(c0 + RESTORE_STRIP, r1);
      // horizontal pass of mask rows [c0, c1) at the tile's columns -> strip (uint8, Pillow's intermediate image)
      for (int r = c0 + (t >> 6); r < c1; r += 4) {
        int v = 0;
        if (in_x) {
          const float* __restrict__ row = m + (size_t)r * mw;
          if (hk) {
            int acc = 1 << 21;
            for (int k = 0; k < hn; ++k) acc += restore_byte(row[hlo + k], mn, scale) * hk[x * hks + k];
            acc >>= 22;
            v = acc < 0 ? 0 : (acc > 255 ? 255 : acc);
          } else {
            v = restore_byte(row[hlo], mn, scale);
          }
        }
        strip[(r - c0) * RESTORE_TW + col] = (unsigned char)v;
      }
      __syncthreads();
      // vertical taps that fall into this strip
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!live[j]) continue;
        const int ka = max(c0 - vlo[j], 0), kb = min(c1 - vlo[j], vn[j]);
        if (vk) {
          const int y = Ya + (t >> 6) + 4 * j - y0;
          for (int k = ka; k < kb; ++k) ss[j] += (int)strip[(vlo[j] + k - c0) * RESTORE_TW + col] * vk[y * vks + k];
        } else if (ka < kb) {
          ss[j] = (int)strip[(vlo[j] - c0) * RESTORE_TW + col];
        }
      }
      __syncthreads();
    }
  }
  int best = 0;
  unsigned char* __restrict__ o = out + offsets[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int Y = Ya + (t >> 6) + 4 * j;
    if (X >= W || Y >= H) continue;
    int v = 0;
    if (live[j]) {
      v = ss[j];
      if (vk) {
        v >>= 22;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
      }
    }
    o[(size_t)Y * W + X] = (unsigned char)v;
    best = max(best, v);
  }
  if (!tile_live) return;  // block-uniform
  for (int s = 32; s > 0; s >>= 1) best = max(best, __shfl_xor(best, s));
  if ((t & 63) == 0) smax[t >> 6] = best;
  __syncthreads();
  if (t == 0) {
    best = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    if (best > 0) atomicMax(&amax[i], best);
  }
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
  const long tiles = (long)((max_w + RESTORE_TW - 1) / RESTORE_TW) * ((max_h + RESTORE_TR - 1) / RESTORE_TR);
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
