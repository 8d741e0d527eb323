// scipy.misc.imresize as the project restates it, once: bytescale + the two passes of Pillow's 8-bit BILINEAR resampler (Resample.c
// ImagingResampleHorizontal_8bpc / Vertical_8bpc, horizontal first, uint8 intermediate image).
//   pil_byte, pil_clip8 / pil_taps   the per-pixel arithmetic, shared with the per-frame kernels of postproc.hip
//   PilPass, pil_scale, pil_tile, pil_block_max   the tiled form: one 64 x 16 tile of a patch per workgroup of 256 threads
//                                    (restore_resample_kernel in restore.hip, soft_resample_kernel in soft_score.hip)
// Integer work, bit-exact by construction; the only floating point is the bytescale, in double: every translation unit that includes
// this file is compiled with -ffp-contract=off (Makefile).  Every index comes from the coefficient blocks and the geometry the caller
// validates on the host (pil_tables.check_pass): there is no bounds check here.
#pragma once
#include <math.h>

#include "common.h"

namespace udet {

#define PIL_TW 64       // tile: 64 columns (one lane per column: rows are read and written in lane order)
#define PIL_TR 16       //       x 16 rows, four per thread: thread t has rows (t >> 6) + 4 j of the tile, j < 4
#define PIL_STRIP 64    // rows of the horizontal intermediate held in LDS at a time
#define PIL_HALF (1 << 21)  // a pass's sum starts at one half of its 22-bit fixed point

// scipy.misc.bytescale of one value: uint8((v - min) * (255 / (max - min)) clipped + 0.5)
__device__ __forceinline__ int pil_byte(double v, double mn, double scale) {
  double b = (v - mn) * scale + 0.0;
  b = fmin(fmax(b, 0.0), 255.0) + 0.5;
  return (int)(unsigned char)b;
}

__device__ __forceinline__ int pil_clip8(int ss) {
  ss >>= 22;
  return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// one output of a pass: ss = 1 << 21; ss += pixel(k) * kk[k], k < n; clip8(ss >> 22)
template <typename Pixel>
__device__ __forceinline__ int pil_taps(const int* __restrict__ kk, int n, Pixel pixel) {
  int ss = PIL_HALF;
  for (int k = 0; k < n; ++k) ss += pixel(k) * kk[k];
  return pil_clip8(ss);
}

// One pass's coefficient block inside coef: kk [out][ks], bounds [out][2] = (first tap, taps).  kk == nullptr: the pass is skipped (its
// output is as long as its input).  (k, b, ks) are the three table integers of the pass, k < 0 for a skipped one.
struct PilPass {
  const int* kk;
  const int* bounds;
  int ks;
};
__device__ __forceinline__ PilPass pil_pass(const int* __restrict__ coef, int k, int b, int ks) {
  return PilPass{k >= 0 ? coef + k : nullptr, k >= 0 ? coef + b : nullptr, ks};
}

// bytescale constants of one mask from its nb partial (min, max) pairs
__device__ __forceinline__ void pil_scale(const float* __restrict__ part, int nb, double& mn, double& scale) {
  float fmn = INFINITY, fmx = -INFINITY;
  for (int b = 0; b < nb; ++b) {
    fmn = fminf(fmn, part[2 * b]);
    fmx = fmaxf(fmx, part[2 * b + 1]);
  }
  mn = (double)fmn;
  double cscale = (double)fmx - mn;
  if (cscale == 0.0) cscale = 1.0;
  scale = 255.0 / cscale;
}

struct PilBytes {
  int v[4];
};

// The thread's four bytes of one tile of a patch: src (row stride ld) bytescaled with (mn, scale) on the fly, the horizontal pass h into
// an LDS strip, the vertical pass v out of it.  The thread stands at patch column x (in_x: inside the patch) and patch rows y + 4 j,
// row j inside the patch and wanted where live[j] (live[j] implies in_x); a row that is not live gives 0.  [ya, yb), ya < yb, are
// the patch rows of the whole tile.  Holds two __syncthreads() per strip: to be entered by every thread of the workgroup or by none.
__device__ __forceinline__ PilBytes pil_tile(const float* __restrict__ src, int ld, const PilPass h, const PilPass v, double mn, double scale,
                                             int x, bool in_x, int y, const bool (&live)[4], int ya, int yb) {
  __shared__ unsigned char strip[PIL_STRIP * PIL_TW];
  const int t = threadIdx.x, col = t & (PIL_TW - 1);
  const int* __restrict__ hk = h.kk;
  const int* __restrict__ vk = v.kk;
  const int* __restrict__ vb = v.bounds;
  int ss[4], vlo[4], vn[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ss[j] = PIL_HALF;
    vlo[j] = 0;
    vn[j] = 0;
    if (live[j]) {
      if (vb) { vlo[j] = vb[2 * (y + 4 * j)]; vn[j] = vb[2 * (y + 4 * j) + 1]; }
      else { vlo[j] = y + 4 * j; vn[j] = 1; }
    }
  }
  // source rows the tile's patch rows read
  const int r0 = vb ? vb[2 * ya] : ya;
  const int r1 = vb ? vb[2 * (yb - 1)] + vb[2 * (yb - 1) + 1] : yb;
  int hlo = 0, hn = 0;
  if (in_x) {
    if (hk) { hlo = h.bounds[2 * x]; hn = h.bounds[2 * x + 1]; }
    else { hlo = x; hn = 1; }
  }
  for (int c0 = r0; c0 < r1; c0 += PIL_STRIP) {
    const int c1 = min(c0 + PIL_STRIP, r1);
    // horizontal pass of source rows [c0, c1) at the tile's columns -> strip (uint8, Pillow's intermediate image)
    for (int r = c0 + (t >> 6); r < c1; r += 4) {
      int b = 0;
      if (in_x) {
        const float* __restrict__ row = src + (size_t)r * ld + hlo;
        b = hk ? pil_taps(hk + x * h.ks, hn, [&](int k) { return pil_byte(row[k], mn, scale); }) : pil_byte(row[0], mn, scale);
      }
      strip[(r - c0) * PIL_TW + col] = (unsigned char)b;
    }
    __syncthreads();
    // vertical taps that fall into this strip
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!live[j]) continue;
      const int ka = max(c0 - vlo[j], 0), kb = min(c1 - vlo[j], vn[j]);
      if (vk) {
        for (int k = ka; k < kb; ++k) ss[j] += (int)strip[(vlo[j] + k - c0) * PIL_TW + col] * vk[(y + 4 * j) * v.ks + k];
      } else if (ka < kb) {
        ss[j] = (int)strip[(vlo[j] - c0) * PIL_TW + col];
      }
    }
    __syncthreads();
  }
  PilBytes out;
#pragma unroll
  for (int j = 0; j < 4; ++j) out.v[j] = !live[j] ? 0 : (vk ? pil_clip8(ss[j]) : ss[j]);
  return out;
}

// the largest of the workgroup's (256 threads) values `best` >= 0 into *dst by an integer atomicMax (exact in any order); to be entered
// by every thread of the workgroup or by none
__device__ __forceinline__ void pil_block_max(int best, int* __restrict__ dst) {
  __shared__ int smax[4];
  const int t = threadIdx.x;
  for (int s = 32; s > 0; s >>= 1) best = max(best, __shfl_xor(best, s, 64));
  if ((t & 63) == 0) smax[t >> 6] = best;
  __syncthreads();
  if (t == 0) {
    best = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    if (best > 0) atomicMax(dst, best);
  }
}

}  // namespace udet
