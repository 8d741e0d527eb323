// The per-pixel arithmetic of the propagation stage (post_processing/generate_soft_score_from_buffer.py:166-185), shared by the per-frame
// kernels of postproc.hip and the sequence kernels of sequence.hip: both must give the same bits, so the expressions exist once.  Every
// translation unit that includes this file is compiled with -ffp-contract=off (Makefile).
#pragma once
#include <math.h>

#include "common.h"

namespace udet {

// cv2.remap(src, flow + grid, None, INTER_LINEAR), BORDER_CONSTANT 0 (OpenCV imgwarp.cpp remapBilinear) at pixel (x, y) of an H x W frame
// whose flow there is (u, v): the float32 map (float)((double)flow + (double)coordinate), coordinates rounded to 1/32 pixel (round half to
// even), float weights (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx summed in that order, taps outside the image read 0
struct RemapTaps {
  long ix, iy;
  float w00, w01, w10, w11;
};
__device__ __forceinline__ RemapTaps remap_taps(float u, float v, int x, int y) {
  const float mxf = (float)((double)u + (double)x), myf = (float)((double)v + (double)y);
  long sx = (long)rint((double)mxf * 32.0), sy = (long)rint((double)myf * 32.0);
  long ix = sx >> 5, iy = sy >> 5;
  const float fx = (float)(sx & 31) / 32.f, fy = (float)(sy & 31) / 32.f;
  RemapTaps t;
  t.ix = ix < -32768 ? -32768 : (ix > 32767 ? 32767 : ix);
  t.iy = iy < -32768 ? -32768 : (iy > 32767 ? 32767 : iy);
  t.w00 = (1.f - fy) * (1.f - fx);
  t.w01 = (1.f - fy) * fx;
  t.w10 = fy * (1.f - fx);
  t.w11 = fy * fx;
  return t;
}
__device__ __forceinline__ float remap_gather(const float* src, const RemapTaps& t, int H, int W) {
  auto tap = [&](long yy, long xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[yy * W + xx] : 0.f; };
  float o = tap(t.iy, t.ix) * t.w00;
  o = o + tap(t.iy, t.ix + 1) * t.w01;
  o = o + tap(t.iy + 1, t.ix) * t.w10;
  o = o + tap(t.iy + 1, t.ix + 1) * t.w11;
  return o;
}

// the denominators of propagate (:178-184): max + 1e-8 summed in double, then rounded to float32
__device__ __forceinline__ float max_denominator(float mx) { return (float)((double)mx + 1e-8); }
// (1 - w_r) * (s2 / max s2) + w_r * ra, unfused
__device__ __forceinline__ float blend_pair(float a, float v, float b, float y) { return a * v + b * y; }

}  // namespace udet
