// The colour bytes of the overlays at native size (visualize.hip: overlay_native_ragged, instances.hip: overlay_instances_ragged): the
// blend of one byte, and the group of four pixels of a row whose twelve colour bytes are three aligned 32-bit words.
#pragma once
#include "common.h"

namespace udet {

// cv2.addWeighted of one byte: v * alpha and the mask's term mb = m * beta are float32 products, their sum a float32 sum (no FMA: the
// files that include this are compiled with -ffp-contract=off), rounded half to even and saturated (both terms are >= 0)
__device__ __forceinline__ unsigned native_blend(unsigned v, float alpha, float mb) {
  return (unsigned)fminf(rintf((float)v * alpha + mb), 255.f);
}

// Four pixels xf .. xf + 3 of the row of width W whose first pixel is element b of the packed batch, b + xf a multiple of 4: read from
// `image` and written to `out` as three aligned 32-bit words when wide != 0 (image and out are 4-byte aligned themselves) and the group
// lies inside the row, byte by byte -- the pixels inside the row only -- otherwise.  px(j, c, v): the byte of channel c of pixel xf + j
// from the frame's byte v.
template <typename Px>
__device__ __forceinline__ void rgb_group4(const unsigned char* __restrict__ image, unsigned char* __restrict__ out, long b, int xf, int W,
                                           int wide, Px px) {
  if (wide && xf >= 0 && xf + 3 < W) {
    const long w0 = 3 * ((b + xf) >> 2);  // 32-bit word index of the group's first byte
    const unsigned* p = reinterpret_cast<const unsigned*>(image) + w0;
    const unsigned src0 = p[0], src1 = p[1], src2 = p[2];
    unsigned dst[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int j = i / 3, c = i % 3;
      const unsigned v = ((i < 4 ? src0 : (i < 8 ? src1 : src2)) >> (8 * (i & 3))) & 255u;
      dst[i >> 2] |= px(j, c, v) << (8 * (i & 3));
    }
    unsigned* q = reinterpret_cast<unsigned*>(out) + w0;
    q[0] = dst[0];
    q[1] = dst[1];
    q[2] = dst[2];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xf + j;
      if (x < 0 || x >= W) continue;
      const long at = 3 * (b + x);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[at + c] = (unsigned char)px(j, c, image[at + c]);
    }
  }
}

}  // namespace udet
