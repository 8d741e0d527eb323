// The rows of a frame's detections and the root-to-rank lookup built from them: what tracks.hip (the link) and instances.hip (the
// instance maps) both read.  The lookup is one int32 per pixel of the packed batch, written at the rows' roots only and never zeroed: a
// lookup counts only when the row it names holds that root.
#pragma once
#include "common.h"

namespace udet {

// rows written for a frame, whatever its counts hold: 0..k
__device__ __forceinline__ int link_rows(const long long* __restrict__ counts3, int k) {
  const long long r = counts3[2];
  return r < 0 ? 0 : r > k ? k : (int)r;
}

// row r of a frame of HW pixels enters its rank at its root (a root outside 0..HW-1 is not entered)
__device__ __forceinline__ void link_enter_roots(const long long* __restrict__ dets, int rows, long long HW, int* __restrict__ lookup,
                                                 int r) {
  if (r >= rows) return;
  const long long root = dets[(size_t)r * UDET_DET_FIELDS];
  if (root >= 0 && root < HW) lookup[root] = r;
}

}  // namespace udet
