// Horizontal runs of equal ids inside a wave: what lets the per-pixel kernels of detections.hip and tracks.hip issue one atomic per run
// and not one per pixel.
#pragma once
#include "common.h"

namespace udet {

// The horizontal run of equal ids (id >= 0) that starts at this lane, for 64 consecutive pixels of one sample: its length, or 0 where
// the lane does not start one.  x: the pixel's column (a run ends at the row's end).  Every lane of the wave calls this.
__device__ __forceinline__ int det_run_length(int id, int x, int lane) {
  const int prev = __shfl_up(id, 1);
  const bool cont = id >= 0 && lane != 0 && x != 0 && prev == id;
  const unsigned long long mcont = __ballot(cont);
  if (id < 0 || cont) return 0;
  const unsigned long long rest = lane == 63 ? 0ull : (mcont >> (lane + 1));  // the top bit of rest is 0: ~rest is never 0
  return __ffsll((long long)~rest);                                          // 1 + the lanes after this one that continue the run
}

}  // namespace udet
