// Argument checks shared by the extern "C" entry points (host code only).  Each sets udet_last_error() with the entry point's name and the
// values it requires and returns true when the call must be refused with UDET_ERR_ARG.
#pragma once
#include "common.h"

namespace udet {

// A batch of n samples (frames, or sequences of frames) in packed buffers: n in 1..65535 (a grid dimension), the largest frame max_h x max_w
// at least 1 x 1 and below 2^31 pixels (32-bit pixel indices inside a frame), total (pixels or frames in all) at least 1.
inline bool bad_batch(const char* fn, int n, int max_h, int max_w, size_t total) {
  if (n >= 1 && n <= 65535 && max_h >= 1 && max_w >= 1 && (long)max_h * max_w <= 0x7fffffffL && total >= 1) return false;
  set_error("%s: bad argument (n = %d in 1..65535, frames of up to %d x %d, at least 1 x 1 and below 2^31 pixels, a total of %zu, at least 1)",
            fn, n, max_h, max_w, total);
  return true;
}

// The caller's workspace: non-null, at least `need` bytes, aligned to `align` (a power of two).
inline bool bad_workspace(const char* fn, const void* ws, size_t have, size_t need, size_t align) {
  if (ws && have >= need && !(reinterpret_cast<uintptr_t>(ws) & (align - 1))) return false;
  set_error("%s: workspace needs %zu bytes, %zu-byte aligned", fn, need, align);
  return true;
}

}  // namespace udet
