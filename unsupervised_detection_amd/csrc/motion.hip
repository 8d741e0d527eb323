// Displacements from a flow field: udet_flow_displacements_ragged samples n flow fields of one common size fh x fw at the
// pixel centres of n native-size frames (packed layout, sample i = H_i x W_i at offsets[i]), scales the vector to native pixels, rounds
// it to integers and packs it, dx in the low 16 bits and dy in the high 16 -- what the motion link of tracks.hip reads.  One launch:
//   flow_disp_kernel   one lane per pixel, a wave on 64 consecutive pixels of one sample: the four taps of the bilinear sample come from
//                      the flow field of the lane's frame (some hundred KB: L2), the result is one aligned 32-bit store
// No LDS, no atomics, no workspace.  include/udet.h fixes the arithmetic operation by operation; every float32 operation below is one
// rounding (the file is compiled without contraction into FMA, see the pragma below), so the output is the header's numbers exactly.  The taps are clamped to the grid and a pixel past its sample is not written, so nothing indexes outside flow and disp
// whatever the flow holds; offsets / hw are validated by the host caller (native_motion.flow_displacements).
#include <math.h>

#include "../../include/udet.h"
#include "common.h"
#include "host_checks.h"

// Contraction is switched off for every expression of this file, here and -- like for the other files whose float32 results are pinned
// -- in the Makefile.  (HIP's __fmul_rn / __fadd_rn are no way round it: they are plain * and + in a header compiled with contraction
// on, and once inlined they fuse whatever this file says.)
#pragma clang fp contract(off)

namespace udet {

#define MOTION_PPT 16  // pixels per thread of the grid: 4096 pixels per workgroup, as for the overlap pass that reads the result

// Where output coordinate v of `size` lies on a grid of `cells`: the lower tap, the upper tap and the weight of the upper one.
__device__ __forceinline__ void flow_tap(int v, float ratio, int cells, int* lo, int* hi, float* a) {
  float g = ((float)v + 0.5f) * ratio - 0.5f;
  g = fminf(fmaxf(g, 0.f), (float)(cells - 1));
  const float f = floorf(g);
  *lo = (int)f;  // 0 .. cells - 1
  *hi = min(*lo + 1, cells - 1);
  *a = g - f;
}

__device__ __forceinline__ float flow_lerp(float p, float q, float a) { return p + a * (q - p); }

// rint (ties to even) of v * scale as a 16-bit displacement: a NaN gives 0, everything else is clamped to -32768 .. 32767.
__device__ __forceinline__ int flow_round(float v, float scale) {
  const float r = rintf(v * scale);
  if (r != r) return 0;
  return (int)fminf(fmaxf(r, -32768.f), 32767.f);
}

__global__ __launch_bounds__(256) void flow_disp_kernel(const float2* __restrict__ flow, int fh, int fw, const long long* __restrict__ offsets,
                                                        const int* __restrict__ hw, int* __restrict__ disp) {
  const int i = blockIdx.y, t = threadIdx.x;
  const int H = hw[2 * i], W = hw[2 * i + 1];
  const long long HW = (long long)H * W;
  const float rx = (float)fw / (float)W, ry = (float)fh / (float)H;  // correctly rounded divisions (hipcc's default for float32)
  const float sx = (float)W / (float)fw, sy = (float)H / (float)fh;
  const float2* __restrict__ field = flow + (size_t)i * fh * fw;
  int* __restrict__ out = disp + offsets[i];
  for (long long base = (long long)blockIdx.x * 256; base < HW; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long p = base + t;
    if (p >= HW) continue;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    int x0, x1, y0, y1;
    float ax, ay;
    flow_tap(x, rx, fw, &x0, &x1, &ax);
    flow_tap(y, ry, fh, &y0, &y1, &ay);
    const float2 f00 = field[(size_t)y0 * fw + x0], f01 = field[(size_t)y0 * fw + x1];
    const float2 f10 = field[(size_t)y1 * fw + x0], f11 = field[(size_t)y1 * fw + x1];
    const float u = flow_lerp(flow_lerp(f00.x, f01.x, ax), flow_lerp(f10.x, f11.x, ax), ay);
    const float v = flow_lerp(flow_lerp(f00.y, f01.y, ax), flow_lerp(f10.y, f11.y, ax), ay);
    const int dx = flow_round(u, sx), dy = flow_round(v, sy);
    out[p] = (int)(((unsigned)dx & 0xffffu) | ((unsigned)dy << 16));
  }
}

}  // namespace udet

using namespace udet;

extern "C" {

int udet_flow_displacements_ragged(const float* flow, int n, int fh, int fw, const long long* offsets, const int* hw, int max_h, int max_w,
                                   size_t total_pixels, int* disp, void* stream) {
  if (bad_batch("flow_displacements_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!flow || !offsets || !hw || !disp) {
    set_error("flow_displacements_ragged: bad argument (non-null flow, offsets, hw and disp)");
    return UDET_ERR_ARG;
  }
  if (fh < 1 || fh > 32767 || fw < 1 || fw > 32767) {
    set_error("flow_displacements_ragged: a flow grid of %d x %d, each in 1..32767, is required", fh, fw);
    return UDET_ERR_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(flow) & 7) || (reinterpret_cast<uintptr_t>(disp) & 3)) {
    set_error("flow_displacements_ragged: flow must be 8-byte aligned (one (u, v) pair per load), disp 4-byte aligned");
    return UDET_ERR_ARG;
  }
  const long nb = ((long)max_h * max_w + 256 * MOTION_PPT - 1) / (256 * MOTION_PPT);  // <= 2^31 / 4096
  hipLaunchKernelGGL(flow_disp_kernel, dim3((unsigned)nb, n), dim3(256), 0, (hipStream_t)stream, (const float2*)flow, fh, fw, offsets, hw,
                     disp);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
