// The second pass of split-K launches of the implicit-GEMM kernels: sum the slabs of partial tiles in split order and run the epilogue.
#include "conv_igemm_common.h"

namespace udet {

// second pass of a split-K launch: sum the partial slabs and run the epilogue.  SL lanes share one output element
// (each sums every SL-th slab, then a fixed-order shuffle tree): small outputs with many splits stay parallel.
template <int SL>
__global__ __launch_bounds__(256) void conv_splitk_epilogue_kernel(const ConvParams p) {
  const int Mall = p.Mall;
  const long total = (long)Mall * p.Cout;
  const int sl = threadIdx.x % SL;
  for (long e = ((long)blockIdx.x * 256 + threadIdx.x) / SL; e < total; e += (long)gridDim.x * (256 / SL)) {
    const int ma = (int)(e / p.Cout), n = (int)(e - (long)ma * p.Cout);
    // four slabs in flight per trip (the loads are independent; a plain loop waits for each before the next add);
    // the additions keep the slab order, so the sum is the same number as before
    float v = 0.f;
    const float* src = p.partial + (size_t)ma * p.ldp + n;
    const size_t slab = (size_t)Mall * p.ldp;
    int s = sl;
    for (; s + 3 * SL < p.ksplit; s += 4 * SL) {
      const float a0 = src[(size_t)s * slab], a1 = src[(size_t)(s + SL) * slab];
      const float a2 = src[(size_t)(s + 2 * SL) * slab], a3 = src[(size_t)(s + 3 * SL) * slab];
      v += a0;
      v += a1;
      v += a2;
      v += a3;
    }
    for (; s < p.ksplit; s += SL) v += src[(size_t)s * slab];
#pragma unroll
    for (int d = SL / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, SL);
    if (sl != 0) continue;
    const int off = row_pixel_off(p, ma);
    conv_epilogue(p, off, n, v);
  }
}

// the one-lane-per-element form with four consecutive channels per thread: 16-byte slab loads (a quarter of the load instructions
// and address arithmetic per byte), the same per-element summation order as conv_splitk_epilogue_kernel<1>.  Rows [row0, Mall) of the
// launch, slabs of those rows only (row0 > 0: the tail split), by workgroup `bid` of `grid`.
__device__ __forceinline__ void splitk_epilogue4_body(const ConvParams& p, const int row0, const int ksplit, const int bid, const int grid) {
  const int nq = p.ldp >> 2;  // quads per partial row (ldp = Cout rounded up to 4)
  const long total = (long)(p.Mall - row0) * nq;
  const size_t slab = (size_t)(p.Mall - row0) * p.ldp;
  const bool vec = epilogue4_out_ok(p);
  for (long e = (long)bid * 256 + threadIdx.x; e < total; e += (long)grid * 256) {
    const int mr = (int)(e / nq), n = (int)(e - (long)mr * nq) * 4;
    const float4 v = splitk_sum4<load4_plain>(p.partial + (size_t)mr * p.ldp + n, slab, ksplit);
    const int off = row_pixel_off(p, row0 + mr);
    if (vec) {  // (Cout a multiple of 4: whole quads)
      if (n < p.Cout) conv_epilogue4(p, off, n, v);
      continue;
    }
    if (n < p.Cout) conv_epilogue(p, off, n, v.x);
    if (n + 1 < p.Cout) conv_epilogue(p, off, n + 1, v.y);
    if (n + 2 < p.Cout) conv_epilogue(p, off, n + 2, v.z);
    if (n + 3 < p.Cout) conv_epilogue(p, off, n + 3, v.w);
  }
}
__global__ __launch_bounds__(256) void conv_splitk_epilogue4_kernel(const ConvParams p) {
  const bool tail = p.tail_ks > 1;  // tail split: rows >= tail_prow0 only
  splitk_epilogue4_body(p, tail ? p.tail_prow0 : 0, tail ? p.tail_ks : p.ksplit, blockIdx.x, gridDim.x);
}
// second pass of a pair launch: blocks [0, xa) reduce problem 0's slabs, the rest problem 1's
__global__ __launch_bounds__(256) void conv_splitk_epilogue4_pair_kernel(const ConvPair pp) {
  const int second = __builtin_amdgcn_readfirstlane((int)blockIdx.x >= pp.xa ? 1 : 0);
  const ConvParams& p = pp.p[second];
  splitk_epilogue4_body(p, 0, p.ksplit, (int)blockIdx.x - (second ? pp.xa : 0), second ? (int)gridDim.x - pp.xa : pp.xa);
}

// second pass of a split-K launch (no tail split, not folded): sums the ksplit slabs of p.partial and runs the epilogue
int launch_splitk_second_pass(const ConvParams& p, hipStream_t stream) {
  const long total = (long)p.Mall * p.Cout;
  // lanes per element: keep >= ~64k threads busy while the split count allows it
  const int sl = (p.ksplit >= 16 && total * 16 <= 262144) ? 16 : ((p.ksplit >= 4 && total * 4 <= 262144) ? 4 : 1);
  long nbl = (total * sl + 255) / 256;
  const int nb = (int)(nbl > 4096 ? 4096 : nbl);
  if (sl == 16) UDET_LAUNCH(conv_splitk_epilogue_kernel<16>, dim3(nb), dim3(256), 0, stream, p);
  else if (sl == 4) UDET_LAUNCH(conv_splitk_epilogue_kernel<4>, dim3(nb), dim3(256), 0, stream, p);
  else if (p.ldp % 4 == 0 && !(reinterpret_cast<uintptr_t>(p.partial) & 15)) {
    const long nb4l = ((long)p.Mall * (p.ldp >> 2) + 255) / 256;
    UDET_LAUNCH(conv_splitk_epilogue4_kernel, dim3((int)(nb4l > 4096 ? 4096 : nb4l)), dim3(256), 0, stream, p);
  } else UDET_LAUNCH(conv_splitk_epilogue_kernel<1>, dim3(nb), dim3(256), 0, stream, p);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

// the slabs of a tail split: rows from tail_prow0 on, tail_ks slices
int launch_splitk_tail_pass(const ConvParams& p, hipStream_t stream) {
  const long nb4l = ((long)(p.Mall - p.tail_prow0) * (p.ldp >> 2) + 255) / 256;
  UDET_LAUNCH(conv_splitk_epilogue4_kernel, dim3((int)(nb4l > 4096 ? 4096 : nb4l)), dim3(256), 0, stream, p);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}
// both problems of a pair launch in one grid (sets pp.xa to the first problem's share of it)
int launch_splitk_pair_pass(ConvPair& pp, hipStream_t stream) {
  const ConvParams &a = pp.p[0], &b = pp.p[1];
  const long na = ((long)a.Mall * (a.ldp >> 2) + 255) / 256, nb = ((long)b.Mall * (b.ldp >> 2) + 255) / 256;
  pp.xa = (int)(na > 2048 ? 2048 : na);
  const int xb = (int)(nb > 2048 ? 2048 : nb);
  UDET_LAUNCH(conv_splitk_epilogue4_pair_kernel, dim3(pp.xa + xb), dim3(256), 0, stream, pp);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
