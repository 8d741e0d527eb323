// The LDS-DMA ring kernels of single launches (FAM_DMA2 / FAM_DMA3 / FAM_DMA4; conv_igemm_ring.h is the body).
#include "common.h"
#ifdef UDET_EXPERIMENT
// the cycle stamps of conv_igemm_common.h: this file's kernels write them, tools/igemm_stamps.py reads them
namespace udet {
#define IGEMM_TS 12
__device__ long long g_igemm_ts[1024 * IGEMM_TS];
}  // namespace udet
#define IGEMM_STAMP_AT(b, i)                                                                                                            \
  do {                                                                                                                               \
    if (threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && (b) < 1024) g_igemm_ts[(b) * IGEMM_TS + (i)] = (long long)__builtin_readcyclecounter(); \
  } while (0)
extern "C" int udet_exp_igemm_stamps(long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(udet::g_igemm_ts), (size_t)(n < 1024 * IGEMM_TS ? n : 1024 * IGEMM_TS) * sizeof(long long));
}
#endif
#include "conv_igemm_ring.h"

namespace udet {

template <int BM, int BN, int WAVES_M, int WAVES_N, int NS, bool F16 = false>
__global__ __launch_bounds__(512, NS == 2 ? 4 : 2) void conv_igemm_dma_kernel(const ConvParams p) {
  conv_igemm_dma_body<BM, BN, WAVES_M, WAVES_N, NS, F16>(p, blockIdx.x, gridDim.x);
}

// (the 4-stage ring is not instantiated in fp16 or on the 256-row tile: those requests run the 3-stage ring)
int launch_igemm_ring(const ConvParams& p, int bm, int bn, int ns, bool f16, dim3 grid, hipStream_t stream) {
#define UDET_TILE_LAUNCH(BM, BN, WM, WN)                                                                                  \
  if (bm == BM && bn == BN) {                                                                                             \
    constexpr int NS4 = BM > 128 ? 3 : 4;                                                                                 \
    if (f16 && ns == 2) UDET_LAUNCH((conv_igemm_dma_kernel<BM, BN, WM, WN, 2, true>), grid, dim3(512), 0, stream, p);     \
    else if (f16) UDET_LAUNCH((conv_igemm_dma_kernel<BM, BN, WM, WN, 3, true>), grid, dim3(512), 0, stream, p);           \
    else if (ns == 2) UDET_LAUNCH((conv_igemm_dma_kernel<BM, BN, WM, WN, 2>), grid, dim3(512), 0, stream, p);             \
    else if (ns == 3) UDET_LAUNCH((conv_igemm_dma_kernel<BM, BN, WM, WN, 3>), grid, dim3(512), 0, stream, p);             \
    else UDET_LAUNCH((conv_igemm_dma_kernel<BM, BN, WM, WN, NS4>), grid, dim3(512), 0, stream, p);                        \
  } else
  UDET_GEMM_TILES(UDET_TILE_LAUNCH) return no_gemm_tile("conv", bm, bn);
#undef UDET_TILE_LAUNCH
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
