// The LDS-DMA ring kernels of pair launches: two problems of the same tile configuration in ONE grid (conv_igemm_ring.h is the body).
#include "conv_igemm_ring.h"

namespace udet {

// Same N blocks and K slices, independent operands: x-blocks [0, xa) belong to problem 0, the rest to problem 1.  The workgroup picks
// its parameter block in the kernel-argument segment with one scalar select.
template <int BM, int BN, int WAVES_M, int WAVES_N, int NS>
__global__ __launch_bounds__(512, NS == 2 ? 4 : 2) void conv_igemm_dma_pair_kernel(const ConvPair pp) {
  const int second = __builtin_amdgcn_readfirstlane((int)blockIdx.x >= pp.xa ? 1 : 0);
  conv_igemm_dma_body<BM, BN, WAVES_M, WAVES_N, NS, false>(pp.p[second], (int)blockIdx.x - (second ? pp.xa : 0),
                                                             second ? (int)gridDim.x - pp.xa : pp.xa);
}

int launch_igemm_ring_pair(const ConvPair& pp, int bm, int bn, int ns, dim3 grid, hipStream_t stream) {
#define UDET_TILE_LAUNCH(BM, BN, WM, WN)                                                                           \
  if (bm == BM && bn == BN) {                                                                                      \
    if (ns == 3) UDET_LAUNCH((conv_igemm_dma_pair_kernel<BM, BN, WM, WN, 3>), grid, dim3(512), 0, stream, pp);     \
    else UDET_LAUNCH((conv_igemm_dma_pair_kernel<BM, BN, WM, WN, 2>), grid, dim3(512), 0, stream, pp);             \
  } else
  UDET_GEMM_TILES(UDET_TILE_LAUNCH) return no_gemm_tile("conv pair", bm, bn);
#undef UDET_TILE_LAUNCH
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
