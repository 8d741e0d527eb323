// The self-staging LDS-DMA kernel (FAM_SELF_STAGING; its staging and MFMA code is conv_igemm_dma.h).
#include "conv_igemm_dma.h"

namespace udet {

// ---------------------------------------------------------------------------------------------------------------
// Self-staging LDS-DMA variant: 256 threads = 4 MFMA waves that also issue the DMA of the next stage themselves (the
// address arithmetic runs in the shadow of the previous MFMAs), 16-wide K stages.  A 128x128 tile then needs 32 KB of
// LDS and one wave per SIMD, so three to four workgroups share a CU -- the MFMA pipe of a SIMD is fed by waves of
// DIFFERENT workgroups that are at different points of their stage (one waits at its barrier or for its fragments while
// another multiplies).  conv_bench on the 128-channel 3x3 layer: one wave-specialised 128x128 workgroup alone on a CU
// keeps the pipe 44 % busy, two co-resident ones 57 %.
// A stage: row-major [BM][16] (64-byte rows, 4 slots of 16 B), slot XOR-swizzled by (row>>1)&3 on the source side; B: [16][BN].
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N, bool F16 = false>
__global__ __launch_bounds__(256, 3) void conv_igemm_dma4_kernel(const ConvParams p) {
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  constexpr int BK = 16;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM * 32 == WTM && TN * 32 == WTN && BM % 64 == 0 && BN % 32 == 0, "tile");
  using Lane = DmaLane<BM, BN, BK>;  // 256 threads cover 64 rows x 4 slots per pass
  constexpr int B_LD = Lane::B_LD;

  __shared__ __attribute__((aligned(16))) float As[2][BM][BK];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];
  __shared__ int rowoff[BM];
  __shared__ int2 tap_yx[UDET_MAX_TAPS];
  __shared__ int tap_w[UDET_MAX_TAPS];
  __shared__ int s_last;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;

  const int bid = xcd_tile_order(blockIdx.x, gridDim.x);
  const TileCls tc = tile_cls<BM>(p, bid);
  const int Mtot = tc.Mtot /* of this class / segment */, m0 = tc.m0, ntc = tc.ntc;
  const int n0 = blockIdx.y * BN;
  const int Hs = p.H >> p.up_shift, Ws = p.W >> p.up_shift;

  fill_tap_tables<256>(p, tc, tap_yx, tap_w, t);
  fill_rowoff<BM, 256>(p, tc, rowoff, t);
  const int Kc = p.Kc;
  // kfast (bit 1: Kc >= 16, no up-sampled read): a stage is ONE (16-channel block, tap) pair -- uniform K cursor, see conv_igemm_dma_kernel
  const bool kfast = (p.kfast & 2) != 0;
  const int nchunks = kfast ? ntc * ((Kc + 15) >> 4) : (ntc * Kc + BK - 1) / BK;
  int c_begin, c_end;
  k_slice(nchunks, blockIdx.z, p.ksplit, c_begin, c_end);
  __syncthreads();

  // ---- staging state of this thread: A_LD rows x one 16-byte slot, B_LD float4 of the weight stage ---------------
  Lane ln;  // (channel group of a lane: slot ^ ((row>>1)&3), row = wave * 16 + lane >> 2 of each pass)
  dma_lane_init(ln, p, tc, t, lane, wave, n0, Hs, Ws);
  const KOrder ko = korder(Kc, ntc);
  ln.ka = kc_init(ko, kfast ? 0 : c_begin * BK + ln.kqs * 4);
#pragma unroll
  for (int j = 0; j < B_LD; ++j) ln.kb[j] = kc_init(ko, kfast ? 0 : c_begin * BK + (t + j * 256) / Lane::B_F4_ROW);
  // uniform cursor: stage s = (16-channel block s / ntc, tap s % ntc), kept in scalars
  const int ntc_ = ntc > 0 ? ntc : 1;
  int s_blk = __builtin_amdgcn_readfirstlane(c_begin / ntc_);
  int s_tap = __builtin_amdgcn_readfirstlane(c_begin - s_blk * ntc_);
  auto issue = [&](int buf) {
    if (kfast) dma_issue_fast<true>(p, ln, tap_yx, tap_w, As, Bs, buf, ntc, s_blk, s_tap);
    else dma_issue_generic<true>(p, ln, ko, tap_yx, tap_w, As, Bs, buf);
  };
  auto meet = [&]() {  // this wave's DMA has landed and its fragment reads are done, then meet the other waves
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  floatx16 acc[TM][TN];
  acc_zero(acc);
  const float xscale = F16 ? p.f16_xscale : 1.f;

  if (c_begin < c_end) issue(0);
  meet();
  {
    int buf = 0;
    for (int c = c_begin; c < c_end; ++c) {
      if (c + 1 < c_end) issue(buf ^ 1);  // lands while this stage is multiplied
      dma_compute_chunk<TM, TN, WTM, WTN, F16>(As, Bs, buf, acc, wm, wn, li, lh, xscale);
      meet();
      buf ^= 1;
    }
  }
  if constexpr (F16) acc_unscale(acc, xscale);
  igemm_store<TM, TN, WTM, WTN>(p, acc, rowoff, wm, wn, li, lh, n0, tc.prow0 + m0, Mtot, p.ksplit > 1,
                                (long)blockIdx.z * p.Mall * p.ldp, xpose_scratch<sizeof(As), sizeof(Bs)>(&As[0][0][0], &Bs[0][0][0], wave));
  if (p.ksplit > 1 && p.fold) splitk_fold<BM, BN, 256>(p, rowoff, &s_last, t, n0, tc.prow0 + m0, Mtot, blockIdx.y * gridDim.x + bid);
}

// The wave layout the kernel is instantiated with on tile bm x bn (waves along M; 0: not instantiated) -- the one statement of which
// tiles self-staging has, for the launcher below and for conv_self_staging_tile
constexpr int self_waves_m(int bm, int bn) { return (bm % 64 == 0 && bn % 64 == 0 && bm <= 128) ? 2 : ((bn == 32 && bm % 128 == 0) ? 4 : 0); }
template <int BM, int BN, bool F16>
static void launch_self(const ConvParams& p, dim3 grid, hipStream_t stream) {
  constexpr int WM = self_waves_m(BM, BN);
  if constexpr (WM != 0) UDET_LAUNCH((conv_igemm_dma4_kernel<BM, BN, WM, 4 / WM, F16>), grid, dim3(256), 0, stream, p);
}
bool conv_self_staging_tile(int bm, int bn) { return conv_gemm_tile(bm, bn) && self_waves_m(bm, bn) != 0; }

int launch_igemm_self(const ConvParams& p, int bm, int bn, bool f16, dim3 grid, hipStream_t stream) {
  if (!conv_self_staging_tile(bm, bn)) {
    set_error("conv: no self-staging kernel for tile %dx%d", bm, bn);
    return UDET_ERR_UNSUPPORTED;
  }
#define UDET_TILE_LAUNCH(BM, BN, WM, WN)          \
  if (bm == BM && bn == BN) {                     \
    if (f16) launch_self<BM, BN, true>(p, grid, stream); \
    else launch_self<BM, BN, false>(p, grid, stream);    \
  }
  UDET_GEMM_TILES(UDET_TILE_LAUNCH)
#undef UDET_TILE_LAUNCH
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
