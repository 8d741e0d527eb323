// The register-staged implicit-GEMM kernel (conv_igemm.hip describes the scheme): global -> registers -> LDS copies, double-buffered LDS,
// the A tile K-major in LDS.  FAM_PLAIN (every wave stages and multiplies) and FAM_WAVE_SPEC.
// (the kernel keeps its inline row decode, tile order and K slice, as it stood before the families were split: see conv_igemm_ring.h)
#include "conv_igemm_common.h"

namespace udet {

// WS (wave specialisation): 512-thread workgroups; waves 0-3 only read fragments from LDS and issue MFMAs, waves
// 4-7 only stage (global -> registers -> LDS) one stage ahead.  The matrix pipe of a SIMD is then fed by waves that
// never wait on HBM/L2 or on address arithmetic; one raw s_barrier per stage hands the buffers over.
template <int BM, int BN, int BK, int WAVES_M, int WAVES_N, bool WS>
__global__ __launch_bounds__(WS ? 512 : 256, WS ? 4 : 2) void conv_igemm_kernel(const ConvParams p) {
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  constexpr int NT = WS ? 512 : 256;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM * 32 == WTM && TN * 32 == WTN, "wave tile must be a multiple of 32");
  constexpr int KQ = BK / 4;                // float4 per A row per stage
  constexpr int LDA = BM + 32 / BK;         // 4*LDA == 32/KQ (mod 32): conflict-free transposing stores
  constexpr int A_ROWS = 256 / KQ;          // A rows staged per pass
  constexpr int A_LD = BM / A_ROWS;
  static_assert(A_LD * A_ROWS == BM, "BM must be a multiple of 256/(BK/4)");
  constexpr int B_F4_ROW = BN / 4;
  constexpr int B_LD = BK * B_F4_ROW / 256;
  static_assert(B_LD * 256 == BK * B_F4_ROW, "BK*BN/4 must be a multiple of 256");

  __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];
  __shared__ int rowoff[BM];
  __shared__ int2 tap_yx[UDET_MAX_TAPS];
  __shared__ int tap_w[UDET_MAX_TAPS];
  __shared__ int s_last;

  const int tid = threadIdx.x;
  const int role = __builtin_amdgcn_readfirstlane(tid >> 8);  // WS: 0 = MFMA waves, 1 = staging waves
  const int t = tid & 255;                                    // index inside the role's 256 threads
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;

  // XCD-aware tile order: consecutive M tiles (which share input halos) stay on one XCD's L2.
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const TileCls tc = tile_cls<BM>(p, bid);
  const int OHWq = tc.OHWq, Mtot = tc.Mtot /* of this class / segment */, m0 = tc.m0, tap0 = tc.tap0, ntc = tc.ntc, ooy = tc.ooy, oox = tc.oox;
  const int n0 = blockIdx.y * BN;
  const int Hs = p.H >> p.up_shift, Ws = p.W >> p.up_shift;

  // ---- per-block tables -----------------------------------------------------
  for (int i = tid; i < ntc; i += NT) {
    const ConvTap tp = conv_tap(p, tap0 + i);
    tap_yx[i] = make_int2(tp.dy, tp.dx);
    tap_w[i] = tp.widx;
  }
  for (int r = tid; r < BM; r += NT) {
    const int m = m0 + r;
    int off = -1;
    if (m < Mtot) {
      const int n = (int)fdiv(m, tc.fd_ohw), rem = m - n * OHWq;
      const int qy = (int)fdiv(rem, tc.fd_ow), qx = rem - qy * tc.OWq;
      off = (n * p.OH + qy * p.osy + ooy) * p.OW + qx * p.osx + oox;
    }
    rowoff[r] = off;
  }
  const int a_kq = t % KQ;
  int a_base[A_LD], a_iy0[A_LD], a_ix0[A_LD];
#pragma unroll
  for (int j = 0; j < A_LD; ++j) {
    const int r = t / KQ + j * A_ROWS;
    const int m = m0 + r;
    if (m < Mtot) {
      const int n = (int)fdiv(m, tc.fd_ohw), rem = m - n * OHWq;
      const int qy = (int)fdiv(rem, tc.fd_ow), qx = rem - qy * tc.OWq;
      a_base[j] = n * Hs * Ws;
      a_iy0[j] = qy * p.isy;
      a_ix0[j] = qx * p.isx;
    } else {
      a_base[j] = 0;
      a_iy0[j] = -(1 << 28);
      a_ix0[j] = 0;
    }
  }

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int Kc = p.Kc;
  const int nchunks = (ntc * Kc + BK - 1) / BK;
  int c_begin = 0, c_end = nchunks;
  if (p.ksplit > 1) {
    c_begin = (int)((unsigned)(nchunks * blockIdx.z) / (unsigned)p.ksplit);  // (32-bit: nchunks * ksplit < 2^31)
    c_end = (int)((unsigned)(nchunks * (blockIdx.z + 1)) / (unsigned)p.ksplit);
  }
  // flat-K cursors of this thread's A float4 and of its B rows; advanced by BK per stage
  const KOrder ko = korder(Kc, ntc);
  KCursor ka = kc_init(ko, c_begin * BK + a_kq * 4), kb[B_LD];
#pragma unroll
  for (int j = 0; j < B_LD; ++j) kb[j] = kc_init(ko, c_begin * BK + (t + j * 256) / B_F4_ROW);
  __syncthreads();  // tap tables visible

  float4 ra[A_LD], rb[B_LD];
  auto load_chunk = [&]() {
    int dy = 0, dx = 0;
    const bool a_ok = kc_valid(ko, ka);
    const int a_c = kc_chan(ko, ka);
    if (a_ok) {
      const int2 yx = tap_yx[ka.tap];
      dy = yx.x;
      dx = yx.y;
    }
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      int iy = a_iy0[j] + dy, ix = a_ix0[j] + dx;
      const bool ok = a_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) {
        iy >>= p.up_shift;
        ix >>= p.up_shift;
        const size_t off = (size_t)(a_base[j] + iy * Ws + ix) * p.ldx + p.x_coff + a_c;
        v = *reinterpret_cast<const float4*>(p.x + off);
        if (p.xa) {
          const float4 a = *reinterpret_cast<const float4*>(p.xa + off);
          v.x *= act_dfo(a.x, p.xact, p.xalpha);
          v.y *= act_dfo(a.y, p.xact, p.xalpha);
          v.z *= act_dfo(a.z, p.xact, p.xalpha);
          v.w *= act_dfo(a.w, p.xact, p.xalpha);
        }
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      const int c4 = (t + j * 256) % B_F4_ROW;
      const int n = n0 + c4 * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kc_valid(ko, kb[j]) && n < p.ldw)
        v = *reinterpret_cast<const float4*>(p.wp + ((size_t)tap_w[kb[j].tap] * Kc + kc_chan(ko, kb[j])) * p.ldw + n);
      rb[j] = v;
    }
    // advance the cursors to the next stage
    kc_advance(ko, ka, BK);
#pragma unroll
    for (int j = 0; j < B_LD; ++j) kc_advance(ko, kb[j], BK);
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      const int r = t / KQ + j * A_ROWS;
      As[buf][a_kq * 4 + 0][r] = ra[j].x;
      As[buf][a_kq * 4 + 1][r] = ra[j].y;
      As[buf][a_kq * 4 + 2][r] = ra[j].z;
      As[buf][a_kq * 4 + 3][r] = ra[j].w;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      const int idx = t + j * 256;
      const int krow = idx / B_F4_ROW, c4 = idx - krow * B_F4_ROW;
      *reinterpret_cast<float4*>(&Bs[buf][krow][c4 * 4]) = rb[j];
    }
  };

  // MFMA stage: fragments are double-buffered in registers (reads for k-pair kk+1 are in flight while the matrix
  // pipe works on kk), so a lone wave keeps the pipe fed without waiting out the LDS latency every 4 MFMAs.
  auto compute_chunk = [&](int buf) {
    float a[2][TM], b[2][TN];
    auto frag = [&](int s, int kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a[s][i] = As[buf][kk * 2 + lh][wm * WTM + i * 32 + li];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[s][j] = Bs[buf][kk * 2 + lh][wn * WTN + j * 32 + li];
    };
    frag(0, 0);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      if (kk + 1 < BK / 2) frag((kk + 1) & 1, kk + 1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk & 1][i], b[kk & 1][j], acc[i][j], 0, 0, 0);
      // pin the order: next k-pair's LDS reads are issued BEFORE this k-pair's MFMAs (hipcc otherwise sinks them)
      if (kk + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
    }
  };

  if constexpr (WS) {
    // raw barriers: only LDS traffic is drained (lgkmcnt), global loads stay in flight across the hand-over
    auto handover = [&]() {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };
    if (role == 1) {
      __builtin_amdgcn_s_setprio(3);  // staging waves first (see conv_igemm_dma_kernel)
      if (c_begin < c_end) {
        load_chunk();
        store_chunk(0);
        if (c_begin + 1 < c_end) load_chunk();
      }
      handover();
      int buf = 0;
      for (int c = c_begin; c < c_end; ++c) {
        if (c + 1 < c_end) {
          store_chunk(buf ^ 1);                  // stage c+1 (loaded during the previous iteration)
          if (c + 2 < c_end) load_chunk();       // stage c+2 stays in flight over the barrier
        }
        handover();
        buf ^= 1;
      }
      return;
    }
    handover();
    int buf = 0;
    for (int c = c_begin; c < c_end; ++c) {
      compute_chunk(buf);
      handover();
      buf ^= 1;
    }
  } else {
    if (c_begin < c_end) {
      load_chunk();
      store_chunk(0);
    }
    __syncthreads();
    int buf = 0;
    for (int c = c_begin; c < c_end; ++c) {
      const bool more = c + 1 < c_end;
      if (more) load_chunk();
      compute_chunk(buf);
      if (more) store_chunk(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // ---- epilogue -------------------------------------------------------------
  igemm_store<TM, TN, WTM, WTN>(p, acc, rowoff, wm, wn, li, lh, n0, tc.prow0 + m0, Mtot, p.ksplit > 1,
                                (long)blockIdx.z * p.Mall * p.ldp, xpose_scratch<sizeof(As), sizeof(Bs)>(&As[0][0][0], &Bs[0][0][0], wave));
  if (p.ksplit > 1 && p.fold) splitk_fold<BM, BN, 256>(p, rowoff, &s_last, t, n0, tc.prow0 + m0, Mtot, blockIdx.y * gridDim.x + bid);
}

int launch_igemm_staged(const ConvParams& p, int bm, int bn, bool wave_spec, dim3 grid, hipStream_t stream) {
#define UDET_TILE_LAUNCH(BM, BN, WM, WN)                                                                              \
  if (bm == BM && bn == BN) {                                                                                         \
    if (wave_spec) UDET_LAUNCH((conv_igemm_kernel<BM, BN, 32, WM, WN, true>), grid, dim3(512), 0, stream, p);         \
    else UDET_LAUNCH((conv_igemm_kernel<BM, BN, 32, WM, WN, false>), grid, dim3(256), 0, stream, p);                  \
  } else
  UDET_GEMM_TILES(UDET_TILE_LAUNCH) return no_gemm_tile("conv", bm, bn);
#undef UDET_TILE_LAUNCH
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
