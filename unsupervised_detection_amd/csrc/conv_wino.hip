// Fused Winograd F(2x2,3x3) convolution on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32).
//
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A          16 multiplications per 2x2 output tile and channel pair instead of 36
//
// for the 3x3 stride-1 convolutions of the path (PWC-Net's dense estimators and context networks, the generator's 64 / 128-channel
// layers) and their backward-data passes (a 3x3 stride-1 convolution with mirrored taps and transposed weights).  Dilation d is
// handled as d*d independent d = 1 problems on the output sub-lattices.
//
// One workgroup = 4 waves = ONE wave per SIMD with the 512-register budget.  A wave owns ALL 16 Winograd positions of a
// 32-tile x 32-channel block: 16 accumulators = 256 registers, so the output transform A^T M A needs no cross-wave traffic.
// Workgroup tile = (WTY x WTX x WN waves): (4 WTY) x (8 WTX) tiles of 2x2 pixels, 32 WN output channels.
// K runs in stages of 8 input channels over a 3-buffer LDS ring:
//   input stage : the RAW (2 TH + 2) x (2 TW + 2) pixel halo, [channel quad][row][column parity][column / 2][4 channels]
//                 (16-byte slots; row stride == 4 (mod 8) slots makes the ds_read_b128 of a lane's 4x4 patch conflict-free);
//                 the input transform B^T d B (32 additions per channel) sits on the LDS -> VGPR path
//   weight stage: the pre-transformed U = G g G^T as the lane layout of the MFMA B operand, [position][lane half][n][4 channels]
//                 (ConvParams::wino_u, built by pack mode 7 / 8 whenever the weights are re-laid-out)
// both land by global_load_lds_dwordx4 issued by the MFMA waves themselves.  Lanes 0-31 hold channels 0-3 of the stage, lanes
// 32-63 channels 4-7: MFMA j of a position consumes component j of both lane halves (K = 2 per MFMA).
// The loop is software-pipelined by hand for one wave per SIMD: a stage is four phases (phase i = position row i: 16 MFMAs on 4
// accumulators), the LDS reads of phase i + 1 are issued before the multiplications of phase i, and the wait + barrier that hands
// stage k + 1 over sits between phases 2 and 3 of stage k -- phase 3 prefetches phase 0 of the next stage, so no phase starts by
// waiting out the LDS latency behind a barrier.  The DMA is inline assembly on purpose: behind the builtin, hipcc orders every later
// LDS read after the DMA with s_waitcnt vmcnt(0) (it models the DMA as a store to LDS), which serialises fill and multiplication in
// a kernel whose waves do both.
//
// Replaces the TF-1.13 Conv2D / Conv2DBackpropInput kernels behind the 3x3 stride-1 layers of
// models/PWCNet/model_pwcnet.py:476-506,559-576 and models/nets.py:19-36 (same call sites as conv_igemm.hip).
// Measured (tools/wino_bench.hip, profiles/r04_wino_proto_v2.txt): pwcnet/ctxt/dc_conv21 439 us against 701 us for the
// implicit GEMM (182 TFLOP/s direct-equivalent); error against a double-precision direct convolution 1.3e-6 of the output scale.
#include <string.h>

#include <type_traits>

#include "common.h"
#include "conv_epilogue.h"
#include "conv_host.h"
#include "wino_common.h"
#include "wino_pack.h"

namespace udet {

// libudet_exp.so only (tools/wino_stamps.py): per-workgroup time stamps of the Winograd kernels -- where a launch's fixed cost goes.
// [workgroup < 512][8]: 0 entry, 1 halo zero-fill + tables done, 2 first stage landed, 3 K loop done, 4 tile in LDS (output transform
// done), 5 stores issued, 6 stores acknowledged (shader cycles)
#ifdef UDET_EXPERIMENT
__device__ long long g_wino_ts[512 * 8];
#define WINO_STAMP(i)                                                                                  \
  do {                                                                                                 \
    if (threadIdx.x == 0 && blockIdx.x < 512 && blockIdx.z == 0) g_wino_ts[blockIdx.x * 8 + (i)] = (long long)__builtin_readcyclecounter(); \
  } while (0)
extern "C" int udet_exp_wino_stamps(long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wino_ts), (size_t)(n < 512 * 8 ? n : 512 * 8) * sizeof(long long));
}
#else
#define WINO_STAMP(i) do {} while (0)
#endif

static constexpr int wino_row_slots(int pw) { return (pw + 3) / 8 * 8 + 4; }  // smallest S >= pw with S % 8 == 4

template <int WTY, int WTX, int WN>
struct WinoGeom {
  static constexpr int NS = 3;
  static constexpr int TH = 4 * WTY, TW = 8 * WTX;        // tiles of a workgroup
  static constexpr int PH = 2 * TH + 2, PW = 2 * TW + 2;  // halo pixels
  static constexpr int CS = PW / 2;                       // used slots per column parity
  static constexpr int S = wino_row_slots(PW);            // slots per halo row
  static constexpr int HP = S / 2;                        // slot offset of the odd columns
  static constexpr int IN_SLOTS = 2 * PH * S;
  static constexpr int IN_INSTR = (IN_SLOTS + 255) / 256;  // DMA instructions per wave and stage (input)
  static constexpr int IN_WINSTR = 4 * IN_INSTR;           // wave-instructions of 64 slots: every round of four is full
  static constexpr int IN_BYTES = IN_WINSTR * 1024;
  static constexpr int BN = 32 * WN;
  static constexpr int W_BYTES = 16 * 2 * BN * 16;
  static constexpr int NW = W_BYTES / 1024;  // weight DMA wave-instructions per stage
  static constexpr int W_INSTR = NW / 4;     // ... per wave of four
  static constexpr int STAGE = IN_BYTES + W_BYTES;
  static constexpr int L = IN_INSTR + W_INSTR;
  static constexpr int LA = (L + 1) / 2;  // part A of a stage's DMA (issued in phase 3), the rest in the next phase 0
  static constexpr int LDS_BYTES = NS * STAGE;
  static_assert(S % 8 == 4 && S >= PW && HP >= CS, "row stride");
  static_assert(LDS_BYTES >= 4 * 128 * 32 * 4 && LDS_BYTES <= 160 * 1024, "the epilogue transposes 16 KB per wave through the stage buffers");
};

template <int WTY, int WTX, int WN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv_wino_kernel(const ConvParams p, const int dil,
                                                                                                  const int BY, const int BX) {
  static_assert(WTY * WTX * WN == 4, "4 waves");
  typedef WinoGeom<WTY, WTX, WN> G;
  constexpr int NS = G::NS, PH = G::PH, S = G::S;
  constexpr int IN_INSTR = G::IN_INSTR, IN_BYTES = G::IN_BYTES, BN = G::BN, STAGE = G::STAGE, L = G::L, LA = G::LA;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int wn = wave % WN, wt = wave / WN, wty = wt / WTX, wtx = wt % WTX;
  const WinoBlock blk = wino_block<BN, G::TH, G::TW>(p, dil, BY, BX);
  const int nb = blk.nb, kg0 = blk.kg0;

  unsigned in_voff[IN_INSTR];
  unsigned long long in_mask[IN_INSTR];
  wino_halo_table<G>(p, blk, smem, wave, lane, true, in_voff, in_mask);
  __syncthreads();
  // weights: (position, lane half) pair `pr` is a run of BN * 16 bytes at U + ((kg * 32 + pr) * np + nb * BN) * 4 floats
  const int np = p.wino_np;
  const float4 bias_pre = wino_bias_prefetch(p, nb * BN + wn * 32 + (lane & 7) * 4);
  const float* ubase = p.wino_u + (size_t)nb * BN * 4;
  const size_t ustride = (size_t)32 * np * 4;  // floats per stage
  unsigned w_voff;                             // this lane's byte offset inside a weight DMA instruction
  if (BN == 64) w_voff = lane * 16;
  else if (BN == 32) w_voff = (unsigned)((lane >> 5) * np + (lane & 31)) * 16;
  else w_voff = lane * 16;

  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  // DMA instructions [i0, i1) of stage kg into ring buffer `buf` (instruction index: input first, then weights)
  auto issue = [&](int kg, int buf, int i0, int i1) {
    const unsigned sb = lds0 + buf * STAGE;
    const int c0 = kg * 8;
    const float* us = ubase + (size_t)kg * ustride;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      if (i < i0 || i >= i1) continue;
      if (i < IN_INSTR) {
        wino_dma_in(in_voff[i], p.x + c0, sb + (i * 4 + wave) * 1024, in_mask[i]);
      } else {
        const int w = (i - IN_INSTR) * 4 + wave;  // wave-instruction index of the weight stage (1 KB each)
        const float* src;
        if (BN == 64) src = us + (size_t)w * np * 4;
        else if (BN == 32) src = us + (size_t)(2 * w) * np * 4;
        else src = us + (size_t)(w >> 1) * np * 4 + (w & 1) * 256;
        wino_dma_w(w_voff, src, sb + IN_BYTES + w * 1024);
      }
    }
  };

  floatx16 acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  const int ty = li >> 3, tx = li & 7;
  const int a_base = ((lh * PH + 2 * (wty * 4 + ty)) * S + (wtx * 8 + tx)) * 16;  // this lane's patch origin inside an input stage
  const int b_base = IN_BYTES + (lh * BN + wn * 32 + li) * 16;

  float4 row[4][4];
  float4 bfr[2][4];
  auto ld_row = [&](const char* sb, int r) { wino_ld_row<G>(sb, a_base, r, row[r]); };
  auto ld_bf = [&](const char* sb, int i, int s) { wino_ld_bf<G>(sb, b_base, i, bfr[s]); };

  const int nkg = blk.kg1 - kg0;
  if (nkg > 0) {
    issue(kg0, 0, 0, L);
    if (nkg > 1) issue(kg0 + 1, 1, 0, L);
    if (nkg > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ld_row(smem, 0);
    ld_row(smem, 2);
    ld_bf(smem, 0, 0);
  }

  int buf = 0;
  for (int k = 0; k < nkg; ++k) {
    const char* sb = smem + buf * STAGE;
    const int b1 = buf + 1 == NS ? 0 : buf + 1, b2 = b1 + 1 == NS ? 0 : b1 + 1;
    const char* sbn = smem + b1 * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // ---- LDS reads of the next phase, DMA parts ----
      if (i == 0) {
        ld_row(sb, 1);
        ld_bf(sb, 1, 1);
        if (k > 0 && k + 1 < nkg) issue(kg0 + k + 1, b1, LA, L);  // part B of the stage whose part A went out in the previous phase 3
      } else if (i == 1) {
        ld_bf(sb, 2, 0);
      } else if (i == 2) {
        ld_row(sb, 3);
        ld_bf(sb, 3, 1);
      } else {
        ld_row(sbn, 0);
        ld_row(sbn, 2);
        ld_bf(sbn, 0, 0);
        if (k + 2 < nkg) issue(kg0 + k + 2, b2, 0, LA);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- phase i: position row i.  t = B^T d row i: d0 - d2, d1 + d2, d2 - d1, d1 - d3 ----
      constexpr int RA[4] = {0, 1, 2, 1}, RB[4] = {2, 2, 1, 3};
      // (the phase's 32 transform additions first, then its 16 MFMAs back to back: measured 7 % faster than letting hipcc interleave
      // them -- tools/wino_bench.hip, profiles/r04_wino_proto_sched.txt)
      float vv[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float a = wino_comp(row[RA[i]][c], j), b = wino_comp(row[RB[i]][c], j);
          t[c] = i == 1 ? a + b : a - b;
        }
        wino_bt(t, vv[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc[4 * i + q] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[j][q], wino_comp(bfr[i & 1][q], j), acc[4 * i + q], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (i == 2) {  // stage k + 1 is in LDS for every wave; the buffer of stage k - 1 is free
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    }
    buf = b1;
  }

  // ---- output transform Y = A^T M A, A^T = [1 1 1 0; 0 1 -1 -1], through LDS so that a lane leaves with four channels ----
  __syncthreads();  // (every wave has read its last fragments: the stage buffers are free)
  float* xp = reinterpret_cast<float*>(smem) + wave * (128 * 32);  // [tile pixel 128][channel 32] of this wave
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = wino_acc_tile(r, lh);
    float s[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[i][0] = acc[i * 4 + 0][r] + acc[i * 4 + 1][r] + acc[i * 4 + 2][r];
      s[i][1] = acc[i * 4 + 1][r] - acc[i * 4 + 2][r] - acc[i * 4 + 3][r];
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      xp[(m * 4 + b) * 32 + li] = s[0][b] + s[1][b] + s[2][b];      // pixel (a = 0, b)
      xp[(m * 4 + 2 + b) * 32 + li] = s[1][b] - s[2][b] - s[3][b];  // pixel (a = 1, b)
    }
  }
  __builtin_amdgcn_wave_barrier();  // same wave: LDS serves its instructions in order, only the compiler must not reorder
  // the wave's 4 x 8 tile block, 128 pixels: quad P = tile * 4 + a * 2 + b
  const int Yb = blk.Y0 + 8 * wty, Xb = blk.X0 + 16 * wtx;
  wino_store_quads<16>(p, xp, lane, nb * BN + wn * 32 + (lane & 7) * 4, [&](int P) { return wino_pixel(p, blk, Yb, Xb, P >> 2, (P >> 1) & 1, P & 1); },
                       bias_pre);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Eight-wave form: TWO waves per SIMD.  What one wave per SIMD pays for (tools/wino_bench.hip, profiles/r04_wino_proto_*.txt): every
// ds_read_b128 and every DMA instruction the wave issues costs the matrix pipe tens of idle cycles that its own MFMAs cannot cover,
// however the instructions are placed.  Here waves 0-3 ("role 0") own position rows 1 and 2 of their 32-tile x 32-channel block and
// waves 4-7 ("role 1") rows 0 and 3 -- 8 accumulators = 128 registers per wave, so two waves share a SIMD and one multiplies while the
// other reads.  Row i of B^T d needs patch rows {0,2} {1,2} {2,1} {1,3}: role 0 reads rows 1 and 2 only (its second phase re-uses
// the first one's registers: d2 - d1 is formed beside d1 + d2), role 1 all four.  A stage is two phases of 16 MFMAs per wave
// (wino_common.h, wino_role_phase0 / 1), the hand-over barrier between them.  The output transform adds the roles' column sums through
// LDS once, in the epilogue: Y0 = s0 + (s1 + s2), Y1 = (s1 - s2) - s3.  Measured against the four-wave form: dc_conv21 388 vs 404 us,
// conv2_3 164 vs 177, conv2_4 168 vs 188, dc_conv31 184 vs 202 (prototype, same tiles).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int WTY, int WTX, int WN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_wino8_kernel(const ConvParams p, const int dil,
                                                                                                   const int BY, const int BX) {
  static_assert(WTY * WTX * WN == 4, "4 wave tiles");
  typedef WinoGeom<WTY, WTX, WN> G;
  constexpr int NS = G::NS, PH = G::PH, S = G::S;
  constexpr int IN_INSTR = G::IN_INSTR, IN_BYTES = G::IN_BYTES, BN = G::BN, STAGE = G::STAGE, NW = G::NW;
  constexpr int PER = (IN_INSTR * 4 + NW + 7) / 8;          // DMA instructions per wave aimed at
  constexpr int W0 = PER > IN_INSTR ? PER - IN_INSTR : 0;   // weight instructions of a role-0 wave (beside its IN_INSTR input ones)
  constexpr int W1 = (NW - 4 * W0) / 4;                     // ... of a role-1 wave
  static_assert(W1 >= 0 && 4 * W0 + 4 * W1 == NW, "weight split");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  WINO_STAMP(0);

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2, sub = wave & 3;
  const int li = lane & 31, lh = lane >> 5;
  const int wn = sub % WN, wt = sub / WN, wty = wt / WTX, wtx = wt % WTX;
  const WinoBlock blk = wino_block<BN, G::TH, G::TW>(p, dil, BY, BX);
  const int nb = blk.nb, kg0 = blk.kg0, nkg = blk.kg1 - blk.kg0;

  // input DMA of the role-0 waves (they also zero the halo / pad slots)
  unsigned in_voff[IN_INSTR];
  unsigned long long in_mask[IN_INSTR];
  wino_halo_table<G>(p, blk, smem, sub, lane, role == 0, in_voff, in_mask);
  __syncthreads();
  WINO_STAMP(1);
  const int np = p.wino_np;
  const float4 bias_pre = wino_bias_prefetch(p, nb * BN + wn * 32 + (lane & 7) * 4);
  const float* ubase = p.wino_u + (size_t)nb * BN * 4;
  const size_t ustride = (size_t)32 * np * 4;  // floats per stage
  const unsigned w_voff = BN == 32 ? (unsigned)((lane >> 5) * np + (lane & 31)) * 16 : (unsigned)lane * 16;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  auto dma_in = [&](int kg, int buf, int i) { wino_dma_in(in_voff[i], p.x + kg * 8, lds0 + buf * STAGE + (i * 4 + sub) * 1024, in_mask[i]); };
  auto dma_w = [&](int kg, int buf, int w) {  // w: wave-instruction index of the weight stage (1 KB each)
    const float* us = ubase + (size_t)kg * ustride + (BN == 64 ? (size_t)w * np * 4 : (size_t)(2 * w) * np * 4);
    wino_dma_w(w_voff, us, lds0 + buf * STAGE + IN_BYTES + w * 1024);
  };
  // this wave's DMA instructions [i0, i1) of a stage (role 0: input first, then its weights; role 1: weights)
  auto dma_part = [&](auto ROLE, int kg, int buf, int i0, int i1) {
    constexpr int R = decltype(ROLE)::value;
    constexpr int LR = R == 0 ? IN_INSTR + W0 : W1;
#pragma unroll
    for (int i = 0; i < LR; ++i) {
      if (i < i0 || i >= i1) continue;
      if (R == 0) {
        if (i < IN_INSTR) dma_in(kg, buf, i);
        else dma_w(kg, buf, (i - IN_INSTR) * 4 + sub);
      } else {
        dma_w(kg, buf, 4 * W0 + i * 4 + sub);
      }
    }
  };

  floatx16 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  const int ty = li >> 3, tx = li & 7;
  const int a_base = ((lh * PH + 2 * (wty * 4 + ty)) * S + (wtx * 8 + tx)) * 16;
  const int b_base = IN_BYTES + (lh * BN + wn * 32 + li) * 16;
  auto ld_row = [&](const char* sb, int r, float4 (&dst)[4]) { wino_ld_row<G>(sb, a_base, r, dst); };
  auto ld_bf = [&](const char* sb, int i, float4 (&dst)[4]) { wino_ld_bf<G>(sb, b_base, i, dst); };

  auto body = [&](auto ROLE) {
    constexpr int R = decltype(ROLE)::value;
    constexpr int LR = R == 0 ? IN_INSTR + W0 : W1;
    constexpr int LA = (LR + 1) / 2;
    constexpr int I0 = R == 0 ? 1 : 0, I1 = R == 0 ? 2 : 3;  // position rows of phase 0 / phase 1
    float4 ra[4], rb[4];  // role 0: patch rows 1, 2; role 1: rows 0, 2 (phase 0)
    float4 rc[4], rd[4];  // role 1: rows 1, 3 (phase 1)
    float4 bf0[4], bf1[4];
    float v1[4][4];       // role 0: phase 1's operands, formed during phase 0 from the same two rows
#pragma unroll
    for (int c = 0; c < 4; ++c) ra[c] = rb[c] = rc[c] = rd[c] = bf0[c] = bf1[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nkg > 0) dma_part(ROLE, kg0, 0, 0, LR);
    if (nkg > 1) dma_part(ROLE, kg0 + 1, 1, 0, LR);
    if (nkg > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LR) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    WINO_STAMP(2);
    ld_row(smem, R == 0 ? 1 : 0, ra);
    ld_row(smem, 2, rb);
    ld_bf(smem, I0, bf0);
    int buf = 0;
    for (int k = 0; k < nkg; ++k) {
      const char* sb = smem + buf * STAGE;
      const int b1 = buf + 1 == NS ? 0 : buf + 1, b2 = b1 + 1 == NS ? 0 : b1 + 1;
      const char* sbn = smem + b1 * STAGE;
      // ---------------- phase 0 ----------------
      if (R == 1) { ld_row(sb, 1, rc); ld_row(sb, 3, rd); }
      ld_bf(sb, I1, bf1);
      if (k > 0 && k + 1 < nkg) dma_part(ROLE, kg0 + k + 1, b1, LA, LR);  // (part A of that stage went out in the previous phase 1)
      __builtin_amdgcn_sched_barrier(0);
      wino_role_phase0<R>(ra, rb, bf0, v1, acc);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage k + 1 is in LDS for every wave; the buffer of stage k - 1 is free
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // ---------------- phase 1 ----------------
      ld_row(sbn, R == 0 ? 1 : 0, ra);
      ld_row(sbn, 2, rb);
      ld_bf(sbn, I0, bf0);
      if (k + 2 < nkg) dma_part(ROLE, kg0 + k + 2, b2, 0, LA);
      __builtin_amdgcn_sched_barrier(0);
      wino_role_phase1<R>(rc, rd, bf1, v1, acc);
      __builtin_amdgcn_sched_barrier(0);
      buf = b1;
    }
  };
  if (role == 0) body(std::integral_constant<int, 0>());
  else body(std::integral_constant<int, 1>());

  // ---- output transform + store: both roles (wino_roles_epilogue) ----
  WINO_STAMP(3);
  __syncthreads();  // (every wave has read its last fragments: the stage buffers are free)
  wino_roles_epilogue(p, blk, acc, reinterpret_cast<float*>(smem) + sub * 4096, role, lane, nb * BN + wn * 32 + (lane & 7) * 4, blk.Y0 + 8 * wty,
                      blk.X0 + 16 * wtx, bias_pre);
#ifdef UDET_EXPERIMENT
  WINO_STAMP(5);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  WINO_STAMP(6);
#endif
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Half-size form (round 6): 32 tiles x 64 channels per workgroup, FOUR waves = the two roles of the eight-wave form x two channel
// halves, a TWO-buffer LDS ring of 39 KB stages -- 78 KB per workgroup, so that TWO workgroups share a CU (two waves per SIMD again,
// now of different workgroups at different points of their stages).  Written for the launches the other forms leave half the chip
// idle on: the generator's 128-channel layers at 48 x 96 (models/nets.py:23-31) are 72 blocks of 64 tiles x 2 channel blocks = 144
// workgroups on 256 CUs, each alone on its CU at ~0.6 of the CU's matrix rate; as 288 half-size workgroups every CU has work and
// the 32 CUs that hold two run them interleaved.  One barrier per stage: stage k + 1's DMA goes out when the barrier that ended
// stage k - 1 has released its buffer, and has the whole of stage k (32 MFMAs per wave) to land.
// ---------------------------------------------------------------------------------------------------------------------------------
struct WinoHalfGeom {
  static constexpr int NS = 2, TH = 4, TW = 8;
  static constexpr int PH = 2 * TH + 2, PW = 2 * TW + 2;  // 10 x 18 halo pixels
  static constexpr int CS = PW / 2, S = wino_row_slots(PW), HP = S / 2;
  static constexpr int IN_SLOTS = 2 * PH * S;              // 400
  static constexpr int IN_WINSTR = (IN_SLOTS + 63) / 64;   // 7 wave-instructions of 64 slots
  static constexpr int IN_INSTR = (IN_WINSTR + 3) / 4;     // per wave (the last round is partly filled)
  static constexpr int IN_BYTES = IN_WINSTR * 1024;
  static constexpr int BN = 64;
  static constexpr int W_BYTES = 16 * 2 * BN * 16;         // 32 KB
  static constexpr int NW = W_BYTES / 1024;                // 32 weight wave-instructions per stage, 8 per wave
  static constexpr int STAGE = IN_BYTES + W_BYTES;         // 39 KB
  static constexpr int LDS_BYTES = NS * STAGE;             // 78 KB: two workgroups per CU
  static_assert(LDS_BYTES >= 4 * 128 * 32 * 4 && 2 * LDS_BYTES <= 160 * 1024, "epilogue scratch / two workgroups per CU");
};
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_wino_half_kernel(const ConvParams p, const int dil, const int BY,
                                                                                                       const int BX) {
  typedef WinoHalfGeom G;
  constexpr int PH = G::PH, S = G::S;
  constexpr int IN_INSTR = G::IN_INSTR, IN_BYTES = G::IN_BYTES, BN = G::BN, STAGE = G::STAGE, NW = G::NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const WinoBlock blk = wino_block<BN, G::TH, G::TW>(p, dil, BY, BX);
  const int nb = blk.nb, kg0 = blk.kg0, nkg = blk.kg1 - blk.kg0;

  // input DMA: all four waves, seven wave-instructions between them
  unsigned in_voff[IN_INSTR];
  unsigned long long in_mask[IN_INSTR];
  wino_halo_table<G>(p, blk, smem, wave, lane, true, in_voff, in_mask);
  __syncthreads();
  const int np = p.wino_np;
  const float4 bias_pre = wino_bias_prefetch(p, nb * BN + wn * 32 + (lane & 7) * 4);
  const float* ubase = p.wino_u + (size_t)nb * BN * 4;
  const size_t ustride = (size_t)32 * np * 4;  // floats per stage
  const unsigned w_voff = (unsigned)lane * 16;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  auto dma_stage = [&](int kg, int buf) {  // this wave's share of a stage: its input rounds, then 8 of the 32 weight instructions
#pragma unroll
    for (int i = 0; i < IN_INSTR; ++i) {
      if (i * 4 + wave < G::IN_WINSTR) wino_dma_in(in_voff[i], p.x + kg * 8, lds0 + buf * STAGE + (i * 4 + wave) * 1024, in_mask[i]);
    }
#pragma unroll
    for (int i = 0; i < NW / 4; ++i) {
      const int w = i * 4 + wave;
      wino_dma_w(w_voff, ubase + (size_t)kg * ustride + (size_t)w * np * 4, lds0 + buf * STAGE + IN_BYTES + w * 1024);
    }
  };

  floatx16 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  const int ty = li >> 3, tx = li & 7;
  const int a_base = ((lh * PH + 2 * ty) * S + tx) * 16;
  const int b_base = IN_BYTES + (lh * BN + wn * 32 + li) * 16;
  auto ld_row = [&](const char* sb, int r, float4 (&dst)[4]) { wino_ld_row<G>(sb, a_base, r, dst); };
  auto ld_bf = [&](const char* sb, int i, float4 (&dst)[4]) { wino_ld_bf<G>(sb, b_base, i, dst); };

  // (both role instantiations execute the same number of barriers: the trip count nkg is workgroup-uniform -- see the barrier contract
  // note in conv_wgrad_wino.hip)
  auto body = [&](auto ROLE) {
    constexpr int R = decltype(ROLE)::value;
    constexpr int I0 = R == 0 ? 1 : 0, I1 = R == 0 ? 2 : 3;  // position rows of phase 0 / phase 1
    float4 ra[4], rb[4], rc[4], rd[4], bf0[4], bf1[4];
    float v1[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) ra[c] = rb[c] = rc[c] = rd[c] = bf0[c] = bf1[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nkg > 0) dma_stage(kg0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    for (int k = 0; k < nkg; ++k) {
      const char* sb = smem + (k & 1) * STAGE;
      if (k + 1 < nkg) dma_stage(kg0 + k + 1, (k + 1) & 1);  // (that buffer held stage k - 1: released by the barrier below)
      ld_row(sb, R == 0 ? 1 : 0, ra);
      ld_row(sb, 2, rb);
      ld_bf(sb, I0, bf0);
      if (R == 1) { ld_row(sb, 1, rc); ld_row(sb, 3, rd); }
      ld_bf(sb, I1, bf1);
      __builtin_amdgcn_sched_barrier(0);
      wino_role_phase0<R>(ra, rb, bf0, v1, acc);
      __builtin_amdgcn_sched_barrier(0);
      wino_role_phase1<R>(rc, rd, bf1, v1, acc);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage k + 1 has landed (this wave's share); every wave is done reading stage k
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  };
  if (role == 0) body(std::integral_constant<int, 0>());
  else body(std::integral_constant<int, 1>());

  // ---- output transform + store: both roles (wino_roles_epilogue), one 16 KB area per channel half ----
  wino_roles_epilogue(p, blk, acc, reinterpret_cast<float*>(smem) + wn * 4096, role, lane, nb * BN + wn * 32 + (lane & 7) * 4, blk.Y0, blk.X0, bias_pre);
}

// ---- weight transform: U = G g G^T, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1] -------------------------------------------------------
__global__ __launch_bounds__(256) void wino_pack_kernel(const PackJob j, const float* __restrict__ src, float* __restrict__ dst) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < j.total; e += (long)gridDim.x * 256) wino_pack_item(j, src, nullptr, 1.f, dst, e);
}
int launch_wino_pack(const float* src, float* dst, int R, int C, int Kc, int np, int k_split, int k_gap, int transposed, hipStream_t stream) {
  PackJob j;
  memset(&j, 0, sizeof(j));
  j.T = 9; j.R = R; j.C = C; j.Kc = Kc; j.ldw = np; j.k_split = k_split; j.k_gap = k_gap;
  j.mode = transposed ? 8 : 7; j.total = (long)(Kc / 8) * 2 * np; j.gamma_off = -1;  // work items: (channel group, lane half, column)
  int nb = (int)((j.total + 255) / 256);
  if (nb > 2048) nb = 2048;
  UDET_LAUNCH(wino_pack_kernel, dim3(nb), dim3(256), 0, stream, j, src, dst);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}
// from PACKED weights [tap][Kc][ldw] + the launch's tap table: widx_at[a * 3 + b] is the packed tap at offset ((a-1) d, (b-1) d)
struct WinoTapMap { int w[9]; };
__global__ __launch_bounds__(256) void wino_from_packed_kernel(const float* __restrict__ wp, int Kc, int ldw, WinoTapMap tm, float* __restrict__ dst,
                                                               int np, long total) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int jj = (int)(e & 3);
    const long r0 = e >> 2;
    const int n = (int)(r0 % np);
    const long r1 = r0 / np;
    const int kh = (int)(r1 & 1), pos = (int)((r1 >> 1) & 15), kg = (int)(r1 >> 5);
    const int k = kg * 8 + kh * 4 + jj;
    float val = 0.f;
    if (n < ldw && k < Kc) {
      const float Gm[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
      const int pi = pos >> 2, pj = pos & 3;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) val += Gm[pi][a] * Gm[pj][b] * wp[((long)tm.w[a * 3 + b] * Kc + k) * ldw + n];
    }
    dst[e] = val;
  }
}
int launch_wino_from_packed(const ConvParams& p, float* dst, int np, hipStream_t stream) {
  int d = 0;
  WinoTapMap tm;
  if (!conv_wino_geometry(p, &d, tm.w)) {
    set_error("wino: the launch is not a 3x3 stride-1 convolution");
    return UDET_ERR_UNSUPPORTED;
  }
  const long total = (long)(p.Kc / 8) * 16 * 2 * np * 4;
  int nb = (int)((total + 255) / 256);
  if (nb > 2048) nb = 2048;
  UDET_LAUNCH(wino_from_packed_kernel, dim3(nb), dim3(256), 0, stream, p.wp, p.Kc, p.ldw, tm, dst, np, total);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int conv_wino_np(int cout) { return cout > 64 ? round_up(cout, 128) : (cout > 32 ? 64 : 32); }
size_t conv_wino_floats(int Kc, int cout) { return (size_t)(Kc / 8) * 16 * 2 * conv_wino_np(cout) * 4; }

// the launch's taps are the 3x3 grid {-d, 0, d}^2 of a stride-1 convolution onto the input grid
bool conv_wino_geometry(const ConvParams& p, int* dil, int widx_at[9]) {
  if (p.ntaps != 9 || p.ncls == 4 || p.up_shift != 0) return false;
  if (p.isy != 1 || p.isx != 1 || p.osy != 1 || p.osx != 1 || p.ooy != 0 || p.oox != 0) return false;
  if (p.OH != p.H || p.OW != p.W || p.OHq != p.OH || p.OWq != p.OW) return false;
  int at[9];
  if (!conv_taps_3x3(p.taps, p.ntaps, dil, at)) return false;
  for (int i = 0; i < 9; ++i) widx_at[i] = p.taps[at[i]].widx;
  return true;
}
bool conv_wino_ok(const ConvParams& p) {
  if (p.nseg) return false;  // segmented launches: implicit-GEMM families only
  int d, w[9];
  if (p.f16 || p.xa != nullptr || p.wino_u == nullptr || p.zero16 == nullptr) return false;
  if ((reinterpret_cast<uintptr_t>(p.zero16) | reinterpret_cast<uintptr_t>(p.wino_u) | reinterpret_cast<uintptr_t>(p.x)) & 15) return false;
  if (p.Kc < 8 || p.Kc % 8 != 0 || p.ldx % 4 != 0 || p.x_coff % 4 != 0) return false;
  if (p.wino_np < 32 || p.wino_np % 32 != 0 || p.wino_np < p.Cout) return false;
  // 32-bit element offsets on the output side, 32-bit BYTE offsets (the saddr form of the LDS-DMA) on the input side
  if ((long)p.N * p.H * p.W * (long)p.ldy >= (1L << 31) || (long)p.N * p.H * p.W * (long)p.ldx >= (1L << 30)) return false;
  return conv_wino_geometry(p, &d, w);
}
static int variant_bn(int v) { return v == 4 ? 64 : ((v & 1) == 0 ? 64 : 32); }  // bit 0: tile shape, bit 1: the eight-wave form; 4: the half-size form
bool conv_wino_variant_ok(const ConvParams& p, int v) {
  if (v < 0 || v > 4) return false;
  const int bn = variant_bn(v);
  if (p.wino_np % bn != 0) return false;
  return p.Cout > bn / 2 || bn == 32;  // (a block twice as wide as the layer only multiplies zeros)
}
static void variant_blocks(const ConvParams& p, int v, int d, int* BY, int* BX) {
  const int th = v == 4 ? 4 : 8, tw = (v & 1) ? 16 : 8;  // tiles per workgroup
  const int Hs = (p.H + d - 1) / d, Ws = (p.W + d - 1) / d;
  *BY = (Hs + 2 * th - 1) / (2 * th);
  *BX = (Ws + 2 * tw - 1) / (2 * tw);
}
long conv_wino_workgroups(const ConvParams& p, int v) {
  int d, w[9], BY, BX;
  if (!conv_wino_geometry(p, &d, w)) return 0;
  variant_blocks(p, v, d, &BY, &BX);
  return (long)p.N * d * d * BY * BX * ((p.Cout + variant_bn(v) - 1) / variant_bn(v));
}
int conv_wino_max_ksplit(const ConvParams& p, int v) {
  (void)v;
  if (!p.partial) return 1;
  int ks = (p.Kc / 8) / 6;  // >= 6 stages per slice
  if (ks > 16) ks = 16;
  const size_t per_split = (size_t)p.N * p.H * p.W * ((p.Cout + 3) & ~3);
  while (ks > 1 && per_split * ks > p.partial_cap) --ks;
  return ks < 1 ? 1 : ks;
}
int launch_splitk_second_pass(const ConvParams& p, hipStream_t stream);

template <class G>
static int launch_variant(void (*kern)(const ConvParams, const int, const int, const int), int threads, const ConvParams& p, int d, int BY, int BX,
                          hipStream_t stream) {
  UDET_TRY(conv_set_dynamic_lds(reinterpret_cast<const void*>(kern), G::LDS_BYTES));
  dim3 grid(p.N * d * d * BY * BX * ((p.Cout + G::BN - 1) / G::BN), 1, p.ksplit > 1 ? p.ksplit : 1);
  UDET_LAUNCH(kern, grid, dim3(threads), G::LDS_BYTES, stream, p, d, BY, BX);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}
int launch_conv_wino(ConvParams& p, int variant, int ks, hipStream_t stream) {
  int d, w[9], BY, BX;
  if (!conv_wino_ok(p) || !conv_wino_geometry(p, &d, w) || !conv_wino_variant_ok(p, variant)) {
    set_error("wino: launch not eligible (variant %d)", variant);
    return UDET_ERR_UNSUPPORTED;
  }
  variant_blocks(p, variant, d, &BY, &BX);
  const int cap = conv_wino_max_ksplit(p, variant);
  p.ksplit = ks > cap ? cap : (ks < 1 ? 1 : ks);
  p.fold = 0; p.tail_full = 0; p.tail_ks = 0; p.tail_prow0 = 0;
  p.ncls = 1;
  if (p.ksplit > 1) p.ldp = (p.Cout + 3) & ~3;
  int rc;
  if (variant == 0) rc = launch_variant<WinoGeom<2, 1, 2>>(conv_wino_kernel<2, 1, 2>, 256, p, d, BY, BX, stream);
  else if (variant == 1) rc = launch_variant<WinoGeom<2, 2, 1>>(conv_wino_kernel<2, 2, 1>, 256, p, d, BY, BX, stream);
  else if (variant == 2) rc = launch_variant<WinoGeom<2, 1, 2>>(conv_wino8_kernel<2, 1, 2>, 512, p, d, BY, BX, stream);
  else if (variant == 4) rc = launch_variant<WinoHalfGeom>(conv_wino_half_kernel, 256, p, d, BY, BX, stream);
  else rc = launch_variant<WinoGeom<2, 2, 1>>(conv_wino8_kernel<2, 2, 1>, 512, p, d, BY, BX, stream);
  if (rc != UDET_OK) return rc;
  if (p.ksplit > 1) return launch_splitk_second_pass(p, stream);
  return UDET_OK;
}

}  // namespace udet