// Internal: an LDS-DMA core, templated on the stage width: the self-staging kernel's (conv_igemm_self.hip, 16-wide stages; the ring
// kernels, 32-wide, keep their own inline form -- conv_igemm_ring.h says why) -- what a staging lane knows about its rows and weight quads, the two ways it issues a
// stage, and the fragment read + MFMA stage.  Who stages, how many stages are in flight and how the waves meet is the kernels' own.
//
// A stage: A row-major [BM][BK] (SLOTS = BK / 4 slots of 16 B per row), the slot index XOR-swizzled by (row >> 1) & (SLOTS - 1) on the
// SOURCE side (DMA writes LDS lane-linearly); B [BK][BN], the packed-weight layout itself.
#pragma once
#include "conv_igemm_common.h"

namespace udet {

typedef __attribute__((address_space(3))) void* lds_ptr;

// The staging state of one of 256 lanes: A_LD rows x one 16-byte slot, B_LD float4 of the weight stage
template <int BM, int BN, int BK>
struct DmaLane {
  static constexpr int SLOTS = BK / 4;
  static constexpr int ROWS = 256 / SLOTS;   // A rows the 256 lanes cover per pass
  static constexpr int WROWS = 64 / SLOTS;   // ... one wave
  static constexpr int A_LD = BM / ROWS;
  static constexpr int B_F4_ROW = BN / 4;
  static constexpr int B_F4 = BK * B_F4_ROW;  // float4 of one weight stage (128 for BK = 16, BN = 32: half of the lanes load)
  static constexpr int B_LD = (B_F4 + 255) / 256;
  static_assert(A_LD * ROWS == BM, "BM must be a multiple of the rows of one pass");
  static_assert(B_F4 % 64 == 0, "whole waves issue the weight DMA");
  int t, wave, n0, Ws;
  int kqs;            // channel group this lane holds: slot ^ ((row >> 1) & (SLOTS - 1))
  const float* zero;  // halo / K-tail lanes read a 16-byte zero block instead of branching
  int a_base[A_LD], a_iy0[A_LD], a_ix0[A_LD];
  // uniform cursor: per lane and row only constants remain -- the element offset of the row's pixel at tap (0,0) and channel slot kqs,
  // the weight row / column of each B quad
  int a_off[A_LD], b_off[B_LD], b_row[B_LD];
  bool b_col[B_LD];
  KCursor ka, kb[B_LD];  // generic cursor (the caller initialises it where it is used)
};
template <int BM, int BN, int BK>
__device__ __forceinline__ void dma_lane_init(DmaLane<BM, BN, BK>& L, const ConvParams& p, const TileCls& tc, int t, int lane, int wave,
                                              int n0, int Hs, int Ws) {
  using D = DmaLane<BM, BN, BK>;
  L.t = t; L.wave = wave; L.n0 = n0; L.Ws = Ws;
  L.kqs = (lane & (D::SLOTS - 1)) ^ ((wave * (D::WROWS / 2) + lane / (2 * D::SLOTS)) & (D::SLOTS - 1));
#pragma unroll
  for (int j = 0; j < D::A_LD; ++j)
    row_a_origin(p, tc, tc.m0 + j * D::ROWS + wave * D::WROWS + lane / D::SLOTS, Hs, Ws, L.a_base[j], L.a_iy0[j], L.a_ix0[j]);
  L.zero = p.zero16;
#pragma unroll
  for (int j = 0; j < D::A_LD; ++j)
    L.a_off[j] = L.a_iy0[j] < -(1 << 27) ? 0 : (L.a_base[j] + L.a_iy0[j] * Ws + L.a_ix0[j]) * p.ldx + p.x_coff + L.kqs * 4;  // (rows past the grid: never read)
#pragma unroll
  for (int j = 0; j < D::B_LD; ++j) {
    const int idx = t + j * 256, row = idx / D::B_F4_ROW, n = n0 + (idx - row * D::B_F4_ROW) * 4;
    L.b_row[j] = row;
    L.b_off[j] = row * p.ldw + n;
    L.b_col[j] = n < p.ldw;
  }
}

// Generic K cursor (stages may straddle taps: Kc < BK or an up-sampled read): per-lane (block, tap, channel) cursors advanced with
// data-dependent control flow -- ~1500 instructions per stage for a 128x128 tile.  The uniform cursor below needs ~100.
// GUARD_B: fewer weight quads than lanes may exist (the test is wave-uniform); the ring's stages always fill whole passes.
template <bool GUARD_B, int BM, int BN, int BK, int NS>
__device__ __forceinline__ void dma_issue_generic(const ConvParams& p, DmaLane<BM, BN, BK>& L, const KOrder& ko, const int2* tap_yx,
                                                  const int* tap_w, float (&As)[NS][BM][BK], float (&Bs)[NS][BK][BN], int buf) {
  using D = DmaLane<BM, BN, BK>;
  int dy = 0, dx = 0;
  const bool a_ok = kc_valid(ko, L.ka);
  const int a_c = kc_chan(ko, L.ka);
  if (a_ok) {
    const int2 yx = tap_yx[L.ka.tap];
    dy = yx.x;
    dx = yx.y;
  }
#pragma unroll
  for (int j = 0; j < D::A_LD; ++j) {
    int iy = L.a_iy0[j] + dy, ix = L.a_ix0[j] + dx;
    const bool ok = a_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    iy >>= p.up_shift;
    ix >>= p.up_shift;
    const float* src = ok ? p.x + ((size_t)(L.a_base[j] + iy * L.Ws + ix) * p.ldx + p.x_coff + a_c) : L.zero;
    __builtin_amdgcn_global_load_lds(src, (lds_ptr)&As[buf][j * D::ROWS + L.wave * D::WROWS][0], 16, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < D::B_LD; ++j) {
    if (!GUARD_B || j * 256 + L.wave * 64 < D::B_F4) {
      const int c4 = (L.t + j * 256) % D::B_F4_ROW;
      const int n = L.n0 + c4 * 4;
      const bool ok = kc_valid(ko, L.kb[j]) && n < p.ldw;
      const int wi = ok ? tap_w[L.kb[j].tap] : 0;
      const float* src = ok ? p.wp + (((size_t)wi * p.Kc + kc_chan(ko, L.kb[j])) * p.ldw + n) : L.zero;
      __builtin_amdgcn_global_load_lds(src, (lds_ptr)(&Bs[buf][0][0] + (j * 256 + L.wave * 64) * 4), 16, 0, 0);
    }
  }
  kc_advance(ko, L.ka, BK);
#pragma unroll
  for (int j = 0; j < D::B_LD; ++j) kc_advance(ko, L.kb[j], BK);
}
// Uniform K cursor: stage s = (BK-channel block s / ntc, tap s % ntc); the caller keeps (s_blk, s_tap) in scalars
template <bool GUARD_B, int BM, int BN, int BK, int NS>
__device__ __forceinline__ void dma_issue_fast(const ConvParams& p, const DmaLane<BM, BN, BK>& L, const int2* tap_yx, const int* tap_w,
                                               float (&As)[NS][BM][BK], float (&Bs)[NS][BK][BN], int buf, int ntc, int& s_blk, int& s_tap) {
  using D = DmaLane<BM, BN, BK>;
  const int2 yx = tap_yx[s_tap];
  const int dy = yx.x, dx = yx.y, c0 = s_blk * BK;
  const int tap_off = (dy * L.Ws + dx) * p.ldx + c0;
  const bool ch_ok = c0 + L.kqs * 4 < p.Kc;
#pragma unroll
  for (int j = 0; j < D::A_LD; ++j) {
    const int iy = L.a_iy0[j] + dy, ix = L.a_ix0[j] + dx;
    const bool ok = ch_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    const float* src = ok ? p.x + (L.a_off[j] + tap_off) : L.zero;
    __builtin_amdgcn_global_load_lds(src, (lds_ptr)&As[buf][j * D::ROWS + L.wave * D::WROWS][0], 16, 0, 0);
  }
  const float* wrow = p.wp + ((size_t)tap_w[s_tap] * p.Kc + c0) * p.ldw;
#pragma unroll
  for (int j = 0; j < D::B_LD; ++j) {
    if (!GUARD_B || j * 256 + L.wave * 64 < D::B_F4) {
      const bool ok = L.b_col[j] && c0 + L.b_row[j] < p.Kc;
      const float* src = ok ? wrow + L.b_off[j] : L.zero;
      __builtin_amdgcn_global_load_lds(src, (lds_ptr)(&Bs[buf][0][0] + (j * 256 + L.wave * 64) * 4), 16, 0, 0);
    }
  }
  if (++s_tap == ntc) { s_tap = 0; ++s_blk; }
}

// MFMA stage.  A wave reads its A fragment as ONE ds_read_b128 per 32 rows per 4 k-pairs (conflict-free under the swizzle) and walks K
// in the permuted order {4g+e : g = 2*kk+half}, which the B fragment reads ([k][n] rows, ds_read_b32) follow.  Fragments are
// double-buffered in registers: the reads for kk+1 are in flight while the matrix pipe works on kk.
template <int TM, int TN, int WTM, int WTN, bool F16, int BM, int BN, int BK, int NS>
__device__ __forceinline__ void dma_compute_chunk(float (&As)[NS][BM][BK], float (&Bs)[NS][BK][BN], int buf, floatx16 (&acc)[TM][TN],
                                                  int wm, int wn, int li, int lh, float xscale) {
  const int swz = (li >> 1) & (BK / 4 - 1);  // (row>>1)&(SLOTS-1) of every row this lane reads (wave / sub-tile offsets are multiples of 2 * SLOTS)
  float4 a[2][TM];
  float b[2][4][TN];
  auto frag = [&](int s, int kk) {
    const int g = 2 * kk + lh;  // channel group of this lane half
#pragma unroll
    for (int i = 0; i < TM; ++i) a[s][i] = *reinterpret_cast<const float4*>(&As[buf][wm * WTM + i * 32 + li][(g ^ swz) * 4]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < TN; ++j) b[s][e][j] = Bs[buf][g * 4 + e][wn * WTN + j * 32 + li];
  };
  frag(0, 0);
#pragma unroll
  for (int kk = 0; kk < BK / 8; ++kk) {
    if (kk + 1 < BK / 8) frag((kk + 1) & 1, kk + 1);
    if constexpr (F16) {  // the lane half's four consecutive K values of a fragment are one fp16 operand of the K = 8 MFMA
      halfx4 ah[TM], bh[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        ah[i] = halfx4{(_Float16)(a[kk & 1][i].x * xscale), (_Float16)(a[kk & 1][i].y * xscale), (_Float16)(a[kk & 1][i].z * xscale),
                       (_Float16)(a[kk & 1][i].w * xscale)};
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bh[j] = halfx4{(_Float16)b[kk & 1][0][j], (_Float16)b[kk & 1][1][j], (_Float16)b[kk & 1][2][j], (_Float16)b[kk & 1][3][j]};
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x8f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float av = e == 0 ? a[kk & 1][i].x : (e == 1 ? a[kk & 1][i].y : (e == 2 ? a[kk & 1][i].z : a[kk & 1][i].w));
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[kk & 1][e][j], acc[i][j], 0, 0, 0);
        }
      }
    }
    // pin the order: the next fragment's LDS reads are issued BEFORE this one's MFMAs (hipcc otherwise sinks them)
    if (kk + 1 < BK / 8) __builtin_amdgcn_sched_group_barrier(0x100, TM + 4 * TN, 0);
    if constexpr (!F16) __builtin_amdgcn_sched_group_barrier(0x008, 4 * TM * TN, 0);
  }
}

}  // namespace udet
