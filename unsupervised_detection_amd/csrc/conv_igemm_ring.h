// Internal: the body of the LDS-DMA ring kernels, shared by conv_igemm_ring.hip (single launches) and conv_igemm_ring_pair.hip (pair
// launches) -- two files so that the build compiles them side by side.
//
// The body keeps its own inline form of the staging and MFMA code, of the row decode and of the tile order, as it stood before the
// families were split: with the shared forms of conv_igemm_common.h / conv_igemm_dma.h (which the self-staging kernel uses) hipcc
// allocated and scheduled the 128x128 kernels differently, and they ran 1.5-4.5 % slower on a 128-channel 3x3 layer
// (profiles/NOTES.md).  In this form 28 of the 29 single-launch kernels are instruction for instruction what they were.
#pragma once
#include "conv_igemm_common.h"

namespace udet {

// ---------------------------------------------------------------------------------------------------------------
// LDS-DMA variant (forward convolutions and backward-data of linear layers: no act' on the A operand).
// The staging waves issue `global_load_lds_dwordx4` (16 B per lane straight into LDS, no VGPR round trip, no
// ds_write pass); halo / K-tail lanes read a 16-byte zero block instead of branching.  DMA writes LDS lane-linearly,
// so the A stage is row-major [BM][32] (one 128-byte line per pixel) with the 16-byte slot index XOR-swizzled by
// (row>>1)&7 on the SOURCE side; the MFMA waves read their fragment as ONE ds_read_b128 per 32 rows per 4 k-pairs
// (conflict-free under the swizzle) and walk K in the permuted order {4g+e : g = 2*kk+half}, which the B fragment
// reads ([k][n] rows, ds_read_b32) follow.  Same flat-K / parity-class / split-K semantics as conv_igemm_kernel.
// ---------------------------------------------------------------------------------------------------------------
// (the body takes the workgroup's x index and the x extent of ITS problem as arguments: a pair launch -- conv_igemm_dma_pair_kernel below --
// runs two problems of the same tile configuration in one grid, each workgroup seeing only its own problem's parameter block)
template <int BM, int BN, int WAVES_M, int WAVES_N, int NS, bool F16>
__device__ __forceinline__ void conv_igemm_dma_body(const ConvParams& p, const int bid_x, const int grid_x) {
  static_assert(NS >= 2 && NS <= 4, "stages");
  static_assert(WAVES_M * WAVES_N == 4, "4 MFMA waves");
  constexpr int BK = 32;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM * 32 == WTM && TN * 32 == WTN && BM % 32 == 0, "tile");
  constexpr int A_LD = BM / 32;               // 256 staging threads cover 32 rows x 8 slots per pass
  constexpr int B_F4_ROW = BN / 4;
  constexpr int B_LD = BK * B_F4_ROW / 256;
  static_assert(B_LD * 256 == BK * B_F4_ROW, "BK*BN/4 must be a multiple of 256");
  typedef __attribute__((address_space(3))) void* lds_ptr;

  __shared__ __attribute__((aligned(16))) float As[NS][BM][BK];
  __shared__ __attribute__((aligned(16))) float Bs[NS][BK][BN];
  __shared__ int rowoff[BM];
  __shared__ int2 tap_yx[UDET_MAX_TAPS];
  __shared__ int tap_w[UDET_MAX_TAPS];
  __shared__ int s_last;

  IGEMM_STAMP(0);
  const int tid = threadIdx.x;
  // Speculative tap fetch (round 6): the tap table of an unsegmented single-class launch starts at taps[0], whatever the block decodes
  // to -- its (vector) load from the kernel-argument block goes out HERE, beside the scalar loads of the fields the decode waits for,
  // instead of behind them (two back-to-back cold misses, ~1 us each, in front of every launch's first DMA)
  int spec_dy = 0, spec_dx = 0, spec_widx = 0;  // (three scalars, not a ConvTap copy: hipcc keeps the 12-byte struct in scratch memory)
  if (tid < UDET_MAX_TAPS) {
    spec_dy = p.taps[tid].dy;
    spec_dx = p.taps[tid].dx;
    spec_widx = p.taps[tid].widx;
  }
  const int role = __builtin_amdgcn_readfirstlane(tid >> 8);  // 0 = MFMA waves, 1 = staging waves
  const int t = tid & 255;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;

  int bid = bid_x;
  int kz = blockIdx.z, knz = p.ksplit;  // K slice of this workgroup / slices of its tile
  {
    int nwg = grid_x;
    if (p.tail_ks > 1) {  // tail split: the x-blocks past tail_full are cut into tail_ks slices, the others run whole
      nwg = p.tail_full;
      knz = 1;
      if (bid >= p.tail_full) {
        const int r = bid - p.tail_full;
        kz = r % p.tail_ks;
        bid = p.tail_full + r / p.tail_ks;
        knz = p.tail_ks;
      }
    }
    if (bid < nwg) {
      const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
      bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
  }
  const TileCls tc = tile_cls<BM>(p, bid);
  const int OHWq = tc.OHWq, Mtot = tc.Mtot /* of this class / segment */, m0 = tc.m0, tap0 = tc.tap0, ntc = tc.ntc, ooy = tc.ooy, oox = tc.oox;
  const int n0 = blockIdx.y * BN;
  const int Hs = p.H >> p.up_shift, Ws = p.W >> p.up_shift;
  IGEMM_STAMP(6);

  if (p.nseg == 0 && tap0 == 0) {  // (uniform) the speculative fetch is this block's table
    if (tid < ntc) {
      tap_yx[tid] = make_int2(spec_dy, spec_dx);
      tap_w[tid] = spec_widx;
    }
  } else {
    for (int i = tid; i < ntc; i += 512) {
      const ConvTap tp = conv_tap(p, tap0 + i);
      tap_yx[i] = make_int2(tp.dy, tp.dx);
      tap_w[i] = tp.widx;
    }
  }
  // (the output row offsets are read by the tile store only: the MFMA waves fill them while they wait for the first stage -- below --
  // instead of in front of the barrier every wave's first DMA waits behind: round 6, tools/igemm_stamps.py)
  const int Kc = p.Kc;
  // kfast (Kc >= 32, no up-sampled read): a stage is ONE (channel block, tap) pair -- the last, narrower block is padded with zero
  // lanes instead of straddling into the next tap -- so the K cursor is wave-uniform (see the staging waves)
  // kfast bit 2 (Kc in {4, 8, 16}): a stage is 32 / Kc WHOLE taps; the tap of a lane follows from its channel slot (a per-lane constant)
  const int tsh = Kc == 4 ? 3 : (Kc == 8 ? 2 : 1);  // log2(taps per stage) of the packed form (Kc = 4, 8, 16): shifts, not run-time divisions
  const int tps = (p.kfast & 4) ? 1 << tsh : 1;     // taps per stage
  const int nchunks = (p.kfast & 1) ? ntc * ((Kc + 31) >> 5) : ((p.kfast & 4) ? (ntc + tps - 1) >> tsh : (ntc * Kc + BK - 1) / BK);
  int c_begin = 0, c_end = nchunks;
  if (knz > 1) {
    c_begin = (int)((unsigned)(nchunks * kz) / (unsigned)knz);  // (nchunks * knz < 2^31: 32-bit divisions, a third of the 64-bit ones' instructions)
    c_end = (int)((unsigned)(nchunks * (kz + 1)) / (unsigned)knz);
  }
  // slab of this slice: regular split-K keeps whole-output slabs, the tail split only the rows from tail_prow0 on
  const long slab_off = p.tail_ks > 1 ? ((long)kz * (p.Mall - p.tail_prow0) - p.tail_prow0) * p.ldp : (long)kz * p.Mall * p.ldp;
  IGEMM_STAMP(7);
  // (the barrier that publishes the tap tables sits inside the two role paths: the staging waves reach it only after their per-row
  // address arithmetic, which needs no table -- that work runs beside the kernel-argument / tap-table latency instead of behind it)

  if (role == 1) {
    // ------------------------------------------------ staging waves ------------------------------------------------
    // issue priority over the MFMA waves of the same SIMD (this and the co-resident workgroups'): a stage's DMA goes out as soon as
    // its buffer is free instead of waiting for gaps between MFMAs (128x64 tile on the 568-channel layer: 920 -> 750 us)
    __builtin_amdgcn_s_setprio(3);
    const int kq = lane & 7;                                  // LDS slot written by this lane (lane-linear)
    const int kqs = kq ^ ((wave * 4 + (lane >> 4)) & 7);      // channel group it holds: slot ^ ((row>>1)&7)
    int a_base[A_LD], a_iy0[A_LD], a_ix0[A_LD];
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
      const int m = m0 + j * 32 + wave * 8 + (lane >> 3);
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
    const float* zero = p.zero16;
    // Generic K cursor (stages may straddle taps: Kc < 32 or an up-sampled read): per-lane (block, tap, channel) cursors advanced
    // with data-dependent control flow -- ~1500 instructions per stage for a 128x128 tile, more than the 4096 MFMA cycles of the
    // stage leave room for on a SIMD that also hosts an MFMA wave.  The uniform cursor below needs ~100.
    // (the generic cursor's set-up is a dozen integer divisions by run-time values, ~40 instructions each: only launches that use it pay
    // for it -- round 6: the staging waves' set-up was ~3 700 cycles in front of EVERY launch's first DMA, tools/igemm_stamps.py)
    const KOrder ko = korder(Kc, ntc);
    KCursor ka, kb[B_LD];
    ka.blk = ka.tap = ka.c = ka.w = 0;
#pragma unroll
    for (int j = 0; j < B_LD; ++j) kb[j] = ka;
    if (!(p.kfast & 5)) {
      ka = kc_init(ko, c_begin * BK + kqs * 4);
#pragma unroll
      for (int j = 0; j < B_LD; ++j) kb[j] = kc_init(ko, c_begin * BK + (t + j * 256) / B_F4_ROW);
    }
    auto issue_generic = [&](int buf) {
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
        iy >>= p.up_shift;
        ix >>= p.up_shift;
        const float* src = ok ? p.x + ((size_t)(a_base[j] + iy * Ws + ix) * p.ldx + p.x_coff + a_c) : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_ptr)&As[buf][j * 32 + wave * 8][0], 16, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < B_LD; ++j) {
        const int c4 = (t + j * 256) % B_F4_ROW;
        const int n = n0 + c4 * 4;
        const bool ok = kc_valid(ko, kb[j]) && n < p.ldw;
        const int wi = ok ? tap_w[kb[j].tap] : 0;
        const float* src = ok ? p.wp + (((size_t)wi * Kc + kc_chan(ko, kb[j])) * p.ldw + n) : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_ptr)(&Bs[buf][0][0] + (j * 256 + wave * 64) * 4), 16, 0, 0);
      }
      kc_advance(ko, ka, BK);
#pragma unroll
      for (int j = 0; j < B_LD; ++j) kc_advance(ko, kb[j], BK);
    };
    // Uniform K cursor: stage s = (block s / ntc, tap s % ntc), kept in scalars.  Per lane and row only constants remain: the
    // element offset of the row's pixel at tap (0,0) and channel slot kqs, the weight row / column of each B quad.
    int a_off[A_LD];
#pragma unroll
    for (int j = 0; j < A_LD; ++j)
      a_off[j] = a_iy0[j] < -(1 << 27) ? 0 : (a_base[j] + a_iy0[j] * Ws + a_ix0[j]) * p.ldx + p.x_coff + kqs * 4;  // (rows past the grid: never read)
    int b_off[B_LD], b_row[B_LD];
    bool b_col[B_LD];
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      const int idx = t + j * 256, row = idx / B_F4_ROW, n = n0 + (idx - row * B_F4_ROW) * 4;
      b_row[j] = row;
      b_off[j] = row * p.ldw + n;
      b_col[j] = n < p.ldw;
    }
    int s_blk = c_begin == 0 ? 0 : __builtin_amdgcn_readfirstlane(c_begin / (ntc > 0 ? ntc : 1));  // (unsplit launches: no division)
    int s_tap = __builtin_amdgcn_readfirstlane(c_begin - s_blk * ntc);
    auto issue_fast = [&](int buf) {
      const int2 yx = tap_yx[s_tap];
      const int dy = yx.x, dx = yx.y, c0 = s_blk << 5;
      const int tap_off = (dy * Ws + dx) * p.ldx + c0;
      const bool ch_ok = c0 + kqs * 4 < Kc;
#pragma unroll
      for (int j = 0; j < A_LD; ++j) {
        const int iy = a_iy0[j] + dy, ix = a_ix0[j] + dx;
        const bool ok = ch_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const float* src = ok ? p.x + (a_off[j] + tap_off) : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_ptr)&As[buf][j * 32 + wave * 8][0], 16, 0, 0);
      }
      const float* wrow = p.wp + ((size_t)tap_w[s_tap] * Kc + c0) * p.ldw;
#pragma unroll
      for (int j = 0; j < B_LD; ++j) {
        const bool ok = b_col[j] && c0 + b_row[j] < Kc;
        const float* src = ok ? wrow + b_off[j] : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_ptr)(&Bs[buf][0][0] + (j * 256 + wave * 64) * 4), 16, 0, 0);
      }
      if (++s_tap == ntc) { s_tap = 0; ++s_blk; }
    };
    // Packed taps (Kc < 32): stage s holds taps s * tps .. s * tps + tps - 1; K index k of the stage = (tap k / Kc, channel k % Kc).
    const int ksh = Kc == 4 ? 2 : (Kc == 8 ? 3 : 4);                      // (packed taps exist for Kc = 4, 8, 16 only: shifts, not divisions)
    const int a_sub = (kqs * 4) >> ksh, a_ch = (kqs * 4) - (a_sub << ksh);  // this lane's A slot
    int b_sub[B_LD], b_poff[B_LD];
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
      b_sub[j] = b_row[j] >> ksh;
      b_poff[j] = (b_row[j] - (b_sub[j] << ksh)) * p.ldw + (b_off[j] - b_row[j] * p.ldw);  // (channel row, column) inside the tap's weight block
    }
    // (the stage index is the caller's counter, not a captured variable of its own: two captured counters incremented in sibling
    // branches end as a pointer phi that keeps both in scratch memory -- 12 bytes of private segment on every launch of this kernel)
    auto issue_pack = [&](int buf, int s_stage) {
      const int ta = s_stage * tps + a_sub;
      const bool ta_ok = ta < ntc;
      const int2 yx = tap_yx[ta_ok ? ta : 0];
      const int dy = yx.x, dx = yx.y;
      const int tap_off = (dy * Ws + dx) * p.ldx + a_ch - kqs * 4;  // (a_off carries + kqs * 4)
#pragma unroll
      for (int j = 0; j < A_LD; ++j) {
        const int iy = a_iy0[j] + dy, ix = a_ix0[j] + dx;
        const bool ok = ta_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const float* src = ok ? p.x + (a_off[j] + tap_off) : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_ptr)&As[buf][j * 32 + wave * 8][0], 16, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < B_LD; ++j) {
        const int tb = s_stage * tps + b_sub[j];
        const bool ok = b_col[j] && tb < ntc;
        const float* src = ok ? p.wp + ((size_t)tap_w[ok ? tb : 0] * Kc * p.ldw + b_poff[j]) : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_ptr)(&Bs[buf][0][0] + (j * 256 + wave * 64) * 4), 16, 0, 0);
      }
    };
    auto issue = [&](int buf, int stage) {
      if (p.kfast & 1) issue_fast(buf);
      else if (p.kfast & 4) issue_pack(buf, stage);
      else issue_generic(buf);
    };
    // NS-deep ring: NS - 1 stages are in flight while the MFMA waves work on one, so a stage has (NS - 1) chunk times to land
    // (one 128x128 chunk is 1.7 us of MFMA work, about one loaded-memory latency: with a single stage in flight a workgroup
    // alone on its CU waits at every barrier).  Loads retire in order: waiting for vmcnt <= (stages issued later) * L is
    // waiting for the stage the MFMA waves need next.
    constexpr int L = A_LD + B_LD;  // DMA instructions per lane and stage
    auto landed = [&](int newer) {  // `newer` (uniform): stages issued after the one that has to be in LDS now
      if (NS > 3 && newer >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L) : "memory");
      else if (NS > 2 && newer == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };
    __syncthreads();  // tap tables visible (the MFMA waves' counterpart: in front of their accumulator set-up)
    int issued = c_begin, ibuf = 0;
    for (int s = 0; s < NS - 1 && issued < c_end; ++s) {
      issue(ibuf, issued);
      ibuf = ibuf + 1 == NS ? 0 : ibuf + 1;
      ++issued;
    }
    landed(issued - c_begin - 1);
    for (int c = c_begin; c < c_end; ++c) {
      if (issued < c_end) {  // its buffer held stage c - 1, which the MFMA waves left at the previous barrier
        issue(ibuf, issued);
        ibuf = ibuf + 1 == NS ? 0 : ibuf + 1;
        ++issued;
      }
      landed(issued - c - 2);  // stage c + 1 in LDS (nothing left to wait for after the last one: vmcnt(0) is free)
    }
    return;
  }

  // -------------------------------------------------- MFMA waves --------------------------------------------------
  __syncthreads();  // (pairs with the staging waves' barrier above)
  IGEMM_STAMP(1);
  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int swz = (li >> 1) & 7;  // (row>>1)&7 of every row this lane reads (wave / sub-tile offsets are multiples of 16)
  const float xscale = F16 ? p.f16_xscale : 1.f;
  auto handover = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  auto compute_chunk = [&](int buf) {
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
    for (int kk = 0; kk < 4; ++kk) {
      if (kk + 1 < 4) frag((kk + 1) & 1, kk + 1);
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
      if (kk + 1 < 4) __builtin_amdgcn_sched_group_barrier(0x100, TM + 4 * TN, 0);
      if constexpr (!F16) __builtin_amdgcn_sched_group_barrier(0x008, 4 * TM * TN, 0);
    }
  };
  float4 bias_pre[TN];  // (only the float4 store path reads it: Cout a multiple of 4 -- igemm_bias_prefetch yields zeros otherwise, unused)
  igemm_bias_prefetch<TN, WTN>(p, n0, wn, lane, knz > 1, bias_pre);
  for (int r = t; r < BM; r += 256) {  // rows of the tile -> output pixel offsets (visible to every MFMA wave behind the hand-over barriers)
    const int m = m0 + r;
    int off = -1;
    if (m < Mtot) {
      const int n = (int)fdiv(m, tc.fd_ohw), rem = m - n * OHWq;
      const int qy = (int)fdiv(rem, tc.fd_ow), qx = rem - qy * tc.OWq;
      off = (n * p.OH + qy * p.osy + ooy) * p.OW + qx * p.osx + oox;
    }
    rowoff[r] = off;
  }
  handover();
  IGEMM_STAMP(2);
  {
    int buf = 0;
    for (int c = c_begin; c < c_end; ++c) {
      compute_chunk(buf);
      handover();
      buf = buf + 1 == NS ? 0 : buf + 1;
    }
  }
  IGEMM_STAMP(3);
  if (F16 && xscale != 1.f) {
    const float inv = 1.f / xscale;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] *= inv;
  }
  igemm_store<TM, TN, WTM, WTN>(p, acc, rowoff, wm, wn, li, lh, n0, tc.prow0 + m0, Mtot, knz > 1, slab_off,
                                xpose_scratch<sizeof(As), sizeof(Bs)>(&As[0][0][0], &Bs[0][0][0], wave), bias_pre);
  if (p.ksplit > 1 && p.fold) splitk_fold<BM, BN, 256>(p, rowoff, &s_last, t, n0, tc.prow0 + m0, Mtot, blockIdx.y * grid_x + bid);
#ifdef UDET_EXPERIMENT
  IGEMM_STAMP(4);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  IGEMM_STAMP(5);
#endif
}

}  // namespace udet
