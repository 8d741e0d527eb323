// Internal: what the implicit-GEMM kernel families share -- the flat-K cursor, the decode of an x-block and of its rows, the tile
// store, the split-K sums -- and the interface between them and the host side in conv_igemm.hip:
//   conv_igemm_staged.hip  conv_igemm_kernel (register-staged, plain and wave-specialised),
//   conv_igemm_ring.hip    conv_igemm_dma_kernel; conv_igemm_ring_pair.hip: conv_igemm_dma_pair_kernel (LDS-DMA ring; body: conv_igemm_ring.h),
//   conv_igemm_self.hip    conv_igemm_dma4_kernel (self-staging LDS-DMA; conv_igemm_dma.h),
//   conv_splitk.hip        the second-pass kernels of split-K launches.
#pragma once
#include "common.h"
#include "conv_epilogue.h"
#include "conv_select.h"

namespace udet {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));

// libudet_exp.so only (tools/igemm_stamps.py): per-workgroup cycle stamps of the LDS-DMA ring kernel -- 0 entry, 1 tables done, 2 first stage
// landed, 3 K loop done, 4 tile stored (issued), 5 stores acknowledged, 6 / 7 block decoded / tables written, 8 / 9 inside the tile store
// (its set-up done / first half block issued; IGEMM_STAMP_B: the x-block index is blockIdx.x -- single launches only).
// The stamp buffer and IGEMM_STAMP_AT are defined by conv_igemm_ring.hip in front of this header (device code is linked per file: a
// buffer declared here could not be shared between the families' files); everywhere else the stamps are compiled out.
#ifdef IGEMM_STAMP_AT
#define IGEMM_STAMP(i) IGEMM_STAMP_AT(bid_x, i)
#define IGEMM_STAMP_B(i) IGEMM_STAMP_AT((int)blockIdx.x, i)
#else
#define IGEMM_STAMP(i) do {} while (0)
#define IGEMM_STAMP_B(i) do {} while (0)
#endif

// ---- the instantiated tiles: the one map from a (bm, bn) pair to a template instantiation ---------------------------------------
// X(BM, BN, WAVES_M, WAVES_N), in the order the tuners scan them
#define UDET_GEMM_TILES(X) X(256, 32, 4, 1) X(128, 32, 4, 1) X(128, 64, 2, 2) X(64, 64, 2, 2) X(128, 96, 4, 1) X(128, 128, 2, 2)

// Flat-K cursor.  K runs channel-block-major: for every block of CB = min(Kc,32) input channels all taps of the launch,
// then the next channel block (the last block may be narrower).  A workgroup therefore re-visits its ~3 input rows
// for all taps of one channel block while they are still in L1/L2, instead of streaming the whole channel depth once
// per tap (9x the algorithmic read traffic out of L2 for a 3x3 layer over 568 channels).
struct KCursor {
  int blk, tap, c, w;
};
struct KOrder {
  int Kc, CB, nblk, wl, ntc;
};
__device__ __forceinline__ KOrder korder(int Kc, int ntc) {
  KOrder o;
  o.Kc = Kc; o.ntc = ntc;
  o.CB = Kc < 32 ? Kc : 32;
  o.nblk = Kc < 32 ? 1 : (Kc + 31) >> 5;  // (= ceil(Kc / CB) without a run-time division)
  o.wl = Kc - (o.nblk - 1) * o.CB;
  return o;
}
__device__ __forceinline__ KCursor kc_init(const KOrder& o, int kf) {
  KCursor k;
  const int per = o.ntc * o.CB;
  int blk = per > 0 ? kf / per : o.nblk;
  if (blk >= o.nblk - 1) {
    const int rem = kf - (o.nblk - 1) * per;
    k.blk = o.nblk - 1; k.w = o.wl;
    k.tap = rem / o.wl; k.c = rem - k.tap * o.wl;
    if (k.tap >= o.ntc) { k.blk = o.nblk; k.tap = 0; }
  } else {
    const int rem = kf - blk * per;
    k.blk = blk; k.w = o.CB;
    k.tap = rem / o.CB; k.c = rem - k.tap * o.CB;
  }
  return k;
}
__device__ __forceinline__ void kc_advance(const KOrder& o, KCursor& k, int step) {
  if (k.w == step) {  // common case (32-channel block, 32-wide stage): same channel offset, next tap
    if (++k.tap == o.ntc) {
      k.tap = 0;
      ++k.blk;
      k.w = k.blk == o.nblk - 1 ? o.wl : o.CB;
    }
  } else {
    k.c += step;
  }
  while (k.c >= k.w) {  // (also re-normalises the offset after stepping into the narrower last block)
    k.c -= k.w;
    if (++k.tap == o.ntc) {
      k.tap = 0;
      ++k.blk;
      k.w = k.blk == o.nblk - 1 ? o.wl : o.CB;
    }
  }
}
__device__ __forceinline__ bool kc_valid(const KOrder& o, const KCursor& k) { return k.blk < o.nblk; }
__device__ __forceinline__ int kc_chan(const KOrder& o, const KCursor& k) { return k.blk * o.CB + k.c; }

// per-wave LDS scratch of the transposing store below: 16 rows x UDET_XP floats, carved out of the (now idle) stage buffers
#define UDET_XP 40
template <size_t SA, size_t SB>
__device__ __forceinline__ float* xpose_scratch(float* a, float* b, int wave) {
  constexpr size_t W = 16 * UDET_XP * sizeof(float);
  if constexpr (SA >= 4 * W) return a + wave * 16 * UDET_XP;
  else if constexpr (SB >= 4 * W) return b + wave * 16 * UDET_XP;
  else if constexpr (SA >= 2 * W && SB >= 2 * W) return (wave < 2 ? a : b) + (wave & 1) * 16 * UDET_XP;
  else return nullptr;
}

// The class (or segment, ConvParams::nseg) an x-block belongs to and that block's place in it
struct TileCls {
  int cls, m0, Mtot, OHWq, OWq, ooy, oox, tap0, ntc, prow0;
  FastDiv fd_ohw, fd_ow;
};
template <int BM>
__device__ __forceinline__ TileCls tile_cls(const ConvParams& p, int bid) {
  TileCls t;
  if (p.nseg == 0) {
    t.OHWq = p.OHq * p.OWq; t.OWq = p.OWq;
    t.Mtot = p.N * t.OHWq;
    const int mtiles = (t.Mtot + BM - 1) / BM;
    t.cls = p.ncls > 1 ? bid / mtiles : 0;  // (one class: no run-time division in front of every launch's first instruction of work)
    t.m0 = (bid - t.cls * mtiles) * BM;
    t.tap0 = p.cls_tap[t.cls];
    t.ntc = p.cls_tap[t.cls + 1] - t.tap0;
    t.ooy = p.ncls > 1 ? (t.cls >> 1) : p.ooy; t.oox = p.ncls > 1 ? (t.cls & 1) : p.oox;
    t.prow0 = t.cls * t.Mtot;
    t.fd_ohw = p.fd_ohw; t.fd_ow = p.fd_ow;
    return t;
  }
  int s = 0, b = bid;
  for (; s < p.nseg - 1; ++s) {
    const int mt = (p.N * p.seg[s].h * p.seg[s].w + BM - 1) / BM;
    if (b < mt) break;
    b -= mt;
  }
  const ConvSeg& g = p.seg[s];
  t.cls = s;
  t.OHWq = g.h * g.w; t.OWq = g.w;
  t.Mtot = p.N * t.OHWq;
  t.m0 = b * BM;
  t.tap0 = p.seg_tap[s];
  t.ntc = p.seg_tap[s + 1] - t.tap0;
  t.ooy = g.oy; t.oox = g.ox;
  t.prow0 = g.prow0;
  t.fd_ohw = g.fd_hw; t.fd_ow = g.fd_w;
  return t;
}
__device__ __forceinline__ ConvTap conv_tap(const ConvParams& p, int i) { return p.nseg ? p.tap_tab[i] : p.taps[i]; }
template <int NT>  // the tap tables of an x-block, by the NT threads of its workgroup
__device__ __forceinline__ void fill_tap_tables(const ConvParams& p, const TileCls& tc, int2* tap_yx, int* tap_w, int tid) {
  for (int i = tid; i < tc.ntc; i += NT) {
    const ConvTap tp = conv_tap(p, tc.tap0 + i);
    tap_yx[i] = make_int2(tp.dy, tp.dx);
    tap_w[i] = tp.widx;
  }
}

// Row m of a sub-grid of OHWq = OHq x OWq pixels per image -> (image, sub-grid row, sub-grid column)
__device__ __forceinline__ void row_decode(int m, int OHWq, int OWq, const FastDiv& fd_ohw, const FastDiv& fd_ow, int& n, int& qy, int& qx) {
  n = (int)fdiv(m, fd_ohw);
  const int rem = m - n * OHWq;
  qy = (int)fdiv(rem, fd_ow);
  qx = rem - qy * OWq;
}
// ... -> the offset of its output pixel (sub-grid origin (ooy, oox), strides osy / osx)
__device__ __forceinline__ int row_out_off(const ConvParams& p, int m, int OHWq, int OWq, const FastDiv& fd_ohw, const FastDiv& fd_ow, int ooy, int oox) {
  int n, qy, qx;
  row_decode(m, OHWq, OWq, fd_ohw, fd_ow, n, qy, qx);
  return (n * p.OH + qy * p.osy + ooy) * p.OW + qx * p.osx + oox;
}
// row m of an x-block's class / segment: its output pixel offset, -1 past the last row
__device__ __forceinline__ int row_out_off(const ConvParams& p, const TileCls& tc, int m) {
  return m < tc.Mtot ? row_out_off(p, m, tc.OHWq, tc.OWq, tc.fd_ohw, tc.fd_ow, tc.ooy, tc.oox) : -1;
}
template <int BM, int NT>  // rows of the tile -> output pixel offsets, by NT threads
__device__ __forceinline__ void fill_rowoff(const ConvParams& p, const TileCls& tc, int* rowoff, int tid) {
  for (int r = tid; r < BM; r += NT) rowoff[r] = row_out_off(p, tc, tc.m0 + r);
}
// ... the A operand's view of the row: image base (in pixels of the Hs x Ws source) and the input position of tap (0, 0); rows past the
// last fail every bounds test (iy0 = -2^28)
__device__ __forceinline__ void row_a_origin(const ConvParams& p, const TileCls& tc, int m, int Hs, int Ws, int& a_base, int& a_iy0, int& a_ix0) {
  a_base = 0;
  a_iy0 = -(1 << 28);
  a_ix0 = 0;
  if (m < tc.Mtot) {
    int n, qy, qx;
    row_decode(m, tc.OHWq, tc.OWq, tc.fd_ohw, tc.fd_ow, n, qy, qx);
    a_base = n * Hs * Ws;
    a_iy0 = qy * p.isy;
    a_ix0 = qx * p.isx;
  }
}
// the chunks [c_begin, c_end) of K slice kz of knz
__device__ __forceinline__ void k_slice(int nchunks, int kz, int knz, int& c_begin, int& c_end) {
  c_begin = 0;
  c_end = nchunks;
  if (knz > 1) {
    c_begin = (int)((unsigned)(nchunks * kz) / (unsigned)knz);  // (nchunks * knz < 2^31: 32-bit divisions, a third of the 64-bit ones' instructions)
    c_end = (int)((unsigned)(nchunks * (kz + 1)) / (unsigned)knz);
  }
}
template <int TM, int TN>
__device__ __forceinline__ void acc_zero(floatx16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
template <int TM, int TN>  // fp16 operands were multiplied by xscale on the way in
__device__ __forceinline__ void acc_unscale(floatx16 (&acc)[TM][TN], float xscale) {
  if (xscale == 1.f) return;
  const float inv = 1.f / xscale;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] *= inv;
}

// output pixel offset of row `ma` of the launch's flat row space (split-K second pass)
__device__ __forceinline__ int row_pixel_off(const ConvParams& p, int ma) {
  int m, OHWq, OWq, ooy, oox;
  FastDiv fa, fb;
  if (p.nseg == 0) {
    OHWq = p.OHq * p.OWq; OWq = p.OWq;
    const int Mtot = p.N * OHWq, cls = ma / Mtot;
    m = ma - cls * Mtot;
    ooy = p.ncls > 1 ? (cls >> 1) : p.ooy; oox = p.ncls > 1 ? (cls & 1) : p.oox;
    fa = p.fd_ohw; fb = p.fd_ow;
  } else {
    int s = 0;
    while (s < p.nseg - 1 && ma >= p.seg[s + 1].prow0) ++s;
    const ConvSeg& g = p.seg[s];
    m = ma - g.prow0;
    OHWq = g.h * g.w; OWq = g.w; ooy = g.oy; oox = g.ox;
    fa = g.fd_hw; fb = g.fd_w;
  }
  return row_out_off(p, m, OHWq, OWq, fa, fb, ooy, oox);
}

// Result of one workgroup: plain launches run the epilogue; split-K launches store the partial tile into slab blockIdx.z
// (row index = parity class * Mtot + pixel).
// The MFMA accumulator holds COLUMN n = lane of 8+8 rows, so a direct store is one dword per lane and (bias, activation, 64-bit
// address, flag tests) once per element -- ~13,000 instructions for a 128x128 tile, more than the instruction cache holds, and
// ~15 % of the run time of a mid-size layer.  With `xp` (16 x UDET_XP floats of LDS per wave) the tile goes through LDS half a
// 32x32 block at a time and leaves as float4 rows: 8 lanes x 16 B per pixel, epilogue arithmetic once per quad, and the
// store loop is not unrolled (4 x 2 copies of its body instead of 256).
// the float4 path of igemm_store for one (activation, operand) variant: a plain function template, NOT a lambda inside igemm_store --
// with a generic lambda instantiated four ways hipcc copied the whole 1752-byte kernel-argument block to scratch in every kernel with a
// tile larger than 64 x 64 (1760 bytes of scratch per lane; round 6)
template <int TM, int TN, int WTM, int WTN, bool ELU, bool PLAIN>
__device__ __forceinline__ void igemm_store_quads(const ConvParams& p, floatx16 (&acc)[TM][TN], const int* rowoff, int wm, int wn, int li, int lh, int n0,
                                                  int prow0, bool slab, long slab_off, float* xp, const float4* bias_pre) {
  const int lane = lh * 32 + li, rr = lane >> 3, c4 = (lane & 7) * 4;
  // the bias quad of a column block does not depend on the row: loaded once per block, not once per quad behind the previous quad's
  // store; the two passes of a half block request their per-pixel operands together; the activation is selected once, by the caller
  // (conv_epilogue.h: epi4_*, EpiAct -- per element it cost five scalar branches).  PLAIN: a launch with neither residual nor accumulate
  // nor dU emission -- or a K slice writing its slab -- has NO global load in its store loop; with one, every wait for it also drains the
  // stores issued before it (loads and stores share vmcnt on gfx950)
  float4 bias[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + wn * WTN + j * 32 + c4;
    if (bias_pre) bias[j] = bias_pre[j];  // (requested in front of the K loop: igemm_bias_prefetch)
    else bias[j] = (!slab && nb < p.Cout) ? epi4_bias(p, nb) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const EpiAct ea = epi_act(p);
  IGEMM_STAMP_B(8);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nb = n0 + wn * WTN + j * 32 + c4;
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // accumulator registers 8h .. 8h+7 are rows 16h .. 16h+15 of the block
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) xp[((r & 3) + 8 * (r >> 2) + 4 * lh) * UDET_XP + li] = acc[i][j][8 * h + r];
        __builtin_amdgcn_wave_barrier();  // same wave: LDS serves its instructions in order, only the compiler must not reorder
        int off[2];
        float4 v[2];
        Epi4Req rq[2];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int row = wm * WTM + i * 32 + h * 16 + pass * 8 + rr;
          off[pass] = rowoff[row];
          v[pass] = *reinterpret_cast<const float4*>(&xp[(pass * 8 + rr) * UDET_XP + c4]);
          if (!PLAIN && !slab && off[pass] >= 0 && nb < p.Cout) epi4_request(p, off[pass], nb, rq[pass]);
        }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int row = wm * WTM + i * 32 + h * 16 + pass * 8 + rr;
          if (off[pass] < 0) continue;
          if (slab) {
            if (nb < p.ldp) *reinterpret_cast<float4*>(p.partial + (slab_off + (long)(prow0 + row) * p.ldp + nb)) = v[pass];
          } else if (nb < p.Cout) {
            if (PLAIN) epi4_finish_plain<ELU>(p, off[pass], nb, v[pass], bias[j], ea.slope);
            else epi4_finish<ELU>(p, off[pass], nb, v[pass], bias[j], rq[pass], ea);
          }
        }
        if (i == 0 && j == 0 && h == 0) IGEMM_STAMP_B(9);
      }
    }
  }
}
// the bias quads of a wave's column blocks, requested in front of the K loop (the quad of the float4 store path: lane & 7): at the head of
// the tile store the same load is a cold miss of ~1 000-2 000 cycles with nothing to hide behind.  Zero for K slices (the second pass adds
// the bias) and for columns beyond the layer.
template <int TN, int WTN>
__device__ __forceinline__ void igemm_bias_prefetch(const ConvParams& p, int n0, int wn, int lane, bool slab, float4 (&bias)[TN]) {
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + wn * WTN + j * 32 + (lane & 7) * 4;
    bias[j] = (!slab && p.bias && nb + 3 < ((p.Cout + 3) & ~3) && (p.Cout & 3) == 0 && nb < p.Cout) ? epi4_bias(p, nb) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void igemm_store(const ConvParams& p, floatx16 (&acc)[TM][TN], const int* rowoff, int wm, int wn, int li,
                                            int lh, int n0, int prow0, int Mtot, bool slab, long slab_off, float* xp = nullptr,
                                            const float4* bias_pre = nullptr) {
  // slab: this workgroup holds a K slice; its partial tile goes to p.partial + slab_off + (class row) * ldp
  if (xp != nullptr && !(slab && p.fold) && (slab ? (reinterpret_cast<uintptr_t>(p.partial) & 15) == 0 : epilogue4_out_ok(p))) {
    const bool plain = slab || epi4_plain(p);
    if (!slab && p.act == ACT_ELU) {
      if (plain) igemm_store_quads<TM, TN, WTM, WTN, true, true>(p, acc, rowoff, wm, wn, li, lh, n0, prow0, slab, slab_off, xp, bias_pre);
      else igemm_store_quads<TM, TN, WTM, WTN, true, false>(p, acc, rowoff, wm, wn, li, lh, n0, prow0, slab, slab_off, xp, bias_pre);
    } else {
      if (plain) igemm_store_quads<TM, TN, WTM, WTN, false, true>(p, acc, rowoff, wm, wn, li, lh, n0, prow0, slab, slab_off, xp, bias_pre);
      else igemm_store_quads<TM, TN, WTM, WTN, false, false>(p, acc, rowoff, wm, wn, li, lh, n0, prow0, slab, slab_off, xp, bias_pre);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int off = rowoff[row];
      if (off < 0) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * 32 + li;
        const float v = acc[i][j][r];
        if (slab) {
          if (n < p.ldp) {
            float* dst = p.partial + (slab_off + (long)(prow0 + row) * p.ldp + n);
            // folded form: the slab is published write-through (device-scope store, `sc1`): it is in memory when the store is
            // acknowledged, so no L2 write-back fence is needed before the ticket (MI355X_MICROARCH.md "publish-large")
            if (p.fold) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else *dst = v;
          }
          continue;
        }
        if (n >= p.Cout) continue;
        conv_epilogue(p, off, n, v);
      }
    }
  }
}

// Split-K without a second launch: every workgroup publishes its partial tile write-through (igemm_store), drains its
// stores, and one lane draws a ticket; the workgroup that draws the last sums the slabs IN SPLIT ORDER (the result does not
// depend on which workgroup arrives last) with device-scope (`sc1`) loads -- they read memory, not a stale line of this XCD's
// L2, which is not coherent with the L2s the other workgroups wrote through -- and runs the epilogue, then resets the ticket
// for the next launch on this stream.  No release / acquire fences: a fence writes back / invalidates the whole L2 and cost
// more than the launch it replaces (r2a: the folded form with __threadfence() lost on every one of 141 split shapes).
// Called by the NT threads [0, NT) of the workgroup that are still alive (the staging waves of the wave-specialised kernels
// have exited: s_barrier counts surviving waves only).
__device__ __forceinline__ float4 load4_device_scope(const float* p) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_float4(__uint_as_float((unsigned)a), __uint_as_float((unsigned)(a >> 32)), __uint_as_float((unsigned)b),
                     __uint_as_float((unsigned)(b >> 32)));
}
__device__ __forceinline__ float4 load4_plain(const float* p) { return *reinterpret_cast<const float4*>(p); }
// the sum of one quad over `ksplit` slabs `slab` floats apart: four slabs in flight per trip (the loads are independent; a plain loop waits
// for each before the next add), added IN SPLIT ORDER -- per element the same chain of additions as a plain loop over the slabs
template <float4 (*LOAD)(const float*)>
__device__ __forceinline__ float4 splitk_sum4(const float* src, size_t slab, int ksplit) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  int s = 0;
  for (; s + 3 < ksplit; s += 4) {
    const float4 a0 = LOAD(src + (size_t)s * slab);
    const float4 a1 = LOAD(src + (size_t)(s + 1) * slab);
    const float4 a2 = LOAD(src + (size_t)(s + 2) * slab);
    const float4 a3 = LOAD(src + (size_t)(s + 3) * slab);
    v.x += a0.x; v.y += a0.y; v.z += a0.z; v.w += a0.w;
    v.x += a1.x; v.y += a1.y; v.z += a1.z; v.w += a1.w;
    v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w;
    v.x += a3.x; v.y += a3.y; v.z += a3.z; v.w += a3.w;
  }
  for (; s < ksplit; ++s) {
    const float4 a0 = LOAD(src + (size_t)s * slab);
    v.x += a0.x; v.y += a0.y; v.z += a0.z; v.w += a0.w;
  }
  return v;
}
template <int BM, int BN, int NT>
__device__ __forceinline__ void splitk_fold(const ConvParams& p, const int* rowoff, int* s_last, int t, int n0, int prow0, int Mtot,
                                            int tile_id) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's slab stores are acknowledged (write-through: in memory)
  __syncthreads();
  if (t == 0) *s_last = atomicAdd(p.tickets + tile_id, 1) == p.ksplit - 1;
  __syncthreads();
  if (!*s_last) return;
  constexpr int C4 = BN / 4, ROWS = NT / C4;
  const int c4 = t % C4, n = n0 + c4 * 4;
  const size_t slab = (size_t)p.Mall * p.ldp;
  if (n < p.ldp && t < ROWS * C4) {  // (BN = 96: 240 of the 256 threads tile the [ROWS][C4] grid exactly)
    for (int row = t / C4; row < BM; row += ROWS) {
      const int off = rowoff[row];
      if (off < 0) continue;
      const float* src = p.partial + (size_t)(prow0 + row) * p.ldp + n;
      const float4 v = splitk_sum4<load4_device_scope>(src, slab, p.ksplit);
      if (n < p.Cout) conv_epilogue(p, off, n, v.x);
      if (n + 1 < p.Cout) conv_epilogue(p, off, n + 1, v.y);
      if (n + 2 < p.Cout) conv_epilogue(p, off, n + 2, v.z);
      if (n + 3 < p.Cout) conv_epilogue(p, off, n + 3, v.w);
    }
  }
  if (t == 0) p.tickets[tile_id] = 0;
}
// Two problems in ONE launch ("pair launch", round 6): same tile configuration, same N blocks and K slices, independent operands --
// x-blocks [0, xa) belong to problem 0, the rest to problem 1.  The recover net's two encoders (nets.py:57-75: aconv_k / bconv_k, same
// geometry per level, separate weights, different batch) and their backward-data passes run this way: each of those launches fills a
// fraction of the chip and costs a launch boundary, two of them side by side cost hardly more than the larger one.  The parameter
// blocks stay in the kernel-argument segment (2 x 1752 bytes of the 4 KB): the workgroup picks its block with one scalar select.
struct ConvPair {
  ConvParams p[2];
  int xa;
};
static_assert(sizeof(ConvPair) <= 4000, "kernel-argument segment");

// ---- the families' launchers: each maps a tile of UDET_GEMM_TILES to its instantiation (an error for a tile the family lacks) ------
// (conv_igemm.hip computes the grid; ns: stages of the ring -- requests the kernels are not instantiated for run the 3-stage ring)
int launch_igemm_staged(const ConvParams& p, int bm, int bn, bool wave_spec, dim3 grid, hipStream_t stream);
int launch_igemm_ring(const ConvParams& p, int bm, int bn, int ns, bool f16, dim3 grid, hipStream_t stream);
int launch_igemm_ring_pair(const ConvPair& pp, int bm, int bn, int ns, dim3 grid, hipStream_t stream);
int launch_igemm_self(const ConvParams& p, int bm, int bn, bool f16, dim3 grid, hipStream_t stream);
int launch_splitk_tail_pass(const ConvParams& p, hipStream_t stream);                           // the slabs of a tail split (rows >= tail_prow0)
int launch_splitk_pair_pass(ConvPair& pp, hipStream_t stream);                                  // both problems' slabs of a pair launch
inline int no_gemm_tile(const char* what, int bm, int bn) {
  set_error("%s: no kernel for tile %dx%d", what, bm, bn);
  return UDET_ERR_UNSUPPORTED;
}

}  // namespace udet
