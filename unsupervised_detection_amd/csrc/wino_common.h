// Device helpers shared by the Winograd F(2x2,3x3) kernels: the forward / backward-data forms of conv_wino.hip (four waves, eight waves,
// half size) and, for the row transform and the accumulator layout, the filter gradient of conv_wgrad_wino.hip.  What is here is the same
// in every form: the workgroup decode, the halo DMA table, the two LDS-DMA issue forms, the fragment loads, the transform arithmetic of a
// phase and the store loop.  What differs on purpose -- the order of loads, DMA parts, waits and barriers of a K loop -- stays in the kernels.
// ConvParams travels by reference only (csrc/Makefile: a by-value copy that the optimizer stops following lands in scratch memory).
#pragma once
#include <type_traits>

#include "common.h"
#include "conv_epilogue.h"

namespace udet {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// ---- workgroup decode ----------------------------------------------------------------------------------------------------------------
struct WinoBlock {
  int nb;          // output-channel block
  int d;           // dilation
  int row0, sx;    // pixel (0, 0) of this workgroup's output sub-lattice (sy, sx) of image n: row n * H + sy of the [N * H][W] grid, column sx
  int Hs, Ws;      // this sub-lattice's grid
  int Y0, X0;      // first output pixel (sub-lattice coordinates)
  int kg0, kg1;    // K slice of this workgroup (stages of 8 channels)
};
// BN output channels, TH x TW tiles of 2x2 pixels per workgroup; the grid is [n][sy][sx][by < BY][bx < BX][nb], K slices in blockIdx.z
template <int BN, int TH, int TW>
__device__ __forceinline__ WinoBlock wino_block(const ConvParams& p, int dil, int BY, int BX) {
  WinoBlock b;
  // XCD-aware block order: consecutive blocks (which share input halos) stay on one XCD's L2
  int bid = xcd_tile_order(blockIdx.x, gridDim.x);
  // the N blocks of one tile block are consecutive workgroups of ONE XCD: they read the same input halo out of that XCD's L2
  // (as blockIdx.y they ran a whole grid apart and the halo came from HBM twice: dc_conv21 338 MB fetched for a 140 MB input)
  const int NB = (p.Cout + BN - 1) / BN;
  b.nb = bid % NB;
  bid /= NB;
  const int d = dil;
  b.d = d;
  const int bx = bid % BX;
  int rem = bid / BX;
  const int by = rem % BY;
  rem /= BY;
  b.sx = rem % d;
  rem /= d;
  const int sy = rem % d;
  const int n = rem / d;
  b.row0 = n * p.H + sy;
  b.Hs = (p.H - sy + d - 1) / d;
  b.Ws = (p.W - b.sx + d - 1) / d;
  b.Y0 = by * 2 * TH;
  b.X0 = bx * 2 * TW;
  const int nkg_all = p.Kc >> 3;
  b.kg0 = 0;
  b.kg1 = nkg_all;
  if (p.ksplit > 1) {
    b.kg0 = (int)((long)nkg_all * blockIdx.z / p.ksplit);
    b.kg1 = (int)((long)nkg_all * (blockIdx.z + 1) / p.ksplit);
  }
  return b;
}
// pixel (a, c) of 2x2 tile m of a wave's 4 x 8 tile block whose first pixel is (Yb, Xb) in sub-lattice coordinates: its element offset in
// the [N][H][W] pixel grid (conv_wino_ok: 32-bit offsets), -1 outside the sub-lattice's grid
__device__ __forceinline__ int wino_pixel(const ConvParams& p, const WinoBlock& b, int Yb, int Xb, int m, int a, int c) {
  const int oy = Yb + 2 * (m >> 3) + a, ox = Xb + 2 * (m & 7) + c;
  return (oy >= b.Hs || ox >= b.Ws) ? -1 : (b.row0 + b.d * oy) * p.W + b.sx + b.d * ox;
}

// ---- input halo DMA ------------------------------------------------------------------------------------------------------------------
// Per-lane DMA sources of a wave (constant over the stages up to the channel offset): byte offset from p.x + an EXEC mask of the lanes
// inside the image.  Wave-instruction j = i * 4 + slot covers the 16-byte slots [64 j, 64 j + 64) of an input stage (G::IN_WINSTR of
// them; where that is no multiple of four the last round is partly filled).  The slots of the other lanes (halo beyond the border, row
// padding) are never written: zeroed once, in every ring buffer, by the waves with `zero_fill` -- no address select per DMA, the stage's
// channel offset rides in the scalar base.
template <class G>
__device__ __forceinline__ void wino_halo_table(const ConvParams& p, const WinoBlock& b, char* smem, int slot, int lane, bool zero_fill,
                                                unsigned (&in_voff)[G::IN_INSTR], unsigned long long (&in_mask)[G::IN_INSTR]) {
  constexpr int PH = G::PH, S = G::S, HP = G::HP, CS = G::CS;
#pragma unroll
  for (int i = 0; i < G::IN_INSTR; ++i) {
    const int j = i * 4 + slot;
    const int Lx = j * 64 + lane;
    const int quad = Lx / (PH * S), r2 = Lx - quad * (PH * S);
    const int row = r2 / S, s = r2 - row * S;
    const int par = s / HP, cs = s - par * HP;
    const int col = 2 * cs + par;
    const int yy = b.Y0 - 1 + row, xx = b.X0 - 1 + col;
    const bool in_stage = G::IN_WINSTR % 4 == 0 || j < G::IN_WINSTR;  // (constant-true for the full-size geometries)
    const bool ok = in_stage && quad < 2 && cs < CS && yy >= 0 && yy < b.Hs && xx >= 0 && xx < b.Ws;
    in_voff[i] = ok ? (unsigned)(((b.row0 + b.d * yy) * p.W + b.sx + b.d * xx) * p.ldx + p.x_coff + quad * 4) * 4u : 0u;
    in_mask[i] = __ballot(ok);
    if (!ok && in_stage && zero_fill) {
#pragma unroll
      for (int r = 0; r < G::NS; ++r) *reinterpret_cast<float4*>(smem + r * G::STAGE + Lx * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}
// The DMA is inline assembly on purpose (conv_wino.hip, file comment).  One wave-instruction = 64 lanes x 16 bytes to LDS byte address `lds`:
// masked input slots ...
__device__ __forceinline__ void wino_dma_in(unsigned voff, const float* src, unsigned lds, unsigned long long mask) {
  asm volatile("s_mov_b32 m0, %2\n\ts_mov_b64 exec, %3\n\tglobal_load_lds_dwordx4 %0, %1\n\ts_mov_b64 exec, -1" ::"v"(voff), "s"(src), "s"(lds), "s"(mask)
               : "m0");
}
// ... and 1 KB of transformed weights
__device__ __forceinline__ void wino_dma_w(unsigned voff, const float* src, unsigned lds) {
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(src), "s"(lds) : "m0");
}

// ---- fragments and transforms --------------------------------------------------------------------------------------------------------
// row r of a lane's 4x4 input patch (patch origin a_base inside stage sb): columns 0..3, four channels each
template <class G>
__device__ __forceinline__ void wino_ld_row(const char* sb, int a_base, int r, float4 (&dst)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) dst[c] = *reinterpret_cast<const float4*>(sb + a_base + (r * G::S + (c & 1) * G::HP + (c >> 1)) * 16);
}
// the MFMA B operands of position row i: positions 4 i .. 4 i + 3, four channels each
template <class G>
__device__ __forceinline__ void wino_ld_bf(const char* sb, int b_base, int i, float4 (&dst)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = *reinterpret_cast<const float4*>(sb + b_base + (4 * i + q) * (2 * G::BN * 16));
}
__device__ __forceinline__ float wino_comp(const float4& v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }
// one row of (B^T d) B from the row t of B^T d,  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
__device__ __forceinline__ void wino_bt(const float (&t)[4], float (&v)[4]) {
  v[0] = t[0] - t[2];
  v[1] = t[1] + t[2];
  v[2] = t[2] - t[1];
  v[3] = t[1] - t[3];
}
// tile (or, in the filter gradient, row) of a wave's 32-row block held by accumulator register r of lane half lh (32x32 MFMA C layout)
__device__ __forceinline__ int wino_acc_tile(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// The arithmetic of a stage in the role-split forms (role 0: position rows {1, 2}, role 1: rows {0, 3}): transform + 16 MFMAs per phase.
// Phase 0: role 0 holds patch rows 1, 2 in ra, rb -> row 1 (d1 + d2) now, row 2 (d2 - d1) into v1 for phase 1; role 1 holds rows 0, 2 ->
// row 0 (d0 - d2).
template <int R>
__device__ __forceinline__ void wino_role_phase0(const float4 (&ra)[4], const float4 (&rb)[4], const float4 (&bf0)[4], float (&v1)[4][4], floatx16 (&acc)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t[4], v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float a = wino_comp(ra[c], j), b = wino_comp(rb[c], j);
      t[c] = R == 0 ? a + b : a - b;
    }
    wino_bt(t, v);
    if (R == 0) {
      float u[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) u[c] = wino_comp(rb[c], j) - wino_comp(ra[c], j);
      wino_bt(u, v1[j]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[q], wino_comp(bf0[q], j), acc[q], 0, 0, 0);
  }
}
// Phase 1: role 0 multiplies what phase 0 left in v1; role 1 holds patch rows 1, 3 in rc, rd -> row 3 (d1 - d3).
template <int R>
__device__ __forceinline__ void wino_role_phase1(const float4 (&rc)[4], const float4 (&rd)[4], const float4 (&bf1)[4], const float (&v1)[4][4], floatx16 (&acc)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v[4];
    if (R == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = v1[j][q];
    } else {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = wino_comp(rc[c], j) - wino_comp(rd[c], j);
      wino_bt(t, v);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[4 + q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[q], wino_comp(bf1[q], j), acc[4 + q], 0, 0, 0);
  }
}

// ---- epilogue ------------------------------------------------------------------------------------------------------------------------
// the bias quad of a lane's four output channels, requested in front of the K loop (at the head of the store loop the load is a cold miss
// with nothing to hide behind); zero where the float4 store path will not use it (K slices, ragged channel counts, columns beyond the layer)
__device__ __forceinline__ float4 wino_bias_prefetch(const ConvParams& p, int n4) {
  return (p.ksplit <= 1 && (p.Cout & 3) == 0 && n4 < p.Cout) ? epi4_bias(p, n4) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// QUADS * 8 output pixels x 32 channels of a wave in `src` ([pixel][32 channels], the LDS transpose of the output transform) through the
// epilogue into memory, or into its K slice's slab.  A lane stores QUADS quads: pixel q = k * 8 + lane / 8 (k < QUADS) of its four
// channels n4 ..; pix(q) is that pixel's element offset, or -1 outside the grid.  Plain launches keep FOUR quads in flight per lane (bias
// loaded once, per-pixel operands requested before the first store: conv_epilogue.h, epi4_*): one quad at a time, each iteration waited
// out a global-load latency behind the previous iteration's store -- ~10 us of the 55 us a 16-stage generator layer took.
template <int QUADS, class Pix>
__device__ __forceinline__ void wino_store_quads(const ConvParams& p, const float* src, int lane, int n4, Pix pix, const float4& bias_pre) {
  const bool slab = p.ksplit > 1;
  const bool vec = slab ? ((reinterpret_cast<uintptr_t>(p.partial) & 15) == 0 && (p.ldp & 3) == 0) : epilogue4_out_ok(p);
  const int c4 = (lane & 7) * 4;
  if (!slab && vec) {
    if (n4 >= p.Cout) return;
    const float4 bias = bias_pre;  // (requested in front of the K loop: wino_bias_prefetch)
    const EpiAct ea = epi_act(p);
    auto loop = [&](auto ELU) {  // (the activation is selected HERE, once -- not per element inside the loop: conv_epilogue.h, EpiAct)
      if (epi4_plain(p)) {  // store-only launches: nothing in the loop waits for memory
#pragma unroll 1
        for (int k0 = 0; k0 < QUADS; k0 += 4) {  // four LDS reads in flight, then four stores
          float4 v[4];
          int off[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int q = (k0 + u) * 8 + (lane >> 3);
            v[u] = *reinterpret_cast<const float4*>(&src[q * 32 + c4]);
            off[u] = pix(q);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (off[u] >= 0) epi4_finish_plain32<decltype(ELU)::value>(p, off[u], n4, v[u], bias, ea.slope);
        }
        return;
      }
      // residual / accumulate / dU emission: the operands of EIGHT quads are requested before the first of them is stored (every wait
      // for a load also drains the stores issued before it: once per eight quads instead of once per quad)
#pragma unroll 1
      for (int k0 = 0; k0 < QUADS; k0 += 8) {
        float4 v[8];
        int off[8];
        Epi4Req rq[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int q = (k0 + u) * 8 + (lane >> 3);
          v[u] = *reinterpret_cast<const float4*>(&src[q * 32 + c4]);
          off[u] = pix(q);
          if (off[u] >= 0) epi4_request(p, off[u], n4, rq[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (off[u] >= 0) epi4_finish<decltype(ELU)::value>(p, off[u], n4, v[u], bias, rq[u], ea);
      }
    };
    if (p.act == ACT_ELU) loop(std::true_type());
    else loop(std::false_type());
    return;
  }
  const long slab_off = (long)blockIdx.z * p.N * p.H * p.W * p.ldp;
#pragma unroll 1
  for (int k = 0; k < QUADS; ++k) {
    const int q = k * 8 + (lane >> 3), off = pix(q);
    const float4 v = *reinterpret_cast<const float4*>(&src[q * 32 + c4]);
    if (off < 0) continue;
    if (slab) {
      float* dst = p.partial + (slab_off + (long)off * p.ldp + n4);
      if (vec) {
        if (n4 < p.ldp) *reinterpret_cast<float4*>(dst) = v;
      } else {
        if (n4 < p.ldp) dst[0] = v.x;
        if (n4 + 1 < p.ldp) dst[1] = v.y;
        if (n4 + 2 < p.ldp) dst[2] = v.z;
        if (n4 + 3 < p.ldp) dst[3] = v.w;
      }
      continue;
    }
    if (n4 < p.Cout) conv_epilogue(p, off, n4, v.x);
    if (n4 + 1 < p.Cout) conv_epilogue(p, off, n4 + 1, v.y);
    if (n4 + 2 < p.Cout) conv_epilogue(p, off, n4 + 2, v.z);
    if (n4 + 3 < p.Cout) conv_epilogue(p, off, n4 + 3, v.w);
  }
}
// Output transform + store of the role-split kernels (eight-wave and half-size forms).  acc[0..3] / acc[4..7] = the wave's two position rows
// ({1, 2} role 0, {0, 3} role 1) of a 32-tile x 32-channel wave tile whose first pixel is (Yb, Xb); `area` = 16 KB of LDS shared by the
// tile's two role waves.  Round 6: BOTH roles store -- role 0 computes the upper pixel row of every 2x2 tile, Y0 = s0 + (s1 + s2), role 1
// the lower one, Y1 = (s1 - s2) - s3 (s_i: column sums of position row i): role 0 sends s1 - s2 and receives s0, role 1 the reverse -- half
// the exchange of the earlier form, in which role 1 sent both of its rows and left, and twice the waves on the transposition and the store
// loop (same values, bit for bit).  Every wave of the workgroup must call it (two workgroup barriers inside).
__device__ __forceinline__ void wino_roles_epilogue(const ConvParams& p, const WinoBlock& blk, floatx16 (&acc)[8], float* area, int role, int lane, int n4, int Yb,
                                                    int Xb, const float4& bias_pre) {
  const int li = lane & 31, lh = lane >> 5;
  float* const mine = area + role * 2048;          // [r][b][lane]: what this role sends
  const float* const theirs = area + (1 - role) * 2048;
  float keep[16][2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float s[2][2];  // [own row 0 / 1][b]
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      s[h][0] = acc[h * 4 + 0][r] + acc[h * 4 + 1][r] + acc[h * 4 + 2][r];
      s[h][1] = acc[h * 4 + 1][r] - acc[h * 4 + 2][r] - acc[h * 4 + 3][r];
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      // role 0 (rows 1, 2): keeps s1 + s2, sends s1 - s2; role 1 (rows 0, 3): sends s0, keeps s3
      keep[r][b] = role == 0 ? s[0][b] + s[1][b] : s[1][b];
      mine[(r * 2 + b) * 64 + lane] = role == 0 ? s[0][b] - s[1][b] : s[0][b];
    }
  }
  __syncthreads();
  float y[16][2];
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float o = theirs[(r * 2 + b) * 64 + lane];
      y[r][b] = role == 0 ? o + keep[r][b] : o - keep[r][b];
    }
  __syncthreads();  // (the transposition below overwrites the exchange area)
  float* const tp = area + role * 2048;  // [q = tile * 2 + b][32 channels]: pixel row a = role of the wave tile's 2x2 tiles, 64 pixels
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = wino_acc_tile(r, lh);
#pragma unroll
    for (int b = 0; b < 2; ++b) tp[(m * 2 + b) * 32 + li] = y[r][b];
  }
  __builtin_amdgcn_wave_barrier();  // same wave: LDS serves its instructions in order, only the compiler must not reorder
  wino_store_quads<8>(p, tp, lane, n4, [&](int q) { return wino_pixel(p, blk, Yb, Xb, q >> 1, role, q & 1); }, bias_pre);
}

}  // namespace udet
