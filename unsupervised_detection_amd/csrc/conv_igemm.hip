// Implicit-GEMM convolution on the fp32 matrix cores of gfx950
// (v_mfma_f32_32x32x2_f32: exact f32, 64 FLOP/clk/SIMD).
//
//   M = output pixels (n,qy,qx)   N = output channels   K = (tap, input channel) flattened
//
// 256-thread workgroups (4 wave64), BM x BN output tile.  K is ONE flat axis over the launch's tap list
// (k = tap*Kc + c): a BK-wide LDS stage may straddle taps, so 7x7/5x5 convolutions over 4..16 channels and
// the ragged PWC slab windows run the same BK=32 pipeline as the 128-channel 3x3 layers; the tail of the
// last stage is zero-filled.  Double-buffered LDS, register-staged global->LDS copies (one barrier per stage).
// The A tile is stored K-major in LDS ([BK][BM+pad], pad chosen so that the transposing ds_write_b32 are
// conflict-free) which makes the MFMA A fragment (lane l -> row l&31, k = l>>5) a conflict-free ds_read_b32;
// the B tile ([BK][BN]) is the packed-weight layout itself.
// Stride-2 backward-data / conv2d_transpose: the four output-parity classes are ONE launch (each workgroup
// belongs to one class and walks only that class's taps: no multiplications by structural zeros).
//
// Replaces the TF-1.13 Conv2D / Conv2DBackpropInput kernels the reference calls through
// tf.layers.conv2d / tf.nn.conv2d / tf.layers.conv2d_transpose
// (models/utils/convolution_utils.py:46,81; models/PWCNet/model_pwcnet.py:161-165,286,484-504,562-574).
//
// This file is the host side: the table of tiles, the grid of a launch, launch_conv_gemm and launch_conv_gemm_pair (conv_select.h).
// The kernels live one family per file (conv_igemm_common.h lists them), each behind a launcher that maps the tile to its
// instantiation.  Which configuration a launch runs is decided in conv_select.hip; the autotuner is conv_tune.hip.
#include "conv_igemm_common.h"

namespace udet {

#define UDET_TILE_ROW(BM, BN, WM, WN) {BM, BN},
const int CONV_GEMM_TILES[CONV_GEMM_NTILES][2] = {UDET_GEMM_TILES(UDET_TILE_ROW)};
#undef UDET_TILE_ROW
bool conv_gemm_tile(int bm, int bn) {
  for (auto& t : CONV_GEMM_TILES)
    if (bm == t[0] && bn == t[1]) return true;
  return false;
}

// x-blocks of a launch: M tiles of every class / segment
int conv_xblocks(const ConvParams& p, int bm) {
  if (p.nseg == 0) return p.ncls * ((p.N * p.OHq * p.OWq + bm - 1) / bm);
  int x = 0;
  for (int s = 0; s < p.nseg; ++s) x += (p.N * p.seg[s].h * p.seg[s].w + bm - 1) / bm;
  return x;
}

static int launch_cfg(ConvParams& p, const ConvCfg& c, hipStream_t stream) {
  const int Mtot = p.N * p.OHq * p.OWq;  // (tail split: unsegmented launches only, launch_conv_gemm)
  dim3 grid(conv_xblocks(p, c.bm), (p.Cout + c.bn - 1) / c.bn, p.ksplit > 1 ? p.ksplit : 1);
  if (p.tail_ks > 1) {  // tail split (launch_conv_gemm checked the kernel family, the slab capacity and the alignment)
    const int mtiles = (Mtot + c.bm - 1) / c.bm;
    p.tail_prow0 = (p.tail_full / mtiles) * Mtot + (p.tail_full % mtiles) * c.bm;
    grid.x = p.tail_full + (grid.x - p.tail_full) * p.tail_ks;
    grid.z = 1;
  }
  if (c.family == FAM_SELF_STAGING) UDET_TRY(launch_igemm_self(p, c.bm, c.bn, p.f16 != 0, grid, stream));
  else if (is_lds_dma(c.family)) UDET_TRY(launch_igemm_ring(p, c.bm, c.bn, c.family == FAM_DMA2 ? 2 : (c.family == FAM_DMA3 ? 3 : 4), p.f16 != 0, grid, stream));
  else UDET_TRY(launch_igemm_staged(p, c.bm, c.bn, c.family != FAM_PLAIN, grid, stream));
  if (p.tail_ks > 1) UDET_TRY(launch_splitk_tail_pass(p, stream));
  else if (p.ksplit > 1 && !p.fold) UDET_TRY(launch_splitk_second_pass(p, stream));
  return UDET_OK;
}

static int launch_pair_cfg(ConvParams& a, ConvParams& b, const ConvCfg& c, hipStream_t stream) {
  ConvPair pp;
  pp.p[0] = a; pp.p[1] = b;
  pp.xa = conv_xblocks(a, c.bm);
  dim3 grid(pp.xa + conv_xblocks(b, c.bm), (a.Cout + c.bn - 1) / c.bn, a.ksplit > 1 ? a.ksplit : 1);
  UDET_TRY(launch_igemm_ring_pair(pp, c.bm, c.bn, c.family == FAM_DMA3 ? 3 : 2, grid, stream));
  if (a.ksplit > 1) UDET_TRY(launch_splitk_pair_pass(pp, stream));
  return UDET_OK;
}

int launch_conv_gemm(ConvParams& p, const ConvCfg& c, hipStream_t stream) {
  if (!conv_gemm_tile(c.bm, c.bn)) return no_gemm_tile("conv", c.bm, c.bn);
  p.ksplit = c.ks > 1 ? c.ks : 1;
  p.fold = 0;
  p.tail_full = 0; p.tail_ks = 0; p.tail_prow0 = 0;
  if (p.ksplit > 1) {
    p.ldp = (p.Cout + 3) & ~3;
    p.fold = c.fold && p.tickets && cfg_tiles(p, c.bm, c.bn) <= UDET_MAX_TICKETS;
    const int Mtot = p.N * p.OHq * p.OWq, mtiles = (Mtot + c.bm - 1) / c.bm, xb = p.ncls * mtiles;
    if (c.tail > 0 && c.tail < xb && !p.nseg && is_lds_dma(c.family) && !(reinterpret_cast<uintptr_t>(p.partial) & 15)) {
      const long prow0 = (long)(c.tail / mtiles) * Mtot + (long)(c.tail % mtiles) * c.bm;
      if ((size_t)((long)p.ncls * Mtot - prow0) * p.ldp * p.ksplit <= p.partial_cap) {
        p.tail_full = c.tail; p.tail_ks = p.ksplit; p.ksplit = 1; p.fold = 0;
      }
    }
  }
  return launch_cfg(p, c, stream);
}

int launch_conv_gemm_pair(ConvParams& a, ConvParams& b, const ConvCfg& c, hipStream_t stream) {
  if (!conv_gemm_tile(c.bm, c.bn)) return no_gemm_tile("conv pair", c.bm, c.bn);
  const int cap = pair_max_ksplit(a, b);
  const int ks = c.ks > cap ? cap : (c.ks < 1 ? 1 : c.ks);
  for (ConvParams* q : {&a, &b}) {
    q->ksplit = ks; q->fold = 0; q->tail_full = 0; q->tail_ks = 0; q->tail_prow0 = 0;
    q->ldp = (q->Cout + 3) & ~3;
  }
  float* const base = a.partial;
  if (ks > 1) {
    if ((reinterpret_cast<uintptr_t>(base) & 15) != 0) { set_error("conv pair: unaligned split-K scratch"); return UDET_ERR_ALIGN; }
    size_t off = (size_t)ks * a.Mall * a.ldp;
    off = (off + 15) & ~(size_t)15;
    b.partial = base + off;
  }
  const int rc = launch_pair_cfg(a, b, c, stream);
  b.partial = base;
  return rc;
}

}  // namespace udet
