// Which kernel family and configuration a forward / backward-data convolution launch runs: argument checks, the built-in
// heuristics, the debug forcing of include/udet_debug.h, the ONE validation of a configuration against a launch (runnable_cfg),
// and the launchers launch_conv / launch_conv_pair.  The families are listed in conv_select.h; the kernels live in conv_igemm_*.hip,
// conv_tile.hip, conv_thin.hip and conv_wino.hip; the autotuner that fills the caches is conv_tune.hip.
#include <mutex>

#include "common.h"
#include "conv_select.h"

namespace udet {

struct TileGeoms;
size_t conv_tile_lds_bytes(const ConvParams& p, int th, int cbmax, TileGeoms* gout, bool* big);
int launch_conv_tile(const ConvParams& p, int th, int cbmax, hipStream_t stream);

// ---- what a launch can take ----------------------------------------------------------------------------------------------------
static int max_class_taps(const ConvParams& p) {
  int mx = 0;
  for (int c = 0; c < p.nseg; ++c) mx = p.seg_tap[c + 1] - p.seg_tap[c] > mx ? p.seg_tap[c + 1] - p.seg_tap[c] : mx;
  if (p.nseg) return mx;
  for (int c = 0; c < p.ncls; ++c) mx = p.cls_tap[c + 1] - p.cls_tap[c] > mx ? p.cls_tap[c + 1] - p.cls_tap[c] : mx;
  return mx;
}
// split count the K depth and `floats_per_split` of slab leave room for
static int ksplit_capacity(const ConvParams& p, size_t floats_per_split) {
  const int nchunks = (max_class_taps(p) * p.Kc + 31) / 32;
  int ks = nchunks / 2 > 64 ? 64 : nchunks / 2;
  while (ks > 1 && floats_per_split * ks > p.partial_cap) --ks;
  return ks < 1 ? 1 : ks;
}
int max_ksplit(const ConvParams& p) { return p.partial ? ksplit_capacity(p, (size_t)p.Mall * ((p.Cout + 3) & ~3)) : 1; }
int pair_max_ksplit(const ConvParams& a, const ConvParams& b) { return ksplit_capacity(a, ((size_t)a.Mall + b.Mall) * ((a.Cout + 3) & ~3) + 64); }
bool tile_ok(const ConvParams& p, int th, int cb) {
  if (p.nseg) return false;  // segmented launches: implicit-GEMM families only
  if (cb == 16 && p.Kc <= 16) return false;  // (the same launch as cb = 32)
  const size_t b = conv_tile_lds_bytes(p, th, cb, nullptr, nullptr);
  // (<= 256 columns: the kernel walks 32-column blocks as blockIdx.y and re-reads the halo per block -- thin inputs with wide outputs,
  // the backward-data view of the recover decoder: 32 -> 194 channels 163 -> 150 us; beyond that the implicit GEMM always won)
  return b > 0 && b <= 96 * 1024 && p.Kc <= 256 && p.Cout <= 256;
}
bool dma_ok(const ConvParams& p) { return p.xa == nullptr && p.zero16 != nullptr && !(reinterpret_cast<uintptr_t>(p.zero16) & 15); }
// tail split for workgroups filling r slots per CU: x-blocks of the whole rounds stay unsplit (*full_x of them), the rest is cut
// into *ks slices so that it fills one more round.  false: the tile count is a whole number of rounds, or less than one.
bool tail_for_rounds(const ConvParams& p, int bm, int bn, int r, int kcap, int* full_x, int* ks) {
  if (p.nseg) return false;
  const int Mtot = p.N * p.OHq * p.OWq, X = p.ncls * ((Mtot + bm - 1) / bm), Y = (p.Cout + bn - 1) / bn;
  const long S = 256L * r, T = (long)X * Y, fullT = T / S * S;
  if (fullT == 0 || fullT == T) return false;
  const int fx = (int)(fullT / Y), rem_x = X - fx;
  if (fx <= 0 || rem_x <= 0) return false;
  long k = S / ((long)rem_x * Y);
  if (k > kcap) k = kcap;
  if (k < 2) return false;
  *full_x = fx;
  *ks = (int)k;
  return true;
}

// ---- the built-in choice -------------------------------------------------------------------------------------------------------
// split count of an untuned launch of `tiles` < 256 output tiles: towards two rounds of the CUs, keeping >= 4 stages per split
static int heuristic_ksplit(long tiles, int cap) {
  const int ks = (int)((512 + tiles - 1) / tiles), half = cap / 2 > 0 ? cap / 2 : 1;
  return ks > half ? half : ks;
}
ConvCfg heuristic_cfg(const ConvParams& p) {
  // N tile from the channel count; M tile shrunk while the launch would leave CUs without a workgroup
  ConvCfg c;
  c.family = FAM_WAVE_SPEC; c.tail = 0;
  if (p.Cout <= 32) { c.bn = 32; c.bm = 256; if (cfg_tiles(p, 256, 32) < 384) c.bm = 128; }
  else if (p.Cout <= 64) { c.bn = 64; c.bm = 128; if (cfg_tiles(p, 128, 64) < 384) c.bm = 64; }
  else if (p.Cout <= 96) { c.bn = 96; c.bm = 128; }
  else { c.bn = 128; c.bm = 128; if (cfg_tiles(p, 128, 128) < 320) { c.bn = 64; if (cfg_tiles(p, 128, 64) < 384) c.bm = 64; } }
  const long tiles = cfg_tiles(p, c.bm, c.bn);
  c.ks = tiles < 256 ? heuristic_ksplit(tiles, max_ksplit(p)) : 1;
  c.fold = 0;  // measured (r2a): the release / acquire of the folded form costs more than the second launch on almost every shape;
               // the tuner still tries it for its winner
  if (p.f16 && dma_ok(p)) c.family = FAM_DMA2;  // fp16 multiplication exists in the LDS-DMA families only
  return c;
}
static ConvCfg pair_heuristic(const ConvParams& a, const ConvParams& b) {
  ConvCfg c = heuristic_cfg(b.Mall >= a.Mall ? b : a);
  c.family = FAM_DMA2; c.fold = 0; c.tail = 0;
  const long tiles = cfg_tiles(a, c.bm, c.bn) + cfg_tiles(b, c.bm, c.bn);
  c.ks = tiles < 256 ? heuristic_ksplit(tiles, pair_max_ksplit(a, b)) : 1;
  return c;
}

int run_conv_cfg(ConvParams& p, const ConvCfg& c, hipStream_t stream) {
  if (is_direct(c.family)) {
    p.ksplit = 1; p.fold = 0; p.tail_full = 0; p.tail_ks = 0;
    return c.family == FAM_THIN_K ? launch_conv_thin_k(p, stream) : launch_conv_thin_n(p, stream);
  }
  if (c.family == FAM_WINO) return launch_conv_wino(p, c.wino_variant(), c.ks, stream);
  if (c.family == FAM_TILE) {
    p.ksplit = 1;
    p.fold = 0;
    return launch_conv_tile(p, c.tile_height(), c.tile_channels(), stream);
  }
  return launch_conv_gemm(p, c, stream);
}

// ---- the one answer to "may this configuration run on this launch?" -------------------------------------------------------------
// c may come from the tuner, a tuning file (udet_tune_load) or the debug hook: never trust it beyond what the launcher would choose
// itself.  Returns the configuration that runs.
static ConvCfg runnable_cfg(const ConvParams& p, ConvCfg c) {
  // only instantiated tiles / known families / variants
  const bool known = c.family == FAM_TILE ? (c.bm == 4 || c.bm == 8) && (c.bn == 16 || c.bn == 32)
                     : c.family == FAM_WINO ? c.bm >= 0 && c.bm <= 4
                     : is_direct(c.family) || (is_gemm(c.family) && conv_gemm_tile(c.bm, c.bn));  // (the direct kernels carry no tile)
  if (!known) return heuristic_cfg(p);
  // the split count inside this launch's capacity, folding only where tickets exist
  const int cap = c.family == FAM_WINO ? 16 : max_ksplit(p);  // (launch_conv_wino clamps to its own capacity)
  if (c.ks < 1) c.ks = 1;
  if (c.ks > cap) { c.ks = cap; c.tail = 0; }
  c.fold = c.fold && p.tickets ? 1 : 0;
  if (c.tail < 0) c.tail = 0;
  // LDS-DMA staging only where the launch allows it, self-staging only on its tiles
  if (stages_by_dma(c.family) && !dma_ok(p)) c.family = FAM_WAVE_SPEC;
  if (c.family == FAM_SELF_STAGING && !conv_self_staging_tile(c.bm, c.bn)) c.family = FAM_DMA2;
  // every configuration of an fp16 launch multiplies alike: the register-staged families have no fp16 form, so where
  // the launcher itself would multiply in fp16 (heuristic_cfg) such an entry runs the LDS-DMA kernel on the same tile and split
  if (p.f16 && dma_ok(p) && (c.family == FAM_PLAIN || c.family == FAM_WAVE_SPEC)) c.family = FAM_DMA2;
  // eligibility of the families that take only some launches; the direct kernels multiply in fp32 only
  if (is_direct(c.family) && (p.f16 || !(c.family == FAM_THIN_K ? conv_thin_k_ok(p) : conv_thin_n_ok(p)))) return heuristic_cfg(p);
  if (c.family == FAM_TILE && !tile_ok(p, c.tile_height(), c.tile_channels())) return heuristic_cfg(p);
  if (c.family == FAM_WINO && (!conv_wino_ok(p) || !conv_wino_variant_ok(p, c.wino_variant()))) return heuristic_cfg(p);
  return c;
}

// ---- debug forcing (libudet_debug.so: udet_debug_force_conv) ---------------------------------------------------------------------
// bm / bn: tile (Winograd: bm = variant), 0: not forced; ks, family, fold (0 second launch, 1 last-arriving workgroup): < 0 not forced;
// tail_rounds > 0: tail split for this many workgroup slots per CU
struct ConvForce {
  int bm = 0, bn = 0, ks = -1, family = -1, fold = -1, tail_rounds = 0;
  bool ring3 = false;  // bit 22 itself, whatever lower family bit won: all a pair launch takes of the family bits
  bool any() const { return bm || family >= 0 || ks >= 0; }
};
static ConvForce g_force;
void conv_force_config(int bm, int bn, int ks) {
  ConvForce f;
  f.bm = bm & 0xffff; f.bn = bn;
  f.ks = ks < 0 ? ks : (ks & 0xff);
  f.tail_rounds = ks < 0 ? 0 : ((ks >> 8) & 0xff);  // ks + 256 r: tail split for r slots per CU (ks & 255 slices; 0: as many as fill a round)
  f.fold = (bm >> 20) & 1 ? 0 : ((bm >> 21) & 1 ? 1 : -1);
  f.ring3 = ((bm >> 22) & 1) != 0;
  // the family bits of bm, the lowest set one wins (bit 24: the direct kernel the launch is eligible for; bit 25: bm & 0xffff = variant)
  static const int BITS[][2] = {{16, FAM_PLAIN}, {17, FAM_DMA2}, {18, FAM_TILE}, {19, FAM_SELF_STAGING},
                                {22, FAM_DMA3}, {23, FAM_DMA4}, {24, FAM_THIN_K}, {25, FAM_WINO}};
  for (auto& b : BITS)
    if (f.family < 0 && ((bm >> b[0]) & 1)) f.family = b[1];
  g_force = f;
}
// test / tool hook: a single-operator launch carries no transformed Winograd weights -- build them here, from the packed ones
static void wino_operands_from_packed(ConvParams& p, hipStream_t stream) {
  int d9, w9[9];
  if (p.wino_u || p.f16 || p.xa || p.Kc % 8 != 0 || p.Kc < 8 || !conv_wino_geometry(p, &d9, w9)) return;
  static float* g_wino_scratch = nullptr;
  static size_t g_wino_cap = 0;
  static std::mutex mu;
  std::lock_guard<std::mutex> l(mu);
  const int np9 = conv_wino_np(p.Cout);
  const size_t need = (size_t)(p.Kc / 8) * 16 * 2 * np9 * 4;
  if (need > g_wino_cap) {
    (void)hipStreamSynchronize(stream);
    if (g_wino_scratch) (void)hipFree(g_wino_scratch);
    g_wino_scratch = nullptr; g_wino_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&g_wino_scratch), need * sizeof(float)) == hipSuccess) g_wino_cap = need;
  }
  if (g_wino_scratch && launch_wino_from_packed(p, g_wino_scratch, np9, stream) == UDET_OK) { p.wino_u = g_wino_scratch; p.wino_np = np9; }
}
// the forced fields over c; a forced family the launch is not eligible for falls back to the built-in choice (here or in runnable_cfg)
static void apply_forced(ConvParams& p, ConvCfg& c, hipStream_t stream) {
  const ConvForce& f = g_force;
  if (f.bm && f.family != FAM_WINO) { c.bm = f.bm; c.bn = f.bn; }
  if (f.ks >= 0) { c.ks = (f.ks > max_ksplit(p) && f.family != FAM_WINO) ? max_ksplit(p) : f.ks; c.tail = 0; }
  if (f.family >= 0) c.family = f.family;
  if (f.fold >= 0) c.fold = f.fold;
  if (f.tail_rounds > 0) {
    int fx = 0, k = 0;
    if (tail_for_rounds(p, c.bm, c.bn, f.tail_rounds, max_ksplit(p), &fx, &k)) { c.tail = fx; c.ks = c.ks >= 2 ? c.ks : k; c.fold = 0; }
  }
  if (f.family == FAM_TILE) { c.bm = f.bm == 4 ? 4 : 8; c.bn = f.bn == 16 ? 16 : 32; }
  if (f.family == FAM_THIN_K) c.family = conv_thin_k_ok(p) ? FAM_THIN_K : (conv_thin_n_ok(p) ? FAM_THIN_N : heuristic_cfg(p).family);
  if (f.family == FAM_WINO) {
    wino_operands_from_packed(p, stream);
    const int v = (f.bm & 7) == 4 ? 4 : (f.bm & 3);
    if (conv_wino_ok(p) && (conv_wino_variant_ok(p, v) || conv_wino_variant_ok(p, v ^ 1))) {
      c = ConvCfg::wino(conv_wino_variant_ok(p, v) ? v : (v ^ 1), f.ks < 0 ? 1 : c.ks);
    } else c = heuristic_cfg(p);
  }
}

// ---- launch_conv -----------------------------------------------------------------------------------------------------------------
static int g_debug_f16 = 0;  // test hook: fp16 multiplication for the single-operator entry points too
void conv_debug_f16(int on) { g_debug_f16 = on; }
int conv_debug_f16_on() { return g_debug_f16; }
static float g_debug_f16_grad_scale = 0.f;  // test hook: what the single-operator backward launches scale their gradient operand by
void conv_debug_f16_grad_scale(float s) { g_debug_f16_grad_scale = s > 0.f ? s : 0.f; }
float conv_debug_f16_grad_scale_now() { return g_debug_f16 ? g_debug_f16_grad_scale : 0.f; }
// argument checks + the derived fields every kernel family reads (Mall, fast divisors, uniform-cursor flags, segment rows)
static int conv_prepare(ConvParams& p) {
  if (g_debug_f16) p.f16 = 1;
  if (p.f16 && !(p.f16_xscale > 0.f)) p.f16_xscale = 1.f;
  // the tuning pass repeats every launch hundreds of times on random data, accumulating launches included: its "gradients" are far
  // larger than real ones and would overflow fp16 under the 4096 scale (every candidate NaN, every shape rejected); the scale does
  // not change a launch's duration
  if (p.f16 && conv_tuning_on()) p.f16_xscale = 1.f;
  if (p.Kc % 4 != 0 || p.ldx % 4 != 0 || p.x_coff % 4 != 0 || p.ldw % 4 != 0) {
    set_error("conv: Kc=%d ldx=%d x_coff=%d ldw=%d violate the 4-float alignment contract", p.Kc, p.ldx, p.x_coff, p.ldw);
    return UDET_ERR_ALIGN;
  }
  if (p.ntaps < 0 || p.ntaps > UDET_MAX_TAPS) {
    set_error("conv: ntaps=%d out of range", p.ntaps);
    return UDET_ERR_SHAPE;
  }
  if ((reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.wp)) & 15) {
    set_error("conv: x / packed weights must be 16-byte aligned");
    return UDET_ERR_ALIGN;
  }
  if (p.nseg) {
    if (p.nseg < 0 || p.nseg > UDET_MAX_SEGS || !p.tap_tab || p.up_shift || p.xa) {
      set_error("conv: malformed segmented launch");
      return UDET_ERR_ARG;
    }
    int prow = 0;
    for (int s = 0; s < p.nseg; ++s) {
      ConvSeg& g = p.seg[s];
      if (g.h < 1 || g.w < 1 || p.seg_tap[s + 1] - p.seg_tap[s] > UDET_MAX_TAPS || p.seg_tap[s + 1] < p.seg_tap[s]) {
        set_error("conv: segment %d is empty or has more than %d taps", s, UDET_MAX_TAPS);
        return UDET_ERR_SHAPE;
      }
      g.prow0 = prow;
      prow += p.N * g.h * g.w;
      g.fd_hw = make_fastdiv((unsigned)(g.h * g.w));
      g.fd_w = make_fastdiv((unsigned)g.w);
    }
    p.Mall = prow;
    p.ncls = 1; p.ntaps = 0; p.cls_tap[0] = p.cls_tap[1] = 0;
    p.OHq = p.seg[0].h; p.OWq = p.seg[0].w;  // (what the untuned heuristics and the log lines look at: the first, largest segment)
  } else {
    if (p.ncls != 4) {
      p.ncls = 1;
      p.cls_tap[0] = 0;
      p.cls_tap[1] = p.ntaps;
    }
    p.Mall = p.ncls * p.N * p.OHq * p.OWq;
  }
  p.fd_ohw = make_fastdiv((unsigned)(p.OHq * p.OWq));
  p.fd_ow = make_fastdiv((unsigned)p.OWq);
  // uniform K cursors (no up-sampled read).  bit 0: Kc >= 32, 32-wide stages (wave-specialised kernel); bit 1: Kc >= 16, 16-wide
  // stages (self-staging kernel); bit 2: Kc in {4, 8, 16}, 32 / Kc whole taps per 32-wide stage (wave-specialised kernel)
  p.kfast = 0;
  if (p.up_shift == 0) p.kfast = p.Kc >= 32 ? 3 : ((p.Kc >= 16 ? 2 : 0) | ((p.Kc == 4 || p.Kc == 8 || p.Kc == 16) ? 4 : 0));
  return UDET_OK;
}
static int g_last_cfg = 0;  // what the most recent launch ran (udet_debug_last_conv)
int conv_last_config() { return g_last_cfg; }
static int config_word(const ConvCfg& c) { return (c.family & 0xff) | ((c.bm & 0xfff) << 8) | ((c.ks & 0xff) << 20); }

int launch_conv(ConvParams& p, hipStream_t stream) {
  UDET_TRY(conv_prepare(p));
  ConvCfg c;
  const uint64_t key = conv_key(p);
  if (!conv_cache_find(key, &c)) {
    if (conv_tuning_on()) {
      c = tune_conv(p, key, stream);
    } else {
      c = heuristic_cfg(p);
      // untuned default for the 2-channel heads: the direct kernels (an order of magnitude fewer padded multiplications)
      // (not while a test pins an implicit-GEMM tile: udet_debug_force_conv)
      if (!g_force.bm && !p.f16 && conv_thin_n_ok(p)) c.family = FAM_THIN_N;
      else if (!g_force.bm && !p.f16 && conv_thin_k_ok(p)) c.family = FAM_THIN_K;
    }
  }
  apply_forced(p, c, stream);
  c = runnable_cfg(p, c);
  g_last_cfg = config_word(c) | ((c.ks > 1 && c.fold && c.family != FAM_TILE ? 1 : 0) << 28) | ((c.ks > 1 && c.tail > 0 ? 1 : 0) << 29);
  return run_conv_cfg(p, c, stream);
}

// ---- pair launches (two problems, one grid; conv_igemm_dma_pair_kernel) -----------------------------------------------------------------
// Eligible: two unsegmented fp32 problems the LDS-DMA family can take, with the same K depth, output width, tap geometry, class
// structure and strides (batch, operands, epilogue may differ).  The pair has ONE configuration (tile, K slices, stage ring), tuned as
// a unit and cached under the pair's own key; family < 0 in the cache = "these two are faster apart".
static int g_force_pair = -1;  // test hook (libudet_debug): 1 pairs whatever the tuner thinks, 0 never pairs
void conv_force_pair(int on) { g_force_pair = on; }
static int g_last_pair = 0;
int conv_last_pair() { return g_last_pair; }
static bool pair_compatible(const ConvParams& a, const ConvParams& b) {
  if (a.nseg || b.nseg || a.f16 || b.f16 || a.up_shift || b.up_shift || !dma_ok(a) || !dma_ok(b)) return false;
  if (a.Kc != b.Kc || a.Cout != b.Cout || a.ldw != b.ldw || a.ntaps != b.ntaps || a.ncls != b.ncls) return false;
  if (a.isy != b.isy || a.isx != b.isx || a.osy != b.osy || a.osx != b.osx || a.kfast != b.kfast) return false;
  if (!a.partial || a.partial != b.partial) return false;  // (one scratch region, carved in two by launch_conv_gemm_pair)
  for (int c = 0; c <= a.ncls; ++c)
    if (a.cls_tap[c] != b.cls_tap[c]) return false;
  for (int t = 0; t < a.ntaps; ++t)
    if (a.taps[t].dy != b.taps[t].dy || a.taps[t].dx != b.taps[t].dx) return false;
  return true;
}
// the configuration a test pins for a pair (udet_debug_force_conv while udet_debug_force_pair(1) is set): the forced tile where it is
// instantiated, the ring of bit 22, the forced split count (clamped by the caller); fold, tail split and the other family bits have
// no pair form and are ignored.  Neither the pair cache nor the tuner is asked.
static ConvCfg forced_pair_cfg(const ConvParams& a, const ConvParams& b) {
  const ConvForce& f = g_force;
  ConvCfg c = pair_heuristic(a, b);
  if (f.bm && conv_gemm_tile(f.bm, f.bn)) { c.bm = f.bm; c.bn = f.bn; }
  c.family = f.ring3 ? FAM_DMA3 : FAM_DMA2;
  if (f.ks >= 0) c.ks = f.ks;
  return c;
}
// Both problems in one launch where that is eligible and (tuned) faster; otherwise the two ordinary launches, a first.
int launch_conv_pair(ConvParams& a, ConvParams& b, hipStream_t stream) {
  g_last_pair = 0;
  UDET_TRY(conv_prepare(a));
  UDET_TRY(conv_prepare(b));
  // (a test that pins a family for single launches is respected)
  if (g_force_pair == 0 || (g_force.any() && g_force_pair != 1) || !pair_compatible(a, b)) {
    UDET_TRY(launch_conv(a, stream));
    return launch_conv(b, stream);
  }
  ConvCfg c;
  const uint64_t key = pair_key(a, b);
  if (g_force_pair == 1 && g_force.any()) {
    c = forced_pair_cfg(a, b);
  } else if (pair_cache_find(key, &c)) {
    if (c.family >= 0) {  // (an entry from a file: instantiated tiles and ring depths only)
      if (!conv_gemm_tile(c.bm, c.bn) || (c.family != FAM_DMA2 && c.family != FAM_DMA3)) c = pair_heuristic(a, b);
      if (c.ks < 1) c.ks = 1;
    }
  } else {
    c = conv_tuning_on() ? tune_conv_pair(a, b, key, stream) : pair_heuristic(a, b);
  }
  if (g_force_pair == 1 && c.family < 0) c = pair_heuristic(a, b);
  if (c.family < 0) {
    UDET_TRY(launch_conv(a, stream));
    return launch_conv(b, stream);
  }
  g_last_pair = 1;
  // (the split count that runs: launch_conv_gemm_pair clamps to the same capacity)
  const int cap = pair_max_ksplit(a, b);
  c.ks = c.ks > cap ? cap : (c.ks < 1 ? 1 : c.ks);
  g_last_cfg = config_word(c) | (1 << 30);
  return launch_conv_gemm_pair(a, b, c, stream);
}

}  // namespace udet
