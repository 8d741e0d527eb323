// Internal: what the convolution launchers share -- the kernel families, a launch's configuration, and the interfaces between
//   conv_igemm.hip   the host side of the implicit GEMM: the tile table, the grid of a launch, launch_conv_gemm / launch_conv_gemm_pair;
//                    the kernels, one family per file, and their launchers are behind conv_igemm_common.h (its header lists the files),
//   conv_select.hip  which configuration a launch runs (heuristics, debug forcing, validation; launch_conv / launch_conv_pair),
//   conv_tune.hip    the autotuner (timing, candidate verification, the three caches and their text form).
#pragma once
#include <functional>

#include "conv_host.h"
namespace udet {

// The kernel families of forward / backward-data launches.  The numbers are in tuning files (udet_tune_save) and in the low byte of
// udet_debug_last_conv: they must not move.
enum ConvFamily : int {
  FAM_PLAIN = 0,         // implicit GEMM, 256 threads, every wave stages and multiplies
  FAM_WAVE_SPEC = 1,     // implicit GEMM, wave-specialised (register-staged copies)
  FAM_DMA2 = 2,          // implicit GEMM, wave-specialised, LDS-DMA staging with a 2-stage ring
  FAM_TILE = 3,          // tile-resident direct convolution (conv_tile.hip)
  FAM_DMA3 = 4,          // LDS-DMA staging, 3-stage ring
  FAM_DMA4 = 5,          // LDS-DMA staging, 4-stage ring
  FAM_SELF_STAGING = 6,  // LDS-DMA staging by the multiplying waves themselves (4 waves, 16-wide stages)
  FAM_THIN_K = 7,        // direct kernel for two input channels (conv_thin.hip)
  FAM_THIN_N = 8,        // direct kernel for two output channels (conv_thin.hip)
  FAM_WINO = 9,          // Winograd F(2x2,3x3) (conv_wino.hip)
};
inline bool is_lds_dma(int f) { return f == FAM_DMA2 || f == FAM_DMA3 || f == FAM_DMA4; }    // the wave-specialised LDS-DMA rings
inline bool stages_by_dma(int f) { return is_lds_dma(f) || f == FAM_SELF_STAGING; }        // needs dma_ok(); multiplies in fp16 when asked to
inline bool is_direct(int f) { return f == FAM_THIN_K || f == FAM_THIN_N; }                // fp32 only
inline bool is_gemm(int f) { return f >= FAM_PLAIN && f <= FAM_SELF_STAGING && f != FAM_TILE; }  // (bm, bn) = an instantiated tile

// A launch's configuration, in the field order of a tuning file's "c" line.  GEMM families: bm x bn tile, ks K slices, summed by the
// last-arriving workgroup (fold) or a second launch; tail > 0: x-blocks [0, tail) unsplit, the rest cut into ks slices
// (ConvParams::tail_full).  The tile and Winograd families re-use bm / bn: build and read them through the functions below.
struct ConvCfg {
  int bm, bn, ks, family, fold, tail;
  static ConvCfg tile(int height, int channels_per_pass) { return {height, channels_per_pass, 1, FAM_TILE, 0, 0}; }
  static ConvCfg wino(int variant, int ks) { return {variant, 0, ks, FAM_WINO, 0, 0}; }
  static ConvCfg direct(int family) { return {0, 0, 1, family, 0, 0}; }
  int tile_height() const { return bm; }
  int tile_channels() const { return bn == 16 ? 16 : 32; }
  int wino_variant() const { return bm; }
  bool operator==(const ConvCfg& o) const { return bm == o.bm && bn == o.bn && ks == o.ks && family == o.family && fold == o.fold && tail == o.tail; }
};

// ---- conv_igemm.hip -----------------------------------------------------------------------------------------------------------
constexpr int CONV_GEMM_NTILES = 6;
extern const int CONV_GEMM_TILES[CONV_GEMM_NTILES][2];  // the instantiated (bm, bn) tiles, in the order the tuners scan them
bool conv_gemm_tile(int bm, int bn);                    // is (bm, bn) one of them?
bool conv_self_staging_tile(int bm, int bn);            // ... and one the self-staging kernel is instantiated for? (conv_igemm_self.hip)
int conv_xblocks(const ConvParams& p, int bm);          // x-blocks of a launch: M tiles of every class / segment
inline long cfg_tiles(const ConvParams& p, int bm, int bn) { return (long)conv_xblocks(p, bm) * ((p.Cout + bn - 1) / bn); }
// a prepared launch on a configuration of a GEMM family / two prepared, pair-compatible launches as one grid (c.family: FAM_DMA2 / FAM_DMA3)
int launch_conv_gemm(ConvParams& p, const ConvCfg& c, hipStream_t stream);
int launch_conv_gemm_pair(ConvParams& a, ConvParams& b, const ConvCfg& c, hipStream_t stream);

// ---- conv_select.hip ----------------------------------------------------------------------------------------------------------
bool dma_ok(const ConvParams& p);
int max_ksplit(const ConvParams& p);                              // capacity / minimum-work bound on the split count
int pair_max_ksplit(const ConvParams& a, const ConvParams& b);    // the same for a pair: both problems' slabs side by side
bool tail_for_rounds(const ConvParams& p, int bm, int bn, int r, int kcap, int* full_x, int* ks);
bool tile_ok(const ConvParams& p, int th, int cb);
ConvCfg heuristic_cfg(const ConvParams& p);
int run_conv_cfg(ConvParams& p, const ConvCfg& c, hipStream_t stream);  // a prepared launch on a configuration of any family, as given

// ---- conv_tune.hip ------------------------------------------------------------------------------------------------------------
bool conv_tuning_on();
bool wgrad_tuning_on();
uint64_t conv_key(const ConvParams& p);
uint64_t pair_key(const ConvParams& a, const ConvParams& b);
uint64_t wgrad_key(const WgradParams& p, int cap, bool dma_ok, int swapped);
bool conv_cache_find(uint64_t key, ConvCfg* c);
bool pair_cache_find(uint64_t key, ConvCfg* c);  // family < 0: "these two are faster apart"
bool wgrad_cache_find(uint64_t key, int* cfg);
// the tuners time their candidates on the caller's stream, verify the winner against the built-in configuration and cache what they return
ConvCfg tune_conv(ConvParams& p, uint64_t key, hipStream_t stream);
ConvCfg tune_conv_pair(ConvParams& a, ConvParams& b, uint64_t key, hipStream_t stream);
// filter gradient: run(cfg) launches GEMM + reduction on cfg = split count | variant << 20; what launch_wgrad_T knows about the launch
// (p: the caller's problem -- log lines, dw / db; g: the view that runs, operands possibly swapped; tiles: output tiles of the GEMM;
// cap: split capacity of the direct variants; maxs: slices the workspace holds; wsz: floats of dw; fused_bn: run() also writes dgamma / dbeta)
struct WgradTuneInfo { const WgradParams &p, &g; long tiles; int cap; size_t maxs; bool dma_ok, wino_ok; size_t wsz; bool fused_bn; };
int tune_wgrad(const WgradTuneInfo& t, int heuristic, uint64_t key, const std::function<int(int)>& run, hipStream_t stream);
}  // namespace udet
