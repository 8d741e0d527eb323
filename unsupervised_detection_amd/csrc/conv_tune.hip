// Autotuner of the convolution launchers.  While tuning is on, the first launch of every distinct problem shape times its candidate
// configurations on the caller's stream and caches the fastest: forward / backward-data launches (tune_conv; candidates of every
// family of conv_select.h), pair launches (tune_conv_pair) and the filter gradient (tune_wgrad).  Also here: the three caches with
// their text form (udet_tune_save / udet_tune_load), the problem keys, and the candidate verification.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "conv_select.h"

namespace udet {

static int tune_log_level() {  // UDET_TUNE_LOG: 1 one line per tuned shape, 2 also the candidates of the late stages
  const char* e = getenv("UDET_TUNE_LOG");
  return !e ? 0 : (atoi(e) > 1 ? 2 : 1);
}

// ---- problem keys (FNV-1a over the fields that decide which configuration is best) ---------------------------------------------
static uint64_t fnv(std::initializer_list<int> fields, uint64_t h = 1469598103934665603ull) {
  for (int v : fields) { h ^= (uint64_t)(uint32_t)v; h *= 1099511628211ull; }
  return h;
}
uint64_t conv_key(const ConvParams& p) {
  uint64_t h = fnv({p.N, p.H, p.W, p.up_shift, p.Kc, p.Cout, p.ntaps, p.ncls, p.OHq, p.OWq, p.isy, p.osy, p.xa ? 1 : 0,
                    p.ldx, p.ldy, p.accumulate, p.res ? 1 : 0, p.y2 ? 1 : 0, p.partial ? 1 : 0, p.cls_tap[1], p.uo ? 1 : 0, p.f16 ? 1 : 0, p.kreal,
                    p.wino_u ? p.wino_np : 0,
                    p.ntaps > 0 ? p.taps[0].dy : 0, p.ntaps > 0 ? p.taps[0].dx : 0});  // (first tap: the dilation -- it decides what the
                                                                                        // Winograd sub-lattices look like)
  for (int s = 0; s < p.nseg; ++s)  // segmented launches: the segment grids and their tap counts (ncls / OHq / OWq / taps[] are zero)
    h = fnv({p.seg[s].oy, p.seg[s].ox, p.seg[s].h, p.seg[s].w, p.seg_tap[s + 1]}, h);
  return h;
}
uint64_t pair_key(const ConvParams& a, const ConvParams& b) {
  uint64_t h = conv_key(a) * 1099511628211ull ^ conv_key(b);
  h ^= 0x9e3779b97f4a7c15ull;
  return h * 1099511628211ull;
}
uint64_t wgrad_key(const WgradParams& p, int cap, bool dma_ok, int swapped) {
  return fnv({p.N, p.H, p.W, p.up_shift, p.Cin, p.Cout, p.ntaps, p.OH, p.OW, p.isy, p.ya ? 1 : 0, p.ldx, p.ldy, cap, dma_ok ? 1 : 0, swapped, p.ycls,
              p.f16 ? 1 : 0,
              p.ntaps > 0 ? p.taps[0].dy : 0, p.ntaps > 0 ? p.taps[0].dx : 0});  // (the first tap's offsets: the dilation, which the Winograd
                                                                                  // family's tile grid depends on)
}

// ---- the caches and their text form -------------------------------------------------------------------------------------------
// A line of a tuning file is "<prefix> <key> <the first `fields` ints of the value>": lets a second process (a rocprofv3 trace of
// timed steps only, the other ranks of a data-parallel job) run exactly the configurations a tuning run picked.
template <class V>
struct TuneCache {
  static_assert(sizeof(V) % sizeof(int) == 0, "values are structs of ints");
  std::mutex mu;
  std::unordered_map<uint64_t, V> map;
  bool find(uint64_t key, V* v) {
    std::lock_guard<std::mutex> l(mu);
    auto it = map.find(key);
    if (it == map.end()) return false;
    *v = it->second;
    return true;
  }
  void put(uint64_t key, const V& v) { std::lock_guard<std::mutex> l(mu); map[key] = v; }
  int size() { std::lock_guard<std::mutex> l(mu); return (int)map.size(); }
  void dump(FILE* f, const char* prefix, int fields) {
    std::lock_guard<std::mutex> l(mu);
    for (auto& kv : map) {
      int v[sizeof(V) / sizeof(int)];
      memcpy(v, &kv.second, sizeof(V));
      fprintf(f, "%s %llu", prefix, (unsigned long long)kv.first);
      for (int i = 0; i < fields; ++i) fprintf(f, " %d", v[i]);
      fprintf(f, "\n");
    }
  }
};
static TuneCache<ConvCfg> g_cache;       // "c key bm bn ks family fold tail"
static TuneCache<ConvCfg> g_pair_cache;  // "p key bm bn ks family" (family < 0: the two problems stay apart)
static TuneCache<int> g_wcache;          // "w key cfg": split count | (variant: 1 / 2 LDS-DMA with a 2- / 3-stage ring, 3 Winograd domain) << 20
bool conv_cache_find(uint64_t key, ConvCfg* c) { return g_cache.find(key, c); }
bool pair_cache_find(uint64_t key, ConvCfg* c) { return g_pair_cache.find(key, c); }
bool wgrad_cache_find(uint64_t key, int* cfg) { return g_wcache.find(key, cfg); }
int tuned_shapes() { return g_cache.size() + g_wcache.size() + g_pair_cache.size(); }
void tune_dump(FILE* f) {
  g_cache.dump(f, "c", 6);
  g_wcache.dump(f, "w", 1);
  g_pair_cache.dump(f, "p", 4);
}
bool tune_put_line(const char* line) {  // one line of a tuning file ("c" lines of earlier files carry no tail); false: not an entry
  unsigned long long key;
  ConvCfg c = {0, 0, 0, 0, 0, 0};
  int w;
  const int nf = sscanf(line, "c %llu %d %d %d %d %d %d", &key, &c.bm, &c.bn, &c.ks, &c.family, &c.fold, &c.tail);
  if (nf == 6 || nf == 7) g_cache.put(key, c);
  else if (sscanf(line, "w %llu %d", &key, &w) == 2) g_wcache.put(key, w);
  else if (sscanf(line, "p %llu %d %d %d %d", &key, &c.bm, &c.bn, &c.ks, &c.family) == 5) g_pair_cache.put(key, ConvCfg{c.bm, c.bn, c.ks, c.family, 0, 0});
  else return false;
  return true;
}

// ---- tuning state, scratch and candidate verification --------------------------------------------------------------------------
// The tuner selects on time; a configuration that is fast because it computes something else must never be cached.  Before
// a winner is stored its output on the tuning data is compared (max-abs, relative to the largest reference element) with the
// output of the reference configuration (built-in heuristic, register-staged wave-specialised kernel).  The two result
// buffers are temporary device allocations that live only while tuning is on (the one place where the library allocates).
static int g_tuning = 0, g_wtuning = 0;
static float* g_vbuf[3] = {nullptr, nullptr, nullptr};  // two result buffers + {max|a-b|, max|a|}
static size_t g_vcap = 0;
static int g_rejected = 0;
int conv_tune_rejected() { return g_rejected; }
bool conv_tuning_on() { return g_tuning != 0; }
bool wgrad_tuning_on() { return g_wtuning != 0; }
void wgrad_set_tuning(int on) { g_wtuning = on; }
void conv_set_tuning(int on) {
  g_tuning = on;
  if (on) return;
  for (int i = 0; i < 3; ++i) { if (g_vbuf[i]) (void)hipFree(g_vbuf[i]); g_vbuf[i] = nullptr; }
  g_vcap = 0;
}
static float* tune_scratch(size_t floats, int which) {
  if (floats > g_vcap) {
    for (int i = 0; i < 2; ++i) { if (g_vbuf[i]) (void)hipFree(g_vbuf[i]); g_vbuf[i] = nullptr; }
    g_vcap = floats + floats / 4;
    for (int i = 0; i < 2; ++i)
      if (hipMalloc(reinterpret_cast<void**>(&g_vbuf[i]), g_vcap * sizeof(float)) != hipSuccess) { g_vbuf[i] = nullptr; g_vcap = 0; return nullptr; }
  }
  if (!g_vbuf[2] && hipMalloc(reinterpret_cast<void**>(&g_vbuf[2]), 2 * sizeof(float)) != hipSuccess) return nullptr;
  return g_vbuf[which];
}
__global__ __launch_bounds__(256) void tune_maxdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ out) {
  float d = 0.f, m = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const float x = a[e], y = b[e];
    float df = fabsf(x - y);
    if (!(df == df)) df = 3.0e38f;  // NaN in either result
    d = fmaxf(d, df);
    m = fmaxf(m, fabsf(x));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { d = fmaxf(d, __shfl_xor(d, o)); m = fmaxf(m, __shfl_xor(m, o)); }
  if ((threadIdx.x & 63) == 0) {  // non-negative floats order like their bit patterns
    atomicMax(reinterpret_cast<int*>(out), __float_as_int(d));
    atomicMax(reinterpret_cast<int*>(out) + 1, __float_as_int(m));
  }
}
// max|a-b| <= 2e-4 * max|a| + 1e-6 ?  (a = reference; split-K orders differ by ~1e-6 relative)
static bool tune_compare(const float* a, const float* b, size_t n, hipStream_t stream, float* diff_out, float* scale_out) {
  float* res = g_vbuf[2];
  if (!res) return false;
  if (hipMemsetAsync(res, 0, 2 * sizeof(float), stream) != hipSuccess) return false;
  long nbl = ((long)n + 255) / 256;
  hipLaunchKernelGGL(tune_maxdiff_kernel, dim3((int)(nbl > 2048 ? 2048 : nbl)), dim3(256), 0, stream, a, b, (long)n, res);
  float h[2] = {3.0e38f, 0.f};
  if (hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return false;
  *diff_out = h[0];
  *scale_out = h[1];
  return h[0] <= 2e-4f * h[1] + 1e-6f;
}
// p's output as plain stores into y, a dense [pixels][Cout rounded up to 4] buffer of *n floats (what the verification compares)
static ConvParams verification_view(const ConvParams& p, size_t* n) {
  ConvParams q = p;
  q.ldy = (p.Cout + 3) & ~3; q.y_coff = 0; q.accumulate = 0; q.y2 = nullptr; q.uo = nullptr;
  *n = (size_t)p.N * p.OH * p.OW * q.ldy;
  return q;
}

// ref and cand each fill a zeroed scratch buffer of n floats: do the two agree?
typedef std::function<int(float*)> FillRun;
static bool same_result(size_t n, const FillRun& ref, const FillRun& cand, hipStream_t stream, float* diff, float* scale) {
  float* r0 = tune_scratch(n, 0);
  float* r1 = tune_scratch(n, 1);
  if (!r0 || !r1) return false;
  (void)hipMemsetAsync(r0, 0, n * sizeof(float), stream);
  (void)hipMemsetAsync(r1, 0, n * sizeof(float), stream);
  return ref(r0) == UDET_OK && cand(r1) == UDET_OK && tune_compare(r0, r1, n, stream, diff, scale);
}

// ---- timing ---------------------------------------------------------------------------------------------------------------------
typedef std::function<int()> Launch;
// ms per call of `reps` calls behind a warm-up call; 1e30 when the launch fails
static float time_calls(const Launch& fn, int reps, hipStream_t stream) {
  static hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!e0) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); }
  if (fn() != UDET_OK) return 1e30f;
  (void)hipEventRecord(e0, stream);
  for (int r = 0; r < reps; ++r) (void)fn();
  (void)hipEventRecord(e1, stream);
  if (hipEventSynchronize(e1) != hipSuccess) return 1e30f;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  return ms / reps;
}
// How a candidate challenges the time to beat.  It is timed `reps` times.  A contender -- under gate x the time to beat and under
// gate_ms -- is timed `confirm` more times (0: never); that second figure replaces the first, or is averaged with it.  The candidate
// takes over when its figure is under factor x the time to beat.
struct Challenge { int reps, confirm; float factor, gate, gate_ms; bool average; };
static const float ANY_MS = 1e30f;
// THE STAGES OF THE TUNERS, in the order they run         reps confirm factor gate  gate_ms average
static const Challenge FIRST_SCAN   = {3, 6, 1.00f, 1.15f, 0.25f, true};     // every (tile, split count), wave-specialised; short launches re-timed
static const Challenge NON_SPEC     = {5, 0, 0.97f, 0.f, ANY_MS, false};     // the winner on the non-specialised kernel
static const Challenge DMA_RESCAN   = {3, 5, 0.98f, 0.98f, ANY_MS, false};   // every (tile, split count) on the LDS-DMA families 2, 4, 5, 6
static const Challenge TAIL_SPLIT   = DMA_RESCAN;                            // ... its tail splits, where the unsplit form is within TAIL_WITHIN
static const float TAIL_WITHIN      = 1.3f;
static const Challenge TILE_OR_WINO = {3, 5, 0.97f, 0.97f, ANY_MS, false};   // tile-resident (4 forms), later Winograd (variants x split counts)
static const Challenge DIRECT       = {5, 0, 0.97f, 0.f, ANY_MS, false};     // the direct kernels for two input / output channels
static const Challenge FOLD         = {5, 0, 0.98f, 0.f, ANY_MS, false};     // the winner's other way of summing its K slices
static const Challenge PAIR_SCAN    = {3, 6, 1.00f, 1.10f, ANY_MS, true};    // pair: every (tile, split count, ring); then PAIR_FACTOR
static const float PAIR_FACTOR      = 0.97f;                                 // ... x the time of the two launches apart
static const Challenge WGRAD_SCAN   = {3, 0, 1.00f, 0.f, ANY_MS, false};     // filter gradient: split counts x staging variants
static const Challenge WGRAD_WINO   = {3, 0, 0.97f, 0.f, ANY_MS, false};     // ... its Winograd-domain family
// true: fn took over and *to_beat is its time.  note(first timing, time to beat), where given, is called behind the first timing.
typedef std::function<void(float, float)> Note;
static bool challenge(const Challenge& s, const Launch& fn, float* to_beat, hipStream_t stream, const Note& note = nullptr) {
  float ms = time_calls(fn, s.reps, stream);
  if (note) note(ms, *to_beat);
  if (s.confirm && ms < *to_beat * s.gate && ms < s.gate_ms) {
    const float again = time_calls(fn, s.confirm, stream);
    ms = s.average ? 0.5f * (ms + again) : again;
  }
  if (!(ms < *to_beat * s.factor)) return false;
  *to_beat = ms;
  return true;
}

// (tile, split count) candidates of the GEMM families for a launch (or a pair) of tiles(bm, bn) output tiles, as wave-specialised
// configurations.  max_rounds: the split counts that fill 1 .. max_rounds whole rounds of the 256 CUs are tried.
static std::vector<ConvCfg> gemm_candidates(int Cout, int kcap, int max_rounds, const std::function<long(int, int)>& ntiles) {
  std::vector<ConvCfg> cand;
  for (auto& t : CONV_GEMM_TILES) {
    const int bm = t[0], bn = t[1];
    // N tiles wider than needed waste MFMA columns; much narrower ones re-read the A operand
    if (Cout <= 32 && bn != 32) continue;
    if (Cout > 32 && Cout <= 64 && bn > 64) continue;
    if (Cout > 64 && Cout <= 96 && bn != 96 && bn != 32) continue;
    if (Cout > 96 && bn < 64) continue;
    if (Cout > 96 && bn == 96 && Cout % 96 != 0 && Cout <= 128) continue;
    const long tiles = ntiles(bm, bn);
    std::vector<int> kss;
    for (int ks = 1; ks <= kcap; ks *= 2) kss.push_back(ks);
    // split counts that fill whole rounds of the 256 CUs (tiles*ks just below a multiple of 256): a 144-tile layer runs
    // at 144/256 of the chip unsplit and at 1008/1024 with 7 splits
    if (tiles < 512)
      for (int k = 1; k <= max_rounds; ++k) {
        const int ks = (int)(256L * k / tiles);
        if (ks >= 3 && ks <= kcap && (ks & (ks - 1)) != 0 && std::find(kss.begin(), kss.end(), ks) == kss.end()) kss.push_back(ks);
      }
    for (int ks : kss) {
      if (ks > 1 && (tiles >= 512 || tiles * ks > 4096)) continue;
      if (tiles * ks < 96 && ks * 2 <= kcap) continue;  // hopelessly under-filled
      cand.push_back({bm, bn, ks, FAM_WAVE_SPEC, 0, 0});
    }
  }
  return cand;
}

// ---- forward / backward-data ----------------------------------------------------------------------------------------------------
ConvCfg tune_conv(ConvParams& p, uint64_t key, hipStream_t stream) {
  // candidates are launched hundreds of times: an accumulating launch would grow its output with every repetition and the layers
  // behind it would be tuned (and verified) on ever larger data -- beyond the fp16 range in fp16 mode.  Timed as plain stores (one
  // read of the output less per element).
  const int acc = p.accumulate;
  p.accumulate = 0;
  auto on = [&p, stream](const ConvCfg& c) -> Launch { return [&p, c, stream]() { return run_conv_cfg(p, c, stream); }; };
  const int verbose = tune_log_level();
  const ConvCfg h = heuristic_cfg(p);
  const int kcap = max_ksplit(p);
  std::vector<ConvCfg> cand = gemm_candidates(p.Cout, kcap, 6, [&p](int bm, int bn) { return cfg_tiles(p, bm, bn); });
  cand.push_back(h);
  ConvCfg best = h;
  float scan_ms = 1e30f;
  for (auto& c : cand)
    if (challenge(FIRST_SCAN, on(c), &scan_ms, stream)) best = c;
  ConvCfg alt = best;
  alt.family = FAM_PLAIN;
  float a = time_calls(on(best), NON_SPEC.reps, stream), b;  // a: best's time; b: the non-specialised form's, taken or not
  if (challenge(NON_SPEC, on(alt), &a, stream, [&b](float ms, float) { b = ms; })) best = alt;
  const bool f16 = p.f16 && dma_ok(p);  // only LDS-DMA configurations multiply in fp16: every candidate must, or results differ per shape
  if (f16) { best = h; a = b = 1e30f; }
  if (dma_ok(p)) {  // LDS-DMA staging: re-scan the tiles, the balance between staging and MFMA waves differs
    for (auto& c : cand) {
      ConvCfg d = c;
      for (int family : {FAM_DMA2, FAM_DMA3, FAM_DMA4, FAM_SELF_STAGING}) {
        if (family == FAM_SELF_STAGING && !conv_self_staging_tile(d.bm, d.bn)) continue;
        d.family = family;
        float ms;
        if (challenge(DMA_RESCAN, on(d), &a, stream, [&ms](float first, float) { ms = first; })) best = d;
        // Tail split of an unsplit candidate: a launch whose workgroups fill r slots per CU for k whole rounds and a fraction of
        // another runs that last round on part of the chip (576 tiles of 64x64 on 256 CUs: three on 64 CUs, two on the rest).
        // Cutting only the LAST round's tiles into K slices makes it a full round of short workgroups, at the slab traffic of
        // those tiles alone.
        if (d.ks <= 1 && is_lds_dma(family) && p.partial && kcap >= 2 && ms < a * TAIL_WITHIN) {
          long seen[4] = {0, 0, 0, 0};
          for (int r = 1; r <= 4; ++r) {
            int full_x = 0, ks = 0;
            if (!tail_for_rounds(p, d.bm, d.bn, r, kcap, &full_x, &ks)) continue;
            const long id = (long)full_x * 1024 + ks;
            if (id == seen[0] || id == seen[1] || id == seen[2]) continue;
            seen[r - 1] = id;
            ConvCfg e = d;
            e.ks = ks; e.tail = full_x; e.fold = 0;
            if (challenge(TAIL_SPLIT, on(e), &a, stream)) best = e;
          }
        }
      }
    }
    b = a;
  }
  for (int cb : {32, 16})  // thin layers: tile-resident direct convolution (multiplies in fp16 too when asked to)
    for (int th : {8, 4}) {  // tile height x channels resident per pass
      if (!tile_ok(p, th, cb)) continue;
      const ConvCfg d = ConvCfg::tile(th, cb);
      if (challenge(TILE_OR_WINO, on(d), &a, stream)) { b = a; best = d; }
    }
  // What the stages from here on must beat.  QUIRK, kept as it was: without LDS-DMA staging b is still the non-specialised form's
  // time, which may be under a without having been taken (not under 0.97 a) -- then this is lower than the time of `best`.
  float to_beat = a < b ? a : b;
  for (int family : {FAM_THIN_K, FAM_THIN_N}) {
    if (!(family == FAM_THIN_K ? conv_thin_k_ok(p) : conv_thin_n_ok(p)) || p.f16) continue;  // (fp16 mode: every configuration must multiply alike)
    const ConvCfg d = ConvCfg::direct(family);
    if (challenge(DIRECT, on(d), &to_beat, stream, [&](float ms, float against) {
          if (verbose > 1) fprintf(stderr, "[udet tune]   direct family %d: %.1f us against %.1f (N=%d %dx%d Kc=%d taps=%d Cout=%d)\n", family, ms * 1e3f,
                               against * 1e3f, p.N, p.OHq, p.OWq, p.Kc, p.ntaps, p.Cout);
        })) best = d;
  }
  if (conv_wino_ok(p)) {  // Winograd F(2x2,3x3): 2.25x fewer multiplications; K slices where the tiles do not fill the chip
    for (int v = 0; v < 5; ++v) {  // (bit 0: tile shape, bit 1: four / eight waves; 4: the half-size form, two workgroups per CU)
      if (!conv_wino_variant_ok(p, v)) continue;
      const long wgs = conv_wino_workgroups(p, v);
      const int cap = conv_wino_max_ksplit(p, v);
      std::vector<int> kss = {1};
      if (wgs < 256 && cap >= 2) kss.push_back(2);  // (under one round of workgroups: two K slices even where no whole round results)
      if (wgs < 384)
        for (int r = 1; r <= 3; ++r) {
          const int ks = (int)(256L * r / (wgs > 0 ? wgs : 1));
          if (ks >= 2 && ks <= cap && std::find(kss.begin(), kss.end(), ks) == kss.end()) kss.push_back(ks);
        }
      for (int ks : kss) {
        const ConvCfg d = ConvCfg::wino(v, ks);
        if (challenge(TILE_OR_WINO, on(d), &to_beat, stream, [&](float ms, float against) {
              if (verbose > 1) fprintf(stderr, "[udet tune]   winograd variant %d ks=%d (%ld workgroups): %.1f us against %.1f (N=%d %dx%d Kc=%d Cout=%d)\n", v, ks, wgs,
                                   ms * 1e3f, against * 1e3f, p.N, p.OHq, p.OWq, p.Kc, p.Cout);
            })) best = d;
      }
    }
  }
  if (best.ks > 1 && is_gemm(best.family) && best.tail == 0) {  // the other way of summing the slabs: last-arriving workgroup <-> second launch
    const ConvCfg w = best;
    for (int ks : {w.ks, w.ks / 2, w.ks / 4}) {  // the folded form sums its slabs in one workgroup: fewer slabs may suit it better
      if (ks < 2) continue;
      ConvCfg d = w;
      d.fold = !w.fold;
      d.ks = ks;
      if (challenge(FOLD, on(d), &to_beat, stream)) best = d;
    }
  }
  // verification against the reference configuration on the tuning data (see above)
  if (!(best == h)) {
    size_t n;
    ConvParams q = verification_view(p, &n);
    float diff = 0.f, scale = 0.f;
    if (!same_result(n, [&](float* y) { q.y = y; return run_conv_cfg(q, h, stream); },
                     [&](float* y) { q.y = y; return run_conv_cfg(q, best, stream); }, stream, &diff, &scale)) {
      fprintf(stderr, "[udet tune] REJECTED N=%d %dx%d Kc=%d taps=%d cls=%d Cout=%d: %dx%d ks=%d ws=%d fold=%d tail=%d differs from the reference "
              "configuration (max|diff| %.3e, scale %.3e); keeping the heuristic\n", p.N, p.OHq, p.OWq, p.Kc, p.ntaps, p.ncls, p.Cout,
              best.bm, best.bn, best.ks, best.family, best.fold, best.tail, diff, scale);
      ++g_rejected;
      best = h;
    }
  }
  if (verbose)
    fprintf(stderr, "[udet tune] N=%d %dx%d Kc=%d taps=%d cls=%d Cout=%d -> %dx%d ks=%d ws=%d fold=%d tail=%d  %.1f us (heuristic %dx%d ks=%d)\n", p.N,
            p.OHq, p.OWq, p.Kc, p.ntaps, p.ncls, p.Cout, best.bm, best.bn, best.ks, best.family, best.fold, best.tail, to_beat * 1e3f, h.bm, h.bn,
            h.ks);
  p.accumulate = acc;
  g_cache.put(key, best);
  return best;
}

// ---- pairs ------------------------------------------------------------------------------------------------------------------------
ConvCfg tune_conv_pair(ConvParams& a, ConvParams& b, uint64_t key, hipStream_t stream) {
  const int acc_a = a.accumulate, acc_b = b.accumulate;
  a.accumulate = b.accumulate = 0;  // (see tune_conv: repeated accumulation would grow the data)
  // what the two cost apart, each on its own tuned configuration (launch_conv tunes a shape the first time it sees it)
  auto apart = [&]() -> int { ConvParams x = a, y = b; int rc = launch_conv(x, stream); return rc != UDET_OK ? rc : launch_conv(y, stream); };
  (void)apart();
  float t_apart = time_calls(apart, 5, stream);
  t_apart = 0.5f * (t_apart + time_calls(apart, 5, stream));
  ConvCfg best = {0, 0, 1, -1, 0, 0};
  float best_ms = 1e30f;
  for (ConvCfg c : gemm_candidates(a.Cout, pair_max_ksplit(a, b), 4, [&](int bm, int bn) { return cfg_tiles(a, bm, bn) + cfg_tiles(b, bm, bn); }))
    for (int family : {FAM_DMA2, FAM_DMA3}) {
      c.family = family;
      if (challenge(PAIR_SCAN, [&]() { return launch_conv_gemm_pair(a, b, c, stream); }, &best_ms, stream)) best = c;
    }
  // verification: each problem's output of the pair launch against its own stand-alone launch on the built-in configuration
  bool ok = best.family >= 0;
  float diff = 0.f, scale = 0.f;
  for (int which = 0; ok && which < 2; ++which) {
    size_t n;
    const ConvParams view = verification_view(which ? b : a, &n);
    ok = same_result(n, [&](float* y) { ConvParams q = view; q.y = y; return run_conv_cfg(q, heuristic_cfg(q), stream); },
                     [&](float* y) {
                       ConvParams q = view, o = which ? a : b;
                       q.y = y;
                       return launch_conv_gemm_pair(which ? o : q, which ? q : o, best, stream);
                     }, stream, &diff, &scale);
  }
  if (best.family >= 0 && !ok) {
    fprintf(stderr, "[udet tune] REJECTED pair N=%d+%d %dx%d Kc=%d taps=%d cls=%d Cout=%d: %dx%d ks=%d ws=%d differs from the stand-alone "
            "launches (max|diff| %.3e, scale %.3e); launching them apart\n", a.N, b.N, a.OHq, a.OWq, a.Kc, a.ntaps, a.ncls, a.Cout, best.bm, best.bn,
            best.ks, best.family, diff, scale);
    ++g_rejected;
    best.family = -1;
  }
  const bool pays = best_ms < t_apart * PAIR_FACTOR;
  if (tune_log_level())
    fprintf(stderr, "[udet tune] pair N=%d+%d %dx%d Kc=%d taps=%d cls=%d Cout=%d -> %dx%d ks=%d ws=%d  %.1f us, apart %.1f us%s\n", a.N, b.N, a.OHq,
            a.OWq, a.Kc, a.ntaps, a.ncls, a.Cout, best.bm, best.bn, best.ks, best.family, best_ms * 1e3f, t_apart * 1e3f, pays ? "" : " (kept apart)");
  if (!pays) best.family = -1;
  a.accumulate = acc_a; b.accumulate = acc_b;
  g_pair_cache.put(key, best);
  return best;
}

// ---- filter gradient: kernel + reduction timed together ---------------------------------------------------------------------------
int tune_wgrad(const WgradTuneInfo& t, int h, uint64_t key, const std::function<int(int)>& run, hipStream_t stream) {
  const WgradParams& p = t.p;
  auto on = [&run](int cfg) -> Launch { return [&run, cfg]() { return run(cfg); }; };
  float best_ms = 1e30f;
  int best = h;
  // candidates: powers of two around the heuristic + the split counts that fill whole rounds of the 256 CUs
  const int hc = h & 0xfffff;  // (the heuristic carries the staging variant in bit 20 in fp16 mode)
  std::vector<int> nss = {hc / 8, hc / 4, hc / 2, hc, hc * 2, hc * 4};
  for (int k : {1, 2, 3, 4, 6, 8}) {
    const int ns = (int)(256L * k / t.tiles);
    if (ns >= 1 && std::find(nss.begin(), nss.end(), ns) == nss.end()) nss.push_back(ns);
  }
  for (int dma = (p.f16 && t.dma_ok) ? 1 : 0; dma <= (t.dma_ok ? (p.f16 ? 1 : 2) : 0); ++dma)
    for (int ns : nss) {
      if (ns < 1 || ns > t.cap) continue;
      const int cfg = ns | (dma << 20);
      if (challenge(WGRAD_SCAN, on(cfg), &best_ms, stream)) best = cfg;
    }
  if (t.wino_ok) {  // the Winograd-domain family: one workgroup per CU and channel-block pair, or a few more / fewer slices
    const int blocks = (t.g.Cin / 64) * (t.g.Cout / 64);
    for (int wg : {256, 192, 384}) {
      const int ns = wgrad_wino_slices(t.g, (wg + blocks - 1) / blocks);
      if (ns < 1 || (size_t)ns > t.maxs) continue;
      const int cfg = ns | (3 << 20);
      if (challenge(WGRAD_WINO, on(cfg), &best_ms, stream, [&](float ms, float against) {
            if (tune_log_level() > 1) fprintf(stderr, "[udet tune]   wgrad winograd %d slices: %.1f us against %.1f (N=%d %dx%d Cin=%d Cout=%d)\n", ns, ms * 1e3f, against * 1e3f,
                                          p.N, p.OH, p.OW, p.Cin, p.Cout);
          })) best = cfg;
    }
  }
  // the winner's filter / bias gradient must equal the heuristic configuration's (candidate verification, above); BN-folded layers whose
  // reduction also forms dgamma / dbeta (wgrad_reduce_bn_kernel: one instantiation per channel width and split count): those two as
  // well.  (The separate form computes them behind run(), from a dw that is compared here, with kernels no configuration changes.)
  if (best != h) {
    const size_t nc = (size_t)p.Cout;
    const bool bn = p.gamma && t.fused_bn && p.dgamma && p.dbeta;
    float* r0 = tune_scratch(t.wsz + 3 * nc, 0);
    bool ok = false;
    float diff = 0.f, scale = 0.f;
    if (r0) {
      run(h);
      (void)hipMemcpyAsync(r0, p.dw, t.wsz * sizeof(float), hipMemcpyDeviceToDevice, stream);
      if (p.db) (void)hipMemcpyAsync(r0 + t.wsz, p.db, nc * sizeof(float), hipMemcpyDeviceToDevice, stream);
      if (bn) {
        (void)hipMemcpyAsync(r0 + t.wsz + nc, p.dgamma, nc * sizeof(float), hipMemcpyDeviceToDevice, stream);
        (void)hipMemcpyAsync(r0 + t.wsz + 2 * nc, p.dbeta, nc * sizeof(float), hipMemcpyDeviceToDevice, stream);
      }
      run(best);
      ok = tune_compare(r0, p.dw, t.wsz, stream, &diff, &scale);
      if (ok && p.db) ok = tune_compare(r0 + t.wsz, p.db, nc, stream, &diff, &scale);
      if (ok && bn) ok = tune_compare(r0 + t.wsz + nc, p.dgamma, nc, stream, &diff, &scale);
      if (ok && bn) ok = tune_compare(r0 + t.wsz + 2 * nc, p.dbeta, nc, stream, &diff, &scale);
    }
    if (!ok) {
      fprintf(stderr, "[udet tune] REJECTED wgrad N=%d %dx%d Cin=%d Cout=%d taps=%d: nsplit=%d dma=%d differs from the heuristic "
              "configuration (max|diff| %.3e, scale %.3e)\n", p.N, p.OH, p.OW, p.Cin, p.Cout, p.ntaps, best & 0xfffff, best >> 20, diff, scale);
      ++g_rejected;
      best = h;
    }
  }
  if (tune_log_level())
    fprintf(stderr, "[udet tune] wgrad N=%d %dx%d Cin=%d Cout=%d taps=%d -> nsplit=%d dma=%d (heuristic %d) %.1f us\n", p.N, p.OH,
            p.OW, p.Cin, p.Cout, p.ntaps, best & 0xfffff, best >> 20, h & 0xfffff, best_ms * 1e3f);
  g_wcache.put(key, best);
  return best;
}

}  // namespace udet
