// Host-only trace of what a step plan enqueues: every launch_* call of plan_build.hip and the plan_*.hip executor files, with its
// stream and every argument, every event / stream / copy call of the HIP runtime they make, and every profiling record -- printed by
// recording stand-ins, so no device code is involved and the tool builds and runs on a machine without a GPU.  Two builds of the
// library's host code enqueue the same work exactly when their traces are equal line for line:
//   C=unsupervised_detection_amd/csrc
//   hipcc --offload-host-only -no-hip-rt -x hip -std=c++17 -O1 -I$C tools/plan_trace.cpp $C/plan_*.hip -o /tmp/plan_trace
//   /tmp/plan_trace all > trace.txt          (or one scenario: plan_trace small0 fp16 pin3 prof)
// Scenario = shape {big: batch 4, 384x640 -> 192x384; small: batch 2, 128x192 -> 64x128; small0: small with the decoder's
// backward-data threshold at 0} x {fp32, fp16} x lanes {serial, pin3, pin1, probe} x {noprof, prof}.
// Pointers print as offsets from fixed fake bases (ws, the weight / gradient / Adam buffers, the images), events and streams as
// ordinal numbers in creation order.  Only the prototypes and the Plan fields of plan.h are used.  The tap-geometry helpers of
// conv_host.hip are restated below (they live in a file with kernels); conv_thin_n_ok and the *_last_config queries are simple
// deterministic rules that send launches down both sides of the branches that read them.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <type_traits>

#include "conv_host.h"
#include "elementwise.h"
#include "lanes.h"
#include "plan.h"

// ------------------------------------------------------------------ output ----
static std::map<const void*, int> g_streams, g_events;
static struct Range { const char* name; uintptr_t base; } const RANGES[] = {
    {"ws", 0x100000000000}, {"w_pwc", 0x200000000000}, {"w_gen", 0x210000000000}, {"w_rec", 0x220000000000}, {"g_gen", 0x230000000000},
    {"g_rec", 0x240000000000}, {"m", 0x250000000000}, {"v", 0x260000000000}, {"img1", 0x270000000000}, {"img2", 0x280000000000}};
static const uintptr_t RANGE_SPAN = 0x10000000000;
template <class T> static T* fake(const char* name) {
  for (const Range& r : RANGES)
    if (!strcmp(r.name, name)) return reinterpret_cast<T*>(r.base);
  return nullptr;
}
static char* g_host = nullptr;  // the one pinned allocation (hipHostMalloc)
static size_t g_host_size = 0;

static void put_ptr(const void* p) {
  const uintptr_t v = (uintptr_t)p;
  if (!p) { printf("null"); return; }
  for (const Range& r : RANGES)
    if (v >= r.base && v < r.base + RANGE_SPAN) { printf("%s+%zu", r.name, (size_t)(v - r.base)); return; }
  if (g_host && (const char*)p >= g_host && (const char*)p < g_host + g_host_size) { printf("host+%zu", (size_t)((const char*)p - g_host)); return; }
  printf("hostmem");
}
static void put_stream(hipStream_t s) {
  auto it = g_streams.find(s);
  if (it == g_streams.end()) printf("s?"); else printf("s%d", it->second);
}
static void put_event(hipEvent_t e) {
  auto it = g_events.find(e);
  if (it == g_events.end()) printf("e?"); else printf("e%d", it->second);
}
template <class T> static void put(const T& v) {
  if constexpr (std::is_same<T, hipStream_t>::value) put_stream(v);
  else if constexpr (std::is_same<T, hipEvent_t>::value) put_event(v);
  else if constexpr (std::is_pointer<T>::value) put_ptr((const void*)v);
  else if constexpr (std::is_floating_point<T>::value) printf("%.9g", (double)v);
  else if constexpr (std::is_unsigned<T>::value) printf("%llu", (unsigned long long)v);
  else printf("%lld", (long long)v);
}
static void args() {}
template <class T, class... R> static void args(const char* name, const T& v, const R&... rest) {
  printf(" %s=", name);
  put(v);
  args(rest...);
}
static void take_sink();
// one trace line: function, stream, name = value pairs
template <class... A> static int line(const char* fn, hipStream_t s, const A&... a) {
  printf("%s stream=", fn);
  put_stream(s);
  args(a...);
  printf("\n");
  take_sink();
  return 0;
}
static uint64_t fnv(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}
#define F(x) #x, p.x

namespace udet {
// ----------------------------------------------------- library stand-ins ----
static char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what) { set_error("HIP error %d at %s", (int)e, what); return UDET_ERR_HIP; }
thread_local LaunchSink* g_launch_sink = nullptr;
bool launch_sink_next(hipEvent_t* a, hipEvent_t* b) {  // (api.hip)
  LaunchSink* s = g_launch_sink;
  if (!s || s->n >= s->cap) return false;
  (void)hipEventCreate(a);
  (void)hipEventCreate(b);
  s->ev[2 * s->n] = *a; s->ev[2 * s->n + 1] = *b;
  ++s->n;
  return true;
}
// streams sit on four hardware queues in creation order (the caller's stream on queue 0)
int streams_concurrent(hipStream_t a, hipStream_t b, bool* c) {
  *c = g_streams[a] % 4 != g_streams[b] % 4;
  return line("streams_concurrent", a, "b", b, "concurrent", (int)*c);
}

// tap geometry, as in conv_host.hip
void same_pad(int in, int k, int s, int d, int* before, int* out) {
  const int o = (in + s - 1) / s;
  int total = (o - 1) * s + (k - 1) * d + 1 - in;
  if (total < 0) total = 0;
  *before = total / 2;
  *out = o;
}
static inline int floordiv2(int v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); }
static void push_tap(ConvParams& p, int dy, int dx, int widx) {
  const int ymax = (p.OHq - 1) * p.isy + dy, xmax = (p.OWq - 1) * p.isx + dx;
  if (dy >= p.H || ymax < 0 || dx >= p.W || xmax < 0) return;
  p.taps[p.ntaps].dy = dy; p.taps[p.ntaps].dx = dx; p.taps[p.ntaps].widx = widx;
  ++p.ntaps;
}
void conv_setup_fwd(ConvParams& p, int N, int H, int W, int kh, int kw, int s, int d) {
  int pt, pl, oh, ow;
  same_pad(H, kh, s, d, &pt, &oh);
  same_pad(W, kw, s, d, &pl, &ow);
  p.N = N; p.H = H; p.W = W;
  p.OH = oh; p.OW = ow; p.OHq = oh; p.OWq = ow;
  p.osy = p.osx = 1; p.ooy = p.oox = 0;
  p.isy = p.isx = s;
  p.ntaps = 0;
  for (int ky = 0; ky < kh; ++ky)
    for (int kx = 0; kx < kw; ++kx) push_tap(p, ky * d - pt, kx * d - pl, ky * kw + kx);
}
int conv_dgrad_classes(int s, int H, int W) { return s == 1 ? 1 : ((H % 2 == 0 && W % 2 == 0) ? 1 : s * s); }
bool conv_setup_dgrad(ConvParams& p, int cls, int N, int H, int W, int kh, int kw, int s, int d) {
  int pt, pl, ohf, owf;
  same_pad(H, kh, s, d, &pt, &ohf);
  same_pad(W, kw, s, d, &pl, &owf);
  p.N = N; p.H = ohf; p.W = owf;
  p.OH = H; p.OW = W;
  p.isy = p.isx = 1;
  p.ntaps = 0;
  p.ncls = 1;
  if (s == 1) {
    p.OHq = H; p.OWq = W; p.osy = p.osx = 1; p.ooy = p.oox = 0;
    for (int ky = 0; ky < kh; ++ky)
      for (int kx = 0; kx < kw; ++kx) push_tap(p, pt - ky * d, pl - kx * d, ky * kw + kx);
    return p.ntaps > 0;
  }
  const bool merged = (H % 2 == 0 && W % 2 == 0);
  p.osy = p.osx = s;
  const int c_lo = merged ? 0 : cls, c_hi = merged ? 4 : cls + 1;
  for (int c = c_lo; c < c_hi; ++c) {
    const int py = c / s, px = c % s;
    p.ooy = py; p.oox = px;
    p.OHq = (H - py + s - 1) / s;
    p.OWq = (W - px + s - 1) / s;
    if (merged) p.cls_tap[c] = p.ntaps;
    if (p.OHq <= 0 || p.OWq <= 0) {
      if (!merged) return false;
      continue;
    }
    for (int ky = 0; ky < kh; ++ky) {
      const int vy = py + pt - ky * d;
      if (((vy % 2) + 2) % 2) continue;
      for (int kx = 0; kx < kw; ++kx) {
        const int vx = px + pl - kx * d;
        if (((vx % 2) + 2) % 2) continue;
        push_tap(p, floordiv2(vy), floordiv2(vx), ky * kw + kx);
      }
    }
  }
  if (merged) {
    p.ncls = 4;
    p.cls_tap[4] = p.ntaps;
    p.ooy = p.oox = 0;
    p.OHq = H / 2; p.OWq = W / 2;
  }
  return true;
}
int conv_wino_np(int cout) { return cout > 64 ? round_up(cout, 128) : (cout > 32 ? 64 : 32); }
size_t conv_wino_floats(int Kc, int cout) { return (size_t)(Kc / 8) * 16 * 2 * conv_wino_np(cout) * 4; }
// (the real test also fits the kernel's tile into the LDS: here every other eligible level passes)
bool conv_thin_n_ok(const ConvParams& p) {
  if (p.nseg || p.Cout > 2 || p.Cout < 1 || p.xa != nullptr || p.Kc % 4 || p.ldw < 2 || p.ntaps < 1 || p.isy != p.isx || p.isy < 1 || p.isy > 2) return false;
  return (p.H / 8) % 2 == 0;
}

// ------------------------------------------------------- launch stand-ins ----
static void put_conv(const char* tag, const ConvParams& p) {
  printf("  %s:", tag);
  args(F(x), F(ldx), F(x_coff), F(N), F(H), F(W), F(up_shift), F(xa), F(xact), F(xalpha), F(wp), F(Kc), F(ldw), F(bias), F(y), F(ldy),
       F(y_coff), F(Cout), F(OH), F(OW), F(OHq), F(OWq), F(osy), F(osx), F(ooy), F(oox), F(isy), F(isx), F(ntaps), F(ncls));
  printf(" cls_tap=%d,%d,%d,%d,%d taps=", p.cls_tap[0], p.cls_tap[1], p.cls_tap[2], p.cls_tap[3], p.cls_tap[4]);
  for (int t = 0; t < p.ntaps && t < UDET_MAX_TAPS; ++t) printf("(%d,%d,%d)", p.taps[t].dy, p.taps[t].dx, p.taps[t].widx);
  printf(" taps_all=%016llx", (unsigned long long)fnv(p.taps, sizeof(p.taps)));
  args(F(nseg));
  for (int s = 0; s < p.nseg; ++s)
    printf(" seg%d=(%d,%d,%d,%d,%d;%u,%u,%u;%u,%u,%u)@%d", s, p.seg[s].oy, p.seg[s].ox, p.seg[s].h, p.seg[s].w, p.seg[s].prow0, p.seg[s].fd_hw.d,
           p.seg[s].fd_hw.mul, p.seg[s].fd_hw.sh, p.seg[s].fd_w.d, p.seg[s].fd_w.mul, p.seg[s].fd_w.sh, p.seg_tap[s]);
  printf(" seg_all=%016llx seg_tap_all=%016llx", (unsigned long long)fnv(p.seg, sizeof(p.seg)), (unsigned long long)fnv(p.seg_tap, sizeof(p.seg_tap)));
  args(F(tap_tab), F(Mall), "fd_ohw.d", p.fd_ohw.d, "fd_ohw.mul", p.fd_ohw.mul, "fd_ohw.sh", p.fd_ohw.sh, "fd_ow.d", p.fd_ow.d, "fd_ow.mul",
       p.fd_ow.mul, "fd_ow.sh", p.fd_ow.sh, F(kfast), F(zero16), F(act), F(alpha), F(res), F(ldres), F(res_coff), F(y2), F(ldy2), F(y2_coff),
       F(accumulate), F(uo), F(ldu), F(u_coff), F(ua), F(ldua), F(ua_coff), F(uact), F(ualpha), F(u_c0), F(u_c1), F(ksplit), F(partial),
       F(partial_cap), F(ldp), F(fold), F(tickets), F(tail_full), F(tail_ks), F(tail_prow0), F(f16), F(f16_xscale), F(wino_u), F(wino_np),
       F(kreal));
  printf("\n");
}
static int g_last_conv = 0, g_last_wgrad = 0;
int conv_last_config() { return g_last_conv; }
int wgrad_last_config() { return g_last_wgrad; }
int launch_conv(ConvParams& p, hipStream_t s) {
  line("launch_conv", s);
  put_conv("p", p);
  g_last_conv = p.wino_u ? 9 : 2;  // (FAM_WINO wherever the operand is there)
  return 0;
}
int launch_conv_pair(ConvParams& a, ConvParams& b, hipStream_t s) {
  line("launch_conv_pair", s);
  put_conv("a", a);
  put_conv("b", b);
  g_last_conv = 2;
  return 0;
}
int launch_tap_gather(const ConvParams& g, const float* z, int ldz, hipStream_t s) {
  line("launch_tap_gather", s, "z", z, "ldz", ldz);
  put_conv("g", g);
  return 0;
}
int launch_wgrad_T(WgradParams& p, int T, hipStream_t s) {
  line("launch_wgrad_T", s, "T", T, F(x), F(ldx), F(x_coff), F(N), F(H), F(W), F(up_shift), F(Cin), F(dy), F(ya), F(ldy), F(y_coff), F(Cout),
       F(yact), F(yalpha), F(OH), F(OW), F(isy), F(isx), F(ycls), F(OHf), F(OWf), F(ntaps), "taps_all", fnv(p.taps, sizeof(p.taps)), F(dw), F(db),
       F(partial), F(partial_floats), F(zero16), F(swapped), F(oCin), F(oCout), F(bias_m), F(Cin4), F(Mpad), F(pbias), "fd_ohw.d", p.fd_ohw.d,
       "fd_ow.d", p.fd_ow.d, F(w), F(b), F(gamma), F(dgamma), F(dbeta), F(bn_c), F(f16), F(f16_yscale));
  printf("  taps=");
  for (int t = 0; t < p.ntaps && t < UDET_MAX_TAPS; ++t) printf("(%d,%d,%d)", p.taps[t].dy, p.taps[t].dx, p.taps[t].widx);
  printf("\n");
  g_last_wgrad = (T == 9 && p.isy == 1 && p.Cin >= 64) ? 3 << 20 : 1;  // (the Winograd-domain family on the wide 3x3 layers)
  return 0;
}
#undef F
#define A(x) #x, x
int launch_bn_finalize(float* dw, int T, int Cin, int Cout, const float* w, const float* b, const float* gamma, float bn_c, float* pd, float* db,
                       float* dgamma, float* dbeta, hipStream_t s) {
  return line("launch_bn_finalize", s, A(dw), A(T), A(Cin), A(Cout), A(w), A(b), A(gamma), A(bn_c), A(pd), A(db), A(dgamma), A(dbeta));
}
int launch_wgrad_up_combine(const float* deff, float* dw, int Cin, int Cout, hipStream_t s) {
  return line("launch_wgrad_up_combine", s, A(deff), A(dw), A(Cin), A(Cout));
}
int launch_pack_weights(const float* src, float* dst, int T, int R, int C, int Kc, int ldw, int k_split, int k_gap, int mode, const float* scale,
                        hipStream_t s) {
  return line("launch_pack_weights", s, A(src), A(dst), A(T), A(R), A(C), A(Kc), A(ldw), A(k_split), A(k_gap), A(mode), A(scale));
}
int launch_pack_taps_into_n(const float* src, float* dst, int T, int R, int C, int Kc, int ldz, int k_split, int k_gap, int transposed, hipStream_t s) {
  return line("launch_pack_taps_into_n", s, A(src), A(dst), A(T), A(R), A(C), A(Kc), A(ldz), A(k_split), A(k_gap), A(transposed));
}
int launch_wino_pack(const float* src, float* dst, int R, int C, int Kc, int np, int k_split, int k_gap, int transposed, hipStream_t s) {
  return line("launch_wino_pack", s, A(src), A(dst), A(R), A(C), A(Kc), A(np), A(k_split), A(k_gap), A(transposed));
}
int launch_pack_jobs(const PackJob* jobs_dev, int njobs, const float* wsrc, float* ws, float bn_c, hipStream_t s) {
  return line("launch_pack_jobs", s, A(jobs_dev), A(njobs), A(wsrc), A(ws), A(bn_c));
}
int launch_copy_channels(const float* src, int lds, int s_coff, float* dst, int ldd, int d_coff, long P, int C, float mul, float add, hipStream_t s) {
  return line("launch_copy_channels", s, A(src), A(lds), A(s_coff), A(dst), A(ldd), A(d_coff), A(P), A(C), A(mul), A(add));
}
int launch_warp_cost_volume(const float* c1, const float* c2, const float* flow, int ldf, int f_coff, float flow_scale, float* out, int ldo,
                            int corr_coff, int c1_coff, float* warped_dbg, int N, int H, int W, int C, hipStream_t s) {
  return line("launch_warp_cost_volume", s, A(c1), A(c2), A(flow), A(ldf), A(f_coff), A(flow_scale), A(out), A(ldo), A(corr_coff), A(c1_coff),
              A(warped_dbg), A(N), A(H), A(W), A(C));
}
int launch_resize_bilinear_fwd(const float* x, int ldx, int x_coff, int N, int H, int W, float* y, int ldy, int y_coff, int OH, int OW, int C,
                               float mul, float div, hipStream_t s) {
  return line("launch_resize_bilinear_fwd", s, A(x), A(ldx), A(x_coff), A(N), A(H), A(W), A(y), A(ldy), A(y_coff), A(OH), A(OW), A(C), A(mul), A(div));
}
int launch_resize_bilinear_bwd(const float* dy, int ldy, int y_coff, int N, int OH, int OW, float* dx, int ldx, int x_coff, int H, int W, int C,
                               int accumulate, hipStream_t s) {
  return line("launch_resize_bilinear_bwd", s, A(dy), A(ldy), A(y_coff), A(N), A(OH), A(OW), A(dx), A(ldx), A(x_coff), A(H), A(W), A(C), A(accumulate));
}
int launch_upb_ring(const float* x, int ld, int N, int H, int W, float* xh, hipStream_t s) {
  return line("launch_upb_ring", s, A(x), A(ld), A(N), A(H), A(W), A(xh));
}
int launch_upb_ring_fold(const float* dxh, int ld, int N, int H, int W, float* dx, hipStream_t s) {
  return line("launch_upb_ring_fold", s, A(dxh), A(ld), A(N), A(H), A(W), A(dx));
}
int launch_share_samples(float* buf, long P, int ld, int coff, int C, int copies, hipStream_t s) {
  return line("launch_share_samples", s, A(buf), A(P), A(ld), A(coff), A(C), A(copies));
}
int launch_fold_samples(float* buf, long P, int ld, int coff, int C, int copies, hipStream_t s) {
  return line("launch_fold_samples", s, A(buf), A(P), A(ld), A(coff), A(C), A(copies));
}
int launch_emit_du(const float* d, const float* a, float* u, long P, int ld, int coff, int C, int act, float alpha, hipStream_t s) {
  return line("launch_emit_du", s, A(d), A(a), A(u), A(P), A(ld), A(coff), A(C), A(act), A(alpha));
}
int launch_pack_pwc_input(const float* i1, const float* i2, float* x8, long P, hipStream_t s) {
  return line("launch_pack_pwc_input", s, A(i1), A(i2), A(x8), A(P));
}
int launch_gen_input(const float* img, const float* f, double* part, float* gin, int B, long HW, hipStream_t s) {
  return line("launch_gen_input", s, A(img), A(f), A(part), A(gin), A(B), A(HW));
}
int launch_mask_rec_inputs(const float* logits, const float* f, float* mask, float* fin, long P, int ncalls, hipStream_t s) {
  return line("launch_mask_rec_inputs", s, A(logits), A(f), A(mask), A(fin), A(P), A(ncalls));
}
int launch_pack_imgin(const float* img, float* imgin, long P, int ncalls, hipStream_t s) {
  return line("launch_pack_imgin", s, A(img), A(imgin), A(P), A(ncalls));
}
int launch_losses(const float* f, const float* mask, const float* pred, long HW, int B, float cbn, float eps, float num_pixels, float* part,
                  float* losses, float* coef, float* sums, hipStream_t s) {
  return line("launch_losses", s, A(f), A(mask), A(pred), A(HW), A(B), A(cbn), A(eps), A(num_pixels), A(part), A(losses), A(coef), A(sums));
}
int launch_rec_loss_bwd(const float* f, const float* mask, const float* pred, float* dpred, long BHW, float cbn, float inv_np, hipStream_t s) {
  return line("launch_rec_loss_bwd", s, A(f), A(mask), A(pred), A(dpred), A(BHW), A(cbn), A(inv_np));
}
int launch_gen_loss_bwd(const float* f, const float* mask, const float* pred, const float* coef, float* dpred, float* dmask, long HW, int B,
                        float cbn, hipStream_t s) {
  return line("launch_gen_loss_bwd", s, A(f), A(mask), A(pred), A(coef), A(dpred), A(dmask), A(HW), A(B), A(cbn));
}
int launch_mask_bwd(const float* dmask, const float* dfin, const float* f, const float* mask, float* dlogits, long P, hipStream_t s) {
  return line("launch_mask_bwd", s, A(dmask), A(dfin), A(f), A(mask), A(dlogits), A(P));
}
int launch_grad_absmean(const float* g, const long* seg_off, const long* seg_len, int nvars, float* vmean, float thresh, float* out, hipStream_t s) {
  return line("launch_grad_absmean", s, A(g), A(seg_off), A(seg_len), A(nvars), A(vmean), A(thresh), A(out));
}
int launch_adam(float* w, float* g, float* m, float* v, long n, float lr_t, float b1, float b2, float eps, float clip, const float* flag,
                uint64_t seed, uint64_t step, hipStream_t s, int mode, const int* skip) {
  return line("launch_adam", s, A(w), A(g), A(m), A(v), A(n), A(lr_t), A(b1), A(b2), A(eps), A(clip), A(flag), A(seed), A(step), A(mode), A(skip));
}
int launch_nonfinite_count(const float* g, long n, int* out, hipStream_t s) { return line("launch_nonfinite_count", s, A(g), A(n), A(out)); }
}  // namespace udet

// every launch made while a profiling group is open takes a start / stop pair from the group's sink, as UDET_LAUNCH does
static bool g_in_runtime = false;
static void take_sink() {
  hipEvent_t a, b;
  if (!g_in_runtime && udet::g_launch_sink) (void)udet::launch_sink_next(&a, &b);
}

// ------------------------------------------------------ runtime stand-ins ----
struct RuntimeCall {  // (runtime calls are not kernel launches: they take nothing from the sink)
  RuntimeCall() { g_in_runtime = true; }
  ~RuntimeCall() { g_in_runtime = false; }
};
static hipEvent_t new_event() {
  const int n = (int)g_events.size() + 1;
  hipEvent_t e = reinterpret_cast<hipEvent_t>((uintptr_t)0x7e0000000000 + 64 * (uintptr_t)n);
  g_events[e] = n;
  return e;
}
static hipStream_t new_stream() {
  const int n = (int)g_streams.size();  // (the caller's stream is s0)
  hipStream_t s = reinterpret_cast<hipStream_t>((uintptr_t)0x750000000000 + 64 * (uintptr_t)n);
  g_streams[s] = n;
  return s;
}
extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) { RuntimeCall rc; *e = new_event(); line("hipEventCreate", nullptr, "event", *e); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  RuntimeCall rc;
  *e = new_event();
  line("hipEventCreateWithFlags", nullptr, "event", *e, A(flags));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { RuntimeCall rc; line("hipEventDestroy", nullptr, "event", e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { RuntimeCall rc; line("hipEventRecord", s, "event", e); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t e) { RuntimeCall rc; line("hipEventQuery", nullptr, "event", e); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { RuntimeCall rc; line("hipEventSynchronize", nullptr, "event", e); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) { RuntimeCall rc; line("hipStreamWaitEvent", s, "event", e, A(flags)); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
  RuntimeCall rc;
  *s = new_stream();
  line("hipStreamCreateWithFlags", *s, A(flags));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { RuntimeCall rc; line("hipStreamDestroy", s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { RuntimeCall rc; line("hipStreamSynchronize", s); return hipSuccess; }
hipError_t hipDeviceSynchronize() { RuntimeCall rc; printf("hipDeviceSynchronize\n"); return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) { RuntimeCall rc; line("hipMemsetAsync", s, A(dst), A(value), A(bytes)); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  RuntimeCall rc;
  if (kind == hipMemcpyHostToDevice) line("hipMemcpyAsync", s, A(dst), "src_hash", fnv(src, bytes), A(bytes), "kind", (int)kind);
  else line("hipMemcpyAsync", s, A(dst), A(src), A(bytes), "kind", (int)kind);
  if (kind == hipMemcpyDeviceToHost) memset(dst, 0, bytes);  // (no overflow to report)
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
  RuntimeCall rc;
  g_host = (char*)calloc(1, bytes);
  g_host_size = bytes;
  *p = g_host;
  line("hipHostMalloc", nullptr, A(bytes), A(flags));
  return hipSuccess;
}
hipError_t hipHostFree(void* p) { RuntimeCall rc; line("hipHostFree", nullptr, "ptr", p); free(p); g_host = nullptr; return hipSuccess; }
}
#undef A

// --------------------------------------------------------------- scenarios ----
using namespace udet;
static void result(const char* what, int rc) {
  printf("== %s rc=%d%s%s\n", what, rc, rc ? " error: " : "", rc ? g_err : "");
  g_err[0] = 0;
}
static void dump_prof(Plan* P) {
  for (Plan::ProfRec* r : P->prof) {
    printf("prof cat=%d name=%s flops=%.17g bytes=%.17g mfma_scale=%.17g kernels=%d a=", r->cat, r->name.c_str(), r->flops, r->bytes, r->mfma_scale, r->sink.n);
    put_event(r->a);
    printf(" b=");
    put_event(r->b);
    printf("\n");
    delete r;
  }
  P->prof.clear();
}
#define CALL(x) do { printf("== call %s\n", #x); const int rc_ = (x); result(#x, rc_); dump_prof(P); } while (0)

static int scenario(const char* shape, const char* prec, const char* lanes, const char* prof) {
  printf("######## scenario %s %s %s %s\n", shape, prec, lanes, prof);
  g_streams.clear();
  g_events.clear();
  hipStream_t s = new_stream();
  Config c;
  memset(&c, 0, sizeof(c));
  const bool big = !strcmp(shape, "big");
  c.batch = big ? 4 : 2; c.in_h = big ? 384 : 128; c.in_w = big ? 640 : 192; c.img_h = big ? 192 : 64; c.img_w = big ? 384 : 128;
  c.flow_normalizer = 80.f; c.cbn = 0.4f; c.epsilon = 0.01f;
  c.lr = 1e-4f; c.beta1 = 0.9f; c.beta2 = 0.999f; c.adam_eps = 1e-8f; c.clip = 10.f;
  c.noise_seed = 1234;
  c.conv_fp16 = !strcmp(prec, "fp16");
  plan_debug_upb_min_pixels(!strcmp(shape, "small0") ? 0 : -1);
  Plan* P = plan_build(c);
  if (!P) { printf("plan_build failed: %s\n", g_err); return 1; }
  printf("plan: %zu buffers, arena %zu floats, layers %zu/%zu/%zu\n", P->bufs.size(), P->arena_floats, P->pwc.size(), P->gen.size(), P->rec.size());
  float* ws = fake<float>("ws");
  const float *w_pwc = fake<float>("w_pwc"), *img1 = fake<float>("img1"), *img2 = fake<float>("img2");
  float *w_gen = fake<float>("w_gen"), *w_rec = fake<float>("w_rec"), *g_gen = fake<float>("g_gen"), *g_rec = fake<float>("g_rec");
  float *m = fake<float>("m"), *v = fake<float>("v");
  P->concurrent = strcmp(lanes, "serial") != 0;
  if (!strncmp(lanes, "pin", 3)) {
    hipStream_t side[3];
    const int n = atoi(lanes + 3);
    for (int i = 0; i < n; ++i) (void)hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking);
    CALL(plan_pin_lanes(P, s, side, n));
    hipStream_t bad[2] = {side[0], side[0]};
    CALL(plan_pin_lanes(P, s, bad, 2));
  }
  int queue[Plan::NLANE];
  CALL(plan_lane_queues(P, s, queue));
  printf("queues %d %d %d %d %d %d\n", queue[0], queue[1], queue[2], queue[3], queue[4], queue[5]);
  CALL(plan_pwc_forward(P, img1, img2, ws, s));  // (refused: nothing packed yet)
  CALL(plan_init_workspace(P, ws, s));
  CALL(plan_pack_pwc(P, w_pwc, ws, s));
  CALL(plan_pack_trainable(P, w_gen, w_rec, ws, s));
  P->profiling = !strcmp(prof, "prof");
  CALL(plan_forward(P, img1, img2, 3, ws, s));
  CALL(plan_backward(P, 3, w_gen, w_rec, g_gen, g_rec, ws, s));
  CALL(plan_apply(P, NET_GEN, w_gen, g_gen, m, v, ws, s));
  CALL(plan_apply(P, NET_REC, w_rec, g_rec, m, v, ws, s));
  CALL(plan_forward(P, nullptr, nullptr, 1, ws, s));
  CALL(plan_backward(P, 1, w_gen, nullptr, g_gen, nullptr, ws, s));
  CALL(plan_prefetch_consume(P, ws, s));  // (refused: no prefetch pending)
  CALL(plan_prefetch(P, img1, img2, ws, s));
  CALL(plan_pwc_forward(P, img1, img2, ws, s));
  CALL(plan_forward(P, img1, img2, 3, ws, s));  // a stand-alone forward while the prefetch is pending
  CALL(plan_forward(P, nullptr, nullptr, 3, ws, s, true));
  CALL(plan_backward(P, 2, nullptr, w_rec, nullptr, g_rec, ws, s));
  CALL(plan_recover_forward(P, 3, ws, s, true));  // caller-packed inputs: encoder A per sample
  CALL(plan_backward(P, 2, nullptr, w_rec, nullptr, g_rec, ws, s));
  CALL(plan_backward(P, 3, w_gen, w_rec, g_gen, g_rec, ws, s));
  CALL(plan_generator_layers(P, ws, s));
  CALL(plan_generator_forward(P, ws, s));
  CALL(plan_recover_forward(P, 0, ws, s));
  CALL(plan_losses(P, ws, s));
  CALL(plan_apply(P, NET_GEN, w_gen, g_gen, m, v, ws, s));
  CALL(plan_apply(P, NET_REC, w_rec, g_rec, m, v, ws, s));
  CALL(plan_apply(P, 0, w_rec, g_rec, m, v, ws, s));
  CALL(plan_check_overflow(P, false));
  CALL(plan_check_overflow(P, true));
  plan_settle_adam_step(P);
  printf("adam_t %ld\n", P->adam_t);
  P->profiling = false;
  printf("== destroy\n");
  delete P;
  return 0;
}

int main(int argc, char** argv) {
  static const char *SHAPES[] = {"big", "small", "small0"}, *PRECS[] = {"fp32", "fp16"}, *LANES[] = {"serial", "pin3", "pin1", "probe"},
                    *PROFS[] = {"noprof", "prof"};
  if (argc == 5) return scenario(argv[1], argv[2], argv[3], argv[4]);
  if (argc == 2 && !strcmp(argv[1], "all")) {
    for (const char* sh : SHAPES)
      for (const char* pr : PRECS)
        for (const char* ln : LANES)
          for (const char* pf : PROFS)
            if (scenario(sh, pr, ln, pf)) return 1;
    return 0;
  }
  fprintf(stderr, "usage: plan_trace all | plan_trace {big|small|small0} {fp32|fp16} {serial|pin3|pin1|probe} {noprof|prof}\n");
  return 2;
}
