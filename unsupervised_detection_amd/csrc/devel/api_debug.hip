// libudet_debug.so -- the test-only hooks of include/udet_debug.h.  They are NOT part of libudet.so: this small library links
// against it and reaches the (process-global) selection state of the convolution launcher through the internal C++
// interface (conv_host.h).  Only tests/ and tools/ load it; the product path never does.
#include <string.h>

#include <vector>

#include "../../../include/udet_debug.h"
#include "../conv_host.h"
#include "../elementwise.h"
#include "../plan_run.h"

using namespace udet;

extern "C" {
int udet_debug_last_conv(void) { return conv_last_config(); }
void udet_debug_force_conv(int bm, int bn, int ks) { conv_force_config(bm, bn, ks); }
void udet_debug_conv_fp16(int on) { conv_debug_f16(on); }
void udet_debug_conv_fp16_grad_scale(float s) { conv_debug_f16_grad_scale(s); }
void udet_debug_force_wgrad(int nsplit, int dma) { wgrad_force(nsplit, dma); }
int udet_debug_last_wgrad(void) { return wgrad_last_config(); }
int udet_debug_last_wgrad_reduce(void) { return wgrad_last_reduce(); }
// the whole of launch_wgrad_T (and launch_wgrad_up_T) as the step plan calls it: channel windows, BN-folded layers, the class-structured
// up form (tests/test_wgrad_gpu.py).  Every argument check comes before the first HIP call.
int udet_debug_conv2d_backward_filter_ex(const float* x, int ldx, int x_coff, const float* dy, int ldy, int y_coff, const float* y_saved, int act,
                                         float alpha, const float* w, const float* b, const float* gamma, float bn_c, float* dw, float* db,
                                         float* dgamma, float* dbeta, int n, int h, int wd, int cin, int cout, int k, int stride, int dilation,
                                         int up, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !dy || !dw || n < 1 || h < 1 || wd < 1 || cin < 1 || cout < 1 || k < 1 || k * k > UDET_MAX_TAPS || dilation < 1 ||
      (stride != 1 && stride != 2) || up < 0 || up > 2) {
    set_error("debug_backward_filter_ex: bad argument");
    return UDET_ERR_ARG;
  }
  if (ldx % 4 || x_coff % 4 || ldy % 4 || y_coff % 4) {
    set_error("debug_backward_filter_ex: ldx=%d x_coff=%d ldy=%d y_coff=%d must be multiples of 4", ldx, x_coff, ldy, y_coff);
    return UDET_ERR_ALIGN;
  }
  // the kernels read whole float4 groups of the window
  if (x_coff < 0 || y_coff < 0 || x_coff + round_up(cin, 4) > ldx || y_coff + round_up(cout, 4) > ldy) {
    set_error("debug_backward_filter_ex: channel window outside the buffer (x %d+%d of %d, dy %d+%d of %d)", x_coff, cin, ldx, y_coff, cout, ldy);
    return UDET_ERR_SHAPE;
  }
  if (gamma && (!w || !b || !db || !dgamma || !dbeta)) {
    set_error("debug_backward_filter_ex: a BN-folded layer needs w, b, db, dgamma and dbeta");
    return UDET_ERR_ARG;
  }
  if (up == 2 && (!gamma || y_saved || k != 3 || stride != 1 || dilation != 1)) {
    set_error("debug_backward_filter_ex: the class-structured form is a BN-folded 3x3 stride-1 layer on dU");
    return UDET_ERR_ARG;
  }
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 63) || workspace_bytes < 128 * sizeof(float)) {
    set_error("debug_backward_filter_ex: workspace must be 64-byte aligned and hold the zero block");
    return UDET_ERR_ARG;
  }
  float* zero = reinterpret_cast<float*>(workspace);  // 64 floats of zeros, then the slabs
  const int us = up ? 1 : 0;
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.ldx = ldx; p.x_coff = x_coff; p.N = n; p.Cin = cin;
  p.dy = dy; p.ldy = ldy; p.y_coff = y_coff; p.Cout = cout;
  if (y_saved && act != UDET_ACT_NONE) { p.ya = y_saved; p.yact = act; p.yalpha = alpha; }
  p.dw = dw; p.db = db;
  p.partial = zero + 64; p.partial_floats = workspace_bytes / sizeof(float) - 64;
  p.zero16 = zero;
  p.f16_yscale = conv_debug_f16_grad_scale_now();  // (udet_debug_conv_fp16_grad_scale; 0: none)
  if (gamma) { p.w = w; p.b = b; p.gamma = gamma; p.dgamma = dgamma; p.dbeta = dbeta; p.bn_c = bn_c; }
  ConvParams g;
  memset(&g, 0, sizeof(g));
  conv_setup_fwd(g, n, h << us, wd << us, k, k, stride, dilation);
  p.H = h << us; p.W = wd << us; p.up_shift = us;
  p.OH = g.OH; p.OW = g.OW; p.isy = p.isx = stride;
  p.ntaps = g.ntaps;
  memcpy(p.taps, g.taps, sizeof(g.taps));
  UDET_HIP(hipMemsetAsync(zero, 0, 64 * sizeof(float), stream));
  if (up == 2) return launch_wgrad_up_T(p, h, wd, stream);
  return launch_wgrad_T(p, k * k, stream);
}
void udet_debug_upb_min_pixels(long v) { plan_debug_upb_min_pixels(v); }
void udet_debug_force_pair(int on) { conv_force_pair(on); }
int udet_debug_last_pair(void) { return conv_last_pair(); }
// two forward convolutions of the same geometry (cin a multiple of 8; separate inputs / weights / biases / outputs, batches na / nb) through
// launch_conv_pair -- ONE launch when udet_debug_force_pair(1) is set and the LDS-DMA family can take both (tests/test_ops_gpu.py)
int udet_debug_conv2d_pair(const float* xa, const float* xb, const float* wa, const float* wb, const float* ba, const float* bb, float* ya, float* yb,
                           int na, int nb, int h, int w, int cin, int cout, int k, int stride, int dilation, int act, float alpha, void* workspace,
                           size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (cin % 8 != 0 || k * k > UDET_MAX_TAPS) { set_error("debug_conv2d_pair: cin must be a multiple of 8"); return UDET_ERR_SHAPE; }
  const int kc = cin, ldw = round_up(cout, 4);
  const size_t wfl = ((size_t)k * k * kc * ldw + 63) & ~(size_t)63, part_fl = (size_t)4 << 20, zero_fl = 64 + UDET_MAX_TICKETS;
  if (workspace_bytes < (2 * wfl + part_fl + zero_fl) * sizeof(float)) { set_error("debug_conv2d_pair: workspace too small"); return UDET_ERR_ARG; }
  float* wpa = reinterpret_cast<float*>(workspace);
  float* wpb = wpa + wfl;
  float* part = wpb + wfl;
  float* zero = part + part_fl;
  UDET_HIP(hipMemsetAsync(zero, 0, zero_fl * sizeof(float), stream));
  UDET_TRY(launch_pack_weights(wa, wpa, k * k, cin, cout, kc, ldw, kc, 0, 0, nullptr, stream));
  UDET_TRY(launch_pack_weights(wb, wpb, k * k, cin, cout, kc, ldw, kc, 0, 0, nullptr, stream));
  ConvParams p[2];
  for (int i = 0; i < 2; ++i) {
    memset(&p[i], 0, sizeof(ConvParams));
    conv_setup_fwd(p[i], i ? nb : na, h, w, k, k, stride, dilation);
    p[i].x = i ? xb : xa; p[i].ldx = cin; p[i].wp = i ? wpb : wpa; p[i].Kc = kc; p[i].ldw = ldw; p[i].bias = i ? bb : ba;
    p[i].y = i ? yb : ya; p[i].ldy = cout; p[i].Cout = cout; p[i].act = act; p[i].alpha = alpha;
    p[i].partial = part; p[i].partial_cap = part_fl; p[i].zero16 = zero; p[i].tickets = reinterpret_cast<int*>(zero + 64);
  }
  return launch_conv_pair(p[0], p[1], stream);
}
// ---- one level of the recover decoder's up-conv algebra, exactly as the plan runs it (tests/test_upconv_lowres_gpu.py) -------------------
// Everything the level does goes through the plan's own functions: build_upb_launches (segments, tap tables), upb_pack_jobs +
// launch_pack_jobs (weight sets, modes 9 / 10), upb_forward / upb_dgrad (ring, parameter blocks, launches, ring fold).  This file only
// lays a workspace out and checks arguments.
}  // extern "C"
namespace {
enum { UPC_TICKETS = 64, UPC_JOBS = UPC_TICKETS + UDET_MAX_TICKETS, UPC_JOBS_CAP = 192, UPC_TAB = UPC_JOBS + UPC_JOBS_CAP, UPC_TAB_CAP = 2048,
       UPC_WSETS = UPC_TAB + UPC_TAB_CAP, UPC_MIN_SLAB = 1 << 20 };
static_assert(UPC_WSETS == UDET_DEBUG_UPCONV_WSETS_OFFSET && UPC_WSETS % 64 == 0 && 8 * sizeof(PackJob) <= UPC_JOBS_CAP * sizeof(float), "workspace layout");
size_t upc_align64(size_t v) { return (v + 63) & ~(size_t)63; }
int upc_kct(int cout) { return round_up(cout, cout <= 4 ? 4 : 8); }
size_t upc_floats(int kc, int ldw) { return UPC_WSETS + upc_align64((size_t)4 * 36 * kc * ldw) + UPC_MIN_SLAB; }
// checks shared by the two directions; 0 or the error code (message set)
int upc_check(const char* who, const void* a, const void* b, const void* c, const void* d, int n, int h, int wd, int cin, int cout, void* workspace,
              size_t workspace_bytes, size_t need_floats) {
  if (!a || !b || !c || !d || n < 1 || cin < 1 || cout < 1) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  if (h < 2 || wd < 2) { set_error("%s: the source grid %d x %d must be at least 2 x 2 (one interior row / column and the last one)", who, h, wd); return UDET_ERR_SHAPE; }
  if ((long)n * (2 * h) * (2 * wd) >= (1L << 28)) { set_error("%s: grid too large", who); return UDET_ERR_SHAPE; }
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 63) || workspace_bytes < need_floats * sizeof(float)) {
    set_error("%s: workspace must be 64-byte aligned and hold %zu bytes", who, need_floats * sizeof(float));
    return UDET_ERR_ARG;
  }
  return UDET_OK;
}
// device copies of the pack jobs and of one tap table, the weight sets packed; the host vectors must outlive the stream's copies
int upc_stage(const Layer::SegLaunch& tab, const std::vector<PackJob>& jobs, const float* w, float* ws, hipStream_t stream) {
  if (tab.taps.size() * sizeof(ConvTap) > UPC_TAB_CAP * sizeof(float) || jobs.size() * sizeof(PackJob) > UPC_JOBS_CAP * sizeof(float)) {
    set_error("debug_upconv_lowres: table larger than its workspace slot");
    return UDET_ERR_ARG;
  }
  UDET_HIP(hipMemsetAsync(ws, 0, UPC_JOBS * sizeof(float), stream));  // zero block + ticket counters
  UDET_HIP(hipMemcpyAsync(ws + UPC_JOBS, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, stream));
  UDET_HIP(hipMemcpyAsync(ws + UPC_TAB, tab.taps.data(), tab.taps.size() * sizeof(ConvTap), hipMemcpyHostToDevice, stream));
  return launch_pack_jobs(reinterpret_cast<const PackJob*>(ws + UPC_JOBS), (int)jobs.size(), w, ws, BN_C, stream);
}
UpbLane upc_lane(float* ws, size_t ws_floats, size_t sets_floats) {
  const size_t off = UPC_WSETS + upc_align64(sets_floats);
  return UpbLane{ws + off, ws_floats - off, ws, reinterpret_cast<int*>(ws + UPC_TICKETS), 0};  // (f16: the udet_debug_conv_fp16 hook, conv_prepare)
}
}  // namespace
extern "C" {

size_t udet_debug_upconv_lowres_workspace_bytes(int ldx, int cin, int cout) {
  if (ldx < 1 || cin < 1 || cout < 1) return 0;
  const size_t f = upc_floats(ldx, round_up(cout, 4)), b = upc_floats(upc_kct(cout), round_up(cin, 4));
  return (f > b ? f : b) * sizeof(float);
}
int udet_debug_max_segs(void) { return UDET_MAX_SEGS; }

int udet_debug_upconv_lowres_fwd(const float* x, int ldx, const float* w, const float* bias, int act, float alpha, float* y, int ldy, int y_coff,
                                 float* xhat, int n, int h, int wd, int cin, int cout, int split, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "debug_upconv_lowres_fwd";
  if (act != UDET_ACT_NONE && act != UDET_ACT_LEAKY && act != UDET_ACT_ELU) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  if (ldx % 4 || ldy % 4 || y_coff % 4) { set_error("%s: ldx=%d ldy=%d y_coff=%d must be multiples of 4", who, ldx, ldy, y_coff); return UDET_ERR_ALIGN; }
  if (ldx < 4 || ldy < 4 || cin > ldx || y_coff < 0 || (cout >= 1 && y_coff + cout > ldy)) {
    set_error("%s: channel window outside the buffer (x %d of %d, y %d+%d of %d)", who, cin, ldx, y_coff, cout, ldy);
    return UDET_ERR_SHAPE;
  }
  if (split && cout > 16) { set_error("%s: the split form is the plan's for cout <= 16 only", who); return UDET_ERR_ARG; }
  Layer L;
  L.cin = cin; L.cout = cout;
  L.Kc = ldx; L.ldw = round_up(cout, 4);  // (the plan: L.Kc = the source slab's channel stride)
  L.k_split = round_up(cin, cin <= 4 ? 4 : 8); L.k_gap = 0;
  L.upb = true; L.upb_bwd = false; L.upb_split = split != 0;
  L.wupb_off = UPC_WSETS;
  const size_t sets = (size_t)4 * 36 * L.Kc * L.ldw;
  UDET_TRY(upc_check(who, x, w, y, xhat, n, h, wd, cin, cout, workspace, workspace_bytes, upc_floats(L.Kc, L.ldw)));
  float* ws = reinterpret_cast<float*>(workspace);
  build_upb_launches(L, h, wd);
  std::vector<PackJob> jobs;
  PackJob base;
  memset(&base, 0, sizeof(base));
  base.gamma_off = base.beta_off = -1;
  upb_pack_jobs(L, base, jobs);
  int st = upc_stage(L.upb_f, jobs, w, ws, stream);
  if (st == UDET_OK) {
    UpbFwd a;
    a.N = n; a.h = h; a.w = wd;
    a.src = x; a.xhat = xhat; a.ld = ldx;
    a.wsets = ws + L.wupb_off; a.Kc = L.Kc; a.ldw = L.ldw; a.bias = bias;
    a.y = y; a.ldy = ldy; a.y_coff = y_coff; a.cout = cout; a.act = act; a.alpha = alpha;
    a.tab = &L.upb_f; a.tab_dev = reinterpret_cast<const ConvTap*>(ws + UPC_TAB); a.split = L.upb_split;
    a.lane = upc_lane(ws, workspace_bytes / sizeof(float), sets);
    st = upb_forward(a, stream);
  }
  (void)hipStreamSynchronize(stream);  // `jobs` and the tap table are host temporaries
  return st;
}

int udet_debug_upconv_lowres_bwd(const float* dy, int ldy, int y_coff, const float* w, float* dx, int ldx, float* dxhat, int n, int h, int wd,
                                 int cin, int cout, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "debug_upconv_lowres_bwd";
  if (ldx % 4 || ldy % 4 || y_coff % 4) { set_error("%s: ldx=%d ldy=%d y_coff=%d must be multiples of 4", who, ldx, ldy, y_coff); return UDET_ERR_ALIGN; }
  const int kct = cout >= 1 ? upc_kct(cout) : 0;  // the launch reads whole padded channel blocks of the dy window
  if (ldx < 4 || ldy < 4 || cin > ldx || y_coff < 0 || y_coff + kct > ldy) {
    set_error("%s: channel window outside the buffer (dy %d+%d of %d, dx %d of %d)", who, y_coff, kct, ldy, cin, ldx);
    return UDET_ERR_SHAPE;
  }
  Layer L;
  L.cin = cin; L.cout = cout;
  L.Kc = ldx; L.ldw = round_up(cout, 4);
  L.k_split = round_up(cin, cin <= 4 ? 4 : 8); L.k_gap = 0;
  L.KcT = kct; L.ldwT = round_up(cin, 4);
  L.upb = true; L.upb_bwd = true;
  L.wupbT_off = UPC_WSETS;
  const size_t sets = (size_t)4 * 36 * L.KcT * L.ldwT;
  UDET_TRY(upc_check(who, dy, w, dx, dxhat, n, h, wd, cin, cout, workspace, workspace_bytes, upc_floats(L.KcT, L.ldwT)));
  float* ws = reinterpret_cast<float*>(workspace);
  build_upb_launches(L, h, wd);
  std::vector<PackJob> all, jobs;
  PackJob base;
  memset(&base, 0, sizeof(base));
  base.gamma_off = base.beta_off = -1;
  upb_pack_jobs(L, base, all);
  for (const PackJob& j : all)  // (the forward sets have no room in this call's workspace: the four mode-10 jobs only)
    if (j.mode == 10) jobs.push_back(j);
  int st = upc_stage(L.upb_b, jobs, w, ws, stream);
  if (st == UDET_OK) {
    UpbBwd a;
    a.N = n; a.h = h; a.w = wd;
    a.du = dy; a.lddu = ldy; a.du_coff = y_coff;
    a.wsetsT = ws + L.wupbT_off; a.KcT = L.KcT; a.ldwT = L.ldwT; a.cout = cout;
    a.dxhat = dxhat; a.dsrc = dx; a.ld = ldx; a.cin = cin;
    a.tab = &L.upb_b; a.tab_dev = reinterpret_cast<const ConvTap*>(ws + UPC_TAB);
    a.lane = upc_lane(ws, workspace_bytes / sizeof(float), sets);
    a.f16_xscale = conv_debug_f16_grad_scale_now();  // (udet_debug_conv_fp16_grad_scale; 0: none -- a plan passes 4096)
    st = upb_dgrad(a, stream);
  }
  (void)hipStreamSynchronize(stream);
  return st;
}

// host only: no HIP call.  seg [nseg][4] = oy, ox, h, w; seg_tap [nseg + 1]; taps [ntaps][3] = dy, dx, widx
int udet_debug_upconv_tables(int h, int w, int backward, int* nseg, int* seg, int* seg_tap, int* taps, int taps_cap, int* ntaps) {
  if (!nseg || !seg || !seg_tap || !taps || !ntaps || taps_cap < 0) { set_error("debug_upconv_tables: bad argument"); return UDET_ERR_ARG; }
  if (h < 2 || w < 2) { set_error("debug_upconv_tables: the source grid %d x %d must be at least 2 x 2", h, w); return UDET_ERR_SHAPE; }
  Layer L;
  build_upb_launches(L, h, w);
  const Layer::SegLaunch& g = backward ? L.upb_b : L.upb_f;
  *nseg = g.nseg;
  *ntaps = (int)g.taps.size();
  if (*ntaps > taps_cap) { set_error("debug_upconv_tables: %d taps, room for %d", *ntaps, taps_cap); return UDET_ERR_ARG; }
  for (int s = 0; s < g.nseg; ++s) {
    seg[4 * s] = g.seg[s].oy; seg[4 * s + 1] = g.seg[s].ox; seg[4 * s + 2] = g.seg[s].h; seg[4 * s + 3] = g.seg[s].w;
    seg_tap[s] = g.seg_tap[s];
  }
  seg_tap[g.nseg] = g.seg_tap[g.nseg];
  for (int t = 0; t < *ntaps; ++t) { taps[3 * t] = g.taps[t].dy; taps[3 * t + 1] = g.taps[t].dx; taps[3 * t + 2] = g.taps[t].widx; }
  return UDET_OK;
}

}  // extern "C"
// ---- one convolution launch as a plan builds it (tests/test_conv_epilogue_gpu.py): channel windows on every operand, the gap map of the
// packed weights, every epilogue option, the four-class up forms.  The parameter block comes from the project's own setup functions
// (conv_setup_fwd / conv_setup_dgrad / setup_up_fwd / setup_up_dgrad), the weights from its own pack code; this file lays the workspace
// out and checks arguments -- all of them before the first HIP call.
namespace {
enum { CEX_TICKETS = 64, CEX_JOB = CEX_TICKETS + UDET_MAX_TICKETS, CEX_W = CEX_JOB + 64 };
const size_t CEX_SLAB_FLOATS = (size_t)8 << 20;  // split-K scratch, as the single-operator entry points of api.hip take it
static_assert(CEX_W % 64 == 0 && sizeof(PackJob) <= 64 * sizeof(float), "workspace layout");
bool cex_backward(int form) { return form == 1 || form == 3; }
int cex_taps(const udet_debug_conv_ex& a) { return a.form >= 2 ? 16 : a.k * a.k; }
size_t cex_weight_floats(const udet_debug_conv_ex& a) {
  const int nout = cex_backward(a.form) ? a.cin : a.cout;
  return upc_align64((size_t)cex_taps(a) * a.kc * round_up(nout, 4));
}
bool cex_known_act(int act) { return act == UDET_ACT_NONE || act == UDET_ACT_LEAKY || act == UDET_ACT_ELU; }
// a window [coff, coff + c) of a row of ld floats
bool cex_outside(int ld, int coff, int c) { return ld < 1 || coff < 0 || (long)coff + c > ld; }
bool cex_misaligned(const void* q, unsigned b) { return (reinterpret_cast<uintptr_t>(q) & (b - 1)) != 0; }
// everything about one struct but its workspace
int cex_check_args(const udet_debug_conv_ex& a, const char* who) {
  if (a.form < 0 || a.form > 3) { set_error("%s: unknown form %d", who, a.form); return UDET_ERR_ARG; }
  if (!a.x || !a.w || !a.y) { set_error("%s: x, w and y must not be NULL", who); return UDET_ERR_ARG; }
  if (a.n < 1 || a.h < 1 || a.wd < 1 || a.cin < 1 || a.cout < 1 || a.k < 1 || a.k * a.k > UDET_MAX_TAPS || a.dilation < 1 ||
      (a.stride != 1 && a.stride != 2) || a.kc < 1 || a.k_gap < 0 || a.k_split < 0 || (a.up != 0 && a.up != 1) ||
      (a.accumulate != 0 && a.accumulate != 1) || (a.pack_job != 0 && a.pack_job != 1)) {
    set_error("%s: bad count", who);
    return UDET_ERR_ARG;
  }
  if ((long)a.n * (2L * a.h) * (2L * a.wd) >= (1L << 28)) { set_error("%s: grid too large", who); return UDET_ERR_ARG; }
  if (!cex_known_act(a.act) || !cex_known_act(a.xact) || !cex_known_act(a.uact)) { set_error("%s: unknown act", who); return UDET_ERR_ARG; }
  if (a.form != 0 && (a.up || a.k_gap || a.k_split != a.kc)) {
    set_error("%s: the loader's NN x2 and the gap map belong to form 0 (elsewhere up = 0, k_gap = 0, k_split = kc)", who);
    return UDET_ERR_ARG;
  }
  if (a.form >= 2 && (a.k != 3 || a.stride != 1 || a.dilation != 1)) { set_error("%s: forms 2 / 3 are NN x2 + 3x3 stride 1", who); return UDET_ERR_ARG; }
  if (a.form == 0 && a.up && a.stride != 1) { set_error("%s: the loader's NN x2 goes with stride 1", who); return UDET_ERR_ARG; }
  if (a.xa && a.form != 1) { set_error("%s: act' on load (xa) belongs to form 1", who); return UDET_ERR_ARG; }
  if (cex_backward(a.form) ? (a.bias != nullptr || a.act != UDET_ACT_NONE) : false) {
    set_error("%s: a backward-data launch has neither bias nor activation", who);
    return UDET_ERR_ARG;
  }
  if (a.uo && !a.ua) { set_error("%s: uo needs ua", who); return UDET_ERR_ARG; }
  // alignment: the A operand is read in float4 groups; every pointer holds floats
  auto mis = cex_misaligned;
  if (a.ldx % 4 || a.x_coff % 4 || a.kc % 4 || mis(a.x, 16) || (a.xa && mis(a.xa, 16))) {
    set_error("%s: ldx=%d x_coff=%d kc=%d must be multiples of 4 and x / xa 16-byte aligned", who, a.ldx, a.x_coff, a.kc);
    return UDET_ERR_ALIGN;
  }
  if (mis(a.w, 4) || mis(a.bias, 4) || mis(a.y, 4) || mis(a.res, 4) || mis(a.y2, 4) || mis(a.uo, 4) || mis(a.ua, 4)) {
    set_error("%s: misaligned float pointer", who);
    return UDET_ERR_ALIGN;
  }
  // windows
  const int kreal = cex_backward(a.form) ? a.cout : a.cin, nout = cex_backward(a.form) ? a.cin : a.cout;
  if (cex_outside(a.ldx, a.x_coff, a.kc)) { set_error("%s: x window %d+%d outside its row of %d", who, a.x_coff, a.kc, a.ldx); return UDET_ERR_SHAPE; }
  if (kreal + a.k_gap > a.kc || (a.k_gap > 0 && a.k_split > kreal)) {
    set_error("%s: %d real channels and a gap of %d at %d do not fit kc=%d", who, kreal, a.k_gap, a.k_split, a.kc);
    return UDET_ERR_SHAPE;
  }
  if (cex_outside(a.ldy, a.y_coff, nout)) { set_error("%s: y window %d+%d outside its row of %d", who, a.y_coff, nout, a.ldy); return UDET_ERR_SHAPE; }
  if (a.res && cex_outside(a.ldres, a.res_coff, nout)) { set_error("%s: res window outside its row", who); return UDET_ERR_SHAPE; }
  if (a.y2 && cex_outside(a.ldy2, a.y2_coff, nout)) { set_error("%s: y2 window outside its row", who); return UDET_ERR_SHAPE; }
  if (a.uo && (a.u_c0 < 0 || a.u_c1 < a.u_c0 || a.u_c1 > nout || a.u_coff < 0 || a.ua_coff < 0 || a.ldu < 1 || a.ldua < 1 ||
               (long)a.u_coff + a.u_c1 > a.ldu || (long)a.ua_coff + a.u_c1 > a.ldua)) {
    set_error("%s: emission columns [%d, %d) outside the launch's %d columns or the rows of uo / ua", who, a.u_c0, a.u_c1, nout);
    return UDET_ERR_SHAPE;
  }
  return UDET_OK;
}
int cex_check(const udet_debug_conv_ex& a, const void* workspace, size_t workspace_bytes) {
  const char* who = "debug_conv2d_ex";
  UDET_TRY(cex_check_args(a, who));
  if (!workspace || cex_misaligned(workspace, 64) || workspace_bytes < udet_debug_conv2d_ex_workspace_bytes(&a)) {
    set_error("%s: workspace must be 64-byte aligned and hold udet_debug_conv2d_ex_workspace_bytes", who);
    return UDET_ERR_ARG;
  }
  return UDET_OK;
}
// the weights of `a` packed to ws + w_off by one of the two packers of a plan: launch_pack_weights (pack_weights_kernel: the PWC-Net layers,
// packed once) or the per-step job table of the trainable networks (pack_jobs_kernel), which has its own copy of the gap map and the only
// form of modes 5 / 6.  j: the caller's host copy of the job, alive until the stream is synchronised.
int cex_pack(const udet_debug_conv_ex& a, float* ws, size_t w_off, PackJob& j, hipStream_t stream) {
  const int ldw = round_up(cex_backward(a.form) ? a.cin : a.cout, 4);
  if (a.form < 2 && !a.pack_job)
    return launch_pack_weights(a.w, ws + w_off, a.k * a.k, a.cin, a.cout, a.kc, ldw, a.k_split, a.k_gap, a.form, nullptr, stream);
  memset(&j, 0, sizeof(j));
  j.gamma_off = j.beta_off = -1;
  j.dst_off = (long)w_off; j.T = cex_taps(a); j.R = a.cin; j.C = a.cout; j.Kc = a.kc; j.ldw = ldw; j.k_split = a.k_split; j.k_gap = a.k_gap;
  j.mode = a.form < 2 ? a.form : (a.form == 2 ? 5 : 6); j.total = (long)j.T * a.kc * ldw;
  UDET_HIP(hipMemcpyAsync(ws + CEX_JOB, &j, sizeof(j), hipMemcpyHostToDevice, stream));
  return launch_pack_jobs(reinterpret_cast<const PackJob*>(ws + CEX_JOB), 1, a.w, ws, 1.f, stream);
}
// launch `cls` of `a` as a parameter block: the project's setup function, then the operands and options; false: a class without a launch
bool cex_params(const udet_debug_conv_ex& a, int cls, float* ws, const float* wp, float* part, ConvParams& p) {
  const bool bwd = cex_backward(a.form);
  const int nout = bwd ? a.cin : a.cout;
  memset(&p, 0, sizeof(p));
  if (a.form == 0) {
    conv_setup_fwd(p, a.n, a.h << a.up, a.wd << a.up, a.k, a.k, a.stride, a.dilation);
    p.up_shift = a.up;
  } else if (a.form == 1) {
    if (!conv_setup_dgrad(p, cls, a.n, a.h, a.wd, a.k, a.k, a.stride, a.dilation)) return false;
  } else if (a.form == 2) {
    setup_up_fwd(p, a.n, a.h, a.wd);
  } else {
    setup_up_dgrad(p, a.n, a.h, a.wd);
  }
  p.x = a.x; p.ldx = a.ldx; p.x_coff = a.x_coff;
  if (a.xa && a.xact != UDET_ACT_NONE) { p.xa = a.xa; p.xact = a.xact; p.xalpha = a.xalpha; }
  p.wp = wp; p.Kc = a.kc; p.ldw = round_up(nout, 4); p.bias = a.bias;
  if (bwd) { p.kreal = a.cout; p.f16_xscale = conv_debug_f16_grad_scale_now(); }  // (the x operand is a gradient; 0: none)
  p.y = a.y; p.ldy = a.ldy; p.y_coff = a.y_coff; p.Cout = nout;
  p.act = a.act; p.alpha = a.alpha;
  if (a.res) { p.res = a.res; p.ldres = a.ldres; p.res_coff = a.res_coff; }
  if (a.y2) { p.y2 = a.y2; p.ldy2 = a.ldy2; p.y2_coff = a.y2_coff; }
  p.accumulate = a.accumulate;
  if (a.uo) {
    p.uo = a.uo; p.ldu = a.ldu; p.u_coff = a.u_coff;
    p.ua = a.ua; p.ldua = a.ldua; p.ua_coff = a.ua_coff;
    p.uact = a.uact; p.ualpha = a.ualpha; p.u_c0 = a.u_c0; p.u_c1 = a.u_c1;
  }
  p.partial = part; p.partial_cap = CEX_SLAB_FLOATS;
  p.zero16 = ws; p.tickets = reinterpret_cast<int*>(ws + CEX_TICKETS);
  return true;
}
// what a pair launch carries (plan_exec.hip fwd_is_plain / dgrad_is_plain): a plain forward launch, or a backward-data pass that is ONE launch
bool cex_pair_form(const udet_debug_conv_ex& a) { return (a.form == 0 || a.form == 1) && a.up == 0; }
}  // namespace
extern "C" {
size_t udet_debug_conv2d_ex_workspace_bytes(const udet_debug_conv_ex* a) {
  if (!a || a->form < 0 || a->form > 3 || a->kc < 1 || a->cin < 1 || a->cout < 1 || a->k < 1 || a->k * a->k > UDET_MAX_TAPS) return 0;
  return (CEX_W + cex_weight_floats(*a) + CEX_SLAB_FLOATS) * sizeof(float);
}
int udet_debug_conv2d_ex(const udet_debug_conv_ex* args, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!args) { set_error("debug_conv2d_ex: bad argument"); return UDET_ERR_ARG; }
  const udet_debug_conv_ex& a = *args;
  UDET_TRY(cex_check(a, workspace, workspace_bytes));
  float* ws = reinterpret_cast<float*>(workspace);
  float* wp = ws + CEX_W;
  float* part = wp + cex_weight_floats(a);
  UDET_HIP(hipMemsetAsync(ws, 0, CEX_JOB * sizeof(float), stream));  // zero block + ticket counters
  PackJob j;  // (a host temporary: the stream is synchronised below)
  UDET_TRY(cex_pack(a, ws, CEX_W, j, stream));
  int st = UDET_OK;
  const int launches = a.form == 1 ? conv_dgrad_classes(a.stride, a.h, a.wd) : 1;
  for (int cls = 0; cls < launches && st == UDET_OK; ++cls) {
    ConvParams p;
    if (!cex_params(a, cls, ws, wp, part, p)) continue;
    st = launch_conv(p, stream);
  }
  const hipError_t e = hipStreamSynchronize(stream);  // (a fault in the launch is this call's error, not the caller's next one)
  if (st == UDET_OK && e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(stream)");
  return st;
}
// two such launches through launch_conv_pair, handed over as a lane hands its couples over: separate packed weights, ONE zero block, one set of
// ticket counters and one split-K scratch region (a.partial == b.partial, one partial_cap)
size_t udet_debug_conv2d_pair_ex_workspace_bytes(const udet_debug_conv_ex* a, const udet_debug_conv_ex* b) {
  if (!udet_debug_conv2d_ex_workspace_bytes(a) || !udet_debug_conv2d_ex_workspace_bytes(b)) return 0;
  return (CEX_W + cex_weight_floats(*a) + cex_weight_floats(*b) + CEX_SLAB_FLOATS) * sizeof(float);
}
int udet_debug_conv2d_pair_ex(const udet_debug_conv_ex* a_, const udet_debug_conv_ex* b_, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "debug_conv2d_pair_ex";
  if (!a_ || !b_) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  const udet_debug_conv_ex* q[2] = {a_, b_};
  for (const udet_debug_conv_ex* a : q) {
    UDET_TRY(cex_check_args(*a, who));
    if (!cex_pair_form(*a)) { set_error("%s: a pair carries forms 0 / 1 with up = 0 only", who); return UDET_ERR_ARG; }
    if (a->form == 1 && conv_dgrad_classes(a->stride, a->h, a->wd) != 1) {
      set_error("%s: backward-data of stride 2 on an odd grid is one launch per class: never a pair", who);
      return UDET_ERR_ARG;
    }
  }
  if (!workspace || cex_misaligned(workspace, 64) || workspace_bytes < udet_debug_conv2d_pair_ex_workspace_bytes(a_, b_)) {
    set_error("%s: workspace must be 64-byte aligned and hold udet_debug_conv2d_pair_ex_workspace_bytes", who);
    return UDET_ERR_ARG;
  }
  float* ws = reinterpret_cast<float*>(workspace);
  const size_t w_off[2] = {CEX_W, CEX_W + cex_weight_floats(*a_)};
  float* part = ws + w_off[1] + cex_weight_floats(*b_);
  UDET_HIP(hipMemsetAsync(ws, 0, CEX_JOB * sizeof(float), stream));  // zero block + ticket counters
  PackJob j[2];  // (host temporaries: the job slot is rewritten in stream order, the stream is synchronised below)
  ConvParams p[2];
  for (int i = 0; i < 2; ++i) {
    UDET_TRY(cex_pack(*q[i], ws, w_off[i], j[i], stream));
    (void)cex_params(*q[i], 0, ws, ws + w_off[i], part, p[i]);  // (one class: checked above)
  }
  const int st = launch_conv_pair(p[0], p[1], stream);
  const hipError_t e = hipStreamSynchronize(stream);  // (a fault in the launch is this call's error, not the caller's next one)
  if (st == UDET_OK && e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(stream)");
  return st;
}
}  // extern "C"
// ---- a 2-channel head in the GEMM + gather form, exactly the sequence of run_fwd's head branch (csrc/plan_exec.hip; tests/test_heads_gpu.py):
// the weights packed with the taps folded into the N axis (modes 3 / 4, either packer of a plan), ONE 1x1 GEMM over the channel axis into z
// [n, h, wd, ldz], then launch_tap_gather (bias + the per-tap shifted reads of z) into the output window.  A change to that branch belongs
// here too.
namespace {
int hex_taps(const udet_debug_head_ex& a) { return a.k * a.k; }
int hex_ldz(const udet_debug_head_ex& a) { return round_up(hex_taps(a) * 2, 32); }
size_t hex_wz_floats(const udet_debug_head_ex& a) { return upc_align64((size_t)a.kc * hex_ldz(a)); }
size_t hex_z_floats(const udet_debug_head_ex& a) { return upc_align64((size_t)a.n * a.h * a.wd * hex_ldz(a)); }
int hex_check(const udet_debug_head_ex& a, const void* workspace, size_t workspace_bytes) {
  const char* who = "debug_conv2d_head_ex";
  if (!a.x || !a.w || !a.y) { set_error("%s: x, w and y must not be NULL", who); return UDET_ERR_ARG; }
  if (a.n < 1 || a.h < 1 || a.wd < 1 || a.cin < 1 || a.k < 1 || a.kc < 1 || a.k_gap < 0 || a.k_split < 0) { set_error("%s: bad count", who); return UDET_ERR_ARG; }
  if (a.transposed != 0 && a.transposed != 1) { set_error("%s: unknown transposed %d", who, a.transposed); return UDET_ERR_ARG; }
  if (a.pack_job != 0 && a.pack_job != 1) { set_error("%s: unknown pack_job %d", who, a.pack_job); return UDET_ERR_ARG; }
  if (a.k > 8 || a.k * a.k * 2 > 64) { set_error("%s: k*k*2 = %d columns exceed the 64 a head's z row holds", who, a.k * a.k * 2); return UDET_ERR_ARG; }
  if (a.transposed && a.k != 4) { set_error("%s: the transposed form is 4x4 stride 2 (k = %d)", who, a.k); return UDET_ERR_ARG; }
  if ((long)a.n * (2L * a.h) * (2L * a.wd) >= (1L << 28)) { set_error("%s: grid too large", who); return UDET_ERR_ARG; }
  if (a.ldx % 4 || a.x_coff % 4 || a.kc % 4 || cex_misaligned(a.x, 16)) {
    set_error("%s: ldx=%d x_coff=%d kc=%d must be multiples of 4 and x 16-byte aligned", who, a.ldx, a.x_coff, a.kc);
    return UDET_ERR_ALIGN;
  }
  if (cex_misaligned(a.w, 4) || cex_misaligned(a.bias, 4) || cex_misaligned(a.y, 4)) { set_error("%s: misaligned float pointer", who); return UDET_ERR_ALIGN; }
  if (cex_outside(a.ldx, a.x_coff, a.kc)) { set_error("%s: x window %d+%d outside its row of %d", who, a.x_coff, a.kc, a.ldx); return UDET_ERR_SHAPE; }
  if ((long)a.cin + a.k_gap > a.kc || (a.k_gap > 0 && a.k_split > a.cin)) {
    set_error("%s: %d real channels and a gap of %d at %d do not fit kc=%d", who, a.cin, a.k_gap, a.k_split, a.kc);
    return UDET_ERR_SHAPE;
  }
  if (cex_outside(a.ldy, a.y_coff, 2)) { set_error("%s: y window %d+2 outside its row of %d", who, a.y_coff, a.ldy); return UDET_ERR_SHAPE; }
  if (!workspace || cex_misaligned(workspace, 64) || workspace_bytes < udet_debug_conv2d_head_ex_workspace_bytes(&a)) {
    set_error("%s: workspace must be 64-byte aligned and hold udet_debug_conv2d_head_ex_workspace_bytes", who);
    return UDET_ERR_ARG;
  }
  return UDET_OK;
}
}  // namespace
extern "C" {
size_t udet_debug_conv2d_head_ex_workspace_bytes(const udet_debug_head_ex* a) {
  if (!a || a->n < 1 || a->h < 1 || a->wd < 1 || a->kc < 1 || a->k < 1 || a->k > 8 || a->k * a->k * 2 > 64) return 0;
  return (CEX_W + hex_wz_floats(*a) + hex_z_floats(*a) + CEX_SLAB_FLOATS) * sizeof(float);
}
int udet_debug_conv2d_head_ex(const udet_debug_head_ex* args, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!args) { set_error("debug_conv2d_head_ex: bad argument"); return UDET_ERR_ARG; }
  const udet_debug_head_ex& a = *args;
  UDET_TRY(hex_check(a, workspace, workspace_bytes));
  float* ws = reinterpret_cast<float*>(workspace);
  float* wz = ws + CEX_W;
  float* z = wz + hex_wz_floats(a);
  float* part = z + hex_z_floats(a);
  const int T = hex_taps(a), ldz = hex_ldz(a);
  UDET_HIP(hipMemsetAsync(ws, 0, CEX_JOB * sizeof(float), stream));  // zero block + ticket counters
  PackJob j;  // (a host temporary: the stream is synchronised below)
  if (!a.pack_job) {
    UDET_TRY(launch_pack_taps_into_n(a.w, wz, T, a.cin, 2, a.kc, ldz, a.k_split, a.k_gap, a.transposed, stream));
  } else {  // the job plan_pack.hip builds for a head of the trainable networks (mode 4: the same job on HWOI weights)
    memset(&j, 0, sizeof(j));
    j.gamma_off = j.beta_off = -1;
    j.dst_off = (long)CEX_W; j.T = T; j.R = a.cin; j.C = 2; j.Kc = a.kc; j.ldw = ldz; j.k_split = a.k_split; j.k_gap = a.k_gap;
    j.mode = a.transposed ? 4 : 3; j.total = (long)a.kc * ldz;
    UDET_HIP(hipMemcpyAsync(ws + CEX_JOB, &j, sizeof(j), hipMemcpyHostToDevice, stream));
    UDET_TRY(launch_pack_jobs(reinterpret_cast<const PackJob*>(ws + CEX_JOB), 1, a.w, ws, 1.f, stream));
  }
  int st;
  {
    ConvParams p;
    memset(&p, 0, sizeof(p));
    conv_setup_fwd(p, a.n, a.h, a.wd, 1, 1, 1, 1);
    p.x = a.x; p.ldx = a.ldx; p.x_coff = a.x_coff;
    p.wp = wz; p.Kc = a.kc; p.ldw = ldz;
    p.y = z; p.ldy = ldz; p.y_coff = 0; p.Cout = T * 2;
    p.partial = part; p.partial_cap = CEX_SLAB_FLOATS;
    p.zero16 = ws; p.tickets = reinterpret_cast<int*>(ws + CEX_TICKETS);
    st = launch_conv(p, stream);
  }
  if (st == UDET_OK) {
    ConvParams g;
    memset(&g, 0, sizeof(g));
    if (a.transposed) (void)conv_setup_dgrad(g, 0, a.n, 2 * a.h, 2 * a.wd, a.k, a.k, 2, 1);
    else conv_setup_fwd(g, a.n, a.h, a.wd, a.k, a.k, 1, 1);
    g.H = a.h; g.W = a.wd;  // Z lives on the input grid
    g.bias = a.bias;
    g.y = a.y; g.ldy = a.ldy; g.y_coff = a.y_coff; g.Cout = 2;
    st = launch_tap_gather(g, z, ldz, stream);
  }
  const hipError_t e = hipStreamSynchronize(stream);  // (a fault in a launch is this call's error, not the caller's next one)
  if (st == UDET_OK && e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(stream)");
  return st;
}
// launch_warp_cost_volume with a plan's slab arguments (csrc/plan_step.hip; tests/test_warp_cost_volume_slab_gpu.py): nothing but checks
int udet_debug_warp_cost_volume_ex(const float* c1, const float* c2, const float* flow, int ldf, int f_coff, float flow_scale, float* out, int ldo,
                                   int corr_coff, int c1_coff, int n, int h, int w, int c, void* stream) {
  const char* who = "debug_warp_cost_volume_ex";
  if (!c1 || !c2 || !out || n < 1 || h < 1 || w < 1 || c < 1) { set_error("%s: NULL operand or bad count", who); return UDET_ERR_ARG; }
  // the launcher's own conditions, before anything reaches it
  if (c % 4 != 0 || (flow && (h < 2 || w < 2))) { set_error("%s: C=%d must be a multiple of 4 and H,W >= 2 with a flow (got %dx%d)", who, c, h, w); return UDET_ERR_SHAPE; }
  if (ldo < 1 || (long)n * h * w * (c > ldo ? c : ldo) >= (1L << 31)) { set_error("%s: tensor too large for 32-bit element offsets", who); return UDET_ERR_SHAPE; }
  if (c1_coff >= 0 && ((c1_coff | ldo) & 3)) { set_error("%s: c1 segment offset %d / row stride %d must be multiples of 4", who, c1_coff, ldo); return UDET_ERR_ALIGN; }
  if (cex_misaligned(c1, 16) || cex_misaligned(c2, 16) || cex_misaligned(flow, 4) || cex_misaligned(out, c1_coff >= 0 ? 16 : 4)) {
    set_error("%s: c1 / c2 (and out with a c1 segment) must be 16-byte aligned, flow a float pointer", who);
    return UDET_ERR_ALIGN;
  }
  // windows
  if (corr_coff < 0 || (long)corr_coff + 81 > ldo) { set_error("%s: corr window %d+81 outside its row of %d", who, corr_coff, ldo); return UDET_ERR_SHAPE; }
  if (c1_coff < -1 || (c1_coff >= 0 && (long)c1_coff + c > ldo)) { set_error("%s: c1 window %d+%d outside its row of %d", who, c1_coff, c, ldo); return UDET_ERR_SHAPE; }
  if (flow && (ldf < 1 || f_coff < 0 || (long)f_coff + 2 > ldf)) { set_error("%s: flow window %d+2 outside its row of %d", who, f_coff, ldf); return UDET_ERR_SHAPE; }
  if (flow && (long)n * h * w * ldf >= (1L << 31)) { set_error("%s: flow tensor too large", who); return UDET_ERR_SHAPE; }
  auto overlap = [](long a0, long a1, long b0, long b1) { return a0 < b1 && b0 < a1; };
  if (c1_coff >= 0 && overlap(corr_coff, corr_coff + 81L, c1_coff, (long)c1_coff + c)) { set_error("%s: the corr and c1 windows overlap", who); return UDET_ERR_ARG; }
  if (flow && flow == out) {  // in place on a slab: the flow columns are read while the other windows are written
    if (ldf != ldo) { set_error("%s: in place needs ldf == ldo", who); return UDET_ERR_ARG; }
    if (overlap(f_coff, f_coff + 2L, corr_coff, corr_coff + 81L) || (c1_coff >= 0 && overlap(f_coff, f_coff + 2L, c1_coff, (long)c1_coff + c))) {
      set_error("%s: the flow window overlaps the corr / c1 window of the same slab", who);
      return UDET_ERR_ARG;
    }
  }
  UDET_TRY(launch_warp_cost_volume(c1, c2, flow, ldf, f_coff, flow_scale, out, ldo, corr_coff, c1_coff, nullptr, n, h, w, c, (hipStream_t)stream));
  return UDET_OK;
}
}  // extern "C"
// ---- the glue launchers of elementwise.hip, one launch each (tests/test_glue_gpu.py): argument checks, then the launcher ---------------------
namespace {
const long GLUE_MAX_PIXELS = 1L << 31;
bool glue_misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }
// a channel window [coff, coff + c) of a row of ld floats; 0 or the error code (message set)
int glue_window(const char* who, const char* what, int ld, int coff, int c) {
  if (c < 1) { set_error("%s: %s needs at least one channel", who, what); return UDET_ERR_ARG; }
  if (ld < 1 || coff < 0 || (long)coff + c > ld) {
    set_error("%s: channel window of %s outside the buffer (%d+%d of %d)", who, what, coff, c, ld);
    return UDET_ERR_SHAPE;
  }
  return UDET_OK;
}
int glue_pixels(const char* who, long p) {
  if (p < 1) { set_error("%s: pixel count must be positive", who); return UDET_ERR_ARG; }
  if (p >= GLUE_MAX_PIXELS) { set_error("%s: pixel count too large", who); return UDET_ERR_SHAPE; }
  return UDET_OK;
}
int glue_align(const char* who, const char* what, const void* p, unsigned bytes) {
  if (glue_misaligned(p, bytes)) { set_error("%s: %s must be %u-byte aligned", who, what, bytes); return UDET_ERR_ALIGN; }
  return UDET_OK;
}
int glue_resize_check(const char* who, const float* src, int lds, int s_coff, float* dst, int ldd, int d_coff, int n, int h, int w, int oh, int ow,
                      int c) {
  if (!src || !dst || n < 1 || h < 1 || w < 1 || oh < 1 || ow < 1) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_window(who, "the source grid's tensor", lds, s_coff, c));
  UDET_TRY(glue_window(who, "the output grid's tensor", ldd, d_coff, c));
  UDET_TRY(glue_pixels(who, (long)n * h * w));
  UDET_TRY(glue_pixels(who, (long)n * oh * ow));
  UDET_TRY(glue_align(who, "the source tensor", src, 4));
  return glue_align(who, "the output tensor", dst, 4);
}
int glue_share_fold_check(const char* who, const float* buf, long p, int ld, int coff, int c, int copies) {
  if (!buf || copies < 1 || copies > 3) { set_error("%s: bad argument (copies 1..3)", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_window(who, "buf", ld, coff, c));
  UDET_TRY(glue_pixels(who, p * copies));
  const bool v4 = ld % 4 == 0 && coff % 4 == 0 && c % 4 == 0;  // (launch_share_fold takes the float4 form then)
  return glue_align(who, "buf", buf, v4 ? 16 : 4);
}
}  // namespace
extern "C" {
int udet_debug_launch_resize_bilinear_fwd(const float* x, int ldx, int x_coff, int n, int h, int w, float* y, int ldy, int y_coff, int oh, int ow,
                                          int c, float mul, float div, void* stream) {
  const char* who = "debug_launch_resize_bilinear_fwd";
  if (!(div != 0.f)) { set_error("%s: div must not be 0", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_resize_check(who, x, ldx, x_coff, y, ldy, y_coff, n, h, w, oh, ow, c));
  return launch_resize_bilinear_fwd(x, ldx, x_coff, n, h, w, y, ldy, y_coff, oh, ow, c, mul, div, (hipStream_t)stream);
}
int udet_debug_launch_resize_bilinear_bwd(const float* dy, int ldy, int y_coff, int n, int oh, int ow, float* dx, int ldx, int x_coff, int h, int w,
                                          int c, int accumulate, void* stream) {
  const char* who = "debug_launch_resize_bilinear_bwd";
  if (accumulate != 0 && accumulate != 1) { set_error("%s: accumulate must be 0 or 1", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_resize_check(who, dy, ldy, y_coff, dx, ldx, x_coff, n, oh, ow, h, w, c));
  return launch_resize_bilinear_bwd(dy, ldy, y_coff, n, oh, ow, dx, ldx, x_coff, h, w, c, accumulate, (hipStream_t)stream);
}
int udet_debug_launch_share_samples(float* buf, long p, int ld, int coff, int c, int copies, void* stream) {
  UDET_TRY(glue_share_fold_check("debug_launch_share_samples", buf, p, ld, coff, c, copies));
  return launch_share_samples(buf, p, ld, coff, c, copies, (hipStream_t)stream);
}
int udet_debug_launch_fold_samples(float* buf, long p, int ld, int coff, int c, int copies, void* stream) {
  UDET_TRY(glue_share_fold_check("debug_launch_fold_samples", buf, p, ld, coff, c, copies));
  return launch_fold_samples(buf, p, ld, coff, c, copies, (hipStream_t)stream);
}
int udet_debug_launch_emit_du(const float* d, const float* a, float* u, long p, int ld, int coff, int c, int act, float alpha, void* stream) {
  const char* who = "debug_launch_emit_du";
  if (!d || !a || !u || (act != UDET_ACT_NONE && act != UDET_ACT_LEAKY && act != UDET_ACT_ELU)) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_window(who, "d / a / u", ld, coff, c));
  UDET_TRY(glue_pixels(who, p));
  if (glue_misaligned(d, 4) || glue_misaligned(a, 4) || glue_misaligned(u, 4)) { set_error("%s: misaligned pointer", who); return UDET_ERR_ALIGN; }
  return launch_emit_du(d, a, u, p, ld, coff, c, act, alpha, (hipStream_t)stream);
}
int udet_debug_launch_pack_pwc_input(const float* i1, const float* i2, float* x8, long p, void* stream) {
  const char* who = "debug_launch_pack_pwc_input";
  if (!i1 || !i2 || !x8) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_pixels(who, 2 * p));
  if (glue_misaligned(i1, 4) || glue_misaligned(i2, 4)) { set_error("%s: misaligned image pointer", who); return UDET_ERR_ALIGN; }
  UDET_TRY(glue_align(who, "x8", x8, 16));
  return launch_pack_pwc_input(i1, i2, x8, p, (hipStream_t)stream);
}
size_t udet_debug_gen_input_workspace_bytes(int b) { return b < 1 ? 0 : flow_stats_doubles(b) * sizeof(double); }
int udet_debug_launch_gen_input(const float* img, const float* f, float* gin, int b, long hw, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "debug_launch_gen_input";
  if (!img || !f || !gin || b < 1 || b > 65535 || !workspace || workspace_bytes < udet_debug_gen_input_workspace_bytes(b)) {
    set_error("%s: bad argument (workspace: udet_debug_gen_input_workspace_bytes)", who);
    return UDET_ERR_ARG;
  }
  if (hw < 1) { set_error("%s: pixel count must be positive", who); return UDET_ERR_ARG; }
  if (hw >= GLUE_MAX_PIXELS / b) { set_error("%s: pixel count too large", who); return UDET_ERR_SHAPE; }
  UDET_TRY(glue_align(who, "img", img, 4));
  UDET_TRY(glue_align(who, "f", f, 8));
  UDET_TRY(glue_align(who, "gin", gin, 16));
  UDET_TRY(glue_align(who, "workspace", workspace, 8));
  return launch_gen_input(img, f, reinterpret_cast<double*>(workspace), gin, b, hw, (hipStream_t)stream);
}
int udet_debug_launch_mask_rec_inputs(const float* logits, const float* f, float* mask, float* fin, long p, int ncalls, void* stream) {
  const char* who = "debug_launch_mask_rec_inputs";
  if (!logits || !f || !mask || !fin || ncalls < 0 || ncalls > 3) { set_error("%s: bad argument (ncalls 0..3)", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_pixels(who, 3 * p));
  if (glue_misaligned(logits, 4) || glue_misaligned(mask, 4)) { set_error("%s: misaligned pointer", who); return UDET_ERR_ALIGN; }
  UDET_TRY(glue_align(who, "f", f, 8));
  UDET_TRY(glue_align(who, "fin", fin, 16));
  return launch_mask_rec_inputs(logits, f, mask, fin, p, ncalls, (hipStream_t)stream);
}
int udet_debug_launch_pack_imgin(const float* img, float* imgin, long p, int ncalls, void* stream) {
  const char* who = "debug_launch_pack_imgin";
  if (!img || !imgin || ncalls < 0 || ncalls > 3) { set_error("%s: bad argument (ncalls 0..3)", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_pixels(who, 3 * p));
  UDET_TRY(glue_align(who, "img", img, 4));
  UDET_TRY(glue_align(who, "imgin", imgin, 16));
  return launch_pack_imgin(img, imgin, p, ncalls, (hipStream_t)stream);
}
int udet_debug_launch_mask_bwd(const float* dmask, const float* dfin, const float* f, const float* mask, float* dlogits, long p, void* stream) {
  const char* who = "debug_launch_mask_bwd";
  if (!dmask || !dfin || !f || !mask || !dlogits) { set_error("%s: bad argument", who); return UDET_ERR_ARG; }
  UDET_TRY(glue_pixels(who, 2 * p));
  if (glue_misaligned(dmask, 4) || glue_misaligned(mask, 4) || glue_misaligned(dlogits, 4)) { set_error("%s: misaligned pointer", who); return UDET_ERR_ALIGN; }
  UDET_TRY(glue_align(who, "dfin", dfin, 16));
  UDET_TRY(glue_align(who, "f", f, 8));
  return launch_mask_bwd(dmask, dfin, f, mask, dlogits, p, (hipStream_t)stream);
}

void udet_debug_set_tuning(int on) {
  conv_set_tuning(on);
  wgrad_set_tuning(on);
}
}
