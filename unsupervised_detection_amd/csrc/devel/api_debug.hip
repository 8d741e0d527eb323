// libudet_debug.so -- the test-only hooks of include/udet_debug.h.  They are NOT part of libudet.so: this small library links
// against it and reaches the (process-global) selection state of the convolution launcher through the internal C++
// interface (conv_host.h).  Only tests/ and tools/ load it; the product path never does.
#include <string.h>

#include "../../../include/udet_debug.h"
#include "../conv_host.h"
#include "../plan.h"

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
void udet_debug_set_tuning(int on) {
  conv_set_tuning(on);
  wgrad_set_tuning(on);
}
}
