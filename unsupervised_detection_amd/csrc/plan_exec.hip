// Plan execution, runners: one layer's forward, backward-data or filter-gradient pass as kernel launches on a lane of the caller's
// choice.  The walk of the step that calls them is plan_step.hip; plan_run.h has the file map.
//
// Reference being replaced: the single sess.run of models/adversarial_learner.py:396 over the graph
// built by build_train_graph (:72-258) / build_test_graph (:450-523).
#include <string.h>

#include "conv_select.h"
#include "elementwise.h"
#include "plan_run.h"

namespace udet {

// algorithmic FLOPs of the convolution a layer stands for (2*MACs, unpadded channels)
static double layer_flops(const Layer& L, int N) {
  const int up = L.up ? 1 : 0;
  double oh, ow;
  if (L.transposed) { oh = 2.0 * L.H; ow = 2.0 * L.W; }
  else { oh = (double)(((L.H << up) + L.stride - 1) / L.stride); ow = (double)(((L.W << up) + L.stride - 1) / L.stride); }
  double taps = (double)L.kh * L.kw;
  if (L.transposed) taps /= 4.0;  // each output pixel of a k4 s2 transposed conv sees 2x2 taps
  return 2.0 * N * oh * ow * L.cout * L.cin * taps;
}
// algorithmic HBM bytes of the same convolution (SURVEY Appendix A's definition: input + output + weights + bias in fp32 if nothing is
// fused; up-sampling layers count their post-resize input, as the appendix does).  The backward-data (dY, dX, W) and backward-filter
// (X, dY, dW) passes of a layer move the same three tensors, so one figure serves all three directions.
static double layer_bytes(const Layer& L, int N) {
  const int up = L.up ? 1 : 0;
  const double ih = (double)(L.H << up), iw = (double)(L.W << up);
  double oh, ow;
  if (L.transposed) { oh = 2.0 * L.H; ow = 2.0 * L.W; }
  else { oh = (double)(((L.H << up) + L.stride - 1) / L.stride); ow = (double)(((L.W << up) + L.stride - 1) / L.stride); }
  return 4.0 * (N * ih * iw * L.cin + N * oh * ow * L.cout + (double)L.kh * L.kw * L.cin * L.cout + L.cout);
}

// timing-only ablation (experiment knob UDET_KNOB_SKIP: libudet_exp.so only, a constant false in the release build; results are wrong on purpose): bit 0 generator filter gradients, 1 recover
// filter gradients, 2 generator backward-data, 3 recover backward-data, 4 PWC-Net forward, 5 generator forward, 6 recover forward
static inline bool skip_launch(int kind, int net) {
  const long k = plan_knob(UDET_KNOB_SKIP);
  if (!k) return false;
  const int bit = kind == 2 ? (net == NET_GEN ? 0 : 1) : (kind == 1 ? (net == NET_GEN ? 2 : 3) : (net == NET_PWC ? 4 : (net == NET_GEN ? 5 : 6)));
  return (k >> bit) & 1;
}

// ------------------------------------------------------------- runners ----
// tf.image.resize_nearest_neighbor(x2) followed by a SAME 3x3 convolution (gen_deconv, convolution_utils.py:58-75) reads, for
// the output pixel (2q+p), up-sampled rows 2q+p-1 .. 2q+p+1 = low-resolution rows {q-1, q, q} (p = 0) or {q, q, q+1} (p = 1): per
// output parity class it is a 2x2 convolution over the low-resolution grid whose weights are sums of the 3x3 taps that read the
// same pixel -- 16 instead of 36 tap products per low-resolution pixel, exactly the arithmetic of the reference up to the order of
// the additions.  Tap t of class (py,px): row offset d(py,ty), column offset d(px,tx), weight matrix class*4 + t.
static inline int up_off(int parity, int t) { return parity == 0 ? (t == 0 ? -1 : 0) : (t == 0 ? 0 : 1); }
// forward: ncls = 4 launch on the low-resolution grid writing the four output sub-lattices
void setup_up_fwd(ConvParams& p, int N, int H, int W) {
  p.N = N; p.H = H; p.W = W;
  p.OH = 2 * H; p.OW = 2 * W; p.OHq = H; p.OWq = W;
  p.osy = p.osx = 2; p.ooy = p.oox = 0; p.isy = p.isx = 1;
  p.ncls = 4; p.ntaps = 16;
  for (int c = 0; c < 4; ++c) {
    p.cls_tap[c] = 4 * c;
    for (int t = 0; t < 4; ++t) {
      ConvTap& tp = p.taps[4 * c + t];
      tp.dy = up_off(c >> 1, t >> 1); tp.dx = up_off(c & 1, t & 1); tp.widx = 4 * c + t;
    }
  }
  p.cls_tap[4] = 16;
}
// backward-data: dX[q] = sum_{class, tap} dU[2(q - d) + p] Weff[class][tap]^T -- a stride-2 walk over the full-resolution dU
void setup_up_dgrad(ConvParams& p, int N, int H, int W) {
  p.N = N; p.H = 2 * H; p.W = 2 * W;
  p.OH = H; p.OW = W; p.OHq = H; p.OWq = W;
  p.osy = p.osx = 1; p.ooy = p.oox = 0; p.isy = p.isx = 2;
  p.ncls = 1; p.ntaps = 16;
  for (int c = 0; c < 4; ++c)
    for (int t = 0; t < 4; ++t) {
      ConvTap& tp = p.taps[4 * c + t];
      tp.dy = (c >> 1) - 2 * up_off(c >> 1, t >> 1); tp.dx = (c & 1) - 2 * up_off(c & 1, t & 1); tp.widx = 4 * c + t;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Recover decoder, levels 1-4 (Layer::upb; backward-data form on the levels with enough source pixels, Layer::upb_bwd): legacy bilinear x2 (out[2j] = x[j], out[2j+1] = (x[j] + x[j+1]) / 2, clamped at the end;
// nets.py:91-110 through tf.image.resize_bilinear) followed by the 4x4 SAME convolution (padding 1 before, 2 after) is, per output
// parity class, a 3x3 convolution over the LOW-resolution source:
//   even rows 2j   read u[2j-1 .. 2j+2] = (x[j-1]+x[j])/2, x[j], (x[j]+x[j+1])/2, x[j+1]      -> x[j-1], x[j], x[j+1] through E
//   odd rows  2j+1 read u[2j .. 2j+3]   = x[j], (x[j]+x[j+1])/2, x[j+1], (x[j+1]+x[j+2])/2    -> x[j], x[j+1], x[j+2] through O
// (E / O: the merge matrices of pack modes 9 / 10, conv_host.hip) -- 9 instead of 16 tap products per output pixel and a source read
// at a quarter of the size.  The borders are exact, not approximated: the source carries a one-pixel ring x^ (upb_ring_kernel) that is
// the NEGATED edge at the top / left (the two halves of the merged even row 0 then cancel to the zero padding of the up-sampled grid)
// and the CLAMPED edge at the bottom / right (the resize's clamp for row 2H-3); only the LAST low-resolution row / column merges
// differently (rows 2H-2, 2H-1 see the clamp and the padding).  Both passes are ONE segmented launch (ConvParams::nseg, 16 segments,
// tables built by plan_build's build_upb_launches): forward = {interior, last row, last column, corner} x 4 parity classes, each
// segment with the weight set of its region; backward-data = the ringed gradient x^[R] collects dU[2R - p - 2a] over the quotient
// pixels q = R - p - a, with the last-row set where q is the last row -- a fixed mix per output row R >= H - 1, hence row groups
// {R < H - 1}, H - 1, H, H + 1 times the same for columns -- followed by the adjoint of the ring (upb_ring_fold), which replaces the
// resize adjoint.  The filter gradient keeps the up-sampled operand.
// ------------------------------------------------------------------------------------------------------------------------------
static void fill_segments(ConvParams& p, const Layer::SegLaunch& g, const ConvTap* tab_dev, int first = 0) {  // segments [first, nseg)
  p.nseg = g.nseg - first;
  memcpy(p.seg, g.seg + first, sizeof(ConvSeg) * p.nseg);
  memcpy(p.seg_tap, g.seg_tap + first, sizeof(int) * (p.nseg + 1));  // (offsets into the whole table)
  p.tap_tab = tab_dev;
}
static void fill_lane(ConvParams& p, const UpbLane& ln, float f16_xscale) {
  p.partial = ln.partial; p.partial_cap = ln.partial_cap;
  p.zero16 = ln.zero16; p.tickets = ln.tickets;
  p.f16 = ln.f16; p.f16_xscale = f16_xscale;
}
// The two passes on OPERANDS (plan_run.h): what run_fwd_upb / run_dgrad_upb below launch for a level of the plan, and what
// libudet_debug's single-layer entry launches for tests/test_upconv_lowres_gpu.py -- one body, so the tests exercise the step's own code.
int upb_forward(const UpbFwd& a, hipStream_t s) {
  const int h = a.h, w = a.w;
  UDET_TRY(launch_upb_ring(a.src, a.ld, a.N, h, w, a.xhat, s));
  ConvParams p;
  memset(&p, 0, sizeof(p));
  p.N = a.N; p.H = h + 2; p.W = w + 2;
  p.OH = 2 * h; p.OW = 2 * w;
  p.osy = p.osx = 2; p.isy = p.isx = 1;
  p.x = a.xhat; p.ldx = a.ld; p.x_coff = 0;
  p.wp = a.wsets; p.Kc = a.Kc; p.ldw = a.ldw; p.bias = a.bias;
  p.y = a.y; p.ldy = a.ldy; p.y_coff = a.y_coff; p.Cout = a.cout;
  p.act = a.act; p.alpha = a.alpha;
  fill_lane(p, a.lane, 1.f);
  const Layer::SegLaunch& F = *a.tab;
  if (a.split) {
    // <= 16 output channels: the tile-resident kernel (conv_tile.hip) is the fast family and takes no segments -- the interior as an
    // ordinary four-class launch (segments 0-3 of the table: weight set 0), the twelve border segments in a second, short launch
    ConvParams q = p;
    q.OHq = h - 1; q.OWq = w - 1;
    q.ncls = 4;
    for (int c = 0; c < 4; ++c) {
      q.cls_tap[c] = q.ntaps;
      for (int t = F.seg_tap[c]; t < F.seg_tap[c + 1]; ++t) q.taps[q.ntaps++] = F.taps[t];
    }
    q.cls_tap[4] = q.ntaps;
    UDET_TRY(launch_conv(q, s));
    fill_segments(p, F, a.tab_dev, 4);
  } else {
    fill_segments(p, F, a.tab_dev);
  }
  return launch_conv(p, s);
}
int upb_dgrad(const UpbBwd& a, hipStream_t s) {
  const int h = a.h, w = a.w;
  ConvParams p;
  memset(&p, 0, sizeof(p));
  p.N = a.N; p.H = 2 * h; p.W = 2 * w;
  p.OH = h + 2; p.OW = w + 2;
  p.osy = p.osx = 1; p.isy = p.isx = 2;
  fill_segments(p, *a.tab, a.tab_dev);
  p.x = a.du; p.ldx = a.lddu; p.x_coff = a.du_coff;
  p.wp = a.wsetsT; p.Kc = a.KcT; p.ldw = a.ldwT; p.kreal = a.cout;
  p.y = a.dxhat; p.ldy = a.ld; p.y_coff = 0; p.Cout = a.cin;
  fill_lane(p, a.lane, a.f16_xscale);
  UDET_TRY(launch_conv(p, s));
  return launch_upb_ring_fold(a.dxhat, a.ld, a.N, h, w, a.dsrc, s);
}

// fp16 mode: gradient operands are multiplied by this power of two before the fp16 conversion (and the fp32 accumulators divided by it)
#define UDET_F16_GRAD_SCALE 4096.f
static void fill_common(Plan* P, ConvParams& p, float* ws, int slot) {
  p.partial = ws + P->scratch_off[slot];
  p.partial_cap = P->scratch_floats;
  p.zero16 = ws + P->small_off + 60000;  // never written after udet_plan_init's memset
  p.tickets = reinterpret_cast<int*>(ws + P->ticket_off) + (size_t)slot * UDET_MAX_TICKETS;
  p.f16 = P->cfg.conv_fp16;
  p.f16_xscale = 1.f;  // (backward-data launches: UDET_F16_GRAD_SCALE, their x operand is a gradient)
}

// ---- operand binders: a buffer (or packed operand) of the workspace into the fields of a parameter block --------------------------
static void bind_x(ConvParams& p, const Buf& b, int coff, float* ws) { p.x = ws + b.off; p.ldx = b.ld; p.x_coff = coff; }
static void bind_y(ConvParams& p, const Buf& b, int coff, int cout, float* ws) { p.y = ws + b.off; p.ldy = b.ld; p.y_coff = coff; p.Cout = cout; }
static void bind_w(ConvParams& p, size_t off, int Kc, int ldw, float* ws) { p.wp = ws + off; p.Kc = Kc; p.ldw = ldw; }
static void bind_res(ConvParams& p, const Buf& b, int coff, float* ws) { p.res = ws + b.off; p.ldres = b.ld; p.res_coff = coff; }
static void bind_y2(ConvParams& p, const Buf& b, float* ws) { p.y2 = ws + b.off; p.ldy2 = b.ld; p.y2_coff = 0; }
static void bind_wino(ConvParams& p, size_t off, int np, float* ws) { p.wino_u = ws + off; p.wino_np = np; }
static void bind_emit(Plan* P, ConvParams& p, const Emit& em, int coff, float* ws) {
  const Buf &bu = P->buf(em.ubuf), &bua = P->buf(em.abuf);
  p.uo = ws + bu.off; p.ldu = bu.ld; p.u_coff = coff;
  p.ua = ws + bua.off; p.ldua = bua.ld; p.ua_coff = coff;
  p.uact = em.act; p.ualpha = em.alpha; p.u_c0 = em.c0; p.u_c1 = em.c1;
}

// the lane-private scratch of fill_common as upb_forward / upb_dgrad take it
static UpbLane upb_lane(Plan* P, float* ws, int slot) {
  ConvParams c;
  fill_common(P, c, ws, slot);
  return UpbLane{c.partial, c.partial_cap, c.zero16, c.tickets, c.f16};
}

static int run_fwd_upb(Plan* P, const Layer& L, int N, float* ws, const Lane& ln) {
  hipStream_t s = ln.s;
  const Buf &bs = P->buf(L.src), &bp = P->buf(L.xhat), &by = P->buf(L.y);
  prof_begin(P, PROF_CONV_FWD, layer_flops(L, N) * 9.0 / 16.0, layer_bytes(L, N), s, L.name.c_str());
  UpbFwd a;
  a.N = N; a.h = bs.h; a.w = bs.w;
  a.src = ws + bs.off; a.xhat = ws + bp.off; a.ld = bp.ld;
  a.wsets = ws + L.wupb_off; a.Kc = L.Kc; a.ldw = L.ldw; a.bias = ws + L.bias_f_off;
  a.y = ws + by.off; a.ldy = by.ld; a.y_coff = L.y_coff; a.cout = L.cout;
  a.act = L.act; a.alpha = L.alpha;
  a.tab = &L.upb_f; a.tab_dev = reinterpret_cast<const ConvTap*>(ws + L.upb_f.tab_off); a.split = L.upb_split;
  a.lane = upb_lane(P, ws, ln.slot);
  UDET_TRY(upb_forward(a, s));
  prof_end(P, s);
  return UDET_OK;
}

int run_dgrad_upb(Plan* P, const Layer& L, int N, int du, int dxhat, int dsrc, float* ws, const Lane& ln) {
  hipStream_t s = ln.s;
  if (skip_launch(1, L.net)) return UDET_OK;
  const Buf &bu = P->buf(du), &bp = P->buf(dxhat), &bd = P->buf(dsrc);
  prof_begin(P, PROF_CONV_DGRAD, layer_flops(L, N) * 9.0 / 16.0, layer_bytes(L, N), s, L.name.c_str());
  UpbBwd a;
  a.N = N; a.h = bd.h; a.w = bd.w;
  a.du = ws + bu.off; a.lddu = bu.ld; a.du_coff = L.y_coff;
  a.wsetsT = ws + L.wupbT_off; a.KcT = L.KcT; a.ldwT = L.ldwT; a.cout = L.cout;
  a.dxhat = ws + bp.off; a.dsrc = ws + bd.off; a.ld = bp.ld; a.cin = L.cin;
  a.tab = &L.upb_b; a.tab_dev = reinterpret_cast<const ConvTap*>(ws + L.upb_b.tab_off);
  a.lane = upb_lane(P, ws, ln.slot);
  a.f16_xscale = UDET_F16_GRAD_SCALE;
  UDET_TRY(upb_dgrad(a, s));
  prof_end(P, s);
  return UDET_OK;
}

// ---- the forward parameter block -----------------------------------------------------------------------------------------------
static bool up_form(const Layer& L) { return L.up && L.wu_off; }  // NN x2 + 3x3 as four 2x2 convolutions (setup_up_fwd)
// launches of a layer's forward in the form fwd_params builds (conv2d_transpose on an odd grid: one per output parity class)
static int fwd_launches(const Layer& L) { return L.transposed ? conv_dgrad_classes(2, 2 * L.H, 2 * L.W) : 1; }
// the forward is ONE plain launch of that block: no transposed / up-sampling / head / up-conv form (what a pair launch can carry)
static bool fwd_is_plain(const Layer& L) { return !L.transposed && !L.up && !L.upb && !L.col2im; }
// the parameter block of forward launch `cls` of a layer; false: that class has no work
static bool fwd_params(Plan* P, const Layer& L, int N, int cls, float* ws, int slot, ConvParams& p) {
  memset(&p, 0, sizeof(p));
  if (L.transposed) {
    if (!conv_setup_dgrad(p, cls, N, 2 * L.H, 2 * L.W, L.kh, L.kw, 2, 1)) return false;
  } else if (up_form(L)) {
    setup_up_fwd(p, N, L.H, L.W);
  } else {
    conv_setup_fwd(p, N, L.H << (L.up ? 1 : 0), L.W << (L.up ? 1 : 0), L.kh, L.kw, L.stride, L.dil);
    p.up_shift = L.up ? 1 : 0;
  }
  bind_x(p, P->buf(L.x), L.x_coff, ws);
  bind_w(p, up_form(L) ? L.wu_off : L.wp_off, L.Kc, L.ldw, ws); p.bias = ws + L.bias_f_off;
  bind_y(p, P->buf(L.y), L.y_coff, L.cout, ws);
  p.act = L.act; p.alpha = L.alpha;
  if (L.res >= 0) bind_res(p, P->buf(L.res), L.res_coff, ws);
  if (L.y2 >= 0) bind_y2(p, P->buf(L.y2), ws);
  if (L.wino_off) bind_wino(p, L.wino_off, L.wino_np, ws);
  fill_common(P, p, ws, slot);
  return true;
}

int run_fwd(Plan* P, const Layer& L, int N, float* ws, const Lane& ln) {
  hipStream_t s = ln.s;
  if (skip_launch(0, L.net)) return UDET_OK;
  // BUFFER CONTRACT (round 5 on): the forward never builds the up-sampled input `rec.r{k+1}` of an up-conv level -- Layer::x of such a
  // layer holds whatever the last recover-loss backward left there (rec_backward rebuilds it for the filter gradient only): these
  // levels run on their ringed low-resolution source only, never through the generic path below.
  if (L.upb) return run_fwd_upb(P, L, N, ws, ln);
  const Buf &bx = P->buf(L.x), &by = P->buf(L.y);
  // (the measurement pass books the multiply-adds the launch executes: 16 of the reference's 36 tap products per low-resolution
  // pixel for the up-sampling layers)
  prof_begin(P, PROF_CONV_FWD, layer_flops(L, N) * (up_form(L) ? 4.0 / 9.0 : 1.0), layer_bytes(L, N), s, L.name.c_str());
  // 2-channel heads: the direct kernel (conv_thin.hip) through the ordinary launch below wherever it is eligible; otherwise
  // (fp16 mode) the GEMM + gather formulation
  bool direct_head = false;
  if (L.col2im && !P->cfg.conv_fp16 && L.Kc <= 64) {  // (deep inputs: the 1x1 GEMM already reads them at the memory rate)
    ConvParams q;
    memset(&q, 0, sizeof(q));
    if (L.transposed) (void)conv_setup_dgrad(q, 0, N, 2 * L.H, 2 * L.W, L.kh, L.kw, 2, 1);
    else conv_setup_fwd(q, N, L.H, L.W, L.kh, L.kw, L.stride, L.dil);
    q.Kc = L.Kc; q.ldw = L.ldw; q.Cout = L.cout;
    if (q.ncls != 4) { q.ncls = 1; q.cls_tap[0] = 0; q.cls_tap[1] = q.ntaps; }
    direct_head = conv_thin_n_ok(q);
  }
  if (L.col2im && !direct_head && fwd_launches(L) == 1) {
    // 2-channel head: the (tap, output channel) pairs become the N axis of ONE 1x1 GEMM over the deep channel axis
    // (every input byte read once, no 16x padding of the MFMA columns per tap), then a gather-sum over the taps
    // (udet_debug_conv2d_head_ex, csrc/devel/api_debug.hip, repeats this sequence for tests/test_heads_gpu.py: carry a change here over there)
    const Buf& bz = P->buf(L.zbuf);
    ConvParams p;
    memset(&p, 0, sizeof(p));
    conv_setup_fwd(p, N, L.H, L.W, 1, 1, 1, 1);
    bind_x(p, bx, L.x_coff, ws);
    bind_w(p, L.wz_off, L.Kc, L.ldz, ws);
    bind_y(p, bz, 0, L.kh * L.kw * L.cout, ws);
    fill_common(P, p, ws, ln.slot);
    UDET_TRY(launch_conv(p, s));
    ConvParams g;
    memset(&g, 0, sizeof(g));
    if (L.transposed) conv_setup_dgrad(g, 0, N, 2 * L.H, 2 * L.W, L.kh, L.kw, 2, 1);
    else conv_setup_fwd(g, N, L.H, L.W, L.kh, L.kw, 1, 1);
    g.H = L.H; g.W = L.W;  // Z lives on the input grid
    g.bias = ws + L.bias_f_off;
    bind_y(g, by, L.y_coff, L.cout, ws);
    UDET_TRY(launch_tap_gather(g, ws + bz.off, bz.ld, s));
    prof_end(P, s);
    return UDET_OK;
  }
  for (int cls = 0; cls < fwd_launches(L); ++cls) {
    ConvParams p;
    if (!fwd_params(P, L, N, cls, ws, ln.slot, p)) continue;
    UDET_TRY(launch_conv(p, s));
    if (P->profiling && (conv_last_config() & 0xff) == FAM_WINO) P->prof.back()->mfma_scale = 4.0 / 9.0;
  }
  prof_end(P, s);
  return UDET_OK;
}

// ---- the backward-data parameter block -----------------------------------------------------------------------------------------
// gradient w.r.t. the LOW-resolution input of an up-sampling layer in one launch (no up-sampled gradient, no pooling)
static bool up_form_T(const Layer& L) { return L.up && L.wuT_off; }
static int dgrad_launches(const Layer& L) { return up_form_T(L) ? 1 : conv_dgrad_classes(L.stride, L.H << (L.up ? 1 : 0), L.W << (L.up ? 1 : 0)); }
// the backward-data pass is ONE plain launch of the block dgrad_params builds (what a pair launch can carry)
static bool dgrad_is_plain(const Layer& L) { return !L.up && !L.upb && !L.transposed && dgrad_launches(L) == 1; }
// the parameter block of backward-data launch `cls` of a layer (arguments: run_dgrad); false: that class has no work
static bool dgrad_params(Plan* P, const Layer& L, int N, int cls, int dy, bool dy_is_du, int dx, int dx_coff, int accumulate, int res,
                         const Emit& em, float* ws, int slot, ConvParams& p) {
  const int up = L.up ? 1 : 0;
  memset(&p, 0, sizeof(p));
  if (up_form_T(L)) setup_up_dgrad(p, N, L.H, L.W);
  else if (!conv_setup_dgrad(p, cls, N, L.H << up, L.W << up, L.kh, L.kw, L.stride, L.dil)) return false;
  bind_x(p, P->buf(dy), L.y_coff, ws);
  if (L.act != ACT_NONE && !dy_is_du) { p.xa = ws + P->buf(L.y2 >= 0 ? L.y2 : L.y).off; p.xact = L.act; p.xalpha = L.alpha; }
  bind_w(p, up_form_T(L) ? L.wuT_off : L.wpT_off, L.KcT, L.ldwT, ws); p.kreal = L.cout;
  bind_y(p, P->buf(dx), dx_coff, L.cin, ws);
  p.accumulate = accumulate;
  if (res >= 0) bind_res(p, P->buf(res), 0, ws);
  if (em.ubuf >= 0) bind_emit(P, p, em, dx_coff, ws);
  if (L.winoT_off && !up_form_T(L)) bind_wino(p, L.winoT_off, L.winoT_np, ws);
  fill_common(P, p, ws, slot);
  p.f16_xscale = UDET_F16_GRAD_SCALE;  // the x operand is a gradient
  return true;
}

int run_dgrad(Plan* P, const Layer& L, int N, int dy, bool dy_is_du, int dx, int dx_coff, int accumulate, int res, const Emit& em, float* ws,
              const Lane& ln) {
  hipStream_t s = ln.s;
  if (skip_launch(1, L.net)) return UDET_OK;
  const Buf &bdy = P->buf(dy), &ba = P->buf(L.y2 >= 0 ? L.y2 : L.y);
  if (ba.ld != bdy.ld) {
    set_error("dgrad(%s): gradient/activation layout mismatch (%d vs %d)", L.name.c_str(), bdy.ld, ba.ld);
    return UDET_ERR_SHAPE;
  }
  prof_begin(P, PROF_CONV_DGRAD, layer_flops(L, N) * (up_form_T(L) ? 4.0 / 9.0 : 1.0), layer_bytes(L, N), s, L.name.c_str());
  for (int cls = 0; cls < dgrad_launches(L); ++cls) {
    ConvParams p;
    if (!dgrad_params(P, L, N, cls, dy, dy_is_du, dx, dx_coff, accumulate, res, em, ws, ln.slot, p)) continue;
    UDET_TRY(launch_conv(p, s));
    if (P->profiling && (conv_last_config() & 0xff) == FAM_WINO) P->prof.back()->mfma_scale = 4.0 / 9.0;
  }
  prof_end(P, s);
  return UDET_OK;
}

int run_wgrad(Plan* P, const Layer& L, int N, int dy, bool dy_is_du, const float* w_flat, float* g_flat, float* ws, const Lane& ln) {
  hipStream_t s = ln.s;
  if (skip_launch(2, L.net)) return UDET_OK;
  const NetParams& np = net_params(L.net);
  const int act_buf = L.y2 >= 0 ? L.y2 : L.y;
  const Buf &bx = P->buf(L.x), &bdy = P->buf(dy), &ba = P->buf(act_buf);
  const int up = L.up ? 1 : 0;
  ConvParams g;
  memset(&g, 0, sizeof(g));
  conv_setup_fwd(g, N, L.H << up, L.W << up, L.kh, L.kw, L.stride, L.dil);
  WgradParams q;
  memset(&q, 0, sizeof(q));
  q.x = ws + bx.off; q.ldx = bx.ld; q.x_coff = L.x_coff;
  q.N = N; q.H = L.H << up; q.W = L.W << up; q.up_shift = up; q.Cin = L.cin;
  q.dy = ws + bdy.off; q.ldy = bdy.ld; q.y_coff = L.y_coff; q.Cout = L.cout;
  if (L.act != ACT_NONE && !dy_is_du) { q.ya = ws + ba.off; q.yact = L.act; q.yalpha = L.alpha; }
  q.OH = g.OH; q.OW = g.OW; q.isy = q.isx = L.stride;
  q.ntaps = g.ntaps;
  memcpy(q.taps, g.taps, sizeof(g.taps));
  q.dw = g_flat + np.p[L.w_idx].offset;
  q.db = g_flat + np.p[L.b_idx].offset;
  q.partial = ws + P->wgrad_off[ln.slot];
  q.zero16 = ws + P->small_off + 60000;
  q.partial_floats = P->wgrad_floats;
  q.f16 = P->cfg.conv_fp16;
  q.f16_yscale = UDET_F16_GRAD_SCALE;
  if (L.g_idx >= 0) {
    q.w = w_flat + np.p[L.w_idx].offset;
    q.b = w_flat + np.p[L.b_idx].offset;
    q.gamma = w_flat + np.p[L.g_idx].offset;
    q.dgamma = g_flat + np.p[L.g_idx].offset;
    q.dbeta = g_flat + np.p[L.be_idx].offset;
    q.bn_c = BN_C;
  }
  if (L.up && L.wu_off && L.g_idx >= 0 && dy_is_du) {
    // NN x2 + 3x3 as four 2x2 convolutions on the low-resolution grid (launch_wgrad_up_T, conv_wgrad.hip)
    prof_begin(P, PROF_CONV_WGRAD, layer_flops(L, N) * 4.0 / 9.0, layer_bytes(L, N), s, L.name.c_str());
    const int rc = launch_wgrad_up_T(q, L.H, L.W, s);
    prof_end(P, s);
    return rc;
  }
  prof_begin(P, PROF_CONV_WGRAD, layer_flops(L, N), layer_bytes(L, N), s, L.name.c_str());
  const int rc = launch_wgrad_T(q, L.kh * L.kw, s);
  if (P->profiling && (wgrad_last_config() >> 20) == 3) P->prof.back()->mfma_scale = 4.0 / 9.0;  // (Winograd-domain family: 16 of 36 products)
  prof_end(P, s);
  return rc;
}

// ---- pair launches (launch_conv_pair, conv_igemm.hip): the recover net's two encoders (nets.py:57-75) -----------------------------
// aconv_k and bconv_k have the same geometry per level, separate weights and (shared image encoder) different batch sizes; their
// forward launches and their backward-data launches are independent of each other.  One launch per level carries both.
// Pair launches are implicit-GEMM launches: the blocks they get carry no Winograd operand.  (Forward blocks lose operand and its
// padded extent, backward-data blocks the operand only -- byte for byte what these runners have always handed over.  Letting
// paired layers keep their Winograd family, ADVICE.md, starts at these two lines.)
int run_fwd_pair(Plan* P, const Layer& La, int Na, const Layer& Lb, int Nb, float* ws, const Lane& ln) {
  if (!pairs_on(P) || !fwd_is_plain(La) || !fwd_is_plain(Lb)) {
    UDET_TRY(run_fwd(P, La, Na, ws, ln));
    return run_fwd(P, Lb, Nb, ws, ln);
  }
  if (skip_launch(0, La.net)) return UDET_OK;
  ConvParams a, b;
  fwd_params(P, La, Na, 0, ws, ln.slot, a);
  fwd_params(P, Lb, Nb, 0, ws, ln.slot, b);
  a.wino_u = b.wino_u = nullptr; a.wino_np = b.wino_np = 0;
  prof_begin(P, PROF_CONV_FWD, layer_flops(La, Na) + layer_flops(Lb, Nb), layer_bytes(La, Na) + layer_bytes(Lb, Nb), ln.s, La.pair_name.c_str());
  const int rc = launch_conv_pair(a, b, ln.s);
  prof_end(P, ln.s);
  return rc;
}
int run_dgrad_pair(Plan* P, const DgradJob& ja, const DgradJob& jb, float* ws, const Lane& ln) {
  ConvParams a, b;
  auto one_launch = [&](const DgradJob& j, ConvParams& p) {
    return dgrad_is_plain(*j.L) && dgrad_params(P, *j.L, j.N, 0, j.dy, true, j.dx, j.dx_coff, j.accumulate, -1, j.em, ws, ln.slot, p);
  };
  if (!pairs_on(P, 1) || !one_launch(ja, a) || !one_launch(jb, b)) {
    UDET_TRY(run_dgrad(P, *ja.L, ja.N, ja.dy, true, ja.dx, ja.dx_coff, ja.accumulate, -1, ja.em, ws, ln));
    return run_dgrad(P, *jb.L, jb.N, jb.dy, true, jb.dx, jb.dx_coff, jb.accumulate, -1, jb.em, ws, ln);
  }
  if (skip_launch(1, ja.L->net)) return UDET_OK;
  a.wino_u = b.wino_u = nullptr;
  prof_begin(P, PROF_CONV_DGRAD, layer_flops(*ja.L, ja.N) + layer_flops(*jb.L, jb.N), layer_bytes(*ja.L, ja.N) + layer_bytes(*jb.L, jb.N), ln.s,
             ja.L->pair_name.c_str());
  const int rc = launch_conv_pair(a, b, ln.s);
  prof_end(P, ln.s);
  return rc;
}

}  // namespace udet
