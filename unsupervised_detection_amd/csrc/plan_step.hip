// Plan execution, the walk of the step: PWC-Net forward (and its prefetch), generator, the recover net's batched calls, the losses and
// the two backward passes, as calls of the runners (plan_exec.hip) on the lanes (plan_lanes.hip).  Every layer and buffer is addressed
// through Plan::R, the indices plan_build resolved: nothing here formats or looks up a name.
#include "conv_host.h"
#include "elementwise.h"
#include "plan_run.h"

namespace udet {

// ------------------------------------------------------------ PWC-Net ----
static const int PWC_CH[7] = {0, 16, 32, 64, 96, 128, 196};
static const char* const WARP_NAME[7] = {"", "", "warp_costvol2", "warp_costvol3", "warp_costvol4", "warp_costvol5", "warp_costvol6"};

// L0: the lane of the pyramid / estimator / context chain; LH: the 2-channel heads, beside the context network
static int pwc_forward_on(Plan* P, const float* img1, const float* img2, float* ws, const Lane& L0, const Lane& LH) {
  if (!P->pwc_packed) {
    set_error("pwc_forward: call udet_pack_pwc first");
    return UDET_ERR_ARG;
  }
  const Config& c = P->cfg;
  const Resolved& R = P->R;
  const int B = c.batch;
  hipStream_t s = L0.s;
  auto fwd = [&](int layer, int N, const Lane& ln) { return run_fwd(P, P->pwc[layer], N, ws, ln); };
  UDET_TRY(launch_pack_pwc_input(img1, img2, ws + P->buf(R.pwc_x8).off, (long)B * c.in_h * c.in_w, s));
  // siamese feature pyramid on the 2B stacked images (model_pwcnet.py:149-168)
  for (int l = 1; l <= 6; ++l)
    for (int j = 0; j < 3; ++j) UDET_TRY(fwd(R.pwc.pyr[l][j], 2 * B, L0));
  for (int l = 6; l >= 2; --l) {
    const int h = c.in_h >> l, w = c.in_w >> l, C = PWC_CH[l];
    const Buf& cb = P->buf(R.pwc_c[l]);
    const Buf& slab = P->buf(R.pwc_slab[l]);
    const float* c1 = ws + cb.off;
    const float* c2 = ws + cb.off + (size_t)B * h * w * C;
    // warp(c2, up_flow * 20/2^l) -> cost volume -> slab segments [corr 81 | c1] in one launch (model_pwcnet.py:616-623);
    // level 6 correlates c1 with c2 itself and has no c1 / up_flow / up_feat segments
    const bool warped = l != 6;
    const double px = (double)B * h * w;
    prof_begin(P, PROF_CORR, 2.0 * px * 81.0 * C, px * ((warped ? 3.0 * C + 2.0 : 2.0 * C) + 81.0) * 4.0, s, WARP_NAME[l]);
    UDET_TRY(launch_warp_cost_volume(c1, c2, warped ? ws + slab.off : nullptr, slab.ld, 532 + C, 20.0f / (float)(1 << l), ws + slab.off,
                                     slab.ld, 448, warped ? 532 : -1, nullptr, B, h, w, C, s));
    prof_end(P, s);
    for (int i = 0; i < 5; ++i) UDET_TRY(fwd(R.pwc.est[l][i], B, L0));
    // upfeat (the slab) is complete: the flow head and the learned upsampling of upfeat only read it, so they run on
    // their own lane while the context network's six wide convolutions occupy the caller's stream
    order_after(P, L0, LH);
    UDET_TRY(fwd(R.pwc.flow[l], B, LH));
    if (l != 2) UDET_TRY(fwd(R.pwc.up_feat[l], B, LH));
    for (int i = 0; i < 6; ++i) UDET_TRY(fwd(R.pwc.ctx[l][i], B, L0));
    order_after(P, LH, L0);
    UDET_TRY(fwd(R.pwc.ctx[l][6], B, L0));  // + flow (residual operand)
    if (l != 2) UDET_TRY(fwd(R.pwc.up_flow[l], B, L0));
  }
  // flow_pred = resize_bilinear(flow2, x4) * 4   (model_pwcnet.py:641-646)
  const Buf& fr = P->buf(R.pwc_rflow2);
  const Buf& ff = P->buf(R.flow_full);
  return launch_resize_bilinear_fwd(ws + fr.off, fr.ld, 0, B, fr.h, fr.w, ws + ff.off, 2, 0, c.in_h, c.in_w, 2, 4.0f, 1.f, s);
}

int plan_pwc_forward(Plan* P, const float* img1, const float* img2, float* ws, hipStream_t s) {
  P->ev_next = 0;
  if (P->prefetch_pending) (void)hipStreamWaitEvent(s, P->prefetch_ev, 0);  // the prefetch owns the PWC buffers until it is done
  return pwc_forward_on(P, img1, img2, ws, lane_of(P, s, 0), lane_of(P, s, 2));
}

// image -> img_h x img_w  (adversarial_learner.py:87-90)
static int plan_prepare_image(Plan* P, const float* img1, int dst, float* ws, hipStream_t s) {
  const Config& c = P->cfg;
  return launch_resize_bilinear_fwd(img1, 3, 0, c.batch, c.in_h, c.in_w, ws + P->buf(dst).off, 3, 0, c.img_h, c.img_w,
                                    3, 1.f, 1.f, s);
}
// flow -> img_h x img_w, flow / flow_normalizer  (adversarial_learner.py:91-97)
static int plan_prepare_flow(Plan* P, int dst, float* ws, hipStream_t s) {
  const Config& c = P->cfg;
  const Buf& ff = P->buf(P->R.flow_full);
  return launch_resize_bilinear_fwd(ws + ff.off, 2, 0, c.batch, c.in_h, c.in_w, ws + P->buf(dst).off, 2, 0, c.img_h,
                                    c.img_w, 2, 1.f, c.flow_normalizer, s);
}

int plan_prefetch(Plan* P, const float* img1, const float* img2, float* ws, hipStream_t s) {
  const Lane L0 = lane_of(P, s, 0), LC = lane_of(P, s, 4), LH = lane_of(P, s, 5);
  P->in_prefetch = true;  // own event pool: the step's pool is recycled while this work is still in flight
  P->ev_next_prefetch = 0;
  order_after(P, L0, LC);
  int rc = pwc_forward_on(P, img1, img2, ws, LC, LH);
  P->in_prefetch = false;
  UDET_TRY(rc);
  UDET_TRY(plan_prepare_flow(P, P->R.flow_next, ws, LC.s));
  UDET_TRY(plan_prepare_image(P, img1, P->R.image_next, ws, LC.s));
  if (!P->prefetch_ev) (void)hipEventCreateWithFlags(&P->prefetch_ev, hipEventDisableTiming);
  (void)hipEventRecord(P->prefetch_ev, LC.s);
  P->prefetch_pending = true;
  return UDET_OK;
}

// --------------------------------------------------- generator / recover ----
int plan_generator_forward(Plan* P, float* ws, hipStream_t s) {
  const Config& c = P->cfg;
  const long HW = (long)c.img_h * c.img_w;
  const Lane L0 = lane_of(P, s, 0);
  double* part = reinterpret_cast<double*>(ws + P->small_off + 4096);
  UDET_TRY(launch_gen_input(ws + P->buf(P->R.image).off, ws + P->buf(P->R.flow).off, part, ws + P->buf(P->R.gen_in).off, c.batch, HW, s));
  for (const auto& L : P->gen) UDET_TRY(run_fwd(P, L, c.batch, ws, L0));
  return UDET_OK;
}
// the 17 layers alone, from a caller-packed "gen.in" ([image 3 | standardised flow 2 | 0 0 0]): nets.generator_net's own contract
int plan_generator_layers(Plan* P, float* ws, hipStream_t s) {
  const Lane L0 = lane_of(P, s, 0);
  for (const auto& L : P->gen) UDET_TRY(run_fwd(P, L, P->cfg.batch, ws, L0));
  return UDET_OK;
}

static int rec_resize(Plan* P, int src, int dst, int N, float* ws, hipStream_t s) {
  const Buf &a = P->buf(src), &b = P->buf(dst);
  return launch_resize_bilinear_fwd(ws + a.off, a.ld, 0, N, a.h, a.w, ws + b.off, b.ld, 0, b.h, b.w, a.ld, 1.f, 1.f, s);
}
// the source of decoder level k's up-sampled input rec.r{k+1}: conv6 / the next coarser level's slab
static int dec_src(const Resolved& R, int k) { return k == 5 ? R.rec_conv6 : R.rec_concat[k + 1]; }

// The image branch of recover_net (nets.py:57-65): image replicated for the `ncalls` invocations + encoder A.  It
// depends on nothing but the image, so the step runs it beside PWC-Net / the generator.
// encoder A's skip tensors (the slab segments aconv1/2/31/41/51 and aconv6), computed for the B images, fanned out to the other calls' samples
static int share_enc_a_output(Plan* P, const Layer& L, int ncalls, float* ws, hipStream_t s) {
  const Buf& y = P->buf(L.y);
  if (ncalls > 1 && L.y_fanned_out) return launch_share_samples(ws + y.off, (long)P->cfg.batch * y.h * y.w, y.ld, L.y_coff, L.cout, ncalls, s);
  return UDET_OK;
}
// with_layers = false (pair mode, round 6): only the encoder's input is packed here; its nine layers ride in encoder B's launches
// (plan_recover_forward), one pair launch per level
static int plan_rec_image_branch(Plan* P, int ncalls, float* ws, const Lane& ln, bool with_layers = true) {
  const Config& c = P->cfg;
  if (ncalls < 1) return UDET_OK;
  const long Ppix = (long)c.batch * c.img_h * c.img_w;
  // every call sees the same image: encoder A runs once on the B images, then the tensors the decoder reads are fanned out
  UDET_TRY(launch_pack_imgin(ws + P->buf(P->R.image).off, ws + P->buf(P->R.rec_imgin).off, Ppix, 1, ln.s));
  if (!with_layers) return UDET_OK;
  for (int i = 0; i < 9; ++i) {
    const Layer& L = P->rec[P->R.rec.enc[0][i]];
    UDET_TRY(run_fwd(P, L, c.batch, ws, ln));
    UDET_TRY(share_enc_a_output(P, L, ncalls, ws, ln.s));
  }
  P->enc_a_shared = true;
  return UDET_OK;
}

// mask, recover inputs, `ncalls` batched recover invocations (nets.py:45-110; adversarial_learner.py:107-131)
int plan_recover_forward(Plan* P, int ncalls, float* ws, hipStream_t s, bool inputs_prepacked, bool skip_enc_a, bool enc_a_input_packed) {
  const Config& c = P->cfg;
  const Resolved& R = P->R;
  const int B = c.batch, N = ncalls * B;
  const long Ppix = (long)B * c.img_h * c.img_w;
  const Lane L0 = lane_of(P, s, 0);
  if (!inputs_prepacked)
    UDET_TRY(launch_mask_rec_inputs(ws + P->buf(R.gen_a17).off, ws + P->buf(R.flow).off, ws + P->buf(R.mask).off, ws + P->buf(R.rec_fin).off,
                                    Ppix, ncalls, s));
  if (ncalls < 1) return UDET_OK;
  auto enc = [&](int e, int i) -> const Layer& { return P->rec[R.rec.enc[e][i]]; };
  if (!skip_enc_a && pairs_on(P)) {
    // pair mode: level by level, encoder A (the B images -- or, caller-packed inputs, every sample) and encoder B (the N samples of the
    // batched calls) in ONE launch (run_fwd_pair); the image encoder's input was packed by the caller of this function or is packed here
    if (!inputs_prepacked && !enc_a_input_packed) UDET_TRY(plan_rec_image_branch(P, ncalls, ws, L0, false));
    for (int i = 0; i < 9; ++i) {
      const Layer& La = enc(0, i);
      UDET_TRY(run_fwd_pair(P, La, inputs_prepacked ? N : B, enc(1, i), N, ws, L0));
      if (!inputs_prepacked) UDET_TRY(share_enc_a_output(P, La, ncalls, ws, s));
    }
    P->enc_a_shared = !inputs_prepacked;
  } else {
    if (!skip_enc_a) {
      if (inputs_prepacked) {  // caller-packed images may differ between the calls: per-sample encoder
        for (int i = 0; i < 9; ++i) UDET_TRY(run_fwd(P, enc(0, i), N, ws, L0));
        P->enc_a_shared = false;
      } else {
        UDET_TRY(plan_rec_image_branch(P, ncalls, ws, L0));
      }
    }
    for (int i = 0; i < 9; ++i) UDET_TRY(run_fwd(P, enc(1, i), N, ws, L0));
  }
  for (int k = 5; k >= 1; --k) {
    // the up-sampled tensor rec.r{k+1}: the forward of an up-conv level (Layer::upb) reads the ringed low-resolution source instead, and
    // nothing else in the forward or in either backward-data pass reads it -- only the level's filter gradient does, which builds it
    // itself (rec_backward).  Inference, the generator-only schedule steps and the generator-loss pass never pay for it.
    const Layer& dcl = P->rec[R.rec.deconv[k]];
    if (!dcl.upb) UDET_TRY(rec_resize(P, dec_src(R, k), R.rec_r[k + 1], N, ws, s));
    UDET_TRY(run_fwd(P, dcl, N, ws, L0));
    if (k < 5) {
      UDET_TRY(rec_resize(P, R.rec_flow[k + 1], R.rec_rf[k + 1], N, ws, s));
      UDET_TRY(run_fwd(P, P->rec[R.rec.upflow[k]], N, ws, L0));
    }
    UDET_TRY(run_fwd(P, P->rec[R.rec.flow[k]], N, ws, L0));
  }
  const Buf& f1 = P->buf(R.rec_flow[1]);
  return launch_resize_bilinear_fwd(ws + f1.off, f1.ld, 0, N, f1.h, f1.w, ws + P->buf(R.pred).off, 2, 0, c.img_h, c.img_w, 2, 1.f, 1.f, s);
}

// small region layout (floats from small_off): [0,8) losses, [16,16+4B) coef, [256,258) noise flag,
// [1024,1024+5B) sums, [2048,..) per-variable |g| partial sums, [4096,..) flow-stat partials (doubles), [8192,..) loss partials
int plan_losses(Plan* P, float* ws, hipStream_t s) {
  const Config& c = P->cfg;
  float* sm = ws + P->small_off;
  const long HW = (long)c.img_h * c.img_w;
  return launch_losses(ws + P->buf(P->R.flow).off, ws + P->buf(P->R.mask).off, ws + P->buf(P->R.pred).off, HW,
                       c.batch, c.cbn, c.epsilon, (float)(c.img_w * c.img_h * c.batch), sm + 8192, sm, sm + 16, sm + UDET_SMALL_SUMS, s);
}

// join the pending prefetch and move its staging buffers into "flow" / "image"
int plan_prefetch_consume(Plan* P, float* ws, hipStream_t s) {
  if (!P->prefetch_pending) {
    set_error("forward_prefetched: no udet_prefetch_flow is pending");
    return UDET_ERR_ARG;
  }
  (void)hipStreamWaitEvent(s, P->prefetch_ev, 0);
  P->prefetch_pending = false;
  const Buf &fn = P->buf(P->R.flow_next), &in = P->buf(P->R.image_next);
  UDET_HIP(hipMemcpyAsync(ws + P->buf(P->R.flow).off, ws + fn.off, fn.floats() * sizeof(float), hipMemcpyDeviceToDevice, s));
  UDET_HIP(hipMemcpyAsync(ws + P->buf(P->R.image).off, ws + in.off, in.floats() * sizeof(float), hipMemcpyDeviceToDevice, s));
  return UDET_OK;
}

// adversarial_learner.py:83-204.  Lane 1 carries the image branch (image resize, recover encoder A) beside
// PWC-Net and the generator on the caller's stream.
int plan_forward(Plan* P, const float* img1, const float* img2, int ncalls, float* ws, hipStream_t s, bool prefetched) {
  P->ev_next = 0;
  const Lane L0 = lane_of(P, s, 0), LI = lane_of(P, s, 1);
  if (prefetched) {
    UDET_TRY(plan_prefetch_consume(P, ws, s));
    img1 = img2 = nullptr;
  } else if (img1 && P->prefetch_pending) {
    // a stand-alone forward (validation between training steps) while a prefetch is in flight: the prefetch owns the
    // PWC buffers until it is done; its staged result stays valid for the next udet_prefetch_consume
    (void)hipStreamWaitEvent(s, P->prefetch_ev, 0);
  }
  order_after(P, L0, LI);
  if (img1) UDET_TRY(plan_prepare_image(P, img1, P->R.image, ws, LI.s));
  hipEvent_t e_img = nullptr;
  if (LI.s != L0.s) {
    e_img = next_event(P);
    (void)hipEventRecord(e_img, LI.s);
  }
  // pair mode: lane 1 only packs the image encoder's input; its layers run inside encoder B's launches (plan_recover_forward)
  const bool paired = pairs_on(P);
  UDET_TRY(plan_rec_image_branch(P, ncalls, ws, LI, !paired));
  if (img1) {
    UDET_TRY(pwc_forward_on(P, img1, img2, ws, L0, lane_of(P, s, 2)));
    UDET_TRY(plan_prepare_flow(P, P->R.flow, ws, s));
  }
  if (e_img) (void)hipStreamWaitEvent(s, e_img, 0);
  UDET_TRY(plan_generator_forward(P, ws, s));
  order_after(P, LI, L0);
  UDET_TRY(plan_recover_forward(P, ncalls, ws, s, false, !paired, paired));
  if (ncalls == 3) UDET_TRY(plan_losses(P, ws, s));
  return UDET_OK;
}

// ------------------------------------------------------------ backward ----
// Recover decoder/encoder backward for the first N samples of the batched calls, seeded by the family's pred gradient.
// `G` is the gradient-buffer family (Resolved::Grad: "d" recover-loss pass, "e" generator-loss pass); its u_* / enc_du / enc_ux members
// mirror it with dU = gradient * act'(activation), emitted by whichever launch writes a region last, so that the backward-data and
// backward-filter launches of every activated layer read their operand without an act' on load.
// with_wgrad: parameter gradients into g_rec, each on lane LW right where its output gradient is final.
// need_dfin: propagate to the b-encoder input.
static int rec_backward(Plan* P, int N, const Resolved::Grad& G, bool with_wgrad, bool need_dfin, const float* w_rec, float* g_rec, float* ws,
                        const Lane& LD, const Lane& LW, const Lane* LAp = nullptr, const Lane* LWdecp = nullptr) {
  const Config& c = P->cfg;
  const Resolved& R = P->R;
  hipStream_t s = LD.s;
  // (LWdec: the filter-gradient lane of the DECODER layers -- the experiment knob UDET_KNOB_REC_DEC_WGRAD_LANE may send them to another
  // lane than the encoders'; every lane that ran one is joined to LD at the end)
  const Lane LWdec = LWdecp ? *LWdecp : LW;
  auto wgrad_on = [&](const Lane& lw, const Layer& L, int dy, bool is_du, int n) -> int {
    order_after(P, LD, lw);
    return run_wgrad(P, L, n < 0 ? N : n, dy, is_du, w_rec, g_rec, ws, lw);
  };
  auto wgrad = [&](const Layer& L, int dy, bool is_du, int n = -1) -> int { return wgrad_on(LW, L, dy, is_du, n); };
  auto wgrad_dec = [&](const Layer& L, int dy, bool is_du) -> int { return wgrad_on(LWdec, L, dy, is_du, -1); };
  // Encoder A's backward (shared image encoder: B samples, 8 backward-data + 9 filter-gradient launches of 12-25 us each) depends on the
  // decoder's gradients only and touches channel segments no launch of encoder B's chain touches, so it may run as its own chain on
  // another lane (LAp) beside encoder B's instead of inside the recover-loss pass's serial chain; joined to LD at the end.
  const Lane LA = LAp ? *LAp : LD;
  const bool a_own_lane = LA.s != LD.s;
  // shared encoder A (plan_rec_image_branch): its activations exist for the B images only and are identical for every
  // call, so the calls' output gradients are summed (fold) where they enter the encoder and its backward runs on B samples
  const int ncopies = N / c.batch;
  const bool a_shared = P->enc_a_shared && ncopies > 1;
  const Emit none;
  const float LEAK = 0.2f;
  // pred = resize(flow1)
  {
    const Buf& df1 = P->buf(G.flow[1]);
    UDET_TRY(launch_resize_bilinear_bwd(ws + P->buf(G.pred).off, 2, 0, N, c.img_h, c.img_w, ws + df1.off, df1.ld, 0, df1.h, df1.w, 2, 0, s));
  }
  for (int k = 1; k <= 5; ++k) {
    const int dconcat = G.concat[k], uconcat = G.u_concat[k];
    const Layer* fl = &P->rec[R.rec.flow[k]];
    const Layer* dc = &P->rec[R.rec.deconv[k]];
    // concat_k feeds flow_k (and, for k>1, the resize of the next finer level wrote it first).  flow_k's backward-data
    // launch is the last writer of the deconv_k segment [0, Cout(deconv_k)): it emits that segment's dU.
    Emit em;
    em.ubuf = uconcat; em.abuf = fl->x; em.c0 = 0; em.c1 = dc->cout; em.act = ACT_LEAKY; em.alpha = LEAK;
    UDET_TRY(run_dgrad(P, *fl, N, G.flow[k], false, dconcat, 0, k == 1 ? 0 : 1, -1, em, ws, LD));
    if (with_wgrad) UDET_TRY(wgrad_dec(*fl, G.flow[k], false));
    if (k < 5) {
      const Layer* uf = &P->rec[R.rec.upflow[k]];
      if (with_wgrad) UDET_TRY(wgrad_dec(*uf, dconcat, false));  // linear layer: raw gradient
      UDET_TRY(run_dgrad(P, *uf, N, dconcat, false, G.rf[k + 1], 0, 0, -1, none, ws, LD));
      const Buf &drf = P->buf(G.rf[k + 1]), &dfn = P->buf(G.flow[k + 1]);
      UDET_TRY(launch_resize_bilinear_bwd(ws + drf.off, drf.ld, 0, N, drf.h, drf.w, ws + dfn.off, dfn.ld, 0, dfn.h, dfn.w, drf.ld, 0, s));
    }
    if (with_wgrad) {
      if (dc->upb) {  // the filter gradient's X operand (plan_recover_forward skipped it): built on the filter-gradient lane, right here
        order_after(P, LD, LWdec);
        UDET_TRY(rec_resize(P, dec_src(R, k), R.rec_r[k + 1], N, ws, LWdec.s));
      }
      UDET_TRY(wgrad_dec(*dc, uconcat, true));
    }
    if (dc->upb_bwd) {
      UDET_TRY(run_dgrad_upb(P, *dc, N, uconcat, G.p[k + 1], G.concat[k + 1], ws, LD));
      continue;
    }
    const int dr = G.r[k + 1];
    UDET_TRY(run_dgrad(P, *dc, N, uconcat, true, dr, 0, 0, -1, none, ws, LD));
    const Buf& bdr = P->buf(dr);
    const Buf& dsrc = P->buf(k == 5 ? G.conv6 : G.concat[k + 1]);
    UDET_TRY(launch_resize_bilinear_bwd(ws + bdr.off, bdr.ld, 0, N, bdr.h, bdr.w, ws + dsrc.off, dsrc.ld, 0, dsrc.h, dsrc.w,
                                        bdr.ld, 0, s));
  }
  // conv6's output gradient was finalised by the resize adjoint: emit its dU with an elementwise pass (3x6 grid)
  {
    const Buf &d6 = P->buf(G.conv6), &a6 = P->buf(R.rec_conv6), &u6 = P->buf(G.u_conv6);
    UDET_TRY(launch_emit_du(ws + d6.off, ws + a6.off, ws + u6.off, (long)N * d6.h * d6.w, d6.ld, 0, d6.ld, ACT_LEAKY, LEAK, s));
  }
  // encoders, deepest first.  gradient buffers mirror the forward buffers of each conv's output / input.
  if (a_own_lane) order_after(P, LD, LA);  // (everything the decoder wrote)
  const bool pair_enc = pairs_on(P, 1) && with_wgrad && !a_own_lane;
  for (int i = 8; i >= 0; --i) {
    DgradJob job[2];
    int njob = 0;
    for (int e = 0; e < 2; ++e) {  // encoder A, encoder B
      // encoder A sees only the image: without parameter gradients (generator-loss pass) nothing upstream needs it
      if (e == 0 && !with_wgrad) continue;
      const Layer* L = &P->rec[R.rec.enc[e][i]];
      const int du = G.enc_du[e][i];  // dU of this layer's output (emitted by its consumer's dgrad)
      const bool shared = e == 0 && a_shared;
      const int Ne = shared ? c.batch : N;
      const bool own = e == 0 && a_own_lane;
      const Lane& LE = own ? LA : LD;  // this encoder's backward-data chain
      hipStream_t se = LE.s;
      if (shared && i == 8) {  // aconv6 half of conv6: dU was emitted per call above
        const Buf& u = P->buf(du);
        UDET_TRY(launch_fold_samples(ws + u.off, (long)c.batch * u.h * u.w, u.ld, L->y_coff, L->cout, ncopies, se));
      }
      if (with_wgrad) {
        if (own) UDET_TRY(run_wgrad(P, *L, Ne, du, true, w_rec, g_rec, ws, LA));  // (same lane: in chain order, no event)
        else UDET_TRY(wgrad(*L, du, true, Ne));
      }
      if (i == 0) {
        if (e == 1 && need_dfin) UDET_TRY(run_dgrad(P, *L, N, du, true, G.fin, 0, 0, -1, none, ws, LD));
        continue;
      }
      const int dx = G.enc_dx[e][i];
      const bool slab_in = L->x_in_slab;  // slab inputs already hold the decoder's gradient
      // this launch is the last writer of the previous encoder layer's output gradient: emit its dU
      Emit em;
      em.ubuf = G.enc_ux[e][i]; em.abuf = L->x; em.c0 = 0; em.c1 = L->cin; em.act = ACT_LEAKY; em.alpha = LEAK;
      if (shared && slab_in) {  // the decoder's gradient of this skip segment, summed over the calls
        const Buf& d = P->buf(dx);
        UDET_TRY(launch_fold_samples(ws + d.off, (long)c.batch * d.h * d.w, d.ld, L->x_coff, L->cin, ncopies, se));
      }
      if (pair_enc) {  // (both encoders' launches of this level go out together below: everything either of them waits for is enqueued)
        job[njob].L = L; job[njob].N = Ne; job[njob].dy = du; job[njob].dx = dx; job[njob].dx_coff = L->x_coff;
        job[njob].accumulate = slab_in ? 1 : 0; job[njob].em = em;
        ++njob;
        continue;
      }
      UDET_TRY(run_dgrad(P, *L, Ne, du, true, dx, L->x_coff, slab_in ? 1 : 0, -1, em, ws, LE));
    }
    if (njob == 2) UDET_TRY(run_dgrad_pair(P, job[0], job[1], ws, LD));
    else if (njob == 1) UDET_TRY(run_dgrad(P, *job[0].L, job[0].N, job[0].dy, true, job[0].dx, job[0].dx_coff, job[0].accumulate, -1, job[0].em, ws, LD));
  }
  if (a_own_lane) order_after(P, LA, LD);
  if (with_wgrad && LWdec.s != LW.s) order_after(P, LWdec, LD);
  return UDET_OK;
}

// d recover_loss / d FlownetS  (loss_utils.py:18; adversarial_learner.py:230-234)
static int backward_recover(Plan* P, const float* w_rec, float* g_rec, float* ws, const Lane& LD, const Lane& LW, const Lane* LA = nullptr,
                            const Lane* LWdec = nullptr) {
  const Config& c = P->cfg;
  const Resolved& R = P->R;
  const long BHW = (long)c.batch * c.img_h * c.img_w;
  UDET_TRY(launch_rec_loss_bwd(ws + P->buf(R.flow).off, ws + P->buf(R.mask).off, ws + P->buf(R.pred).off, ws + P->buf(R.grad[0].pred).off, BHW,
                               c.cbn, 1.0f / (float)(c.img_w * c.img_h * c.batch), LD.s));
  return rec_backward(P, 3 * c.batch, R.grad[0], true, false, w_rec, g_rec, ws, LD, LW, LA, LWdec);
}

// d generator_loss / d MaskNet  (adversarial_learner.py:224-228): through recover calls 1 and 2 (data gradient only,
// "e" buffers), the mask, then the generator.
static int backward_generator(Plan* P, const float* w_gen, float* g_gen, float* ws, const Lane& LD, const Lane& LW, const Lane* LWlate = nullptr,
                              int nlate = 0) {
  const Config& c = P->cfg;
  const Resolved& R = P->R;
  const int B = c.batch;
  const long HW = (long)c.img_h * c.img_w;
  hipStream_t s = LD.s;
  float* sm = ws + P->small_off;
  UDET_TRY(launch_gen_loss_bwd(ws + P->buf(R.flow).off, ws + P->buf(R.mask).off, ws + P->buf(R.pred).off, sm + 16,
                               ws + P->buf(R.grad[1].pred).off, ws + P->buf(R.d_mask).off, HW, B, c.cbn, s));
  UDET_TRY(rec_backward(P, 2 * B, R.grad[1], false, true, nullptr, nullptr, ws, LD, LD));
  UDET_TRY(launch_mask_bwd(ws + P->buf(R.d_mask).off, ws + P->buf(R.grad[1].fin).off, ws + P->buf(R.flow).off, ws + P->buf(R.mask).off,
                           ws + P->buf(R.gen_d[17]).off, B * HW, s));
  // generator, last layer first.  gen.d{k} = gradient w.r.t. layer k's (post-skip) output; gen.u{k} = that times
  // act'(a_k), emitted by the launch that finalises gen.d{k} (the next layer's backward-data launch or the 2x2 pooling).
  for (int i = 16; i >= 0; --i) {
    const Layer& L = P->gen[i];
    const bool has_act = L.act != ACT_NONE;
    const int dy = has_act ? R.gen_u[i + 1] : R.gen_d[i + 1];
    const Lane& LWi = (LWlate && i < nlate) ? *LWlate : LW;  // (experiment knob: the last `nlate` layers' filter gradients on another lane)
    order_after(P, LD, LWi);
    UDET_TRY(run_wgrad(P, L, B, dy, has_act, w_gen, g_gen, ws, LWi));
    if (i == 0) break;
    // skip gradients: x2 = a6 (+ d11), x1 = a3 (+ d14), x0 = a1 (+ d15)   (nets.py:29,32,33)
    const int res = i == 6 ? R.gen_d[11] : (i == 3 ? R.gen_d[14] : (i == 1 ? R.gen_d[15] : -1));
    const int dx = R.gen_d[i];
    const Layer& Lp = P->gen[i - 1];  // the layer whose output gradient this launch produces
    const int ap = Lp.y2 >= 0 ? Lp.y2 : Lp.y;
    {
      // (up-sampling layers too: their backward-data launch walks the full-resolution dU with stride 2 and produces the gradient of
      // the low-resolution input directly -- see setup_up_dgrad)
      Emit em;
      if (Lp.act != ACT_NONE) { em.ubuf = R.gen_u[i]; em.abuf = ap; em.c0 = 0; em.c1 = L.cin; em.act = Lp.act; em.alpha = Lp.alpha; }
      UDET_TRY(run_dgrad(P, L, B, dy, has_act, dx, 0, 0, res, em, ws, LD));
    }
  }
  return UDET_OK;
}

// Both passes only read the forward state, so with which == 3 they run concurrently: the recover-loss pass on the
// caller's stream (its filter gradients on lane 2), the generator-loss pass on lane 1 (filter gradients on lane 3).
int plan_backward(Plan* P, int which, const float* w_gen, const float* w_rec, float* g_gen, float* g_rec, float* ws, hipStream_t s) {
  P->ev_next = 0;
  const Lane L0 = lane_of(P, s, 0), L1 = lane_of(P, s, 1), L2 = lane_of(P, s, 2), L3 = lane_of(P, s, 3);
  // grad_ev[net]: recorded where that network's flat gradient buffer is final, BEFORE the caller's stream joins the other
  // pass -- a communication stream that waits on it (udet_stream_wait_grads) can exchange the recover gradients while the
  // (longer) generator-loss pass is still running
  auto mark = [&](int net) {
    if (!P->grad_ev[net]) (void)hipEventCreateWithFlags(&P->grad_ev[net], hipEventDisableTiming);
    (void)hipEventRecord(P->grad_ev[net], s);
  };
  if (which == 3) {
    order_after(P, L0, L1);
    const int la = (int)plan_knob(UDET_KNOB_ENC_A_LANE);
    const Lane LA = lane_of(P, s, la > 0 && la < Plan::NLANE ? la : 0);
    // The recover DECODER's filter gradients (deconv / flow / upflow of the five levels, 0.65 ms of large launches, ready from the first
    // 0.1 ms of the pass on) run on lane 3 -- the generator's filter-gradient queue, which has nothing to do until the generator-loss pass
    // has walked the recover net (~0.8 ms) -- instead of lane 2, which shares its hardware queue with the recover-loss pass's own
    // backward-data chain: on one queue they executed strictly behind each other, on two the large filter-gradient launches fill the CUs the
    // chain's many small launches leave idle.  8.89 -> 8.70 ms per step (two boxes, alternating runs); the ENCODERS' filter gradients
    // there as well: 8.96 (they then sit in front of the generator's, which are on the step's critical tail).  profiles/NOTES.md, round 5.
    const int lw = (int)plan_knob(UDET_KNOB_REC_DEC_WGRAD_LANE), le = (int)plan_knob(UDET_KNOB_REC_ENC_WGRAD_LANE);
    const Lane LWD = lane_of(P, s, lw > 0 && lw < Plan::NLANE ? lw : 3);
    const Lane LWE = lane_of(P, s, le > 0 && le < Plan::NLANE ? le : 2);
    UDET_TRY(backward_recover(P, w_rec, g_rec, ws, L0, LWE, la > 0 ? &LA : nullptr, &LWD));
    if (LWE.s != L2.s) order_after(P, LWE, L0);
    // The filter gradients of the generator's first four layers (the LAST ones the generator-loss pass reaches: conv4_downsample ... conv1) run
    // on lane 2 instead of lane 3: they are the tail of the step, and lane 2 -- the recover encoders' filter gradients -- has long drained by
    // then, so the two queues finish the tail side by side.  Round 6 sweep, three runs each on one box (ms per step): 0 layers 8.274,
    // 2: 8.224, 3: 8.218, 4: 8.216, 6: 8.236, 8: 8.278.  (Round 3 measured the same move as a loss -- the kernels behind it were slower then.)
    // (experiment knob, libudet_exp.so only: v > 0 that many layers, v < 0 none)
    const long kl = plan_knob(UDET_KNOB_GEN_WGRAD_LATE);
    const int nlate = kl > 0 ? (int)kl : (kl < 0 ? 0 : 4);
    // the recover gradients are final HERE (rec_backward joined its filter-gradient lanes): their event is recorded before the generator's
    // late filter gradients are enqueued on lane 2, so a communication stream waiting on it still starts under the generator-loss pass
    order_after(P, L2, L0);
    mark(NET_REC);
    UDET_TRY(backward_generator(P, w_gen, g_gen, ws, L1, L3, nlate > 0 ? &L2 : nullptr, nlate));
    order_after(P, L2, L0);
    order_after(P, L1, L0);
    order_after(P, L3, L0);
    mark(NET_GEN);
  } else if (which == 2) {
    UDET_TRY(backward_recover(P, w_rec, g_rec, ws, L0, L2, nullptr, &L3));  // (decoder filter gradients on lane 3's queue, as above)
    order_after(P, L2, L0);
    mark(NET_REC);
  } else {
    UDET_TRY(backward_generator(P, w_gen, g_gen, ws, L0, L3));
    order_after(P, L3, L0);
    mark(NET_GEN);
  }
  return UDET_OK;
}

}  // namespace udet
