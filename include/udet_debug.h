/* Test-only hooks (NOT part of the drop-in surface in udet.h, NOT exported by libudet.so): they live in libudet_debug.so, a
 * small library that links against libudet.so; tools/conv_bench.py and the kernel-family tests load it
 * (unsupervised_detection_amd/_devel.py) to pin one convolution kernel family / tile / split-K mode and to ask which one ran. */
#ifndef UDET_DEBUG_H
#define UDET_DEBUG_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
/* force (bm, bn, split-K) for every convolution launch (bm bit 16: non-specialised kernel, bit 17: LDS-DMA staging,
 * bit 18: tile-resident kernel with bm & 0xffff = tile height, bit 19: self-staging LDS-DMA kernel, bit 20: split-K summed by a
 * second launch, bit 21: split-K summed by the last-arriving workgroup, bit 22 / 23: LDS-DMA kernel with a 3 / 4 stage
 * ring, bit 24: the direct kernels for 2-channel inputs / outputs where the launch is eligible, bit 25: the Winograd F(2x2,3x3) family with
 * bm & 0xffff = variant; ks + 256 r: tail split for r workgroup slots per CU); (0,0,-1) restores.  A forced family a launch is not eligible
 * for, or a tile that is not instantiated, falls back to the built-in choice.  Process-global state: never call it from product code.
 * Pair launches (launch_conv_pair) launch their two problems apart while a configuration is forced, each on that configuration -- unless
 * udet_debug_force_pair(1) is set: then the pair itself runs the forced configuration as far as a pair has one.  Tile: (bm & 0xffff, bn) if it
 * is an instantiated GEMM tile, else the pair heuristic's.  Ring: 3 stages if bit 22 is set, else 2.  Split count: ks & 0xff, clamped to the
 * pair's capacity (both problems' slabs side by side in one scratch region); ks < 0: the heuristic's.  The pair kernels exist only as LDS-DMA
 * kernels with a 2- / 3-stage ring and a second-launch summation: bits 16 - 21 and 23 - 25 and the tail split (ks + 256 r) are ignored there. */
void udet_debug_force_conv(int bm, int bn, int ks);
/* fp16 multiplication (fp32 accumulation) in the single-operator convolution entry points; plans take it from
 * udet_config.conv_fp16.  Process-global state: tests only. */
void udet_debug_conv_fp16(int on);
/* while that hook is on and s > 0: the single-operator backward-data launches scale their gradient operand dy by s on the fp16
 * conversion (f16_xscale = s) and the backward-filter launches theirs (f16_yscale = s; udet_debug_conv2d_backward_filter_ex included),
 * and divide the fp32 accumulators by it -- what a plan does with 4096.  Forward and transposed-forward launches keep scale 1;
 * s <= 0 restores the default (scale 1 everywhere).  Plans are untouched.  Process-global state: tests only. */
void udet_debug_conv_fp16_grad_scale(float s);
/* while on, the first single-op launch of every distinct problem shape times its candidate configurations and caches the winner
 * (what udet_autotune does for a plan); tools/conv_bench.py / wgrad_bench.py use it to measure the tuned kernels stand-alone */
/* filter gradient: nsplit > 0 pins the number of pixel slices (clamped to the workspace capacity), dma = 0 / 1 / 2 the staging variant
 * (register-staged / LDS-DMA with a 2- / 3-stage ring / 3: the Winograd-domain family; -1: as tuned); nsplit = 0 restores the tuned / heuristic choice */
void udet_debug_force_wgrad(int nsplit, int dma);
/* what the most recent filter-gradient launch ran: K slices | variant << 20 (0 register-staged, 1 / 2 LDS-DMA, 3 the Winograd-domain family of
 * conv_wgrad_wino.hip; dma = 3 above forces it where a launch is eligible: 3x3 stride-1, whole 64-channel blocks) */
int udet_debug_last_wgrad(void);
/* the reduction behind that launch: lanes per element SL | CW << 8 (channel width of the fused BN reduction; 0: the plain slab reduction) |
 * rows per block << 16 (fused BN reduction) | 1 << 26 fused BN reduction | 1 << 27 separate BN finalisation (dot + finish launches) |
 * 1 << 28 operand-swapped view | 1 << 29 class-structured view */
int udet_debug_last_wgrad_reduce(void);
/* The filter gradient exactly as the step plan calls it.  x [n,h,w,ldx] and dy [n,oh,ow,ldy] (y_saved like dy; act' on load when given with
 * act != none) carry the layer's channels at x_coff / y_coff (all four multiples of 4; the float4 groups of a window must lie inside the row).
 * gamma != null: BN-folded layer y = gamma*bn_c*(conv + b) + beta -- needs w, b, db, dgamma, dbeta.  up: 0 none, 1 NN x2 fused into the
 * loader (x on the h x w grid, dy on 2h x 2w), 2 the class-structured low-resolution form of the same layer (3x3, BN-folded, dy = dU).
 * workspace: 64-byte aligned; 64 floats + 1024*cout rounded up to 16 + one (bias, filter) slab per split at the padded tile sizes
 * (+ 16*cin*cout + 64*cout + 1024 floats for up = 2); the split count is clamped to what fits. */
int udet_debug_conv2d_backward_filter_ex(const float* x, int ldx, int x_coff, const float* dy, int ldy, int y_coff, const float* y_saved, int act,
                                         float alpha, const float* w, const float* b, const float* gamma, float bn_c, float* dw, float* db,
                                         float* dgamma, float* dbeta, int n, int h, int wd, int cin, int cout, int k, int stride, int dilation,
                                         int up, void* workspace, size_t workspace_bytes, void* stream);
/* plans created after this call: the recover decoder's backward-data pass takes the low-resolution ("up-conv algebra") form on every
 * level whose source has at least `v` pixels (batch included); v < 0 restores the default of 8192.  Tests use 0 on small plans. */
void udet_debug_upb_min_pixels(long v);
void udet_debug_set_tuning(int on);
/* pair launches (two convolutions of the same geometry in ONE launch: the recover net's two encoders, csrc/conv_select.hip launch_conv_pair):
 * on = 1 pairs every compatible couple whatever the tuner thinks -- on the configuration of udet_debug_force_conv where one is forced (tile,
 * ring and split count as described there; neither the pair cache nor the tuner is asked then), 0 never pairs, -1 restores (tuned / heuristic
 * choice; a forced configuration then launches the two apart);
 * udet_debug_last_pair: 1 when the most recent pair call went out as one launch.  udet_debug_last_conv then carries bit 30, the tile, family 2 / 4
 * and the split count that ran (after the clamp to the pair's capacity) */
void udet_debug_force_pair(int on);
int udet_debug_last_pair(void);
/* two forward convolutions (same shape parameters; cin a multiple of 8; batches na / nb; HWIO weights) through the pair launcher;
 * workspace >= (2 * k*k*cin*roundup(cout,4) + 4 Mi + 8192) floats */
int udet_debug_conv2d_pair(const float* xa, const float* xb, const float* wa, const float* wb, const float* ba, const float* bb, float* ya, float* yb,
                           int na, int nb, int h, int w, int cin, int cout, int k, int stride, int dilation, int act, float alpha, void* workspace,
                           size_t workspace_bytes, void* stream);
/* ---- One level of the recover decoder in its low-resolution ("up-conv algebra") form, exactly as a plan runs it --------------------------
 * y = act(conv4x4_SAME(legacy_bilinear_x2(x), w) + bias) computed as the plan computes levels 1-4: the ringed source x^ (upb_ring), four merged
 * 3x3 weight sets (pack modes 9 / 10), one 16-segment launch (forward; `split`: the interior as a four-class launch and the 12 border
 * segments in a second one, legal for cout <= 16 as in a plan) or one 16-segment backward-data launch followed by the ring's adjoint.  The
 * entries call the plan's own table builder, pack jobs and launch code (csrc/plan_exec.hip upb_forward / upb_dgrad); they only lay out a
 * workspace.  They synchronise the stream before they return.
 *   forward:  x [n,h,w,ldx] channels [0,cin) (the weight rows of channels [cin,ldx) are zero: Kc = ldx as in a plan, those values must be
 *             finite); w HWIO [4,4,cin,cout]; bias [cout] or NULL; y [n,2h,2w,ldy] channels [y_coff, y_coff+cout) written, nothing else;
 *             xhat [n,h+2,w+2,ldx] receives the ringed source (all ldx channels).
 *   backward: dy [n,2h,2w,ldy] channels [y_coff, y_coff+kt), kt = cout rounded up to 8 (4 for cout <= 4), read (rows past cout meet zero
 *             weights: finite values); dxhat [n,h+2,w+2,ldx] channels [0,cin) receive the ringed gradient BEFORE the fold (other channels
 *             are read by the fold, not written: initialise them); dx [n,h,w,ldx] = ring adjoint of dxhat (all ldx channels written).
 *             fp16 mode: the gradient operand is scaled by udet_debug_conv_fp16_grad_scale's value (a plan uses 4096).
 * Every argument is checked before the first HIP call: ldx, ldy, y_coff not multiples of 4 -> UDET_ERR_ALIGN; a channel window outside its
 * row (cin > ldx, y_coff + cout > ldy, backward y_coff + kt > ldy) -> UDET_ERR_SHAPE; h < 2 or w < 2 -> UDET_ERR_SHAPE (the forward table
 * has h - 1 interior rows and one last row, the ring fold needs both edges distinct: a 1-pixel-high source is refused, a plan never
 * builds one); NULL pointers, n / cin / cout < 1, an unknown act, split with cout > 16, a workspace that is NULL, not 64-byte aligned or
 * smaller than udet_debug_upconv_lowres_workspace_bytes(ldx, cin, cout) -> UDET_ERR_ARG.
 * Workspace (floats): [0, UDET_DEBUG_UPCONV_WSETS_OFFSET) zero block, ticket counters, device tables; from that offset the four weight
 * sets [4][36][K][ld] (forward: K = ldx, ld = cout rounded up to 4; backward: K = kt, ld = cin rounded up to 4), valid after the call
 * (tests read them back); then the split-K slabs. */
#define UDET_DEBUG_UPCONV_WSETS_OFFSET 6400
size_t udet_debug_upconv_lowres_workspace_bytes(int ldx, int cin, int cout);
int udet_debug_upconv_lowres_fwd(const float* x, int ldx, const float* w, const float* bias, int act, float alpha, float* y, int ldy, int y_coff,
                                 float* xhat, int n, int h, int wd, int cin, int cout, int split, void* workspace, size_t workspace_bytes,
                                 void* stream);
int udet_debug_upconv_lowres_bwd(const float* dy, int ldy, int y_coff, const float* w, float* dx, int ldx, float* dxhat, int n, int h, int wd,
                                 int cin, int cout, void* workspace, size_t workspace_bytes, void* stream);
/* Host only (no HIP call, works without a device): the segment and tap tables build_upb_launches makes for an h x w source (h, w >= 2,
 * else UDET_ERR_SHAPE), forward (backward = 0: taps read the ringed source x^ at segment pixel (qy, qx) + (dy, dx), outputs at
 * (oy + 2 qy, ox + 2 qx)) or backward-data (taps read dU at (2 qy + dy, 2 qx + dx), outputs on the ringed grid at (oy + qy, ox + qx)).
 * seg [nseg][4] = oy, ox, h, w; seg_tap [nseg + 1]; taps [ntaps][3] = dy, dx, widx with widx = weight set * 36 + class * 9 + 3 a + b.
 * taps_cap < ntaps: UDET_ERR_ARG with *ntaps set.  udet_debug_max_segs: UDET_MAX_SEGS of the launcher. */
int udet_debug_upconv_tables(int h, int w, int backward, int* nseg, int* seg, int* seg_tap, int* taps, int taps_cap, int* ntaps);
int udet_debug_max_segs(void);
/* ---- The glue launchers of csrc/elementwise.hip that have no entry point in udet.h, one launch each (tests/test_glue_gpu.py) ----------------
 * udet_debug_<launcher>(...) checks its arguments and calls launch_<launcher> with them; nothing else.  Every check comes before the
 * first HIP call:  a NULL pointer, a count < 1, ncalls outside 0..3, copies outside 1..3, an unknown act, a workspace that is too small
 * -> UDET_ERR_ARG;  ld < 1, coff < 0 or a channel window [coff, coff + c) that does not fit in ld -> UDET_ERR_SHAPE;  a pointer that is not
 * aligned for the vector accesses of its kernel -> UDET_ERR_ALIGN (float2: flow-shaped tensors f; float4: x8, gin, fin, dfin, imgin and, for
 * share / fold, buf whenever ld, coff and c are all multiples of 4 -- the float4 form; double: the gen_input workspace).
 * Layouts (NHWC, P = pixels of the B samples):
 *   resize fwd:  y[n,oh,ow,ldy] channels [y_coff, y_coff + c) = legacy_bilinear(x[n,h,w,ldx] channels [x_coff, x_coff + c)) * mul / div
 *   resize bwd:  dx[n,h,w,ldx] window (+)= adjoint of the same resize applied to dy[n,oh,ow,ldy] window
 *   share / fold: buf [copies * P, ld], window [coff, coff + c): share copies rows [0, P) to rows [k P, (k + 1) P), k = 1..copies - 1;
 *                fold adds those rows onto rows [0, P) in the order (x0 + x1) + x2 and leaves them as they are
 *   emit_du:     u = d * act'(a) on the window of [P, ld] rows, act' taken from the stored output a
 *   pack_pwc_input: x8 [2P, 4] = [i1 + 0.5 | 0] then [i2 + 0.5 | 0];  i1, i2 [P, 3]
 *   gen_input:   gin [B, HW, 8] = [img (3), standardised flow (2), 0, 0, 0];  workspace: udet_debug_gen_input_workspace_bytes(B), 8-byte aligned
 *   mask_rec_inputs: logits [P, 8] (channels 0, 1 read), f [P, 2] -> mask [P], fin [3P, 4] (rows of the first `ncalls` calls written)
 *   pack_imgin:  imgin [ncalls * P, 4] = [img | 0] per call;  mask_bwd: dlogits [P, 8], channels 0 and 1 written */
int udet_debug_launch_resize_bilinear_fwd(const float* x, int ldx, int x_coff, int n, int h, int w, float* y, int ldy, int y_coff, int oh, int ow,
                                          int c, float mul, float div, void* stream);
int udet_debug_launch_resize_bilinear_bwd(const float* dy, int ldy, int y_coff, int n, int oh, int ow, float* dx, int ldx, int x_coff, int h, int w,
                                          int c, int accumulate, void* stream);
int udet_debug_launch_share_samples(float* buf, long p, int ld, int coff, int c, int copies, void* stream);
int udet_debug_launch_fold_samples(float* buf, long p, int ld, int coff, int c, int copies, void* stream);
int udet_debug_launch_emit_du(const float* d, const float* a, float* u, long p, int ld, int coff, int c, int act, float alpha, void* stream);
int udet_debug_launch_pack_pwc_input(const float* i1, const float* i2, float* x8, long p, void* stream);
size_t udet_debug_gen_input_workspace_bytes(int b);
int udet_debug_launch_gen_input(const float* img, const float* f, float* gin, int b, long hw, void* workspace, size_t workspace_bytes, void* stream);
int udet_debug_launch_mask_rec_inputs(const float* logits, const float* f, float* mask, float* fin, long p, int ncalls, void* stream);
int udet_debug_launch_pack_imgin(const float* img, float* imgin, long p, int ncalls, void* stream);
int udet_debug_launch_mask_bwd(const float* dmask, const float* dfin, const float* f, const float* mask, float* dlogits, long p, void* stream);
/* ---- One convolution launch exactly as a step plan builds it (tests/test_conv_epilogue_gpu.py) --------------------------------------------
 * The single-operator entries of udet.h launch dense operands without epilogue options.  This entry takes what a plan's launches carry:
 * channel windows on every operand, the gap map of the packed weights, residual / second output / accumulate / dU emission, act' on load
 * and the two four-class forms of NN x2 + 3x3.  It lays a workspace out, packs the weights with the project's pack code (modes 0 / 1 with
 * k_split / k_gap through either packer of a plan: launch_pack_weights, or with pack_job = 1 a job of launch_pack_jobs; jobs of modes 5 / 6), fills a ConvParams with the project's setup functions and calls launch_conv:
 * nothing else.  udet_debug_force_conv / udet_debug_last_conv / udet_debug_conv_fp16(_grad_scale) act on it as on every launch; a forced
 * Winograd family gets its transformed operand from the packed weights as the single-operator entries do.  The stream is synchronised
 * before the entry returns, and an error of that synchronisation is the entry's (UDET_ERR_HIP).
 *   form 0  forward: conv_setup_fwd on the (h << up) x (wd << up) grid; x [n,h,wd,ldx] (up = 1: read through the loader's NN x2), y on the SAME
 *           output grid; pack mode 0 with the gap map: packed row r < k_split is input channel r, rows [k_split, k_split + k_gap) are zero,
 *           row r beyond is channel r - k_gap.
 *   form 1  backward-data of that convolution (up = 0): x = dy on the forward output grid, y = dx [n,h,wd,ldy]; conv_dgrad_classes launches of
 *           conv_setup_dgrad (stride 2 on an odd grid: one per parity class), pack mode 1, kreal = cout; xa (layout of x) with xact != none:
 *           x *= act'(xa) on load.  fp16 mode: f16_xscale = udet_debug_conv_fp16_grad_scale's value.
 *   form 2  NN x2 + 3x3 SAME as four 2x2 convolutions on the low-resolution grid: setup_up_fwd, pack mode 5; x [n,h,wd,ldx], y [n,2h,2wd,ldy].
 *   form 3  its backward-data pass: setup_up_dgrad, pack mode 6, kreal = cout; x = dU [n,2h,2wd,ldx], y = dx [n,h,wd,ldy].
 * w: HWIO [k,k,cin,cout] in every form.  The launch reads x at channels [x_coff, x_coff + kc): kc is the K extent as a plan sets it (a
 * multiple of 4, >= the real channels cin (forms 0 / 2) or cout (1 / 3) plus the gap); channels past the real ones and inside the gap meet zero
 * weight rows and need only be finite.  With C = cout (forms 0 / 2) or cin (1 / 3) the launch writes y at [y_coff, y_coff + C) and nowhere
 * else, in conv_epilogue's order:  v = act(conv + bias);  y2 <- v;  v += res;  v += old y (accumulate);  y <- v;
 * u <- v * act'(ua) for columns [u_c0, u_c1), act' taken from the stored output (a > 0 ? 1 : leaky alpha / ELU a + 1 / none 1).  res, y2, uo
 * and ua live on y's grid with their own ld / coff (column c of the launch at coff + c).  Backward forms take neither bias nor act.
 * Every argument is checked before the first HIP call:  NULL x / w / y or args, counts < 1, k*k > 49, stride not 1 / 2, an unknown act or
 * form, pack_job not 0 / 1, 4 n h wd >= 2^28, up / gap map outside form 0, xa outside form 1, bias or act on a backward form, uo without ua, a workspace that is NULL, not 64-byte aligned or smaller than
 * udet_debug_conv2d_ex_workspace_bytes(args) -> UDET_ERR_ARG;  ldx, x_coff or kc not multiples of 4, x / xa not 16-byte aligned, any other
 * pointer not 4-byte aligned -> UDET_ERR_ALIGN (the output side may be unaligned: the kernels then take their scalar store paths);  a
 * window outside its row (x_coff + kc > ldx, real channels + gap > kc, y / res / y2 window, [u_c0, u_c1) outside [0, C] or the rows of
 * uo / ua) -> UDET_ERR_SHAPE.
 * Workspace (floats): zero block [0, 64), ticket counters, one pack job, from 4224 the packed weights, then 8 Mi floats of split-K slabs. */
typedef struct udet_debug_conv_ex {
  int form;
  int n, h, wd, cin, cout, k, stride, dilation, up;
  int kc, k_split, k_gap;
  const float* x;
  int ldx, x_coff;
  const float* xa;
  int xact;
  float xalpha;
  const float* w;
  const float* bias;
  int act;
  float alpha;
  float* y;
  int ldy, y_coff;
  const float* res;
  int ldres, res_coff;
  float* y2;
  int ldy2, y2_coff;
  int accumulate;
  float* uo;
  int ldu, u_coff;
  const float* ua;
  int ldua, ua_coff, uact;
  float ualpha;
  int u_c0, u_c1;
  int pack_job; /* forms 0 / 1: 0 pack with launch_pack_weights, 1 with a pack job of mode 0 / 1 (launch_pack_jobs) */
} udet_debug_conv_ex;
size_t udet_debug_conv2d_ex_workspace_bytes(const udet_debug_conv_ex* args);
int udet_debug_conv2d_ex(const udet_debug_conv_ex* args, void* workspace, size_t workspace_bytes, void* stream);
/* Two such problems through the pair launcher, as a lane of a step plan hands a couple over (tests/test_conv_pair_epilogue_gpu.py): every
 * window and option above per problem, separate packed-weight regions, ONE zero block, one set of ticket counters and one split-K scratch
 * region for both (partial and partial_cap are the same in the two parameter blocks), then one call of launch_conv_pair and a
 * synchronisation of the stream, whose error is the entry's.  Only what a plan pairs is accepted: forms 0 and 1 with up = 0, form 1 only where
 * the backward-data pass is ONE launch (stride 2 on an odd grid is one launch per class: UDET_ERR_ARG).  A couple the pair launcher declines
 * (different kc, columns or taps, xa given, fp16 mode, udet_debug_force_pair(0)) is not refused: it goes out as two launches, a first, and
 * udet_debug_last_pair reports 0.  Every argument is checked before the first HIP call: each struct as in udet_debug_conv2d_ex (problem a
 * first); NULL structs, an unaccepted form, a workspace that is NULL, not 64-byte aligned or smaller than
 * udet_debug_conv2d_pair_ex_workspace_bytes(a, b) -> UDET_ERR_ARG.
 * Workspace (floats): zero block, ticket counters and one pack job as above, from 4224 the packed weights of a, then those of b (each rounded up
 * to 64), then 8 Mi floats of split-K slabs. */
size_t udet_debug_conv2d_pair_ex_workspace_bytes(const udet_debug_conv_ex* a, const udet_debug_conv_ex* b);
int udet_debug_conv2d_pair_ex(const udet_debug_conv_ex* a, const udet_debug_conv_ex* b, void* workspace, size_t workspace_bytes, void* stream);
/* ---- A 2-channel head in the GEMM + gather form, exactly as a plan runs it (csrc/plan_exec.hip run_fwd's head branch; tests/test_heads_gpu.py) ----
 * A plan runs every layer plan_build.hip's mark_heads marks (2 output channels over a deep input, k*k*2 <= 64, stride 1 or the transposed 4x4
 * stride-2 form) in three steps wherever the direct kernel of conv_thin.hip is not taken -- in fp32 every head with Kc > 64, in fp16 mode every head:
 *   1. the weights packed with the taps folded into the N axis, wz [kc][ldz], ldz = k*k*2 rounded up to 32, column t*2 + c (pack mode 3; mode 4 for
 *      the transposed form), with the gap map of form 0 above;  pack_job 0: launch_pack_taps_into_n (pack_job_kernel: the frozen PWC-Net weights),
 *      1: a job of launch_pack_jobs (pack_jobs_kernel: the per-step table of the trainable networks);
 *   2. ONE 1x1 convolution (conv_setup_fwd, launch_conv) of x [n,h,wd,ldx] channels [x_coff, x_coff + kc) with wz into z [n,h,wd,ldz];
 *   3. launch_tap_gather on the tap table of conv_setup_fwd(k, k, 1, 1) / conv_setup_dgrad(2h, 2wd, 4, 4, 2, 1): y = bias + the per-tap shifted
 *      reads of z, written to y [n,oh,ow,ldy] channels [y_coff, y_coff + 2) and nowhere else (oh x ow = h x wd; transposed: 2h x 2wd).  An even
 *      ldy and y_coff with an 8-byte aligned y take tap_gather2_kernel (float2 per tap), everything else the generic tap_gather_kernel.
 * This entry lays a workspace out and runs those three steps with the project's own functions; udet_debug_force_conv / udet_debug_last_conv /
 * udet_debug_conv_fp16 act on the GEMM of step 2.  The stream is synchronised before the entry returns, and an error of that synchronisation
 * is the entry's (UDET_ERR_HIP).
 * w: HWIO [k,k,cin,2], transposed: HWOI [4,4,2,cin].  bias [2] or NULL.  kc, k_split, k_gap as in udet_debug_conv_ex (no gap: k_gap = 0,
 * k_split = kc); channels past the real ones and inside the gap meet zero weight rows and need only be finite.
 * Every argument is checked before the first HIP call:  NULL args / x / w / y, counts < 1, k_gap or k_split < 0, transposed or pack_job not
 * 0 / 1, k*k*2 > 64, transposed with k != 4, 4 n h wd >= 2^28, a workspace that is NULL, not 64-byte aligned or smaller than
 * udet_debug_conv2d_head_ex_workspace_bytes(args) -> UDET_ERR_ARG;  ldx, x_coff or kc not multiples of 4, x not 16-byte aligned, w / bias / y not
 * 4-byte aligned -> UDET_ERR_ALIGN;  a window outside its row (x_coff + kc > ldx, y_coff + 2 > ldy) or a gap that does not fit (cin + k_gap > kc,
 * k_split > cin with a gap) -> UDET_ERR_SHAPE.
 * Workspace (floats): zero block [0, 64), ticket counters, one pack job, from 4224 wz (rounded up to 64), then z (rounded up to 64), then
 * 8 Mi floats of split-K slabs. */
typedef struct udet_debug_head_ex {
  int n, h, wd, cin, k;
  int kc, k_split, k_gap;
  const float* x;
  int ldx, x_coff;
  const float* w;
  const float* bias;
  float* y;
  int ldy, y_coff;
  int transposed; /* 0: k x k stride 1; 1: 4x4 stride-2 transpose, output 2h x 2wd */
  int pack_job;   /* 0: launch_pack_taps_into_n; 1: a mode 3 / 4 job through launch_pack_jobs */
} udet_debug_head_ex;
size_t udet_debug_conv2d_head_ex_workspace_bytes(const udet_debug_head_ex* args);
int udet_debug_conv2d_head_ex(const udet_debug_head_ex* args, void* workspace, size_t workspace_bytes, void* stream);
/* ---- launch_warp_cost_volume with the slab arguments of a plan (csrc/plan_step.hip; tests/test_warp_cost_volume_slab_gpu.py) ----------------
 * udet_warp_cost_volume (udet.h) passes a dense flow and a dense 81-column output without a c1 segment.  A plan calls the launcher IN PLACE on a
 * level's slab: out[.., corr_coff + d] = the 81 correlations of c1 with warp(c2, flow * flow_scale), out[.., c1_coff + c] = c1 (c1_coff = -1:
 * no such segment), the flow read at flow[.., f_coff + 0 / 1] of rows ldf wide -- flow == out, ldf == ldo on the slab -- and nothing else of a
 * row written.  flow = NULL: c2 is not warped (level 6).  One launch, not synchronised.
 * Checked before the launch:  NULL c1 / c2 / out or a count < 1 -> UDET_ERR_ARG;  the launcher's own conditions (c a multiple of 4; h, w >= 2
 * with a flow; n h w max(c, ldo) < 2^31 -> UDET_ERR_SHAPE;  c1_coff and ldo multiples of 4 with a c1 segment -> UDET_ERR_ALIGN);  c1 / c2 (out
 * with a c1 segment) not 16-byte aligned -> UDET_ERR_ALIGN;  a window outside its row (corr_coff + 81 > ldo, c1_coff + c > ldo,
 * f_coff + 2 > ldf, negative offsets) -> UDET_ERR_SHAPE;  the corr and c1 windows overlapping, or with flow == out a different ldf / a flow
 * window that overlaps the corr or c1 window -> UDET_ERR_ARG. */
int udet_debug_warp_cost_volume_ex(const float* c1, const float* c2, const float* flow, int ldf, int f_coff, float flow_scale, float* out, int ldo,
                                   int corr_coff, int c1_coff, int n, int h, int w, int c, void* stream);
/* (The experiment knobs of earlier rounds -- lane choices and the work-skipping ablation mask -- are no longer reachable from any library
 * that links against libudet.so: they are compiled out of it.  `make -C unsupervised_detection_amd/csrc exp` builds libudet_exp.so, the same
 * sources with -DUDET_EXPERIMENT, which exports udet_exp_knob(id, value); tools/knob_bench.py is its only user.  csrc/plan.h lists the ids.) */
/* what the most recent convolution launch actually ran: family (0 plain, 1 wave-specialised, 2 LDS-DMA, 3 tile-resident,
 * 4 / 5 LDS-DMA with a 3 / 4 stage ring, 6 self-staging LDS-DMA, 7 / 8 direct kernel for two input / two output channels,
 * 9 Winograd F(2x2,3x3); csrc/conv_select.h) | tile rows << 8 (family 3: tile height, 9: variant) | split count << 20 |
 * folded split-K << 28 | tail split << 29 | pair launch << 30 */
int udet_debug_last_conv(void);
#ifdef __cplusplus
}
#endif
#endif
