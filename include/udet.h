/* libudet.so -- C ABI of the MI355X-native adversarial_learner hot path.
 *
 * The reference (antonilo/unsupervised_detection) has no FFI/plugin layer: its hot path is a
 * TF-1.13 graph assembled by models/adversarial_learner.py:72-258 from models/nets.py,
 * models/PWCNet/{model_pwcnet,core_warp,core_costvol}.py and models/utils/{convolution,loss,flow}_utils.py.  Each entry
 * point below names the reference function (file:line under /root/reference) it replaces.
 *
 * Conventions
 *  - every tensor is float32, NHWC, contiguous unless a channel stride is given; pointers are
 *    DEVICE pointers owned by the caller; the library never allocates device memory;
 *  - convolution weights are HWIO ([kh][kw][cin][cout]) exactly like the TF variables;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *    asynchronously on it; no internal threads, no global state except the thread-local error;
 *  - return value: 0 = ok, <0 = error (UDET_ERR_*); udet_last_error() describes the failure.
 */
#ifndef UDET_H
#define UDET_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UDET_OK 0
#define UDET_ERR_SHAPE (-1)
#define UDET_ERR_ALIGN (-2)
#define UDET_ERR_HIP (-3)
#define UDET_ERR_UNSUPPORTED (-4)
#define UDET_ERR_ARG (-5)
#define UDET_ERR_OVERFLOW (-6) /* conv_fp16 mode: an optimizer update was dropped because its gradients were not finite */

#define UDET_ACT_NONE 0
#define UDET_ACT_LEAKY 1
#define UDET_ACT_ELU 2

int udet_version(void);
const char* udet_last_error(void);

/* ---- single-op entry points (parity tests) -------------------------------------------- */

/* dense_image_warp(image, flow*flow_scale): models/PWCNet/core_warp.py:153-202 (+ :42-150);
 * model_pwcnet.py:240-245,616-617.  c % 4 == 0. */
int udet_warp(const float* image, const float* flow, float flow_scale, float* out, int n, int h, int w, int c,
              void* stream);
/* same, additionally dumping the int32 (floor_y,floor_x) and float (alpha_y,alpha_x) per pixel
 * ([n,h,w,2] each) -- the grid-index math that must be bit-exact (core_warp.py:99-115). */
int udet_warp_debug(const float* image, const float* flow, float flow_scale, float* out, int* floor_yx,
                    float* alpha_yx, int n, int h, int w, int c, void* stream);
/* cost_volume(c1, warp, search_range=4) incl. leaky 0.1: models/PWCNet/core_costvol.py:20-40. out [n,h,w,81] */
int udet_cost_volume(const float* c1, const float* warp, float* out, int n, int h, int w, int c, void* stream);
/* The fused form the step plan launches once per pyramid level (model_pwcnet.py:616-623): warped = dense_image_warp(c2,
 * flow*flow_scale) is produced tile by tile in LDS and correlated with c1 at once -- the warped tensor never exists in HBM.
 * flow == NULL: no warp (level 6 correlates c1 with c2).  corr [n,h,w,81]; warped_dbg: optional [n,h,w,c] dump of the warped
 * features (test hook).  Bit-identical to udet_warp followed by udet_cost_volume. */
int udet_warp_cost_volume(const float* c1, const float* c2, const float* flow, float flow_scale, float* corr, float* warped_dbg,
                          int n, int h, int w, int c, void* stream);

/* tf.image.resize_images(x,[oh,ow]) / tf.image.resize_bilinear, TF-1.13 legacy sampling (align_corners=False, no
 * half-pixel centres): models/adversarial_learner.py:87-90, models/nets.py:108, models/utils/convolution_utils.py:88,
 * data/davis2016_data_utils.py:86-91.  x [n,h,w,c] -> y [n,oh,ow,c]; bwd is its exact adjoint (dy [n,oh,ow,c] -> dx). */
int udet_resize_bilinear_legacy_fwd(const float* x, float* y, int n, int h, int w, int c, int oh, int ow, void* stream);
int udet_resize_bilinear_legacy_bwd(const float* dy, float* dx, int n, int h, int w, int c, int oh, int ow, void* stream);

/* Input stage ("next" row N1): the readers' per-image pipeline in one pass -- optional uint8 -> v/div + add
 * (preprocess_image / preprocess_mask, data/davis2016_data_utils.py:86-99; identical in fbms_/segtrackv2_data_utils.py),
 * flip (data/aug_flips.py:3-16), crop window (tf.random_crop :101-127 / tf.image.central_crop :129-133), TF-1.13
 * legacy bilinear or nearest-neighbour resize (tf.image.resize_images) to [oh,ow].  src [n,h,w,c] uint8 or float32,
 * dst [n,oh,ow,c] float32, params6 device int32 [n][6] = {y0, x0, crop_h, crop_w, flip_lr, flip_td} or NULL. */
int udet_crop_flip_resize(const void* src, int src_is_u8, int nearest, int n, int h, int w, int c, const int* params6,
                          float* dst, int oh, int ow, float div, float add, void* stream);
/* The same input stage over n sources of DIFFERENT sizes in one launch (mixed-resolution FBMS-59 / SegTrackV2 batches).
 * src: packed uint8 or float32 elements; offsets: device int64 [n], element offset of sample i; hw: device int32 [n][2] =
 * {h_i, w_i}; params6: device int32 [n][6] = {y0, x0, crop_h, crop_w, flip_lr, flip_td} relative to sample i's own h_i x w_i,
 * or NULL (whole image, no flip).  Every sample has c channels; dst [n,oh,ow,c] float32.  dst[i] is bit-identical to
 * udet_crop_flip_resize on sample i alone with params6[i].  Only the scalar arguments are checked here: the tables are
 * device memory and must describe windows inside each sample and samples inside src (the Python wrapper validates them). */
int udet_crop_flip_resize_ragged(const void* src, int src_is_u8, int nearest, int n, int c, const long long* offsets,
                                 const int* hw, const int* params6, float* dst, int oh, int ow, float div, float add,
                                 void* stream);

/* Evaluation tail ("next" row N2): the per-sample sums behind compute_boundary_score / disambiguate_forw_back /
 * tf_iou_computation / compute_all_IoU (models/utils/general_utils.py:89-159) and compute_IoU / compute_mae
 * (test_generator.py:19-40).  pred_masks, gt_masks [n,h,w,1] device float32; stats8 [n][8] device doubles =
 * {border sum (two-pixel strips, corners twice), |pred|, |gt|, |pred & gt|, sum pred*|gt-1|, sum (1-pred)*|gt|,
 *  sum (1-pred)*|gt-1|, sum pred*|gt|} with pred = mask > threshold, gt = gt_mask > gt_threshold. */
int udet_mask_stats(const float* pred_masks, const float* gt_masks, int n, int h, int w, float threshold, float gt_threshold,
                    double* stats8, void* stream);

/* DAVIS contour accuracy: the four integers per frame behind the boundary F-measure of the DAVIS-2016 benchmark table.  A
 * restatement of the published measure db_eval_boundary (Perazzi et al., CVPR 2016, and the benchmark's toolkit); the reference has
 * no code for it (its authors ran the external toolkit).  pred_masks, gt_masks [n,h,w,1] device float32, thresholded like
 * udet_mask_stats (seg = mask > threshold, gt = gt_mask > gt_threshold); stats8: the device doubles udet_mask_stats wrote for the
 * same prediction, or NULL: sample i's prediction is complemented when stats8[i][0] / (4w + 4h) >= 0.6 (disambiguate_forw_back, the
 * rule of udet_flow_to_image / udet_overlay_mask; NULL: never).  For each of the two boolean masks seg [h,w]:
 *  - boundary map b [h,w]: with e[y,x] = seg[y,x+1], s[y,x] = seg[y+1,x], se[y,x] = seg[y+1,x+1] (0 where the shift leaves the
 *    mask), b = (seg^e) | (seg^s) | (seg^se); then the last row b[h-1,:] = seg^e, the last column b[:,w-1] = seg^s and the corner
 *    b[h-1,w-1] = 0.  An all-ones and an all-zeros mask both have an empty boundary.
 *  - a boundary pixel of A matches when B has a boundary pixel at squared distance dx^2 + dy^2 <= radius^2, i.e.
 *    A_boundary & binary_dilation(B_boundary, disk(radius)) with zeros outside the image.  The caller derives the radius from the
 *    benchmark's bound_th: radius = bound_th >= 1 ? bound_th : ceil(bound_th * sqrt(h^2 + w^2)), default bound_th = 0.008 (4 at
 *    192 x 384, 8 at 480 x 854, 36 at 2160 x 3840).
 * counts4: device uint64 [n][4] = {n_fg, n_gt, fg_match, gt_match} (boundary pixels of the prediction / of the ground truth, and how
 * many of each match the other), zeroed by the call; exact integers, independent of the order of accumulation.  Precision, recall
 * and F are the host's: (1, 0) when n_fg = 0 < n_gt, (0, 1) when n_gt = 0 < n_fg, (1, 1) when both are 0, else fg_match / n_fg and
 * gt_match / n_gt; F = 2pr / (p + r), 0 when p + r = 0.  bmap_pred, bmap_gt: optional device uint8 [n,h,w] (0 / 1), the two boundary
 * maps themselves.  One launch: bit-packed rows in LDS, tiles of 32 (radius <= 16) or 64 rows x 256 columns plus the halo, no
 * workspace.  1 <= radius <= UDET_BOUNDARY_MAX_RADIUS (one 64-column halo word per side); above: UDET_ERR_UNSUPPORTED; radius < 1, a
 * NULL mask or counts4, n outside 1..65535 or h, w < 1: UDET_ERR_ARG.  Nothing is enqueued on an error. */
#define UDET_BOUNDARY_MAX_RADIUS 63
int udet_boundary_stats(const float* pred_masks, const float* gt_masks, const double* stats8, int n, int h, int w, float threshold,
                        float gt_threshold, int radius, unsigned long long* counts4, unsigned char* bmap_pred, unsigned char* bmap_gt,
                        void* stream);

/* Native-resolution restore of a batch of masks (post_processing/crf_refine.py:84-97 run_crf_original_resolution,
 * post_processing/post_processing.py:32-46): what the benchmarks score -- every frame at its own size, the strip outside the central
 * crop counted as background.  masks: n soft masks [n,mh,mw] device float32, all of one size.  data: packed device uint8, sample i =
 * H_i x W_i bytes at byte offset offsets[i] (device int64 [n]).  tables12: device int32 [n][12] =
 *   {y0, x0, h, w, H, W,  hk, hb, hks,  vk, vb, vks}
 * the box of the patch inside the frame (restore_box: h = int(H * crop), w = int(W * crop), y0 = (H - h) / 2, x0 = (W - w) / 2; the
 * whole frame when crop >= 1), the frame's size, and for the horizontal (mw -> w) and the vertical (mh -> h) pass the int32 offsets
 * into coef of that pass's Pillow coefficients kk [out][ks] (22-bit fixed point) and bounds [out][2] = (first tap, taps), computed
 * by the host exactly as Pillow's Resample.c does (BILINEAR); hk / vk = -1: the pass's output length equals its input length and the
 * pass is skipped (not run with identity weights).  Per sample:
 *   byte = uint8(clip((v - mn) * (255 / cscale), 0, 255) + 0.5) in double, mn / mx over the WHOLE mask, cscale = mx - mn or 1 if 0
 *          (scipy.misc.bytescale as udet_post_bytescale defines it: pil_byte of csrc/pil_resample.h in both);
 *   horizontal pass, uint8 intermediate, vertical pass, each ss = 1 << 21; ss += pixel * kk; clip8(ss >> 22) (udet_post_resample_u8);
 *   the patch lands at (y0, x0), every other byte of the sample is 0; amax[i] (device int32 [n]) = the largest byte of the patch;
 *   binary (optional, NULL: off): packed like data, 1 where (double)byte / (amax + 1e-8) > threshold (a real float64 division,
 *          crf_refine.py:94), else 0.  A constant mask restores to zeros, amax = 0, binary zeros.
 * At most three launches whatever n is (min / max partials; bytescale + both passes + placement on 64 x 16 tiles of each frame, the
 * tile routine of csrc/pil_resample.h, integer atomicMax into amax; the binary mask), many workgroups per sample.  max_h / max_w:
 * the largest H_i / W_i (sizes the grid).
 * workspace: udet_restore_workspace_bytes(n) bytes, 4-byte aligned.  amax is zeroed by the call.  Only the scalars and pointers
 * are checked here (UDET_ERR_ARG; nothing is enqueued on an error): the tables are device memory, and every index the kernels form is
 * bounded by them -- offsets inside data, boxes inside their frames, coefficient windows inside coef and taps inside the mask must
 * hold (native_results.check_restore_tables validates them on the host before every launch). */
size_t udet_restore_workspace_bytes(int n);
int udet_restore_masks_ragged(const float* masks, int n, int mh, int mw, const long long* offsets, const int* tables12, const int* coef,
                              int max_h, int max_w, unsigned char* data, int* amax, unsigned char* binary, double threshold,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Connected components of the restored masks and the choice of one per sample: the step post_processing/post_processing.py:32-35 names
 * ("selects the best detection candidate from the set of predicted connected masks, by measuring overlap with the GT mask") and has no
 * code for; the definition is this project's own.  binary: the packed device uint8 buffer udet_restore_masks_ragged writes (sample i =
 * H_i x W_i bytes at offsets[i], device int64 [n]; any byte != 0 is foreground); hw: device int32 [n][2] = (H_i, W_i); gt: optional,
 * packed the same way (!= 0: annotated).  Per sample:
 *  - a component is a maximal 4- or 8-connected (`connectivity`) set of foreground pixels; its root is the smallest row-major index
 *    y * W + x among its pixels.  labels (optional device int32, same offsets counted in elements): root + 1 on a foreground pixel, 0 on
 *    background.  Ranking a sample's roots in ascending order gives scipy.ndimage.label's numbering.
 *  - area = |C|, inter = |C & gt| (0 without gt), G = |gt| over the sample (0 without gt).
 *  - mode UDET_COMPONENTS_LABEL: nothing is chosen.  UDET_COMPONENTS_LARGEST: the largest area, ties to the smaller root.
 *    UDET_COMPONENTS_BEST_GT (needs gt): the largest IoU with the annotation inter / (area + G - inter), compared by 64-bit integer
 *    cross-multiplication, ties to the larger area, then to the smaller root (no component touches the annotation: the largest one).
 *  - selected (device uint8, packed like binary; may be NULL in mode LABEL): 1 on the chosen component, 0 elsewhere (all 0 for a
 *    sample without foreground, and in mode LABEL).  info: device int64 [n][4] = {components, chosen root or -1, its area, its inter}.
 * Exact integers, identical from run to run.  Five launches whatever n is: union-find in LDS on UDET_COMPONENTS_TILE_H x _TILE_W tiles,
 * unions across tile edges and corners in global memory (agent-scope atomicMin, the larger root always under the smaller), flatten +
 * area / inter per root, partial winners per workgroup, the final reduce + selected.  No workgroup waits for another.  max_h / max_w:
 * the largest H_i / W_i (sizes the grid); total_pixels: the element count of the packed buffers (every offsets[i] + H_i * W_i lies
 * within it); workspace: udet_components_workspace_bytes(total_pixels, n) bytes, 8-byte aligned.  Only the scalars and pointers are
 * checked here (UDET_ERR_ARG -- connectivity not 4 / 8, an unknown mode, BEST_GT without gt, a selecting mode without selected, NULL
 * binary / offsets / hw / info, n outside 1..65535, a short or misaligned workspace; nothing is enqueued on an error): the tables are
 * device memory (native_results.check_component_tables validates offsets, overlap and H * W < 2^31 on the host before every launch). */
#define UDET_COMPONENTS_LABEL 0
#define UDET_COMPONENTS_LARGEST 1
#define UDET_COMPONENTS_BEST_GT 2
#define UDET_COMPONENTS_TILE_H 32
#define UDET_COMPONENTS_TILE_W 64
size_t udet_components_workspace_bytes(size_t total_pixels, int n);
int udet_select_components_ragged(const unsigned char* binary, const unsigned char* gt, int n, const long long* offsets, const int* hw,
                                  int max_h, int max_w, size_t total_pixels, int connectivity, int mode, int* labels,
                                  unsigned char* selected, long long* info, void* workspace, size_t workspace_bytes, void* stream);

/* Every connected component of a ragged batch as a scored box: the detections at native size.  labels: the packed device
 * int32 buffer udet_select_components_ragged writes (mode UDET_COMPONENTS_LABEL, or any mode with `labels`): root + 1 on every foreground
 * pixel, root = the smallest row-major index of its component, 0 on background; a value outside 0..H_i*W_i is background, so no label
 * indexes outside its sample.  score: optional device uint8, packed like labels (the restored soft bytes).  offsets / hw / max_h / max_w
 * / total_pixels as for udet_select_components_ragged.  Per sample, in exact integers, for every component: area; the box y0, x0
 * (inclusive minima) and y1, x1 (exclusive: maxima + 1, the `stop` of scipy.ndimage.find_objects' slices); sum_y and sum_x over its
 * pixels (the numerators of the centroid); score_sum, the sum of its score bytes (0 without score).  The components with area >=
 * min_area are kept and ranked by area, descending, ties to the smaller root (UDET_COMPONENTS_LARGEST's order); the first min(kept, k)
 * go to dets[i][rank][0..8] (device int64 [n][k][UDET_DET_FIELDS]), every other row holds root = -1 and zeros.  counts: device int64
 * [n][3] = {components, kept, rows written}.  Four launches whatever n and the number of components: zero the counters; area per root
 * (one integer atomic per horizontal run of a wave) and the list of kept roots; one workgroup per sample picks the k winners in k
 * rounds; box / sums of the winners (per-workgroup partials in LDS, then one 64-bit integer atomic per touched value).  No host round
 * trip, no workgroup waits for another, no float atomics: identical from run to run and for a sample alone or inside a batch.
 * workspace: udet_component_boxes_workspace_bytes(total_pixels, n, k) bytes (8 per pixel + 8 per sample), 8-byte aligned.
 * UDET_ERR_ARG, nothing enqueued: NULL labels / offsets / hw / dets / counts, n outside 1..65535, max_h or max_w < 1, total_pixels < 1,
 * k outside 1..UDET_DET_MAX_K, min_area < 1, a short or misaligned workspace, labels not 4-byte or dets / counts not 8-byte aligned.  The
 * tables are device memory: the host caller validates them before the launch (native_results.check_component_tables). */
#define UDET_DET_FIELDS 9   /* root, area, y0, x0, y1, x1, sum_y, sum_x, score_sum */
#define UDET_DET_MAX_K 64
size_t udet_component_boxes_workspace_bytes(size_t total_pixels, int n, int k);
int udet_component_boxes_ragged(const int* labels, const unsigned char* score, int n, const long long* offsets, const int* hw,
                                int max_h, int max_w, size_t total_pixels, int min_area, int k,
                                long long* dets, long long* counts, void* workspace, size_t workspace_bytes, void* stream);

/* The frames of the written detections painted onto packed rgb frames, in place: image_rgb is device uint8, sample i = H_i x W_i x 3
 * bytes at byte 3 * offsets[i] (the contract of udet_overlay_native_ragged); dets / counts / k: what udet_component_boxes_ragged wrote,
 * read on the device.  A pixel (y, x) of a box [y0, y1) x [x0, x1) is painted rgb (0xRRGGBB) when y < y0 + t, y >= y1 - t, x < x0 + t or
 * x >= x1 - t, t = thickness in 1..UDET_DRAW_MAX_THICKNESS: the line goes inward (nothing is drawn outside the box), a box narrower
 * than 2 t is filled.  One colour per call, so overlapping boxes write equal bytes and the result does not depend on order; every
 * other byte is untouched.  One launch, one workgroup per (row, sample); a box is clipped to its frame and the row count to k, so
 * nothing is written outside a sample whatever dets and counts hold.  UDET_ERR_ARG, nothing enqueued: a NULL pointer, n outside
 * 1..65535, total_pixels < 1, k outside 1..UDET_DET_MAX_K, thickness outside 1..8, rgb above 0xffffff, misaligned dets / counts. */
#define UDET_DRAW_MAX_THICKNESS 8
int udet_draw_boxes_ragged(unsigned char* image_rgb, int n, const long long* offsets, const int* hw, size_t total_pixels,
                           const long long* dets, const long long* counts, int k, int thickness, unsigned rgb, void* stream);

/* Detections linked into tracks across consecutive frames, by mask overlap.  labels / offsets / hw / max_h / max_w /
 * total_pixels: the packed device int32 labels of n frames as for udet_component_boxes_ragged (a value outside 0..H_i*W_i is background);
 * dets / counts / k: what udet_component_boxes_ragged wrote for those labels, read on the device; rows_i = counts[i][2] clamped to 0..k.
 * link: device int32 [n]; link[i] != 0: frame i continues frame i - 1 (frame 0: the carried frame), link[i] = 0: frame i starts a
 * sequence, so one call may hold several sequences.  The carried frame, the tail of the previous call, is optional: carry_labels (device
 * int32, carry_h x carry_w), carry_dets (its k rows, int64 [k][UDET_DET_FIELDS]), carry_counts (int64 [3], its counts row), carry_ids
 * (int32 [k], the track ids of its rows) and carry_next_id (int32 [1], the next free id of its sequence); absent: every one NULL and
 * carry_h = carry_w = 0, and link[0] is then taken as 0.  A frame is linked when link says so and its predecessor has its H x W;
 * linked (device int32 [n]) reports it as 1, else 0.  For a linked frame c with predecessor p, a < rows_p and b < rows_c, exact integers:
 *  - inter[c][a][b] (device int64 [n][k][k]) = the number of positions where labels_p = root_a + 1 and labels_c = root_b + 1; every other
 *    entry, and every entry of a frame that is not linked, is 0.
 *  - union = area_a + area_b - inter (areas from dets); (a, b) is a candidate when inter > 0 and 1000 inter >= min_iou_permille union.
 *  - greedy matching: repeatedly the candidate with the largest inter / union among rows still free on both sides, compared by 64-bit
 *    cross-multiplication, ties to the smaller a, then to the smaller b.  match[c][b] (device int32 [n][k]) = a, or -1 for an unmatched
 *    row, a row past rows_c and a frame that is not linked.
 *  - ids (device int32 [n][k]), per sequence from 0: a sequence's first frame gives its rows 0 .. rows - 1 in rank order; in a linked
 *    frame a matched row inherits ids[p][a] and the unmatched rows take the next free ids in rank order; rows past rows_c get -1.  A
 *    sequence that continues the carried frame starts from carry_ids and carry_next_id.  A component that vanishes for a frame comes back
 *    under a new id.
 *  - seq_tracks (device int32 [n]): at a sequence's last frame within the call the number of ids handed out so far, elsewhere 0;
 *    next_id (device int32 [1]): that number for the call's last sequence -- the carry_next_id of the call that continues it.
 * Four launches whatever n and the number of sequences and components: zero inter and enter every row's rank at its root in the
 * workspace; the overlap pass over every pixel of every linked frame (a rows_p x rows_c histogram in LDS, one LDS atomic per
 * horizontal run of a wave, then one 64-bit integer atomic per non-zero entry per workgroup); one workgroup per linked frame matches; one
 * wave per sequence walks its frames and hands out the ids.  No host round trip, no workgroup waits for another, integer atomics only:
 * identical from run to run and for a sequence alone or inside a batch.
 * workspace: udet_link_detections_workspace_bytes(total_pixels, n, k, carry_h, carry_w) bytes (4 per pixel, the carried frame's
 * included), 4-byte aligned.  UDET_ERR_ARG, nothing enqueued: a NULL labels / offsets / hw / dets / counts / link or output, n outside
 * 1..65535, max_h or max_w < 1, total_pixels < 1, k outside 1..UDET_DET_MAX_K, min_iou_permille outside 1..1000, a carried frame that is
 * neither absent nor whole, a short or misaligned workspace, an int32 buffer not 4-byte or dets / counts / inter not 8-byte aligned.
 * The tables are device memory: the host caller validates them before the launch (native_results.link_detections); every index a kernel
 * forms is bounded whatever labels, dets, counts and the workspace hold. */
size_t udet_link_detections_workspace_bytes(size_t total_pixels, int n, int k, int carry_h, int carry_w);
int udet_link_detections_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                const int* carry_labels, int carry_h, int carry_w, const long long* carry_dets,
                                const long long* carry_counts, const int* carry_ids, const int* carry_next_id, int min_iou_permille,
                                long long* inter, int* match, int* ids, int* linked, int* seq_tracks, int* next_id, void* workspace,
                                size_t workspace_bytes, void* stream);

/* udet_link_detections_ragged with gap bridging: a row that found no predecessor in the frame before it may continue a
 * track that ended up to max_gap frames earlier (max_gap in 1..UDET_TRACK_MAX_GAP).  labels .. link, min_iou_permille, inter, match, ids,
 * linked, seq_tracks, next_id: as above.  In the place of the carried frame stands a history: the last m <= max_gap + 1 frames of the
 * sequence frame 0 may continue, oldest first, every one hist_h x hist_w -- hist_labels (device int32 [m][hist_h * hist_w]), hist_dets
 * (int64 [m][k][UDET_DET_FIELDS]), hist_counts (int64 [m][3]), hist_ids (int32 [m][k]), hist_open (int32 [m][k], in / out: the `open` the
 * earlier calls wrote for these frames) and hist_next_id (int32 [1]); absent: every pointer NULL and m = hist_h = hist_w = 0.  Frame 0's
 * predecessor is history frame m - 1; a history of another size than frame 0 means frame 0 starts a sequence.
 * Stage 1 is udet_link_detections_ragged's link, unchanged: linked, inter and match are equal to it entry for entry.  Stage 2 runs per
 * sequence, in frame order, for a linked frame c, in exact integers:
 *  - a row a of an earlier frame f of the same sequence is open while no row of any later frame continues it, through stage 1
 *    (match[f + 1][b] = a) or through a bridge; an orphan is a row b < rows_c with match[c][b] = -1.
 *  - gap_inter[c][d - 2][a][b] (device int64 [n][max_gap][k][k]), d = 2 .. max_gap + 1 with frame c - d in c's sequence (no link = 0,
 *    no size change and no sequence start in between; the sequence may reach back into the history) = the number of positions where
 *    labels_{c-d} = root_a + 1 and labels_c = root_b + 1, a < rows_{c-d}, b < rows_c; 0 everywhere else.  The ranks are looked up and
 *    the labels' range is taken as for inter.
 *  - (d, a, b) is a candidate when b is an orphan, (c - d, a) is open, gap_inter > 0 and 1000 gap_inter >= min_iou_permille (area_a +
 *    area_b - gap_inter).  Greedy choice: repeatedly the candidate with the largest gap_inter / union among orphans still free and rows
 *    still open, compared by 64-bit cross-multiplication, ties to the smaller d, then the smaller a, then the smaller b.  The winner
 *    gets back[c][b] = d, prev[c][b] = a, ids[c][b] = ids[c - d][a], and (c - d, a) is closed.
 *  - rows matched in stage 1 have back = 1, prev = match: a stage-1 match is never undone by a better bridge.  The remaining orphans take
 *    the sequence's next free ids in rank order, back = 0, prev = -1, as every row of a sequence's first frame; rows past rows_c get
 *    ids = -1, back = 0, prev = -1 (back, prev: device int32 [n][k]).  Within a frame no id occurs twice.
 *  - open (device int32 [n][k]): 1 for a < rows_c without a successor so far, else 0 -- with ids the state the next call needs.  A
 *    history row that this call continues, by stage 1 or by a bridge, is closed in hist_open in place.
 * Six launches whatever n, the sequences, the components and max_gap: the four phases above with the id walk replaced, the zeroing of
 * gap_inter with the older history frames' ranks, and the gap-overlap pass (the overlap pass once per distance, d on a grid axis).  One
 * workgroup per sequence walks its frames with the open flags, ids and areas of the last max_gap + 1 frames in LDS: per frame at most
 * `orphans` rounds of a block arg-max over the candidates, then the fresh ids by a ballot prefix.  No host round trip, no workgroup
 * waits for another, integer atomics only: identical from run to run and for a sequence alone or inside a batch.
 * workspace: udet_link_detections_gap_workspace_bytes(total_pixels, n, k, max_gap, m, hist_h, hist_w) bytes (4 per pixel of the batch
 * and of the history), 4-byte aligned.  UDET_ERR_ARG, nothing enqueued: everything udet_link_detections_ragged refuses, a NULL gap_inter
 * / back / prev / open, max_gap outside 1..UDET_TRACK_MAX_GAP, m outside 0..max_gap + 1, a history that is neither absent nor whole, a
 * short or misaligned workspace, an int32 buffer not 4-byte or gap_inter / hist_dets / hist_counts not 8-byte aligned.  Every index a
 * kernel forms is bounded whatever labels, dets, counts, ids, open, the history and the workspace hold. */
#define UDET_TRACK_MAX_GAP 8
size_t udet_link_detections_gap_workspace_bytes(size_t total_pixels, int n, int k, int max_gap, int m, int hist_h, int hist_w);
int udet_link_detections_gap_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                    size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                    int max_gap, int m, const int* hist_labels, int hist_h, int hist_w, const long long* hist_dets,
                                    const long long* hist_counts, const int* hist_ids, int* hist_open, const int* hist_next_id,
                                    int min_iou_permille, long long* inter, int* match, int* ids, int* linked, int* seq_tracks,
                                    int* next_id, long long* gap_inter, int* back, int* prev, int* open, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* One packed integer displacement per pixel of a ragged batch from a batch of flow fields of one common size: what the
 * motion link below reads.  flow: device float32 [n][fh][fw][2], (u, v) in flow-grid pixels, row i from frame i to the frame before it
 * (the convention of flow_prev in udet_post_propagate_sequences).  offsets / hw / max_h / max_w / total_pixels: the packed layout of the
 * link entries.  disp: device int32 [total_pixels]; sample i's H x W values at offsets[i]; dx in the low 16 bits, dy in the high 16, both
 * signed.  For pixel (x, y) of a sample H x W, in float32 with every operation rounded once and nothing fused:
 *  - rx = fw / W, ry = fh / H, sx = W / fw, sy = H / fh (one division each, of the integers as floats).
 *  - gx = ((float)x + 0.5f) * rx - 0.5f, clamped to [0, fw - 1]; x0 = (int)floorf(gx), x1 = min(x0 + 1, fw - 1), ax = gx - (float)x0;
 *    gy, y0, y1 and ay from y, ry and fh in the same way.
 *  - per channel, with f00 = flow[i][y0][x0], f01 = flow[i][y0][x1], f10 = flow[i][y1][x0], f11 = flow[i][y1][x1]:
 *    top = f00 + ax * (f01 - f00), bot = f10 + ax * (f11 - f10), val = top + ay * (bot - top).
 *  - dx = rint(u * sx) and dy = rint(v * sy), ties to even; a NaN gives 0; the result is clamped to -32768 .. 32767.
 * One launch, one pixel per lane, a wave on 64 consecutive pixels of one sample; no LDS, no atomics, no workspace; disp is written as
 * aligned 32-bit stores and nothing else is written: identical from run to run and for a sample alone or inside a batch.
 * UDET_ERR_ARG, nothing enqueued: a NULL pointer, n outside 1..65535, max_h or max_w < 1, total_pixels < 1, fh or fw outside 1..32767,
 * flow not 8-byte or disp not 4-byte aligned.  The tables are device memory: the host caller validates them
 * (native_motion.flow_displacements); the taps are clamped to the grid, so nothing indexes outside flow whatever it holds. */
int udet_flow_displacements_ragged(const float* flow, int n, int fh, int fw, const long long* offsets, const int* hw, int max_h, int max_w,
                                   size_t total_pixels, int* disp, void* stream);

/* udet_link_detections_ragged and udet_link_detections_gap_ragged with motion compensation: the predecessor's labels are
 * read where a displacement says each pixel came from.  Every argument is the co-located entry's; disp: device int32 [total_pixels],
 * packed like labels, dx in the low 16 bits and dy in the high 16, both signed (udet_flow_displacements_ragged writes it; any other source
 * will do).  Everything the co-located entries define holds, with one change: inter[c][a][b] counts the positions (x, y) of frame c
 * where labels_c(x, y) = root_b + 1, the source (x + dx, y + dy) with (dx, dy) = disp_c(x, y) lies inside the H x W frame, and
 * labels_p(x + dx, y + dy) = root_a + 1.  A position whose source lies outside the frame contributes nothing; disp of a frame that is not
 * linked is not read; for frame 0 the predecessor is the carried frame (the history's newest frame) and the displacement is frame 0's
 * own, so nothing new is carried between calls.  Areas, the candidate rule, the threshold, the greedy order, the ids and seq_tracks are
 * unchanged: every pixel of b is counted at most once, so inter <= area_b and the union stays positive, while inter may exceed area_a
 * where the displacements map many pixels onto one (inter / union may then exceed 1).  In the gap entry only stage 1 is warped:
 * gap_inter at distances d >= 2 stays co-located.  With disp all zero every output equals the co-located entry's, entry for entry.
 * The launches are the co-located entries' four and six, the overlap pass of stage 1 in its motion form (one more coalesced 32-bit load
 * per pixel, a 2-D bounds test, then the predecessor's label gathered at (y + dy) W + x + dx); the workspaces are those of
 * udet_link_detections_workspace_bytes and udet_link_detections_gap_workspace_bytes.  UDET_ERR_ARG, nothing enqueued: everything the
 * co-located entry refuses, and a NULL or misaligned disp.  Every index a kernel forms is bounded whatever disp holds. */
int udet_link_detections_motion_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                       size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                       const int* carry_labels, int carry_h, int carry_w, const long long* carry_dets,
                                       const long long* carry_counts, const int* carry_ids, const int* carry_next_id, int min_iou_permille,
                                       long long* inter, int* match, int* ids, int* linked, int* seq_tracks, int* next_id, const int* disp,
                                       void* workspace, size_t workspace_bytes, void* stream);
int udet_link_detections_gap_motion_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                           size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                           int max_gap, int m, const int* hist_labels, int hist_h, int hist_w, const long long* hist_dets,
                                           const long long* hist_counts, const int* hist_ids, int* hist_open, const int* hist_next_id,
                                           int min_iou_permille, long long* inter, int* match, int* ids, int* linked, int* seq_tracks,
                                           int* next_id, long long* gap_inter, int* back, int* prev, int* open, const int* disp,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* The boxes of the written detections painted in the colour of their track, in place: the contract of udet_draw_boxes_ragged with two
 * differences.  The colour of row r of sample i is palette[ids[i][r] mod palette_size] (ids: device int32 [n][k], what
 * udet_link_detections_ragged wrote; palette: device uint32 [palette_size], 0xRRGGBB, palette_size in 1..UDET_TRACK_MAX_PALETTE), and a
 * row whose id is -1 is not painted.  Where the lines of several painted boxes cover a pixel the smallest rank wins: a workgroup per
 * (row, sample) skips every pixel that lies on the line of a painted lower-ranked box, so the result does not depend on the order in
 * which workgroups run.  One launch.  UDET_ERR_ARG, nothing enqueued: a NULL pointer, n outside 1..65535, total_pixels < 1, k outside
 * 1..UDET_DET_MAX_K, thickness outside 1..8, palette_size outside 1..64, misaligned dets / counts / ids / palette. */
#define UDET_TRACK_MAX_PALETTE 64
int udet_draw_track_boxes_ragged(unsigned char* image_rgb, int n, const long long* offsets, const int* hw, size_t total_pixels,
                                 const long long* dets, const long long* counts, int k, const int* ids, int thickness,
                                 const unsigned* palette, int palette_size, void* stream);

/* Dense CRF of a ragged batch at each frame's own size: step 2 of post_processing/crf_refine.py:65-108 run_crf_original_resolution
 * (DenseCRF2D + setUnaryEnergy + addPairwiseBilateral(sxy, srgb, rgbim, compat) + inference(iters) on the untouched frame).  Packed
 * layout of the two calls above: sample i = H_i x W_i elements at element offset offsets[i] (device int64 [n]); hw: device int32 [n][2].
 * image_rgb: device uint8, 3 bytes per element (sample i at byte 3 * offsets[i]); unary: device float32 [2][total_pixels], the energies
 * of label 0 and of label 1.  Per sample, exactly the definition of udet_post_dense_crf (Kraehenbuehl & Koltun 2011, one bilateral
 * Potts term, symmetric normalisation; samples do not interact):
 *   k_ij = exp(-(|dp|^2 / sxy^2 + |dI|^2 / srgb^2) / 2)  for |dy|, |dx| <= radius, j != i, j inside the frame (a square window)
 *   n_i = 1 / sqrt(sum_j k_ij + 1e-20);  Q <- softmax(-unary);  iters times: Q <- softmax(-unary + compat * n * K (n * Q))
 * iters = 0 returns softmax(-unary).  q1 (optional, device float32, packed): the marginal of label 1 (Q0 = 1 - Q1).  labels (optional,
 * device uint8, packed like `binary` above, so it feeds udet_select_components_ragged and the scoring kernels unchanged): 1 where
 * Q1 > Q0 strictly (np.argmax: ties to 0).  At least one of the two.  Elements of q1 / labels between the samples are not written.
 * iters + 2 launches of one kernel whatever n is (K 1 -> n; K n with the first softmax; one launch per iteration whose epilogue does
 * the softmax update and writes n * Q1 into the other of two field buffers): 64-column tiles of each frame, the window walked in
 * strips staged in LDS (16 KiB whatever the radius; zeros outside the frame, so the inner loop has no bounds checks), several targets
 * per thread, the exponent as FMAs + one v_exp_f32, the tap j = i excluded by construction.  No atomics, no workgroup waits for
 * another, a fixed summation order per pixel: bit-identical from run to run and between a sample alone and inside a batch.
 * max_h / max_w: the largest H_i / W_i (sizes the grid); workspace: udet_dense_crf_workspace_bytes(total_pixels, n) bytes, 16-byte
 * aligned.  Only the scalars and pointers are checked here (UDET_ERR_ARG -- n outside 1..65535, iters < 0, radius < 1, sxy or
 * srgb <= 0, NULL unary / image_rgb / offsets / hw, both outputs NULL, a short or misaligned workspace; nothing is enqueued on an
 * error): the tables are device memory (native_results.check_crf_tables validates offsets, overlap and H * W < 2^31 on the host before
 * every launch).
 * udet_dense_crf_rows_per_thread: the rows of a tile each thread of that call holds (tiles are 64 columns x 4 times that many rows): the one
 * of 1, 2, 4 with the smallest estimated time max(2, ceil(workgroups of the grid of (max_h, max_w, n) / 256)) x cost per workgroup
 * (52, 66, 120), ties to the larger -- small batches get short tiles, large ones the packed forms; 0 for a bad argument.  The results do not depend on
 * it, bit for bit (tests/test_crf_native_gpu.py runs all three on the same samples).
 * udet_crf_unary_lookup: unary[l][offsets[i] + k] = table[i][l][data[offsets[i] + k]] -- the unary of crf_refine.py:113-121 from the
 * restored bytes of udet_restore_masks_ragged (`data`); table: device float32 [n][2][256], built by the host in float64
 * (post_processing.unary_table). */
size_t udet_dense_crf_workspace_bytes(size_t total_pixels, int n);
int udet_dense_crf_rows_per_thread(int n, int max_h, int max_w);
int udet_dense_crf_ragged(const float* unary, const unsigned char* image_rgb, int n, const long long* offsets, const int* hw, int max_h,
                          int max_w, size_t total_pixels, float sxy, float srgb, float compat, int iters, int radius, float* q1,
                          unsigned char* labels, void* workspace, size_t workspace_bytes, void* stream);
int udet_crf_unary_lookup(const unsigned char* data, const float* table, int n, const long long* offsets, const int* hw, int max_h,
                          int max_w, size_t total_pixels, float* unary, void* stream);

/* Post-processing stage ("next" row N4; post_processing/generate_soft_score_from_buffer.py, crf_refine.py).  The third-party
 * routines those scripts call are absent from the reference tree; each entry point names the routine it restates and the call
 * site that fixes its arguments.  Frames are small (192x384): one workgroup reductions, double accumulation like numpy float64.
 *  - udet_post_border_mean: sanity_check (:116-125): mean over the four two-pixel border strips of n masks [n,h,w] -> out[n].
 *  - udet_post_bytescale / udet_post_resample_u8 / udet_post_place: rectify_pred_mask (:98-114) = scipy.misc.imresize (scipy <=
 *    1.2: bytescale with the window's own min / max + Pillow's 8-bit BILINEAR resampler, Resample.c; kk [n_out][ksize] 22-bit
 *    fixed-point coefficients and bounds [n_out][2] = (first tap, taps) are computed by the host exactly as Pillow does; axis 1 =
 *    horizontal pass, 0 = vertical pass) and the placement on a zero canvas divided by (max + 1e-6).
 *  - udet_post_minmax_norm: pred_mask = (score - min) / (max - min + 1e-6) (:88-90).
 *  - udet_post_remap: cv2.remap(src, flow + pixel grid, None, INTER_LINEAR) with BORDER_CONSTANT 0 (propagate :166-176; OpenCV
 *    remapBilinear: coordinates rounded to 1/32 pixel, float 4-tap weights); flow_uv [h,w,2] = (u, v).
 *  - udet_post_blend: y = a * x / (max(x) + 1e-8) + b * y, optionally followed by y /= (max(y) + 1e-8) (propagate :177-184).
 *  - udet_post_gauss1d: one axis of scipy.ndimage.gaussian_filter (mode 'reflect'), weights k[2r+1] on the device (crf_refine :113).
 *  - udet_post_dense_crf: DenseCRF2D + setUnaryEnergy + addPairwiseBilateral(sxy, srgb, rgbim, compat) + inference(iters)
 *    (crf_refine.py:110-130; Kraehenbuehl & Koltun 2011, mean field with one bilateral Potts term, symmetric normalisation), the
 *    Gaussian kernel evaluated exactly inside a (2*radius+1)^2 window; unary [2,h,w] energies, image_rgb uint8 [h,w,3],
 *    q [2,h,w] marginals out. */
int udet_post_border_mean(const float* s, int n, int h, int w, double* out, void* stream);
int udet_post_bytescale(const double* src, int ld, int y0, int x0, int h, int w, unsigned char* dst, void* stream);
int udet_post_resample_u8(const unsigned char* src, int h, int w, unsigned char* dst, int oh, int ow, const int* kk, const int* bounds,
                          int ksize, int axis, void* stream);
int udet_post_place(const unsigned char* patch, int hh, int ww, int y0, int x0, int h, int w, double* canvas, void* stream);
int udet_post_minmax_norm(const double* score, int n, double* out, void* stream);
int udet_post_remap(const float* src, const float* flow_uv, float* dst, int h, int w, void* stream);
int udet_post_blend(const float* x, float a, float* y, float b, int n, int renorm, void* stream);
int udet_post_gauss1d(const double* src, double* dst, int h, int w, const double* k, int r, int axis, void* stream);
size_t udet_post_crf_workspace_bytes(int h, int w);
int udet_post_dense_crf(const float* unary, const unsigned char* image_rgb, int h, int w, float sxy, float srgb, float compat, int iters,
                        int radius, float* q, void* workspace, size_t workspace_bytes, void* stream);

/* The sequence stage of the same pass, batched (csrc/sequence.hip).
 * udet_post_propagate_sequences: generate_soft_score_from_buffer.py propagate :127-231 for n_seq sequences and both directions, given the
 * flows.  The frames of all sequences lie in one array of total_frames frames; sequence s is frames seq_first[s] .. seq_first[s] +
 * seq_len[s] - 1 (device int32 [n_seq]; lengths >= 1, ranges inside the array and disjoint -- device memory, so validated by the host
 * caller before anything is launched: post_processing.check_sequence_tables).  masks [total][h][w]; flow_prev / flow_next [total][h][w][2]
 * = (u, v) from frame k to frame k - 1 / k + 1 (the entry of a sequence's first / last frame is not read); avg_f / avg_b [total][h][w].
 * Per sequence: avg_f[first] = mask[first], then for k = first + 1 ..: with s2 = remap(mask[k-1], flow_prev[k]) and ra = remap(avg_f[k-1],
 * flow_prev[k]) (udet_post_remap), avg_f[k] = r / den(max r), r = w_s * (s2 / den(max s2)) + w_r * (ra / den(max ra)), den(m) =
 * (float)((double)m + 1e-8) -- operation for operation what udet_post_remap x 2 + udet_post_blend x 2 compute per step (one set of
 * device functions, csrc/post_remap.h): bit-identical to that chain.  avg_b likewise from the last frame down along flow_next.  w_s and
 * w_r are the two float32 weights as udet_post_blend takes them (the reference: float32(1 - 0.85) and float32(0.85); 1 - w_r is rounded
 * from the caller's double, so it cannot be derived from the float32 w_r here).
 * Two launches whatever the batch: (a) max s2 of every step, which does not depend on the recurrence -- workgroups (slice, sequence,
 * direction), 32 partial maxima per step into the workspace, no atomics; (b) one workgroup of 1024 threads per (sequence, direction)
 * that walks the frames: avg[k] is the state (a step gathers from avg[k -+ 1]), barriers of the workgroup only, no workgroup waits for
 * another.  max is exact in any order and everything else is per element: bit-identical from run to run and between a sequence alone
 * and inside a batch.  workspace: udet_post_propagate_workspace_bytes(total_frames, n_seq) bytes (256 per frame; no per-pixel
 * intermediate), 16-byte aligned.  UDET_ERR_ARG, nothing enqueued: n_seq outside 1..65535, h, w or total_frames < 1, h * w >= 2^31, a NULL
 * pointer, a flow array that is not 8-byte aligned, masks / avg_f / avg_b not three different buffers, a short or misaligned workspace.
 * udet_post_select_unary: crf_refine.py:40-52 and :113-121 for n frames of hw pixels each (pred, avg_f, avg_b, gt: [n][hw]).  Launch 1,
 * a workgroup per (frame, candidate): scores[n][3] = sum(p * gt) / (sum(p) + 1e-8), the product in float32, the sums in double in a
 * fixed order.  Launch 2, a workgroup per frame: choice[n] by the reference's rule on (m, f, b) = scores[i] (m >= f and m >= b: 0; else
 * f >= m and f >= b: 1; else 2), soft[n][hw] = the chosen candidate, U = clamp((double)p / (max p + 1e-8), 1e-6, 1 - 1e-6), unary[0] =
 * (float)-log(1 - U), unary[1] = (float)-log(U) in double, unary [2][n * hw] with frame i at element i * hw of each half -- the packed
 * layout of udet_dense_crf_ragged with offsets[i] = i * hw.  The Gaussian of crf_refine.py:113 is the identity here (radius int(4 *
 * gauss_k + 0.5) = 0, the reference's 0.1).  UDET_ERR_ARG, nothing enqueued: n outside 1..65535, hw < 1, a NULL pointer, scores not
 * 8-byte aligned. */
size_t udet_post_propagate_workspace_bytes(int total_frames, int n_seq);
int udet_post_propagate_sequences(const float* masks, const float* flow_prev, const float* flow_next, int n_seq, const int* seq_first,
                                  const int* seq_len, int total_frames, int h, int w, float w_s, float w_r, float* avg_f, float* avg_b,
                                  void* workspace, size_t workspace_bytes, void* stream);
int udet_post_select_unary(const float* pred, const float* avg_f, const float* avg_b, const float* gt, int n, int hw, int* choice,
                           double* scores, float* soft, float* unary, void* stream);

/* The soft scores of the ensemble for a batch of frames (csrc/soft_score.hip): the per-frame body of
 * generate_soft_score_from_buffer.py buffer_to_soft_score :38-93 -- what udet_post_border_mean, udet_post_bytescale, udet_post_resample_u8,
 * udet_post_place and udet_post_minmax_norm compute in about a hundred launches and a host round trip per frame -- for n frames in four
 * launches, without a host synchronisation or a copy to the host, bit for bit.
 *   masks      device float32 [n][2][ns][nc][h][w]: direction 0 the backward run (-shift), 1 the forward run; shift index, crop index
 *   pred_mask  device float64 [n][h][w] (8-byte aligned)
 *   san_t      the sanity threshold as a double: the reference compares a float64 mean with the Python float 0.6
 *   geom       device int32 [ns * nc][UDET_SOFT_SCORE_GEOM], row shift index * nc + crop index =
 *                {mode, sy0, sx0, sh, sw, hh, ww, y0, x0, hk, hb, hks, vk, vb, vks, 0}
 *              mode 0, identity (shift 1 at the base crop): the term is the raw s_b + s_f and the rest of the row is not read; mode 1,
 *              rectify: the window [sy0, sy0 + sh) x [sx0, sx0 + sw) of the mask is bytescaled with the window's own min / max (cscale == 0
 *              -> 1) and resampled to the hh x ww patch that lands at (y0, x0) of the h x w canvas, zeros around it (rectify_pred_mask
 *              :98-114); hk / hb / hks: the int32 offsets into coef of the horizontal pass's (sw -> ww) Pillow coefficients kk [ww][hks] and
 *              bounds [ww][2] = (first tap, taps) and their row length, as udet_restore_masks_ragged takes them; vk / vb / vks: the vertical
 *              pass (sh -> hh); hk / vk < 0: the pass is skipped (out == in)
 *   coef       device int32: the concatenated coefficient blocks
 * Launch 1, per mask: the border mean (udet_post_border_mean's loop and tree: the same double) and the min / max of the source window as
 * partial pairs.  Launch 2: every raw mask of a rectify row is bytescaled and resampled on 64 x 16 tiles of its patch (the tile routine of
 * udet_restore_masks_ragged, csrc/pil_resample.h: horizontal pass into a uint8 LDS strip, vertical pass out of it) into the workspace, the
 * patch's largest byte by an integer atomicMax.  Launch 3, one thread per
 * pixel: per (frame, shift, crop) both means >= san_t: both slots are zeros; only the backward run's: its slot takes the forward run's patch
 * and maximum; only the forward run's: the reverse; term = vb / (maxb + 1e-6) + vf / (maxf + 1e-6) in double with zeros outside the patch
 * (identity: (double)s_b + (double)s_f); score = term_0, then score += term_k shift-major, crop-minor -- the order of the reference's loops;
 * the score and a (min, max) pair per workgroup.  Launch 4: (score - min) / (max - min + 1e-6).  No workgroup waits for another, no
 * floating-point atomics: bit-identical from run to run and between a frame alone and inside a batch.
 * workspace: udet_post_soft_score_workspace_bytes(n, ns, nc, h, w) bytes, 16-byte aligned: the uint8 patches (n * 2 * ns * nc * h * w
 * bytes) and per-mask / per-workgroup scalars; linear in n; 0 for an argument below 1.
 * UDET_ERR_ARG, nothing enqueued: n, ns, nc below 1, h or w below 4, h * w >= 2^31, n * 2 * ns * nc above 65535 (a grid dimension), a NULL
 * pointer, pred_mask not 8-byte aligned, a non-finite san_t, a short or misaligned workspace.  The tables are device memory and are not read
 * here: windows and patches inside the frame, coefficient blocks inside coef and taps inside their window must hold
 * (post_processing.check_soft_score_tables validates them on the host before anything is launched). */
#define UDET_SOFT_SCORE_GEOM 16
size_t udet_post_soft_score_workspace_bytes(int n, int ns, int nc, int h, int w);
int udet_post_soft_score_batch(const float* masks, int n, int ns, int nc, int h, int w, const int* geom, const int* coef, double san_t,
                               double* pred_mask, void* workspace, size_t workspace_bytes, void* stream);

/* Visualisation and training summaries (models/utils/flow_utils.py:14-100, models/adversarial_learner.py:260-298,
 * test_generator.py:93-117): the images and gradient histograms of a run, from buffers that already sit on the device.
 *  - udet_flow_to_image: flow_to_image + compute_color (flow_utils.py:46-100) with the arithmetic the reference has on a float32
 *    flow under numpy 2.x: a component with |u| > 1e7 or |v| > 1e7 zeroes both; each sample's maximum radius is float32 (sqrtf of the
 *    float32 u*u + v*v, no FMA); sample i is divided by the RUNNING maximum over samples 0..i (the reference's maxrad lives across
 *    its batch loop, :83-97) widened to double plus DBL_EPSILON, and everything after that division is double: rad = sqrt(u*u+v*v),
 *    a = atan2(-v,-u)/pi, fk = (a+1)/2*54 + 1, k0 = floor(fk), k1 = k0+1 (56 -> 1), f = fk-k0, per channel
 *    col = (1-f)*wheel[k0-1]/255 + f*wheel[k1-1]/255, col = rad <= 1 ? 1 - rad*(1-col) : col*0.75, out = floor(255*col); wheel =
 *    make_color_wheel (:14-42).  The pixel that attains the maximum has rad within an ulp of 1: this precision mix decides its branch.
 *    A NaN component paints the pixel black and is EXCLUDED from the maximum.  (In the reference a NaN reaches Python's
 *    max(maxrad, nan), whose result depends on the argument order: an accident that turns every later sample of the batch black.)
 *    mask [n,h,w,1] and stats8 (the device doubles udet_mask_stats wrote for that mask) are both NULL or both given: the mask is
 *    then thresholded (> threshold) and complemented per sample when stats8[i][0] / (4w + 4h) >= 0.6 (disambiguate_forw_back,
 *    general_utils.py:100-109), and a pixel inside the resulting object mask is written as (127,127,127) -- the zero of the
 *    reference's img/255 - 0.5 image times (1 - mask) (adversarial_learner.py:269-272).  No host round trip in between.
 *    flow [n,h,w,2] -> rgb [n,h,w,3] uint8.  Two launches: per-sample partial maxima into `workspace` (4-byte aligned,
 *    >= udet_flow_to_image_workspace_bytes(n)), then the colouring, which takes the prefix maximum itself.
 *  - udet_overlay_mask: test_generator.py:101-107 in one launch.  image [n,h,w,3] in [-0.5,0.5] -> postprocess_image ((x+0.5)*255 in
 *    float32, truncated toward zero, clamped to 0..255); the disambiguated boolean mask (as above; stats8 NULL: never complemented)
 *    -> postprocess_mask (0 / 255 in the middle channel only); cv2.addWeighted(img, 0.5, mask, 0.4, 0) in float32, rounded half to
 *    even, saturated; cv2.resize to oh x ow, 8-bit INTER_LINEAR: fx = (float)((dx+0.5)*w/ow - 0.5), taps (floor(fx), +1) clamped at
 *    the edges with weight 0 on the clamped side, coefficients round(weight*2048), horizontal pass in int32, vertical pass
 *    (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.  The four blended source pixels of an output pixel are computed on the fly.
 *    out [n,oh,ow,3] uint8, RGB (the reference's BGR order is cv2.imwrite's convention).
 *  - udet_grad_histogram: tf.summary.histogram (adversarial_learner.py:284-289) of every variable of a flat gradient buffer in one
 *    call.  Segment s is g[seg_offsets[s] .. seg_offsets[s+1]) (device int64 [nseg+1], any ranges inside g).  Bucket limits are
 *    TensorFlow's defaults (udet_histogram_limits: v = 1e-12, v *= 1.1 while v < 1e20 -- 774 values --, DBL_MAX, the negated mirror
 *    and 0: UDET_HISTOGRAM_BUCKETS = 1551 ascending doubles, built once on the host and uploaded with every call).  A value counts
 *    in the first limit strictly greater than it (upper_bound, compared in double); +inf and NaN, which have none, in the last.
 *    counts [nseg][1551] uint32 (zeroed by the call); stats [nseg][5] doubles = {min, max, count, sum, sum of squares}, the sums by
 *    a deterministic two-stage reduction.  workspace: 8-byte aligned, >= udet_grad_histogram_workspace_bytes(nseg). */
#define UDET_HISTOGRAM_BUCKETS 1551
size_t udet_flow_to_image_workspace_bytes(int n);
int udet_flow_to_image(const float* flow, const float* mask, const double* stats8, float threshold, int n, int h, int w,
                       unsigned char* rgb, void* workspace, size_t workspace_bytes, void* stream);
int udet_overlay_mask(const float* image, const float* mask, const double* stats8, float threshold, int n, int h, int w,
                      unsigned char* out, int oh, int ow, void* stream);
int udet_histogram_limits(double* limits, int n); /* host memory */
size_t udet_grad_histogram_workspace_bytes(int nseg);
int udet_grad_histogram(const float* g, const long long* seg_offsets, int nseg, double* stats, unsigned* counts, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The final mask of every frame drawn on the untouched frame at the frame's own size, for a ragged batch in one launch (csrc/visualize.hip,
 * DESIGN.md 7.6): the picture of test_generator.py:101-106 without its resize, plus the mask's contour.  Packed layout of
 * udet_dense_crf_ragged: sample i = H_i x W_i elements at element offset offsets[i] (device int64 [n]), hw device int32 [n][2]; image_rgb
 * and out_rgb 3 bytes per element (sample i at byte 3 * offsets[i]); mask 1 byte per element (the `binary`, `labels` or `selected` buffer
 * of the calls above), fg = mask != 0.  Colours are 0xRRGGBB.  Per sample and channel c, with m_c the channel of mask_rgb on a
 * foreground pixel and 0 elsewhere:
 *   t = rint(fl32(fl32(img_c) * alpha) + fl32(fl32(m_c) * beta))   two float32 products and one float32 sum, each rounded on its own (no
 *                                                                  FMA), rint to even, saturated to 0..255: cv2.addWeighted as
 *                                                                  udet_overlay_mask has it (0.5, 0.4, 0x00FF00: the reference's picture)
 * edge >= 1: a foreground pixel (y, x) is a contour pixel when some (y + dy, x + dx), |dy|, |dx| <= edge, INSIDE the frame is background
 * (positions outside the frame never count as background: an object cut by the frame border gets no line along the border) -- fg &
 * ~binary_erosion(fg, ones((2 edge + 1, 2 edge + 1)), border_value=1); it is written as edge_rgb, unblended.  edge = 0: no contour, no
 * neighbour is read.  Bytes of out_rgb between the samples are not written; out_rgb must not overlap the inputs.
 * One launch whatever n is, no workspace, no atomics, no workgroup waits for another: the grid is the 32 x 64 tiles of (max_h, max_w)
 * times n, workgroups beyond a smaller sample's tiles leave at once; the tile's foreground bits and an edge-wide halo are bit-packed in
 * LDS (128 columns per row), the windowed minimum is separable on the packed words; a thread takes the four pixels whose twelve colour
 * bytes form three aligned 32-bit words (the tile's columns are shifted per row by the row's element offset modulo 4, since 3 *
 * offsets[i] is not aligned in general; image_rgb / out_rgb that are not 4-byte aligned, and the groups cut by a row end, go byte by byte).
 * UDET_ERR_ARG, nothing enqueued: n outside 1..65535, a NULL pointer, max_h or max_w < 1 (or max_h * max_w >= 2^31), total_pixels < 1,
 * edge < 0, a negative or non-finite alpha or beta.  UDET_ERR_UNSUPPORTED: edge > UDET_OVERLAY_MAX_EDGE.  UDET_ERR_SHAPE: more than 2^23
 * tiles per sample.  The tables are device memory: the host caller validates them before the launch (ragged.as_layout / PackedLayout). */
#define UDET_OVERLAY_MAX_EDGE 8
int udet_overlay_native_ragged(const unsigned char* image_rgb, const unsigned char* mask, int n, const long long* offsets,
                               const int* hw, int max_h, int max_w, size_t total_pixels, float alpha, float beta,
                               unsigned mask_rgb, int edge, unsigned edge_rgb, unsigned char* out_rgb, void* stream);

/* tf.nn.conv2d / tf.layers.conv2d, padding='SAME', + bias + activation
 * (models/utils/convolution_utils.py:46,81-84; models/PWCNet/model_pwcnet.py:161-165,484-504,562-574).
 * upsample2x != 0 first applies tf.image.resize_nearest_neighbor(x2, align_corners=True)
 * (convolution_utils.py:70-71) fused into the loader.  workspace >= udet_conv2d_workspace_bytes(). */
size_t udet_conv2d_workspace_bytes(int n, int h, int w, int cin, int cout, int kh, int kw, int upsample2x);
int udet_conv2d(const float* x, const float* w_hwio, const float* bias, float* y, int n, int h, int w, int cin, int cout,
                int kh, int kw, int stride, int dilation, int upsample2x, int act, float alpha, void* workspace,
                size_t workspace_bytes, void* stream);
/* gradients of the op above w.r.t. its input (dx, [n,h,w,cin]) and w.r.t. weights / bias
 * (tf.gradients through Conv2D: Conv2DBackpropInput / Conv2DBackpropFilter / BiasAddGrad).
 * dy is the gradient w.r.t. the activated output; y_saved is the forward output (needed when act != NONE). */
int udet_conv2d_backward_data(const float* dy, const float* y_saved, const float* w_hwio, float* dx, int n, int h, int w,
                              int cin, int cout, int kh, int kw, int stride, int dilation, int act, float alpha,
                              void* workspace, size_t workspace_bytes, void* stream);
int udet_conv2d_backward_filter(const float* x, const float* dy, const float* y_saved, float* dw_hwio, float* dbias, int n,
                                int h, int w, int cin, int cout, int kh, int kw, int stride, int dilation, int upsample2x,
                                int act, float alpha, void* workspace, size_t workspace_bytes, void* stream);
/* tf.layers.conv2d_transpose(x, cout, 4, 2, 'same') + bias: models/PWCNet/model_pwcnet.py:283-286.
 * w is [4][4][cout][cin]; y is [n,2h,2w,cout]. */
int udet_conv2d_transpose4x4s2(const float* x, const float* w_hwoi, const float* bias, float* y, int n, int h, int w,
                               int cin, int cout, void* workspace, size_t workspace_bytes, void* stream);


/* ---- per-stage entry points of the loss / optimizer tail (parity tests, callers that keep their own graph) ------------
 * `workspace` (device, 8-byte aligned) >= udet_stage_workspace_bytes(n) holds the deterministic two-stage reduction partials. */
size_t udet_stage_workspace_bytes(int n);
/* preprocess_flow_batch(flow): models/utils/flow_utils.py:5-12 -- per sample and channel (f - mean) / sqrt(var), population
 * variance, no epsilon.  flow, out [n,h,w,2]. */
int udet_flow_normalize(const float* flow, float* out, int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
/* charbonnier_loss(gt_flows, pred_flows, masks, cbn): models/utils/loss_utils.py:34-51.  out[n] (device) = sum over h,w,c of
 * ((gt - pred)^2 + 0.001^2)^cbn * mask; masks [n,h,w,mask_channels] with 1 (broadcast) or 2 channels, or NULL (ones). */
int udet_charbonnier_loss(const float* gt_flows, const float* pred_flows, const float* masks, int mask_channels, int n, int h, int w,
                          float cbn, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* losses{} of models/adversarial_learner.py:141-204 from flow [b,h,w,2], mask [b,h,w,1] and the three recover predictions
 * pred3 [3b,h,w,2] (calls: masked, complement, image-only).  losses8 (device) in the order of :196-204; coef [b][4] (device) =
 * d generator_loss / d {R_b, D_b, Rc_b, Dc_b}, consumed by udet_losses_backward. */
int udet_losses_forward(const float* flow, const float* mask, const float* pred3, int b, int h, int w, float cbn, float epsilon,
                        float* losses8, float* coef, void* workspace, size_t workspace_bytes, void* stream);
/* tf.gradients of the two losses w.r.t. the predictions (models/utils/loss_utils.py:18 through :141-204):
 * which = 2: d recover_loss / d pred3 -> dpred [3b,h,w,2];  which = 1: d generator_loss / d pred3[0:2b] -> dpred [2b,h,w,2]
 * and the direct mask term -> dmask [b,h,w,1] (coef from udet_losses_forward). */
int udet_losses_backward(const float* flow, const float* mask, const float* pred3, const float* coef, int which, int b, int h, int w,
                         float cbn, float* dpred, float* dmask, void* stream);
/* train_op, second half (models/utils/loss_utils.py:22-31): g <- flag2[1] != 0 ? |U(-clip,clip)| (counter-based stream keyed by
 * (seed, step, index)) : clip(g, +-clip).  flag2: device {avg, flag} from udet_grad_absmean, or NULL (clip only). */
int udet_clip_or_noise(float* g, size_t n, float clip, const float* flag2, unsigned long long seed, long step, void* stream);
/* tf.train.AdamOptimizer(lr, beta1).apply_gradients (adversarial_learner.py:216; TF form lr_t = lr*sqrt(1-b2^t)/(1-b1^t)) on a
 * flat buffer; t = number of applies of the shared optimizer object including this one (>= 1). */
int udet_adam_step(float* w, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, long t,
                   void* stream);

/* ---- the step plan ------------------------------------------------------------------------
 * One plan = one (batch, shapes, flags) specialisation of the graph assembled by
 * AdversarialLearner.build_train_graph / build_test_graph / build_aug_test_graph
 * (models/adversarial_learner.py:72-258, 450-523, 525-592).  The caller owns one workspace of
 * udet_workspace_bytes() bytes (256-byte aligned) that holds packed weights, every activation,
 * every activation-gradient and all scratch; udet_buffer_info() names its regions so the host
 * wrapper can view them as tensors without copies.  Weights, gradients and Adam slots are flat
 * fp32 buffers per network in TF variable order (udet_param_info), owned by the caller; the
 * gradient buffers are the RCCL all-reduce payload.
 * net / which: 0 = pwcnet (frozen), 1 = generator "MaskNet", 2 = recover "FlownetS"; which=3 both. */
typedef struct udet_plan udet_plan;
typedef struct {
  int batch;                 /* frame pairs per GPU (common_flags.py:8) */
  int in_h, in_w;            /* PWC-Net input size: 384 x 640 after the readers' resize (multiples of 64) */
  int img_h, img_w;          /* generator / recover size: flags img_height/img_width = 192 x 384 */
  float flow_normalizer;     /* 80   (common_flags.py:10) */
  float cbn;                 /* 0.5  (common_flags.py:17) */
  float epsilon;             /* 75   (common_flags.py:18) */
  float lr, beta1, beta2, adam_eps; /* 1e-4, flag beta1=0.9, 0.999, 1e-8 (adversarial_learner.py:216) */
  float clip;                /* 0.2  (adversarial_learner.py:227,233) */
  unsigned long long noise_seed;    /* stream of the escape-noise branch (loss_utils.py:7-10,19-26) */
  int conv_fp16;             /* 0 (default): fp32 MFMA, the reference's arithmetic.  1: BASELINE.json configs[4] -- the convolution
                              * GEMMs (forward, backward-data, backward-filter) multiply in fp16 with fp32 accumulation
                              * (v_mfma_f32_32x32x8_f16; gradient operands scaled by 4096 against underflow); tensors, losses,
                              * reductions and the optimizer stay fp32.  Not a reference capability: parity tolerance 2e-2.
                              * Overflow guard: a gradient operand beyond 16 (65504 / 4096) becomes inf in fp16 and reaches the
                              * flat gradient buffer as inf / NaN; udet_apply counts the non-finite gradient values on the
                              * device and DROPS the update when there are any (weights / Adam slots untouched); the next
                              * forward / backward call on the plan that finds the count returns UDET_ERR_OVERFLOW -- once per
                              * report, BEFORE it enqueues anything, so the caller simply re-issues the call (what
                              * trainer.train_step does, counting the event) -- and udet_fp16_overflow_count synchronises and
                              * returns the number of dropped updates.  No report is lost when the host never synchronises:
                              * udet_apply consumes the report of the network's previous apply before it re-uses the slot.
                              * The shared Adam step count advances for a dropped update too (the host cannot know at enqueue
                              * time): one bias-correction step is skipped. */
} udet_config;

int udet_plan_create(const udet_config* cfg, udet_plan** out);
void udet_plan_destroy(udet_plan* plan);
size_t udet_workspace_bytes(const udet_plan* plan);
/* zero-fills the workspace and uploads the static tables; call once per workspace (synchronises the stream) */
int udet_plan_init(udet_plan* plan, void* workspace, void* stream);

int udet_param_count(int net);
size_t udet_param_total(int net);
int udet_param_info(int net, int index, const char** name, int* rank, int* shape4, size_t* offset_floats);
int udet_buffer_count(const udet_plan* plan);
int udet_buffer_info(const udet_plan* plan, int index, const char** name, size_t* offset_bytes, int* dims_nhw_ld);

/* re-layout of the TF-format weights for the kernels (K-padded, BN folded, transposed for dgrad).
 * pwc: once per checkpoint; trainable: after every optimizer apply (udet_train_step does it). */
int udet_pack_pwc(udet_plan* plan, const float* w_pwc, void* workspace, void* stream);
int udet_pack_trainable(udet_plan* plan, const float* w_gen, const float* w_rec, void* workspace, void* stream);

/* ModelPWCNet().predict_from_img_pairs(img1, img2): models/PWCNet/model_pwcnet.py:61-76 -> nn() :599-649.
 * img1,img2 [B,in_h,in_w,3] in [-0.5,0.5]; result in buffer "flow_full" [B,in_h,in_w,2]. */
int udet_pwc_forward(udet_plan* plan, const float* img1, const float* img2, void* workspace, void* stream);
/* adversarial_learner.py:83-204: PWC flow, legacy resize of image/flow, flow/normalizer, generator_net,
 * `ncalls` recover_net invocations (3 = train graph, 1 = test graph :509-513, 0 = aug-test graph :579),
 * and (ncalls==3) the 8 entries of losses{} (:196-204) into buffer "losses".
 * Results: buffers "image","flow","mask","pred" ([ncalls*B,...]). */
int udet_forward(udet_plan* plan, const float* img1, const float* img2, int ncalls, void* workspace, void* stream);
/* Cross-step pipelining.  PWC-Net is frozen (adversarial_learner.py:211-214), so the flow of the NEXT pair does not
 * depend on this step's optimizer update: udet_prefetch_flow enqueues PWC flow + the two resizes of (img1,img2) on the
 * plan's side streams, forked from `stream` at call time, into staging buffers ("image.next","flow.next"); it runs
 * concurrently with whatever is enqueued on `stream` afterwards (typically udet_backward of the current step).
 * udet_forward_prefetched joins it, moves the staging buffers into "image"/"flow" and continues like udet_forward.
 * img1/img2 must stay valid until that join.  One prefetch may be pending at a time. */
int udet_prefetch_flow(udet_plan* plan, const float* img1, const float* img2, void* workspace, void* stream);
int udet_forward_prefetched(udet_plan* plan, int ncalls, void* workspace, void* stream);
/* the first half of udet_forward_prefetched alone (join + staging -> "image"/"flow"); follow it with the NEXT
 * udet_prefetch_flow and then udet_forward_from_flow: the next pair's PWC flow then also overlaps this step's forward */
int udet_prefetch_consume(udet_plan* plan, void* workspace, void* stream);
/* same but starting from caller-filled "image" and "flow" buffers (generator_net/recover_net surface, nets.py:4,45) */
int udet_forward_from_flow(udet_plan* plan, int ncalls, void* workspace, void* stream);
/* generator_net(images, flows) alone (models/nets.py:4-42): reads "image","flow", writes "mask" (flow standardisation
 * of models/utils/flow_utils.py:5-12 included). */
int udet_generator_forward(udet_plan* plan, void* workspace, void* stream);
/* generator_net's own contract (models/nets.py:4-42): `flows` arrives ALREADY standardised (the call site passes
 * preprocess_flow_batch(flow), adversarial_learner.py:99-105).  Reads the caller-packed buffer "gen.in" ([.,.,.,8]: image 3,
 * standardised flow 2, zeros), writes "mask". */
int udet_generator_layers(udet_plan* plan, void* workspace, void* stream);
/* recover_net(img1, flow_masked, mask) alone (models/nets.py:45-110) on n*B samples whose inputs the caller packed into
 * "rec.imgin" ([.,.,.,4]: image, 0) and "rec.fin" ([.,.,.,4]: flow_masked(2), 1, 1-mask); writes "pred". */
int udet_recover_forward(udet_plan* plan, int n, void* workspace, void* stream);
/* optimizer.compute_gradients of losses['generator'] w.r.t. MaskNet and/or losses['recover'] w.r.t. FlownetS
 * (models/utils/loss_utils.py:18; adversarial_learner.py:211-234) into the flat gradient buffers. */
int udet_backward(udet_plan* plan, int which, const float* w_gen, const float* w_rec, float* g_gen, float* g_rec,
                  void* workspace, void* stream);
/* Data-parallel overlap: makes `stream` (a communication stream) wait until the flat gradient buffer of `net` written by the
 * last udet_backward is final -- with which=3 the recover gradients are final while the longer generator-loss pass still
 * runs, so their all-reduce overlaps it. */
int udet_stream_wait_grads(udet_plan* plan, int net, void* stream);
/* the two passes alone: train_generator_op / train_recover_op's compute_gradients (adversarial_learner.py:224-234) */
int udet_generator_backward(udet_plan* plan, const float* w_gen, float* g_gen, void* workspace, void* stream);
int udet_recover_backward(udet_plan* plan, const float* w_rec, float* g_rec, void* workspace, void* stream);
/* train_op, first half (loss_utils.py:19-21): out2 (device) = {mean over the variables of mean|g_v|, that < 1e-5 ? 1 : 0};
 * g is the flat gradient buffer of `net` (1 or 2). */
int udet_grad_absmean(udet_plan* plan, int net, const float* g, float* out2, void* workspace, void* stream);
/* the rest of train_op (loss_utils.py:19-32): clip +-0.2 / escape noise (generator only), Adam apply with the
 * shared beta-power accumulators; g is overwritten with the clipped gradient. */
int udet_apply(udet_plan* plan, int net, float* w, float* g, float* m, float* v, void* workspace, void* stream);
/* conv_fp16 plans: synchronises the pending overflow reports and returns how many optimizer updates were dropped so far because
 * their gradients held non-finite values (0 for fp32 plans); never an error by itself */
long udet_fp16_overflow_count(udet_plan* plan);
/* Number of optimizer updates applied so far (ONE Adam object for both networks: shared beta powers, adversarial_learner.py:216).
 * conv_fp16 plans: an update dropped by the overflow guard does not count.  The drop is known on the host only when the apply has
 * run, so both calls first wait for the plan's pending overflow reports (a stream synchronisation in that mode only) and book them:
 * the count returned -- e.g. into a checkpoint -- equals the updates that really happened, and a count set here is not decremented
 * afterwards by the report of an apply that preceded the call.  Applies ENQUEUED between a dropped update and its report used the
 * advanced count for their bias correction (at most the other network's apply and this network's next): a transient of one step. */
long udet_get_adam_step(const udet_plan* plan);
void udet_set_adam_step(udet_plan* plan, long t);
/* pack + forward + backward + apply for `which` on one GPU (no gradient exchange) */
int udet_train_step(udet_plan* plan, int which, const float* img1, const float* img2, float* w_gen, float* w_rec,
                    float* g_gen, float* g_rec, float* m_gen, float* v_gen, float* m_rec, float* v_rec, void* workspace,
                    void* stream);

/* Autotuner (the MI355X analogue of TF's cuDNN autotune the reference relies on implicitly): runs one untimed
 * forward + both backward passes over random data; every distinct convolution problem of the plan times its candidate
 * kernel configurations on `stream` and the fastest is cached process-wide (keyed by problem shape) for all later
 * launches.  Needs packed weights (udet_pack_pwc / udet_pack_trainable); overwrites g_gen / g_rec and re-zeroes the
 * activation regions of the workspace.  Optional: without it the built-in heuristics choose the configurations.
 * Every winner's output on the tuning data is compared with the built-in configuration's before it is cached (a
 * configuration that differs is rejected and reported on stderr); the comparison buffers are the one temporary device
 * allocation the library makes, freed before udet_autotune returns. */
int udet_autotune(udet_plan* plan, const float* w_gen, const float* w_rec, float* g_gen, float* g_rec, void* workspace,
                  void* stream);
int udet_tuned_shapes(void);
/* The tuned configurations as a text file (keys are hashes of the problem shapes): a later process loads them instead of
 * tuning again, e.g. a rocprofv3 trace that should contain timed steps only.  udet_tune_load returns the number of entries
 * read (>= 0) or an error code.  The header line carries the build's tuning ABI: a file of another build is rejected.  Loaded
 * entries are not trusted blindly: at launch time a cached configuration is used only if its tile / kernel family is
 * instantiated, its split count is clamped to the launch's capacity, and anything else falls back to the built-in choice. */
int udet_tune_save(const char* path);
int udet_tune_load(const char* path);
/* autotuner winners rejected because their output differed from the built-in configuration's (0 on a healthy build) */
int udet_tune_rejected(void);
/* Measurement aid (bench.py): between begin/end every convolution / warp-cost-volume launch group is timed on the launch
 * stream.  out[cat*5 + {0..4}] = {groups, kernel ms, algorithmic FLOPs, algorithmic bytes, bracket ms} for cat 0 conv fwd,
 * 1 conv dgrad, 2 conv wgrad, 3 (unused), 4 warp + cost volume.  "kernel ms" sums the kernels' own start -> stop times (event
 * pairs carried by the dispatch packets: what rocprofv3 --kernel-trace reports); "bracket ms" is hipEventRecord before / after
 * each group, which additionally contains the event packets and dispatch gaps. */
int udet_profile_begin(udet_plan* plan);
int udet_profile_end(udet_plan* plan, double* out, int ncat, void* stream);

/* Concurrency switch.  A plan runs independent chains of a step on its own side streams, forked from / joined to the caller's
 * stream with events.  on = 0 collapses every lane onto the caller's stream: the plain program order, results
 * bit-identical (tests/test_autotune_gpu.py), used for serial kernel traces.  Takes effect from the next call on the plan.
 *
 * Environment variables the library reads -- all diagnostic, none on a launch path, none changes a result:
 *   UDET_SERIAL=1      read once by udet_plan_create: the plan starts with udet_plan_set_concurrent(plan, 0);
 *   UDET_TUNE_LOG=1    read by the autotuner (udet_autotune): one stderr line per tuned problem shape;
 *   UDET_PROF_DUMP=F   read by udet_profile_end: appends one CSV line per launch group of the measurement pass to F.
 * Kernel-selection forcing for tests lives in a separate library (include/udet_debug.h, libudet_debug.so). */
int udet_plan_set_concurrent(udet_plan* plan, int on);

/* Lane placement.  ROCm maps every stream of a process onto one of GPU_MAX_HW_QUEUES (default 4) hardware queues when the stream is
 * created, and two streams on one queue execute in submission order -- which lanes of a plan share a queue changes the step time by up
 * to 20 % and depends on every other stream the process (PyTorch's pool, RCCL) created before.  A plan therefore owns candidate
 * streams (eight; up to 32 are drawn while fewer than three independent queues have been found) and, the first time it is driven from a given caller stream, probes (a 200 us spin kernel on one stream, an empty kernel on
 * the other) which candidates run concurrently with the caller's stream and with each other, then lays its six lanes out on
 * four independent queues: {0 = the caller's stream, 2} {1} {3} {4, 5}; with fewer independent queues lanes are merged.  That first
 * call synchronises the device once (~3 ms).  udet_plan_lane_queues places the lanes for `stream` if that has not happened yet and
 * writes the queue-group index of each of the six lanes (0 = the caller's queue) to queue[6]; returns the number of independent
 * queues in use (4 on a default runtime), < 0 on error.  Do not raise GPU_MAX_HW_QUEUES: above four queues a cross-stream dependency
 * costs 79 us instead of 12 (profiles/r03_hop_bench.txt). */
int udet_plan_lane_queues(udet_plan* plan, void* stream, int* queue);
/* The same layout without the timing probe, for a host that knows its streams: side_streams[0..n-1] (n = 0..3, created by the host
 * and kept alive as long as the plan is driven from `stream`) are taken to sit on n distinct hardware queues, none of them `stream`'s;
 * lanes {1} {3} {4, 5} go to them in that order (fewer streams: merged exactly as a probe that finds fewer queues would).  Replaces
 * any placement the plan holds for `stream`.  A probe is a ~200 us spin kernel against an empty kernel, repeated up to three times
 * when it sees no overlap (a positive result is proof, a negative one may be a slow host or a GPU shared with another process);
 * a deployment that cannot tolerate that heuristic pins. */
int udet_plan_pin_lanes(udet_plan* plan, void* stream, void* const* side_streams, int n);

/* Per-track instance maps (csrc/instances.hip): after the link, every pixel of every frame learns which track it belongs
 * to.  labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts and k are what udet_link_detections_ragged takes; ids: device
 * int32 [n][k], as either link call wrote them; gt: optional (NULL: none) device uint8 packed like labels, the buffer
 * udet_select_components_ragged takes, foreground where != 0.  map: device uint8 packed like labels; row_gt: device int64 [n][k];
 * frame_stats: device int64 [n][3].  With rows_i = counts[i][2] clamped to 0..k, for pixel p of sample i and L = labels[offsets[i] + p]:
 *   L outside 1..H_i*W_i                                       map = 0 (outside the range is background, as for the other calls);
 *   else, root = L - 1: some row r < rows_i has dets[i][r][0] == root and ids[i][r] >= 0
 *                                                              map = 1 + (ids[i][r] mod UDET_INSTANCE_WRAP), a value in 1..252;
 *   else                                                       map = UDET_INSTANCE_UNASSIGNED: foreground of a component that has no row
 *                                                              (below min_area, past k) or whose row has no id.
 * row_gt[i][r] is the number of pixels of row r's component with gt != 0 (0 for r >= rows_i; every entry is 0 when gt is NULL);
 * frame_stats[i] = {pixels with map in 1..252, pixels with map = 255, pixels with gt != 0} (the last is 0 without gt).  Bytes of map
 * between the samples are not written.  The wrap is 252 and not 254 because 252 is a multiple of the twelve colours of the default
 * track palette: palette[(map - 1) mod 12] == palette[id mod 12] for every id, so a filled instance and the rectangle
 * udet_draw_track_boxes_ragged paints for it share a colour; the values 253 and 254 stay unused.
 * Two launches whatever n, k, the components and the sequences are, no host round trip, no workgroup waits for another, integer atomics
 * only: the outputs are exact, identical from run to run and for a sample alone or inside a batch.  The first launch zeroes row_gt and
 * frame_stats and enters every row's rank at its root in the workspace (the lookup of the link: one int32 per pixel, never zeroed, a
 * lookup counts only when the row it names holds that root); the second takes one pixel per lane, 64 consecutive pixels of one sample
 * per wave: the pixels of a row under gt are counted by one LDS atomic per horizontal run of a wave, k partials per workgroup, then one
 * 64-bit integer atomic per non-zero partial; the map is written as aligned 32-bit words of four pixels (the pixels of a sample are
 * contiguous, so a word may span a row end), the bytes of a sample's head and tail that share a word with its neighbours one by one.
 * workspace: udet_track_instance_maps_workspace_bytes(total_pixels, n, k) bytes (4 per pixel), 4-byte aligned; 0 for bad arguments.
 * UDET_ERR_ARG, nothing enqueued: a NULL labels, offsets, hw, dets, counts, ids, map, row_gt or frame_stats, n outside 1..65535, k
 * outside 1..UDET_DET_MAX_K, max_h or max_w < 1, total_pixels < 1, a short or misaligned workspace, labels / ids not 4-byte or dets /
 * counts / row_gt / frame_stats not 8-byte aligned.  Every index a kernel forms is bounded, whatever labels, dets, counts, ids and the
 * workspace hold; the tables are device memory: the host caller validates them (native_instances.instance_maps). */
#define UDET_INSTANCE_WRAP 252
#define UDET_INSTANCE_UNASSIGNED 255
size_t udet_track_instance_maps_workspace_bytes(size_t total_pixels, int n, int k);
int udet_track_instance_maps_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                    size_t total_pixels, const long long* dets, const long long* counts, int k, const int* ids,
                                    const unsigned char* gt, unsigned char* map, long long* row_gt, long long* frame_stats,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* The instance map drawn on the untouched frames, every instance in the colour of its track: udet_overlay_native_ragged with `map` in
 * the place of `mask` and a colour per value.  image_rgb, out_rgb, offsets, hw, max_h, max_w, total_pixels, alpha, beta and edge are what
 * that call takes; palette: device uint32 [palette_size], 0xRRGGBB, palette_size in 1..UDET_TRACK_MAX_PALETTE; other_rgb: the colour of
 * the value 255.  The colour of a pixel with value v is none for v = 0, palette[(v - 1) mod palette_size] for v in 1..252 and other_rgb
 * for 253..255.  The blend is that call's, unchanged: t = rint(fl32(fl32(img_c) * alpha) + fl32(fl32(m_c) * beta)) with m_c the pixel's
 * own colour channel, or 0 on background -- two float32 products and one sum, each rounded on its own (no FMA), rint to even, saturated
 * to 0..255.  edge >= 1: a pixel with v != 0 is a contour pixel when some position (y + dy, x + dx), |dy|, |dx| <= edge, INSIDE the frame
 * holds a value different from v (positions outside the frame never count) -- (v != 0) & ((minimum_filter(v, 2 edge + 1,
 * mode="nearest") != v) | (maximum_filter(v, 2 edge + 1, mode="nearest") != v)); a contour pixel is written in its own colour,
 * unblended.  So two touching instances are separated by a line of each one's colour, and an object cut by the frame border gets no
 * line along the border.  edge = 0: no contour, no neighbour is read.  Bytes of out_rgb between the samples are not written; out_rgb
 * must not overlap the inputs.
 * One launch, no workspace, no atomics: the grid is the 32 x 64 tiles of (max_h, max_w) times n, workgroups beyond a smaller sample's
 * tiles leave at once; the tile's bytes and an edge-wide halo are held in LDS, read with their coordinates clamped into the frame; the
 * windowed minimum and maximum are separable, rows then columns; the colour bytes go through the aligned three-word groups of
 * udet_overlay_native_ragged (csrc/rgb_groups.h).  UDET_ERR_ARG, nothing enqueued: everything udet_overlay_native_ragged refuses, a NULL
 * or misaligned palette, palette_size outside 1..64, other_rgb above 0xffffff.  UDET_ERR_UNSUPPORTED: edge > UDET_OVERLAY_MAX_EDGE.
 * UDET_ERR_SHAPE: more than 2^23 tiles per sample. */
int udet_overlay_instances_ragged(const unsigned char* image_rgb, const unsigned char* map, int n, const long long* offsets, const int* hw,
                                  int max_h, int max_w, size_t total_pixels, float alpha, float beta, const unsigned* palette,
                                  int palette_size, unsigned other_rgb, int edge, unsigned char* out_rgb, void* stream);

/* The masks of whole tracks (csrc/follow.hip): a choice of rows per frame -- made on the host once a sequence is known,
 * native_follow.choose_tracks -- turned back into binary masks on the device.  labels, n, offsets, hw, max_h, max_w, total_pixels, dets,
 * counts and k are what udet_track_instance_maps_ragged takes; keep: device uint64 [n], bit r of keep[i] = keep row r of frame i; gt:
 * optional (NULL: none) device uint8 packed like labels, foreground where != 0.  selected: device uint8 packed like labels; stats: device
 * int64 [n][4].  With rows_i = min(counts[i][2], k) (clamped to 0..k), for pixel p of sample i and L = labels[offsets[i] + p]:
 *   selected = 1 exactly when L lies in 1..H_i*W_i, L - 1 is the root dets[i][r][0] of a row r < rows_i and bit r of keep[i] is set;
 *   selected = 0 otherwise (outside the range is background, as for the other calls).
 * Bits of keep[i] at or above rows_i are ignored.  stats[i] = {kept pixels, dropped foreground pixels, kept pixels with gt != 0, pixels
 * with gt != 0}: dropped foreground is a label in range that is not kept; the last two are 0 when gt is NULL.  Bytes of selected between
 * the samples are not written.
 * Two launches whatever n, k, the components and the sequences are, no host round trip, no workgroup waits for another, integer atomics
 * only: the outputs are exact, identical from run to run and for a sample alone or inside a batch.  The first launch zeroes stats and
 * enters every row's rank at its root in the workspace (the lookup of the link: one int32 per pixel, never zeroed, a lookup counts only
 * when the row it names holds that root); the second takes one pixel per lane, 64 consecutive pixels of one sample per wave, 4096 pixels
 * per workgroup: the keep word is uniform over a sample, one scalar load and a bit test, not a table lookup per pixel; the four counts
 * are ballots summed per wave, reduced in LDS, then one 64-bit integer atomic per non-zero partial per workgroup; selected is written as
 * aligned 32-bit words of four pixels whatever the sample's offset and the buffer's alignment, the bytes of a sample's head and tail
 * that share a word with its neighbours one by one (csrc/packed_bytes.h, the instance map's store).
 * workspace: udet_follow_tracks_workspace_bytes(total_pixels, n, k) bytes (4 per pixel), 4-byte aligned; 0 for bad arguments.
 * UDET_ERR_ARG, nothing enqueued: a NULL labels, offsets, hw, dets, counts, keep, selected or stats, n outside 1..65535, k outside
 * 1..UDET_DET_MAX_K, max_h or max_w < 1, total_pixels < 1, a short or misaligned workspace, labels not 4-byte or dets / counts / keep /
 * stats not 8-byte aligned.  Every index a kernel forms is bounded, whatever labels, dets, counts, keep and the workspace hold; the
 * tables are device memory: the host caller validates them (native_follow.follow_tracks). */
size_t udet_follow_tracks_workspace_bytes(size_t total_pixels, int n, int k);
int udet_follow_tracks_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                              long long total_pixels, const long long* dets, const long long* counts, int k,
                              const unsigned long long* keep, const unsigned char* gt, unsigned char* selected, long long* stats,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Tracks against multi-object annotations (csrc/objects.hip): what the one-to-one matching of annotated objects to
 * tracks needs from the pixels, counted on the device.  labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts and k are what
 * udet_track_instance_maps_ragged takes; objects: device uint8 packed like labels, 0 background, 1..num_objects an annotated object,
 * anything above num_objects "void"; num_objects (O) in 1..UDET_MAX_OBJECTS.  row_obj: device int64 [n][k][O]; obj_area: device int64
 * [n][O]; frame_stats: device int64 [n][2].  With rows_i = counts[i][2] clamped to 0..k:
 *   row_obj[i][r][o]  the pixels whose label is the root of row r (L - 1 == dets[i][r][0], r < rows_i) and whose object byte is o + 1;
 *                     0 for r >= rows_i;
 *   obj_area[i][o]    the pixels of sample i with object byte o + 1, whatever their label;
 *   frame_stats[i]    {pixels with byte in 1..O, pixels with byte > O}.
 * A label outside 1..H_i*W_i is background, as for the other calls.
 * Two launches whatever n, k, O and the content are, no host round trip, no workgroup waits for another, integer atomics only: the
 * outputs are exact, identical from run to run and for a sample alone or inside a batch.  The first launch zeroes the three outputs
 * and enters every row's rank at its root in the workspace (the lookup of the link: one int32 per pixel, never zeroed, a lookup counts
 * only when the row it names holds that root); the second takes one pixel per lane, 64 consecutive pixels of one sample per wave, 4096
 * pixels per workgroup: the object byte is one coalesced byte load per lane, a pair (r, o) is counted by one LDS atomic per horizontal
 * run of a wave into k x O partials and an object's own pixels by one per run into O partials (dynamic LDS, (k O + O) ints: 8.3 KB at
 * most), the two frame counts are ballots; then one 64-bit integer atomic per non-zero partial per workgroup.  Nothing is written per
 * pixel.
 * workspace: udet_track_object_overlaps_workspace_bytes(total_pixels, n, k) bytes (4 per pixel), 4-byte aligned; 0 for bad arguments.
 * UDET_ERR_ARG, nothing enqueued: a NULL labels, offsets, hw, dets, counts, objects, row_obj, obj_area or frame_stats, n outside
 * 1..65535, k outside 1..UDET_DET_MAX_K, num_objects outside 1..UDET_MAX_OBJECTS, max_h or max_w < 1, total_pixels < 1, a short or
 * misaligned workspace, labels not 4-byte or dets / counts / row_obj / obj_area / frame_stats not 8-byte aligned.  Every index a kernel
 * forms is bounded, whatever labels, dets, counts, objects and the workspace hold; the tables are device memory: the host caller
 * validates them (native_objects.object_overlaps). */
#define UDET_MAX_OBJECTS 32
size_t udet_track_object_overlaps_workspace_bytes(size_t total_pixels, int n, int k);
int udet_track_object_overlaps_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                      size_t total_pixels, const long long* dets, const long long* counts, int k,
                                      const unsigned char* objects, int num_objects, long long* row_obj, long long* obj_area,
                                      long long* frame_stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UDET_H */
