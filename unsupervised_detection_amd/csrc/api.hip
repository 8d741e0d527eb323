// extern "C" surface of libudet.so (see include/udet.h).
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include "../../include/udet.h"
#include "common.h"
#include "conv_host.h"
#include "elementwise.h"
#include "host_checks.h"

namespace udet {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  return UDET_ERR_HIP;
}

thread_local LaunchSink* g_launch_sink = nullptr;
bool launch_sink_next(hipEvent_t* a, hipEvent_t* b) {
  LaunchSink* s = g_launch_sink;
  if (!s || s->n >= s->cap) return false;
  if (hipEventCreate(a) != hipSuccess) return false;
  if (hipEventCreate(b) != hipSuccess) { (void)hipEventDestroy(*a); return false; }
  s->ev[2 * s->n] = *a;
  s->ev[2 * s->n + 1] = *b;
  ++s->n;
  return true;
}

// bump allocator over the caller's workspace (256-byte granules)
struct Arena {
  char* base;
  size_t cap, used;
  Arena(void* p, size_t n) : base((char*)p), cap(n), used(0) {}
  float* take(size_t floats) {
    const size_t bytes = (floats * sizeof(float) + 255) & ~(size_t)255;
    if (!base || used + bytes > cap) return nullptr;
    float* r = (float*)(base + used);
    used += bytes;
    return r;
  }
};
static inline size_t gran(size_t floats) { return (floats * sizeof(float) + 255) & ~(size_t)255; }
#define SPLITK_FLOATS ((size_t)8 << 20)  // 32 MiB of split-K scratch for the single-op entry points
}  // namespace udet

using namespace udet;

extern "C" {

int udet_version(void) { return 101; }
const char* udet_last_error(void) { return g_err; }

int udet_warp(const float* image, const float* flow, float flow_scale, float* out, int n, int h, int w, int c,
              void* stream) {
  return launch_warp(image, flow, 2, 0, flow_scale, out, n, h, w, c, nullptr, nullptr, (hipStream_t)stream);
}
int udet_warp_debug(const float* image, const float* flow, float flow_scale, float* out, int* floor_yx, float* alpha_yx,
                    int n, int h, int w, int c, void* stream) {
  return launch_warp(image, flow, 2, 0, flow_scale, out, n, h, w, c, floor_yx, alpha_yx, (hipStream_t)stream);
}
int udet_cost_volume(const float* c1, const float* warp, float* out, int n, int h, int w, int c, void* stream) {
  return launch_cost_volume(c1, warp, out, 81, 0, n, h, w, c, (hipStream_t)stream);
}

int udet_resize_bilinear_legacy_fwd(const float* x, float* y, int n, int h, int w, int c, int oh, int ow, void* stream) {
  if (n < 1 || h < 1 || w < 1 || c < 1 || oh < 1 || ow < 1) { set_error("resize: bad shape"); return UDET_ERR_SHAPE; }
  return launch_resize_bilinear_fwd(x, c, 0, n, h, w, y, c, 0, oh, ow, c, 1.f, 1.f, (hipStream_t)stream);
}
int udet_resize_bilinear_legacy_bwd(const float* dy, float* dx, int n, int h, int w, int c, int oh, int ow, void* stream) {
  if (n < 1 || h < 1 || w < 1 || c < 1 || oh < 1 || ow < 1) { set_error("resize: bad shape"); return UDET_ERR_SHAPE; }
  return launch_resize_bilinear_bwd(dy, c, 0, n, oh, ow, dx, c, 0, h, w, c, 0, (hipStream_t)stream);
}

int udet_crop_flip_resize(const void* src, int src_is_u8, int nearest, int n, int h, int w, int c, const int* params6,
                          float* dst, int oh, int ow, float div, float add, void* stream) {
  if (n < 1 || h < 1 || w < 1 || c < 1 || oh < 1 || ow < 1 || !src || !dst) { set_error("crop_flip_resize: bad argument"); return UDET_ERR_ARG; }
  return launch_crop_flip_resize(src, src_is_u8, nearest, n, h, w, c, params6, dst, oh, ow, div, add, (hipStream_t)stream);
}
int udet_crop_flip_resize_ragged(const void* src, int src_is_u8, int nearest, int n, int c, const long long* offsets,
                                 const int* hw, const int* params6, float* dst, int oh, int ow, float div, float add, void* stream) {
  if (n < 1 || c < 1 || oh < 1 || ow < 1 || !src || !dst || !offsets || !hw) { set_error("crop_flip_resize_ragged: bad argument"); return UDET_ERR_ARG; }
  return launch_crop_flip_resize_ragged(src, src_is_u8, nearest, n, c, offsets, hw, params6, dst, oh, ow, div, add, (hipStream_t)stream);
}

int udet_mask_stats(const float* pred_masks, const float* gt_masks, int n, int h, int w, float threshold, float gt_threshold,
                    double* stats8, void* stream) {
  if (n < 1 || h < 4 || w < 4 || !pred_masks || !gt_masks || !stats8) { set_error("mask_stats: bad argument"); return UDET_ERR_ARG; }
  return launch_mask_stats(pred_masks, gt_masks, n, h, w, threshold, gt_threshold, stats8, (hipStream_t)stream);
}

int udet_boundary_stats(const float* pred_masks, const float* gt_masks, const double* stats8, int n, int h, int w, float threshold,
                        float gt_threshold, int radius, unsigned long long* counts4, unsigned char* bmap_pred, unsigned char* bmap_gt,
                        void* stream) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || radius < 1 || !pred_masks || !gt_masks || !counts4) {
    set_error("boundary_stats: bad argument (n = %d in 1..65535, h = %d, w = %d, radius = %d >= 1, non-null masks and counts)", n, h, w, radius);
    return UDET_ERR_ARG;
  }
  if (radius > UDET_BOUNDARY_MAX_RADIUS) {
    set_error("boundary_stats: radius %d is above the supported maximum %d", radius, UDET_BOUNDARY_MAX_RADIUS);
    return UDET_ERR_UNSUPPORTED;
  }
  return launch_boundary_stats(pred_masks, gt_masks, stats8, n, h, w, threshold, gt_threshold, radius, counts4, bmap_pred, bmap_gt,
                               (hipStream_t)stream);
}

size_t udet_restore_workspace_bytes(int n) { return n < 1 ? 0 : restore_workspace_bytes(n); }
int udet_restore_masks_ragged(const float* masks, int n, int mh, int mw, const long long* offsets, const int* tables12, const int* coef,
                              int max_h, int max_w, unsigned char* data, int* amax, unsigned char* binary, double threshold,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("restore_masks_ragged", n, max_h, max_w, 1)) return UDET_ERR_ARG;
  if (mh < 1 || mw < 1 || (long)mh * mw > 0x7fffffffL || !masks || !offsets || !tables12 || !coef || !data || !amax) {
    set_error("restore_masks_ragged: bad argument (mask %d x %d, non-null masks, tables, data and amax)", mh, mw);
    return UDET_ERR_ARG;
  }
  if (binary && (!(threshold >= 0.0) || isinf(threshold) || binary == data)) {
    set_error("restore_masks_ragged: the binary mask needs a finite threshold >= 0 and a buffer of its own");
    return UDET_ERR_ARG;
  }
  if (bad_workspace("restore_masks_ragged", workspace, workspace_bytes, restore_workspace_bytes(n), 4)) return UDET_ERR_ARG;
  return launch_restore_masks_ragged(masks, n, mh, mw, offsets, tables12, coef, max_h, max_w, data, amax, binary, threshold, workspace,
                                     (hipStream_t)stream);
}

size_t udet_components_workspace_bytes(size_t total_pixels, int n) {
  return (n < 1 || total_pixels < 1) ? 0 : components_workspace_bytes(total_pixels, n);
}
int udet_select_components_ragged(const unsigned char* binary, const unsigned char* gt, int n, const long long* offsets, const int* hw,
                                  int max_h, int max_w, size_t total_pixels, int connectivity, int mode, int* labels,
                                  unsigned char* selected, long long* info, void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("select_components_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!binary || !offsets || !hw || !info) {
    set_error("select_components_ragged: bad argument (non-null binary, offsets, hw and info)");
    return UDET_ERR_ARG;
  }
  if (connectivity != 4 && connectivity != 8) {
    set_error("select_components_ragged: connectivity %d is neither 4 nor 8", connectivity);
    return UDET_ERR_ARG;
  }
  if (mode != UDET_COMPONENTS_LABEL && mode != UDET_COMPONENTS_LARGEST && mode != UDET_COMPONENTS_BEST_GT) {
    set_error("select_components_ragged: mode %d is none of UDET_COMPONENTS_LABEL / _LARGEST / _BEST_GT", mode);
    return UDET_ERR_ARG;
  }
  if (mode == UDET_COMPONENTS_BEST_GT && !gt) {
    set_error("select_components_ragged: UDET_COMPONENTS_BEST_GT needs the annotation (gt)");
    return UDET_ERR_ARG;
  }
  if ((mode != UDET_COMPONENTS_LABEL && !selected) || (selected && (selected == binary || selected == gt))) {
    set_error("select_components_ragged: a selecting mode needs `selected`, a buffer of its own");
    return UDET_ERR_ARG;
  }
  if (bad_workspace("select_components_ragged", workspace, workspace_bytes, components_workspace_bytes(total_pixels, n), 8)) return UDET_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(labels) & 3) {
    set_error("select_components_ragged: labels must be 4-byte aligned");
    return UDET_ERR_ARG;
  }
  return launch_select_components_ragged(binary, gt, n, offsets, hw, max_h, max_w, total_pixels, connectivity, mode, labels, selected, info,
                                         workspace, (hipStream_t)stream);
}

size_t udet_component_boxes_workspace_bytes(size_t total_pixels, int n, int k) {
  return (n < 1 || total_pixels < 1 || k < 1 || k > UDET_DET_MAX_K) ? 0 : component_boxes_workspace_bytes(total_pixels, n);
}
int udet_component_boxes_ragged(const int* labels, const unsigned char* score, int n, const long long* offsets, const int* hw,
                                int max_h, int max_w, size_t total_pixels, int min_area, int k, long long* dets, long long* counts,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("component_boxes_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!labels || !offsets || !hw || !dets || !counts) {
    set_error("component_boxes_ragged: bad argument (non-null labels, offsets, hw, dets and counts)");
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K || min_area < 1) {
    set_error("component_boxes_ragged: k = %d in 1..UDET_DET_MAX_K = %d and min_area = %d >= 1 are required", k, UDET_DET_MAX_K, min_area);
    return UDET_ERR_ARG;
  }
  if (bad_workspace("component_boxes_ragged", workspace, workspace_bytes, component_boxes_workspace_bytes(total_pixels, n), 8)) return UDET_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(labels) & 3) || ((reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts)) & 7)) {
    set_error("component_boxes_ragged: labels must be 4-byte aligned, dets and counts 8-byte aligned");
    return UDET_ERR_ARG;
  }
  return launch_component_boxes_ragged(labels, score, n, offsets, hw, max_h, max_w, total_pixels, min_area, k, dets, counts, workspace,
                                       (hipStream_t)stream);
}

int udet_draw_boxes_ragged(unsigned char* image_rgb, int n, const long long* offsets, const int* hw, size_t total_pixels,
                           const long long* dets, const long long* counts, int k, int thickness, unsigned rgb, void* stream) {
  if (bad_batch("draw_boxes_ragged", n, 1, 1, total_pixels)) return UDET_ERR_ARG;
  if (!image_rgb || !offsets || !hw || !dets || !counts) {
    set_error("draw_boxes_ragged: bad argument (non-null image_rgb, offsets, hw, dets and counts)");
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K || thickness < 1 || thickness > UDET_DRAW_MAX_THICKNESS || rgb > 0xffffffu) {
    set_error("draw_boxes_ragged: k = %d in 1..UDET_DET_MAX_K = %d, thickness = %d in 1..%d and rgb = 0x%x of 24 bits are required", k,
              UDET_DET_MAX_K, thickness, UDET_DRAW_MAX_THICKNESS, rgb);
    return UDET_ERR_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts)) & 7) {
    set_error("draw_boxes_ragged: dets and counts must be 8-byte aligned");
    return UDET_ERR_ARG;
  }
  return launch_draw_boxes_ragged(image_rgb, n, offsets, hw, dets, counts, k, thickness, rgb, (hipStream_t)stream);
}

// the carried frame of udet_link_detections_ragged: absent (no pointer, 0 x 0) or whole (every pointer, at least 1 x 1, below 2^31 pixels)
static bool link_carry_ok(const void* labels, int h, int w, const void* dets, const void* counts, const void* ids, const void* next_id) {
  if (!labels && !dets && !counts && !ids && !next_id) return h == 0 && w == 0;
  return labels && dets && counts && ids && next_id && h >= 1 && w >= 1 && (long)h * w <= 0x7fffffffL;
}
size_t udet_link_detections_workspace_bytes(size_t total_pixels, int n, int k, int carry_h, int carry_w) {
  const bool carry = carry_h != 0 || carry_w != 0;
  if (n < 1 || total_pixels < 1 || k < 1 || k > UDET_DET_MAX_K) return 0;
  if (carry && (carry_h < 1 || carry_w < 1 || (long)carry_h * carry_w > 0x7fffffffL)) return 0;
  return link_detections_workspace_bytes(total_pixels, carry_h, carry_w);
}
// udet_link_detections_ragged (disp = nullptr, motion = false) and udet_link_detections_motion_ragged: the same checks under the entry's name
static int link_detections_checked(const char* fn, bool motion, const int* labels, int n, const long long* offsets, const int* hw, int max_h,
                                   int max_w, size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                   const int* carry_labels, int carry_h, int carry_w, const long long* carry_dets,
                                   const long long* carry_counts, const int* carry_ids, const int* carry_next_id, int min_iou_permille,
                                   long long* inter, int* match, int* ids, int* linked, int* seq_tracks, int* next_id, const int* disp,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch(fn, n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (motion && (!disp || (reinterpret_cast<uintptr_t>(disp) & 3))) {
    set_error("%s: disp must be a non-null, 4-byte aligned int32 buffer of total_pixels elements", fn);
    return UDET_ERR_ARG;
  }
  if (!labels || !offsets || !hw || !dets || !counts || !link || !inter || !match || !ids || !linked || !seq_tracks || !next_id) {
    set_error("%s: bad argument (non-null labels, offsets, hw, dets, counts, link and outputs)", fn);
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K || min_iou_permille < 1 || min_iou_permille > 1000) {
    set_error("%s: k = %d in 1..UDET_DET_MAX_K = %d and min_iou_permille = %d in 1..1000 are required", fn, k,
              UDET_DET_MAX_K, min_iou_permille);
    return UDET_ERR_ARG;
  }
  if (!link_carry_ok(carry_labels, carry_h, carry_w, carry_dets, carry_counts, carry_ids, carry_next_id)) {
    set_error("%s: the carried frame is either absent (no pointer, 0 x 0) or whole (labels, dets, counts, ids and "
              "next id, %d x %d at least 1 x 1 and below 2^31 pixels)", fn, carry_h, carry_w);
    return UDET_ERR_ARG;
  }
  if (bad_workspace(fn, workspace, workspace_bytes, link_detections_workspace_bytes(total_pixels, carry_h, carry_w), 4))
    return UDET_ERR_ARG;
  const uintptr_t a4 = reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(link) | reinterpret_cast<uintptr_t>(carry_labels) |
                       reinterpret_cast<uintptr_t>(carry_ids) | reinterpret_cast<uintptr_t>(carry_next_id) |
                       reinterpret_cast<uintptr_t>(match) | reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(linked) |
                       reinterpret_cast<uintptr_t>(seq_tracks) | reinterpret_cast<uintptr_t>(next_id);
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(carry_dets) |
                       reinterpret_cast<uintptr_t>(carry_counts) | reinterpret_cast<uintptr_t>(inter);
  if ((a4 & 3) || (a8 & 7)) {
    set_error("%s: the int32 buffers must be 4-byte aligned, dets, counts and inter 8-byte aligned", fn);
    return UDET_ERR_ARG;
  }
  return launch_link_detections_ragged(labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts, k, link, carry_labels, carry_h,
                                       carry_w, carry_dets, carry_counts, carry_ids, carry_next_id, min_iou_permille, inter, match, ids,
                                       linked, seq_tracks, next_id, disp, workspace, (hipStream_t)stream);
}
int udet_link_detections_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                const int* carry_labels, int carry_h, int carry_w, const long long* carry_dets,
                                const long long* carry_counts, const int* carry_ids, const int* carry_next_id, int min_iou_permille,
                                long long* inter, int* match, int* ids, int* linked, int* seq_tracks, int* next_id, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return link_detections_checked("link_detections_ragged", false, labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts, k, link,
                                 carry_labels, carry_h, carry_w, carry_dets, carry_counts, carry_ids, carry_next_id, min_iou_permille, inter,
                                 match, ids, linked, seq_tracks, next_id, nullptr, workspace, workspace_bytes, stream);
}
int udet_link_detections_motion_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                       size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                       const int* carry_labels, int carry_h, int carry_w, const long long* carry_dets,
                                       const long long* carry_counts, const int* carry_ids, const int* carry_next_id, int min_iou_permille,
                                       long long* inter, int* match, int* ids, int* linked, int* seq_tracks, int* next_id, const int* disp,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return link_detections_checked("link_detections_motion_ragged", true, labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts, k,
                                 link, carry_labels, carry_h, carry_w, carry_dets, carry_counts, carry_ids, carry_next_id, min_iou_permille,
                                 inter, match, ids, linked, seq_tracks, next_id, disp, workspace, workspace_bytes, stream);
}

// the history of udet_link_detections_gap_ragged: absent (no pointer, m = 0, 0 x 0) or whole (every pointer, 1..max_gap + 1 frames of at
// least 1 x 1 and below 2^31 pixels each)
static bool link_history_ok(int max_gap, int m, const void* labels, int h, int w, const void* dets, const void* counts, const void* ids,
                            const void* open, const void* next_id) {
  if (!labels && !dets && !counts && !ids && !open && !next_id) return m == 0 && h == 0 && w == 0;
  return labels && dets && counts && ids && open && next_id && m >= 1 && m <= max_gap + 1 && h >= 1 && w >= 1 &&
         (long)h * w <= 0x7fffffffL;
}
size_t udet_link_detections_gap_workspace_bytes(size_t total_pixels, int n, int k, int max_gap, int m, int hist_h, int hist_w) {
  if (n < 1 || total_pixels < 1 || k < 1 || k > UDET_DET_MAX_K || max_gap < 1 || max_gap > UDET_TRACK_MAX_GAP) return 0;
  if (m == 0 ? (hist_h != 0 || hist_w != 0) : (m < 1 || m > max_gap + 1 || hist_h < 1 || hist_w < 1 || (long)hist_h * hist_w > 0x7fffffffL))
    return 0;
  return link_detections_gap_workspace_bytes(total_pixels, m, hist_h, hist_w);
}
// udet_link_detections_gap_ragged (disp = nullptr, motion = false) and udet_link_detections_gap_motion_ragged
static int link_detections_gap_checked(const char* fn, bool motion, const int* labels, int n, const long long* offsets, const int* hw,
                                       int max_h, int max_w, size_t total_pixels, const long long* dets, const long long* counts, int k,
                                       const int* link, int max_gap, int m, const int* hist_labels, int hist_h, int hist_w,
                                       const long long* hist_dets, const long long* hist_counts, const int* hist_ids, int* hist_open,
                                       const int* hist_next_id, int min_iou_permille, long long* inter, int* match, int* ids, int* linked,
                                       int* seq_tracks, int* next_id, long long* gap_inter, int* back, int* prev, int* open, const int* disp,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch(fn, n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (motion && (!disp || (reinterpret_cast<uintptr_t>(disp) & 3))) {
    set_error("%s: disp must be a non-null, 4-byte aligned int32 buffer of total_pixels elements", fn);
    return UDET_ERR_ARG;
  }
  if (!labels || !offsets || !hw || !dets || !counts || !link || !inter || !match || !ids || !linked || !seq_tracks || !next_id ||
      !gap_inter || !back || !prev || !open) {
    set_error("%s: bad argument (non-null labels, offsets, hw, dets, counts, link and outputs)", fn);
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K || min_iou_permille < 1 || min_iou_permille > 1000 || max_gap < 1 || max_gap > UDET_TRACK_MAX_GAP) {
    set_error("%s: k = %d in 1..UDET_DET_MAX_K = %d, min_iou_permille = %d in 1..1000 and max_gap = %d in "
              "1..UDET_TRACK_MAX_GAP = %d are required", fn, k, UDET_DET_MAX_K, min_iou_permille, max_gap, UDET_TRACK_MAX_GAP);
    return UDET_ERR_ARG;
  }
  if (!link_history_ok(max_gap, m, hist_labels, hist_h, hist_w, hist_dets, hist_counts, hist_ids, hist_open, hist_next_id)) {
    set_error("%s: the history is either absent (no pointer, m = 0, 0 x 0) or whole (labels, dets, counts, ids, "
              "open and next id; m = %d in 1..max_gap + 1 = %d frames of %d x %d, at least 1 x 1 and below 2^31 pixels)", fn, m, max_gap + 1,
              hist_h, hist_w);
    return UDET_ERR_ARG;
  }
  if (bad_workspace(fn, workspace, workspace_bytes,
                    link_detections_gap_workspace_bytes(total_pixels, m, hist_h, hist_w), 4))
    return UDET_ERR_ARG;
  const uintptr_t a4 = reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(link) | reinterpret_cast<uintptr_t>(hist_labels) |
                       reinterpret_cast<uintptr_t>(hist_ids) | reinterpret_cast<uintptr_t>(hist_open) |
                       reinterpret_cast<uintptr_t>(hist_next_id) | reinterpret_cast<uintptr_t>(match) | reinterpret_cast<uintptr_t>(ids) |
                       reinterpret_cast<uintptr_t>(linked) | reinterpret_cast<uintptr_t>(seq_tracks) | reinterpret_cast<uintptr_t>(next_id) |
                       reinterpret_cast<uintptr_t>(back) | reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(open);
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(hist_dets) |
                       reinterpret_cast<uintptr_t>(hist_counts) | reinterpret_cast<uintptr_t>(inter) | reinterpret_cast<uintptr_t>(gap_inter);
  if ((a4 & 3) || (a8 & 7)) {
    set_error("%s: the int32 buffers must be 4-byte aligned, dets, counts, inter and gap_inter 8-byte aligned", fn);
    return UDET_ERR_ARG;
  }
  return launch_link_detections_gap_ragged(labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts, k, link, max_gap, m, hist_labels,
                                           hist_h, hist_w, hist_dets, hist_counts, hist_ids, hist_open, hist_next_id, min_iou_permille, inter,
                                           match, ids, linked, seq_tracks, next_id, gap_inter, back, prev, open, disp, workspace,
                                           (hipStream_t)stream);
}
int udet_link_detections_gap_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                    size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                    int max_gap, int m, const int* hist_labels, int hist_h, int hist_w, const long long* hist_dets,
                                    const long long* hist_counts, const int* hist_ids, int* hist_open, const int* hist_next_id,
                                    int min_iou_permille, long long* inter, int* match, int* ids, int* linked, int* seq_tracks,
                                    int* next_id, long long* gap_inter, int* back, int* prev, int* open, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return link_detections_gap_checked("link_detections_gap_ragged", false, labels, n, offsets, hw, max_h, max_w, total_pixels, dets, counts, k,
                                     link, max_gap, m, hist_labels, hist_h, hist_w, hist_dets, hist_counts, hist_ids, hist_open, hist_next_id,
                                     min_iou_permille, inter, match, ids, linked, seq_tracks, next_id, gap_inter, back, prev, open, nullptr,
                                     workspace, workspace_bytes, stream);
}
int udet_link_detections_gap_motion_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                           size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                           int max_gap, int m, const int* hist_labels, int hist_h, int hist_w, const long long* hist_dets,
                                           const long long* hist_counts, const int* hist_ids, int* hist_open, const int* hist_next_id,
                                           int min_iou_permille, long long* inter, int* match, int* ids, int* linked, int* seq_tracks,
                                           int* next_id, long long* gap_inter, int* back, int* prev, int* open, const int* disp,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return link_detections_gap_checked("link_detections_gap_motion_ragged", true, labels, n, offsets, hw, max_h, max_w, total_pixels, dets,
                                     counts, k, link, max_gap, m, hist_labels, hist_h, hist_w, hist_dets, hist_counts, hist_ids, hist_open,
                                     hist_next_id, min_iou_permille, inter, match, ids, linked, seq_tracks, next_id, gap_inter, back, prev,
                                     open, disp, workspace, workspace_bytes, stream);
}


int udet_draw_track_boxes_ragged(unsigned char* image_rgb, int n, const long long* offsets, const int* hw, size_t total_pixels,
                                 const long long* dets, const long long* counts, int k, const int* ids, int thickness,
                                 const unsigned* palette, int palette_size, void* stream) {
  if (bad_batch("draw_track_boxes_ragged", n, 1, 1, total_pixels)) return UDET_ERR_ARG;
  if (!image_rgb || !offsets || !hw || !dets || !counts || !ids || !palette) {
    set_error("draw_track_boxes_ragged: bad argument (non-null image_rgb, offsets, hw, dets, counts, ids and palette)");
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K || thickness < 1 || thickness > UDET_DRAW_MAX_THICKNESS || palette_size < 1 ||
      palette_size > UDET_TRACK_MAX_PALETTE) {
    set_error("draw_track_boxes_ragged: k = %d in 1..UDET_DET_MAX_K = %d, thickness = %d in 1..%d and a palette of %d in 1..%d colours are "
              "required", k, UDET_DET_MAX_K, thickness, UDET_DRAW_MAX_THICKNESS, palette_size, UDET_TRACK_MAX_PALETTE);
    return UDET_ERR_ARG;
  }
  if (((reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts)) & 7) ||
      ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(palette)) & 3)) {
    set_error("draw_track_boxes_ragged: dets and counts must be 8-byte aligned, ids and palette 4-byte aligned");
    return UDET_ERR_ARG;
  }
  return launch_draw_track_boxes_ragged(image_rgb, n, offsets, hw, dets, counts, k, ids, thickness, palette, palette_size,
                                        (hipStream_t)stream);
}

size_t udet_conv2d_workspace_bytes(int n, int h, int w, int cin, int cout, int kh, int kw, int upsample2x) {
  const int kc = round_up(cin > cout ? cin : cout, 8), ldw = round_up(cin > cout ? cin : cout, 4);
  const size_t pix_in = (size_t)n * h * w, pix_out = pix_in * (upsample2x ? 4 : 1);
  size_t b = 0;
  b += gran((size_t)kh * kw * kc * ldw);                       // packed weights
  b += gran(pix_in * round_up(cin, 8));                          // channel-padded x
  b += 2 * gran(pix_out * round_up(cout, 8));                    // channel-padded dy / y_saved
  b += gran(SPLITK_FLOATS);                                      // split-K partials
  b += gran(64 * wgrad_partial_floats_needed(kh * kw, cin, cout));
  return b + 8192 + gran(64 + UDET_MAX_TICKETS);
}

int udet_conv2d(const float* x, const float* w_hwio, const float* bias, float* y, int n, int h, int w, int cin, int cout,
                int kh, int kw, int stride, int dilation, int upsample2x, int act, float alpha, void* workspace,
                size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (kh * kw > UDET_MAX_TAPS || n < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || stride < 1 || dilation < 1) {
    set_error("conv2d: bad shape");
    return UDET_ERR_SHAPE;
  }
  Arena ar(workspace, workspace_bytes);
  const int kc = round_up(cin, 8), ldw = round_up(cout, 4);
  float* wp = ar.take((size_t)kh * kw * kc * ldw);
  const float* xin = x;
  int ldx = cin;
  if (cin % 8 != 0) {
    float* xp = ar.take((size_t)n * h * w * kc);
    if (!xp) { set_error("conv2d: workspace too small"); return UDET_ERR_ARG; }
    UDET_HIP(hipMemsetAsync(xp, 0, (size_t)n * h * w * kc * sizeof(float), stream));
    UDET_TRY(launch_copy_channels(x, cin, 0, xp, kc, 0, (long)n * h * w, cin, 1.f, 0.f, stream));
    xin = xp;
    ldx = kc;
  }
  float* part = ar.take(SPLITK_FLOATS);
  float* zero = ar.take(64 + UDET_MAX_TICKETS);  // 16-byte zero block + split-K tickets
  if (!wp || !part || !zero) { set_error("conv2d: workspace too small"); return UDET_ERR_ARG; }
  UDET_HIP(hipMemsetAsync(zero, 0, (64 + UDET_MAX_TICKETS) * sizeof(float), stream));
  UDET_TRY(launch_pack_weights(w_hwio, wp, kh * kw, cin, cout, kc, ldw, kc, 0, 0, nullptr, stream));
  ConvParams p;
  memset(&p, 0, sizeof(p));
  const int us = upsample2x ? 1 : 0;
  conv_setup_fwd(p, n, h << us, w << us, kh, kw, stride, dilation);
  p.x = xin; p.ldx = ldx; p.x_coff = 0; p.up_shift = us;
  p.wp = wp; p.Kc = kc; p.ldw = ldw; p.bias = bias;
  p.y = y; p.ldy = cout; p.y_coff = 0; p.Cout = cout;
  p.act = act; p.alpha = alpha;
  p.partial = part; p.partial_cap = SPLITK_FLOATS;
  p.zero16 = zero;
  p.tickets = reinterpret_cast<int*>(zero + 64);
  return launch_conv(p, stream);
}

int udet_conv2d_transpose4x4s2(const float* x, const float* w_hwoi, const float* bias, float* y, int n, int h, int w,
                               int cin, int cout, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  Arena ar(workspace, workspace_bytes);
  const int kc = round_up(cin, 8), ldw = round_up(cout, 4);
  float* wp = ar.take((size_t)16 * kc * ldw);
  const float* xin = x;
  int ldx = cin;
  if (cin % 8 != 0) {
    float* xp = ar.take((size_t)n * h * w * kc);
    if (!xp) { set_error("conv2d_transpose: workspace too small"); return UDET_ERR_ARG; }
    UDET_HIP(hipMemsetAsync(xp, 0, (size_t)n * h * w * kc * sizeof(float), stream));
    UDET_TRY(launch_copy_channels(x, cin, 0, xp, kc, 0, (long)n * h * w, cin, 1.f, 0.f, stream));
    xin = xp;
    ldx = kc;
  }
  float* part = ar.take(SPLITK_FLOATS);
  float* zero = ar.take(64 + UDET_MAX_TICKETS);  // 16-byte zero block + split-K tickets
  if (!wp || !part || !zero) { set_error("conv2d_transpose: workspace too small"); return UDET_ERR_ARG; }
  UDET_HIP(hipMemsetAsync(zero, 0, (64 + UDET_MAX_TICKETS) * sizeof(float), stream));
  // w is [t][cout][cin]; B operand wants [t][k=cin][n=cout]  -> mode 1 with (R=cout, C=cin)
  UDET_TRY(launch_pack_weights(w_hwoi, wp, 16, cout, cin, kc, ldw, kc, 0, 1, nullptr, stream));
  for (int cls = 0; cls < conv_dgrad_classes(2, 2 * h, 2 * w); ++cls) {
    ConvParams p;
    memset(&p, 0, sizeof(p));
    if (!conv_setup_dgrad(p, cls, n, 2 * h, 2 * w, 4, 4, 2, 1)) continue;
    p.x = xin; p.ldx = ldx; p.wp = wp; p.Kc = kc; p.ldw = ldw; p.bias = bias;
    p.y = y; p.ldy = cout; p.Cout = cout;
    p.partial = part; p.partial_cap = SPLITK_FLOATS;
    p.zero16 = zero;
    p.tickets = reinterpret_cast<int*>(zero + 64);
    UDET_TRY(launch_conv(p, stream));
  }
  return UDET_OK;
}

int udet_conv2d_backward_data(const float* dy, const float* y_saved, const float* w_hwio, float* dx, int n, int h, int w,
                              int cin, int cout, int kh, int kw, int stride, int dilation, int act, float alpha,
                              void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (stride != 1 && stride != 2) { set_error("conv2d_backward_data: stride %d unsupported", stride); return UDET_ERR_UNSUPPORTED; }
  Arena ar(workspace, workspace_bytes);
  const int kc = round_up(cout, 8), ldw = round_up(cin, 4);
  float* wp = ar.take((size_t)kh * kw * kc * ldw);
  int pt, pl, oh, ow;
  same_pad(h, kh, stride, dilation, &pt, &oh);
  same_pad(w, kw, stride, dilation, &pl, &ow);
  const float *dyin = dy, *yain = (act != UDET_ACT_NONE) ? y_saved : nullptr;
  int ldy = cout;
  if (cout % 8 != 0) {
    const size_t fl = (size_t)n * oh * ow * kc;
    float* a = ar.take(fl);
    float* b = ar.take(fl);
    if (!a || !b) { set_error("conv2d_backward_data: workspace too small"); return UDET_ERR_ARG; }
    UDET_HIP(hipMemsetAsync(a, 0, fl * sizeof(float), stream));
    UDET_TRY(launch_copy_channels(dy, cout, 0, a, kc, 0, (long)n * oh * ow, cout, 1.f, 0.f, stream));
    dyin = a;
    if (yain) {
      UDET_HIP(hipMemsetAsync(b, 0, fl * sizeof(float), stream));
      UDET_TRY(launch_copy_channels(y_saved, cout, 0, b, kc, 0, (long)n * oh * ow, cout, 1.f, 0.f, stream));
      yain = b;
    }
    ldy = kc;
  }
  float* part = ar.take(SPLITK_FLOATS);
  float* zero = ar.take(64 + UDET_MAX_TICKETS);  // 16-byte zero block + split-K tickets
  if (!wp || !part || !zero) { set_error("conv2d_backward_data: workspace too small"); return UDET_ERR_ARG; }
  UDET_HIP(hipMemsetAsync(zero, 0, (64 + UDET_MAX_TICKETS) * sizeof(float), stream));
  UDET_TRY(launch_pack_weights(w_hwio, wp, kh * kw, cin, cout, kc, ldw, kc, 0, 1, nullptr, stream));
  for (int cls = 0; cls < conv_dgrad_classes(stride, h, w); ++cls) {
    ConvParams p;
    memset(&p, 0, sizeof(p));
    if (!conv_setup_dgrad(p, cls, n, h, w, kh, kw, stride, dilation)) continue;
    p.x = dyin; p.ldx = ldy; p.xa = yain; p.xact = act; p.xalpha = alpha;
    p.wp = wp; p.Kc = kc; p.ldw = ldw; p.kreal = cout;
    p.f16_xscale = conv_debug_f16_grad_scale_now();  // (test hook; 0: none -- the x operand of this launch is a gradient)
    p.y = dx; p.ldy = cin; p.Cout = cin;
    p.partial = part; p.partial_cap = SPLITK_FLOATS;
    p.zero16 = zero;
    p.tickets = reinterpret_cast<int*>(zero + 64);
    UDET_TRY(launch_conv(p, stream));
  }
  return UDET_OK;
}

int udet_conv2d_backward_filter(const float* x, const float* dy, const float* y_saved, float* dw_hwio, float* dbias, int n,
                                int h, int w, int cin, int cout, int kh, int kw, int stride, int dilation, int upsample2x,
                                int act, float alpha, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  Arena ar(workspace, workspace_bytes);
  const int us = upsample2x ? 1 : 0;
  ConvParams g;
  memset(&g, 0, sizeof(g));
  conv_setup_fwd(g, n, h << us, w << us, kh, kw, stride, dilation);
  WgradParams p;
  memset(&p, 0, sizeof(p));
  const int cin8 = round_up(cin, 8), cout8 = round_up(cout, 8);
  const float* xin = x;
  int ldx = cin;
  if (cin % 4 != 0) {
    const size_t fl = (size_t)n * h * w * cin8;
    float* xp = ar.take(fl);
    if (!xp) { set_error("conv2d_backward_filter: workspace too small"); return UDET_ERR_ARG; }
    UDET_HIP(hipMemsetAsync(xp, 0, fl * sizeof(float), stream));
    UDET_TRY(launch_copy_channels(x, cin, 0, xp, cin8, 0, (long)n * h * w, cin, 1.f, 0.f, stream));
    xin = xp;
    ldx = cin8;
  }
  const float *dyin = dy, *yain = (act != UDET_ACT_NONE) ? y_saved : nullptr;
  int ldy = cout;
  if (cout % 4 != 0) {
    const size_t fl = (size_t)n * g.OH * g.OW * cout8;
    float* a = ar.take(fl);
    float* b = ar.take(fl);
    if (!a || !b) { set_error("conv2d_backward_filter: workspace too small"); return UDET_ERR_ARG; }
    UDET_HIP(hipMemsetAsync(a, 0, fl * sizeof(float), stream));
    UDET_TRY(launch_copy_channels(dy, cout, 0, a, cout8, 0, (long)n * g.OH * g.OW, cout, 1.f, 0.f, stream));
    dyin = a;
    if (yain) {
      UDET_HIP(hipMemsetAsync(b, 0, fl * sizeof(float), stream));
      UDET_TRY(launch_copy_channels(y_saved, cout, 0, b, cout8, 0, (long)n * g.OH * g.OW, cout, 1.f, 0.f, stream));
      yain = b;
    }
    ldy = cout8;
  }
  float* zero = ar.take(64);
  if (!zero) { set_error("conv2d_backward_filter: workspace too small"); return UDET_ERR_ARG; }
  UDET_HIP(hipMemsetAsync(zero, 0, 64 * sizeof(float), stream));
  const size_t pf = 64 * wgrad_partial_floats_needed(kh * kw, cin, cout);
  size_t avail = (ar.cap - ar.used) / sizeof(float);
  if (avail > 256) avail -= 256;
  const size_t takef = pf < avail ? pf : avail;
  float* part = ar.take(takef);
  if (!part) { set_error("conv2d_backward_filter: workspace too small"); return UDET_ERR_ARG; }
  p.x = xin; p.ldx = ldx; p.N = n; p.H = h << us; p.W = w << us; p.up_shift = us; p.Cin = cin;
  p.dy = dyin; p.ya = yain; p.ldy = ldy; p.Cout = cout; p.yact = act; p.yalpha = alpha;
  p.OH = g.OH; p.OW = g.OW; p.isy = p.isx = stride;
  p.ntaps = g.ntaps;
  memcpy(p.taps, g.taps, sizeof(g.taps));
  p.dw = dw_hwio; p.db = dbias; p.partial = part; p.partial_floats = takef;
  p.zero16 = zero;
  p.f16_yscale = conv_debug_f16_grad_scale_now();  // (test hook; 0: none)
  return launch_wgrad_T(p, kh * kw, stream);
}

/* ---- per-stage entry points of the loss / optimizer tail (SURVEY 8b minimum export list) ---------------------------- */
int udet_flow_normalize(const float* flow, float* out, int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!flow || !out || n < 1 || h < 1 || w < 1) { set_error("flow_normalize: bad argument"); return UDET_ERR_ARG; }
  if (bad_workspace("flow_normalize", workspace, workspace_bytes, flow_stats_doubles(n) * sizeof(double), 8)) return UDET_ERR_ARG;
  return launch_flow_normalize(flow, (double*)workspace, out, n, (long)h * w, (hipStream_t)stream);
}
size_t udet_stage_workspace_bytes(int n) {
  const size_t a = flow_stats_doubles(n) * sizeof(double), b = (loss_part_floats(n) + 5 * (size_t)n + 64) * sizeof(float);
  return (a > b ? a : b) + 256;
}
int udet_charbonnier_loss(const float* gt_flows, const float* pred_flows, const float* masks, int mask_channels, int n, int h, int w,
                          float cbn, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!gt_flows || !pred_flows || !out || n < 1 || h < 1 || w < 1 || (masks && mask_channels != 1 && mask_channels != 2)) {
    set_error("charbonnier_loss: bad argument (masks: null, 1 or 2 channels)");
    return UDET_ERR_ARG;
  }
  if (!workspace || workspace_bytes < udet_stage_workspace_bytes(n)) { set_error("charbonnier_loss: workspace too small"); return UDET_ERR_ARG; }
  return launch_charbonnier(gt_flows, pred_flows, masks, masks ? mask_channels : 1, n, (long)h * w, cbn, (float*)workspace, out, (hipStream_t)stream);
}
int udet_losses_forward(const float* flow, const float* mask, const float* pred3, int b, int h, int w, float cbn, float epsilon,
                        float* losses8, float* coef, void* workspace, size_t workspace_bytes, void* stream) {
  if (!flow || !mask || !pred3 || !losses8 || !coef || b < 1 || h < 1 || w < 1) { set_error("losses_forward: bad argument"); return UDET_ERR_ARG; }
  if (!workspace || workspace_bytes < udet_stage_workspace_bytes(b)) { set_error("losses_forward: workspace too small"); return UDET_ERR_ARG; }
  float* part = (float*)workspace;
  float* sums = part + loss_part_floats(b);
  return launch_losses(flow, mask, pred3, (long)h * w, b, cbn, epsilon, (float)w * (float)h * (float)b, part, losses8, coef, sums,
                       (hipStream_t)stream);
}
int udet_losses_backward(const float* flow, const float* mask, const float* pred3, const float* coef, int which, int b, int h, int w,
                         float cbn, float* dpred, float* dmask, void* stream) {
  if (!flow || !mask || !pred3 || !dpred || b < 1 || h < 1 || w < 1) { set_error("losses_backward: bad argument"); return UDET_ERR_ARG; }
  const long HW = (long)h * w;
  if (which == 2) return launch_rec_loss_bwd(flow, mask, pred3, dpred, (long)b * HW, cbn, 1.0f / ((float)w * (float)h * (float)b), (hipStream_t)stream);
  if (which == 1) {
    if (!coef || !dmask) { set_error("losses_backward: the generator loss needs coef (udet_losses_forward) and dmask"); return UDET_ERR_ARG; }
    return launch_gen_loss_bwd(flow, mask, pred3, coef, dpred, dmask, HW, b, cbn, (hipStream_t)stream);
  }
  set_error("losses_backward: which must be 1 (generator loss) or 2 (recover loss)");
  return UDET_ERR_ARG;
}
int udet_clip_or_noise(float* g, size_t n, float clip, const float* flag2, unsigned long long seed, long step, void* stream) {
  if (!g) { set_error("clip_or_noise: null gradient"); return UDET_ERR_ARG; }
  return launch_adam(nullptr, g, nullptr, nullptr, (long)n, 0.f, 0.f, 0.f, 0.f, clip, flag2, seed, (uint64_t)step, (hipStream_t)stream, 1);
}
int udet_adam_step(float* w, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, long t,
                   void* stream) {
  if (!w || !g || !m || !v || t < 1) { set_error("adam_step: bad argument (t counts applies from 1)"); return UDET_ERR_ARG; }
  const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t));
  return launch_adam(w, const_cast<float*>(g), m, v, (long)n, (float)lr_t, beta1, beta2, eps, 0.f, nullptr, 0, 0, (hipStream_t)stream, 2);
}
/* fused warp -> cost volume of one pyramid level (what the step plan launches); corr [n,h,w,81]; warped_dbg optional [n,h,w,c] */
int udet_warp_cost_volume(const float* c1, const float* c2, const float* flow, float flow_scale, float* corr, float* warped_dbg, int n,
                          int h, int w, int c, void* stream) {
  if (!c1 || !c2 || !corr) { set_error("warp_cost_volume: null argument"); return UDET_ERR_ARG; }
  return launch_warp_cost_volume(c1, c2, flow, 2, 0, flow_scale, corr, 81, 0, -1, warped_dbg, n, h, w, c, (hipStream_t)stream);
}

}  // extern "C"
