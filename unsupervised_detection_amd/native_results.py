"""Output stage at native resolution: restore a batch of masks to each frame's own size, score them there and export them.

Every mask the networks produce is img_height x img_width (192 x 384) and covers the central test_crop (0.9) of the frame; the
benchmarks (DAVIS-2016, FBMS-59, SegTrackV2) are scored on the full frame at each frame's own size with the strip outside the crop
counted as background.  The reference has that step in post_processing/crf_refine.py:84-97 (run_crf_original_resolution) and
post_processing/post_processing.py:32-46:

    soft = imresize(soft, (int(0.9 H), int(0.9 W)));  soft = soft / (amax(soft) + 1e-8);  zeros((H, W))[dh:dh+h, dw:dw+w] = soft

  restore_box(H, W, crop)                       the patch's box (y0, x0, h, w) inside an H x W frame
  build_restore_tables / check_restore_tables   the host tables of udet_restore_masks_ragged and their validation (no GPU needed)
  restore_masks(masks, native_hw, ...)          one call of the ragged kernel (csrc/restore.hip) -> RestoredMasks
  select_components(binary, offsets, hw, gt, mode, ...)   connected components of the restored masks and the choice of one per sample
                                                (csrc/components.hip, udet_select_components_ragged) -> ComponentSelection
  component_boxes(selection_or_labels, score, min_area, max_detections)   every component of the labelled masks as a scored box, the
                                                largest first (csrc/detections.hip, udet_component_boxes_ragged) -> Detections;
                                                detection_records: the same as plain records (box, area, centroid, score, root)
  link_detections(selection_or_labels, detections, link, carry, min_iou, max_gap)   the detections of consecutive frames linked into
                                                tracks by mask overlap (csrc/tracks.hip, udet_link_detections_ragged) -> Tracks; tail()
                                                carries the last frame into the next call; track_records / summarise_tracks: the records
                                                with their tracks, and every track of a sequence.  max_gap > 0: a track also survives
                                                up to max_gap frames without its component (udet_link_detections_gap_ragged), and tail()
                                                carries the last max_gap + 1 frames (TrackHistory)
  RestoredMasks / GtBatch / ComponentSelection  buffers of one batch in one ragged.PackedLayout (the packed layout): the
                                                annotations' layout is built once per batch and handed from call to call
  check_crf_tables / load_images_device / crf_refine_restored   the full-resolution dense CRF of run_crf_original_resolution on the
                                                restored batch: unary from the restored bytes, the frames read at their own size,
                                                one call of udet_dense_crf_ragged (csrc/crf.hip) -> the labels as the binary masks
  restore_results_dir(results_dir, frame_lists, out_dir, ...)   restore [+ CRF] [+ component selection] [+ detections [+ tracks]] + J / F +
                                                <sequence>/<frame>.png, result_<k>.mat, native_eval.json [, detections/<sequence>.json
                                                [, tracks/<sequence>.json]]
  frame_lists_from_reader(flags)                {category: [(image, annotation), ...]} in the readers' own test order; (image, None) for
                                                a folder of frames without annotations (--dataset FRAMES), which restore_results_dir
                                                takes in its annotation-free mode; overlay=... draws the final masks on the frames
                                                (visualize.overlay_native)

scipy.misc.imresize is restated as bytescale + Pillow's 8-bit bilinear resampler.  The "best detection candidate from
the set of predicted connected masks" the reference only mentions in a comment (post_processing.py:32-35) is select_components
(DESIGN.md 7.3).  The full-resolution CRF (sxy = 60) is restore_results_dir(crf={...}).  Every component as a box with
its area, centroid and score -- the detections -- is restore_results_dir(detections={...}); linking them across the
frames of a sequence is restore_results_dir(tracks={...}), across frames in which a component is missing with
tracks={"max_gap": G}."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import ragged
from ._ffi import c_i, c_p, c_sz, check, lib, sig
from .pil_tables import CoefBlocks, check_pass
from .post_processing import CRF_MAX_SAMPLES, default_radius, dense_crf_ragged, unary_from_restored
from .ragged import PackedLayout, PackedSamples, as_layout, check_packed_tables, require_tensor, workspace

sig("udet_restore_workspace_bytes", c_sz, c_i)
sig("udet_restore_masks_ragged", c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, ctypes.c_double, c_p, c_sz, c_p)
sig("udet_components_workspace_bytes", c_sz, c_sz, c_i)
sig("udet_select_components_ragged", c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p)

TAB = 12  # int32 per sample: y0 x0 h w H W | hk hb hks | vk vb vks   (include/udet.h)


def restore_box(H, W, crop):
    """(y0, x0, h, w) of the restored patch in an H x W frame: h = int(H * crop), w = int(W * crop) (Python float product,
    truncated, crf_refine.py:91-92), y0 = (H - h) // 2, x0 = (W - w) // 2; crop >= 1: the whole frame.  h, w >= 1."""
    H, W, crop = int(H), int(W), float(crop)
    if H < 1 or W < 1 or not crop > 0:
        raise ValueError("restore_box: frame {} x {} and crop {} must be positive".format(H, W, crop))
    if crop >= 1:
        return 0, 0, H, W
    h, w = int(H * crop), int(W * crop)
    if h < 1 or w < 1:
        raise ValueError("restore_box: the crop {} of a {} x {} frame is empty".format(crop, H, W))
    return (H - h) // 2, (W - w) // 2, h, w


def build_restore_tables(native_hw, mh, mw, crop=0.9, offsets=None):
    """Host tables of udet_restore_masks_ragged for masks of mh x mw restored into frames native_hw [n,2]: (offsets int64 [n],
    tab int32 [n,12], coef int32 [m]).  offsets default to the packed layout (sample i right after sample i-1).  One coefficient
    table (kk [out][ks] then bounds [out][2]) per distinct (in, out) length, concatenated in coef; a pass whose output length
    equals its input length gets index -1 (skipped)."""
    hw = np.asarray(native_hw, dtype=np.int64).reshape(-1, 2)
    n = len(hw)
    if n < 1:
        raise ValueError("restore needs at least one sample")
    if offsets is None:
        off = PackedLayout.packed(hw).offsets
    else:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        if len(off) != n:
            raise ValueError("one offset per sample")
    tab = np.zeros((n, TAB), np.int32)
    blocks = CoefBlocks()
    for i, (H, W) in enumerate(hw):
        y0, x0, h, w = restore_box(H, W, crop)
        tab[i] = (y0, x0, h, w, H, W) + blocks.block(mw, w) + blocks.block(mh, h)
    return off, tab, blocks.coef()


def check_restore_tables(offsets, tab, coef, numel, mh, mw):
    """Host validation of the device tables of udet_restore_masks_ragged (its C entry point does not read device memory): raises
    ValueError on tables ragged.check_packed_tables refuses for an output buffer of `numel` bytes, a box outside its own frame, a
    coefficient window outside coef, or a tap outside the mask.  Returns the three arrays in the dtypes the kernel reads."""
    tab = np.ascontiguousarray(np.asarray(tab, dtype=np.int32).reshape(-1, TAB))
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.int32).reshape(-1))
    if mh < 1 or mw < 1:
        raise ValueError("restore needs a mask of at least 1x1")
    t = tab.astype(np.int64)
    y0, x0, h, w, H, W = (t[:, k] for k in range(6))
    off, _ = check_packed_tables(offsets, t[:, 4:6], numel, buffer="output buffer")
    n = len(off)
    if (y0 < 0).any() or (x0 < 0).any() or (h < 1).any() or (w < 1).any() or (y0 + h > H).any() or (x0 + w > W).any():
        raise ValueError("box outside its own frame")
    for i in range(n):
        for name, block, n_in, n_out in (("horizontal", t[i, 6:9], mw, w[i]), ("vertical", t[i, 9:12], mh, h[i])):
            check_pass(coef, block, n_in, n_out, "sample {}".format(i), name)
    return off, tab, coef


class RestoredMasks(PackedSamples):
    """Result of restore_masks: data (packed uint8, device), binary (same layout, 0 / 1, or None), amax (device int32 [n]); their
    `layout` is given as host offsets [n] / hw [n,2], or as the PackedLayout itself (hw=None)."""

    def __init__(self, data, binary, offsets, hw, amax):
        PackedSamples.__init__(self, as_layout(offsets, hw, data.numel()), data.device)
        self.data, self.binary, self.amax = data, binary, amax

    def sample(self, i):
        """[H_i, W_i] uint8 view of sample i."""
        return self._view(self.data, i)

    def binary_sample(self, i):
        if self.binary is None:
            raise ValueError("restored without a threshold: no binary mask")
        return self._view(self.binary, i)

    def soft(self, i):
        """float64 [H_i, W_i] = byte / (amax + 1e-8): the mask run_crf_original_resolution hands to its CRF (crf_refine.py:94)."""
        return self.sample(i).double() / (self.amax[i].double() + 1e-8)


# Everything the restore tables are built from -> [the layout of a call that gave none, off, tab, coef, {device: (tab, coef) there}]: a
# batch with the sizes of an earlier one (every DAVIS batch) has its tables built, validated and uploaded once.
_restore_tables = {}


def restore_masks(masks, native_hw, crop=0.9, threshold=None, offsets=None, out=None, binary_out=None) -> RestoredMasks:
    """n soft masks [n,mh,mw] or [n,mh,mw,1] (device float32, or an array) -> each restored to its own native_hw[i] = (H_i, W_i):
    bytescale over the whole mask, Pillow's 8-bit bilinear resize to restore_box(H_i, W_i, crop), pasted into zeros; amax[i] = the
    patch's largest byte; threshold (float, optional): also the binary mask byte / (amax + 1e-8) > threshold (float64).  One call
    of udet_restore_masks_ragged: at most three launches for the whole batch.  offsets / out / binary_out: a caller-owned packed
    uint8 buffer and the byte offset of every sample in it (default: a fresh buffer, samples back to back).  native_hw may be the
    PackedLayout of the output (the annotations' own: its sizes, offsets and device tables are used as they are).  The tables are
    validated on the host before anything is launched (ValueError)."""
    m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32))
    if m.dim() == 4 and m.shape[-1] == 1:
        m = m[..., 0]
    if m.dim() != 3:
        raise ValueError("masks must be [n,mh,mw] or [n,mh,mw,1]")
    n, mh, mw = (int(v) for v in m.shape)
    given = native_hw if isinstance(native_hw, PackedLayout) else None
    hw = np.asarray(native_hw, dtype=np.int64).reshape(-1, 2)
    if len(hw) != n or (given is not None and offsets is not None):
        raise ValueError("one native size per mask (a PackedLayout brings its own offsets)")
    if given is not None:
        offsets = given.offsets
    total = int(out.numel()) if out is not None else (int((hw[:, 0] * hw[:, 1]).sum()) if given is None else given.numel)
    if threshold is not None and not (0.0 <= float(threshold) < float("inf")):
        raise ValueError("threshold must be finite and >= 0")
    key = (hw.tobytes(), None if offsets is None else np.asarray(offsets, dtype=np.int64).tobytes(), total, mh, mw, float(crop))
    if key not in _restore_tables:  # before the device is touched
        off, tab, coef = check_restore_tables(*build_restore_tables(hw, mh, mw, crop, offsets), total, mh, mw)
        if len(_restore_tables) >= 16:
            _restore_tables.clear()
        _restore_tables[key] = [None, off, tab, coef, {}]
    entry = _restore_tables[key]
    if given is None and entry[0] is None:
        entry[0] = PackedLayout(entry[1], hw, total, buffer="output buffer")
    layout = entry[0] if given is None else as_layout(given, None, total, buffer="output buffer")
    tab, coef, on_device = entry[2:]
    m = m.to("cuda", torch.float32).contiguous()
    dev = m.device
    for buf, name in ((out, "out"), (binary_out, "binary_out")):
        if buf is not None:
            require_tensor(buf, name + " (the output buffer)", torch.uint8, 1, total)
    data = torch.empty(total, dtype=torch.uint8, device=dev) if out is None else out
    binary = None
    if threshold is not None:
        binary = torch.empty(total, dtype=torch.uint8, device=dev) if binary_out is None else binary_out
    if dev not in on_device:
        on_device[dev] = ragged.upload_tables([tab, coef], dev)
        torch.cuda.current_stream(dev).synchronize()  # once per table set: a later call may run on another stream
    (d_tab, d_coef), (d_off, _) = on_device[dev], layout.device_tables(dev)
    amax = torch.empty(n, dtype=torch.int32, device=dev)  # zeroed by the call
    ws = workspace(lib.udet_restore_workspace_bytes(n), 4, dev)
    check(lib.udet_restore_masks_ragged(m.data_ptr(), n, mh, mw, d_off.data_ptr(), d_tab.data_ptr(), d_coef.data_ptr(),
                                        layout.max_h, layout.max_w, data.data_ptr(), amax.data_ptr(),
                                        None if binary is None else binary.data_ptr(), 0.0 if threshold is None else float(threshold),
                                        ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return RestoredMasks(data, binary, layout, None, amax)


# ---------------------------------------------------------------------------------------------------------------------------
# Ground truth at native size, scoring and export
# ---------------------------------------------------------------------------------------------------------------------------
class GtRule(object):
    """How a dataset's annotation becomes a boolean mask at native size: loader(path, channels) -> uint8 [H,W,1] on the host (None:
    the 8-bit grey decode of data._read_image), then value / 255 > threshold on the device."""

    def __init__(self, loader=None, threshold=0.1):
        self.loader, self.threshold = loader, float(threshold)


def _fbms_loader(path, channels):
    from . import data, datasets
    return datasets.fbms_gt_mask(path, data._read_image(path, 3))


def _segtrack_loader(path, channels):
    from . import datasets
    return datasets.read_decode_jpeg(path, 1)


# DAVIS and SegTrackV2: scipy.misc.imread(gt) / 255. > 0.1 (crf_refine.py:89,131).  FBMS: datasets.fbms_gt_mask -- the per-sequence
# binarisation of the source annotation and the JPEG round trip of the reference's converted files; 0.5 undoes the round trip's
# ringing and gives back the binarised annotation.
GT_RULES = {"DAVIS2016": GtRule(None, 0.1), "SEGTRACK": GtRule(_segtrack_loader, 0.1), "FBMS": GtRule(_fbms_loader, 0.5)}


class GtBatch(PackedSamples):
    """Annotations of one batch, binarised at native size: data (packed uint8 0 / 1) in the layout given as host offsets / hw, or as
    the PackedLayout itself (hw=None)."""

    def __init__(self, data, offsets, hw=None):
        PackedSamples.__init__(self, as_layout(offsets, hw, data.numel()), data.device)
        self.data = data

    def sample(self, i):
        return self._view(self.data, i)

    binary_sample = sample


_ragged_loader = None


def load_gt_device(paths, rule):
    """The annotations of a batch through data.RaggedLoader (mixed sizes: one pinned buffer, one copy), binarised on the device."""
    global _ragged_loader
    from . import data
    if _ragged_loader is None:
        _ragged_loader = data.RaggedLoader()
    rb = _ragged_loader.load(list(paths), 1, loader=rule.loader)
    return GtBatch((rb.data.double() / 255.0 > rule.threshold).to(torch.uint8), rb.layout)


def score_device(gt_stack, pred_stack, bound_th):
    """(J, F) per frame of [k,H,W,1] 0 / 1 stacks, scored as they are (no fg/bg flip)."""
    from .evaluation import evaluate_batch_davis
    _, _, _, j, f = evaluate_batch_davis(gt_stack, pred_stack, 0.5, bound_th, disambiguate=False)
    return j, f


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


# ---------------------------------------------------------------------------------------------------------------------------
# Connected components and the choice of one candidate per sample (csrc/components.hip)
# ---------------------------------------------------------------------------------------------------------------------------
COMPONENT_MODES = {"label": 0, "largest": 1, "best_gt": 2}  # UDET_COMPONENTS_LABEL / _LARGEST / _BEST_GT (include/udet.h)
COMPONENT_TILE = (32, 64)  # UDET_COMPONENTS_TILE_H / _W: the tile of the LDS union-find


def check_component_tables(offsets, hw, numel):
    """Host validation of the device tables of udet_select_components_ragged: ragged.check_packed_tables for a packed buffer of
    `numel` elements.  Returns (offsets int64 [n], hw int32 [n,2]) as the kernels read them."""
    return check_packed_tables(offsets, hw, numel)


class ComponentSelection(PackedSamples):
    """Result of select_components: selected (packed uint8 0 / 1, device; None in mode "label"), labels (packed int32, root + 1 /
    0, or None), info (device int64 [n,4] = components, chosen root or -1, its area, its inter); their `layout` is given as host
    offsets [n] / hw [n,2], or as the PackedLayout itself (hw=None).  binary_sample / stack have the contract of RestoredMasks: the
    scoring and export loops take either."""

    def __init__(self, selected, labels, info, offsets, hw):
        if isinstance(offsets, PackedLayout) or selected is not None or labels is not None:
            numel = offsets.numel if isinstance(offsets, PackedLayout) else (labels if selected is None else selected).numel()
        else:  # no packed buffer to measure: the tables' own extent
            numel = int((np.asarray(offsets, np.int64).reshape(-1) + np.asarray(hw, np.int64).reshape(-1, 2).prod(1)).max())
        PackedSamples.__init__(self, as_layout(offsets, hw, numel), info.device)
        self.selected, self.labels, self.info = selected, labels, info

    def binary_sample(self, i):
        if self.selected is None:
            raise ValueError("labelled without a selection: no selected mask")
        return self._view(self.selected, i)

    def labels_sample(self, i):
        if self.labels is None:
            raise ValueError("selected without want_labels: no labels")
        return self._view(self.labels, i)


def select_components(binary, offsets=None, hw=None, gt=None, mode="largest", connectivity=8, want_labels=False) -> ComponentSelection:
    """Connected components of n packed binary masks and one of them chosen per sample, in one call of
    udet_select_components_ragged (five launches whatever n is).  binary: a RestoredMasks (its binary masks and layout), or a 1-D
    uint8 device tensor with host offsets [n] / hw [n,2] (or a PackedLayout as offsets, hw=None: taken as it is); gt: a GtBatch or a
    1-D uint8 device tensor packed like binary, or None.  connectivity 4 or 8.  mode "label": components only; "largest": the largest component, ties to the smaller root (the
    smallest row-major index of the component); "best_gt": the largest IoU with gt, ties to the larger area, then the smaller root.
    want_labels: also the int32 labels (root + 1, background 0; the roots in ascending order number as scipy.ndimage.label does).
    Arguments and tables are validated on the host before the device is touched (ValueError)."""
    if isinstance(binary, RestoredMasks):
        if binary.binary is None:
            raise ValueError("restored without a threshold: no binary mask")
        binary, offsets, hw = binary.binary, binary.layout, None
    if offsets is None or (hw is None and not isinstance(offsets, PackedLayout)):
        raise ValueError("a packed buffer needs its offsets and sizes")
    if mode not in COMPONENT_MODES:
        raise ValueError("mode must be one of {}".format(sorted(COMPONENT_MODES)))
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    total = int(require_tensor(binary, "binary (packed samples)", torch.uint8, 1, cuda=False).numel())
    layout = as_layout(offsets, hw, total)  # raw tables: validated before the device is touched
    if isinstance(gt, GtBatch):
        if not gt.layout.same_as(layout):
            raise ValueError("the annotations must be packed like the masks (same offsets and sizes)")
        gt = gt.data
    if mode == "best_gt" and gt is None:
        raise ValueError('mode "best_gt" needs the annotations')
    dev, n = binary.device, layout.n
    if gt is not None:
        require_tensor(gt, "gt (packed like binary)", torch.uint8, 1, total, dev)
    require_tensor(binary, "binary (packed samples)", torch.uint8, 1)
    d_off, d_hw = layout.device_tables(dev)
    selected = torch.empty(total, dtype=torch.uint8, device=dev) if mode != "label" else None
    labels = torch.empty(total, dtype=torch.int32, device=dev) if want_labels else None
    info = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ws = workspace(lib.udet_components_workspace_bytes(total, n), 8, dev)
    check(lib.udet_select_components_ragged(binary.data_ptr(), None if gt is None else gt.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(),
                                            layout.max_h, layout.max_w, total, int(connectivity), COMPONENT_MODES[mode],
                                            None if labels is None else labels.data_ptr(), None if selected is None else selected.data_ptr(),
                                            info.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return ComponentSelection(selected, labels, info, layout, None)


# ---------------------------------------------------------------------------------------------------------------------------
# Every component as a scored box: the detections at native size (csrc/detections.hip)
# ---------------------------------------------------------------------------------------------------------------------------
DET_FIELDS = 9  # UDET_DET_FIELDS: root, area, y0, x0, y1, x1, sum_y, sum_x, score_sum
DET_MAX_K = 64  # UDET_DET_MAX_K
DETECTION_DEFAULTS = {"min_area": 64, "max_detections": 16}


def detection_params(detections=None):
    """The `detections` dict of restore_results_dir ({} or None: the defaults) with the defaults filled in and checked (ValueError):
    min_area an integer >= 1, max_detections an integer in 1..DET_MAX_K."""
    p = dict(DETECTION_DEFAULTS)
    if detections is not None:
        if not isinstance(detections, dict) or not set(detections) <= set(DETECTION_DEFAULTS):
            raise ValueError("detections must be a dict with keys among {}".format(sorted(DETECTION_DEFAULTS)))
        p.update({k: v for k, v in detections.items() if v is not None})
    for k in p:
        if isinstance(p[k], bool) or int(p[k]) != p[k]:
            raise ValueError("detections: {} must be an integer".format(k))
        p[k] = int(p[k])
    if p["min_area"] < 1 or p["min_area"] > ragged.INT32_MAX or not 1 <= p["max_detections"] <= DET_MAX_K:
        raise ValueError("detections: min_area >= 1 (below 2^31) and max_detections in 1..{} are required".format(DET_MAX_K))
    return p


class Detections(PackedSamples):
    """Result of component_boxes: dets (device int64 [n, k, DET_FIELDS]: per sample the components with area >= min_area, largest first,
    ties to the smaller root; the rows past the last one hold root = -1 and zeros), counts (device int64 [n, 3] = components, kept, rows
    written), min_area, k; `layout` is that of the labels they were computed from."""

    def __init__(self, dets, counts, layout, min_area, k):
        PackedSamples.__init__(self, layout, dets.device)
        self.dets, self.counts, self.min_area, self.k = dets, counts, int(min_area), int(k)
        self._host = None

    def host(self):
        """(dets, counts) as numpy arrays: one copy of each per Detections, made on first use."""
        if self._host is None:
            self._host = (_host(self.dets), _host(self.counts))
        return self._host

    def rows(self, i):
        """Host view int64 [rows written, DET_FIELDS] of sample i."""
        dets, counts = self.host()
        return dets[i, :int(counts[i, 2])]


def component_boxes(selection_or_labels, score=None, min_area=64, max_detections=16, offsets=None, hw=None) -> Detections:
    """Every connected component of n labelled masks as a scored box, in one call of udet_component_boxes_ragged (four launches
    whatever n and the number of components; nothing comes back to the host).  selection_or_labels: a ComponentSelection that has labels
    (select_components(..., want_labels=True), any mode), or a 1-D int32 device tensor of labels (root + 1 / 0) with host offsets [n] /
    hw [n,2] (or a PackedLayout as offsets, hw=None).  score: optional, a RestoredMasks (its soft bytes `data`) or a 1-D uint8 device
    tensor packed like the labels.  Per sample the components of at least min_area pixels, largest first (ties to the smaller root),
    at most max_detections (1..DET_MAX_K) of them: root, area, y0, x0, y1, x1 (y1 / x1 exclusive), sum_y, sum_x, score_sum -- exact
    integers.  Arguments and tables are validated on the host before the device is touched (ValueError)."""
    if isinstance(selection_or_labels, ComponentSelection):
        if selection_or_labels.labels is None:
            raise ValueError("selected without want_labels: no labels")
        if offsets is not None or hw is not None:
            raise ValueError("a ComponentSelection brings its own layout")
        labels, offsets = selection_or_labels.labels, selection_or_labels.layout
    else:
        labels = selection_or_labels
    if offsets is None or (hw is None and not isinstance(offsets, PackedLayout)):
        raise ValueError("a packed buffer needs its offsets and sizes")
    p = detection_params({"min_area": min_area, "max_detections": max_detections})
    total = int(require_tensor(labels, "labels (packed samples)", torch.int32, 1, cuda=False).numel())
    layout = as_layout(offsets, hw, total, max_samples=65535)  # raw tables: validated before the device is touched
    if isinstance(score, RestoredMasks):
        if not score.layout.same_as(layout):
            raise ValueError("the scores must be packed like the labels (same offsets and sizes)")
        score = score.data
    if score is not None:
        require_tensor(score, "score (packed like the labels)", torch.uint8, 1, total, cuda=False)
    require_tensor(labels, "labels (packed samples)", torch.int32, 1)
    dev, n, k = labels.device, layout.n, p["max_detections"]
    if score is not None:
        require_tensor(score, "score (packed like the labels)", torch.uint8, 1, total, dev)
    d_off, d_hw = layout.device_tables(dev)
    dets = torch.empty((n, k, DET_FIELDS), dtype=torch.int64, device=dev)
    counts = torch.empty((n, 3), dtype=torch.int64, device=dev)
    ws = workspace(lib.udet_component_boxes_workspace_bytes(total, n, k), 8, dev)
    check(lib.udet_component_boxes_ragged(labels.data_ptr(), None if score is None else score.data_ptr(), n, d_off.data_ptr(),
                                          d_hw.data_ptr(), layout.max_h, layout.max_w, total, p["min_area"], k, dets.data_ptr(),
                                          counts.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return Detections(dets, counts, layout, p["min_area"], k)


def detection_records(detections, amax):
    """The detections of a batch as plain records: per frame a list, in rank order, of {"box": [x0, y0, x1, y1] (x1 / y1 exclusive),
    "area", "centroid": [sum_x / area, sum_y / area], "score": score_sum / (area * (amax + 1e-8)) in float64 -- the mean of
    RestoredMasks.soft over the component -- and "root"}.  detections: a Detections (or anything with len() and rows(i)); amax: the
    batch's RestoredMasks.amax (one integer per frame)."""
    amax = _host(amax).reshape(-1)
    if len(amax) != len(detections):
        raise ValueError("one amax per frame")
    out = []
    for i in range(len(detections)):
        recs = []
        for root, area, y0, x0, y1, x1, sy, sx, ss in (tuple(int(v) for v in row) for row in detections.rows(i)):
            recs.append({"box": [x0, y0, x1, y1], "area": area, "centroid": [sx / area, sy / area],
                         "score": float(np.float64(ss) / (np.float64(area) * (np.float64(amax[i]) + 1e-8))), "root": root})
        out.append(recs)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Detections linked into tracks across consecutive frames (csrc/tracks.hip)
# ---------------------------------------------------------------------------------------------------------------------------
TRACK_DEFAULTS = {"min_iou": 0.1}


def min_iou_permille(min_iou):
    """round(1000 min_iou) as the kernels take the threshold: an integer in 1..1000 (ValueError otherwise)."""
    try:
        p = int(round(1000.0 * float(min_iou)))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("tracks: min_iou must be a number")
    if isinstance(min_iou, bool) or not 1 <= p <= 1000:
        raise ValueError("tracks: min_iou must round to a permille in 1..1000: round(1000 min_iou)")
    return p


def track_params(tracks=None):
    """The `tracks` dict of restore_results_dir ({} or None: the defaults) with the defaults filled in and checked (ValueError)."""
    p = dict(TRACK_DEFAULTS)
    if tracks is not None:
        if not isinstance(tracks, dict) or not set(tracks) <= set(TRACK_DEFAULTS) | {"max_gap"}:
            raise ValueError("tracks must be a dict with keys among {}".format(sorted(set(TRACK_DEFAULTS) | {"max_gap"})))
        p.update({k: v for k, v in tracks.items() if v is not None})
    min_iou_permille(p["min_iou"])
    p["min_iou"] = float(p["min_iou"])
    gap = track_max_gap(p.pop("max_gap", 0))
    if gap:  # the key only when gaps are bridged: without it the dict is what it was
        p["max_gap"] = gap
    return p


TRACK_MAX_GAP = 8  # UDET_TRACK_MAX_GAP


def track_max_gap(max_gap):
    """max_gap as the link takes it: an int in 0..TRACK_MAX_GAP, 0: no gap bridging (ValueError otherwise; bools and floats are refused)."""
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= TRACK_MAX_GAP:
        raise ValueError("tracks: max_gap must be an int in 0..{}".format(TRACK_MAX_GAP))
    return int(max_gap)


def _clone(x):
    return x.clone() if isinstance(x, torch.Tensor) else np.array(x, copy=True)


class TrackTail(object):
    """The last frame of a link_detections call, as the next call's `carry`: labels (int32 [h * w]), hw = (h, w), dets (int64 [k, 9]),
    counts (int64 [3]), ids (int32 [k]) and next_id (int32 [1]: the next free id of the frame's sequence) -- copies, on the device."""

    def __init__(self, labels, hw, dets, counts, ids, next_id):
        self.labels, self.hw, self.dets, self.counts, self.ids, self.next_id = labels, (int(hw[0]), int(hw[1])), dets, counts, ids, next_id
        self.k = int(dets.shape[0])


class TrackHistory(object):
    """The last m <= max_gap + 1 frames of a sequence linked with gap bridging, oldest first, as the next call's `carry`: labels (int32
    [m, h * w]), hw = (h, w), dets (int64 [m, k, 9]), counts (int64 [m, 3]), ids and open (int32 [m, k]: open is 1 on a row without a
    successor so far) and next_id (int32 [1]) -- copies, on the device."""

    def __init__(self, labels, hw, dets, counts, ids, open, next_id, max_gap):
        self.labels, self.hw, self.dets, self.counts, self.ids, self.open, self.next_id = labels, (int(hw[0]), int(hw[1])), dets, counts, ids, open, next_id
        self.m, self.k, self.max_gap = int(dets.shape[0]), int(dets.shape[1]), int(max_gap)


def _frames(parts):
    return torch.cat(parts) if isinstance(parts[0], torch.Tensor) else np.concatenate(parts)


class Tracks(object):
    """Result of link_detections for the n frames of `detections`: inter (int64 [n, k, k]), match (int32 [n, k]), ids (int32 [n, k]),
    linked (int32 [n]), seq_tracks (int32 [n]) and next_id (int32 [1]) as include/udet.h defines them, on the device; labels: the packed
    labels they were computed from; carry: the TrackTail frame 0 was linked against, or None.  Linked with gap bridging (max_gap > 0):
    gap_inter (int64 [n, max_gap, k, k]), back, prev and open (int32 [n, k]) as well, carry is the TrackHistory or None and hist_open
    (int32 [m, k]) its open flags after this call."""

    def __init__(self, inter, match, ids, linked, seq_tracks, next_id, labels, detections, carry=None, back=None, prev=None, gap_inter=None,
                 open=None, max_gap=0, hist_open=None):
        self.inter, self.match, self.ids, self.linked, self.seq_tracks, self.next_id = inter, match, ids, linked, seq_tracks, next_id
        self.labels, self.detections, self.carry, self.k = labels, detections, carry, int(ids.shape[1])
        self.back, self.prev, self.gap_inter, self.open, self.max_gap, self.hist_open = back, prev, gap_inter, open, int(max_gap), hist_open
        self.layout = getattr(detections, "layout", None)  # (a numpy stand-in of the detections has none: it brings its own tail())
        self._host = self._host_gaps = None

    def __len__(self):
        return int(self.ids.shape[0])

    def host(self):
        """(inter, match, ids, linked, seq_tracks) as numpy arrays: one copy of each per Tracks, made on first use."""
        if self._host is None:
            self._host = tuple(_host(t) for t in (self.inter, self.match, self.ids, self.linked, self.seq_tracks))
        return self._host

    def rows(self, i):
        """Host views (ids, match) of the rows written for frame i, in rank order."""
        _, match, ids, _, _ = self.host()
        r = len(self.detections.rows(i))
        return ids[i, :r], match[i, :r]

    def host_gaps(self):
        """(gap_inter, back, prev, open) as numpy arrays (max_gap > 0): one copy of each per Tracks, made on first use."""
        if self._host_gaps is None:
            self._host_gaps = tuple(_host(t) for t in (self.gap_inter, self.back, self.prev, self.open))
        return self._host_gaps

    def tail(self):
        """The last frame -- its labels, det rows, counts, ids -- and its sequence's next free id, cloned: the next call's `carry`.
        With max_gap > 0 a TrackHistory: the last min(max_gap + 1, frames of the call's last sequence, the history's included) frames
        with their open flags as this call left them (reads `linked` on the host)."""
        i = len(self) - 1
        o, (h, w) = int(self.layout.offsets[i]), (int(v) for v in self.layout.hw[i])
        if not self.max_gap:
            return TrackTail(_clone(self.labels[o:o + h * w]), (h, w), _clone(self.detections.dets[i]), _clone(self.detections.counts[i]),
                             _clone(self.ids[i]), _clone(self.next_id))
        linked = self.host()[3]
        first = i  # of the call's last sequence
        while first > 0 and linked[first]:
            first -= 1
        lo = max(first, i - self.max_gap)  # the call's frames lo .. i
        offs = [int(self.layout.offsets[f]) for f in range(lo, i + 1)]
        parts = [[self.labels[o:o + h * w].reshape(1, h * w) for o in offs], [self.detections.dets[lo:i + 1]],
                 [self.detections.counts[lo:i + 1]], [self.ids[lo:i + 1]], [self.open[lo:i + 1]]]
        if first == 0 and linked[0]:  # the sequence reaches into the history: its newest frames in front
            c = self.carry
            keep = slice(max(0, c.m - (self.max_gap - i)), c.m)
            parts = [[old[keep]] + new for old, new in zip((c.labels.reshape(c.m, h * w), c.dets, c.counts, c.ids, self.hist_open), parts)]
        lab, dets, counts, ids, open = (_clone(_frames(p)) for p in parts)
        return TrackHistory(lab, (h, w), dets, counts, ids, open, _clone(self.next_id), self.max_gap)


def check_link_arguments(layout, detections, link, carry, min_iou, max_gap=0):
    """The host validation of link_detections (ValueError): `layout` (the labels') equals the detections', dets / counts have their shapes, link is None or n values 0 / 1, carry is None or a TrackTail of the same k (max_gap > 0: a TrackHistory of the same k and max_gap), min_iou
    rounds to a permille in 1..1000.  Returns (link as int32 [n] or None when it is a device tensor, permille)."""
    n, k = detections.layout.n, int(detections.k)
    if not layout.same_as(detections.layout):
        raise ValueError("the labels must be packed like the detections' frames (same offsets and sizes)")
    if tuple(detections.dets.shape) != (n, k, DET_FIELDS) or tuple(detections.counts.shape) != (n, 3) or not 1 <= k <= DET_MAX_K:
        raise ValueError("detections: dets must be [{}, k, {}] and counts [{}, 3] with k in 1..{}".format(n, DET_FIELDS, n, DET_MAX_K))
    permille = min_iou_permille(min_iou)
    if max_gap and carry is not None:
        if not isinstance(carry, TrackHistory) or carry.k != k or carry.max_gap != max_gap:
            raise ValueError("carry must be the tail() of the previous call's Tracks, linked with the same k = {} and max_gap = {}".format(k, max_gap))
        m, hw = carry.m, carry.hw[0] * carry.hw[1]
        shapes = ((carry.labels, (m, hw)), (carry.dets, (m, k, DET_FIELDS)), (carry.counts, (m, 3)), (carry.ids, (m, k)), (carry.open, (m, k)),
                  (carry.next_id, (1,)))
        if not 1 <= m <= max_gap + 1 or min(carry.hw) < 1 or any(tuple(t.shape) != s for t, s in shapes):
            raise ValueError("carry: the history must hold 1..max_gap + 1 frames of h * w labels with their dets, counts, ids and open flags")
    elif carry is not None:
        if not isinstance(carry, TrackTail):
            raise ValueError("carry must be the tail() of the previous call's Tracks")
        if carry.k != k or tuple(carry.dets.shape) != (k, DET_FIELDS) or int(np.prod(carry.ids.shape)) != k:
            raise ValueError("carry: the carried frame was linked with k = {}, this call has k = {}".format(carry.k, k))
        if int(np.prod(carry.labels.shape)) != carry.hw[0] * carry.hw[1] or min(carry.hw) < 1:
            raise ValueError("carry: labels must hold h * w elements")
    if link is None:
        return np.ones(n, np.int32), permille
    if isinstance(link, torch.Tensor) and link.is_cuda:
        require_tensor(link, "link (one int32 per frame)", torch.int32, 1, n)
        return None, permille
    host = np.asarray(_host(link)).reshape(-1)
    if len(host) != n or not np.isin(host, (0, 1)).all():
        raise ValueError("link must hold one 0 / 1 per frame ({} frames)".format(n))
    return np.ascontiguousarray(host.astype(np.int32)), permille


def link_detections(selection_or_labels, detections, link=None, carry=None, min_iou=0.1, max_gap=0) -> Tracks:
    """The detections of n consecutive frames linked into tracks by mask overlap, in one call of udet_link_detections_ragged (four
    launches whatever n and the number of sequences and components; nothing comes back to the host).  selection_or_labels: the
    ComponentSelection (with labels) or the 1-D int32 device tensor of labels `detections` (a Detections) was computed from.  link: one
    0 / 1 per frame, 1: the frame continues the one before it (frame 0: `carry`), 0: it starts a sequence; None: every frame continues.
    carry: the tail() of the previous call's Tracks, or None (frame 0 then starts a sequence).  A frame whose predecessor has another
    size starts a sequence too.  Rows a of the predecessor and b of the frame share inter pixels; pairs with IoU = inter / (area_a +
    area_b - inter) >= min_iou (as the permille round(1000 min_iou), 1..1000) are matched greedily, the largest IoU first (ties to
    the smaller a, then the smaller b); a matched row inherits its predecessor's track id, the others take the sequence's next free
    ids in rank order -- exact integers (include/udet.h).  Validated on the host before the device is touched (ValueError).
    max_gap (0; 1..8: DESIGN.md 7.9): one call of udet_link_detections_gap_ragged (six launches) in its place -- a row without a
    predecessor in the frame before it may continue a track that ended up to max_gap frames earlier, by the same IoU rule against that
    track's last-seen component; the Tracks carries gap_inter, back, prev and open as well, and carry is the TrackHistory that tail()
    of a Tracks with the same k and max_gap returns (its tensors stay as they are: the open flags this call closes are in hist_open)."""
    max_gap = track_max_gap(max_gap)
    if isinstance(selection_or_labels, ComponentSelection):
        if selection_or_labels.labels is None:
            raise ValueError("selected without want_labels: no labels")
        labels, layout = selection_or_labels.labels, selection_or_labels.layout
    else:
        labels, layout = selection_or_labels, detections.layout
    total = int(require_tensor(labels, "labels (packed samples)", torch.int32, 1, cuda=False).numel())
    as_layout(layout, None, total, max_samples=65535)
    for t, name, nd in ((detections.dets, "dets", 3), (detections.counts, "counts", 2)):
        require_tensor(t, "detections." + name, torch.int64, nd, cuda=False)
    host_link, permille = check_link_arguments(layout, detections, link, carry, min_iou, max_gap)
    require_tensor(labels, "labels (packed samples)", torch.int32, 1)
    dev, n, k = labels.device, layout.n, detections.k
    require_tensor(detections.dets, "detections.dets", torch.int64, 3, device=dev)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    if carry is not None:
        for t, name, dt in ((carry.labels, "labels", torch.int32), (carry.dets, "dets", torch.int64), (carry.counts, "counts", torch.int64),
                            (carry.ids, "ids", torch.int32), (carry.next_id, "next_id", torch.int32)) + (
                                ((carry.open, "open", torch.int32),) if max_gap else ()):
            require_tensor(t, "carry." + name, dt, device=dev)
    d_link = link if host_link is None else torch.from_numpy(host_link).to(dev)
    d_off, d_hw = layout.device_tables(dev)
    inter = torch.empty((n, k, k), dtype=torch.int64, device=dev)
    match, ids = (torch.empty((n, k), dtype=torch.int32, device=dev) for _ in range(2))
    linked, seq_tracks = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    next_id = torch.empty(1, dtype=torch.int32, device=dev)
    if max_gap:
        gap_inter = torch.empty((n, max_gap, k, k), dtype=torch.int64, device=dev)
        back, prev, open = (torch.empty((n, k), dtype=torch.int32, device=dev) for _ in range(3))
        m, (ch, cw) = (carry.m, carry.hw) if carry is not None else (0, (0, 0))
        hist_open = None if carry is None else carry.open.clone()  # closed in place by the call: the carry stays what it is
        ws = workspace(lib.udet_link_detections_gap_workspace_bytes(total, n, k, max_gap, m, ch, cw), 4, dev)
        c_lab, c_det, c_cnt, c_ids, c_open, c_next = ([None] * 6 if carry is None else [t.data_ptr() for t in (
            carry.labels, carry.dets, carry.counts, carry.ids, hist_open, carry.next_id)])
        check(lib.udet_link_detections_gap_ragged(labels.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, total,
                                                  detections.dets.data_ptr(), detections.counts.data_ptr(), k, d_link.data_ptr(), max_gap, m,
                                                  c_lab, ch, cw, c_det, c_cnt, c_ids, c_open, c_next, permille, inter.data_ptr(),
                                                  match.data_ptr(), ids.data_ptr(), linked.data_ptr(), seq_tracks.data_ptr(),
                                                  next_id.data_ptr(), gap_inter.data_ptr(), back.data_ptr(), prev.data_ptr(), open.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
        return Tracks(inter, match, ids, linked, seq_tracks, next_id, labels, detections, carry, back, prev, gap_inter, open, max_gap, hist_open)
    ch, cw = carry.hw if carry is not None else (0, 0)
    ws = workspace(lib.udet_link_detections_workspace_bytes(total, n, k, ch, cw), 4, dev)
    c_lab, c_det, c_cnt, c_ids, c_next = ([None] * 5 if carry is None else
                                          [t.data_ptr() for t in (carry.labels, carry.dets, carry.counts, carry.ids, carry.next_id)])
    check(lib.udet_link_detections_ragged(labels.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, total,
                                          detections.dets.data_ptr(), detections.counts.data_ptr(), k, d_link.data_ptr(), c_lab, ch, cw,
                                          c_det, c_cnt, c_ids, c_next, permille, inter.data_ptr(), match.data_ptr(), ids.data_ptr(),
                                          linked.data_ptr(), seq_tracks.data_ptr(), next_id.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    return Tracks(inter, match, ids, linked, seq_tracks, next_id, labels, detections, carry)


def track_records(records, tracks):
    """The per-frame detection records (detection_records' lists, in the frames' order) with their tracks: every record gains "track"
    (its id within its sequence), "prev" (the rank of the row it continues in the frame before, or None) and "iou" (inter / (area_a +
    area_b - inter) of that pair in float64, or None).  tracks: a Tracks (or anything with its host(), detections.dets and carry.dets).  Returns
    new lists; the records given stay as they are.  Linked with gap bridging (tracks.max_gap > 0, host_gaps() and a TrackHistory as
    carry), every record gains "back" as well (1: it continues the frame before, d >= 2: a bridge to frame c - d, 0: a new track),
    "prev" is the rank in frame c - back and the "iou" of a bridged row comes from gap_inter."""
    inter, match, ids, _, _ = tracks.host()
    if len(records) != len(ids):
        raise ValueError("one list of records per frame")
    dets = _host(tracks.detections.dets)
    gaps = getattr(tracks, "max_gap", 0) > 0
    if gaps:
        gap_inter, back, prev_rank, _ = tracks.host_gaps()
        hist = None if tracks.carry is None else _host(tracks.carry.dets)  # [m, k, 9]: frame -1 is its last
    out = []
    for i, recs in enumerate(records):
        if len(recs) > ids.shape[1]:
            raise ValueError("frame {}: more records than rows".format(i))
        before = dets[i - 1] if i else (None if gaps or tracks.carry is None else _host(tracks.carry.dets))
        new = []
        for b, rec in enumerate(recs):
            d, a, prev, more = 1, int(match[i, b]), before, {}
            if gaps:
                d, a = int(back[i, b]), int(prev_rank[i, b])
                prev, more = dets[i - d] if i >= d else hist[len(hist) + i - d], {"back": d}
            iou = None
            if a >= 0:
                it = int(inter[i, a, b] if d == 1 else gap_inter[i, d - 2, a, b])
                iou = float(np.float64(it) / np.float64(int(prev[a, 1]) + int(dets[i, b, 1]) - it))
            new.append(dict(rec, track=int(ids[i, b]), prev=a if a >= 0 else None, iou=iou, **more))
        out.append(new)
    return out


def summarise_tracks(stems, records, starts, gaps=None):
    """The tracks of a category's frames, per sequence: stems (the frames' names), records (track_records' lists) and starts (per frame,
    true where a sequence starts: the category's first frame, and every frame that was not linked) -> a list of sequences in the frames'
    order, each {"first": stem, "frames": count, "tracks": [...]} with one entry per track id, ascending: {"id", "first" / "last" (the
    stems of the first and last frame it appears in), "frames" (in how many), "area_mean", "score_mean" (over those frames, float64)
    and "boxes": {stem: [x0, y0, x1, y1]}}.  gaps (None: true when a record carries "back", the link with gap bridging): every track
    gains "span" (the frames from its first to its last, inclusive) and "gaps" (span - frames), every sequence "bridged" (its records
    with back >= 2)."""
    if not (len(stems) == len(records) == len(starts)):
        raise ValueError("one stem, one list of records and one start flag per frame")
    if gaps is None:
        gaps = any("back" in rec for recs in records for rec in recs)
    out = []
    for i, (stem, recs) in enumerate(zip(stems, records)):
        if i == 0 or starts[i]:
            out.append({"first": stem, "frames": 0, "tracks": {}, "bridged": 0})
        seq = out[-1]
        seq["frames"] += 1
        for rec in recs:
            t = seq["tracks"].setdefault(int(rec["track"]), {"id": int(rec["track"]), "first": stem, "at": i, "area": [], "score": [], "boxes": {}})
            t["last"], t["to"] = stem, i
            t["area"].append(rec["area"])
            t["score"].append(rec["score"])
            t["boxes"][stem] = list(rec["box"])
            seq["bridged"] += int(rec.get("back", 0) >= 2)
    for seq in out:
        seq["tracks"] = [dict({"id": t["id"], "first": t["first"], "last": t["last"], "frames": len(t["area"]),
                               "area_mean": float(np.mean(np.asarray(t["area"], np.float64))),
                               "score_mean": float(np.mean(np.asarray(t["score"], np.float64))), "boxes": t["boxes"]},
                              **({"span": t["to"] - t["at"] + 1, "gaps": t["to"] - t["at"] + 1 - len(t["area"])} if gaps else {}))
                         for _, t in sorted(seq["tracks"].items())]
        if not gaps:
            del seq["bridged"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The dense CRF at native resolution (csrc/crf.hip)
# ---------------------------------------------------------------------------------------------------------------------------
CRF_KEYS = ("sxy", "srgb", "compat", "gauss_k", "iters", "radius")


def check_crf_tables(offsets, hw, numel):
    """Host validation of the device tables of udet_dense_crf_ragged / udet_crf_unary_lookup: ragged.check_packed_tables for packed
    buffers of `numel` elements and at most 65535 samples.  Returns (offsets int64 [n], hw int32 [n,2]) as the kernels read them."""
    return check_packed_tables(offsets, hw, numel, max_samples=CRF_MAX_SAMPLES)


def crf_params(crf):
    """The `crf` dict of restore_results_dir with its defaults filled in (iters 50, radius ceil(3 sxy)) and checked (ValueError)."""
    if not isinstance(crf, dict) or not {"sxy", "srgb", "compat", "gauss_k"} <= set(crf) or not set(crf) <= set(CRF_KEYS):
        raise ValueError("crf must be a dict with sxy, srgb, compat, gauss_k and optionally iters, radius")
    p = {k: float(crf[k]) for k in ("sxy", "srgb", "compat", "gauss_k")}
    p["iters"] = 50 if crf.get("iters") is None else int(crf["iters"])
    p["radius"] = default_radius(p["sxy"]) if crf.get("radius") is None else int(crf["radius"])
    if not (p["sxy"] > 0 and p["srgb"] > 0 and p["gauss_k"] >= 0 and p["iters"] >= 0 and p["radius"] >= 1):
        raise ValueError("crf: sxy, srgb > 0, gauss_k >= 0, iters >= 0 and radius >= 1 are required")
    return p


def load_images_device(paths):
    """The frames of a batch at their own size through data.RaggedLoader (mixed sizes: one pinned buffer, one copy) -> RaggedBatch
    (data: packed rgb bytes on the device, offsets in bytes)."""
    global _ragged_loader
    from . import data
    if _ragged_loader is None:
        _ragged_loader = data.RaggedLoader()
    return _ragged_loader.load(list(paths), 3)


def crf_refine_restored(res, images, crf) -> RestoredMasks:
    """refine (crf_refine.py:110-130) of a restored batch at native size: the unary from the restored bytes
    (post_processing.unary_from_restored), the dense CRF on the frames `images` (a RaggedBatch of rgb frames in the order and of the
    sizes of res -- or anything with its data / offsets / hw; they stay on the device) in one call of post_processing.dense_crf_ragged,
    both on res's own layout.  Returns res with the CRF's labels in the place of the thresholded binary masks."""
    p = crf_params(crf)
    frames = images.layout if hasattr(images, "layout") else PackedLayout(images.offsets, images.hw, images.data.numel(), 3)
    if not frames.same_as(res.layout, scale=3):
        raise ValueError("the frames must be packed like the restored masks (their sizes, three times their offsets)")
    unary = unary_from_restored(res.data, res.layout, None, res.amax, p["gauss_k"])
    _, labels = dense_crf_ragged(unary, images.data, res.layout, None, p["sxy"], p["srgb"], p["compat"], p["iters"], p["radius"],
                                 want_q=False, want_labels=True)
    return RestoredMasks(res.data, labels, res.layout, None, res.amax)


def load_sizes_header(paths):
    """[(H, W), ...] of image files from their headers alone (Pillow opens lazily: nothing is decoded)."""
    from PIL import Image
    sizes = []
    for p in paths:
        with Image.open(p) as im:
            sizes.append((im.size[1], im.size[0]))
    return sizes


def draw_overlays(frames, masks, overlay):
    """visualize.overlay_native(frames, masks, **overlay): the masks of a batch on their frames, one launch."""
    from .visualize import overlay_native
    return overlay_native(frames, masks, **overlay)


def draw_detection_boxes(overlays, detections, boxes):
    """visualize.draw_boxes(overlays, detections, **boxes): the boxes of a batch on its overlays, in place, one launch."""
    from .visualize import draw_boxes
    return draw_boxes(overlays, detections, **boxes)


def draw_track_detection_boxes(overlays, detections, tracks, boxes):
    """visualize.draw_track_boxes(overlays, detections, tracks, thickness=boxes["thickness"]): the boxes of a batch on its overlays, each in
    the colour of its track (visualize.TRACK_PALETTE), in place, one launch."""
    from .visualize import draw_track_boxes
    return draw_track_boxes(overlays, detections, tracks, thickness=boxes["thickness"])


def restore_results_dir(results_dir, frame_lists, out_dir, mask_key="mask", crop=0.9, threshold=0.5, batch=16, restore=restore_masks,
                        gt_rule="DAVIS2016", load_gt=load_gt_device, score=score_device, bound_th=None, skip_ends=True, verbose=True,
                        component=None, connectivity=8, select=select_components, crf=None, load_images=load_images_device,
                        refine=crf_refine_restored, load_sizes=load_sizes_header, overlay=None, draw=draw_overlays, detections=None,
                        detect=component_boxes, draw_boxes=draw_detection_boxes, tracks=None, link=link_detections,
                        draw_track_boxes=draw_track_detection_boxes):
    """Restore, score and export a folder of <category>/result_<k>.mat files (test_generator --generate_visualization,
    post_processing.run_crf, ...) at native resolution.  frame_lists: {category: [(image_path, annotation_path), ...]} in the
    reader's own test order; result_<k>.mat of a category belongs to entry k-1 (the numbering evaluation.evaluate_masks writes; for
    DAVIS that of crf_refine.py:86-88).  A category whose .mat count differs from its list is an IOError.  Per category, `batch`
    masks (mat[mask_key]) at a time are restored to the sizes of their annotations (restore: restore_masks), the annotations
    binarised by gt_rule (a GT_RULES name or a GtRule) at native size, J and F computed per distinct frame shape
    (evaluation.evaluate_batch_davis, disambiguate=False).  Writes <out_dir>/<category>/<frame stem>.png (8-bit, 0 / 255),
    <out_dir>/<category>/result_<k>.mat (mask uint8 0 / 1, soft_mask float32, gt_mask uint8 0 / 1: `davis_eval --results_dir
    <out_dir> --mask_key mask` reads them unchanged) and <out_dir>/native_eval.json; returns the json's content.
    component "largest" / "best_gt" (None: off): the restored binary masks of each batch go through one call of select
    (select_components; "best_gt" together with the batch's annotations), and the selected component is what is scored, written to
    the .png and stored as `mask`; soft_mask and gt_mask stay as they are, and the json gains "component", "connectivity" and per
    sequence "components_mean" (the mean number of components per frame).
    crf (None: off): a dict with sxy, srgb, compat, gauss_k and optionally iters (50), radius (ceil(3 sxy)) -- the full-resolution
    pass of crf_refine.run_crf_original_resolution.  The batch's frames are read at their own size (load_images(paths), in the list's
    order) and refine(restored, frames, crf) (crf_refine_restored: unary from the restored bytes + one dense-CRF call for the batch)
    returns the restored batch with the CRF's labels as its binary masks; they take the place of the thresholded masks for
    everything downstream (component selection, J / F, the .png, `mask`); soft_mask stays the restored soft mask and the json gains
    "crf" with the parameters used.
    Annotation-free mode (a folder of one's own frames, datasets.FrameFolderReader): every annotation of frame_lists is None (a mix
    of None and paths is a ValueError).  The frames' sizes then come from load_sizes(paths) -> [(H, W), ...] (load_sizes_header: the
    image header, no decode); load_gt and score are not called and gt_rule is not looked at; component "best_gt" is a ValueError;
    result_<k>.mat holds mask and soft_mask only; native_eval.json carries "annotations": false, no J / F / IoU key, and per sequence
    frames, foreground_mean (the mean over its frames of |mask| / (H W), from integer counts) and, with a component mode,
    components_mean.
    overlay (None: off): a dict of the parameters of visualize.overlay_native (alpha, beta, colour, edge, edge_colour; {} for the
    defaults).  Every frame's final binary mask -- after the CRF and the component selection -- is drawn on the untouched frame at its
    own size (draw: one call of overlay_native per batch, on the frames the CRF already loaded when it is on) and written to
    <out_dir>/overlay/<category>/<frame stem>.png; the mask folders keep only masks; the json gains "overlay" with the parameters used.
    detections (None: off): a dict with min_area (64) and max_detections (16; at most 64), {} for the defaults.  The batch's binary masks
    -- after the CRF, before the component selection -- are labelled once under `connectivity`: with a component mode by the same select
    call, made with want_labels=True, otherwise by one select call in mode "label"; detect(labelled, score=restored, min_area=...,
    max_detections=...) (component_boxes: four launches per batch) then gives every component of at least min_area pixels as a box, the
    largest first, at most max_detections per frame.  detection_records of each frame go to <out_dir>/detections/<category>.json ({frame
    stem: [record, ...]}, in the list's order); the json gains "detections": {min_area, max_detections, connectivity} and per sequence
    "detections_mean" (the mean number of records per frame).  With and without annotations.  overlay["boxes"] (needs detections; a dict
    with thickness (2; 1..8) and colour ((255, 255, 0)), {} for the defaults): draw_boxes(overlays, detections, boxes) paints the boxes on
    the batch's overlays after the mask (visualize.draw_boxes, one launch), and the json's "overlay" carries "boxes".
    tracks (None: off; needs detections): a dict with min_iou (0.1), {} for the default.  A category's batches are consecutive frames, so
    every batch goes through link(labelled, det, link=[1, ...] with 0 at the category's first frame, carry=the previous batch's
    tail(), min_iou=...) (link_detections: four launches per batch); a frame of another size than the one before it starts a new
    sequence inside its category.  The records of detections/<category>.json gain "track", "prev" and "iou" (track_records),
    <out_dir>/tracks/<category>.json holds summarise_tracks' list, and the json gains "tracks": {min_iou} and per sequence "tracks" (the
    ids handed out) and "track_len_mean" (the mean number of frames of a track).  With overlay["boxes"] the boxes are painted by
    draw_track_boxes(overlays, detections, tracks, boxes) in the colour of their track, in the place of the single-colour call.
    tracks["max_gap"] (0; 1..8: DESIGN.md 7.9) lets a row continue a track that ended up to max_gap frames earlier: link is then called
    with max_gap= as well and the tail() it carries is the history of the last max_gap + 1 frames; the records gain "back", the tracks
    "span" and "gaps", the sequences "bridged", and the json's "tracks" carries max_gap.  With 0 or without the key nothing changes.
    restore / load_gt / score / select / load_images / refine / load_sizes / draw / detect / draw_boxes / link / draw_track_boxes are
    injectable: the host logic runs without a GPU on numpy stand-ins."""
    import json
    import re
    import scipy.io as sio
    from PIL import Image
    from .evaluation import BOUND_TH, _davis_summary, _nanmean, _print_davis_table
    bound_th = BOUND_TH if bound_th is None else bound_th
    batch = max(1, int(batch))
    if component not in (None, "largest", "best_gt"):
        raise ValueError('component must be None, "largest" or "best_gt"')
    if (component is not None or detections is not None) and connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    crf = None if crf is None else crf_params(crf)
    detections = None if detections is None else detection_params(detections)
    if tracks is not None:
        if detections is None:
            raise ValueError("tracks links the detections: it needs detections")
        tracks = track_params(tracks)
    boxes = None
    if overlay is not None:
        from .visualize import box_params, overlay_params
        if isinstance(overlay, dict) and overlay.get("boxes") is not None:
            if detections is None:
                raise ValueError('overlay["boxes"] draws the detections: it needs detections')
            boxes = box_params(overlay["boxes"])
        overlay = overlay_params({k: v for k, v in overlay.items() if k != "boxes"} if isinstance(overlay, dict) else overlay)
    missing = [a is None for entries in frame_lists.values() for _, a in entries]
    free = bool(missing) and all(missing)  # annotation-free: sizes from the frames, nothing to score against
    if any(missing) and not free:
        raise ValueError("frame_lists mixes frames with and without an annotation")
    if free and component == "best_gt":
        raise ValueError('component "best_gt" needs annotations: use "largest" or None')
    if not free:
        rule = GT_RULES[gt_rule] if isinstance(gt_rule, str) else gt_rule
    cat_j, cat_f, cat_nc, cat_fg, cat_nd, cat_nt, cat_tl = {}, {}, {}, {}, {}, {}, {}
    for cat, entries in frame_lists.items():
        d = os.path.join(results_dir, cat)
        ks = sorted(int(m.group(1)) for m in (re.fullmatch(r"result_(\d+)\.mat", f) for f in (os.listdir(d) if os.path.isdir(d) else [])) if m)
        if ks != list(range(1, len(entries) + 1)):
            raise IOError("category {!r}: {} result_<k>.mat under {!r} for {} listed frames".format(cat, len(ks), d, len(entries)))
        od = os.path.join(out_dir, cat)
        os.makedirs(od, exist_ok=True)
        if overlay is not None:
            os.makedirs(os.path.join(out_dir, "overlay", cat), exist_ok=True)
        j, f, nc, fg = np.empty(len(entries)), np.empty(len(entries)), np.zeros(len(entries)), np.zeros(len(entries))
        records = {}  # frame stem -> its detections, in the list's order
        tail, starts = None, []  # tracks: the previous batch's last frame; per frame, whether it starts a sequence
        for s in range(0, len(entries), batch):
            rows = entries[s:s + batch]
            masks = []
            for k in range(s + 1, s + len(rows) + 1):
                mat = sio.loadmat(os.path.join(d, "result_{}.mat".format(k)))
                if mask_key not in mat:
                    raise KeyError("{}: result_{}.mat has no {!r}".format(d, k, mask_key))
                masks.append(np.squeeze(mat[mask_key]).astype(np.float32))
                if masks[-1].ndim != 2 or masks[-1].shape != masks[0].shape:
                    raise ValueError("{}: result_{}.mat: masks must be 2-D and of one shape".format(d, k))
            if free:
                gt = None
                sizes = np.asarray(load_sizes([img for img, _ in rows]), dtype=np.int64).reshape(-1, 2)
                if len(sizes) != len(rows):
                    raise ValueError("load_sizes must return one (H, W) per path")
                res = restore(np.stack(masks), sizes, crop, threshold)
            else:
                gt = load_gt([a for _, a in rows], rule)
                res = restore(np.stack(masks), getattr(gt, "layout", gt.hw), crop, threshold)  # the annotations' layout is the batch's
            pred = res  # what is scored and exported as the binary mask
            frames = load_images([img for img, _ in rows]) if crf is not None or overlay is not None else None  # read once for both
            if crf is not None:
                pred = refine(res, frames, crf)
            labelled = None  # the batch's labels, for the detections: what the CRF left, labelled once
            if component is not None:
                pred = select(pred, gt=gt if component == "best_gt" else None, mode=component, connectivity=connectivity,
                              **({} if detections is None else {"want_labels": True}))
                nc[s:s + len(rows)] = _host(pred.info)[:, 0]
                labelled = pred
            elif detections is not None:
                labelled = select(pred, mode="label", connectivity=connectivity, want_labels=True)
            det = None
            if detections is not None:
                det = detect(labelled, score=res, min_area=detections["min_area"], max_detections=detections["max_detections"])
                recs = detection_records(det, res.amax)
                if tracks is not None:
                    trk = link(labelled, det, link=[0 if s + i == 0 else 1 for i in range(len(rows))], carry=tail, min_iou=tracks["min_iou"],
                               **({"max_gap": tracks["max_gap"]} if "max_gap" in tracks else {}))
                    tail = trk.tail()
                    recs = track_records(recs, trk)
                    starts += [not v for v in trk.host()[3]]
                for (img, _), r in zip(rows, recs):
                    records[os.path.splitext(os.path.basename(img))[0]] = r
            if not free:
                shapes = [tuple(int(v) for v in hw) for hw in gt.hw]
                for shape in sorted(set(shapes)):
                    idx = [i for i, sh in enumerate(shapes) if sh == shape]
                    jj, ff = score(gt.stack(idx), pred.stack(idx), bound_th)
                    j[[s + i for i in idx]], f[[s + i for i in idx]] = jj, ff
            drawn = draw(frames, pred, overlay) if overlay is not None else None
            if boxes is not None:
                drawn = draw_boxes(drawn, det, boxes) if tracks is None else draw_track_boxes(drawn, det, trk, boxes)
            for i, (img, _) in enumerate(rows):
                stem = os.path.splitext(os.path.basename(img))[0]
                binm = _host(pred.binary_sample(i)).astype(np.uint8)
                Image.fromarray(binm * np.uint8(255), "L").save(os.path.join(od, stem + ".png"))
                mat = {"mask": binm, "soft_mask": _host(res.soft(i)).astype(np.float32)}
                if free:
                    fg[s + i] = int(np.count_nonzero(binm)) / int(binm.size)
                else:
                    mat["gt_mask"] = _host(gt.sample(i)).astype(np.uint8)
                sio.savemat(os.path.join(od, "result_{}.mat".format(s + i + 1)), mat)
                if drawn is not None:
                    Image.fromarray(np.ascontiguousarray(_host(drawn.sample(i)), dtype=np.uint8), "RGB").save(
                        os.path.join(out_dir, "overlay", cat, stem + ".png"))
        cat_j[cat], cat_f[cat], cat_nc[cat] = j.tolist(), f.tolist(), float(nc.mean()) if len(nc) else 0.0
        cat_fg[cat] = float(fg.mean()) if len(fg) else 0.0
        if detections is not None:
            os.makedirs(os.path.join(out_dir, "detections"), exist_ok=True)
            with open(os.path.join(out_dir, "detections", cat + ".json"), "w") as fh:
                json.dump(records, fh, indent=1)
            cat_nd[cat] = float(np.mean([len(r) for r in records.values()])) if records else 0.0
        if tracks is not None:
            summary = summarise_tracks(list(records), list(records.values()), starts, gaps=True if "max_gap" in tracks else None)
            os.makedirs(os.path.join(out_dir, "tracks"), exist_ok=True)
            with open(os.path.join(out_dir, "tracks", cat + ".json"), "w") as fh:
                json.dump(summary, fh, indent=1)
            lengths = [t["frames"] for seq in summary for t in seq["tracks"]]
            cat_nt[cat], cat_tl[cat] = len(lengths), float(np.mean(lengths)) if lengths else 0.0
    if not cat_j:
        raise IOError("no category to restore")
    if free:
        out = {"mask_key": mask_key, "threshold": threshold, "crop": crop, "annotations": False,
               "sequences": {c: {"frames": len(cat_j[c]), "foreground_mean": cat_fg[c]} for c in cat_j}}
        if component is not None:
            out["component"], out["connectivity"] = component, int(connectivity)
            for c in out["sequences"]:
                out["sequences"][c]["components_mean"] = cat_nc[c]
        if crf is not None:
            out["crf"] = crf
        if overlay is not None:
            out["overlay"] = overlay if boxes is None else dict(overlay, boxes=boxes)
        if detections is not None:
            out["detections"] = dict(detections, connectivity=int(connectivity))
            for c in out["sequences"]:
                out["sequences"][c]["detections_mean"] = cat_nd[c]
        if tracks is not None:
            out["tracks"] = tracks
            for c in out["sequences"]:
                out["sequences"][c]["tracks"], out["sequences"][c]["track_len_mean"] = cat_nt[c], cat_tl[c]
        if verbose:
            print("Native resolution ({} frames, crop {}, no annotations):".format(sum(len(v) for v in cat_j.values()), crop))
            for c, v in out["sequences"].items():
                print("  {:<24s} {:5d} frames   foreground {:.4f}".format(c, v["frames"], v["foreground_mean"]))
        with open(os.path.join(out_dir, "native_eval.json"), "w") as fh:
            json.dump(out, fh, indent=1)
        return out
    per, tot = _davis_summary(cat_j, cat_f, skip_ends)
    cat_iou = {c: _nanmean(cat_j[c]) for c in cat_j}
    out = {"mask_key": mask_key, "threshold": threshold, "crop": crop, "bound_th": bound_th, "skip_ends": bool(skip_ends),
           "sequences": {c: dict(per[c], frames=len(cat_j[c])) for c in per}, "J": tot["J"], "F": tot["F"], "J&F": tot["J&F"],
           "category_iou": cat_iou, "sequence_iou": _nanmean(list(cat_iou.values()))}
    if component is not None:
        out["component"], out["connectivity"] = component, int(connectivity)
        for c in out["sequences"]:
            out["sequences"][c]["components_mean"] = cat_nc[c]
    if crf is not None:
        out["crf"] = crf
    if overlay is not None:
        out["overlay"] = overlay if boxes is None else dict(overlay, boxes=boxes)
    if detections is not None:
        out["detections"] = dict(detections, connectivity=int(connectivity))
        for c in out["sequences"]:
            out["sequences"][c]["detections_mean"] = cat_nd[c]
    if tracks is not None:
        out["tracks"] = tracks
        for c in out["sequences"]:
            out["sequences"][c]["tracks"], out["sequences"][c]["track_len_mean"] = cat_nt[c], cat_tl[c]
    if verbose:
        print("Native resolution ({} frames, crop {}):".format(sum(len(v) for v in cat_j.values()), crop))
        _print_davis_table(per, tot)
    with open(os.path.join(out_dir, "native_eval.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    return out


def frame_lists_from_reader(flags):
    """{category: [(image_path, annotation_path), ...]} of the test pass of --dataset under --root_dir, in the order the reader's
    test_inputs visits a category's frames; categories named as evaluate_masks names them (fname.split("/")[-2])."""
    from .cli import _reader
    rd = _reader(flags, 0, 1)
    if flags.dataset == "FRAMES":  # no annotations: (image, None)
        return {str(seq[0]).split("/")[-2]: [(str(i), None) for i in seq] for seq in rd.get_filenames_list()[0]}
    if flags.dataset == "FBMS":
        pairs = [(t[0], t[2]) for t in rd.get_test_tuples(flags.test_partition, flags.test_temporal_shift)]
    else:
        imgs, anns = rd.get_filenames_list() if flags.dataset == "SEGTRACK" else rd.get_filenames_list(flags.test_partition)
        pairs = [(i, a) for seq_i, seq_a in zip(imgs, anns) for i, a in zip(seq_i, seq_a)]
    lists = {}
    for img, ann in pairs:
        lists.setdefault(str(img).split("/")[-2], []).append((str(img), str(ann)))
    return lists
