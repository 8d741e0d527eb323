"""Flow / mask visualisation and training summaries, computed on the device (csrc/visualize.hip):

  flow_to_image(flow, mask=None, threshold=0.1)    models/utils/flow_utils.py:46-100 (+ the masked flow image of
                                                   models/adversarial_learner.py:269-272 when `mask` is given)
  overlay_mask(image, mask, out_hw=(384, 640))     test_generator.py:101-107 (postprocess_image / postprocess_mask, cv2.addWeighted,
                                                   cv2.resize)
  overlay_native(images, masks, ...)               the same blend at every frame's own size for a ragged batch, without the resize, plus
                                                   the mask's contour: what native_results writes with overlay=...
  grad_histograms(g, net) / bucket_limits()        tf.summary.histogram of every variable's gradient (adversarial_learner.py:284-289)
  postprocess_image / postprocess_mask             models/utils/general_utils.py:23-51 on host arrays (RGB order is kept)
  SummaryWriter(dir)                               the step_sum summaries of collect_summaries (:260-291) as plain files:
      scalars.jsonl                                one JSON object per call: {"step": s, <the eight losses{}>}
      images/step_%08d_<tag>.png                   input_image, next_image, PWC_Flow, masked_flow, Rec_flow, Rec_flow_compl
      histograms/step_%08d_<net>.npz               names [V], stats [V,5] = (min, max, count, sum, sum of squares), counts [V,1551],
                                                   limits [1551]
There is no TensorBoard event-file writer: the JSON-lines / PNG / npz layout is the interface.

The device functions take and return device tensors and do not synchronise; the images and bucket counts come from the kernels of
libudet.so (no PyTorch fallback), torch only holds the memory."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import evaluation as _ev  # (declares udet_mask_stats)
from . import weights as W
from ._ffi import check, lib
from .ragged import PackedLayout, PackedSamples, as_layout, require_tensor

N_BUCKETS = 1551  # UDET_HISTOGRAM_BUCKETS
DES_HW = (384, 640)  # test_generator.py:14-15


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t, name, last):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4
            and t.shape[-1] == last):
        raise ValueError("%s must be a contiguous float32 CUDA(HIP) tensor [N,H,W,%d]" % (name, last))
    return t


def _mask_stats_device(mask, threshold):
    """udet_mask_stats of `mask` against an empty annotation, left on the device: [N,8] float64 (column 0 is the border sum)."""
    n, h, w, _ = mask.shape
    st = torch.empty((n, 8), dtype=torch.float64, device=mask.device)
    check(lib.udet_mask_stats(mask.data_ptr(), torch.zeros_like(mask).data_ptr(), n, h, w, threshold, 0.0, st.data_ptr(), _stream()))
    return st


def flow_to_image(flow: torch.Tensor, mask: torch.Tensor = None, threshold: float = 0.1) -> torch.Tensor:
    """Colour-wheel image of a flow batch [N,H,W,2] -> uint8 device tensor [N,H,W,3] (flow_to_image of the reference: sample i is
    normalised by the largest radius of samples 0..i).  With `mask` [N,H,W,1] the pixels of the disambiguated object mask
    (mask > threshold, complemented per sample when it hugs the image border) are painted (127,127,127): the reference's
    "masked_flow" summary.  The border statistics go from udet_mask_stats to the colouring kernel on the device."""
    _f32(flow, "flow", 2)
    n, h, w, _ = flow.shape
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=flow.device)
    ws = torch.empty(int(lib.udet_flow_to_image_workspace_bytes(n)), dtype=torch.uint8, device=flow.device)
    mp = sp = None
    if mask is not None:
        _f32(mask, "mask", 1)
        if tuple(mask.shape[:3]) != (n, h, w):
            raise ValueError("mask must be [N,H,W,1] like the flow")
        st = _mask_stats_device(mask, threshold)
        mp, sp = mask.data_ptr(), st.data_ptr()
    check(lib.udet_flow_to_image(flow.data_ptr(), mp, sp, threshold, n, h, w, rgb.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return rgb


def overlay_mask(image: torch.Tensor, mask: torch.Tensor, out_hw=DES_HW, threshold: float = 0.1) -> torch.Tensor:
    """The frame the reference's test script saves (test_generator.py:101-107): image [N,H,W,3] in [-0.5,0.5] un-normalised to 8 bit,
    blended 0.5 / 0.4 with the disambiguated mask [N,H,W,1] in the green channel, resized to out_hw with OpenCV's 8-bit bilinear
    rule -> uint8 device tensor [N,oh,ow,3], RGB."""
    _f32(image, "image", 3)
    _f32(mask, "mask", 1)
    n, h, w, _ = image.shape
    if tuple(mask.shape[:3]) != (n, h, w):
        raise ValueError("mask must be [N,H,W,1] like the image")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    st = _mask_stats_device(mask, threshold)
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=image.device)
    check(lib.udet_overlay_mask(image.data_ptr(), mask.data_ptr(), st.data_ptr(), threshold, n, h, w, out.data_ptr(), oh, ow, _stream()))
    return out


# ------------------------------------------------------------------------------------------- overlays at native size ----
OVERLAY_MAX_EDGE = 8  # UDET_OVERLAY_MAX_EDGE
OVERLAY_DEFAULTS = {"alpha": 0.5, "beta": 0.4, "colour": (0, 255, 0), "edge": 2, "edge_colour": (255, 255, 255)}


def _rgb24(colour, name):
    c = [int(v) for v in colour]
    if len(c) != 3 or min(c) < 0 or max(c) > 255 or any(int(v) != v for v in colour):
        raise ValueError("{} must be three integers in 0..255 (r, g, b)".format(name))
    return (c[0] << 16) | (c[1] << 8) | c[2]


def overlay_params(overlay=None):
    """The parameters of overlay_native (a dict, or None for the defaults) with the defaults filled in and checked (ValueError):
    alpha, beta finite and >= 0, edge an integer in 0..OVERLAY_MAX_EDGE, colour / edge_colour three integers in 0..255."""
    p = dict(OVERLAY_DEFAULTS)
    if overlay is not None:
        if not isinstance(overlay, dict) or not set(overlay) <= set(OVERLAY_DEFAULTS):
            raise ValueError("overlay must be a dict with keys among {}".format(sorted(OVERLAY_DEFAULTS)))
        p.update({k: v for k, v in overlay.items() if v is not None})
    p["alpha"], p["beta"] = float(p["alpha"]), float(p["beta"])
    if not (0.0 <= p["alpha"] < float("inf") and 0.0 <= p["beta"] < float("inf")):
        raise ValueError("overlay: alpha and beta must be finite and >= 0")
    if int(p["edge"]) != p["edge"] or not 0 <= int(p["edge"]) <= OVERLAY_MAX_EDGE:
        raise ValueError("overlay: edge must be an integer in 0..{}".format(OVERLAY_MAX_EDGE))
    p["edge"] = int(p["edge"])
    p["colour"], p["edge_colour"] = tuple(int(v) for v in p["colour"]), tuple(int(v) for v in p["edge_colour"])
    _rgb24(p["colour"], "colour"), _rgb24(p["edge_colour"], "edge_colour")
    return p


class NativeOverlays(PackedSamples):
    """Result of overlay_native: data (packed uint8 rgb, device) in the frames' own layout (three bytes per pixel)."""

    def __init__(self, data, layout):
        PackedSamples.__init__(self, layout, data.device)
        self.data = data

    def sample(self, i):
        """[H_i, W_i, 3] uint8 view of sample i."""
        return self._view(self.data, i)


def overlay_native(images, masks, alpha=0.5, beta=0.4, colour=(0, 255, 0), edge=2, edge_colour=(255, 255, 255), out=None) -> NativeOverlays:
    """Every mask of a ragged batch drawn on its own frame at the frame's own size, in one call of udet_overlay_native_ragged (one
    launch whatever the batch): cv2.addWeighted(frame, alpha, mask painted `colour`, beta) -- with the defaults the picture of
    test_generator.py:101-106 without its resize -- and, for edge >= 1, the mask's contour (the foreground pixels with a background pixel
    of the frame within `edge` columns and rows) in edge_colour, unblended.  images: a RaggedBatch of rgb frames (or anything with its
    data / offsets / hw); masks: anything that holds packed 0 / non-0 bytes of the same sizes in the same order at a third of the frames'
    offsets -- a RestoredMasks (its binary masks), a ComponentSelection (its selected component), a GtBatch (its data).  out: a
    caller-owned uint8 buffer of the frames' bytes that does not overlap the inputs (bytes between the samples stay as they are);
    default: a fresh zeroed one.  Everything is validated on the host before the device is touched (ValueError)."""
    p = overlay_params({"alpha": alpha, "beta": beta, "colour": colour, "edge": edge, "edge_colour": edge_colour})
    frames = images.layout if hasattr(images, "layout") else PackedLayout(images.offsets, images.hw, images.data.numel(), 3, overlap_ok=True)
    buf = next((b for b in (getattr(masks, k, None) for k in ("binary", "selected", "data")) if b is not None), None)
    if buf is None:
        raise ValueError("masks holds no packed binary buffer (binary, selected or data)")
    total = int(require_tensor(buf, "masks (packed samples)", torch.uint8, 1, cuda=False).numel())
    layout = masks.layout if hasattr(masks, "layout") else as_layout(masks.offsets, masks.hw, total)
    if frames.c != 3 or not frames.same_as(layout, scale=3):
        raise ValueError("the frames must be rgb and packed like the masks (their sizes, three times their offsets)")
    as_layout(layout, None, total, max_samples=65535)
    dev = buf.device
    require_tensor(buf, "masks (packed samples)", torch.uint8, 1)
    require_tensor(images.data, "images (rgb, packed like the masks)", torch.uint8, 1, 3 * total, dev)
    if out is None:
        out = torch.zeros(3 * total, dtype=torch.uint8, device=dev)
    else:
        require_tensor(out, "out", torch.uint8, 1, 3 * total, dev)
        for t in (images.data, buf):
            if out.data_ptr() < t.data_ptr() + t.numel() and t.data_ptr() < out.data_ptr() + out.numel():
                raise ValueError("out must not overlap the frames or the masks")
    d_off, d_hw = layout.device_tables(dev)
    check(lib.udet_overlay_native_ragged(images.data.data_ptr(), buf.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h,
                                         layout.max_w, total, p["alpha"], p["beta"], _rgb24(p["colour"], "colour"), p["edge"],
                                         _rgb24(p["edge_colour"], "edge_colour"), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return NativeOverlays(out, frames)


DRAW_MAX_THICKNESS = 8  # UDET_DRAW_MAX_THICKNESS
BOX_DEFAULTS = {"thickness": 2, "colour": (255, 255, 0)}


def box_params(boxes=None):
    """The parameters of draw_boxes (a dict, or None for the defaults) with the defaults filled in and checked (ValueError): thickness an
    integer in 1..DRAW_MAX_THICKNESS, colour three integers in 0..255."""
    p = dict(BOX_DEFAULTS)
    if boxes is not None:
        if not isinstance(boxes, dict) or not set(boxes) <= set(BOX_DEFAULTS):
            raise ValueError("boxes must be a dict with keys among {}".format(sorted(BOX_DEFAULTS)))
        p.update({k: v for k, v in boxes.items() if v is not None})
    if isinstance(p["thickness"], bool) or int(p["thickness"]) != p["thickness"] or not 1 <= int(p["thickness"]) <= DRAW_MAX_THICKNESS:
        raise ValueError("boxes: thickness must be an integer in 1..{}".format(DRAW_MAX_THICKNESS))
    _rgb24(p["colour"], "colour")
    p["thickness"], p["colour"] = int(p["thickness"]), tuple(int(v) for v in p["colour"])
    return p


def draw_boxes(overlays, detections, thickness=2, colour=(255, 255, 0)) -> NativeOverlays:
    """The frames of a batch's detections painted on its overlays, in place, in one call of udet_draw_boxes_ragged (one launch; dets
    and counts are read on the device).  overlays: a NativeOverlays (or anything with packed rgb `data` and its `layout`: a RaggedBatch of
    frames); detections: the native_results.Detections of the same frames (their sizes in the same order at a third of the overlays'
    offsets).  A pixel of a box [y0, y1) x [x0, x1) is painted `colour` when it lies within `thickness` (1..8) rows or columns of the
    box's edge, inward; a box narrower than twice the thickness is filled; every other byte stays.  Returns overlays.  Validated on the
    host before the device is touched (ValueError)."""
    p = box_params({"thickness": thickness, "colour": colour})
    frames, layout = overlays.layout, detections.layout
    if frames.c != 3 or not frames.same_as(layout, scale=3):
        raise ValueError("the overlays must be rgb and packed like the detections' frames (their sizes, three times their offsets)")
    as_layout(layout, None, layout.numel, max_samples=65535)
    for t, name, shape in ((detections.dets, "dets", (layout.n, detections.k, 9)), (detections.counts, "counts", (layout.n, 3))):
        require_tensor(t, "detections." + name, torch.int64, len(shape), cuda=False)
        if tuple(t.shape) != shape:
            raise ValueError("detections.{} must be {} for {} frames".format(name, list(shape), layout.n))
    dev = detections.dets.device
    require_tensor(detections.dets, "detections.dets", torch.int64, 3)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    require_tensor(overlays.data, "overlays (rgb, packed like the detections' frames)", torch.uint8, 1, 3 * layout.numel, dev)
    d_off, d_hw = layout.device_tables(dev)
    check(lib.udet_draw_boxes_ragged(overlays.data.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.numel,
                                     detections.dets.data_ptr(), detections.counts.data_ptr(), detections.k, p["thickness"],
                                     _rgb24(p["colour"], "colour"), torch.cuda.current_stream(dev).cuda_stream))
    return overlays


TRACK_MAX_PALETTE = 64  # UDET_TRACK_MAX_PALETTE
# twelve distinct colours (the qualitative "Paired" scheme of ColorBrewer): track id t is drawn in TRACK_PALETTE[t mod 12]
TRACK_PALETTE = [(166, 206, 227), (31, 120, 180), (178, 223, 138), (51, 160, 44), (251, 154, 153), (227, 26, 28),
                 (253, 191, 111), (255, 127, 0), (202, 178, 214), (106, 61, 154), (255, 255, 153), (177, 89, 40)]


def palette_words(palette):
    """A palette -- 1..TRACK_MAX_PALETTE colours of three integers in 0..255 -- as a tuple of 0xRRGGBB words (ValueError otherwise)."""
    try:
        colours = [tuple(c) for c in palette]
    except TypeError:
        raise ValueError("palette must be a list of (r, g, b) colours")
    if not 1 <= len(colours) <= TRACK_MAX_PALETTE:
        raise ValueError("palette must hold 1..{} colours".format(TRACK_MAX_PALETTE))
    return tuple(_rgb24(c, "palette colour") for c in colours)


def draw_track_boxes(overlays, detections, tracks, thickness=2, palette=TRACK_PALETTE) -> NativeOverlays:
    """The boxes of a batch's detections painted on its overlays in the colour of their track, in place, in one call of
    udet_draw_track_boxes_ragged (one launch; dets, counts and ids are read on the device).  overlays / detections / thickness: as for
    draw_boxes; tracks: the native_results.Tracks of those detections.  Row r of frame i is painted palette[ids[i][r] mod len(palette)]
    (palette: 1..64 colours, TRACK_PALETTE's twelve by default); a row without an id (-1) is not painted; where the lines of several
    boxes cover a pixel, the box of the smallest rank wins.  Returns overlays.  Validated on the host before the device is touched
    (ValueError)."""
    p = box_params({"thickness": thickness})
    words = palette_words(palette)
    frames, layout = overlays.layout, detections.layout
    if frames.c != 3 or not frames.same_as(layout, scale=3):
        raise ValueError("the overlays must be rgb and packed like the detections' frames (their sizes, three times their offsets)")
    as_layout(layout, None, layout.numel, max_samples=65535)
    for t, name, dt, shape in ((detections.dets, "detections.dets", torch.int64, (layout.n, detections.k, 9)),
                               (detections.counts, "detections.counts", torch.int64, (layout.n, 3)),
                               (tracks.ids, "tracks.ids", torch.int32, (layout.n, detections.k))):
        require_tensor(t, name, dt, len(shape), cuda=False)
        if tuple(t.shape) != shape:
            raise ValueError("{} must be {} for {} frames".format(name, list(shape), layout.n))
    dev = detections.dets.device
    require_tensor(detections.dets, "detections.dets", torch.int64, 3)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    require_tensor(tracks.ids, "tracks.ids", torch.int32, 2, device=dev)
    require_tensor(overlays.data, "overlays (rgb, packed like the detections' frames)", torch.uint8, 1, 3 * layout.numel, dev)
    d_pal = torch.tensor(words, dtype=torch.int32, device=dev)
    d_off, d_hw = layout.device_tables(dev)
    check(lib.udet_draw_track_boxes_ragged(overlays.data.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.numel,
                                           detections.dets.data_ptr(), detections.counts.data_ptr(), detections.k, tracks.ids.data_ptr(),
                                           p["thickness"], d_pal.data_ptr(), len(words), torch.cuda.current_stream(dev).cuda_stream))
    return overlays


def overlay_instances(images, maps, alpha=0.5, beta=0.4, edge=2, palette=TRACK_PALETTE, other_colour=(128, 128, 128), out=None) -> NativeOverlays:
    """The instance maps of a ragged batch drawn on their frames at the frames' own size, in one call of udet_overlay_instances_ragged
    (one launch whatever the batch): overlay_native's blend with a colour per pixel -- value v in 1..252 in palette[(v - 1) mod
    len(palette)] (so a track's pixels take the colour draw_track_boxes gives its box), 253..255 in other_colour, 0 the frame alone --
    and, for edge >= 1, a contour in the pixel's own colour, unblended, wherever another value lies within `edge` columns and rows
    inside the frame: two touching instances are separated by a line of each one's colour.  images: as for overlay_native; maps: a
    native_results.InstanceMaps (or anything that holds the packed bytes as `map` or `data` with their `layout`).  out: as for
    overlay_native.  Everything is validated on the host before the device is touched (ValueError)."""
    p = overlay_params({"alpha": alpha, "beta": beta, "edge": edge})
    words, other = palette_words(palette), _rgb24(other_colour, "other_colour")
    frames = images.layout if hasattr(images, "layout") else PackedLayout(images.offsets, images.hw, images.data.numel(), 3, overlap_ok=True)
    buf = next((b for b in (getattr(maps, k, None) for k in ("map", "data")) if b is not None), None)
    if buf is None:
        raise ValueError("maps holds no packed instance map (map or data)")
    total = int(require_tensor(buf, "maps (packed samples)", torch.uint8, 1, cuda=False).numel())
    layout = maps.layout if hasattr(maps, "layout") else as_layout(maps.offsets, maps.hw, total)
    if frames.c != 3 or not frames.same_as(layout, scale=3):
        raise ValueError("the frames must be rgb and packed like the maps (their sizes, three times their offsets)")
    as_layout(layout, None, total, max_samples=65535)
    dev = buf.device
    require_tensor(buf, "maps (packed samples)", torch.uint8, 1)
    require_tensor(images.data, "images (rgb, packed like the maps)", torch.uint8, 1, 3 * total, dev)
    if out is None:
        out = torch.zeros(3 * total, dtype=torch.uint8, device=dev)
    else:
        require_tensor(out, "out", torch.uint8, 1, 3 * total, dev)
        for t in (images.data, buf):
            if out.data_ptr() < t.data_ptr() + t.numel() and t.data_ptr() < out.data_ptr() + out.numel():
                raise ValueError("out must not overlap the frames or the maps")
    d_pal = torch.tensor(words, dtype=torch.int32, device=dev)
    d_off, d_hw = layout.device_tables(dev)
    check(lib.udet_overlay_instances_ragged(images.data.data_ptr(), buf.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h,
                                            layout.max_w, total, p["alpha"], p["beta"], d_pal.data_ptr(), len(words), other, p["edge"],
                                            out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return NativeOverlays(out, frames)


# ------------------------------------------------------------------------------------------------------- histograms ----
def bucket_limits() -> np.ndarray:
    """TensorFlow's default histogram bucket limits, as the library builds them: 1551 ascending float64."""
    out = np.empty(N_BUCKETS, np.float64)
    check(lib.udet_histogram_limits(out.ctypes.data, N_BUCKETS))
    return out


def segment_histograms(g: torch.Tensor, seg_offsets):
    """udet_grad_histogram over the segments [seg_offsets[s], seg_offsets[s+1]) of the flat float32 device buffer g.  Returns host
    arrays (stats [S,5] float64 = min, max, count, sum, sum of squares; counts [S,1551] uint32), fetched in ONE device-to-host copy.
    seg_offsets: a sequence of S+1 integers or a device int64 tensor made by `device_offsets` (then it is not validated again)."""
    if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 1):
        raise ValueError("g must be a flat contiguous float32 CUDA(HIP) tensor")
    off = seg_offsets if isinstance(seg_offsets, torch.Tensor) else device_offsets(seg_offsets, g.numel(), g.device)
    nseg = off.numel() - 1
    nstat = nseg * 5 * 8
    out = torch.empty(nstat + nseg * N_BUCKETS * 4, dtype=torch.uint8, device=g.device)  # stats, then counts: one copy
    ws = torch.empty(int(lib.udet_grad_histogram_workspace_bytes(nseg)), dtype=torch.uint8, device=g.device)
    check(lib.udet_grad_histogram(g.data_ptr(), off.data_ptr(), nseg, out.data_ptr(), out.data_ptr() + nstat, ws.data_ptr(),
                                  ws.numel(), _stream()))
    host = out.cpu().numpy()
    return host[:nstat].view(np.float64).reshape(nseg, 5), host[nstat:].view(np.uint32).reshape(nseg, N_BUCKETS)


def device_offsets(seg_offsets, total, device="cuda") -> torch.Tensor:
    """Validated segment table on the device: S+1 offsets, non-decreasing pairwise ranges inside [0, total]."""
    off = np.asarray(seg_offsets, dtype=np.int64).reshape(-1)
    if off.size < 2 or off.min() < 0 or off.max() > total or np.any(off[1:] < off[:-1]):
        raise ValueError("seg_offsets must be S+1 non-decreasing offsets inside the buffer")
    return torch.from_numpy(off).to(device)


_net_tables = {}


def _net_table(net, device):
    """(variable names, device offsets) of a network's flat buffer: variables are contiguous in TF creation order."""
    key = (net, str(device))
    if key not in _net_tables:
        tab = W.param_table(net)
        offs = [o for _, _, o in tab] + [W.param_total(net)]
        _net_tables[key] = ([n for n, _, _ in tab], device_offsets(offs, W.param_total(net), device))
    return _net_tables[key]


def grad_histograms(g: torch.Tensor, net: int):
    """{variable name: (stats [5], counts [1551])} of a network's flat gradient buffer (weights.param_table(net) gives the segments)."""
    if g.numel() != W.param_total(net):
        raise ValueError("g has %d elements, network %d has %d" % (g.numel(), net, W.param_total(net)))
    names, off = _net_table(net, g.device)
    stats, counts = segment_histograms(g, off)
    return {n: (stats[i], counts[i]) for i, n in enumerate(names)}


# ------------------------------------------------------------------------------------------------ host post-processing ----
def postprocess_image(image) -> np.ndarray:
    """general_utils.py:23-35: [H,W,3] in [-0.5,0.5] -> uint8.  RGB order is kept (the reference converts to BGR for cv2.imwrite)."""
    return np.asarray(np.clip((np.asarray(image, np.float32) + np.float32(0.5)) * np.float32(255), 0, 255), np.uint8)


def postprocess_mask(mask) -> np.ndarray:
    """general_utils.py:37-51: [H,W,1] mask in [0,1] (or boolean) -> uint8 [H,W,3] with the mask in the middle channel."""
    un = np.asarray(np.asarray(mask, np.float64) * 255.0, np.uint8)
    tile = np.zeros_like(un, dtype=np.uint8)
    return np.concatenate((tile, un, tile), axis=-1)


# -------------------------------------------------------------------------------------------------------------- writer ----
class SummaryWriter(object):
    """Plain-file summaries under `dir` (layout in the module docstring).  Takes host arrays; nothing here touches the device."""

    def __init__(self, dir):
        self.dir = dir
        os.makedirs(os.path.join(dir, "images"), exist_ok=True)
        os.makedirs(os.path.join(dir, "histograms"), exist_ok=True)

    def add_scalars(self, step, losses):
        rec = {"step": int(step)}
        rec.update({k: float(v) for k, v in losses.items()})
        with open(os.path.join(self.dir, "scalars.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")

    def add_image(self, step, tag, image_u8):
        from PIL import Image
        a = np.ascontiguousarray(image_u8)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image must be uint8 [H,W,3]")
        path = os.path.join(self.dir, "images", "step_%08d_%s.png" % (step, tag))
        Image.fromarray(a).save(path)
        return path

    def add_histograms(self, step, net_name, names, stats, counts):
        path = os.path.join(self.dir, "histograms", "step_%08d_%s.npz" % (step, net_name))
        np.savez_compressed(path, names=np.asarray(list(names)), stats=np.asarray(stats, np.float64),
                            counts=np.asarray(counts, np.uint32), limits=bucket_limits())
        return path


IMAGE_TAGS = ("input_image", "next_image", "PWC_Flow", "masked_flow", "Rec_flow", "Rec_flow_compl")


def write_training_summary(writer: SummaryWriter, step, engine, state, which, img2, losses=None):
    """One summary step of AdversarialLearner.train: the eight losses, the six images of collect_summaries for sample 0
    (max_outputs=1) and the gradient histograms of the network this step trained, read from its flat gradient buffer after
    udet_apply (which left the clipped gradient -- what the reference logs -- there).

    The reference evaluates BOTH networks' gradients at a summary step; that would need a second backward pass, so only the
    trained network's histograms are written here.  Everything is enqueued on the caller's stream behind the step and only reads
    plan buffers that stay untouched until the next step consumes its prefetch; two device-to-host copies are added."""
    from . import data as _data
    from .engine import GEN
    e = engine
    B = e.cfg.batch_size
    image, flow, mask, pred = (e.buffer(k) for k in ("image", "flow", "mask", "pred"))
    h, w = image.shape[1], image.shape[2]
    to_u8 = lambda x: ((x + 0.5) * 255.0).clamp_(0.0, 255.0).to(torch.uint8)  # postprocess_image
    nxt = _data.crop_flip_resize(img2[:1].contiguous(), h, w, None, False)  # the graph's resize of image_2_batch (:87-90)
    flows = torch.cat([flow[:1], pred[:1], pred[B:B + 1]], 0).contiguous()
    # each flow image is a call of its own in the reference: every one is normalised by its own maximum
    pics = torch.cat([to_u8(image[:1]), to_u8(nxt), flow_to_image(flows[0:1]), flow_to_image(flows[0:1], mask[:1].contiguous()),
                      flow_to_image(flows[1:2]), flow_to_image(flows[2:3])], 0).cpu().numpy()  # copy 1
    net = W.NET_GEN if which & GEN else W.NET_REC
    g = state.g_gen if which & GEN else state.g_rec
    names, off = _net_table(net, g.device)
    stats, counts = segment_histograms(g, off)  # copy 2
    writer.add_scalars(step, losses if losses is not None else e.losses())
    for tag, pic in zip(IMAGE_TAGS, pics):
        writer.add_image(step, tag, pic)
    writer.add_histograms(step, "generator" if net == W.NET_GEN else "recover", names, stats, counts)
