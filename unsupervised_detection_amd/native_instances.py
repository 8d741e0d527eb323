"""Native-resolution stage, step 5: what the link knows, handed to the pixels -- per frame an instance map in which every pixel names
its track, and per track its overlap with the annotation (csrc/instances.hip).

  instance_maps(selection_or_labels, detections, tracks, gt)   one call of udet_track_instance_maps_ragged -> InstanceMaps: the byte
                                                maps (0 background, 1 + id mod 252 a track, 255 foreground without a track), row_gt and
                                                frame_stats
  check_instance_arguments                      its host validation (no GPU needed)
  instance_params                               the `instances` dict of native_results.restore_results_dir, filled in and checked
  INSTANCE_PALETTE_BYTES                        the palette of the indexed PNGs: a track's colour is its boxes' (visualize.TRACK_PALETTE)
  track_gt_scores(records, row_gt, gt_area, starts)   per sequence and track the mean J against the annotation, from the integers"""
import numpy as np
import torch

from ._ffi import check, lib
from .native_components import ComponentSelection, packed_labels
from .native_detections import DET_FIELDS, DET_MAX_K, _host
from .ragged import PackedSamples, as_layout, require_tensor, workspace

INSTANCE_WRAP = 252        # UDET_INSTANCE_WRAP: a multiple of the palette's twelve colours
INSTANCE_UNASSIGNED = 255  # UDET_INSTANCE_UNASSIGNED
INSTANCE_DEFAULTS = {"overlay": False}


def _palette_bytes():
    from .visualize import TRACK_PALETTE
    pal = [(0, 0, 0)] * 256
    for j in range(INSTANCE_WRAP):
        pal[1 + j] = tuple(TRACK_PALETTE[j % len(TRACK_PALETTE)])
    pal[INSTANCE_UNASSIGNED] = (128, 128, 128)
    return bytes(v for c in pal for v in c)


# 768 bytes: index 0 black, 1 + j the colour of track j (j < 252), 253 / 254 black, 255 grey
INSTANCE_PALETTE_BYTES = _palette_bytes()


def instance_params(instances=None):
    """The `instances` dict of restore_results_dir ({} or None: the defaults) with the defaults filled in and checked (ValueError):
    overlay a bool."""
    p = dict(INSTANCE_DEFAULTS)
    if instances is not None:
        if not isinstance(instances, dict) or not set(instances) <= set(INSTANCE_DEFAULTS):
            raise ValueError("instances must be a dict with keys among {}".format(sorted(INSTANCE_DEFAULTS)))
        p.update({k: v for k, v in instances.items() if v is not None})
    if not isinstance(p["overlay"], (bool, np.bool_)):
        raise ValueError("instances: overlay must be a bool")
    p["overlay"] = bool(p["overlay"])
    return p


class InstanceMaps(PackedSamples):
    """Result of instance_maps for the n frames of the detections: map (packed uint8 like the labels: 0 background, 1 + (id mod 252) the
    pixels of a row with a track id, 255 foreground without one), row_gt (int64 [n, k]: the pixels of row r's component under the
    annotation, zeros without one) and frame_stats (int64 [n, 3] = pixels with a track, pixels of value 255, annotated pixels), on the
    device, in the labels' `layout`."""

    def __init__(self, map, row_gt, frame_stats, layout):
        PackedSamples.__init__(self, layout, map.device)
        self.map, self.row_gt, self.frame_stats = map, row_gt, frame_stats
        self.data = map  # (what visualize.overlay_instances and the other takers of packed bytes look for)
        self._host = None

    def sample(self, i):
        """[H_i, W_i] uint8 view of frame i's map."""
        return self._view(self.map, i)

    def host(self):
        """(row_gt, frame_stats) as numpy arrays: one copy of each per InstanceMaps, made on first use."""
        if self._host is None:
            self._host = (_host(self.row_gt), _host(self.frame_stats))
        return self._host


def check_instance_arguments(layout, detections, ids, gt=None):
    """The host validation of instance_maps (ValueError): `layout` (the labels') equals the detections', dets / counts have their shapes
    with k in 1..DET_MAX_K, ids is an int32 tensor [n, k], gt is None, a PackedSamples in the same layout (its `data`) or a uint8 tensor of
    the labels' length.  Returns the annotation's packed buffer, or None."""
    n, k = detections.layout.n, int(detections.k)
    if not layout.same_as(detections.layout):
        raise ValueError("the labels must be packed like the detections' frames (same offsets and sizes)")
    if tuple(detections.dets.shape) != (n, k, DET_FIELDS) or tuple(detections.counts.shape) != (n, 3) or not 1 <= k <= DET_MAX_K:
        raise ValueError("detections: dets must be [{}, k, {}] and counts [{}, 3] with k in 1..{}".format(n, DET_FIELDS, n, DET_MAX_K))
    require_tensor(ids, "tracks.ids", torch.int32, 2, cuda=False)
    if tuple(ids.shape) != (n, k):
        raise ValueError("tracks.ids must be [{}, {}]: one id per row of the detections".format(n, k))
    if isinstance(gt, PackedSamples):
        if not gt.layout.same_as(layout):
            raise ValueError("the annotations must be packed like the labels (same offsets and sizes)")
        gt = gt.data
    if gt is not None:
        require_tensor(gt, "gt (packed like the labels)", torch.uint8, 1, layout.numel, cuda=False)
    return gt


def instance_maps(selection_or_labels, detections, tracks, gt=None) -> InstanceMaps:
    """The instance maps of n linked frames in one call of udet_track_instance_maps_ragged (two launches whatever n, k and the number of
    components and sequences; nothing comes back to the host).  selection_or_labels / detections: what link_detections took; tracks: the
    Tracks it returned (or anything with its `ids`, int32 [n, k] on the device); gt: optional, the batch's annotations -- a
    native_results.GtBatch (any PackedSamples with the 0 / non-0 bytes as `data`) or a 1-D uint8 device tensor packed like the labels.
    A pixel whose label is the root of row r takes 1 + (ids[i][r] mod 252) when the row has an id; foreground of any other component
    (below min_area, past max_detections, a row without an id) takes 255, background 0; row_gt[i][r] counts the pixels of row r's
    component under the annotation and frame_stats[i] = (pixels with a track, pixels of value 255, annotated pixels) -- exact integers
    (include/udet.h).  Validated on the host before the device is touched (ValueError)."""
    labels, layout, _ = packed_labels(selection_or_labels, None if isinstance(selection_or_labels, ComponentSelection) else detections.layout)
    total = int(require_tensor(labels, "labels (packed samples)", torch.int32, 1, cuda=False).numel())
    layout = as_layout(layout, None, total, max_samples=65535)
    for t, name, nd in ((detections.dets, "dets", 3), (detections.counts, "counts", 2)):
        require_tensor(t, "detections." + name, torch.int64, nd, cuda=False)
    gt = check_instance_arguments(layout, detections, tracks.ids, gt)
    require_tensor(labels, "labels (packed samples)", torch.int32, 1)
    dev, n, k = labels.device, layout.n, int(detections.k)
    require_tensor(detections.dets, "detections.dets", torch.int64, 3, device=dev)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    require_tensor(tracks.ids, "tracks.ids", torch.int32, 2, device=dev)
    if gt is not None:
        require_tensor(gt, "gt (packed like the labels)", torch.uint8, 1, total, dev)
    d_off, d_hw = layout.device_tables(dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    row_gt = torch.empty((n, k), dtype=torch.int64, device=dev)
    frame_stats = torch.empty((n, 3), dtype=torch.int64, device=dev)
    ws = workspace(lib.udet_track_instance_maps_workspace_bytes(total, n, k), 4, dev)
    check(lib.udet_track_instance_maps_ragged(labels.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, total,
                                              detections.dets.data_ptr(), detections.counts.data_ptr(), k, tracks.ids.data_ptr(),
                                              None if gt is None else gt.data_ptr(), out.data_ptr(), row_gt.data_ptr(),
                                              frame_stats.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return InstanceMaps(out, row_gt, frame_stats, layout)


def track_gt_scores(records, row_gt, gt_area, starts):
    """How good every single track is against the annotation, per sequence: records (track_records' lists, one per frame: every record
    has "track" and "area", in rank order), row_gt (per frame the integers of InstanceMaps.row_gt, at least one per record), gt_area (per
    frame the annotated pixels, frame_stats[:, 2]) and starts (per frame, true where a sequence starts) -> a list of sequences in the
    frames' order, each {"frames", "gt_j_mean": {id: mean}, "best_track": {"id", "gt_j_mean"} or None, "best_j"}.  Per frame a track with
    a row has j = row_gt / (area + gt_area - row_gt) in float64 from the integers; where it has no row, j = 1.0 if the frame's gt_area
    is 0, else 0.0 -- the "both empty is 1" convention of evaluate_batch_davis.  gt_j_mean is the mean over ALL frames of the sequence:
    the first and the last frame are not skipped (unlike the DAVIS table's J), so a track that appears late or ends early pays for
    every frame it misses.  best_track is the largest mean, ties to the smaller id, None for a sequence without tracks; best_j is its
    mean, or for a sequence without tracks the mean of the frames' "no row" value."""
    if not (len(records) == len(row_gt) == len(gt_area) == len(starts)):
        raise ValueError("one list of records, one row of row_gt, one gt_area and one start flag per frame")
    bounds = [i for i in range(len(records)) if i == 0 or starts[i]] + [len(records)]
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        absent = np.array([1.0 if int(gt_area[i]) == 0 else 0.0 for i in range(lo, hi)], np.float64)
        per = {}
        for i in range(lo, hi):
            if len(records[i]) > len(row_gt[i]):
                raise ValueError("frame {}: more records than rows".format(i))
            for r, rec in enumerate(records[i]):
                inter = int(row_gt[i][r])
                j = per.setdefault(int(rec["track"]), absent.copy())
                j[i - lo] = np.float64(inter) / np.float64(int(rec["area"]) + int(gt_area[i]) - inter)
        means = {t: float(np.mean(j)) for t, j in sorted(per.items())}
        best = None
        for t, m in means.items():  # ascending ids: a tie keeps the smaller
            if best is None or m > best["gt_j_mean"]:
                best = {"id": t, "gt_j_mean": m}
        out.append({"frames": hi - lo, "gt_j_mean": means, "best_track": best,
                    "best_j": best["gt_j_mean"] if best is not None else float(np.mean(absent))})
    return out
