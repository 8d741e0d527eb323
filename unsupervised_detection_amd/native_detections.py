"""Native-resolution stage, step 3: every connected component as a scored box -- the detections at native size
(csrc/detections.hip).

  component_boxes(selection_or_labels, score, min_area, max_detections)   every component of the labelled masks as a scored box, the
                                                largest first (udet_component_boxes_ragged) -> Detections
  detection_records(detections, amax)           the same as plain records (box, area, centroid, score, root)
  detection_params(detections)                  the `detections` dict of native_results.restore_results_dir, filled in and checked"""
import numpy as np
import torch

from ._ffi import check, lib
from .native_components import packed_labels
from .native_restore import RestoredMasks
from .ragged import INT32_MAX, PackedSamples, as_layout, require_tensor, workspace

DET_FIELDS = 9  # UDET_DET_FIELDS: root, area, y0, x0, y1, x1, sum_y, sum_x, score_sum
DET_MAX_K = 64  # UDET_DET_MAX_K
DETECTION_DEFAULTS = {"min_area": 64, "max_detections": 16}


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


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
    if p["min_area"] < 1 or p["min_area"] > INT32_MAX or not 1 <= p["max_detections"] <= DET_MAX_K:
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
    labels, offsets, hw = packed_labels(selection_or_labels, offsets, hw)
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
