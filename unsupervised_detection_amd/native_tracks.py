"""Native-resolution stage, step 4: the detections of consecutive frames linked into tracks by mask overlap (csrc/tracks.hip,
DESIGN.md 7.8), across frames in which a component is missing with max_gap > 0, along a displacement per pixel with
disp (native_motion.flow_displacements makes one from the optical flow).

  link_detections(selection_or_labels, detections, link, carry, min_iou, max_gap)   one call of udet_link_detections_ragged -> Tracks;
                                                tail() carries the last frame into the next call (TrackTail).  max_gap > 0: a track also
                                                survives up to max_gap frames without its component (udet_link_detections_gap_ragged),
                                                and tail() carries the last max_gap + 1 frames (TrackHistory)
  check_link_arguments                          its host validation (no GPU needed)
  track_records / summarise_tracks              the detection records with their tracks, and every track of a sequence
  track_params / track_max_gap / min_iou_permille   the `tracks` dict of native_results.restore_results_dir, filled in and checked"""
import numpy as np
import torch

from ._ffi import check, lib
from .native_components import ComponentSelection, packed_labels
from .native_detections import DET_FIELDS, DET_MAX_K, _host
from .ragged import as_layout, require_tensor, workspace

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
        if not isinstance(tracks, dict) or not set(tracks) <= set(TRACK_DEFAULTS) | {"max_gap", "motion"}:
            raise ValueError("tracks must be a dict with keys among {}".format(sorted(set(TRACK_DEFAULTS) | {"max_gap", "motion"})))
        p.update({k: v for k, v in tracks.items() if v is not None})
    min_iou_permille(p["min_iou"])
    p["min_iou"] = float(p["min_iou"])
    gap, motion = track_max_gap(p.pop("max_gap", 0)), p.pop("motion", None)
    if gap:  # the key only when gaps are bridged: without it the dict is what it was
        p["max_gap"] = gap
    if motion is not None:  # likewise: {"size": (fh, fw)} only when the link follows the flow
        from .native_motion import motion_params
        p["motion"] = motion_params(motion)
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
    (int32 [m, k]) its open flags after this call.  motion: whether it was linked through displacements (inter / union may then exceed 1)."""

    def __init__(self, inter, match, ids, linked, seq_tracks, next_id, labels, detections, carry=None, back=None, prev=None, gap_inter=None,
                 open=None, max_gap=0, hist_open=None, motion=False):
        self.inter, self.match, self.ids, self.linked, self.seq_tracks, self.next_id = inter, match, ids, linked, seq_tracks, next_id
        self.labels, self.detections, self.carry, self.k = labels, detections, carry, int(ids.shape[1])
        self.back, self.prev, self.gap_inter, self.open, self.max_gap, self.hist_open = back, prev, gap_inter, open, int(max_gap), hist_open
        self.motion = bool(motion)
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


def check_link_arguments(layout, detections, link, carry, min_iou, max_gap=0, disp=None):
    """The host validation of link_detections (ValueError): `layout` (the labels') equals the detections', dets / counts have their shapes, link is None or n values 0 / 1, carry is None or a TrackTail of the same k (max_gap > 0: a TrackHistory of the same k and max_gap), min_iou
    rounds to a permille in 1..1000, disp is None or an int32 tensor of one element per element of the labels' buffer.  Returns (link as int32 [n] or None when it is a device tensor, permille)."""
    n, k = detections.layout.n, int(detections.k)
    if not layout.same_as(detections.layout):
        raise ValueError("the labels must be packed like the detections' frames (same offsets and sizes)")
    if tuple(detections.dets.shape) != (n, k, DET_FIELDS) or tuple(detections.counts.shape) != (n, 3) or not 1 <= k <= DET_MAX_K:
        raise ValueError("detections: dets must be [{}, k, {}] and counts [{}, 3] with k in 1..{}".format(n, DET_FIELDS, n, DET_MAX_K))
    permille = min_iou_permille(min_iou)
    if disp is not None:
        require_tensor(disp, "disp (one packed displacement per pixel, laid out like the labels)", torch.int32, 1, layout.numel, cuda=False)
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


def link_detections(selection_or_labels, detections, link=None, carry=None, min_iou=0.1, max_gap=0, disp=None) -> Tracks:
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
    of a Tracks with the same k and max_gap returns (its tensors stay as they are: the open flags this call closes are in hist_open).
    disp (None): a device int32 tensor of one packed displacement per element of labels (dx in the low 16 bits, dy in the
    high 16; native_motion.flow_displacements) -- one call of udet_link_detections_motion_ragged (with max_gap: of
    udet_link_detections_gap_motion_ragged) in its place: inter counts a pixel of the frame against the predecessor's label at
    (x + dx, y + dy), a source outside the frame counts nothing, and everything else is as above (only stage 1 of the gap form is warped).
    The Tracks says so in `motion`.  None is the co-located call, byte for byte."""
    max_gap = track_max_gap(max_gap)
    labels, layout, _ = packed_labels(selection_or_labels, None if isinstance(selection_or_labels, ComponentSelection) else detections.layout)
    total = int(require_tensor(labels, "labels (packed samples)", torch.int32, 1, cuda=False).numel())
    as_layout(layout, None, total, max_samples=65535)
    for t, name, nd in ((detections.dets, "dets", 3), (detections.counts, "counts", 2)):
        require_tensor(t, "detections." + name, torch.int64, nd, cuda=False)
    host_link, permille = check_link_arguments(layout, detections, link, carry, min_iou, max_gap, disp)
    require_tensor(labels, "labels (packed samples)", torch.int32, 1)
    dev, n, k = labels.device, layout.n, detections.k
    if disp is not None:
        require_tensor(disp, "disp (one packed displacement per pixel, laid out like the labels)", torch.int32, 1, total, device=dev)
    require_tensor(detections.dets, "detections.dets", torch.int64, 3, device=dev)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    carried = {}  # the carry's tensors by name, in the order they are checked; `open` is the TrackHistory's alone
    if carry is not None:
        carried = {name: getattr(carry, name) for name in ("labels", "dets", "counts", "ids", "next_id") + (("open",) if max_gap else ())}
    for name, t in carried.items():
        require_tensor(t, "carry." + name, torch.int64 if name in ("dets", "counts") else torch.int32, device=dev)
    d_link = link if host_link is None else torch.from_numpy(host_link).to(dev)
    d_off, d_hw = layout.device_tables(dev)
    inter = torch.empty((n, k, k), dtype=torch.int64, device=dev)
    match, ids = (torch.empty((n, k), dtype=torch.int32, device=dev) for _ in range(2))
    linked, seq_tracks = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    next_id = torch.empty(1, dtype=torch.int32, device=dev)
    gap_inter = back = prev = open = hist_open = None
    if max_gap:
        gap_inter = torch.empty((n, max_gap, k, k), dtype=torch.int64, device=dev)
        back, prev, open = (torch.empty((n, k), dtype=torch.int32, device=dev) for _ in range(3))
        if carry is not None:
            hist_open = carried["open"] = carry.open.clone()  # closed in place by the call: the carry stays what it is
    ch, cw = carry.hw if carry is not None else (0, 0)
    c = {name: t.data_ptr() for name, t in carried.items()}.get  # c(name): the pointer, NULL without a carry
    frames = (labels.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, total, detections.dets.data_ptr(),
              detections.counts.data_ptr(), k, d_link.data_ptr())
    results = (inter.data_ptr(), match.data_ptr(), ids.data_ptr(), linked.data_ptr(), seq_tracks.data_ptr(), next_id.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    moved = () if disp is None else (disp.data_ptr(),)  # the motion entries take disp in front of the workspace
    if max_gap:
        m = carry.m if carry is not None else 0
        ws = workspace(lib.udet_link_detections_gap_workspace_bytes(total, n, k, max_gap, m, ch, cw), 4, dev)
        entry = lib.udet_link_detections_gap_ragged if disp is None else lib.udet_link_detections_gap_motion_ragged
        check(entry(*frames, max_gap, m, c("labels"), ch, cw, c("dets"), c("counts"), c("ids"), c("open"), c("next_id"), permille, *results,
                    gap_inter.data_ptr(), back.data_ptr(), prev.data_ptr(), open.data_ptr(), *moved, ws.data_ptr(), ws.numel(), stream))
    else:
        ws = workspace(lib.udet_link_detections_workspace_bytes(total, n, k, ch, cw), 4, dev)
        entry = lib.udet_link_detections_ragged if disp is None else lib.udet_link_detections_motion_ragged
        check(entry(*frames, c("labels"), ch, cw, c("dets"), c("counts"), c("ids"), c("next_id"), permille, *results, *moved, ws.data_ptr(),
                    ws.numel(), stream))
    return Tracks(inter, match, ids, linked, seq_tracks, next_id, labels, detections, carry, back, prev, gap_inter, open, max_gap, hist_open,
                  disp is not None)


def track_records(records, tracks):
    """The per-frame detection records (detection_records' lists, in the frames' order) with their tracks: every record gains "track"
    (its id within its sequence), "prev" (the rank of the row it continues in the frame before, or None) and "iou" (inter / (area_a +
    area_b - inter) of that pair in float64, or None).  tracks: a Tracks (or anything with its host(), detections.dets and carry.dets).  Returns
    new lists; the records given stay as they are.  Linked with gap bridging (tracks.max_gap > 0, host_gaps() and a TrackHistory as
    carry), every record gains "back" as well (1: it continues the frame before, d >= 2: a bridge to frame c - d, 0: a new track),
    "prev" is the rank in frame c - back and the "iou" of a bridged row comes from gap_inter.  Linked with motion (tracks.motion), "iou" is
    min(1.0, inter / union): displacements may map many pixels onto one, so inter may exceed the predecessor's area."""
    inter, match, ids, _, _ = tracks.host()
    if len(records) != len(ids):
        raise ValueError("one list of records per frame")
    dets = _host(tracks.detections.dets)
    gaps, motion = getattr(tracks, "max_gap", 0) > 0, bool(getattr(tracks, "motion", False))
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
                if motion:
                    iou = min(1.0, iou)
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
