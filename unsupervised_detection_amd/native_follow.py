"""Native-resolution stage, step 6: the masks of whole tracks -- which tracks of a sequence to follow is decided on the host once the
sequence is known, and the choice is turned back into binary masks on the device (csrc/follow.hip).

  follow_params(follow)                         the `follow` dict of native_results.restore_results_dir, filled in and checked
  choose_tracks(records, score_sums, starts, rule, min_frames, gt_j_mean)   per sequence the tracks kept, per frame their ranks (host, integers)
  keep_words(kept_ranks, n)                     the ranks as one 64-bit word per frame
  follow_tracks(selection_or_labels, detections, keep, gt)   one call of udet_follow_tracks_ragged -> FollowedMasks: the binary masks of the
                                                kept rows and per frame (kept, dropped, kept under gt, gt) pixel counts
  check_follow_arguments                        its host validation (no GPU needed)"""
import numpy as np
import torch

from ._ffi import check, lib
from .native_components import ComponentSelection, packed_labels
from .native_detections import DET_FIELDS, DET_MAX_K, _host
from .ragged import PackedSamples, as_layout, require_tensor, workspace

FOLLOW_RULES = ("mass", "area", "length", "best_gt", "all")
FOLLOW_DEFAULTS = {"rule": "mass", "min_frames": 1}


def follow_params(follow=None):
    """The `follow` dict of restore_results_dir ({} or None: the defaults) with the defaults filled in and checked (ValueError): rule one
    of FOLLOW_RULES, min_frames an integer >= 1."""
    p = dict(FOLLOW_DEFAULTS)
    if follow is not None:
        if not isinstance(follow, dict) or not set(follow) <= set(FOLLOW_DEFAULTS):
            raise ValueError("follow must be a dict with keys among {}".format(sorted(FOLLOW_DEFAULTS)))
        p.update(follow)
    if not isinstance(p["rule"], str) or p["rule"] not in FOLLOW_RULES:
        raise ValueError("follow: rule must be one of {}".format(", ".join(FOLLOW_RULES)))
    m = p["min_frames"]
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 1:
        raise ValueError("follow: min_frames must be an integer >= 1")
    p["min_frames"] = int(m)
    return p


def choose_tracks(records, score_sums, starts, rule, min_frames, gt_j_mean=None):
    """Which tracks to follow, per sequence, once the sequence is known: records (track_records' lists, one per frame: every record has
    "track" and "area", in rank order), score_sums (per frame the integer score_sum of its rows, dets[..., 8], at least one per record),
    starts (per frame, true where a sequence starts -- what summarise_tracks takes) -> (kept_ranks: per frame the ranks of the kept rows,
    ascending; kept_ids: per sequence the ids of the kept tracks, ascending).  A track is eligible when it has rows in at least min_frames
    frames of its sequence.  rule "all" keeps every eligible track; the others keep one per sequence: "mass" the largest sum of score_sum
    over its frames, "area" the largest sum of area, "length" the most frames, "best_gt" the largest gt_j_mean (gt_j_mean: per sequence
    the {id: mean} of track_gt_scores).  Python integers throughout (float64 for gt_j_mean); ties go to the track with more frames, then
    the smaller id; a sequence without an eligible track keeps nothing."""
    p = follow_params({"rule": rule, "min_frames": min_frames})
    if not (len(records) == len(score_sums) == len(starts)):
        raise ValueError("one list of records, one list of score_sums and one start flag per frame")
    bounds = [i for i in range(len(records)) if i == 0 or starts[i]] + [len(records)]
    if p["rule"] == "best_gt" and (gt_j_mean is None or len(gt_j_mean) != len(bounds) - 1):
        raise ValueError('rule "best_gt" needs gt_j_mean: one {id: mean} per sequence')
    kept_ranks, kept_ids = [[] for _ in records], []
    for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        frames, mass, area = {}, {}, {}
        for i in range(lo, hi):
            if len(records[i]) > len(score_sums[i]):
                raise ValueError("frame {}: more records than score_sums".format(i))
            for r, rec in enumerate(records[i]):  # (an id names at most one row of a frame)
                t = int(rec["track"])
                frames[t] = frames.get(t, 0) + 1
                mass[t] = mass.get(t, 0) + int(score_sums[i][r])
                area[t] = area.get(t, 0) + int(rec["area"])
        eligible = sorted(t for t, c in frames.items() if c >= p["min_frames"])
        if p["rule"] == "all" or not eligible:
            keep = eligible
        else:
            value = {"mass": mass, "area": area, "length": frames}.get(p["rule"])
            if value is None:
                value = {t: np.float64(gt_j_mean[s][t]) for t in eligible}
            keep = [max(eligible, key=lambda t: (value[t], frames[t], -t))]
        kept_ids.append(keep)
        for i in range(lo, hi):
            kept_ranks[i] = [r for r, rec in enumerate(records[i]) if int(rec["track"]) in keep]
    return kept_ranks, kept_ids


def keep_words(kept_ranks, n):
    """uint64 [n]: bit r of word i is set for every rank r of kept_ranks[i] (ranks in 0..DET_MAX_K - 1; ValueError otherwise)."""
    if len(kept_ranks) != int(n):
        raise ValueError("one list of kept ranks per frame")
    words = np.zeros(int(n), np.uint64)
    for i, ranks in enumerate(kept_ranks):
        w = 0
        for r in ranks:
            if isinstance(r, (bool, np.bool_)) or int(r) != r or not 0 <= int(r) < DET_MAX_K:
                raise ValueError("frame {}: a kept rank must be an integer in 0..{}".format(i, DET_MAX_K - 1))
            w |= 1 << int(r)
        words[i] = w
    return words


class FollowedMasks(PackedSamples):
    """Result of follow_tracks for the n frames of the detections: selected (packed uint8 0 / 1 like the labels, also `data`: 1 on the
    pixels of the kept rows) and stats (int64 [n, 4] = kept pixels, dropped foreground pixels, kept pixels under the annotation, annotated
    pixels), on the device, in the labels' `layout`.  binary_sample / stack have the contract of ComponentSelection / RestoredMasks: the
    scoring, drawing and export loops take either."""

    def __init__(self, selected, stats, layout):
        PackedSamples.__init__(self, layout, selected.device)
        self.selected, self.stats = selected, stats
        self.data = selected
        self._host = None

    def binary_sample(self, i):
        """[H_i, W_i] uint8 view of frame i's mask."""
        return self._view(self.selected, i)

    sample = binary_sample

    def host(self):
        """stats as a numpy array: one copy per FollowedMasks, made on first use."""
        if self._host is None:
            self._host = _host(self.stats)
        return self._host


def check_follow_arguments(layout, detections, keep, gt=None):
    """The host validation of follow_tracks (ValueError): `layout` (the labels') equals the detections', dets / counts have their shapes
    with k in 1..DET_MAX_K, keep is one 64-bit word per frame -- an array or sequence of n non-negative integers below 2^64 (keep_words' result), or
    an int64 tensor [n] holding the same bits -- and gt is None, a PackedSamples in the same layout (its `data`) or a uint8 tensor of the
    labels' length.  Returns (keep as an int64 tensor [n], where it was given, the annotation's packed buffer or None)."""
    n, k = detections.layout.n, int(detections.k)
    if not layout.same_as(detections.layout):
        raise ValueError("the labels must be packed like the detections' frames (same offsets and sizes)")
    if tuple(detections.dets.shape) != (n, k, DET_FIELDS) or tuple(detections.counts.shape) != (n, 3) or not 1 <= k <= DET_MAX_K:
        raise ValueError("detections: dets must be [{}, k, {}] and counts [{}, 3] with k in 1..{}".format(n, DET_FIELDS, n, DET_MAX_K))
    if isinstance(keep, torch.Tensor):
        if keep.dtype != torch.int64 or tuple(keep.shape) != (n,):
            raise ValueError("keep must be one 64-bit word per frame: an int64 tensor [{}]".format(n))
    else:
        words = np.asarray(keep)
        if words.shape != (n,) or words.dtype.kind not in "iu" or (words.dtype.kind == "i" and (words < 0).any()):
            raise ValueError("keep must be one 64-bit word per frame: {} unsigned integers (keep_words)".format(n))
        keep = torch.from_numpy(np.ascontiguousarray(words.astype(np.uint64)).view(np.int64))
    if isinstance(gt, PackedSamples):
        if not gt.layout.same_as(layout):
            raise ValueError("the annotations must be packed like the labels (same offsets and sizes)")
        gt = gt.data
    if gt is not None:
        require_tensor(gt, "gt (packed like the labels)", torch.uint8, 1, layout.numel, cuda=False)
    return keep, gt


def follow_tracks(selection_or_labels, detections, keep, gt=None) -> FollowedMasks:
    """The binary masks of the kept rows of n frames in one call of udet_follow_tracks_ragged (two launches whatever n, k and the number of
    components and sequences; nothing comes back to the host).  selection_or_labels / detections: what link_detections took; keep: one
    64-bit word per frame, bit r = keep row r (keep_words of choose_tracks' ranks; a host array is uploaded, an int64 device tensor is
    taken as it is); gt: optional, the batch's annotations -- a native_results.GtBatch (any PackedSamples with the 0 / non-0 bytes as
    `data`) or a 1-D uint8 device tensor packed like the labels.  A pixel is 1 exactly when its label is the root of a row r below the
    frame's rows and bit r of its frame's word is set; bits at or above the rows are ignored; stats[i] = (kept, dropped foreground, kept
    under gt, gt) pixels -- exact integers (include/udet.h).  Validated on the host before the device is touched (ValueError)."""
    labels, layout, _ = packed_labels(selection_or_labels, None if isinstance(selection_or_labels, ComponentSelection) else detections.layout)
    total = int(require_tensor(labels, "labels (packed samples)", torch.int32, 1, cuda=False).numel())
    layout = as_layout(layout, None, total, max_samples=65535)
    for t, name, nd in ((detections.dets, "dets", 3), (detections.counts, "counts", 2)):
        require_tensor(t, "detections." + name, torch.int64, nd, cuda=False)
    keep, gt = check_follow_arguments(layout, detections, keep, gt)
    require_tensor(labels, "labels (packed samples)", torch.int32, 1)
    dev, n, k = labels.device, layout.n, int(detections.k)
    require_tensor(detections.dets, "detections.dets", torch.int64, 3, device=dev)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    if gt is not None:
        require_tensor(gt, "gt (packed like the labels)", torch.uint8, 1, total, dev)
    keep = require_tensor(keep if keep.is_cuda else keep.to(dev), "keep", torch.int64, 1, n, dev)
    d_off, d_hw = layout.device_tables(dev)
    selected = torch.empty(total, dtype=torch.uint8, device=dev)
    stats = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ws = workspace(lib.udet_follow_tracks_workspace_bytes(total, n, k), 4, dev)
    check(lib.udet_follow_tracks_ragged(labels.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, total,
                                        detections.dets.data_ptr(), detections.counts.data_ptr(), k, keep.data_ptr(),
                                        None if gt is None else gt.data_ptr(), selected.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream))
    return FollowedMasks(selected, stats, layout)
