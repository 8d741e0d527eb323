"""Native-resolution stage, step 7: the tracks against multi-object annotations -- per frame the pixels every row shares with every
annotated object, counted on the device (csrc/objects.hip), and per sequence the one-to-one matching of objects to tracks with region
similarity J per object, as the DAVIS-2017 unsupervised protocol judges instance ids.

  ObjectRule / OBJECT_RULES / load_objects_device   an annotation decoded as object ids at native size (a mode-"P" PNG: its palette
                                                indices; a mode-"L" image: its grey values), in one ragged.PackedLayout per batch
  object_overlaps(selection_or_labels, detections, objects, num_objects)   one call of udet_track_object_overlaps_ragged ->
                                                ObjectOverlaps: row_obj, obj_area and frame_stats
  check_object_arguments                        its host validation (no GPU needed)
  object_params                                 the `objects` dict of native_results.restore_results_dir, filled in and checked
  match_tracks(records, ids_rows, row_obj, obj_area, starts, skip_ends)   per sequence the assignment and every object's J
  objects_summary                               the dataset numbers of native_eval.json from the sequences' records"""
import numpy as np
import torch

from ._ffi import check, lib
from .native_components import ComponentSelection, packed_labels
from .native_detections import DET_FIELDS, DET_MAX_K, _host
from .ragged import PackedSamples, as_layout, require_tensor, workspace

MAX_OBJECTS = 32  # UDET_MAX_OBJECTS
OBJECT_VOID = 255  # the void label of the DAVIS / YouTube-VOS annotations: never an object, never warned about
OBJECT_DEFAULTS = {"max": 16, "dir": None}


class ObjectRule(object):
    """How a dataset's annotation becomes object ids at native size: loader(path, channels) -> uint8 [H,W,1] on the host (None:
    read_object_ids, the raw palette indices or grey values).  Nothing is binarised."""

    def __init__(self, loader=None):
        self.loader = loader


def read_object_ids(path, channels=1):
    """uint8 [H,W,1] object ids of an annotation file: the raw palette indices of a mode-"P" image (the DAVIS-2017 layout), the raw
    grey values of a mode-"L" image; any other mode is a ValueError that names the file."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("P", "L"):
            raise ValueError("{}: an object annotation must be an indexed (mode P) or grey (mode L) image, not mode {}".format(path, im.mode))
        return np.asarray(im, dtype=np.uint8).reshape(im.size[1], im.size[0], 1)


# every dataset with id annotations reads them the same way; per-object folders (SegTrackV2) and colour-coded files (FBMS) are converted
# to id PNGs by the user and passed as objects["dir"]
OBJECT_RULES = {"DAVIS2016": ObjectRule(), "SEGTRACK": ObjectRule(), "FBMS": ObjectRule()}


class ObjectBatch(PackedSamples):
    """Object annotations of one batch at native size: data (packed uint8 ids) in the layout given; max_id: per frame the largest byte
    other than OBJECT_VOID, seen on the host while the file was decoded (None: not known)."""

    def __init__(self, data, layout, max_id=None):
        PackedSamples.__init__(self, as_layout(layout, None, data.numel()), data.device)
        self.data, self.max_id = data, max_id

    def sample(self, i):
        return self._view(self.data, i)


def load_objects_device(paths, rule=None):
    """The object annotations of a batch through data.RaggedLoader (the loader load_gt_device uses: mixed sizes, one pinned buffer, one
    copy) -> a PackedSamples whose `data` is the uint8 id buffer, with every frame's largest id below 255 as `max_id`."""
    from .native_results import _loader
    paths = list(paths)
    decode = (rule.loader if rule is not None else None) or read_object_ids
    top = {}

    def load(path, channels):
        a = decode(path, channels)
        top[path] = int(np.max(a, initial=0, where=a != OBJECT_VOID))
        return a

    rb = _loader().load(paths, 1, loader=load)
    return ObjectBatch(rb.data, rb.layout, [top[p] for p in paths])


def object_params(objects=None):
    """The `objects` dict of restore_results_dir ({} or None: the defaults) with the defaults filled in and checked (ValueError): max an
    int in 1..32 (16), dir None or a path."""
    p = dict(OBJECT_DEFAULTS)
    if objects is not None:
        if not isinstance(objects, dict) or not set(objects) <= set(OBJECT_DEFAULTS):
            raise ValueError("objects must be a dict with keys among {}".format(sorted(OBJECT_DEFAULTS)))
        p.update({k: v for k, v in objects.items() if v is not None})
    if isinstance(p["max"], (bool, np.bool_)) or not isinstance(p["max"], (int, np.integer)) or not 1 <= int(p["max"]) <= MAX_OBJECTS:
        raise ValueError("objects: max must be an int in 1..{}".format(MAX_OBJECTS))
    p["max"] = int(p["max"])
    if p["dir"] is not None:
        import os
        if not isinstance(p["dir"], (str, os.PathLike)):
            raise ValueError("objects: dir must be None or a path")
        p["dir"] = os.fspath(p["dir"])
    return p


class ObjectOverlaps(object):
    """Result of object_overlaps for the n frames of the detections: row_obj (int64 [n, k, O]: the pixels of row r's component with object
    byte o + 1), obj_area (int64 [n, O]: the pixels with object byte o + 1) and frame_stats (int64 [n, 2] = pixels of an object, void
    pixels), on the device, in the labels' `layout`."""

    def __init__(self, row_obj, obj_area, frame_stats, layout, num_objects):
        self.row_obj, self.obj_area, self.frame_stats, self.layout, self.num_objects = row_obj, obj_area, frame_stats, layout, int(num_objects)
        self._host = None

    def host(self):
        """(row_obj, obj_area, frame_stats) as numpy arrays: one copy of each per ObjectOverlaps, made on first use."""
        if self._host is None:
            self._host = (_host(self.row_obj), _host(self.obj_area), _host(self.frame_stats))
        return self._host


def check_object_arguments(layout, detections, objects, num_objects):
    """The host validation of object_overlaps (ValueError): `layout` (the labels') equals the detections', dets / counts have their shapes
    with k in 1..DET_MAX_K, objects is a PackedSamples in the same layout (its `data`) or a uint8 tensor of the labels' length, num_objects
    an int in 1..MAX_OBJECTS.  Returns (the annotation's packed buffer, num_objects)."""
    n, k = detections.layout.n, int(detections.k)
    if not layout.same_as(detections.layout):
        raise ValueError("the labels must be packed like the detections' frames (same offsets and sizes)")
    if tuple(detections.dets.shape) != (n, k, DET_FIELDS) or tuple(detections.counts.shape) != (n, 3) or not 1 <= k <= DET_MAX_K:
        raise ValueError("detections: dets must be [{}, k, {}] and counts [{}, 3] with k in 1..{}".format(n, DET_FIELDS, n, DET_MAX_K))
    if isinstance(num_objects, (bool, np.bool_)) or not isinstance(num_objects, (int, np.integer)) or not 1 <= int(num_objects) <= MAX_OBJECTS:
        raise ValueError("num_objects must be an int in 1..{}".format(MAX_OBJECTS))
    if objects is None:
        raise ValueError("objects (the annotations' ids, packed like the labels) are required")
    if isinstance(objects, PackedSamples):
        if not objects.layout.same_as(layout):
            raise ValueError("the object annotations must be packed like the labels (same offsets and sizes)")
        objects = objects.data
    require_tensor(objects, "objects (packed like the labels)", torch.uint8, 1, layout.numel, cuda=False)
    return objects, int(num_objects)


def object_overlaps(selection_or_labels, detections, objects, num_objects) -> ObjectOverlaps:
    """What n linked frames share with their annotated objects, in one call of udet_track_object_overlaps_ragged (two launches whatever
    n, k, num_objects and the content; nothing comes back to the host).  selection_or_labels / detections: what link_detections took;
    objects: the batch's object annotations -- load_objects_device's result (any PackedSamples with the id bytes as `data`) or a 1-D uint8
    device tensor packed like the labels: 0 background, 1..num_objects an object, above that void.  row_obj[i][r][o] counts the pixels of
    row r's component with byte o + 1, obj_area[i][o] the pixels with byte o + 1, frame_stats[i] = (pixels of an object, void pixels) --
    exact integers (include/udet.h).  Validated on the host before the device is touched (ValueError)."""
    labels, layout, _ = packed_labels(selection_or_labels, None if isinstance(selection_or_labels, ComponentSelection) else detections.layout)
    total = int(require_tensor(labels, "labels (packed samples)", torch.int32, 1, cuda=False).numel())
    layout = as_layout(layout, None, total, max_samples=65535)
    for t, name, nd in ((detections.dets, "dets", 3), (detections.counts, "counts", 2)):
        require_tensor(t, "detections." + name, torch.int64, nd, cuda=False)
    objects, num_objects = check_object_arguments(layout, detections, objects, num_objects)
    require_tensor(labels, "labels (packed samples)", torch.int32, 1)
    dev, n, k = labels.device, layout.n, int(detections.k)
    require_tensor(detections.dets, "detections.dets", torch.int64, 3, device=dev)
    require_tensor(detections.counts, "detections.counts", torch.int64, 2, device=dev)
    require_tensor(objects, "objects (packed like the labels)", torch.uint8, 1, total, dev)
    d_off, d_hw = layout.device_tables(dev)
    row_obj = torch.empty((n, k, num_objects), dtype=torch.int64, device=dev)
    obj_area = torch.empty((n, num_objects), dtype=torch.int64, device=dev)
    frame_stats = torch.empty((n, 2), dtype=torch.int64, device=dev)
    ws = workspace(lib.udet_track_object_overlaps_workspace_bytes(total, n, k), 4, dev)
    check(lib.udet_track_object_overlaps_ragged(labels.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, total,
                                                detections.dets.data_ptr(), detections.counts.data_ptr(), k, objects.data_ptr(), num_objects,
                                                row_obj.data_ptr(), obj_area.data_ptr(), frame_stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream(dev).cuda_stream))
    return ObjectOverlaps(row_obj, obj_area, frame_stats, layout, num_objects)


def _frame_j(inter, area_t, area_o):
    union = area_t + area_o - inter
    return 1.0 if union == 0 else float(np.float64(inter) / np.float64(union))


def match_tracks(records, ids_rows, row_obj, obj_area, starts, skip_ends=True):
    """Every annotated object matched to at most one track, one-to-one, per sequence, and its region similarity J: records (track_records'
    lists, one per frame, in rank order: every record has "area"), ids_rows (per frame the track id of every row, Tracks.ids, at least
    one per record), row_obj (per frame [rows][O] integers of ObjectOverlaps.row_obj), obj_area (per frame [O]) and starts (per frame,
    true where a sequence starts) -> a list of sequences in the frames' order, each {"frames", "objects": {id: {"track": id or None,
    "J": {mean, recall, decay}, "frames_annotated"}}, "J_mean", "unmatched_tracks": [ids]}.
    Per frame, track t and object o: inter = row_obj[f][r][o - 1] of the row r whose id is t (0 without such a row), area_t that row's
    area (or 0), J = 1.0 if area_t + obj_area - inter == 0 else inter / (area_t + obj_area - inter), in float64 from Python integers --
    the "both empty is 1" convention of track_gt_scores and evaluate_batch_davis.  The frames counted are those of the DAVIS table
    (evaluation.davis_statistics: without the first and the last when skip_ends is set, so a sequence of one or two frames counts none and
    its numbers are NaN, which the dataset mean ignores).  An object takes part when it has a pixel somewhere in the sequence; a track is a
    candidate when it shares a pixel with some object in a counted frame (one without can never beat "unmatched").  The assignment
    maximises the sum over the objects of the mean J over the counted frames (scipy.optimize.linear_sum_assignment, maximize=True, on the
    rectangular matrix objects x (candidates, then one "unmatched" column per object that holds the object's empty-prediction mean): an
    object is left unmatched where a track would score below the empty prediction, so the total is the maximum over every one-to-one
    assignment); a matched pair that shares no pixel in the counted frames is reported as unmatched, and an unmatched object scores the
    empty prediction: 1.0 where its area is 0, else 0.0.  mean / recall / decay are davis_statistics' of the
    object's per-frame J; J_mean is the mean over the sequence's objects (NaN without one); unmatched_tracks are the sequence's track ids
    that no object took."""
    from scipy.optimize import linear_sum_assignment

    from .evaluation import _nanmean, davis_statistics
    if not (len(records) == len(ids_rows) == len(row_obj) == len(obj_area) == len(starts)):
        raise ValueError("one list of records, one row of ids, one table of row_obj, one of obj_area and one start flag per frame")
    bounds = [i for i in range(len(records)) if i == 0 or starts[i]] + [len(records)]
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        nf = hi - lo
        counted = list(range(nf))[1:-1] if skip_ends else list(range(nf))
        num_o = max((len(obj_area[i]) for i in range(lo, hi)), default=0)
        area_o = [[int(obj_area[lo + f][o]) if o < len(obj_area[lo + f]) else 0 for f in range(nf)] for o in range(num_o)]
        objs = [o for o in range(num_o) if any(area_o[o])]
        rows = {}  # track id -> {frame: (area, [inter per object])}
        for f in range(nf):
            i = lo + f
            if len(records[i]) > len(ids_rows[i]) or len(records[i]) > len(row_obj[i]):
                raise ValueError("frame {}: more records than rows".format(i))
            for r, rec in enumerate(records[i]):
                t = int(ids_rows[i][r])
                if t >= 0:
                    rows.setdefault(t, {})[f] = (int(rec["area"]), [int(v) for v in row_obj[i][r]])
        shared = {t: {o: sum(fr[f][1][o] for f in counted if f in fr) for o in objs} for t, fr in rows.items()}
        cands = sorted(t for t in rows if any(shared[t].values()))

        def per_frame(t, o):
            fr = rows.get(t, {}) if t is not None else {}
            return [_frame_j(fr[f][1][o], fr[f][0], area_o[o][f]) if f in fr else _frame_j(0, 0, area_o[o][f]) for f in range(nf)]

        match = {}
        if objs and cands and counted:
            mean = lambda t, o: float(np.mean([per_frame(t, o)[f] for f in counted]))
            m = np.array([[mean(t, o) for t in cands] + [mean(None, o)] * len(objs) for o in objs], np.float64)
            for a, b in zip(*linear_sum_assignment(m, maximize=True)):
                if b < len(cands) and shared[cands[b]][objs[a]] > 0:
                    match[objs[a]] = cands[b]
        seq = {"frames": nf, "objects": {}}
        for o in objs:
            t = match.get(o)
            seq["objects"][o + 1] = {"track": t, "J": davis_statistics(per_frame(t, o), skip_ends),
                                     "frames_annotated": sum(1 for a in area_o[o] if a)}
        seq["J_mean"] = _nanmean([v["J"]["mean"] for v in seq["objects"].values()])
        seq["unmatched_tracks"] = sorted(set(rows) - set(match.values()))
        out.append(seq)
    return out


def objects_summary(params, cats):
    """native_eval.json's "objects" from the categories' lists of match_tracks records ({category: [sequence, ...]}): max, J = {mean,
    recall, decay} as the mean over all objects of all sequences (the DAVIS-2017 protocol's dataset number; NaN entries are ignored) and
    per category its J_mean (the mean over its objects)."""
    from .evaluation import _nanmean
    every = [v["J"] for seqs in cats.values() for seq in seqs for v in seq["objects"].values()]
    return {"max": params["max"], "J": {k: _nanmean([j[k] for j in every]) for k in ("mean", "recall", "decay")},
            "sequences": {c: _nanmean([v["J"]["mean"] for seq in seqs for v in seq["objects"].values()]) for c, seqs in cats.items()}}
