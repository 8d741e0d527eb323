"""Output stage at native resolution: restore a batch of masks to each frame's own size, score them there and export them.

The steps live in one module each -- native_restore (restore_masks), native_components (select_components), native_detections
(component_boxes), native_tracks (link_detections), native_instances (instance_maps), native_follow (follow_tracks) and native_objects (object_overlaps, match_tracks) -- and this module drives them over a folder of results.  Their public names are
importable from here as well.

  GtRule / GT_RULES / GtBatch / load_gt_device  a dataset's annotations binarised at native size, in one ragged.PackedLayout per batch
                                                (the packed layout): built once per batch and handed from call to call
  score_device                                  J / F of a batch (evaluation.evaluate_batch_davis)
  check_crf_tables / load_images_device / crf_refine_restored   the full-resolution dense CRF of run_crf_original_resolution on the
                                                restored batch: unary from the restored bytes, the frames read at their own size,
                                                one call of udet_dense_crf_ragged (csrc/crf.hip) -> the labels as the binary masks
  restore_results_dir(results_dir, frame_lists, out_dir, ...)   restore [+ CRF] [+ component selection] [+ detections [+ tracks
                                                [+ instances] [+ objects]]] + J / F + <sequence>/<frame>.png, result_<k>.mat, native_eval.json
                                                [, detections/<sequence>.json [, tracks/<sequence>.json [, instances/<sequence>/<frame>.png] [, objects/<sequence>.json]]]
  frame_lists_from_reader(flags)                {category: [(image, annotation), ...]} in the readers' own test order; (image, None) for
                                                a folder of frames without annotations (--dataset FRAMES), which restore_results_dir
                                                takes in its annotation-free mode; overlay=... draws the final masks on the frames
                                                (visualize.overlay_native)

The full-resolution CRF (sxy = 60) is restore_results_dir(crf={...}).  Every component as a box with its area, centroid
and score -- the detections -- is restore_results_dir(detections={...}); linking them across the frames of a sequence
is restore_results_dir(tracks={...}), across frames in which a component is missing with tracks={"max_gap": G}
(DESIGN.md 7.9); the tracks as per-frame instance maps, their picture and a track's J against the annotation is
restore_results_dir(instances={...}); exporting and scoring the masks of whole tracks, chosen without the annotation, is
restore_results_dir(follow={...}) (native_follow); linking along the optical flow between the frames is
restore_results_dir(tracks={"motion": {...}}) (native_motion); matching the tracks one-to-one to the objects of a
multi-object annotation, with J per object, is restore_results_dir(objects={...}) (native_objects)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

from .native_components import COMPONENT_MODES, COMPONENT_TILE, ComponentSelection, check_component_tables, select_components  # noqa: F401
from .native_detections import (DET_FIELDS, DET_MAX_K, DETECTION_DEFAULTS, Detections, _host, component_boxes,  # noqa: F401
                                detection_params, detection_records)
from .native_follow import (FOLLOW_DEFAULTS, FOLLOW_RULES, FollowedMasks, check_follow_arguments, choose_tracks, follow_params,  # noqa: F401
                            follow_tracks, keep_words)
from .native_instances import (INSTANCE_PALETTE_BYTES, INSTANCE_UNASSIGNED, INSTANCE_WRAP, InstanceMaps, check_instance_arguments,  # noqa: F401
                               instance_maps, instance_params, track_gt_scores)
from .native_objects import (MAX_OBJECTS, OBJECT_DEFAULTS, OBJECT_RULES, ObjectOverlaps, ObjectRule, check_object_arguments,  # noqa: F401
                             load_objects_device, match_tracks, object_overlaps, object_params, objects_summary)
from .native_restore import TAB, RestoredMasks, build_restore_tables, check_restore_tables, restore_box, restore_masks  # noqa: F401
from .native_motion import BackwardFlow, flow_displacements  # noqa: F401
from .native_tracks import (TRACK_DEFAULTS, TRACK_MAX_GAP, TrackHistory, Tracks, TrackTail, check_link_arguments,  # noqa: F401
                            link_detections, min_iou_permille, summarise_tracks, track_max_gap, track_params, track_records)
from .post_processing import CRF_MAX_SAMPLES, default_radius, dense_crf_ragged, unary_from_restored
from .ragged import PackedLayout, PackedSamples, as_layout, check_packed_tables


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


@functools.lru_cache(maxsize=None)
def _loader():
    """The one data.RaggedLoader the annotations and the frames of every batch go through, made on first use."""
    from . import data
    return data.RaggedLoader()


def load_gt_device(paths, rule):
    """The annotations of a batch through data.RaggedLoader (mixed sizes: one pinned buffer, one copy), binarised on the device."""
    rb = _loader().load(list(paths), 1, loader=rule.loader)
    return GtBatch((rb.data.double() / 255.0 > rule.threshold).to(torch.uint8), rb.layout)


def score_device(gt_stack, pred_stack, bound_th):
    """(J, F) per frame of [k,H,W,1] 0 / 1 stacks, scored as they are (no fg/bg flip)."""
    from .evaluation import evaluate_batch_davis
    _, _, _, j, f = evaluate_batch_davis(gt_stack, pred_stack, 0.5, bound_th, disambiguate=False)
    return j, f


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
    return _loader().load(list(paths), 3)


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


def draw_instance_overlays(frames, maps, overlay):
    """visualize.overlay_instances(frames, maps, alpha, beta, edge of `overlay`): the instance maps of a batch on their frames, every
    track in its colour (visualize.TRACK_PALETTE), one launch."""
    from .visualize import overlay_instances
    return overlay_instances(frames, maps, alpha=overlay["alpha"], beta=overlay["beta"], edge=overlay["edge"])


# ---------------------------------------------------------------------------------------------------------------------------
# The driver: options -> every category through the injected callables -> native_eval.json
# ---------------------------------------------------------------------------------------------------------------------------
def _resolve_options(o):
    """The options of restore_results_dir (`o`: its arguments by their names) checked in this order (ValueError) and filled in, in place:
    batch and bound_th, the dicts through crf_params / detection_params / track_params / visualize.overlay_params / instance_params / follow_params; o gains `boxes`
    (overlay["boxes"] through visualize.box_params, None: no boxes), `free` (no frame has an annotation) and `rule` (the GtRule)."""
    from .evaluation import BOUND_TH
    o.bound_th = BOUND_TH if o.bound_th is None else o.bound_th
    o.batch = max(1, int(o.batch))
    if o.component not in (None, "largest", "best_gt"):
        raise ValueError('component must be None, "largest" or "best_gt"')
    if (o.component is not None or o.detections is not None) and o.connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    o.crf = None if o.crf is None else crf_params(o.crf)
    o.detections = None if o.detections is None else detection_params(o.detections)
    if o.tracks is not None:
        if o.detections is None:
            raise ValueError("tracks links the detections: it needs detections")
        o.tracks = track_params(o.tracks)
        if "motion" in o.tracks and o.motion_flow is None:
            o.motion_flow = BackwardFlow(size=o.tracks["motion"]["size"])
    o.boxes = None
    if o.overlay is not None:
        from .visualize import box_params, overlay_params
        if isinstance(o.overlay, dict) and o.overlay.get("boxes") is not None:
            if o.detections is None:
                raise ValueError('overlay["boxes"] draws the detections: it needs detections')
            o.boxes = box_params(o.overlay["boxes"])
        o.overlay = overlay_params({k: v for k, v in o.overlay.items() if k != "boxes"} if isinstance(o.overlay, dict) else o.overlay)
    if o.instances is not None:
        if o.tracks is None:
            raise ValueError("instances paints the tracks: it needs tracks")
        o.instances = instance_params(o.instances)
        if o.instances["overlay"] and o.overlay is None:
            raise ValueError('instances["overlay"] draws the maps on the overlays: it needs overlay')
    missing = [a is None for entries in o.frame_lists.values() for _, a in entries]
    o.free = bool(missing) and all(missing)  # annotation-free: sizes from the frames, nothing to score against
    if any(missing) and not o.free:
        raise ValueError("frame_lists mixes frames with and without an annotation")
    if o.free and o.component == "best_gt":
        raise ValueError('component "best_gt" needs annotations: use "largest" or None')
    if o.follow is not None:
        if o.tracks is None:
            raise ValueError("follow chooses among the tracks: it needs tracks")
        if o.component is not None:
            raise ValueError("follow and component are alternative answers to which component is the mask: pass one of them")
        o.follow = follow_params(o.follow)
        if o.follow["rule"] == "best_gt" and (o.instances is None or o.free):
            raise ValueError('follow rule "best_gt" scores the tracks against the annotation: it needs instances and annotations')
    o.rule = None if o.free else (GT_RULES[o.gt_rule] if isinstance(o.gt_rule, str) else o.gt_rule)
    if o.objects is not None:
        if o.tracks is None:
            raise ValueError("objects matches the annotated objects to the tracks: it needs tracks")
        if o.free:
            raise ValueError("objects scores the tracks against multi-object annotations: it needs annotations")
        o.objects = object_params(o.objects)
        o.object_rule = OBJECT_RULES.get(o.gt_rule, ObjectRule()) if isinstance(o.gt_rule, str) else ObjectRule()


def _dump_json(content, *path):
    import json
    os.makedirs(os.path.join(*path[:-1]), exist_ok=True)
    with open(os.path.join(*path), "w") as fh:
        json.dump(content, fh, indent=1)


def _score_batch(o, s, gt, pred, j, f):
    """J / F of the batch whose first frame is the category's frame s, per distinct frame shape, into j / f."""
    shapes = [tuple(int(v) for v in hw) for hw in gt.hw]
    for shape in sorted(set(shapes)):
        idx = [i for i, sh in enumerate(shapes) if sh == shape]
        j[[s + i for i in idx]], f[[s + i for i in idx]] = o.score(gt.stack(idx), pred.stack(idx), o.bound_th)


def _draw_batch(o, frames, pred, inst, det, trk):
    """The batch's overlays: every tracked component in its track's colour (inst given and instances["overlay"]), or the final mask
    `pred`; then the boxes, when asked."""
    drawn = o.draw_instances(frames, inst, o.overlay) if inst is not None and o.instances["overlay"] else o.draw(frames, pred, o.overlay)
    if o.boxes is not None:
        drawn = o.draw_boxes(drawn, det, o.boxes) if trk is None else o.draw_track_boxes(drawn, det, trk, o.boxes)
    return drawn


def _write_batch(o, cat, s, stems, gt, res, pred, inst, drawn, fg):
    """The files of a batch's frames: with pred, <stem>.png and result_<k>.mat (and, annotation-free, the frame's share of foreground
    into fg); with inst, the instance map; with drawn, the overlay."""
    import scipy.io as sio
    from PIL import Image
    od = os.path.join(o.out_dir, cat)
    for i, stem in enumerate(stems):
        if pred is not None:
            binm = _host(pred.binary_sample(i)).astype(np.uint8)
            Image.fromarray(binm * np.uint8(255), "L").save(os.path.join(od, stem + ".png"))
            mat = {"mask": binm, "soft_mask": _host(res.soft(i)).astype(np.float32)}
            if o.free:
                fg[s + i] = int(np.count_nonzero(binm)) / int(binm.size)
            else:
                mat["gt_mask"] = _host(gt.sample(i)).astype(np.uint8)
            sio.savemat(os.path.join(od, "result_{}.mat".format(s + i + 1)), mat)
        if inst is not None:
            im = Image.fromarray(np.ascontiguousarray(_host(inst.sample(i)), dtype=np.uint8), "P")
            im.putpalette(INSTANCE_PALETTE_BYTES)
            im.save(os.path.join(o.out_dir, "instances", cat, stem + ".png"))
        if drawn is not None:
            Image.fromarray(np.ascontiguousarray(_host(drawn.sample(i)), dtype=np.uint8), "RGB").save(
                os.path.join(o.out_dir, "overlay", cat, stem + ".png"))


HELD_TRACK_DROPS = ("carry", "hist_open", "inter", "gap_inter")  # of a batch's Tracks: pass 2 reads its ids alone
HELD_RESTORED_DROPS = ("binary",)                               # of a batch's RestoredMasks: pass 2 reads its soft bytes and amax


def _held(obj, drops):
    """A shallow copy of obj with the attributes `drops` set to None where it has them: what pass 2 of `follow` does not read is not
    kept alive between the passes -- the carried frames' labels a Tracks references above all (4 bytes per pixel of up to max_gap + 1
    frames per batch).  obj itself stays as it is."""
    import copy
    c = copy.copy(obj)
    for name in drops:
        if getattr(c, name, None) is not None:
            setattr(c, name, None)
    return c


def _object_paths(o, cat, rows):
    """The object annotations of a batch's frames: the frame list's own annotation paths, or with objects["dir"]
    <dir>/<category>/<frame stem>.png -- a missing file is an IOError that names it."""
    if o.objects["dir"] is None:
        return [a for _, a in rows]
    paths = [os.path.join(o.objects["dir"], cat, os.path.splitext(os.path.basename(img))[0] + ".png") for img, _ in rows]
    for p in paths:
        if not os.path.isfile(p):
            raise IOError("objects: no object annotation {!r}".format(p))
    return paths


def _match_category(cat, records, obj, starts, o):
    """The end of a category under `objects`: match_tracks over the held host tables (obj: per frame ids, row_obj, obj_area, void pixels
    and the largest id seen), every sequence's record with its void_pixels, one warning per sequence with ids above objects["max"], and
    <out_dir>/objects/<category>.json."""
    import warnings
    seqs = match_tracks(list(records.values()), obj["ids"], obj["row_obj"], obj["area"], starts, o.skip_ends)
    lo, out = 0, []
    for seq in seqs:
        hi = lo + seq["frames"]
        void = sum(obj["void"][lo:hi])
        if any(m > o.objects["max"] for m in obj["max_id"][lo:hi]):
            warnings.warn("{}: object ids up to {} in the annotations of frames {}..{}, above objects_max = {}: those pixels count as void; "
                          "pass a larger --objects_max".format(cat, max(obj["max_id"][lo:hi]), lo + 1, hi, o.objects["max"]))
        out.append({"frames": seq["frames"], "objects": seq["objects"], "J_mean": seq["J_mean"], "void_pixels": int(void),
                    "unmatched_tracks": seq["unmatched_tracks"]})
        lo = hi
    _dump_json(out, o.out_dir, "objects", cat + ".json")
    return out


def _follow_category(cat, held, words, o, j, f, fg):
    """Pass 2 of a category under `follow`: per held batch, in this order, load gt, keep (the kept rows' masks), score, draw, draw boxes,
    write.  The frames of the overlay are read again, not held.  Returns per frame kept / (kept + dropped), 0 without foreground."""
    kept = []
    for s, rows, stems, labelled, det, trk, res in held:
        gt = None if o.free else o.load_gt([a for _, a in rows], o.rule)
        pred = o.keep(labelled, det, words[s:s + len(rows)], gt=gt)
        kept += [int(a) / (int(a) + int(b)) if int(a) + int(b) else 0.0 for a, b in pred.host()[:, :2]]
        if not o.free:
            _score_batch(o, s, gt, pred, j, f)
        drawn = None
        if o.overlay is not None and not (o.instances is not None and o.instances["overlay"]):  # (that picture was pass 1's)
            drawn = _draw_batch(o, o.load_images([img for img, _ in rows]), pred, None, det, trk)
        _write_batch(o, cat, s, stems, gt, res, pred, None, drawn, fg)
    return kept


def _restore_category(cat, entries, o):
    """One category of restore_results_dir under the resolved options `o`: its batches through the injected callables in the order load
    gt or sizes, restore, load frames, refine, select, detect, link, paint, score, draw, draw boxes, write.  Writes the category's files and
    returns its record for the summary: frames, components_mean, foreground_mean; annotated: j and f (per frame); with detections:
    detections_mean; with tracks: tracks and track_len_mean; with instances: unassigned_mean and, annotated, best_track_j.  With follow
    the loop stops after paint (pass 1: the batch's labels, detections, track ids and restored soft bytes stay on the device), choose_tracks runs
    once, and _follow_category (pass 2) scores, draws and writes the kept tracks' masks; the record gains kept_mean."""
    import re
    import scipy.io as sio
    d = os.path.join(o.results_dir, cat)
    ks = sorted(int(m.group(1)) for m in (re.fullmatch(r"result_(\d+)\.mat", f) for f in (os.listdir(d) if os.path.isdir(d) else [])) if m)
    if ks != list(range(1, len(entries) + 1)):
        raise IOError("category {!r}: {} result_<k>.mat under {!r} for {} listed frames".format(cat, len(ks), d, len(entries)))
    od = os.path.join(o.out_dir, cat)
    os.makedirs(od, exist_ok=True)
    if o.overlay is not None:
        os.makedirs(os.path.join(o.out_dir, "overlay", cat), exist_ok=True)
    if o.instances is not None:
        os.makedirs(os.path.join(o.out_dir, "instances", cat), exist_ok=True)
    j, f, nc, fg = np.empty(len(entries)), np.empty(len(entries)), np.zeros(len(entries)), np.zeros(len(entries))
    records = {}  # frame stem -> its detections, in the list's order
    tail, starts = None, []  # tracks: the previous batch's last frame; per frame, whether it starts a sequence
    motion = o.tracks is not None and "motion" in o.tracks  # the link follows the flow between the frames
    if motion and hasattr(o.motion_flow, "reset"):
        o.motion_flow.reset()  # the category's first frame has no frame before it
    row_gts, gt_area, unassigned = [], [], []  # instances, per frame: row_gt of its records, its annotated pixels, the share of value 255
    obj = {"ids": [], "row_obj": [], "area": [], "void": [], "max_id": []}  # objects, per frame: the small host tables match_tracks reads
    held, score_sums = [], []  # follow: per batch what pass 2 reads, held on the device; per frame the score_sum of its rows
    own_overlay = o.overlay is not None and (o.follow is None or (o.instances is not None and o.instances["overlay"]))  # drawn in this loop
    for s in range(0, len(entries), o.batch):
        rows = entries[s:s + o.batch]
        images = [img for img, _ in rows]
        stems = [os.path.splitext(os.path.basename(img))[0] for img in images]
        masks = []
        for k in range(s + 1, s + len(rows) + 1):
            mat = sio.loadmat(os.path.join(d, "result_{}.mat".format(k)))
            if o.mask_key not in mat:
                raise KeyError("{}: result_{}.mat has no {!r}".format(d, k, o.mask_key))
            masks.append(np.squeeze(mat[o.mask_key]).astype(np.float32))
            if masks[-1].ndim != 2 or masks[-1].shape != masks[0].shape:
                raise ValueError("{}: result_{}.mat: masks must be 2-D and of one shape".format(d, k))
        gt = None if o.free else o.load_gt([a for _, a in rows], o.rule)
        # the sizes the batch is restored to: the annotations' own layout, or the frames' headers
        sizes = np.asarray(o.load_sizes(images), dtype=np.int64).reshape(-1, 2) if o.free else getattr(gt, "layout", gt.hw)
        if o.free and len(sizes) != len(rows):
            raise ValueError("load_sizes must return one (H, W) per path")
        res = o.restore(np.stack(masks), sizes, o.crop, o.threshold)
        pred = res  # what is scored and exported as the binary mask
        frames = o.load_images(images) if o.crf is not None or own_overlay or motion else None  # read once for all of them
        if o.crf is not None:
            pred = o.refine(res, frames, o.crf)
        if o.component is not None:  # with detections: the batch's labels as well -- what the CRF left, labelled once
            pred = labelled = o.select(pred, gt=gt if o.component == "best_gt" else None, mode=o.component, connectivity=o.connectivity,
                                       **({} if o.detections is None else {"want_labels": True}))
            nc[s:s + len(rows)] = _host(pred.info)[:, 0]
        elif o.detections is not None:
            labelled = o.select(pred, mode="label", connectivity=o.connectivity, want_labels=True)
        det = trk = inst = None
        if o.detections is not None:
            det = o.detect(labelled, score=res, min_area=o.detections["min_area"], max_detections=o.detections["max_detections"])
            recs = detection_records(det, res.amax)
            if o.tracks is not None:
                more = {"max_gap": o.tracks["max_gap"]} if "max_gap" in o.tracks else {}
                if motion:  # row i: from frame i to the frame before it, the previous batch's last frame for row 0
                    more["disp"] = o.displace(o.motion_flow(frames), labelled)
                trk = o.link(labelled, det, link=[0 if s + i == 0 else 1 for i in range(len(rows))], carry=tail, min_iou=o.tracks["min_iou"],
                             **more)
                tail = trk.tail()
                recs = track_records(recs, trk)
                starts += [not v for v in trk.host()[3]]
                if o.instances is not None:
                    inst = o.paint(labelled, det, trk, gt=None if o.free else gt)
                    row_gt, stats = inst.host()
                    row_gts += [[int(v) for v in row_gt[i][:len(r)]] for i, r in enumerate(recs)]
                    gt_area += [int(v) for v in stats[:, 2]]
                    unassigned += [int(u) / (int(a) + int(u)) if int(a) + int(u) else 0.0 for a, u in stats[:, :2]]
                if o.objects is not None:
                    ann = o.load_objects(_object_paths(o, cat, rows), o.object_rule)
                    row_obj, obj_area, ostats = o.overlaps(labelled, det, ann, o.objects["max"]).host()
                    ids = trk.host()[2]
                    obj["ids"] += [[int(v) for v in ids[i][:len(r)]] for i, r in enumerate(recs)]
                    obj["row_obj"] += [[[int(v) for v in row] for row in row_obj[i][:len(r)]] for i, r in enumerate(recs)]
                    obj["area"] += [[int(v) for v in obj_area[i]] for i in range(len(rows))]
                    obj["void"] += [int(v) for v in ostats[:, 1]]
                    top = getattr(ann, "max_id", None)
                    obj["max_id"] += [0] * len(rows) if top is None else [int(v) for v in top]
                    ann = None  # no per-pixel data is held
            records.update(zip(stems, recs))
        if o.follow is not None:  # pass 1 of 2: what depends on the final binary mask waits until the category's tracks are known
            held.append((s, rows, stems, labelled, det, _held(trk, HELD_TRACK_DROPS), _held(res, HELD_RESTORED_DROPS)))
            score_sums += [[int(v) for v in det.rows(i)[:, DET_FIELDS - 1]] for i in range(len(rows))]
            drawn = _draw_batch(o, frames, None, inst, det, trk) if own_overlay else None
            _write_batch(o, cat, s, stems, None, None, None, inst, drawn, fg)
            continue
        if not o.free:
            _score_batch(o, s, gt, pred, j, f)
        drawn = None if o.overlay is None else _draw_batch(o, frames, pred, inst, det, trk)
        _write_batch(o, cat, s, stems, gt, res, pred, inst, drawn, fg)
    scores = track_gt_scores(list(records.values()), row_gts, gt_area, starts) if o.instances is not None and not o.free else None
    if o.follow is not None:  # the category's tracks are known: choose once, then pass 2 over the held batches
        gt = res = pred = frames = labelled = det = trk = inst = tail = None  # (the last batch's own objects are let go as well)
        means = [sc["gt_j_mean"] for sc in scores] if o.follow["rule"] == "best_gt" else None
        kept_ranks, followed = choose_tracks(list(records.values()), score_sums, starts, o.follow["rule"], o.follow["min_frames"], means)
        kept = _follow_category(cat, held, keep_words(kept_ranks, len(entries)), o, j, f, fg)
    rec = {"frames": len(entries), "components_mean": float(nc.mean()) if len(nc) else 0.0, "foreground_mean": float(fg.mean()) if len(fg) else 0.0}
    if not o.free:
        rec["j"], rec["f"] = j.tolist(), f.tolist()
    if o.detections is not None:
        _dump_json(records, o.out_dir, "detections", cat + ".json")
        rec["detections_mean"] = float(np.mean([len(r) for r in records.values()])) if records else 0.0
    if o.tracks is not None:
        summary = summarise_tracks(list(records), list(records.values()), starts, gaps=True if "max_gap" in o.tracks else None)
        if o.instances is not None:
            rec["unassigned_mean"] = float(np.mean(unassigned)) if unassigned else 0.0
            for seq in summary:
                if any(t["id"] >= INSTANCE_WRAP for t in seq["tracks"]):
                    seq["wrapped"] = True  # two of its tracks share a value of the map
            if not o.free:
                for seq, sc in zip(summary, scores):
                    for t in seq["tracks"]:
                        t["gt_j_mean"] = sc["gt_j_mean"][t["id"]]
                    seq["best_track"] = sc["best_track"]
                rec["best_track_j"] = float(sum(sc["frames"] * sc["best_j"] for sc in scores) / sum(sc["frames"] for sc in scores)) if scores else 0.0
        if o.follow is not None:
            rec["kept_mean"] = float(np.mean(kept)) if kept else 0.0
            for seq, ids in zip(summary, followed):
                seq["followed"] = ids
        if o.objects is not None:
            rec["objects"] = _match_category(cat, records, obj, starts, o)
            for seq, m in zip(summary, rec["objects"]):
                taken = {v["track"]: oid for oid, v in m["objects"].items() if v["track"] is not None}
                for t in seq["tracks"]:
                    t["object"] = taken.get(t["id"])
        _dump_json(summary, o.out_dir, "tracks", cat + ".json")
        lengths = [t["frames"] for seq in summary for t in seq["tracks"]]
        rec["tracks"], rec["track_len_mean"] = len(lengths), float(np.mean(lengths)) if lengths else 0.0
    return rec


def _summary(cats, o):
    """native_eval.json's content from the categories' records: the head for annotated data (bound_th, skip_ends, J / F / IoU; prints the
    DAVIS table) or for a folder of frames ("annotations": false, foreground_mean; prints a line per sequence), then what each option
    adds, once -- the key order at top level and inside a sequence is what it was."""
    from .evaluation import _davis_summary, _nanmean, _print_davis_table
    out = {"mask_key": o.mask_key, "threshold": o.threshold, "crop": o.crop}
    if o.verbose:
        print("Native resolution ({} frames, crop {}{}):".format(sum(r["frames"] for r in cats.values()), o.crop, ", no annotations" if o.free else ""))
    if o.free:
        out.update({"annotations": False, "sequences": {c: {"frames": r["frames"], "foreground_mean": r["foreground_mean"]} for c, r in cats.items()}})
        if o.verbose:
            for c, v in out["sequences"].items():
                print("  {:<24s} {:5d} frames   foreground {:.4f}".format(c, v["frames"], v["foreground_mean"]))
    else:
        per, tot = _davis_summary({c: r["j"] for c, r in cats.items()}, {c: r["f"] for c, r in cats.items()}, o.skip_ends)
        cat_iou = {c: _nanmean(r["j"]) for c, r in cats.items()}
        out.update({"bound_th": o.bound_th, "skip_ends": bool(o.skip_ends), "sequences": {c: dict(per[c], frames=cats[c]["frames"]) for c in per},
                    "J": tot["J"], "F": tot["F"], "J&F": tot["J&F"], "category_iou": cat_iou, "sequence_iou": _nanmean(list(cat_iou.values()))})
        if o.verbose:
            _print_davis_table(per, tot)
    per_sequence = []  # the records' keys every sequence gains, in the order they are written
    if o.component is not None:
        out["component"], out["connectivity"] = o.component, int(o.connectivity)
        per_sequence += ["components_mean"]
    if o.crf is not None:
        out["crf"] = o.crf
    if o.overlay is not None:
        out["overlay"] = o.overlay if o.boxes is None else dict(o.overlay, boxes=o.boxes)
    if o.detections is not None:
        out["detections"] = dict(o.detections, connectivity=int(o.connectivity))
        per_sequence += ["detections_mean"]
    if o.tracks is not None:
        out["tracks"] = {k: v for k, v in o.tracks.items() if k != "motion"}
        per_sequence += ["tracks", "track_len_mean"]
    if o.instances is not None:
        out["instances"] = o.instances
        per_sequence += ["unassigned_mean"] + ([] if o.free else ["best_track_j"])
    for c, seq in out["sequences"].items():
        seq.update((k, cats[c][k]) for k in per_sequence)
    if o.instances is not None and not o.free:
        out["best_track_J"] = _nanmean([r["best_track_j"] for r in cats.values()])
    if o.follow is not None:
        out["follow"] = o.follow
        for c, seq in out["sequences"].items():
            seq["kept_mean"] = cats[c]["kept_mean"]
    if o.tracks is not None and "motion" in o.tracks:
        out["track_motion"] = {"size": list(o.tracks["motion"]["size"])}
    if o.objects is not None:
        out["objects"] = objects_summary(o.objects, {c: r["objects"] for c, r in cats.items()})
        if o.verbose:
            for c, v in out["objects"]["sequences"].items():
                print("  {:<24s} {:3d} objects   J mean {:.4f}".format(c, sum(len(q["objects"]) for q in cats[c]["objects"]), v))
    return out


def restore_results_dir(results_dir, frame_lists, out_dir, mask_key="mask", crop=0.9, threshold=0.5, batch=16, restore=restore_masks,
                        gt_rule="DAVIS2016", load_gt=load_gt_device, score=score_device, bound_th=None, skip_ends=True, verbose=True,
                        component=None, connectivity=8, select=select_components, crf=None, load_images=load_images_device,
                        refine=crf_refine_restored, load_sizes=load_sizes_header, overlay=None, draw=draw_overlays, detections=None,
                        detect=component_boxes, draw_boxes=draw_detection_boxes, tracks=None, link=link_detections,
                        draw_track_boxes=draw_track_detection_boxes, instances=None, paint=instance_maps,
                        draw_instances=draw_instance_overlays, follow=None, keep=follow_tracks, motion_flow=None,
                        displace=flow_displacements, objects=None, load_objects=load_objects_device, overlaps=object_overlaps):
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
    tracks["motion"] (None: off; {} or {"size": (fh, fw)}, both multiples of 64, default 384 x 640: DESIGN.md 7.12) links along the
    optical flow: the frames are loaded for every batch, motion_flow(frames) (None: a native_motion.BackwardFlow of that size; its
    reset(), where it has one, is called at every category's start) returns the flow from every frame to the frame before it, float32
    [n, fh, fw, 2], displace(flow, labelled) (flow_displacements) turns it into one displacement per pixel, and link is called with
    disp= as well; the "iou" of the records is then clamped to 1 and the json gains "track_motion": {"size": [fh, fw]} after its other
    keys.  Without the key link receives no disp= and every file is what it was.
    instances (None: off; needs tracks): {} or {"overlay": bool}.  After the link every batch goes through paint(labelled, det, tracks,
    gt=the batch's annotations or None) (instance_maps: two launches per batch) and every frame's map is written to
    <out_dir>/instances/<category>/<frame stem>.png, an indexed PNG (Pillow mode "P", INSTANCE_PALETTE_BYTES) whose bytes are the map's: 0
    background, 1 + (track id mod 252) a tracked component, 255 foreground without a track -- the layout multi-object tools read.  The
    tracks of tracks/<category>.json gain "gt_j_mean" and its sequences "best_track" (track_gt_scores; annotated data only), and a
    sequence whose ids reached 252 is flagged "wrapped": true; the json gains "instances" with the parameters used, per sequence
    "unassigned_mean" (the mean over its frames of the share of foreground pixels with value 255) and, on annotated data, "best_track_j"
    (the frames-weighted mean of its sequences' best gt_j_mean) and at top level "best_track_J", the mean over the categories.  With
    instances["overlay"] (needs overlay) the overlay picture comes from draw_instances(frames, maps, overlay) in the place of draw: every
    tracked component in its track's colour (visualize.overlay_instances with the overlay's alpha, beta and edge) -- those the component
    selection removed from the exported binary mask too; the boxes are still painted on top when asked.  With None nothing of this
    runs and every file is byte for byte what it is without the argument.
    follow (None: off; needs tracks; not together with a component mode -- the two are alternative answers to the same question):
    {"rule": "mass" | "area" | "length" | "best_gt" | "all" ("mass"), "min_frames": N (1)}, {} for the defaults.  The exported binary mask
    becomes that of whole tracks, chosen per sequence once the sequence is known, so a category runs in two passes.  Pass 1 is the loop
    above up to and including paint: the detections, tracks and instance-map files (and, with instances["overlay"], the overlay) come out
    of it unchanged; J / F, <stem>.png, result_<k>.mat, foreground_mean and the overlay of the final mask wait, and every batch's labels,
    detections, track ids and restored soft bytes stay on the device (5 bytes per pixel and frame -- the frames a batch was linked against
    and its thresholded mask are let go: DESIGN.md 7.11).  choose_tracks then runs once
    per category -- a track is eligible with rows in at least min_frames frames of its sequence; "all" keeps every eligible track, the
    other rules one per sequence: the largest sum of score_sum ("mass"), of area ("area"), the most frames ("length") or the largest
    gt_j_mean ("best_gt": needs instances and annotations) -- and pass 2 takes the held batches in the order load gt, keep(labelled, det,
    words, gt=...) (follow_tracks: two launches per batch), score, draw (the frames are read again), draw boxes, write.  A frame in which
    no kept track has a row exports an empty mask.  The json gains "follow": {rule, min_frames} and per sequence "kept_mean" (the mean
    over its frames of kept / (kept + dropped) foreground pixels, 0 for a frame without foreground), the sequences of
    tracks/<category>.json "followed": [ids]; new keys come after the existing ones.  With None nothing of this runs and every file is
    byte for byte what it is without the argument.
    objects (None: off; needs tracks and annotations -- each missing one is a ValueError that names it): {"max": O (16; 1..32), "dir": D
    (None)}, {} for the defaults.  After the link every batch's object annotations are read as ids, not binarised (load_objects(paths,
    rule): load_objects_device -- a mode-"P" PNG gives its palette indices, a mode-"L" image its grey values) from the frame list's own
    annotation paths, or with dir from <dir>/<category>/<frame stem>.png (a missing file is an IOError that names it), and go through
    overlaps(labelled, det, ids, max) (object_overlaps: two launches per batch); only its small host tables and the rows' track ids are
    kept.  At the category's end match_tracks assigns every annotated object at most one track, one-to-one, maximising the summed
    sequence-mean J over the frames the DAVIS table counts (skip_ends), and <out_dir>/objects/<category>.json holds per sequence
    {"frames", "objects": {id: {"track", "J": {mean, recall, decay}, "frames_annotated"}}, "J_mean", "void_pixels", "unmatched_tracks"};
    every track of tracks/<category>.json gains "object" (id or null) after its other keys and the json gains "objects": {"max", "J":
    {mean, recall, decay} over all objects of all sequences, "sequences": {name: J_mean}} after its other keys.  Bytes above max count as
    void_pixels; ids in max + 1..254 give one warning per sequence that suggests a larger --objects_max (255 is the void label and warns
    nothing).  The binarised annotation and everything computed from it stay as they are; with None nothing of this runs and every file
    is byte for byte what it is without the argument.
    restore / load_gt / score / select / load_images / refine / load_sizes / draw / detect / draw_boxes / link / draw_track_boxes / paint /
    draw_instances / keep / motion_flow / displace / load_objects / overlaps are injectable: the host logic runs without a GPU on numpy stand-ins."""
    o = SimpleNamespace(**locals())  # every argument under its own name: the options and the injected callables
    _resolve_options(o)
    cats = {cat: _restore_category(cat, entries, o) for cat, entries in frame_lists.items()}
    if not cats:
        raise IOError("no category to restore")
    out = _summary(cats, o)
    _dump_json(out, out_dir, "native_eval.json")
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
