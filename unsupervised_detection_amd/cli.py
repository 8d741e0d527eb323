"""Entry points with the reference's command-line flags (common_flags.py), for the three scripts that drive the hot path:

  python -m unsupervised_detection_amd.cli train --dataset DAVIS2016 --root_dir ... [--flow_ckpt ...]        (train.py)
  python -m unsupervised_detection_amd.cli test_generator --root_dir ... --ckpt_file ...                    (test_generator.py)
  python -m unsupervised_detection_amd.cli test_generator_ensemble --root_dir ... --test_save_dir ...       (test_generator_ensemble.py)
  python -m unsupervised_detection_amd.cli davis_eval --results_dir D [--mask_key pred_mask|mask|soft_mask] [--threshold T]
                                                      [--bound_th B] [--keep_ends]                          (no reference script)
  python -m unsupervised_detection_amd.cli restore_results --results_dir D --out_dir O --dataset ... --root_dir ...
                                                      [--test_partition val] [--test_temporal_shift 1] [--mask_key pred_mask|mask|soft_mask]
                                                      [--crop 0.9] [--threshold 0.5] [--keep_ends]         (crf_refine.py:84-97)
                                                      [--component none|largest|best_gt] [--connectivity 4|8]  (post_processing.py:32-35)
                                                      [--crf] [--sxy 60] [--srgb 5] [--scomp 5] [--gauss_k 0.1] [--crf_iters 50]
                                                      [--crf_radius R]                                      (crf_refine.py:65-108)
                                                      [--overlay] [--overlay_edge 2] [--overlay_alpha 0.5] [--overlay_beta 0.4]
                                                      [--overlay_colour 0,255,0] [--overlay_edge_colour 255,255,255]   (test_generator.py:101-106)
                                                      [--detections] [--det_min_area 64] [--det_max 16]     (no reference script)
                                                      [--overlay_boxes] [--overlay_box_thickness 2] [--overlay_box_colour 255,255,0]
                                                      [--tracks] [--track_min_iou 0.1] [--track_max_gap 0]
                                                      [--track_motion] [--track_motion_size 384 640]
                                                      [--instances] [--overlay_instances]
                                                      [--follow none|mass|area|length|best_gt|all] [--track_min_frames 1]
                                                      [--objects] [--objects_max 16] [--objects_dir D]
  python -m unsupervised_detection_amd.cli post_process --buffer_dir B --out_dir O [--dprefix davis_shift] [--max_shift 2]
                                                      [--sxy 25] [--srgb 5] [--scomp 5] [--gauss_k 0.1] [--crf_batch 16] [--flow_batch 8]
                                                      [--score_batch 0]
                                                      [--benchmark --dataset ... --root_dir ... [--native_sxy 60] [--component best_gt]
                                                       [--overlay ...] [--detections ...] [--overlay_boxes ...] [--tracks ...]
                                                       [--instances] [--overlay_instances] [--follow ...] [--track_min_frames N]
                                                       [--objects] [--objects_max O] [--objects_dir D]]
                                                                                                            (post_processing.py)

test_generator --davis_metrics adds the DAVIS-2016 benchmark table (J and F: mean, recall, decay) to the reference's report;
davis_eval scores a folder of <sequence>/result_<k>.mat files (what test_generator --generate_visualization and the
post-processing stages write) against their gt_mask key the same way and writes D/davis_eval.json.  restore_results brings such a
folder back to every frame's own size (the mask is the central --crop of the frame, the strip around it background), scores it there
against the untouched annotations and writes O/<sequence>/<frame>.png (0 / 255, the DAVIS tools' layout), O/<sequence>/result_<k>.mat
and O/native_eval.json; test_generator --native_resolution (with --generate_visualization --test_save_dir D) does the same for the
masks it has just saved, into D/native.  With --component largest / best_gt (both commands; default none) each restored mask is
reduced to one connected component (--connectivity 4 or 8, default 8) before it is scored and written: the largest one, or the one
whose IoU with the annotation is largest -- the "best detection candidate" of post_processing/post_processing.py:32-35.  With --crf
(both commands) the restored soft mask of every frame is first refined by the dense CRF on the untouched frame at its own size
(crf_refine.run_crf_original_resolution; --sxy / --srgb / --scomp / --gauss_k default to post_processing.py:24-28,40, --crf_radius to
ceil(3 sxy)), and the CRF's labels are what is selected from, scored and written.  The reference's whole benchmark pass is run_crf
followed by `restore_results --mask_key soft_mask --crf --component best_gt`.

post_process is the reference's post_processing/post_processing.py as one command over the buffers test_generator_ensemble wrote under
--buffer_dir (<dprefix>_<+-shift>/<sequence>/result_<k>.mat; the sequences and their lengths are read from <dprefix>_1 instead of the
reference's hard-coded DAVIS lists): buffer_to_soft_score into O/soft (all flows in calls of --flow_batch pairs, all sequences
propagated in one call), run_crf into O/crf_resized (--crf_batch frames per dense-CRF call) and, with --benchmark,
run_crf_original_resolution into O/crf_original (the CRF at --native_sxy on the untouched frames of --dataset under --root_dir, one
--component per mask); O/post_process.json holds the parameters, the training-size IoU and the benchmark table.  --crf_batch 0 /
--flow_batch 0 select the per-frame paths.  --score_batch N (default 0: a soft_score call per frame) computes the soft scores of N frames of a
sequence per call (post_processing.soft_score_batch).

The TF-specific lines of the originals (tf.train.Saver / Supervisor, `train.py:19`, `test_generator.py:45-55`) have no
counterpart; checkpoints are torch.save'd {tf_name: tensor} dicts.  --dataset picks the reader:
DAVIS2016 (data.Davis2016Reader), FBMS (datasets.FBMS59Reader), SEGTRACK (datasets.SegTrackV2Reader; --test_partition does
not apply to it, as in the reference) or FRAMES (datasets.FrameFolderReader: a plain folder of frames under --root_dir -- every
sub-directory that holds .jpg / .jpeg / .png / .bmp files is a sequence, or the folder itself is one; frames in natural order -- without
any annotation: the reference's "testing for your own video", scripts/create_data_frvideo.py + scripts/test_video.sh, as

  test_generator --dataset FRAMES --root_dir V --ckpt_file C --generate_visualization --test_save_dir D --native_resolution
                 --component largest --overlay

train runs without a validation pass and model.best; the native-resolution stage takes the frames' sizes from the image headers, scores
nothing and reports frames / foreground_mean per sequence; --component best_gt is refused; post_process reports "iou_resized": null and
keeps pred_mask as run_crf's candidate, what the reference's rule picks on its black fake annotation).  With --overlay (restore_results,
test_generator --native_resolution, post_process --benchmark; any dataset) every frame's final mask is also drawn on the untouched frame
at its own size -- blended --overlay_alpha / --overlay_beta in --overlay_colour, its contour --overlay_edge pixels wide (0..8, 0: none)
in --overlay_edge_colour -- into <out>/overlay/<sequence>/<frame>.png (visualize.overlay_native, one kernel launch per batch).  With
--detections (the same three commands) every connected component (--connectivity) of at least --det_min_area pixels of a frame's mask --
after the CRF, before --component -- is reported as a box, the largest first, at most --det_max (1..64) per frame: box [x0, y0, x1, y1],
area, centroid, score (the mean restored soft mask over the component) and root, in <out>/detections/<sequence>.json
(native_results.component_boxes).  --overlay_boxes (needs --overlay and --detections) also paints the boxes on the overlays,
--overlay_box_thickness (1..8) pixels wide in --overlay_box_colour (visualize.draw_boxes).  --tracks (needs --detections) links the
detections of consecutive frames of a sequence by mask overlap -- a box continues the box of the frame before it with which its component
shares the largest IoU, at least --track_min_iou (0.1) -- and numbers the tracks per sequence: the records gain track / prev / iou,
<out>/tracks/<sequence>.json lists every track, and --overlay_boxes paints each box in its track's colour
(native_results.link_detections, visualize.draw_track_boxes).  --track_max_gap G (needs --tracks; 0..8, default 0: off) lets a box
without a predecessor in the frame before it continue a track whose component was missing for up to G frames, by the same IoU rule
against that track's last-seen component: the object keeps its id and its colour, the records gain back, the tracks span / gaps and
the sequences bridged.  --track_motion (needs --tracks) links along the optical flow: every pixel of a frame is compared with the pixel
of the frame before it that the backward PWC flow, computed at --track_motion_size FH FW (multiples of 64, default 384 640), says it
came from, so an object that moves further than its own extent between two frames keeps its id (native_motion.flow_displacements,
DESIGN.md 7.12); native_eval.json gains track_motion.  --instances (needs --tracks) hands the tracks to the pixels: <out>/instances/<sequence>/<frame>.png is an indexed
PNG at the frame's own size in which a pixel's value names its track (0 background, 1 + id mod 252 a tracked component in its track's
colour, 255 foreground without a track), the tracks of <out>/tracks/<sequence>.json gain gt_j_mean -- the mean J of that one track
against the annotation over all frames of its sequence -- and the sequences best_track, and native_eval.json reports unassigned_mean,
best_track_j and best_track_J (native_results.instance_maps).  --overlay_instances (needs --overlay and --instances) draws the
instance map on the overlays in the place of the single mask: every tracked component in its track's colour, also those --component
removed from the exported binary mask, touching instances separated by a line of each one's colour (visualize.overlay_instances).
--follow mass|area|length|best_gt|all (needs --tracks; default none; not together with a --component mode, so post_process --benchmark
takes it with --component none) makes the exported and scored binary mask that of whole tracks, chosen without the annotation once a
sequence is known: among the tracks with boxes in at least --track_min_frames (1) frames of their sequence, the one with the largest
summed score (mass), the largest summed area, the most frames (length) or -- with --instances, on annotated data -- the largest mean J
against the annotation (best_gt), ties to the longer track, then the smaller id; all keeps every such track.  The stage then runs every
sequence in two passes, a frame in which the followed track has no box exports an empty mask, the J / F table is that of one consistently
followed object, native_eval.json gains follow and per sequence kept_mean, and the sequences of <out>/tracks/<sequence>.json gain followed
(native_results.follow_tracks).  --objects (needs --tracks and annotations; the same three commands; with or without --instances,
--follow, --track_max_gap and --track_motion) scores the tracks against multi-object annotations the way the DAVIS-2017 unsupervised
protocol judges instance ids: every annotation is read as object ids (an indexed PNG's palette indices, a grey image's values; nothing is
binarised), ids 1..--objects_max (1..32, default 16) are objects and anything above is void, from the dataset's own annotation files or,
with --objects_dir D, from D/<sequence>/<frame>.png; every annotated object is matched to at most one track over its sequence,
one-to-one, so that the summed mean J is largest, <out>/objects/<sequence>.json holds per object its track and J mean / recall / decay,
the tracks of <out>/tracks/<sequence>.json gain object, and native_eval.json gains objects with the mean over all objects of all
sequences (native_results.object_overlaps, native_results.match_tracks).
Like the
reference, a missing dataset, an unsupported --dataset or a missing
--flow_ckpt is an IOError; --synthetic opts in to synthetic DAVIS-shaped pairs and seeded random weights (benchmarks, smoke
runs)."""
from __future__ import annotations

import os
import sys

import numpy as np


def _sources(flags, mode):
    """data_source / val_source of the learner from the dataset flags (adversarial_learner.py:30-70, 459-477, 537-552)."""
    if getattr(flags, "synthetic", False):
        return
    dataset_sources(flags, mode)


def _reader(flags, rank, world):
    """The reader --dataset names, with the shard of this rank; a missing dataset root is an IOError."""
    from . import data, datasets
    root = getattr(flags, "root_dir", "")
    kw = dict(max_temporal_len=flags.max_temporal_len, min_temporal_len=flags.min_temporal_len, num_threads=flags.num_threads,
              seed=8964, shard=(rank, world))
    if flags.dataset == "DAVIS2016":
        if not (root and os.path.isfile(os.path.join(root, "ImageSets", "480p", "val.txt"))):
            raise IOError("Partition file not found under --root_dir {!r} (DAVIS2016 layout: ImageSets/480p/val.txt)".format(root))
        return data.Davis2016Reader(root, **kw)
    if flags.dataset == "FBMS":
        if not (root and os.path.isdir(root)):
            raise IOError("Directory {!r} not found (FBMS layout: Trainingset/ and Testset/)".format(root))
        return datasets.FBMS59Reader(root, **kw)
    if flags.dataset == "SEGTRACK":
        if not (root and os.path.isfile(os.path.join(root, "ImageSets", "all.txt"))):
            raise IOError("Division file not found under --root_dir {!r} (SegTrackV2 layout: ImageSets/all.txt)".format(root))
        return datasets.SegTrackV2Reader(root, **kw)
    if flags.dataset == "FRAMES":
        if not (root and os.path.isdir(root)):
            raise IOError("Directory {!r} not found (FRAMES layout: <sequence>/<frame>.jpg|.jpeg|.png|.bmp, or the frames themselves)".format(root))
        return datasets.FrameFolderReader(root, **kw)
    raise IOError("Dataset should be DAVIS2016 / FBMS / SEGTRACK / FRAMES")


class _Listed(list):
    """A one-pass test reader read out once: `n` batches (AdversarialLearner.setup_inference counts test samples by it)."""

    def __init__(self, batches):
        super().__init__(batches)
        self.n = len(self)


def dataset_sources(flags, mode):
    """_sources without the --synthetic short cut: the readers of --dataset under --root_dir for `mode` (train / test /
    ensemble), on flags.data_source (and flags.val_source when training)."""
    import torch.distributed as dist
    ddp = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
    # data-parallel training: one shuffle shared by the ranks, each takes its own rows of every global batch (disjoint pairs;
    # an epoch = the pair table once = num_samples_train / (batch_size * world) steps, see AdversarialLearner.train)
    rd = _reader(flags, rank, world)
    frames = flags.dataset == "FRAMES"  # a folder of frames: no annotation, hence no validation IoU
    segtrack = flags.dataset == "SEGTRACK" or frames  # no partition argument (segtrackv2_data_utils.py)
    part = lambda p: {} if segtrack else {"partition": p}
    if mode == "train":
        flags.data_source = rd.image_inputs(batch_size=flags.batch_size, train_crop=flags.train_crop, **part(flags.train_partition))

        class _Val:
            def __iter__(self_inner):
                # adversarial_learner.py:34-37: the validation reader uses test_temporal_shift / test_crop
                return iter(rd.test_inputs(batch_size=flags.batch_size, t_len=flags.test_temporal_shift, test_crop=flags.test_crop,
                                           **part("val")))
        flags.val_source = None if frames else _Val()  # None: no validation pass and no model.best, the periodic checkpoints stay
    elif mode == "test":
        flags.data_source = _Listed(rd.test_inputs(batch_size=flags.batch_size, t_len=flags.test_temporal_shift, with_fname=True,
                                                   test_crop=flags.test_crop, **part(flags.test_partition)))
    else:
        if flags.dataset == "FBMS":
            assert "FBMS" in flags.root_dir  # adversarial_learner.py:542
        flags.data_source = _Listed(rd.test_inputs(batch_size=1, t_len=flags.test_temporal_shift, with_fname=True, test_crop=1.0,
                                                   **part(flags.test_partition)))


DATASETS = ("DAVIS2016", "FBMS", "SEGTRACK", "FRAMES")


def _add_overlay_arguments(ap):
    """--overlay and its parameters (visualize.overlay_native), for the parsers that do not take config._DEFS."""
    ap.add_argument("--overlay", action="store_true", help="also draw every final mask on its frame: <out>/overlay/<sequence>/<frame>.png")
    ap.add_argument("--overlay_edge", type=int, default=2, help="half-width of the contour line in pixels, 0..8; 0: no contour")
    ap.add_argument("--overlay_alpha", type=float, default=0.5)
    ap.add_argument("--overlay_beta", type=float, default=0.4)
    ap.add_argument("--overlay_colour", default="0,255,0", help="r,g,b of the mask")
    ap.add_argument("--overlay_edge_colour", default="255,255,255", help="r,g,b of the contour")
    ap.add_argument("--detections", action="store_true", help="report every connected component as a box: <out>/detections/<sequence>.json")
    ap.add_argument("--det_min_area", type=int, default=64, help="the smallest component reported, in pixels")
    ap.add_argument("--det_max", type=int, default=16, help="detections per frame, the largest first (1..64)")
    ap.add_argument("--overlay_boxes", action="store_true", help="with --overlay and --detections: also paint the boxes on the overlays")
    ap.add_argument("--overlay_box_thickness", type=int, default=2, help="width of a box's line in pixels, 1..8 (inward)")
    ap.add_argument("--overlay_box_colour", default="255,255,0", help="r,g,b of the boxes")
    ap.add_argument("--tracks", action="store_true", help="with --detections: link the boxes of consecutive frames: <out>/tracks/<sequence>.json")
    ap.add_argument("--track_min_iou", type=float, default=0.1, help="the smallest mask IoU that links two boxes")
    ap.add_argument("--track_max_gap", type=int, default=0,
                    help="with --tracks: a box may continue a track whose component was missing for up to this many frames (0..8; 0: none)")
    ap.add_argument("--track_motion", action="store_true",
                    help="with --tracks: link along the optical flow between the frames, so that fast small objects keep their id")
    ap.add_argument("--track_motion_size", type=int, nargs=2, default=(384, 640), metavar=("FH", "FW"),
                    help="with --track_motion: the size the flow is computed at, two multiples of 64")
    ap.add_argument("--instances", action="store_true",
                    help="with --tracks: write every frame's instance map, <out>/instances/<sequence>/<frame>.png, and score every track")
    ap.add_argument("--overlay_instances", action="store_true",
                    help="with --overlay and --instances: draw every tracked component in its track's colour on the overlays, in the place of "
                         "the single mask -- the components --component removed from the exported binary mask too")
    ap.add_argument("--follow", default="none", choices=("none", "mass", "area", "length", "best_gt", "all"),
                    help="with --tracks: export and score the masks of whole tracks, one per sequence by its summed score (mass), summed "
                         "area, length or mean J against the annotation (best_gt), or all of them; not together with --component")
    ap.add_argument("--track_min_frames", type=int, default=1, help="with --follow: only tracks with boxes in at least this many frames")
    ap.add_argument("--objects", action="store_true",
                    help="with --tracks: match every object of a multi-object annotation to one track and report J per object: "
                         "<out>/objects/<sequence>.json")
    ap.add_argument("--objects_max", type=int, default=16, help="with --objects: annotation values 1..this are objects (1..32), above it void")
    ap.add_argument("--objects_dir", default=None,
                    help="with --objects: read the object ids from <objects_dir>/<sequence>/<frame>.png, not from the dataset's annotations")


def _overlay(flags):
    """--overlay and its parameters as restore_results_dir takes them: None without --overlay; with --overlay_boxes also "boxes".  A bad
    value, or --overlay_boxes without --overlay and --detections, is a SystemExit."""
    boxes = getattr(flags, "overlay_boxes", False)
    if boxes and not (getattr(flags, "overlay", False) and getattr(flags, "detections", False)):
        raise SystemExit("--overlay_boxes paints the detections on the overlays: it needs --overlay and --detections")
    if not getattr(flags, "overlay", False):
        return None
    from .visualize import box_params, overlay_params
    try:
        colour, edge_colour = ([int(v) for v in str(c).split(",")] for c in (flags.overlay_colour, flags.overlay_edge_colour))
        p = overlay_params({"alpha": flags.overlay_alpha, "beta": flags.overlay_beta, "colour": colour, "edge": flags.overlay_edge,
                            "edge_colour": edge_colour})
    except ValueError as e:
        raise SystemExit("--overlay: {} (--overlay_colour / --overlay_edge_colour are r,g,b)".format(e))
    if boxes:
        try:
            p["boxes"] = box_params({"thickness": flags.overlay_box_thickness,
                                     "colour": [int(v) for v in str(flags.overlay_box_colour).split(",")]})
        except ValueError as e:
            raise SystemExit("--overlay_boxes: {} (--overlay_box_colour is r,g,b)".format(e))
    return p


def _detections(flags):
    """--detections and its parameters as restore_results_dir takes them: None without --detections.  A bad value is a SystemExit."""
    if not getattr(flags, "detections", False):
        return None
    from .native_detections import detection_params
    try:
        return detection_params({"min_area": flags.det_min_area, "max_detections": flags.det_max})
    except ValueError as e:
        raise SystemExit("--detections: {} (--det_min_area / --det_max)".format(e))


def _tracks(flags):
    """--tracks and its parameter as restore_results_dir takes them: None without --tracks.  --tracks without --detections, or a bad
    value, is a SystemExit."""
    gap, motion = getattr(flags, "track_max_gap", 0), getattr(flags, "track_motion", False)
    size = tuple(getattr(flags, "track_motion_size", (384, 640)))
    if not getattr(flags, "tracks", False):
        if gap:
            raise SystemExit("--track_max_gap bridges the frames in which a track's component is missing: it needs --tracks")
        if motion or size != (384, 640):
            raise SystemExit("--track_motion links the detections along the optical flow: it needs --tracks")
        return None
    if not getattr(flags, "detections", False):
        raise SystemExit("--tracks links the detections of consecutive frames: it needs --detections")
    if size != (384, 640) and not motion:
        raise SystemExit("--track_motion_size is the size the flow of --track_motion is computed at: it needs --track_motion")
    from .native_tracks import track_params
    try:
        return track_params(dict({"min_iou": flags.track_min_iou, "max_gap": gap}, **({"motion": {"size": size}} if motion else {})))
    except ValueError as e:
        raise SystemExit("--tracks: {} (--track_min_iou / --track_max_gap / --track_motion_size)".format(e))


def _instances(flags):
    """--instances and --overlay_instances as restore_results_dir takes them: None without --instances.  --instances without --tracks, or
    --overlay_instances without --overlay and --instances, is a SystemExit."""
    drawn = getattr(flags, "overlay_instances", False)
    if drawn and not (getattr(flags, "overlay", False) and getattr(flags, "instances", False)):
        raise SystemExit("--overlay_instances draws the instance maps on the overlays: it needs --overlay and --instances")
    if not getattr(flags, "instances", False):
        return None
    if not getattr(flags, "tracks", False):
        raise SystemExit("--instances paints the tracks into per-frame instance maps: it needs --tracks")
    from .native_instances import instance_params
    return instance_params({"overlay": bool(drawn)})


def _follow(flags):
    """--follow and --track_min_frames as restore_results_dir takes them: None for "none".  --follow without --tracks, together with a
    --component mode, best_gt without --instances or on --dataset FRAMES, --track_min_frames without --follow, or a bad value, is a
    SystemExit."""
    rule, frames = getattr(flags, "follow", "none"), getattr(flags, "track_min_frames", 1)
    if rule in (None, "none"):
        if frames != 1:
            raise SystemExit("--track_min_frames drops the short tracks from what --follow keeps: it needs --follow")
        return None
    if not getattr(flags, "tracks", False):
        raise SystemExit("--follow exports the masks of whole tracks: it needs --tracks")
    if _component(flags) is not None:
        raise SystemExit("--follow and --component are alternative answers to which component is the mask: pass --component none")
    if rule == "best_gt" and not getattr(flags, "instances", False):
        raise SystemExit("--follow best_gt scores the tracks against the annotation: it needs --instances")
    if rule == "best_gt" and getattr(flags, "dataset", None) == "FRAMES":
        raise SystemExit("--dataset FRAMES has no annotations: pass --follow mass|area|length|all (best_gt needs them)")
    from .native_follow import follow_params
    try:
        return follow_params({"rule": rule, "min_frames": frames})
    except ValueError as e:
        raise SystemExit("--follow: {} (--track_min_frames)".format(e))


def _objects(flags):
    """--objects, --objects_max and --objects_dir as restore_results_dir takes them: None without --objects.  --objects without --tracks or
    on --dataset FRAMES, --objects_max / --objects_dir without --objects, or a bad value, is a SystemExit."""
    most, folder = getattr(flags, "objects_max", 16), getattr(flags, "objects_dir", None)
    if not getattr(flags, "objects", False):
        if most != 16 or folder:
            raise SystemExit("--objects_max / --objects_dir say how --objects reads the annotations: they need --objects")
        return None
    if not getattr(flags, "tracks", False):
        raise SystemExit("--objects matches the annotated objects to the tracks: it needs --tracks")
    if getattr(flags, "dataset", None) == "FRAMES":
        raise SystemExit("--dataset FRAMES has no annotations: --objects needs them")
    from .native_objects import object_params
    try:
        return object_params({"max": most, "dir": folder or None})
    except ValueError as e:
        raise SystemExit("--objects: {} (--objects_max / --objects_dir)".format(e))


def check_frames_component(flags):
    """A folder of frames has no annotation to pick the best component by."""
    if getattr(flags, "dataset", None) == "FRAMES" and getattr(flags, "component", "none") == "best_gt":
        raise SystemExit("--dataset FRAMES has no annotations: pass --component largest|none (best_gt needs them)")


def parse_davis_eval_args(argv):
    """The arguments of the davis_eval subcommand."""
    import argparse
    ap = argparse.ArgumentParser(prog="davis_eval")
    ap.add_argument("--results_dir", required=True)
    ap.add_argument("--mask_key", default="pred_mask", choices=("pred_mask", "mask", "soft_mask"))
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--bound_th", type=float, default=0.008)
    ap.add_argument("--keep_ends", action="store_true", help="score the first and last frame of a sequence too")
    return ap.parse_args(argv)


def parse_restore_results_args(argv):
    """The arguments of the restore_results subcommand: its own and, for the reader of --dataset, the flags of common_flags.py."""
    import argparse
    from .config import default_flags
    ap = argparse.ArgumentParser(prog="restore_results")
    ap.add_argument("--results_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--dataset", default="DAVIS2016", choices=DATASETS)
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--test_partition", default="val")
    ap.add_argument("--test_temporal_shift", type=int, default=1)
    ap.add_argument("--mask_key", default="mask", choices=("pred_mask", "mask", "soft_mask"))
    ap.add_argument("--crop", type=float, default=0.9)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--keep_ends", action="store_true", help="score the first and last frame of a sequence too")
    ap.add_argument("--component", default="none", choices=("none", "largest", "best_gt"),
                    help="keep one connected component of each restored mask: the largest, or the best IoU with the annotation")
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    ap.add_argument("--crf", action="store_true", help="refine every restored mask by the dense CRF on the frame at its own size")
    ap.add_argument("--sxy", type=float, default=60.0)
    ap.add_argument("--srgb", type=float, default=5.0)
    ap.add_argument("--scomp", type=float, default=5.0)
    ap.add_argument("--gauss_k", type=float, default=0.1)
    ap.add_argument("--crf_iters", type=int, default=50)
    ap.add_argument("--crf_radius", type=int, default=0, help="window radius of the CRF's kernel; 0: ceil(3 sxy)")
    _add_overlay_arguments(ap)
    a = ap.parse_args(argv)
    flags = default_flags()
    for k, v in vars(a).items():
        setattr(flags, k, v)
    check_frames_component(flags)
    _overlay(flags)
    _detections(flags)
    _tracks(flags)
    _instances(flags)
    _follow(flags)
    _objects(flags)
    return flags


def parse_post_process_args(argv):
    """The arguments of the post_process subcommand; the defaults are the constants of post_processing/post_processing.py:24-27,40."""
    import argparse
    from .config import default_flags
    ap = argparse.ArgumentParser(prog="post_process")
    ap.add_argument("--buffer_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--dprefix", default="davis_shift")
    ap.add_argument("--max_shift", type=int, default=2)
    ap.add_argument("--sxy", type=float, default=25.0)
    ap.add_argument("--srgb", type=float, default=5.0)
    ap.add_argument("--scomp", type=float, default=5.0)
    ap.add_argument("--gauss_k", type=float, default=0.1)
    ap.add_argument("--crf_batch", type=int, default=16, help="frames per dense-CRF call; 0: a frame at a time")
    ap.add_argument("--flow_batch", type=int, default=8, help="frame pairs per flow-network call; 0: a pair at a time, a step at a time")
    ap.add_argument("--score_batch", type=int, default=0, help="frames per soft-score call; 0: a frame at a time")
    ap.add_argument("--benchmark", action="store_true", help="also refine and score at every frame's own size")
    ap.add_argument("--native_sxy", type=float, default=60.0)
    ap.add_argument("--dataset", default="DAVIS2016", choices=DATASETS)
    ap.add_argument("--root_dir", default="")
    ap.add_argument("--test_partition", default="val")
    ap.add_argument("--test_temporal_shift", type=int, default=1)
    ap.add_argument("--component", default="best_gt", choices=("none", "largest", "best_gt"))
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    _add_overlay_arguments(ap)
    a = ap.parse_args(argv)
    if a.benchmark and not a.root_dir:
        ap.error("--benchmark needs --root_dir (and --dataset)")
    if a.max_shift < 1 or a.crf_batch < 0 or a.flow_batch < 0 or a.score_batch < 0:
        ap.error("--max_shift >= 1, --crf_batch >= 0, --flow_batch >= 0 and --score_batch >= 0")
    flags = default_flags()
    for k, v in vars(a).items():
        setattr(flags, k, v)
    if a.benchmark:
        check_frames_component(flags)
        _overlay(flags)
        _detections(flags)
        _tracks(flags)
        _instances(flags)
        _follow(flags)
        _objects(flags)
    return flags


def discover_sequences(buffer_dir, dprefix="davis_shift"):
    """(names, lengths) of the sequences under <buffer_dir>/<dprefix>_1: every folder that holds result_1.mat .. result_<n>.mat, by name;
    a folder whose numbering has a hole is an IOError (the frames are walked as 1..n)."""
    root = os.path.join(buffer_dir, "%s_1" % dprefix)
    if not os.path.isdir(root):
        raise IOError("Directory {!r} not found (the buffers of test_generator_ensemble at shift 1)".format(root))
    names, lengths = [], []
    for name in sorted(os.listdir(root)):
        d = os.path.join(root, name)
        if not os.path.isdir(d):
            continue
        ks = sorted(int(f[len("result_"):-len(".mat")]) for f in os.listdir(d)
                    if f.startswith("result_") and f.endswith(".mat") and f[len("result_"):-len(".mat")].isdigit())
        if not ks:
            continue
        if ks != list(range(1, len(ks) + 1)):
            raise IOError("{!r}: result_<k>.mat must be numbered 1..{} without a hole".format(d, len(ks)))
        names.append(name)
        lengths.append(len(ks))
    if not names:
        raise IOError("No <sequence>/result_<k>.mat under {!r}".format(root))
    return names, lengths


def post_process(a):
    """post_processing/post_processing.py on parse_post_process_args' flags; returns (and writes to O/post_process.json) the report."""
    import json
    from . import post_processing as pp
    names, lengths = discover_sequences(a.buffer_dir, a.dprefix)
    soft, resized, original = (os.path.join(a.out_dir, d) for d in ("soft", "crf_resized", "crf_original"))
    score = {"score_batch": a.score_batch} if a.score_batch > 0 else {}  # 0: the keyword is not passed at all (the per-frame path)
    pp.buffer_to_soft_score(a.buffer_dir, soft, names, lengths, max_shift=a.max_shift, dprefix=a.dprefix, flow_batch=a.flow_batch or None, **score)
    with np.errstate(**({"divide": "ignore", "invalid": "ignore"} if a.dataset == "FRAMES" else {})):  # no annotation: run_crf's IoU is 0 / 0
        iou = pp.run_crf(soft, a.sxy, a.srgb, a.scomp, a.gauss_k, out_path=resized, batch=a.crf_batch or None)
    report = {"sequences": dict(zip(names, lengths)), "sxy": a.sxy, "srgb": a.srgb, "scomp": a.scomp, "gauss_k": a.gauss_k,
              "crf_batch": a.crf_batch, "flow_batch": a.flow_batch,
              "iou_resized": None if a.dataset == "FRAMES" else float(iou)}  # no annotations: nothing to score the resized masks against
    report.update(score)
    if a.benchmark:
        from .native_results import frame_lists_from_reader
        report["native_sxy"] = a.native_sxy
        overlay, detections = _overlay(a), _detections(a)
        more = {} if overlay is None else {"overlay": overlay}
        if detections is not None:
            more.update(detections=detections, connectivity=a.connectivity)
        if _tracks(a) is not None:
            more.update(tracks=_tracks(a))
        if _instances(a) is not None:
            more.update(instances=_instances(a))
        if _follow(a) is not None:
            more.update(follow=_follow(a))
        if _objects(a) is not None:
            more.update(objects=_objects(a))
        report["benchmark"] = pp.run_crf_original_resolution(resized, frame_lists_from_reader(a), a.native_sxy, a.srgb, a.scomp, a.gauss_k,
                                                             out_path=original, component=_component(a), gt_rule=a.dataset, **more)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "post_process.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def _component(flags):
    """--component as restore_results_dir takes it: None for "none"."""
    c = getattr(flags, "component", "none")
    return None if c in (None, "none") else c


def _crf(flags):
    """--crf and its parameters as restore_results_dir takes them: None without --crf."""
    if not getattr(flags, "crf", False):
        return None
    return {"sxy": flags.sxy, "srgb": flags.srgb, "compat": flags.scomp, "gauss_k": flags.gauss_k, "iters": flags.crf_iters,
            "radius": flags.crf_radius if flags.crf_radius > 0 else None}


def check_native_flags(flags):
    """--native_resolution works on the masks test_generator saves: it needs --generate_visualization --test_save_dir and a dataset."""
    if getattr(flags, "native_resolution", False) and not (flags.generate_visualization and flags.test_save_dir):
        raise SystemExit("--native_resolution requires --generate_visualization --test_save_dir D")
    if getattr(flags, "native_resolution", False) and getattr(flags, "synthetic", False):
        raise SystemExit("--native_resolution needs the annotations of a dataset (not --synthetic)")
    if getattr(flags, "component", "none") not in ("none", "largest", "best_gt") or getattr(flags, "connectivity", 8) not in (4, 8):
        raise SystemExit("--component is none, largest or best_gt and --connectivity 4 or 8")
    if getattr(flags, "native_resolution", False):
        check_frames_component(flags)
        _overlay(flags)
        _detections(flags)
        _tracks(flags)
        _instances(flags)
        _follow(flags)
        _objects(flags)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in ("train", "test_generator", "test_generator_ensemble", "davis_eval", "restore_results", "post_process"):
        print(__doc__)
        return 2
    if argv[0] == "post_process":
        post_process(parse_post_process_args(argv[1:]))
        return 0
    if argv[0] == "restore_results":
        a = parse_restore_results_args(argv[1:])
        from .native_results import frame_lists_from_reader, restore_results_dir
        restore_results_dir(a.results_dir, frame_lists_from_reader(a), a.out_dir, mask_key=a.mask_key, crop=a.crop, threshold=a.threshold,
                            batch=a.batch, gt_rule=a.dataset, skip_ends=not a.keep_ends, component=_component(a), connectivity=a.connectivity,
                            crf=_crf(a), overlay=_overlay(a), detections=_detections(a), tracks=_tracks(a), instances=_instances(a), follow=_follow(a),
                            objects=_objects(a))
        return 0
    if argv[0] == "davis_eval":
        a = parse_davis_eval_args(argv[1:])
        from .evaluation import evaluate_results_dir
        evaluate_results_dir(a.results_dir, a.mask_key, a.threshold, a.bound_th, skip_ends=not a.keep_ends)
        return 0
    from .config import parse_flags
    from .learner import AdversarialLearner
    cmd, flags = argv[0], parse_flags(argv[1:])
    if cmd == "test_generator":
        check_native_flags(flags)
    np.random.seed(8964)  # train.py:18
    learner = AdversarialLearner()
    if cmd == "train":
        _sources(flags, "train")
        learner.train(flags)
        return 0
    if cmd == "test_generator":
        _sources(flags, "test")  # --ckpt_file is restored by the learner (every network the checkpoint holds)
        learner.setup_inference(flags, aug_test=False)
        from .evaluation import evaluate_masks
        evaluate_masks(learner, save_dir=flags.test_save_dir if flags.generate_visualization else None,
                       davis_metrics=flags.davis_metrics)
        if flags.native_resolution:
            from .native_results import frame_lists_from_reader, restore_results_dir
            restore_results_dir(flags.test_save_dir, frame_lists_from_reader(flags), os.path.join(flags.test_save_dir, "native"),
                                mask_key="pred_mask", crop=flags.test_crop, gt_rule=flags.dataset, component=_component(flags),
                                connectivity=flags.connectivity, crf=_crf(flags), overlay=_overlay(flags),
                                detections=_detections(flags), tracks=_tracks(flags), instances=_instances(flags),
                                follow=_follow(flags), objects=_objects(flags))
        return 0
    _sources(flags, "ensemble")
    learner.setup_inference(flags, aug_test=True)
    from .evaluation import evaluate_ensemble
    evaluate_ensemble(learner, save_dir=flags.test_save_dir if flags.generate_visualization else None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
