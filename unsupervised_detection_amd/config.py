"""The flags of common_flags.py:6-54 (same names, same defaults) without python-gflags (not installed here).
`FLAGS` can be passed as `config` wherever the reference passes gflags.FLAGS."""
import argparse
from types import SimpleNamespace

_DEFS = [
    ("img_width", int, 384), ("img_height", int, 192), ("batch_size", int, 16), ("beta1", float, 0.9),
    ("flow_normalizer", float, 80.0), ("max_epochs", int, 40), ("num_samples_train", int, 5000), ("train_crop", float, 0.9),
    ("max_temporal_len", int, 2), ("min_temporal_len", int, 1), ("cbn", float, 0.5), ("epsilon", float, 75.0),
    ("iters_rec", int, 1), ("iters_gen", int, 3), ("num_threads", int, 6), ("resume_train", bool, False),
    ("root_dir", str, "/your/path/to/DAVIS_2016"), ("train_partition", str, "trainval"), ("dataset", str, "DAVIS2016"),
    ("recover_ckpt", str, ""), ("flow_ckpt", str, ""), ("full_model_ckpt", str, ""), ("checkpoint_dir", str, ""),
    ("summary_freq", int, 30), ("save_freq", int, 5), ("generate_visualization", bool, False), ("test_crop", float, 0.9),
    ("test_temporal_shift", int, 1), ("ckpt_file", str, ""), ("test_partition", str, "val"), ("test_save_dir", str, ""),
    # not a reference flag: also write checkpoints in tf.train.Saver format under the reference's variable names
    ("save_tf_checkpoint", bool, False),
    # not a reference flag: explicit opt-in to synthetic DAVIS-shaped pairs / seeded random weights when no dataset or checkpoint
    # is given (the reference raises IOError in those cases, adversarial_learner.py:66-67,339-343; so does this port without it)
    ("synthetic", bool, False),
    # not a reference flag: BASELINE.json configs[4] -- fp16 multiplication (fp32 accumulation) in the convolution GEMMs
    ("conv_fp16", bool, False),
    # not a reference flag: the one-off kernel autotune of the training plan at start-up (~10 s; rank 0 tunes, the other ranks of a
    # data-parallel job load its configurations).  Untuned plans run on the built-in tile heuristics (12.3 instead of 10.9 ms per step at the benchmark shape).
    ("autotune", bool, True),
    # not a reference flag: directory of the training summaries (visualize.SummaryWriter: scalars.jsonl, images/, histograms/ every
    # summary_freq steps -- the reference writes TensorBoard events into checkpoint_dir); "" = off
    ("summary_dir", str, ""),
    # not a reference flag: test_generator also reports the DAVIS-2016 benchmark measures (J and F: mean, recall, decay), which the
    # reference leaves to the external DAVIS toolkit
    ("davis_metrics", bool, False),
    # not a reference flag: after test_generator --generate_visualization --test_save_dir D, restore the saved masks to every frame's
    # own size (test_crop pasted into a zero canvas), score them there and export them under D/native (native_results.py)
    ("native_resolution", bool, False),
    # not reference flags: with --native_resolution, keep one connected component of every restored mask before it is scored and
    # exported -- none | largest | best_gt (the best IoU with the annotation: post_processing.py:32-35) -- under 4- or 8-connectivity
    ("component", str, "none"),
    ("connectivity", int, 8),
    # not reference flags: with --native_resolution, --crf runs the reference's full-resolution pass on the restored masks
    # (crf_refine.run_crf_original_resolution; defaults of post_processing.py:24-28,40): the dense CRF on every frame at its own size;
    # crf_radius 0 = ceil(3 sxy)
    ("crf", bool, False),
    ("sxy", float, 60.0),
    ("srgb", float, 5.0),
    ("scomp", float, 5.0),
    ("gauss_k", float, 0.1),
    ("crf_iters", int, 50),
    ("crf_radius", int, 0),
    # not reference flags: with --native_resolution, --overlay also draws every final mask on its frame at the frame's own size
    # (visualize.overlay_native) into D/native/overlay: the mask blended overlay_alpha / overlay_beta in overlay_colour (r,g,b), its
    # contour overlay_edge pixels wide (0..8; 0: none) in overlay_edge_colour
    ("overlay", bool, False),
    ("overlay_edge", int, 2),
    ("overlay_alpha", float, 0.5),
    ("overlay_beta", float, 0.4),
    ("overlay_colour", str, "0,255,0"),
    ("overlay_edge_colour", str, "255,255,255"),
    # not reference flags: with --native_resolution, --detections reports every connected component (--connectivity) of at least
    # det_min_area pixels as a box, at most det_max (1..64) per frame, into D/native/detections/<sequence>.json
    # (native_results.component_boxes); --overlay_boxes (with --overlay) paints them on the overlays, overlay_box_thickness (1..8) pixels
    # wide in overlay_box_colour (r,g,b)
    ("detections", bool, False),
    ("det_min_area", int, 64),
    ("det_max", int, 16),
    ("overlay_boxes", bool, False),
    ("overlay_box_thickness", int, 2),
    ("overlay_box_colour", str, "255,255,0"),
    # not reference flags: with --native_resolution and --detections, --tracks links the boxes of consecutive frames by mask overlap (IoU
    # at least track_min_iou) into D/native/tracks/<sequence>.json (native_results.link_detections)
    ("tracks", bool, False),
    ("track_min_iou", float, 0.1),
    # ... and a box may continue a track whose component was missing for up to track_max_gap frames (0..8, 0: off)
    ("track_max_gap", int, 0),
    # ... and track_motion links along the optical flow between the frames, computed at track_motion_size (fh fw, multiples of 64;
    # DESIGN.md 7.12): an object that moves further than its own extent between two frames keeps its id
    ("track_motion", bool, False),
    ("track_motion_size", int, (384, 640)),
    # not reference flags: with --tracks, --instances writes every frame's instance map (an indexed PNG, a pixel's value names its track) into
    # D/native/instances/<sequence>/ and scores every track against the annotation; --overlay_instances (with --overlay) draws the maps, every
    # track in its colour, in the place of the single mask (native_results.instance_maps, visualize.overlay_instances)
    ("instances", bool, False),
    ("overlay_instances", bool, False),
    # not reference flags: with --tracks, --follow mass|area|length|best_gt|all exports and scores the masks of whole tracks, chosen per
    # sequence among those with rows in at least track_min_frames frames (native_results.follow_tracks); none: off
    ("follow", str, "none"),
    ("track_min_frames", int, 1),
    # not reference flags: with --tracks, --objects matches every object of a multi-object annotation (ids 1..objects_max, read from the
    # dataset's annotations or from objects_dir/<sequence>/<frame>.png) to one track and reports J per object
    # (native_results.object_overlaps, native_results.match_tracks)
    ("objects", bool, False),
    ("objects_max", int, 16),
    ("objects_dir", str, ""),
]


def default_flags():
    return SimpleNamespace(**{k: v for k, _, v in _DEFS})


def parse_flags(argv=None):
    ap = argparse.ArgumentParser()
    for k, t, v in _DEFS:
        if t is bool:
            ap.add_argument("--" + k, type=lambda s: s.lower() in ("1", "true", "yes"), default=v, nargs="?", const=True)
        elif isinstance(v, tuple):  # a fixed number of values: --track_motion_size 384 640
            ap.add_argument("--" + k, type=t, nargs=len(v), default=v)
        else:
            ap.add_argument("--" + k, type=t, default=v)
    return ap.parse_args(argv)


FLAGS = default_flags()
