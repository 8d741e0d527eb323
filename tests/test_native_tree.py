"""CPU: everything restore_results_dir writes with every option on at once, pinned to what it wrote before the native-resolution stage
was split into one module per step -- native_eval.json, detections/*.json and tracks/*.json as parsed objects, the key order of
native_eval.json and of one of its sequences, and every .png / .mat by a digest of its decoded content.

tests/golden/native_tree.json holds native_tree() of commit d5e7c6a ("Keep a track's id across frames where its component is missing"),
the last one with the whole stage in native_results.py.  The run uses the numpy stand-ins of the stage's other CPU tests."""
import hashlib
import json
import os

import numpy as np

from test_components import speckled_restore_np
from test_crf_native import ImagesNp, RefinedNp, crf_np
from test_detections import detect_np, select_labels_np
from test_frames_folder import frames_flags, make_frames_tree, raises
from test_native_results import davis_flags, load_gt_np, make_davis_tree, score_np
from test_overlay_native_gpu import overlay_np
from test_track_gaps import link_gap_np
from test_tracks import draw_track_boxes_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_tree.json")


# --------------------------------------------------------------------------------------------------------------- stand-ins ----
def load_images_np(paths):
    from unsupervised_detection_amd.data import _read_image
    return ImagesNp([_read_image(p, 3) for p in paths])


def refine_np(restored, images, crf):
    assert np.array_equal(images.hw, restored.hw)
    return RefinedNp(restored, [crf_np(a, restored.soft(i)) for i, a in enumerate(images.arrays)])


class OverlaysNp(object):
    def __init__(self, images):
        self.images = images

    def sample(self, i):
        return self.images[i]


def draw_np(frames, pred, overlay):
    return OverlaysNp([overlay_np(a, pred.binary_sample(i), **overlay)[0] for i, a in enumerate(frames.arrays)])


def draw_track_boxes_tree_np(overlays, det, trk, boxes):
    from unsupervised_detection_amd.visualize import TRACK_PALETTE
    ids = trk.host()[2]
    overlays.images = [draw_track_boxes_np(im, det.rows(i), ids[i], boxes["thickness"], TRACK_PALETTE) for i, im in enumerate(overlays.images)]
    return overlays


# ------------------------------------------------------------------------------------------------------------- the digest ----
def _sha(arrays):
    """sha256 over (name, dtype, shape, bytes) of every array: the decoded content, not the file's bytes."""
    h = hashlib.sha256()
    for name, a in arrays:
        a = np.ascontiguousarray(a)
        h.update("{} {} {} ".format(name, a.dtype.str, a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def digest_tree(out):
    """{"json": {path: parsed}, "keys": the ordered keys of native_eval.json and of its first sequence, "sha256": {path: digest}}."""
    import scipy.io as sio
    from PIL import Image
    parsed, digests = {}, {}
    for d, _, files in os.walk(out):
        for f in files:
            path = os.path.join(d, f)
            rel = os.path.relpath(path, out).replace(os.sep, "/")
            if f.endswith(".json"):
                with open(path) as fh:
                    parsed[rel] = json.load(fh)
            elif f.endswith(".png"):
                with Image.open(path) as im:
                    digests[rel] = _sha([(im.mode, np.asarray(im))])
            elif f.endswith(".mat"):
                mat = sio.loadmat(path)
                digests[rel] = _sha([(k, mat[k]) for k in sorted(mat) if not k.startswith("__")])
            else:
                raise AssertionError("unexpected file " + rel)
    top = parsed["native_eval.json"]
    first = next(iter(top["sequences"]))
    return {"json": dict(sorted(parsed.items())), "keys": {"native_eval": list(top), "sequence": [first, list(top["sequences"][first])]},
            "sha256": dict(sorted(digests.items()))}


def native_tree(tmp_path):
    """Run A (annotated, component "largest") and run B (a folder of frames, component None) with CRF, detections, tracks with gap
    bridging and an overlay with boxes, each digested."""
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    options = dict(batch=3, connectivity=4, verbose=False, restore=speckled_restore_np,
                   crf={"sxy": 4, "srgb": 5, "compat": 5, "gauss_k": 0.1, "iters": 3}, load_images=load_images_np, refine=refine_np,
                   detections={"min_area": 2, "max_detections": 3}, detect=detect_np,
                   overlay={"edge": 1, "boxes": {"thickness": 1}}, draw=draw_np, draw_boxes=raises, draw_track_boxes=draw_track_boxes_tree_np)
    tracks = {"min_iou": 0.2, "max_gap": 2}
    root, res, _ = make_davis_tree(tmp_path / "a", mixed=True, frames=7)
    restore_results_dir(res, frame_lists_from_reader(davis_flags(root)), str(tmp_path / "a" / "native"), load_gt=load_gt_np, score=score_np,
                        component="largest", select=select_labels_np([]), tracks=dict(tracks), link=link_gap_np([]), **options)
    root, res, _ = make_frames_tree(tmp_path / "b")
    restore_results_dir(res, frame_lists_from_reader(frames_flags(root)), str(tmp_path / "b" / "native"), mask_key="pred_mask", gt_rule="FRAMES",
                        load_gt=raises, score=raises, component=None, select=select_labels_np([]), tracks=dict(tracks), link=link_gap_np([]),
                        **options)
    return {"annotated": digest_tree(str(tmp_path / "a" / "native")), "frames": digest_tree(str(tmp_path / "b" / "native"))}


def test_the_whole_output_is_the_parents(tmp_path):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(native_tree(tmp_path)))
    for run in ("annotated", "frames"):
        assert sorted(got[run]["json"]) == sorted(want[run]["json"]) and sorted(got[run]["sha256"]) == sorted(want[run]["sha256"])
        for path in want[run]["json"]:
            assert got[run]["json"][path] == want[run]["json"][path], (run, path)
        assert got[run]["keys"] == want[run]["keys"]  # as lists: a reordering fails
        assert got[run]["sha256"] == want[run]["sha256"]
    # the runs exercise what they are meant to: every extra in the summary, boxes bridged over a gap, both heads
    a, b = want["annotated"]["json"]["native_eval.json"], want["frames"]["json"]["native_eval.json"]
    assert {"component", "connectivity", "crf", "overlay", "detections", "tracks", "J", "F"} <= set(a) and a["tracks"]["max_gap"] == 2
    assert b["annotations"] is False and {"crf", "overlay", "detections", "tracks"} <= set(b) and "component" not in b
    assert any(t["frames"] > 1 for run in (want["annotated"], want["frames"]) for p, v in run["json"].items() if p.startswith("tracks/")
               for s in v for t in s["tracks"])
