"""CPU: the host side of the detections at native size (native_results.component_boxes / detection_records, visualize.draw_boxes,
csrc/detections.hip) -- the numpy / scipy restatement of the definition, what the inputs of the GPU comparison promise,
the C entry points' argument checks, the wrappers' host validation, the records' arithmetic, restore_results_dir(detections=...) on
numpy stand-ins and the command-line flags.

boxes_np restates the definition from scipy.ndimage.label / find_objects and np.bincount alone; the ranking is a sort of Python
integers.  tests/test_detections_gpu.py compares the kernels with it for exact equality."""
import json
import os

import numpy as np
import pytest

from test_components import (DENSITIES, RAGGED_SHAPES, _tree_files, checkerboard, components_np, ragged_masks, roots_of, run_component_tree,
                             select_np, speckled_restore_np, structure)
from test_frames_folder import frames_flags, make_frames_tree, raises
from test_native_results import SEQS, frame_hw

FIELDS = 9  # root, area, y0, x0, y1, x1, sum_y, sum_x, score_sum


# ------------------------------------------------------------------------------------------------------------ restatement ----
def rank_rows(rows, min_area, k):
    """All components' rows -> (dets int64 [k, 9], counts [3]): kept, ranked (Python integers) and cut at k; the rest -1, 0, ..."""
    kept = sorted((r for r in rows if r[1] >= min_area), key=lambda r: (-r[1], r[0]))
    dets = np.zeros((k, FIELDS), np.int64)
    dets[:, 0] = -1
    for j, r in enumerate(kept[:k]):
        dets[j] = r
    return dets, [len(rows), len(kept), min(len(kept), k)]


def rows_np(binary, score=None, connectivity=8):
    """[root, area, y0, x0, y1, x1, sum_y, sum_x, score_sum] of every component of one frame, in scipy's order."""
    from scipy import ndimage
    fg = np.asarray(binary) != 0
    lab, nc = ndimage.label(fg, structure=structure(connectivity))
    roots = roots_of(lab, nc)
    flat = lab.ravel()
    yy, xx = np.divmod(np.arange(flat.size, dtype=np.int64), fg.shape[1])
    sc = np.zeros(flat.size, np.int64) if score is None else np.asarray(score, np.uint8).astype(np.int64).ravel()
    area = np.bincount(flat, minlength=nc + 1)
    sums = [np.zeros(nc + 1, np.int64) for _ in range(3)]
    for s, v in zip(sums, (yy, xx, sc)):
        np.add.at(s, flat, v)  # int64: exact
    rows = []
    for c, sl in enumerate(ndimage.find_objects(lab), 1):
        rows.append([int(roots[c - 1]), int(area[c]), sl[0].start, sl[1].start, sl[0].stop, sl[1].stop] + [int(s[c]) for s in sums])
    return rows


def boxes_np(binary, score=None, min_area=1, k=16, connectivity=8):
    """(dets int64 [k, 9], counts [components, kept, written]) of one frame."""
    return rank_rows(rows_np(binary, score, connectivity), min_area, k)


def boxes_from_labels_np(labels, score=None, min_area=1, k=16):
    """The same from a frame's labels (root + 1 / 0) alone; a value outside 1..H*W is background."""
    labels = np.asarray(labels)
    H, W = labels.shape
    sc = np.zeros((H, W), np.int64) if score is None else np.asarray(score).astype(np.int64)
    rows = []
    lab = np.where((labels >= 1) & (labels <= H * W), labels, 0)
    for v in np.unique(lab[lab > 0]):
        y, x = np.nonzero(lab == v)
        rows.append([int(v) - 1, len(y), int(y.min()), int(x.min()), int(y.max()) + 1, int(x.max()) + 1, int(y.sum()), int(x.sum()),
                     int(sc[y, x].sum())])
    return rank_rows(rows, min_area, k)


def draw_boxes_np(img, rows, thickness=2, colour=(255, 255, 0)):
    """include/udet.h, udet_draw_boxes_ragged, written as its sentence: a pixel of a box is painted when it lies within `thickness` rows
    or columns of the box's edge.  Returns a painted copy."""
    out = np.array(img, copy=True)
    t = int(thickness)
    for _, _, y0, x0, y1, x1 in (tuple(int(v) for v in r[:6]) for r in rows):
        y, x = np.mgrid[y0:y1, x0:x1]
        line = (y < y0 + t) | (y >= y1 - t) | (x < x0 + t) | (x >= x1 - t)
        out[y0:y1, x0:x1][line] = np.asarray(colour, np.uint8)
    return out


class DetectionsNp(object):
    def __init__(self, dets, counts):
        self.dets, self.counts = np.asarray(dets, np.int64), np.asarray(counts, np.int64)

    def __len__(self):
        return len(self.dets)

    def rows(self, i):
        return self.dets[i, :int(self.counts[i, 2])]


class LabelledNp(object):
    """select_np's result with the labels of every frame."""

    def __init__(self, sel, labels):
        self.sel, self.labels, self.info, self.hw = sel, labels, sel.info, sel.hw

    def binary_sample(self, i):
        return self.sel.binary_sample(i)

    def stack(self, idx):
        return self.sel.stack(idx)


def select_labels_np(calls):
    """Stand-in for select_components with want_labels: select_np plus the labels of components_np; every call is noted in `calls`."""
    def select(res, gt=None, mode="largest", connectivity=8, want_labels=False):
        calls.append((mode, connectivity, want_labels))
        sel = select_np(res, gt, mode, connectivity)
        if not want_labels:
            return sel
        return LabelledNp(sel, [components_np(res.binary_sample(i), None, "label", connectivity)[0] for i in range(len(res.hw))])
    return select


def detect_np(labelled, score=None, min_area=64, max_detections=16):
    out = [boxes_from_labels_np(lab, None if score is None else score.sample(i), min_area, max_detections) for i, lab in enumerate(labelled.labels)]
    return DetectionsNp([o[0] for o in out], [o[1] for o in out])


def records_np(rows, amax):
    """detection_records of one frame, from the issue's sentence."""
    return [{"box": [int(r[3]), int(r[2]), int(r[5]), int(r[4])], "area": int(r[1]), "centroid": [int(r[7]) / int(r[1]), int(r[6]) / int(r[1])],
             "score": int(r[8]) / (int(r[1]) * (float(amax) + 1e-8)), "root": int(r[0])} for r in rows]


def scores_for(masks, seed=9):
    """Random bytes that include 0 and 255 on every frame of more than one pixel."""
    rng = np.random.default_rng(seed)
    out = []
    for m in masks:
        s = rng.integers(0, 256, m.shape, dtype=np.uint8)
        if s.size > 1:
            s.reshape(-1)[0], s.reshape(-1)[-1] = 0, 255
        out.append(s)
    return out


# ----------------------------------------------------------------------------------------------------------------- tests ----
def test_the_inputs_exercise_what_they_are_meant_to():
    assert RAGGED_SHAPES[3:] == [(37, 53), (67, 131), (130, 259)]
    m = ragged_masks(0.3)
    full = [boxes_np(m[i], None, 1, 64 * 80, 4) for i in (3, 4, 5)]
    assert [c[1][0] for c in full] == [264, 1135, 4383]  # more components than k = 16 and k = 64: both cut
    assert [boxes_np(m[i], None, 4, 64, 4)[1] for i in (3, 4, 5)] == [[264, 41, 41], [1135, 192, 64], [4383, 744, 64]]
    ties = 0
    for d in DENSITIES:
        for b in ragged_masks(d)[3:]:
            for conn in (4, 8):
                dets, counts = boxes_np(b, None, 1, 80, conn)
                for k in (16, 64):
                    if counts[1] > k and dets[k - 1, 1] == dets[k, 1]:  # equal areas on both sides of the cut: the root decides
                        assert dets[k - 1, 0] < dets[k, 0]
                        ties += 1
    assert ties >= 3  # "several"
    assert not ragged_masks(0.593)[0].any() and boxes_np(ragged_masks(0.593)[0], None, 1, 16, 8)[1] == [0, 0, 0]
    assert boxes_np(checkerboard(), None, 1, 64, 4)[1] == [980, 980, 64] and boxes_np(checkerboard(), None, 1, 64, 8)[1] == [1, 1, 1]
    for s in scores_for(m):
        assert s.size == 1 or (s.min() == 0 and s.max() == 255)


def test_restatement_is_consistent():
    """boxes_np's first row is the LARGEST choice of components_np; the label-based form agrees with it; find_objects' stops are the
    exclusive ends; the rows past the written ones are -1, 0, ..."""
    for d in (0.3, 0.593):
        masks = ragged_masks(d)
        for b, s in zip(masks, scores_for(masks)):
            for conn in (4, 8):
                labels, sel, info = components_np(b, None, "largest", conn)
                dets, counts = boxes_np(b, s, 1, 16, conn)
                assert counts[0] == info[0] and dets[0, :2].tolist() == info[1:3]
                got = boxes_from_labels_np(labels, s, 1, 16)
                assert np.array_equal(got[0], dets) and got[1] == counts
                if info[1] >= 0:
                    y, x = np.nonzero(sel)
                    assert dets[0, 2:].tolist() == [y.min(), x.min(), y.max() + 1, x.max() + 1, y.sum(), x.sum(), int(s[sel != 0].astype(np.int64).sum())]
                assert (dets[counts[2]:, 0] == -1).all() and not dets[counts[2]:, 1:].any()
                assert boxes_np(b, s, 10 ** 6, 16, conn)[1] == [info[0], 0, 0]
    img = np.zeros((12, 15, 3), np.uint8)
    out = draw_boxes_np(img, [[0, 1, 1, 2, 11, 14], [0, 1, 0, 0, 3, 15]], 2, (1, 2, 3))
    painted = out.any(2)
    assert painted[0:3].all() and painted[3:11, 2:4].all() and painted[9:11, 2:14].all() and not painted[3:9, 4:12].any()  # the second box: filled
    assert not painted[11].any() and not painted[3:, :2].any() and not painted[3:, 14].any() and (out[painted] == (1, 2, 3)).all()


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    assert lib.udet_component_boxes_workspace_bytes(1000, 2, 16) >= 8 * 1000
    assert lib.udet_component_boxes_workspace_bytes(1000, 2, 16) <= 12 * 1000  # about 8 bytes per pixel: less than the labelling call's 12
    for bad in ((0, 2, 16), (1000, 0, 16), (1000, 2, 0), (1000, 2, 65)):
        assert lib.udet_component_boxes_workspace_bytes(*bad) == 0
    ok = dict(labels=64, score=128, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, min_area=1, k=16, dets=256, counts=512, ws=64,
              ws_bytes=1 << 20, stream=None)
    for change in (dict(labels=None), dict(offsets=None), dict(hw=None), dict(dets=None), dict(counts=None), dict(n=0), dict(n=-3),
                   dict(n=65536), dict(k=0), dict(k=65), dict(k=-1), dict(min_area=0), dict(min_area=-5), dict(max_h=0), dict(max_w=0),
                   dict(total=0), dict(ws=None), dict(ws_bytes=64), dict(ws=68), dict(labels=66), dict(dets=260), dict(counts=516)):
        a = dict(ok, **change)
        rc = lib.udet_component_boxes_ragged(a["labels"], a["score"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"],
                                             a["min_area"], a["k"], a["dets"], a["counts"], a["ws"], a["ws_bytes"], a["stream"])
        assert rc == -5 and b"component_boxes_ragged" in lib.udet_last_error(), change
    ok = dict(rgb=64, n=2, offsets=64, hw=64, total=3180, dets=256, counts=512, k=16, thickness=2, colour=0xffff00, stream=None)
    for change in (dict(rgb=None), dict(offsets=None), dict(hw=None), dict(dets=None), dict(counts=None), dict(n=0), dict(n=65536),
                   dict(total=0), dict(k=0), dict(k=65), dict(thickness=0), dict(thickness=9), dict(colour=0x1000000), dict(dets=260),
                   dict(counts=516)):
        a = dict(ok, **change)
        rc = lib.udet_draw_boxes_ragged(a["rgb"], a["n"], a["offsets"], a["hw"], a["total"], a["dets"], a["counts"], a["k"], a["thickness"],
                                        a["colour"], a["stream"])
        assert rc == -5 and b"draw_boxes_ragged" in lib.udet_last_error(), change


def test_wrappers_validate_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd.native_results import ComponentSelection, Detections, component_boxes, detection_params
    from unsupervised_detection_amd.ragged import PackedLayout
    from unsupervised_detection_amd.visualize import box_params, draw_boxes
    hw = [(30, 53), (13, 26)]
    total = 30 * 53 + 13 * 26
    lab = torch.zeros(total, dtype=torch.int32)  # a host tensor: anything that got past the validation would fail on it, not launch

    def bad(match, **kw):
        args = dict(selection_or_labels=lab, offsets=[0, 30 * 53], hw=hw)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            component_boxes(**args)
    bad("overlap", offsets=[0, 30 * 53 - 1])
    bad("outside the packed buffer", offsets=[0, 30 * 53 + 1])
    bad("outside the packed buffer", selection_or_labels=lab[:-1])
    bad("at least 1x1", hw=[(30, 53), (0, 26)])
    bad("one \\(H, W\\) per offset", hw=[(30, 53)])
    bad("offsets and sizes", offsets=None)
    bad("int32", selection_or_labels=lab.long())
    bad("min_area", min_area=0)
    bad("max_detections", max_detections=0)
    bad("max_detections", max_detections=65)
    bad("integer", max_detections=2.5)
    bad("packed like the labels", score=torch.zeros(total - 1, dtype=torch.uint8))
    bad("uint8", score=torch.zeros(total, dtype=torch.int32))
    bad("no labels", selection_or_labels=ComponentSelection(None, None, torch.zeros((2, 4), dtype=torch.int64), [0, 30 * 53], hw), offsets=None, hw=None)
    bad("CUDA")  # everything valid but the host tensor: refused before any call into the library
    assert detection_params(None) == detection_params({}) == {"min_area": 64, "max_detections": 16}
    assert detection_params({"min_area": 3, "max_detections": 64}) == {"min_area": 3, "max_detections": 64}
    for d in ({"k": 3}, {"min_area": 0}, {"max_detections": 65}, {"min_area": 1.5}, [3]):
        with pytest.raises(ValueError, match="detections"):
            detection_params(d)
    assert box_params(None) == {"thickness": 2, "colour": (255, 255, 0)} and box_params({"thickness": 8, "colour": [1, 2, 3]})["colour"] == (1, 2, 3)
    for b in ({"thickness": 0}, {"thickness": 9}, {"thickness": 1.5}, {"width": 2}):
        with pytest.raises(ValueError, match="boxes"):
            box_params(b)
    with pytest.raises(ValueError, match="colour"):
        box_params({"colour": (0, 0, 256)})
    # draw_boxes: host tensors throughout
    layout = PackedLayout.packed(hw)
    det = Detections(torch.zeros((2, 4, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, 4)

    class Frames(object):
        def __init__(self, data, lay):
            self.data, self.layout = data, lay
    rgb = PackedLayout(3 * layout.offsets, hw, 3 * total, 3)
    with pytest.raises(ValueError, match="three times their offsets"):
        draw_boxes(Frames(torch.zeros(total, dtype=torch.uint8), layout), det)
    with pytest.raises(ValueError, match="thickness"):
        draw_boxes(Frames(torch.zeros(3 * total, dtype=torch.uint8), rgb), det, thickness=9)
    with pytest.raises(ValueError, match="dets must be"):
        draw_boxes(Frames(torch.zeros(3 * total, dtype=torch.uint8), rgb), Detections(det.dets[:, :3], det.counts, layout, 1, 4))
    with pytest.raises(ValueError, match="CUDA"):
        draw_boxes(Frames(torch.zeros(3 * total, dtype=torch.uint8), rgb), det)
    assert det.rows(0).shape == (0, 9)


def test_detection_records_arithmetic():
    from unsupervised_detection_amd.native_results import detection_records
    dets = np.zeros((2, 3, FIELDS), np.int64)
    dets[:, :, 0] = -1
    dets[0, 0] = [17, 6, 1, 2, 4, 5, 13, 19, 700]
    dets[0, 1] = [3, 1, 0, 3, 1, 4, 0, 3, 0]
    got = detection_records(DetectionsNp(dets, [[5, 2, 2], [0, 0, 0]]), np.array([200, 0], np.int32))
    assert got[1] == [] and len(got[0]) == 2
    assert got[0][0] == {"box": [2, 1, 5, 4], "area": 6, "centroid": [19 / 6, 13 / 6], "score": 700 / (6 * (200.0 + 1e-8)), "root": 17}
    assert got[0][1] == {"box": [3, 0, 4, 1], "area": 1, "centroid": [3.0, 0.0], "score": 0.0, "root": 3}
    assert got[0] == records_np(dets[0, :2], 200)
    assert all(type(v) in (int, float) for r in got[0] for f in r.values() for v in (f if isinstance(f, list) else [f]))
    json.dumps(got)
    # the score is the mean of RestoredMasks.soft over the component
    rng = np.random.default_rng(0)
    data, amax = rng.integers(0, 201, (9, 11), dtype=np.uint8), 200
    m = np.zeros((9, 11), np.uint8)
    m[2:6, 3:9] = 1
    d, c = boxes_np(m, data, 1, 1, 8)
    soft = data.astype(np.float64) / (np.float64(amax) + 1e-8)
    rec = detection_records(DetectionsNp([d], [c]), [amax])[0][0]
    assert abs(rec["score"] - soft[m != 0].mean()) < 1e-14 and rec["box"] == [3, 2, 9, 6] and rec["centroid"] == [5.5, 3.5]
    with pytest.raises(ValueError, match="amax"):
        detection_records(DetectionsNp([d], [c]), [amax, amax])


def want_records(restored, i, conn, min_area, k):
    dets, counts = boxes_np(restored.binary_sample(i), restored.sample(i), min_area, k, conn)
    return records_np(dets[:counts[2]], restored.amax[i])


@pytest.mark.parametrize("component", [None, "largest"])
def test_restore_results_dir_with_detections(tmp_path, component):
    calls = []
    kw = dict(select=select_labels_np(calls), detect=detect_np, detections={"min_area": 2, "max_detections": 3}, connectivity=4)
    out0, js0, masks = run_component_tree(tmp_path, "plain", True, component=component, select=select_np, connectivity=4)
    out, js, _ = run_component_tree(tmp_path, "det", True, component=component, **kw)
    assert calls == [(component or "label", 4, True)] * 4  # two sequences of three frames, batch = 2: labelled once per batch
    assert js["detections"] == {"min_area": 2, "max_detections": 3, "connectivity": 4}
    assert {k: v for k, v in js.items() if k not in ("detections", "sequences", "connectivity")} == {k: v for k, v in js0.items() if k not in ("sequences", "connectivity")}
    with open(os.path.join(out, "native_eval.json")) as f:
        assert json.load(f) == json.loads(json.dumps(js))
    f0, f1 = _tree_files(out0), _tree_files(out)
    assert sorted(set(f1) - set(f0)) == [os.path.join("detections", s + ".json") for s in SEQS]
    assert all(f0[k] == f1[k] for k in f0 if k != "native_eval.json")  # masks and .mat files are what they were
    for seq in SEQS:
        with open(os.path.join(out, "detections", seq + ".json")) as f:
            got = json.load(f)
        assert list(got) == ["%05d" % k for k in range(3)]  # the list's order
        n = []
        for k in range(3):
            r = speckled_restore_np(masks[seq][k][None], [frame_hw(seq, k, True)], 0.9, 0.5)
            want = want_records(r, 0, 4, 2, 3)
            assert got["%05d" % k] == json.loads(json.dumps(want)) and 2 <= len(want) <= 3, (seq, k)
            assert want[0]["area"] >= want[-1]["area"] >= 2 and 0.0 < want[0]["score"] <= 1.0
            n.append(len(want))
        assert js["sequences"][seq]["detections_mean"] == float(np.mean(n))
        assert {k: v for k, v in js["sequences"][seq].items() if k != "detections_mean"} == js0["sequences"][seq]


def test_detections_without_annotations_and_with_boxes(tmp_path):
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_frames_tree(tmp_path)
    lists = frame_lists_from_reader(frames_flags(root))
    calls, drawn = [], []
    kw = dict(mask_key="pred_mask", restore=speckled_restore_np, load_gt=raises, score=raises, verbose=False, batch=2, gt_rule="FRAMES")

    class Frames(object):
        def __init__(self, paths):
            from PIL import Image
            self.images = [np.asarray(Image.open(p).convert("RGB")) for p in paths]

        def sample(self, i):
            return self.images[i]

    def draw(frames, pred, overlay):
        return frames

    def draw_boxes(overlays, det, boxes):
        drawn.append(boxes)
        overlays.images = [draw_boxes_np(im, det.rows(i), **boxes) for i, im in enumerate(overlays.images)]
        return overlays
    out = str(tmp_path / "native")
    js = restore_results_dir(res, lists, out, detections={}, select=select_labels_np(calls), detect=detect_np, load_images=Frames, draw=draw,
                             overlay={"edge": 0, "boxes": {"thickness": 1}}, draw_boxes=draw_boxes, **kw)
    assert calls == [("label", 8, True)] * 3 and drawn == [{"thickness": 1, "colour": (255, 255, 0)}] * 3
    assert js["annotations"] is False and js["detections"] == {"min_area": 64, "max_detections": 16, "connectivity": 8}
    assert js["overlay"]["boxes"] == {"thickness": 1, "colour": (255, 255, 0)} and js["overlay"]["edge"] == 0
    assert sorted(os.listdir(os.path.join(out, "detections"))) == ["clip.json", "other.json"]
    from PIL import Image
    from test_frames_folder import FRAME_HW
    for (seq, k), (H, W) in sorted(FRAME_HW.items()):
        r = speckled_restore_np(masks[seq][k][None], [(H, W)], 0.9, 0.5)
        dets, counts = boxes_np(r.binary_sample(0), r.sample(0), 64, 16, 8)
        with open(os.path.join(out, "detections", seq + ".json")) as f:
            assert json.load(f)["f%d" % k] == json.loads(json.dumps(records_np(dets[:counts[2]], r.amax[0])))
        assert counts[2] == 1  # the blob; the specks are below min_area
        with Image.open(os.path.join(root, seq, "f%d.png" % k)) as im:
            frame = np.asarray(im.convert("RGB"))
        with Image.open(os.path.join(out, "overlay", seq, "f%d.png" % k)) as im:
            assert np.array_equal(np.asarray(im), draw_boxes_np(frame, dets[:1], 1))
    assert all(set(v) == {"frames", "foreground_mean", "detections_mean"} and v["detections_mean"] == 1.0 for v in js["sequences"].values())
    for bad, match in ((dict(overlay={"boxes": {}}), "needs detections"), (dict(detections={"k": 1}), "detections"),
                       (dict(detections={}, overlay={"boxes": {"thickness": 9}}), "thickness"), (dict(detections={}, connectivity=6), "connectivity")):
        with pytest.raises(ValueError, match=match):
            restore_results_dir(res, lists, str(tmp_path / "bad"), select=select_labels_np(calls), detect=detect_np, load_images=Frames, draw=draw,
                                draw_boxes=draw_boxes, **dict(kw, **bad))


def test_detections_none_changes_nothing(tmp_path):
    """detections=None (the default): neither callable runs, select is called as before, every file equals a run without the argument."""
    out0, js0, _ = run_component_tree(tmp_path, "a", True, component="largest", select=select_np)
    out1, js1, _ = run_component_tree(tmp_path, "b", True, component="largest", select=select_np, detections=None, detect=raises, draw_boxes=raises)
    assert js0 == js1
    f0, f1 = _tree_files(out0), _tree_files(out1)
    assert sorted(f0) == sorted(f1) and len(f0) == 13 and all(f0[k] == f1[k] for k in f0)


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    a = cli.parse_restore_results_args(base)
    assert (a.detections, a.det_min_area, a.det_max, a.overlay_boxes) == (False, 64, 16, False)
    assert cli._detections(a) is None and cli._overlay(a) is None
    a = cli.parse_restore_results_args(base + ["--detections", "--det_min_area", "9", "--det_max", "64", "--connectivity", "4"])
    assert cli._detections(a) == {"min_area": 9, "max_detections": 64} and a.connectivity == 4
    a = cli.parse_restore_results_args(base + ["--detections", "--overlay", "--overlay_boxes", "--overlay_box_thickness", "3",
                                               "--overlay_box_colour", "1,2,3"])
    assert cli._overlay(a)["boxes"] == {"thickness": 3, "colour": (1, 2, 3)} and cli._overlay(a)["edge"] == 2
    assert "boxes" not in cli._overlay(cli.parse_restore_results_args(base + ["--detections", "--overlay"]))
    for bad, said in ((["--overlay_boxes"], "--overlay and --detections"), (["--overlay_boxes", "--overlay"], "--overlay and --detections"),
                      (["--overlay_boxes", "--detections"], "--overlay and --detections"), (["--detections", "--det_max", "65"], "--det_max"),
                      (["--detections", "--det_min_area", "0"], "--det_min_area"),
                      (["--detections", "--overlay", "--overlay_boxes", "--overlay_box_thickness", "9"], "thickness"),
                      (["--detections", "--overlay", "--overlay_boxes", "--overlay_box_colour", "1,2"], "r,g,b")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    d = default_flags()
    assert (d.detections, d.det_min_area, d.det_max, d.overlay_boxes, d.overlay_box_thickness, d.overlay_box_colour) == (False, 64, 16, False, 2, "255,255,0")
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D"]
    f = parse_flags(native + ["--detections", "--det_max", "8", "--overlay", "--overlay_boxes"])
    cli.check_native_flags(f)
    assert cli._detections(f) == {"min_area": 64, "max_detections": 8} and cli._overlay(f)["boxes"]["thickness"] == 2
    for bad in (["--overlay_boxes"], ["--detections", "--det_max", "0"]):
        with pytest.raises(SystemExit):
            cli.check_native_flags(parse_flags(native + bad))
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R"]
    a = cli.parse_post_process_args(pp + ["--detections", "--overlay", "--overlay_boxes"])
    assert cli._detections(a) == {"min_area": 64, "max_detections": 16} and cli._overlay(a)["boxes"]["colour"] == (255, 255, 0)
    with pytest.raises(SystemExit):
        cli.parse_post_process_args(pp + ["--overlay_boxes", "--overlay"])
    for flag in ("--detections", "--det_min_area", "--det_max", "--overlay_boxes", "--overlay_box_thickness", "--overlay_box_colour"):
        assert flag in cli.__doc__
