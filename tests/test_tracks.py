"""CPU: the host side of the detections linked into tracks (native_results.link_detections / track_records / summarise_tracks,
visualize.draw_track_boxes, csrc/tracks.hip) -- the numpy restatement of the definition, what the inputs of the GPU
comparison promise, the C entry points' argument checks, the wrappers' host validation, the records' and the summary's arithmetic,
restore_results_dir(tracks=...) on numpy stand-ins, the command-line flags and the header's sentences.

links_np restates include/udet.h's definition: inter is a bincount over (rank_a, rank_b) of the co-located pixels, the matching a Python
loop over integers, the id walk plain Python.  tests/test_tracks_gpu.py compares the kernels with it for exact equality."""
import functools
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from test_components import _tree_files, components_np, select_np, speckled_restore_np
from test_detections import DetectionsNp, boxes_np, detect_np, select_labels_np
from test_native_results import SEQS, davis_flags, frame_hw, load_gt_np, make_davis_tree, score_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = 9


# ------------------------------------------------------------------------------------------------------------ restatement ----
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def rank_map(labels, dets, rows):
    """Per pixel the rank of the row whose root its label names, or -1 (background, an out-of-range label, a component without a row)."""
    labels = np.asarray(labels)
    hw = labels.size
    table = np.full(hw, -1, np.int64)
    for r in range(rows):
        if 0 <= int(dets[r, 0]) < hw:
            table[int(dets[r, 0])] = r
    valid = (labels >= 1) & (labels <= hw)
    return np.where(valid, table[np.where(valid, labels.astype(np.int64) - 1, 0)], -1)


def greedy_match(inter, area_p, area_c, permille):
    """{b: a} of the greedy matching: the candidates in the order "larger inter / union, then smaller a, then smaller b" (integers,
    cross-multiplied), each taken when both of its rows are still free -- what taking the best free candidate repeatedly gives."""
    cands = []
    for a in range(len(area_p)):
        for b in range(len(area_c)):
            it = int(inter[a, b])
            union = int(area_p[a]) + int(area_c[b]) - it
            if it > 0 and 1000 * it >= permille * union:
                cands.append((it, union, a, b))

    def order(p, q):
        l, r = p[0] * q[1], q[0] * p[1]
        if l != r:
            return -1 if l > r else 1
        return -1 if p[2:] < q[2:] else 1
    match, used = {}, set()
    for it, union, a, b in sorted(cands, key=functools.cmp_to_key(order)):
        if a not in used and b not in match:
            match[b] = a
            used.add(a)
    return match


def links_np(labels_list, dets, counts, link, min_iou_permille, carry=None):
    """include/udet.h, udet_link_detections_ragged, written as its sentences.  labels_list: per frame the [H, W] labels; dets [n, k, 9],
    counts [n, 3]; link: n values; carry: None or an object with labels / hw / dets / counts / ids / next_id (native_results.TrackTail).
    Returns a namespace of inter, match, ids, linked, seq_tracks (arrays of the kernels' dtypes) and next_id."""
    dets, counts = _np(dets).astype(np.int64), _np(counts).astype(np.int64)
    n, k = dets.shape[:2]
    out = SimpleNamespace(inter=np.zeros((n, k, k), np.int64), match=np.full((n, k), -1, np.int32), ids=np.full((n, k), -1, np.int32),
                          linked=np.zeros(n, np.int32), seq_tracks=np.zeros(n, np.int32), next_id=0)
    rows = [min(max(int(c[2]), 0), k) for c in counts]
    prev = None
    if carry is not None:
        prev = (_np(carry.labels).reshape(carry.hw), _np(carry.dets).astype(np.int64), min(max(int(_np(carry.counts)[2]), 0), k),
                _np(carry.ids).reshape(-1))
        out.next_id = int(_np(carry.next_id).reshape(-1)[0])
    for i in range(n):
        lab = np.asarray(labels_list[i])
        if not (int(link[i]) != 0 and prev is not None and prev[0].shape == lab.shape):
            if i:
                out.seq_tracks[i - 1] = out.next_id
            out.ids[i, :rows[i]] = np.arange(rows[i])
            out.next_id = rows[i]
        else:
            out.linked[i] = 1
            ra, rb = rank_map(prev[0], prev[1], prev[2]).ravel(), rank_map(lab, dets[i], rows[i]).ravel()
            both = (ra >= 0) & (rb >= 0)
            out.inter[i] = np.bincount(ra[both] * k + rb[both], minlength=k * k).reshape(k, k)
            match = greedy_match(out.inter[i], prev[1][:prev[2], 1], dets[i, :rows[i], 1], min_iou_permille)
            for b in range(rows[i]):
                if b in match:
                    out.match[i, b], out.ids[i, b] = match[b], prev[3][match[b]]
                else:
                    out.ids[i, b] = out.next_id
                    out.next_id += 1
        prev = (lab, dets[i], rows[i], out.ids[i])
    out.seq_tracks[n - 1] = out.next_id
    return out


def draw_track_boxes_np(img, rows, ids, thickness=2, palette=((255, 255, 0),)):
    """include/udet.h, udet_draw_track_boxes_ragged: every row with an id painted as draw_boxes_np paints it, in its track's colour, the
    larger ranks first -- so that where lines cross the smallest rank is what remains.  Returns a painted copy."""
    out = np.array(img, copy=True)
    t = int(thickness)
    for r in reversed(range(len(rows))):
        if int(ids[r]) < 0 or int(rows[r][0]) < 0:
            continue
        y0, x0, y1, x1 = (int(v) for v in rows[r][2:6])
        y, x = np.mgrid[y0:y1, x0:x1]
        line = (y < y0 + t) | (y >= y1 - t) | (x < x0 + t) | (x >= x1 - t)
        out[y0:y1, x0:x1][line] = np.asarray(palette[int(ids[r]) % len(palette)], np.uint8)
    return out


def tail_np(labels, dets, counts, ids, next_id):
    """The last frame of a links_np result as the next call's carry."""
    from unsupervised_detection_amd.native_results import TrackTail
    return TrackTail(np.array(labels, np.int32).reshape(-1), np.asarray(labels).shape, np.array(dets, np.int64), np.array(counts, np.int64),
                     np.array(ids, np.int32), np.array([next_id], np.int32))


def inputs_np(frames, k, min_area=1, conn=8):
    """(labels_list, dets [n, k, 9], counts [n, 3]) of binary frames, from the scipy restatements of the labelling and the boxes."""
    labels = [components_np(f, None, "label", conn)[0] for f in frames]
    boxes = [boxes_np(f, None, min_area, k, conn) for f in frames]
    return labels, np.stack([b[0] for b in boxes]), np.array([b[1] for b in boxes], np.int64)


# ------------------------------------------------------------------------------------------------------- hand-built cases ----
def rects(hw, *boxes):
    m = np.zeros(hw, np.uint8)
    for y0, x0, y1, x1 in boxes:
        m[y0:y1, x0:x1] = 1
    return m


def hand_cases():
    """{name: (frames, k, permille)}: one short sequence per property the issue lists (8-connected, min_area 1)."""
    s = (8, 18)
    two, bridge = rects(s, (1, 1, 3, 4), (1, 6, 3, 9)), rects(s, (1, 3, 3, 7))
    return {
        # A moves by a pixel and is matched; B appears: unmatched, a new id
        "matched and unmatched": ([rects(s, (1, 1, 5, 7)), rects(s, (1, 2, 5, 8), (6, 12, 8, 16))], 4, 100),
        # 3 x 12 loses column 9: parts of 21 and 12 pixels, IoU 21 / 36 and 12 / 36
        "split": ([rects(s, (2, 2, 5, 14)), rects(s, (2, 2, 5, 9), (2, 10, 5, 14))], 4, 100),
        "merge": ([rects(s, (2, 2, 5, 9), (2, 10, 5, 14)), rects(s, (2, 2, 5, 14))], 4, 100),
        # two blobs of 6, a bridge of 8 that shares 2 pixels with each, the two blobs again: 2 / 12 four times
        "tie": ([two, bridge, two], 4, 100),
        # 5 and 5 pixels sharing 2: 1000 * 2 == 250 * 8
        "on the threshold": ([rects(s, (1, 1, 2, 6)), rects(s, (1, 4, 2, 9))], 4, 250),
        # one pixel more in the union: 1000 * 2 < 250 * 9
        "below the threshold": ([rects(s, (1, 1, 2, 6)), rects(s, (1, 4, 2, 10))], 4, 250),
        # C stays, A is gone for a frame and comes back
        "vanish and return": ([rects(s, (1, 1, 6, 7), (2, 10, 5, 14)), rects(s, (1, 1, 6, 7)), rects(s, (1, 1, 6, 7), (2, 10, 5, 14))], 4, 100),
        # k = 2: X (20) and Y (10) have rows; then Z (15) appears and pushes Y past the cut
        "past the cut": ([rects(s, (1, 1, 5, 6), (6, 1, 8, 6)), rects(s, (1, 1, 5, 6), (6, 1, 8, 6), (1, 10, 4, 15))], 2, 100),
        # the third frame has another size: it starts a sequence although link says 1
        "size change": ([rects(s, (1, 1, 5, 7)), rects(s, (1, 2, 5, 8)), rects((9, 18), (1, 2, 5, 8)), rects((9, 18), (1, 3, 5, 9), (6, 1, 8, 4))], 4, 100),
    }


def run_case(name, k=None):
    frames, k0, permille = hand_cases()[name]
    labels, dets, counts = inputs_np(frames, k or k0)
    return links_np(labels, dets, counts, [1] * len(frames), permille), dets, counts


def test_the_hand_built_cases_are_what_they_claim():
    r, dets, _ = run_case("matched and unmatched")
    assert r.linked.tolist() == [0, 1] and r.match[1, :2].tolist() == [0, -1] and r.ids[1].tolist() == [0, 1, -1, -1]
    assert r.inter[1, 0, 0] == 4 * 5 and r.seq_tracks.tolist() == [0, 2] and r.next_id == 2
    r, dets, _ = run_case("split")
    assert dets[1, :2, 1].tolist() == [21, 12] and r.inter[1, 0, :2].tolist() == [21, 12]
    assert r.match[1, :2].tolist() == [0, -1] and r.ids[1, :2].tolist() == [0, 1]  # the larger IoU inherits, the other is new
    r, dets, _ = run_case("merge")
    assert r.inter[1, :2, 0].tolist() == [21, 12] and r.match[1, 0] == 0 and r.ids[1, 0] == 0 and r.seq_tracks.tolist() == [0, 2]
    r, dets, _ = run_case("tie")
    assert r.inter[1, :2, 0].tolist() == [2, 2] and dets[0, :2, 1].tolist() == [6, 6] and dets[1, 0, 1] == 8  # 2 / 12 against 2 / 12
    assert r.match[1, 0] == 0 and r.ids[1, 0] == 0                                                   # ... to the smaller a
    assert r.inter[2, 0, :2].tolist() == [2, 2] and r.match[2, :2].tolist() == [0, -1] and r.ids[2, :2].tolist() == [0, 2]  # ... then the smaller b
    r, dets, _ = run_case("on the threshold")
    it, union = int(r.inter[1, 0, 0]), int(dets[0, 0, 1] + dets[1, 0, 1] - r.inter[1, 0, 0])
    assert (it, union) == (2, 8) and 1000 * it == 250 * union and r.match[1, 0] == 0 and r.ids[1, 0] == 0  # kept
    r, dets, _ = run_case("below the threshold")
    it, union = int(r.inter[1, 0, 0]), int(dets[0, 0, 1] + dets[1, 0, 1] - r.inter[1, 0, 0])
    assert (it, union) == (2, 9) and 1000 * it < 250 * union and r.match[1, 0] == -1 and r.ids[1, 0] == 1  # dropped
    r, dets, counts = run_case("vanish and return")
    assert counts[:, 2].tolist() == [2, 1, 2] and r.ids[:, :2].tolist() == [[0, 1], [0, -1], [0, 2]] and r.next_id == 3  # back under a new id
    r, dets, counts = run_case("past the cut")
    assert counts[1].tolist() == [3, 3, 2] and dets[1, :, 1].tolist() == [20, 15]
    assert r.ids.tolist() == [[0, 1], [0, 2]] and r.match[1].tolist() == [0, -1]
    full, fd, _ = run_case("past the cut", k=3)  # with a third row Y is linked: it overlaps its predecessor
    assert fd[1, 2, 1] == 10 and full.match[1].tolist() == [0, -1, 1] and full.ids[1].tolist() == [0, 2, 1]
    r, dets, _ = run_case("size change")
    assert r.linked.tolist() == [0, 1, 0, 1] and r.seq_tracks.tolist() == [0, 1, 0, 2] and r.ids[:, :2].tolist() == [[0, -1], [0, -1], [0, -1], [0, 1]]
    assert not r.inter[2].any() and (r.match[2] == -1).all()
    # every property occurs; link = 0 cuts a sequence like a size change does
    frames, k, permille = hand_cases()["tie"]
    labels, dets, counts = inputs_np(frames, k)
    cut = links_np(labels, dets, counts, [1, 0, 1], permille)
    assert cut.linked.tolist() == [0, 0, 1] and cut.seq_tracks.tolist() == [2, 0, 2] and not cut.inter[1].any()


def moving_sequence(base, n, seed):
    """n frames from one binary frame: each the one before rolled by a pixel or two, a block dropped and a block added."""
    rng = np.random.default_rng(seed)
    out = [np.array(base, np.uint8)]
    H, W = base.shape
    for _ in range(n - 1):
        f = np.roll(out[-1], (int(rng.integers(0, 2)), int(rng.integers(1, 3))), (0, 1))
        for v in (0, 1):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            f[y:y + max(1, H // 5), x:x + max(1, W // 7)] = v
        out.append(f)
    return out


def test_carry_restated_a_sequence_in_pieces_is_the_sequence():
    from test_components import ragged_masks
    frames = moving_sequence(ragged_masks(0.45)[3], 7, 1)
    labels, dets, counts = inputs_np(frames, 16, 2, 4)
    whole = links_np(labels, dets, counts, [1] * 7, 100)
    assert whole.linked.tolist() == [0] + [1] * 6 and (whole.match >= 0).sum() > 20 and whole.next_id > 16 and (whole.ids[1:] >= 16).any()
    for cuts in ((3, 3, 1), (1,) * 7):
        carry, s = None, 0
        for c in cuts:
            part = links_np(labels[s:s + c], dets[s:s + c], counts[s:s + c], [1] * c, 100, carry)
            for f in ("inter", "match", "ids"):
                assert np.array_equal(getattr(part, f)[1 if s == 0 else 0:], getattr(whole, f)[s + (1 if s == 0 else 0):s + c]), (cuts, s, f)
            assert part.linked.tolist() == whole.linked[s:s + c].tolist() and part.seq_tracks[-1] == part.next_id
            carry = tail_np(labels[s + c - 1], dets[s + c - 1], counts[s + c - 1], part.ids[-1], part.next_id)
            s += c
        assert part.next_id == whole.next_id
    img = np.zeros((12, 15, 3), np.uint8)
    out = draw_track_boxes_np(img, [[0, 1, 1, 2, 11, 14], [0, 1, 0, 0, 3, 15], [0, 1, 5, 5, 9, 9]], [12, 1, -1], 1, [(9, 9, 9), (1, 2, 3)])
    assert (out[1, 2:14] == (9, 9, 9)).all() and (out[0] == (1, 2, 3)).all() and (out[2, 3] == (1, 2, 3)).all()  # 12 mod 2 = 0
    assert (out[2, 2] == (9, 9, 9)).all() and (out[2, 13] == (9, 9, 9)).all()  # both boxes' lines: rank 0 stays on top
    assert not out[6, 6].any() and not out[5, 5].any()  # the row without an id is not painted


# ------------------------------------------------------------------------------------------------ arguments and the header ----
LINK_OK = dict(labels=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, dets=256, counts=512, k=16, link=64, c_labels=None, c_h=0,
               c_w=0, c_dets=None, c_counts=None, c_ids=None, c_next=None, permille=100, inter=1024, match=64, ids=128, linked=192, seq=320,
               next_id=448, ws=64, ws_bytes=1 << 20, stream=None)
LINK_ORDER = ("labels n offsets hw max_h max_w total dets counts k link c_labels c_h c_w c_dets c_counts c_ids c_next permille inter match ids "
              "linked seq next_id ws ws_bytes stream").split()
CARRY_OK = dict(c_labels=64, c_h=30, c_w=53, c_dets=256, c_counts=512, c_ids=64, c_next=64)
LINK_BAD = ([dict(**{p: None}) for p in ("labels", "offsets", "hw", "dets", "counts", "link", "inter", "match", "ids", "linked", "seq", "next_id", "ws")] +
            [dict(n=0), dict(n=65536), dict(k=0), dict(k=65), dict(permille=0), dict(permille=1001), dict(max_h=0), dict(max_w=0), dict(total=0),
             dict(ws_bytes=64), dict(ws=66), dict(labels=66), dict(link=65), dict(dets=260), dict(counts=516), dict(inter=1028), dict(ids=130),
             dict(c_labels=64), dict(c_h=30, c_w=53), dict(CARRY_OK, c_ids=None), dict(CARRY_OK, c_next=None), dict(CARRY_OK, c_h=0),
             dict(CARRY_OK, c_dets=260), dict(CARRY_OK, c_ids=66), dict(CARRY_OK, ws_bytes=4 * 3180)])
DRAW_OK = dict(rgb=64, n=2, offsets=64, hw=64, total=3180, dets=256, counts=512, k=16, ids=64, thickness=2, palette=64, p=12, stream=None)
DRAW_BAD = ([dict(**{p: None}) for p in ("rgb", "offsets", "hw", "dets", "counts", "ids", "palette")] +
            [dict(n=0), dict(n=65536), dict(total=0), dict(k=0), dict(k=65), dict(thickness=0), dict(thickness=9), dict(p=0), dict(p=65),
             dict(dets=260), dict(counts=516), dict(ids=66), dict(palette=65)])


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    assert lib.udet_link_detections_workspace_bytes(1000, 2, 16, 0, 0) == 4 * 1000
    assert lib.udet_link_detections_workspace_bytes(1000, 2, 16, 10, 20) == 4 * 1200  # one int32 per pixel, the carried frame's too
    for bad in ((0, 2, 16, 0, 0), (1000, 0, 16, 0, 0), (1000, 2, 0, 0, 0), (1000, 2, 65, 0, 0), (1000, 2, 16, 0, 5), (1000, 2, 16, -1, 5)):
        assert lib.udet_link_detections_workspace_bytes(*bad) == 0
    for change in LINK_BAD:
        a = dict(LINK_OK, **change)
        assert lib.udet_link_detections_ragged(*[a[p] for p in LINK_ORDER]) == -5 and b"link_detections_ragged" in lib.udet_last_error(), change
    for change in DRAW_BAD:
        a = dict(DRAW_OK, **change)
        rc = lib.udet_draw_track_boxes_ragged(a["rgb"], a["n"], a["offsets"], a["hw"], a["total"], a["dets"], a["counts"], a["k"], a["ids"],
                                              a["thickness"], a["palette"], a["p"], a["stream"])
        assert rc == -5 and b"draw_track_boxes_ragged" in lib.udet_last_error(), change


def test_the_header_says_what_the_symbols_do():
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert re.search(r"\bsize_t udet_link_detections_workspace_bytes\(size_t total_pixels, int n, int k, int carry_h, int carry_w\);", hdr)
    assert re.search(r"\bint udet_link_detections_ragged\(const int\* labels, int n, const long long\* offsets, const int\* hw,", hdr)
    assert re.search(r"\bint udet_draw_track_boxes_ragged\(unsigned char\* image_rgb, int n,", hdr)
    assert re.search(r"#define UDET_TRACK_MAX_PALETTE 64\b", hdr)
    for sentence in ("inter > 0 and 1000 inter >= min_iou_permille union", "ties to the smaller a, then to the smaller b",
                     "a matched row inherits ids[p][a]", "comes back under a new id", "Four launches whatever n",
                     "integer atomics only", "nothing enqueued", "a row whose id is -1 is not painted", "the smallest rank wins",
                     "does not depend on the order in which workgroups run"):
        assert sentence in flat, sentence
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7.8" in design and "udet_link_detections_ragged" in design and "gap" in design.lower()
    assert "Out of scope: linking detections into tracks" not in design


def test_wrappers_validate_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd.native_results import (ComponentSelection, Detections, Tracks, TrackTail, link_detections, min_iou_permille,
                                                           track_params)
    from unsupervised_detection_amd.ragged import PackedLayout
    from unsupervised_detection_amd.visualize import TRACK_PALETTE, draw_track_boxes, palette_words
    hw = [(30, 53), (30, 53)]
    total, k = 2 * 30 * 53, 4
    layout = PackedLayout.packed(hw)
    lab = torch.zeros(total, dtype=torch.int32)  # host tensors: anything that got past the validation would fail on them, not launch
    det = Detections(torch.zeros((2, k, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, k)
    tail = TrackTail(torch.zeros(30 * 53, dtype=torch.int32), (30, 53), torch.zeros((k, 9), dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
                     torch.zeros(k, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))

    def bad(match, labels=lab, detections=det, **kw):
        with pytest.raises(ValueError, match=match):
            link_detections(labels, detections, **kw)
    other = ComponentSelection(None, torch.zeros(total + 7, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int64), [7, 7 + 30 * 53], hw)
    bad("packed like the detections", labels=other)                                    # the layouts must be equal
    bad("no labels", labels=ComponentSelection(None, None, torch.zeros((2, 4), dtype=torch.int64), layout, None))
    bad("int32", labels=lab.long())
    bad("PackedLayout|elements", labels=lab[:-1])
    bad("dets must be", detections=Detections(det.dets[:, :, :8], det.counts, layout, 1, k))
    bad("k = 3", carry=TrackTail(tail.labels, (30, 53), tail.dets[:3], tail.counts, tail.ids[:3], tail.next_id))  # k must be equal
    bad("tail\\(\\)", carry={"labels": lab})
    bad("h \\* w", carry=TrackTail(tail.labels[:-1], (30, 53), tail.dets, tail.counts, tail.ids, tail.next_id))
    bad("one 0 / 1 per frame", link=[1])
    bad("one 0 / 1 per frame", link=[1, 2])
    for v in (0.0, 0.0004, 1.0006, -0.1, float("nan"), "x", None, True):
        bad("min_iou", min_iou=v)
    bad("CUDA")  # everything valid but the host tensors: refused before any call into the library
    bad("CUDA", carry=tail, link=[0, 1], min_iou=1.0)
    assert [min_iou_permille(v) for v in (0.1, 0.0006, 1, 0.2504, 0.9996)] == [100, 1, 1000, 250, 1000]
    assert track_params(None) == track_params({}) == {"min_iou": 0.1} and track_params({"min_iou": 0.5}) == {"min_iou": 0.5}
    for t in ({"iou": 0.1}, {"min_iou": 0}, {"min_iou": 2}, [0.1]):
        with pytest.raises(ValueError, match="tracks"):
            track_params(t)
    # draw_track_boxes: host tensors throughout
    assert len(TRACK_PALETTE) == 12 and len(set(TRACK_PALETTE)) == 12 and palette_words([(1, 2, 3)]) == (0x010203,)
    trk = Tracks(*[torch.zeros(s, dtype=d) for s, d in (((2, k, k), torch.int64), ((2, k), torch.int32), ((2, k), torch.int32), (2, torch.int32),
                                                         (2, torch.int32), (1, torch.int32))], lab, det)
    rgb = SimpleNamespace(data=torch.zeros(3 * total, dtype=torch.uint8), layout=PackedLayout(3 * layout.offsets, hw, 3 * total, 3))
    for match, kw in (("thickness", dict(thickness=9)), ("1..64 colours", dict(palette=[])), ("1..64 colours", dict(palette=[(0, 0, 0)] * 65)),
                      ("0..255", dict(palette=[(0, 0, 256)])), ("CUDA", {})):
        with pytest.raises(ValueError, match=match):
            draw_track_boxes(rgb, det, trk, **kw)
    with pytest.raises(ValueError, match="three times their offsets"):
        draw_track_boxes(SimpleNamespace(data=rgb.data[:total], layout=layout), det, trk)
    with pytest.raises(ValueError, match="tracks.ids must be"):
        draw_track_boxes(rgb, det, Tracks(trk.inter, trk.match, trk.ids[:, :3], trk.linked, trk.seq_tracks, trk.next_id, lab, det))
    assert [len(v) for v in trk.rows(0)] == [0, 0] and len(trk) == 2 and trk.tail().hw == (30, 53)


# ------------------------------------------------------------------------------------------------- records and the summary ----
class TracksNp(object):
    """links_np's result with the interface of native_results.Tracks that restore_results_dir and track_records use."""

    def __init__(self, r, labels, detections, carry):
        self.r, self.labels, self.detections, self.carry = r, labels, detections, carry

    def host(self):
        return self.r.inter, self.r.match, self.r.ids, self.r.linked, self.r.seq_tracks

    def tail(self):
        return tail_np(self.labels[-1], self.detections.dets[-1], self.detections.counts[-1], self.r.ids[-1], self.r.next_id)


def link_np(calls):
    """Stand-in for link_detections over the stand-ins of test_detections: links_np on the labels select_labels_np kept."""
    def link(labelled, det, link=None, carry=None, min_iou=0.1):
        from unsupervised_detection_amd.native_results import min_iou_permille
        calls.append((list(link), carry is not None, min_iou))
        return TracksNp(links_np(labelled.labels, det.dets, det.counts, link, min_iou_permille(min_iou), carry), labelled.labels, det, carry)
    return link


def test_track_records_and_summary_arithmetic():
    from unsupervised_detection_amd.native_results import detection_records, summarise_tracks, track_records
    frames, k, permille = hand_cases()["split"]
    frames = frames + [frames[1]]
    labels, dets, counts = inputs_np(frames, k)
    det = DetectionsNp(dets, counts)
    recs = detection_records(det, [255] * 3)
    r = links_np(labels, dets, counts, [1] * 3, permille)
    got = track_records(recs, TracksNp(r, labels, det, None))
    assert [[(d["track"], d["prev"], d["iou"]) for d in f] for f in got] == [[(0, None, None)], [(0, 0, 21 / 36), (1, None, None)], [(0, 0, 1.0), (1, 1, 1.0)]]
    assert all(set(d) == set(recs[0][0]) | {"track", "prev", "iou"} for f in got for d in f) and "track" not in recs[0][0]
    assert {k: v for k, v in got[1][0].items() if k not in ("track", "prev", "iou")} == recs[1][0]
    json.dumps(got)
    # frame 0 linked to a carried frame: the predecessor's area comes from the carry
    carry = tail_np(labels[0], dets[0], counts[0], [5, -1, -1, -1], 9)
    r = links_np(labels[1:], dets[1:], counts[1:], [1, 1], permille, carry)
    got = track_records(recs[1:], TracksNp(r, labels[1:], DetectionsNp(dets[1:], counts[1:]), carry))
    assert [(d["track"], d["prev"], d["iou"]) for d in got[0]] == [(5, 0, 21 / 36), (9, None, None)] and r.next_id == 10
    with pytest.raises(ValueError, match="per frame"):
        track_records(recs, TracksNp(r, labels[1:], DetectionsNp(dets[1:], counts[1:]), carry))
    # the summary: two sequences, the second starts at frame "c"
    rec = lambda t, area, score, box: {"track": t, "area": area, "score": score, "box": box}
    s = summarise_tracks(["a", "b", "c", "d"], [[rec(0, 10, 0.5, [0, 0, 2, 5]), rec(1, 4, 1.0, [5, 5, 7, 7])], [rec(1, 6, 0.5, [5, 5, 8, 7])],
                                                [rec(0, 3, 0.25, [1, 1, 2, 4])], []], [True, False, True, False])
    assert s == [{"first": "a", "frames": 2, "tracks": [
        {"id": 0, "first": "a", "last": "a", "frames": 1, "area_mean": 10.0, "score_mean": 0.5, "boxes": {"a": [0, 0, 2, 5]}},
        {"id": 1, "first": "a", "last": "b", "frames": 2, "area_mean": 5.0, "score_mean": 0.75, "boxes": {"a": [5, 5, 7, 7], "b": [5, 5, 8, 7]}}]},
                 {"first": "c", "frames": 2, "tracks": [
        {"id": 0, "first": "c", "last": "c", "frames": 1, "area_mean": 3.0, "score_mean": 0.25, "boxes": {"c": [1, 1, 2, 4]}}]}]
    with pytest.raises(ValueError):
        summarise_tracks(["a"], [[], []], [True])


# ------------------------------------------------------------------------------------------------------ restore_results_dir ----
def run_tree(tmp_path, name, mixed, batch, **kw):
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_davis_tree(tmp_path / name, mixed, frames=7)
    out = str(tmp_path / name / "native")
    args = dict(restore=speckled_restore_np, load_gt=load_gt_np, score=score_np, batch=batch, verbose=False, connectivity=4)
    args.update(kw)
    return out, restore_results_dir(res, frame_lists_from_reader(davis_flags(root)), out, **args), masks


@pytest.mark.parametrize("mixed", [False, True])
def test_restore_results_dir_with_tracks(tmp_path, mixed):
    calls, calls7 = [], []
    det = dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3})
    out0, js0, masks = run_tree(tmp_path, "det", mixed, 3, **det)
    out, js, _ = run_tree(tmp_path, "trk", mixed, 3, tracks={"min_iou": 0.2}, link=link_np(calls), **det)
    out7, js7, _ = run_tree(tmp_path, "trk7", mixed, 7, tracks={"min_iou": 0.2}, link=link_np(calls7), **det)
    assert calls == [([0, 1, 1], False, 0.2), ([1, 1, 1], True, 0.2), ([1], True, 0.2)] * 2 and calls7 == [([0] + [1] * 6, False, 0.2)] * 2
    assert js["tracks"] == {"min_iou": 0.2} and js == js7
    assert {k: v for k, v in js.items() if k not in ("tracks", "sequences")} == {k: v for k, v in js0.items() if k != "sequences"}
    with open(os.path.join(out, "native_eval.json")) as f:
        assert json.load(f) == json.loads(json.dumps(js))
    f0, f1, f7 = _tree_files(out0), _tree_files(out), _tree_files(out7)
    assert sorted(set(f1) - set(f0)) == [os.path.join("tracks", s + ".json") for s in SEQS]
    changed = {"native_eval.json"} | {os.path.join("detections", s + ".json") for s in SEQS}
    assert all(f0[k] == f1[k] for k in f0 if k not in changed) and all(f0[k] != f1[k] for k in changed)
    assert sorted(f1) == sorted(f7) and all(f1[k] == f7[k] for k in f1)  # batch 3 and batch 7: the same files, byte for byte
    for seq in SEQS:
        stems = ["%05d" % k for k in range(7)]
        frames = [speckled_restore_np(masks[seq][k][None], [frame_hw(seq, k, mixed)], 0.9, 0.5).binary_sample(0) for k in range(7)]
        labels, dets, counts = inputs_np(frames, 3, 2, 4)
        r = links_np(labels, dets, counts, [0] + [1] * 6, 200)
        want_linked = [0] + [0 if mixed and seq == "goat" and k in (1, 2) else 1 for k in range(1, 7)]
        assert r.linked.tolist() == want_linked and (r.match >= 0).sum() >= 4
        with open(os.path.join(out, "detections", seq + ".json")) as f:
            got = json.load(f)
        with open(os.path.join(out0, "detections", seq + ".json")) as f:
            plain = json.load(f)
        assert list(got) == stems
        for i, stem in enumerate(stems):
            assert [{k: v for k, v in d.items() if k not in ("track", "prev", "iou")} for d in got[stem]] == plain[stem]
            assert [d["track"] for d in got[stem]] == r.ids[i, :counts[i, 2]].tolist()
            assert [d["prev"] for d in got[stem]] == [None if a < 0 else a for a in r.match[i, :counts[i, 2]].tolist()]
            for b, d in enumerate(got[stem]):
                a = int(r.match[i, b])
                it = int(r.inter[i, a, b])
                assert d["iou"] == (None if a < 0 else it / (int(dets[i - 1, a, 1]) + int(dets[i, b, 1]) - it))
        with open(os.path.join(out, "tracks", seq + ".json")) as f:
            summary = json.load(f)
        starts = [i for i in range(7) if not want_linked[i]]
        assert [s["first"] for s in summary] == [stems[i] for i in starts] and sum(s["frames"] for s in summary) == 7
        assert [len(s["tracks"]) for s in summary] == [int(v) for v in r.seq_tracks if v] and r.seq_tracks[[i - 1 for i in starts[1:]]].all()
        for s, i0 in zip(summary, starts):
            for t in s["tracks"]:
                where = [(i, b) for i in range(i0, i0 + s["frames"]) for b in range(counts[i, 2]) if r.ids[i, b] == t["id"]]
                assert t["frames"] == len(where) and t["first"] == stems[where[0][0]] and t["last"] == stems[where[-1][0]]
                assert t["area_mean"] == float(np.mean([float(dets[i, b, 1]) for i, b in where]))
                assert t["boxes"] == {stems[i]: [int(dets[i, b, v]) for v in (3, 2, 5, 4)] for i, b in where}
                assert t["score_mean"] == float(np.mean([got[stems[i]][b]["score"] for i, b in where]))
        lengths = [t["frames"] for s in summary for t in s["tracks"]]
        assert js["sequences"][seq]["tracks"] == len(lengths) and js["sequences"][seq]["track_len_mean"] == float(np.mean(lengths))
        assert {k: v for k, v in js["sequences"][seq].items() if k not in ("tracks", "track_len_mean")} == js0["sequences"][seq]
        assert max(lengths) >= 3  # the blob is followed across batches


def test_tracks_paint_the_boxes_by_track(tmp_path):
    painted = []

    def draw(frames, pred, overlay):
        return frames

    def never(*a, **k):
        raise AssertionError("the single-colour call must not run with tracks")

    def draw_track_boxes(overlays, det, trk, boxes):
        painted.append((len(det), trk.host()[2].shape, boxes))
        return overlays

    class Frames(object):
        def __init__(self, paths):
            from PIL import Image
            self.images = [np.asarray(Image.open(p).convert("RGB")) for p in paths]

        def sample(self, i):
            return self.images[i]
    out, js, _ = run_tree(tmp_path, "boxes", False, 4, tracks={}, link=link_np([]), select=select_labels_np([]), detect=detect_np,
                          detections={"min_area": 2, "max_detections": 3}, overlay={"boxes": {"thickness": 1}}, load_images=Frames, draw=draw,
                          draw_boxes=never, draw_track_boxes=draw_track_boxes)
    assert painted == [(4, (4, 3), {"thickness": 1, "colour": (255, 255, 0)}), (3, (3, 3), {"thickness": 1, "colour": (255, 255, 0)})] * 2
    assert js["tracks"] == {"min_iou": 0.1} and js["overlay"]["boxes"]["thickness"] == 1
    assert len(os.listdir(os.path.join(out, "overlay", "bear"))) == 7


def test_tracks_none_changes_nothing(tmp_path):
    """tracks=None (the default): neither callable runs and every file equals a run without the argument; tracks needs detections."""
    def never(*a, **k):
        raise AssertionError("called with tracks=None")
    det = dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3}, component="largest")
    out0, js0, _ = run_tree(tmp_path, "a", True, 3, **det)
    out1, js1, _ = run_tree(tmp_path, "b", True, 3, tracks=None, link=never, draw_track_boxes=never, **det)
    assert js0 == js1 and "tracks" not in js0
    f0, f1 = _tree_files(out0), _tree_files(out1)
    assert sorted(f0) == sorted(f1) and len(f0) == 2 * 14 + 3 and all(f0[k] == f1[k] for k in f0)
    assert not os.path.exists(os.path.join(out1, "tracks"))
    with pytest.raises(ValueError, match="needs detections"):
        run_tree(tmp_path, "c", False, 3, tracks={}, link=never, select=select_np)
    for bad in ({"min_iou": 0}, {"iou": 0.5}):
        with pytest.raises(ValueError, match="tracks"):
            run_tree(tmp_path, "d" + str(len(bad)) + list(bad)[0], False, 3, tracks=bad, link=never, **det)


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    a = cli.parse_restore_results_args(base)
    assert (a.tracks, a.track_min_iou) == (False, 0.1) and cli._tracks(a) is None
    assert cli._tracks(cli.parse_restore_results_args(base + ["--detections"])) is None
    a = cli.parse_restore_results_args(base + ["--detections", "--tracks"])
    assert cli._tracks(a) == {"min_iou": 0.1} and cli._detections(a) == {"min_area": 64, "max_detections": 16}
    assert cli._tracks(cli.parse_restore_results_args(base + ["--detections", "--tracks", "--track_min_iou", "0.35"])) == {"min_iou": 0.35}
    for bad, said in ((["--tracks"], "it needs --detections"), (["--tracks", "--track_min_iou", "0.5"], "it needs --detections"),
                      (["--detections", "--tracks", "--track_min_iou", "0"], "--track_min_iou"),
                      (["--detections", "--tracks", "--track_min_iou", "1.5"], "--track_min_iou")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    d = default_flags()
    assert (d.tracks, d.track_min_iou) == (False, 0.1)
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D"]
    f = parse_flags(native + ["--detections", "--tracks", "--track_min_iou", "0.25"])
    cli.check_native_flags(f)
    assert cli._tracks(f) == {"min_iou": 0.25}
    with pytest.raises(SystemExit) as e:
        cli.check_native_flags(parse_flags(native + ["--tracks"]))
    assert "it needs --detections" in str(e.value)
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R"]
    assert cli._tracks(cli.parse_post_process_args(pp + ["--detections", "--tracks"])) == {"min_iou": 0.1}
    with pytest.raises(SystemExit) as e:
        cli.parse_post_process_args(pp + ["--tracks"])
    assert "it needs --detections" in str(e.value)
    for flag in ("--tracks", "--track_min_iou"):
        assert flag in cli.__doc__
