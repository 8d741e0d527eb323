"""CPU: the host side of the masks of whole tracks (native_results.follow_tracks / choose_tracks / keep_words, csrc/follow.hip, DESIGN.md
7.11) -- the numpy restatement of the header's definition, the hand-built cases, what the random inputs of the GPU comparison promise, the
C entry points' argument checks, the wrappers' host validation, the choice of tracks by hand, restore_results_dir(follow=...) on numpy
stand-ins, the command-line flags and the header's sentences.

follow_np restates include/udet.h; tests/test_follow_gpu.py compares the kernels with it for exact equality.  Everything is integers and
bytes: no tolerance anywhere."""
import json
import os
import re

import numpy as np
import pytest

from test_components import DENSITIES, _tree_files, speckled_restore_np
from test_instances import instance_maps_np, never, paint_np, random_gts, sequences, stand_ins
from test_native_results import SEQS, frame_hw, load_gt_np, score_np
from test_tracks import inputs_np, links_np, rank_map, rects, run_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 2 ** 64 - 1


# ------------------------------------------------------------------------------------------------------------ restatement ----
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def follow_np(labels_list, dets, counts, keep, gts=None):
    """include/udet.h, udet_follow_tracks_ragged, written as its sentences.  labels_list: per frame the [H, W] labels; dets [n, k, 9],
    counts [n, 3]; keep: n 64-bit words; gts: None or per frame the [H, W] annotation (foreground where != 0).  Returns (masks: a list of
    uint8 [H, W], stats int64 [n, 4])."""
    dets, counts = _np(dets).astype(np.int64), _np(counts).astype(np.int64)
    n, k = dets.shape[:2]
    masks, stats = [], np.zeros((n, 4), np.int64)
    for i in range(n):
        lab = np.asarray(labels_list[i]).astype(np.int64)
        rows = min(max(int(counts[i, 2]), 0), k)
        inside = (lab >= 1) & (lab <= lab.size)                  # L lies in 1..H*W
        rank = rank_map(lab, dets[i], rows)                      # L - 1 is the root of a row r < rows, or -1
        word = int(np.asarray(keep).reshape(-1)[i]) & ONES
        bits = np.array([(word >> r) & 1 for r in range(max(rows, 1))], bool)  # bits at or above rows are never looked at
        kept = inside & (rank >= 0) & bits[np.maximum(rank, 0)]
        g = np.zeros(lab.shape, bool) if gts is None else np.asarray(gts[i]) != 0
        stats[i] = [int(kept.sum()), int((inside & ~kept).sum()), int((kept & g).sum()), int(g.sum())]
        masks.append(kept.astype(np.uint8))
    return masks, stats


def records_of(dets, counts, ids):
    """What choose_tracks reads of track_records' lists: per frame, in rank order, every row's track and area."""
    dets, counts, ids = _np(dets), _np(counts), _np(ids)
    return [[{"track": int(ids[i, r]), "area": int(dets[i, r, 1])} for r in range(min(max(int(counts[i, 2]), 0), dets.shape[1]))]
            for i in range(len(dets))]


def keep_cases(dets, counts, ids, linked, labels=None, gts=None, seed=0):
    """{name: (uint64 [n] keep words, the kept ids per sequence or None)}: all-zero, all-ones (bits at and above the rows included), one
    random bit per frame, random words, and what choose_tracks keeps under every rule (best_gt with labels and gts)."""
    from unsupervised_detection_amd.native_results import choose_tracks, keep_words, track_gt_scores
    dets, counts, ids = _np(dets), _np(counts), _np(ids)
    n, k = ids.shape
    rng = np.random.default_rng(seed)
    cases = {"zeros": (np.zeros(n, np.uint64), None), "ones": (np.full(n, ONES, np.uint64), None),
             "bit": (np.uint64(1) << rng.integers(0, k, n).astype(np.uint64), None), "random": (rng.integers(0, ONES, n, dtype=np.uint64, endpoint=True), None)}
    recs, starts = records_of(dets, counts, ids), [not v for v in linked]
    sums = [[int(v) for v in dets[i, :len(r), 8]] for i, r in enumerate(recs)]
    rules = [("mass", 1), ("area", 2), ("length", 1), ("all", 2)]
    means = None
    if gts is not None:
        _, row_gt, stats = instance_maps_np(labels, dets, counts, ids, gts)
        means = [sc["gt_j_mean"] for sc in track_gt_scores(recs, row_gt.tolist(), stats[:, 2].tolist(), starts)]
        rules.append(("best_gt", 1))
    for rule, min_frames in rules:
        ranks, kept = choose_tracks(recs, sums, starts, rule, min_frames, means)
        cases[rule] = (keep_words(ranks, n), kept)
    return cases


# ------------------------------------------------------------------------------------------------------- hand-built cases ----
def hand_cases():
    """[(name, labels [H, W], dets [1, k, 9], counts [1, 3], keep word, gt or None, the mask, the four counts)]: the hand-built cases, with
    what the definition gives written out by hand.  tests/test_follow_gpu.py feeds the same cases through follow_tracks."""
    s = (8, 10)
    small, large = rects(s, (1, 1, 4, 4)), rects(s, (4, 4, 7, 8))  # they touch diagonally: two components under 4-connectivity
    touch = small | large
    gt = rects(s, (0, 0, 3, 10))
    lab4, dets4, counts4 = (v[0] for v in inputs_np([touch], 4, 1, 4))
    lab1, dets1, counts1 = (v[0] for v in inputs_np([touch], 1, 1, 4))
    assert counts4.tolist() == [2, 2, 2] and dets4[:2, 1].tolist() == [12, 9] and counts1.tolist() == [2, 2, 1]  # the larger one is row 0
    poisoned = lab4.copy()
    poisoned[1:4, 1:4] = 8 * 10 + 1
    poisoned[4, 4:8] = -3
    many, few = counts4.copy(), counts4.copy()
    many[2], few[2] = 99, -5
    cases = [("two touching components, one kept", lab4, dets4, counts4, 0b10, gt, small, [9, 12, 6, 30]),
             ("the other one kept, without gt the last two are 0", lab4, dets4, counts4, 0b01, None, large, [12, 9, 0, 0]),
             ("both kept", lab4, dets4, counts4, 0b11, gt, touch, [21, 0, 6, 30]),
             ("a kept bit above rows", lab4, dets4, counts4, 0b1010, gt, small, [9, 12, 6, 30]),
             ("the highest bit", lab4, dets4, counts4, 0b10 | 1 << 63, gt, small, [9, 12, 6, 30]),
             ("all ones but bit 0", lab4, dets4, counts4, ONES & ~1, gt, small, [9, 12, 6, 30]),
             ("only bits above rows", lab4, dets4, counts4, 0b1100, gt, 0 * touch, [0, 21, 0, 30]),
             ("a row past k: no bit keeps it", lab1, dets1, counts1, ONES, None, large, [12, 9, 0, 0]),
             ("a label out of range is neither kept nor dropped", poisoned, dets4, counts4, ONES, gt, rects(s, (5, 4, 7, 8)), [8, 0, 0, 30]),
             ("an empty keep word", lab4, dets4, counts4, 0, gt, 0 * touch, [0, 21, 0, 30]),
             ("counts above k are clamped", lab4, dets4, many, ONES, None, touch, [21, 0, 0, 0]),
             ("counts below 0 are clamped", lab4, dets4, few, ONES, None, 0 * touch, [0, 21, 0, 0])]
    return [(name, lab, dets[None], counts[None], word, g, np.asarray(m, np.uint8), st) for name, lab, dets, counts, word, g, m, st in cases]


def test_the_hand_built_cases_are_what_they_claim():
    for name, lab, dets, counts, word, gt, mask, st in hand_cases():
        masks, stats = follow_np([lab], dets, counts, [word], None if gt is None else [gt])
        assert np.array_equal(masks[0], mask) and masks[0].dtype == np.uint8 and stats[0].tolist() == st, name


def test_the_random_inputs_exercise_what_they_are_meant_to():
    """What tests/test_follow_gpu.py compares on, asserted on the restatement so that the comparison cannot pass vacuously."""
    for density in DENSITIES:
        frames, link = sequences(density)
        gts = random_gts(frames)
        both = empty_frame = absent = high_bits = hit = False
        for k, min_area, conn in ((1, 1, 8), (16, 2, 4), (64, 1, 4)):
            labels, dets, counts = inputs_np(frames, k, min_area, conn)
            r = links_np(labels, dets, counts, link, 100)
            rows = np.clip(counts[:, 2], 0, k)
            for name, (words, kept_ids) in keep_cases(dets, counts, r.ids, r.linked, labels, gts).items():
                masks, stats = follow_np(labels, dets, counts, words, gts)
                assert np.array_equal(stats[:, 0] + stats[:, 1], [((lab >= 1) & (lab <= lab.size)).sum() for lab in labels]), (density, k, name)
                assert all(stats[i, 0] == sum(int(dets[i, b, 1]) for b in range(rows[i]) if int(words[i]) >> b & 1) for i in range(len(frames)))
                assert np.array_equal(stats[:, 3], [(g != 0).sum() for g in gts]) and (stats[:, 2] <= stats[:, 0]).all()
                assert not follow_np(labels, dets, counts, words)[1][:, 2:].any()
                both |= bool(stats[:, 0].sum() and stats[:, 1].sum())
                hit |= bool(stats[:, 2].sum())
                high_bits |= any(int(words[i]) >> int(rows[i]) for i in range(len(frames)) if rows[i] < 64)
                if kept_ids is not None:
                    empty_frame |= any(not int(words[i]) & ((1 << int(rows[i])) - 1) for i in range(len(frames)))
                    starts = [i for i in range(len(frames)) if not r.linked[i]] + [len(frames)]
                    for ids, lo, hi in zip(kept_ids, starts[:-1], starts[1:]):
                        absent |= any(t not in r.ids[i, :rows[i]] for t in ids for i in range(lo, hi))
        assert both and empty_frame and absent and high_bits and hit, (density, both, empty_frame, absent, high_bits, hit)


# ------------------------------------------------------------------------------------------------ arguments and the header ----
FOLLOW_OK = dict(labels=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, dets=256, counts=512, k=16, keep=64, gt=None, selected=65,
                 stats=2048, ws=64, ws_bytes=1 << 20, stream=None)
FOLLOW_ORDER = "labels n offsets hw max_h max_w total dets counts k keep gt selected stats ws ws_bytes stream".split()
FOLLOW_BAD = ([dict(**{p: None}) for p in ("labels", "offsets", "hw", "dets", "counts", "keep", "selected", "stats", "ws")] +
              [dict(n=0), dict(n=65536), dict(k=0), dict(k=65), dict(max_h=0), dict(max_w=0), dict(total=0), dict(total=-1), dict(total=-2 ** 40),
               dict(ws_bytes=64), dict(ws_bytes=4 * 3180 - 1), dict(ws=66), dict(labels=66), dict(dets=260), dict(counts=516), dict(keep=68),
               dict(stats=2052)])


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    ws = lib.udet_follow_tracks_workspace_bytes
    assert ws(1000, 2, 16) == 4 * 1000 and ws(1, 1, 1) == 4 and ws(3180, 65535, 64) == 4 * 3180  # 4 bytes per pixel, no per-sample term
    for bad in ((0, 2, 16), (1000, 0, 16), (1000, 65536, 16), (1000, 2, 0), (1000, 2, 65), (1000, -1, 16)):
        assert ws(*bad) == 0, bad
    for change in FOLLOW_BAD:
        a = dict(FOLLOW_OK, **change)
        assert lib.udet_follow_tracks_ragged(*[a[p] for p in FOLLOW_ORDER]) == -5 and b"follow_tracks_ragged" in lib.udet_last_error(), change


def test_the_header_and_the_documents_say_what_the_symbol_does():
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert re.search(r"\bsize_t udet_follow_tracks_workspace_bytes\(size_t total_pixels, int n, int k\);", hdr)
    assert re.search(r"\bint udet_follow_tracks_ragged\(const int\* labels, int n, const long long\* offsets, const int\* hw,", hdr)
    for sentence in ("rows_i = min(counts[i][2], k)", "bit r of keep[i] is set", "selected = 0 otherwise", "outside the range is background",
                     "Bits of keep[i] at or above rows_i are ignored", "dropped foreground is a label in range that is not kept",
                     "the last two are 0 when gt is NULL", "Bytes of selected between the samples are not written", "integer atomics only",
                     "one scalar load and a bit test, not a table lookup per pixel", "never zeroed", "aligned 32-bit words of four pixels",
                     "one 64-bit integer atomic per non-zero partial per workgroup", "Two launches whatever n", "nothing enqueued"):
        assert sentence in flat, sentence
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7.11" in design and "udet_follow_tracks_ragged" in design and "bytes per pixel" in design
    for gone in ("it is not built", "a `--component` mode that follows one track", "removing short-lived tracks from the exported binary masks and re-scoring them (a second"):
        assert gone not in design, gone
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--follow" in readme and "--track_min_frames" in readme and "follow_bench.py" in readme
    assert "follow_tracks" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    notes = open(os.path.join(ROOT, "profiles", "NOTES.md")).read()
    assert "follow_paint_kernel" in notes and "inst_paint_kernel" in notes and "tools/follow_bench.py" in notes


def test_wrappers_validate_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd import native_results
    from unsupervised_detection_amd.native_results import (ComponentSelection, Detections, FollowedMasks, GtBatch, check_follow_arguments,
                                                           follow_params, follow_tracks, keep_words)
    from unsupervised_detection_amd.ragged import PackedLayout
    assert native_results.follow_tracks.__module__.endswith("native_follow") and native_results.choose_tracks.__module__.endswith("native_follow")
    hw = [(30, 53), (30, 53)]
    total, k = 2 * 30 * 53, 4
    layout = PackedLayout.packed(hw)
    lab = torch.zeros(total, dtype=torch.int32)  # host tensors: anything that got past the validation would fail on them, not launch
    det = Detections(torch.zeros((2, k, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, k)
    words = keep_words([[0], [1, 3]], 2)
    assert words.dtype == np.uint64 and words.tolist() == [1, 10] and keep_words([[63], []], 2).tolist() == [2 ** 63, 0]

    def bad(match, labels=lab, detections=det, keep=words, **kw):
        with pytest.raises(ValueError, match=match):
            follow_tracks(labels, detections, keep, **kw)
    other = ComponentSelection(None, torch.zeros(total + 7, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int64), [7, 7 + 30 * 53], hw)
    bad("packed like the detections", labels=other)
    bad("no labels", labels=ComponentSelection(None, None, torch.zeros((2, 4), dtype=torch.int64), layout, None))
    bad("int32", labels=lab.long())
    bad("dets must be", detections=Detections(det.dets[:, :, :8], det.counts, layout, 1, k))
    for keep in (words[:1], np.zeros((2, 1), np.uint64), [0.5, 1.0], [-1, 0], torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), None):
        bad("one 64-bit word per frame", keep=keep)
    bad("gt", gt=torch.zeros(total - 1, dtype=torch.uint8))
    bad("gt", gt=torch.zeros(total, dtype=torch.int32))
    bad("packed like the labels", gt=GtBatch(torch.zeros(total + 7, dtype=torch.uint8), [7, 7 + 30 * 53], hw))
    bad("CUDA")  # everything valid but the host tensors: refused before any call into the library
    bad("CUDA", keep=torch.zeros(2, dtype=torch.int64), gt=torch.zeros(total, dtype=torch.uint8))
    kept, gt = check_follow_arguments(layout, det, np.array([ONES, 2 ** 63], np.uint64), None)
    assert gt is None and kept.dtype == torch.int64 and kept.tolist() == [-1, -2 ** 63]  # the same 64 bits
    wide = Detections(torch.zeros((2, 65, 9), dtype=torch.int64), det.counts, layout, 1, 65)
    with pytest.raises(ValueError, match="k in 1..64"):
        check_follow_arguments(layout, wide, words)
    for ranks, n in (([[0]], 2), ([[64], []], 2), ([[-1], []], 2), ([[0.5], []], 2)):
        with pytest.raises(ValueError, match="kept rank"):
            keep_words(ranks, n)
    assert follow_params(None) == follow_params({}) == {"rule": "mass", "min_frames": 1}
    assert follow_params({"rule": "all", "min_frames": 3}) == {"rule": "all", "min_frames": 3}
    for v in ({"rule": "largest"}, {"rule": None}, {"min_frames": None}, {"min_frames": 0}, {"min_frames": 1.5}, {"min_frames": True}, {"frames": 2}, ["mass"], "mass", {"rule": 3}):
        with pytest.raises(ValueError, match="follow"):
            follow_params(v)
    m = FollowedMasks(torch.zeros(total, dtype=torch.uint8), torch.zeros((2, 4), dtype=torch.int64), layout)
    assert tuple(m.binary_sample(1).shape) == (30, 53) and m.data is m.selected and m.host().shape == (2, 4) and m.host() is m.host()
    assert tuple(m.stack([0, 1]).shape) == (2, 30, 53, 1) and len(m) == 2


# --------------------------------------------------------------------------------------------------------------- the choice ----
def test_choose_tracks_by_hand():
    from unsupervised_detection_amd.native_results import choose_tracks
    rec = lambda t, area: {"track": t, "area": area}
    #            frame 0                     frame 1           frame 2        | frame 3     frame 4 (a second sequence)
    records = [[rec(0, 10), rec(1, 40)], [rec(0, 10), rec(2, 5)], [rec(0, 10)], [rec(0, 7)], [rec(1, 7), rec(0, 9)]]
    sums = [[100, 900], [100, 5], [100], [3], [50, 4]]
    starts = [True, False, False, True, False]
    choose = lambda rule, m=1, means=None: choose_tracks(records, sums, starts, rule, m, means)
    # mass: track 1 has 900 in one frame, track 0 has 300 in three; second sequence: track 1 has 50, track 0 has 7
    assert choose("mass") == ([[1], [], [], [], [0]], [[1], [1]])
    # area: 40 against 30 and 5; then 16 against 7
    assert choose("area") == ([[1], [], [], [0], [1]], [[1], [0]])
    # length: 3 frames against 1 and 1; then 2 against 1
    assert choose("length") == ([[0], [0], [0], [0], [1]], [[0], [0]])
    # min_frames removes the otherwise-chosen track: mass and area fall back to track 0; the second sequence keeps its only 2-frame track
    assert choose("mass", 2) == ([[0], [0], [0], [0], [1]], [[0], [0]]) and choose("area", 2) == choose("mass", 2)
    # a sequence with no eligible track keeps nothing
    assert choose("mass", 3) == ([[0], [0], [0], [], []], [[0], []]) and choose("all", 4) == ([[], [], [], [], []], [[], []])
    # all: every eligible track, ranks ascending
    assert choose("all") == ([[0, 1], [0, 1], [0], [0], [0, 1]], [[0, 1, 2], [0, 1]])
    assert choose("all", 2) == ([[0], [0], [0], [0], [1]], [[0], [0]])
    # best_gt: the largest mean; float64
    means = [{0: 0.25, 1: 0.5, 2: 0.5}, {0: 0.1, 1: 0.1}]
    assert choose("best_gt", 1, means) == ([[1], [], [], [0], [1]], [[1], [0]])  # 1 and 2 tie, one frame each: the smaller id; 0 and 1 tie: more frames
    assert choose("best_gt", 2, means) == ([[0], [0], [0], [0], [1]], [[0], [0]])
    # every tie level: equal value -> more frames; equal value and frames -> the smaller id
    tie = [[rec(3, 5), rec(1, 5), rec(2, 4)], [rec(2, 6), rec(4, 5)], [rec(4, 5)]]
    tsums = [[7, 7, 4], [10, 7], [0]]
    assert choose_tracks(tie, tsums, [True, False, False], "mass", 1)[1] == [[2]]             # 14 against 7, 7 and 7
    assert choose_tracks(tie, [[7, 7, 4], [3, 4], [3]], [True, False, False], "mass", 1)[1] == [[2]]  # 7 four times: 2 and 4 have two frames, the smaller id
    assert choose_tracks(tie, [[7, 7, 4], [2, 4], [3]], [True, False, False], "mass", 1)[1] == [[4]]  # 7, 7, 6, 7: 4 has more frames than 1 and 3
    assert choose_tracks(tie, tsums, [True, False, False], "area", 1)[1] == [[2]] and choose_tracks(tie, tsums, [True, False, False], "length", 1)[1] == [[2]]
    assert choose_tracks(tie[:1], tsums[:1], [True], "mass", 1) == ([[1]], [[1]])               # 7 and 7, one frame each: the smaller id, rank 1
    # integers of any size
    big = [[rec(0, 1), rec(1, 1)]]
    assert choose_tracks(big, [[2 ** 70, 2 ** 70 + 1]], [True], "mass", 1)[1] == [[1]]
    assert choose_tracks([], [], [], "mass", 1) == ([], [])
    for args, said in (((records, sums[:4], starts, "mass", 1), "per frame"), ((records, sums, starts, "best_gt", 1), "gt_j_mean"),
                       ((records, sums, starts, "best_gt", 1, means[:1]), "gt_j_mean"), ((records, sums, starts, "largest", 1), "rule"),
                       ((records, sums, starts, "mass", 0), "min_frames"), ((records, [[1]] + sums[1:], starts, "mass", 1), "more records")):
        with pytest.raises(ValueError, match=said):
            choose_tracks(*args)


# ------------------------------------------------------------------------------------------------------ restore_results_dir ----
class FollowedNp(object):
    """follow_np's result with the interface of native_results.FollowedMasks that restore_results_dir uses."""

    def __init__(self, masks, stats):
        self.masks, self.stats = masks, stats

    def binary_sample(self, i):
        return self.masks[i]

    sample = binary_sample

    def stack(self, idx):
        return np.stack([self.masks[i] for i in idx]).astype(np.float32)[..., None]

    def host(self):
        return self.stats


def keep_np(calls):
    """Stand-in for follow_tracks over the stand-ins of test_detections / test_tracks."""
    def keep(labelled, det, words, gt=None):
        calls.append((len(det), [int(w) for w in words], gt is not None))
        return FollowedNp(*follow_np(labelled.labels, det.dets, det.counts, words, None if gt is None else [gt.sample(i) for i in range(len(det))]))
    return keep


def logged(log, **fns):
    """The callables with their names noted in `log` as they are called."""
    def wrap(name, fn):
        def call(*a, **k):
            log.append(name)
            return fn(*a, **k)
        return call
    return {name: wrap(name, fn) for name, fn in fns.items()}


def expected_follow(tmp_path, name, seq, rule, min_frames, k=3, min_area=2, conn=4, permille=200):
    """The followed masks of one sequence of the small tree, from the restatements alone: (masks, stats, kept ids per sequence, gts)."""
    from PIL import Image
    from unsupervised_detection_amd.native_results import choose_tracks, keep_words
    import scipy.io as sio
    from test_detections import boxes_from_labels_np
    res = os.path.join(str(tmp_path), name, "results", seq)
    frames = []
    for kk in range(7):
        m = sio.loadmat(os.path.join(res, "result_%d.mat" % (kk + 1)))["mask"].astype(np.float32)
        frames.append(speckled_restore_np(m[None], [frame_hw(seq, kk, True)], 0.9, 0.5))
    binaries = [f.binary_sample(0) for f in frames]
    labels, dets, counts = inputs_np(binaries, k, min_area, conn)
    for i, f in enumerate(frames):  # detect_np's score: the restored soft bytes
        dets[i], counts[i] = boxes_from_labels_np(labels[i], f.sample(0), min_area, k)
    r = links_np(labels, dets, counts, [0] + [1] * 6, permille)
    gts = []
    for kk in range(7):
        with Image.open(os.path.join(str(tmp_path), name, "DAVIS", "Annotations", "480p", seq, "%05d.png" % kk)) as im:
            gts.append((np.asarray(im) / 255.0 > 0.1).astype(np.uint8))
    recs = records_of(dets, counts, r.ids)
    sums = [[int(v) for v in dets[i, :len(rc), 8]] for i, rc in enumerate(recs)]
    ranks, kept = choose_tracks(recs, sums, [not v for v in r.linked], rule, min_frames)
    words = keep_words(ranks, 7)
    return follow_np(labels, dets, counts, words, gts) + (kept, gts, words)


def test_restore_results_dir_with_follow(tmp_path):
    import scipy.io as sio
    from PIL import Image
    from unsupervised_detection_amd.evaluation import _nanmean
    base = {k: v for k, v in stand_ins([], [], 0).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    out0, js0, _ = run_tree(tmp_path, "trk", True, 3, **base)
    log, kept_calls = [], []
    fns = logged(log, load_gt=load_gt_np, select=base["select"], detect=base["detect"], link=base["link"], score=score_np, keep=keep_np(kept_calls))
    out, js, _ = run_tree(tmp_path, "fol", True, 3, follow={"rule": "mass", "min_frames": 2}, **dict(base, **fns))
    # two passes per category: the loop up to the link for every batch, then load gt, keep, score per held batch (score once per frame shape)
    one = ["load_gt", "select", "detect", "link"] * 3
    assert log[:12] == one and log[12:14] == ["load_gt", "keep"] and log.count("keep") == 6 and log.count("load_gt") == 12
    second = log[12:log.index("select", 12) - 1]  # up to the next category's first load_gt
    assert [c for c in second if c != "score"] == ["load_gt", "keep"] * 3 and second.count("score") == 3
    goat = log[12 + len(second):]
    assert goat[:12] == one and [c for c in goat[12:] if c != "score"] == ["load_gt", "keep"] * 3 and goat[12:].count("score") == 4  # one odd frame
    assert [(n, gt) for n, _, gt in kept_calls] == [(3, True), (3, True), (1, True)] * 2
    # the new keys come after the existing ones
    assert js["follow"] == {"rule": "mass", "min_frames": 2} and list(js)[:len(js0)] == list(js0) and list(js)[len(js0):] == ["follow"]
    f0, f1 = _tree_files(out0), _tree_files(out)
    same = {os.path.join("detections", s + ".json") for s in SEQS}
    assert sorted(f0) == sorted(f1) and all(f0[k] == f1[k] for k in same)
    for seq in SEQS:
        masks, stats, kept, gts, words = expected_follow(tmp_path, "fol", seq, "mass", 2)
        assert [w for _, ws, _ in kept_calls[(0 if seq == "bear" else 3):][:3] for w in ws] == [int(w) for w in words]
        assert sum(int(m.sum()) for m in masks) > 0 and stats[:, 1].sum() > 0  # something is kept and something is dropped
        for k in range(7):
            with Image.open(os.path.join(out, seq, "%05d.png" % k)) as im:
                assert im.mode == "L" and np.array_equal(np.asarray(im), masks[k] * 255), (seq, k)
            mat = sio.loadmat(os.path.join(out, seq, "result_%d.mat" % (k + 1)))
            plain = sio.loadmat(os.path.join(out0, seq, "result_%d.mat" % (k + 1)))
            assert np.array_equal(mat["mask"], masks[k]) and np.array_equal(mat["soft_mask"], plain["soft_mask"]) and np.array_equal(mat["gt_mask"], gts[k])
            assert mat["mask"].dtype == np.uint8 and (mat["mask"] <= plain["mask"]).all()
        j = np.concatenate([score_np(np.stack([gts[k]])[..., None], np.stack([masks[k]])[..., None], 0.008)[0] for k in range(7)])
        assert js["category_iou"][seq] == _nanmean(j.tolist()) and js["category_iou"][seq] != js0["category_iou"][seq]
        got, was = js["sequences"][seq], js0["sequences"][seq]
        assert list(got) == list(was) + ["kept_mean"] and {k: got[k] for k in ("frames", "detections_mean", "tracks", "track_len_mean")} == {
            k: was[k] for k in ("frames", "detections_mean", "tracks", "track_len_mean")}
        assert got["kept_mean"] == float(np.mean([a / (a + b) if a + b else 0.0 for a, b in stats[:, :2].tolist()])) and 0 < got["kept_mean"] < 1
        with open(os.path.join(out, "tracks", seq + ".json")) as fh:
            summary = json.load(fh)
        with open(os.path.join(out0, "tracks", seq + ".json")) as fh:
            plain = json.load(fh)
        assert [list(s) for s in summary] == [list(p) + ["followed"] for p in plain] and [s["followed"] for s in summary] == kept
        assert [{k: v for k, v in s.items() if k != "followed"} for s in summary] == plain
    # with instances the maps are pass 1's, unchanged, and best_gt follows every sequence's best track
    painted = []
    out2, js2, _ = run_tree(tmp_path, "inst", True, 3, instances={}, follow={"rule": "best_gt"}, keep=keep_np([]), paint=paint_np(painted), **base)
    out3, js3, _ = run_tree(tmp_path, "inst0", True, 3, instances={}, paint=paint_np([]), **base)
    f2, f3 = _tree_files(out2), _tree_files(out3)
    assert painted == [(3, True), (3, True), (1, True)] * 2 and sorted(f2) == sorted(f3)
    assert all(f2[k] == f3[k] for k in f2 if k.startswith(("instances", "detections")))
    assert list(js2)[:len(js3)] == list(js3) and list(js2)[len(js3):] == ["follow"] and js2["best_track_J"] == js3["best_track_J"]
    for seq in SEQS:
        with open(os.path.join(out2, "tracks", seq + ".json")) as fh:
            summary = json.load(fh)
        assert all(list(s)[-2:] == ["best_track", "followed"] and s["followed"] == ([s["best_track"]["id"]] if s["best_track"] else []) for s in summary)
        assert list(js2["sequences"][seq])[-2:] == ["best_track_j", "kept_mean"]


def held_bytes(objs, least):
    """Bytes that `objs` keep alive in per-pixel buffers: every distinct tensor of at least `least` elements reachable through their
    attributes."""
    import torch
    seen, todo, done = {}, list(objs), set()
    while todo:
        x = todo.pop()
        if isinstance(x, torch.Tensor):
            if x.numel() >= least:
                seen[x.data_ptr()] = x.numel() * x.element_size()
        elif hasattr(x, "__dict__") and id(x) not in done:
            done.add(id(x))
            todo += list(vars(x).values())
    return sum(seen.values())


def pixel_bytes(objs, total):
    """held_bytes per pixel of a batch of `total` pixels (tensors of at least that many elements)."""
    return held_bytes(objs, total) / total


def test_pass_one_holds_only_what_pass_two_reads(tmp_path, monkeypatch):
    """Between the passes a batch keeps its labels (4 bytes per pixel) and its restored soft bytes (1): not the frames its Tracks was linked
    against (`carry`: up to max_gap + 1 frames of labels per batch), not the overlap tables, not the thresholded mask."""
    import torch
    from unsupervised_detection_amd import native_results as nr
    from unsupervised_detection_amd.ragged import PackedLayout
    seen, linked = [], []
    real = nr._follow_category

    def spy(cat, held, *a):
        seen.extend(held)
        return real(cat, held, *a)
    monkeypatch.setattr(nr, "_follow_category", spy)
    for max_gap in (0, 1):
        del seen[:], linked[:]
        base = {k: v for k, v in stand_ins([], [], max_gap).items() if k not in ("paint", "draw_instances", "load_images", "draw")}

        def link(*a, _link=base["link"], **k):
            linked.append(_link(*a, **k))
            return linked[-1]
        run_tree(tmp_path, "held%d" % max_gap, False, 3, follow={}, keep=keep_np([]), **dict(base, link=link))
        assert len(seen) == len(linked) == 6 and [t.carry is not None for t in linked] == [False, True, True] * 2  # pass 1 did carry ...
        for (s, rows, stems, labelled, det, trk, res), was in zip(seen, linked):
            assert trk is not was and trk.carry is None and trk.host()[2] is was.host()[2]                      # ... and pass 2 holds none of it
            assert len(rows) == len(stems) == len(det) and s in (0, 3, 6)
    # the real containers: 5 bytes per pixel and frame after _held, whatever the batch's Tracks was linked against
    hw, k = [(30, 53)] * 3, 4
    layout = PackedLayout.packed(hw)
    total = layout.numel
    labels = torch.zeros(total, dtype=torch.int32)
    sel = nr.ComponentSelection(None, labels, torch.zeros((3, 4), dtype=torch.int64), layout, None)
    det = nr.Detections(torch.zeros((3, k, 9), dtype=torch.int64), torch.zeros((3, 3), dtype=torch.int64), layout, 1, k)
    history = nr.TrackHistory(torch.zeros((9, 30 * 53), dtype=torch.int32), (30, 53), torch.zeros((9, k, 9), dtype=torch.int64),
                              torch.zeros((9, 3), dtype=torch.int64), torch.zeros((9, k), dtype=torch.int32), torch.zeros((9, k), dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32), 8)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    trk = nr.Tracks(torch.zeros((3, k, k), dtype=torch.int64), z(3, k), z(3, k), z(3), z(3), z(1), labels, det, carry=history, back=z(3, k), prev=z(3, k),
                    gap_inter=torch.zeros((3, 8, k, k), dtype=torch.int64), open=z(3, k), max_gap=8, hist_open=z(9, k))
    res = nr.RestoredMasks(torch.zeros(total, dtype=torch.uint8), torch.zeros(total, dtype=torch.uint8), layout, None, z(3))
    assert pixel_bytes([sel, det, trk, res], total) == 4 + 4 * 9 / 3 + 1 + 1  # what holding the objects as they are would pin
    ht, hr = nr._held(trk, nr.HELD_TRACK_DROPS), nr._held(res, nr.HELD_RESTORED_DROPS)
    assert pixel_bytes([sel, det, ht, hr], total) == 5
    assert ht.carry is None and ht.inter is None and ht.gap_inter is None and ht.hist_open is None and ht.ids is trk.ids and ht.detections is det
    assert hr.binary is None and hr.data is res.data and hr.amax is res.amax and tuple(hr.soft(1).shape) == (30, 53)
    assert trk.carry is history and trk.inter is not None and res.binary is not None  # the originals stay as they are
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**5 bytes per pixel and frame**" in design and "6 bytes per pixel" not in design


def test_follow_draws_in_pass_two_and_reads_the_frames_again(tmp_path):
    from test_instances import DrawnNp, FramesNp
    log = []

    def draw(frames, pred, overlay):
        log.append(("draw", len(frames.images), int(sum(int(pred.binary_sample(i).sum()) for i in range(len(frames.images))))))
        return DrawnNp([np.array(im) for im in frames.images])

    def load_images(paths):
        log.append(("load_images", len(paths)))
        return FramesNp(paths)

    def boxes(overlays, det, trk, b):
        log.append(("boxes", len(det)))
        return overlays
    base = {k: v for k, v in stand_ins([], [], 0).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    out, js, _ = run_tree(tmp_path, "drawn", False, 4, follow={"rule": "length"}, keep=keep_np([]), overlay={"boxes": {}}, draw=draw,
                          load_images=load_images, draw_track_boxes=boxes, **base)
    assert [c[:2] for c in log] == [("load_images", 4), ("draw", 4), ("boxes", 4), ("load_images", 3), ("draw", 3), ("boxes", 3)] * 2
    assert all(c[2] > 0 for c in log if c[0] == "draw") and len(os.listdir(os.path.join(out, "overlay", "bear"))) == 7
    # with the instance overlay the picture is pass 1's: draw never runs, the frames are read once
    log2, drawn = [], []
    both = stand_ins([], drawn, 0)
    out2, _, _ = run_tree(tmp_path, "inst", False, 4, follow={"rule": "all"}, keep=keep_np([]), overlay={}, instances={"overlay": True},
                          **dict(both, load_images=lambda p: (log2.append(len(p)), FramesNp(p))[1]))
    assert drawn == [4, 3] * 2 and log2 == [4, 3] * 2 and len(os.listdir(os.path.join(out2, "overlay", "goat"))) == 7


def test_follow_without_annotations(tmp_path):
    from unsupervised_detection_amd.native_results import restore_results_dir
    from test_native_results import davis_flags, make_davis_tree
    from unsupervised_detection_amd.native_results import frame_lists_from_reader
    root, res, _ = make_davis_tree(tmp_path / "free", False, frames=7)
    lists = {c: [(i, None) for i, _ in e] for c, e in frame_lists_from_reader(davis_flags(root)).items()}
    base = {k: v for k, v in stand_ins([], [], 0).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    calls = []
    args = dict(restore=speckled_restore_np, load_gt=never, score=never, load_sizes=lambda paths: [(30, 53)] * len(paths), batch=3, verbose=False,
                connectivity=4, **base)
    js0 = restore_results_dir(res, lists, str(tmp_path / "free" / "n0"), **args)
    js = restore_results_dir(res, lists, str(tmp_path / "free" / "n1"), follow={}, keep=keep_np(calls), **args)
    assert [gt for _, _, gt in calls] == [False] * 6 and js["follow"] == {"rule": "mass", "min_frames": 1} and js["annotations"] is False
    for seq in SEQS:
        assert 0 < js["sequences"][seq]["foreground_mean"] < js0["sequences"][seq]["foreground_mean"]
        assert list(js["sequences"][seq]) == list(js0["sequences"][seq]) + ["kept_mean"]
    with pytest.raises(ValueError, match="needs instances and annotations"):
        restore_results_dir(res, lists, str(tmp_path / "free" / "n2"), follow={"rule": "best_gt"}, instances={}, paint=never, keep=never, **args)


def test_follow_none_changes_nothing_and_the_refusals(tmp_path):
    """follow=None (the default): keep never runs and every file equals a run without the argument; every refusal the options list."""
    base = {k: v for k, v in stand_ins([], [], 0).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    out0, js0, _ = run_tree(tmp_path, "a", True, 3, component="largest", **base)
    out1, js1, _ = run_tree(tmp_path, "b", True, 3, component="largest", follow=None, keep=never, **base)
    f0, f1 = _tree_files(out0), _tree_files(out1)
    assert js0 == js1 and list(js0) == list(js1) and "follow" not in js0 and "kept_mean" not in js0["sequences"]["bear"]
    assert sorted(f0) == sorted(f1) and all(f0[k] == f1[k] for k in f0)
    no_tracks = {k: v for k, v in base.items() if k not in ("tracks", "link")}
    for name, said, kw in (("c", "needs tracks", dict(no_tracks, follow={})),
                           ("d", "alternative answers", dict(base, follow={}, component="largest")),
                           ("e", "alternative answers", dict(base, follow={"rule": "all"}, component="best_gt")),
                           ("f", "needs instances and annotations", dict(base, follow={"rule": "best_gt"})),
                           ("g", "follow", dict(base, follow={"rule": "largest"})),
                           ("h", "follow", dict(base, follow={"min_frames": 0})),
                           ("i", "follow", dict(base, follow="mass"))):
        with pytest.raises(ValueError, match=said):
            run_tree(tmp_path, name, False, 3, keep=never, **kw)


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    linked = base + ["--detections", "--tracks"]
    a = cli.parse_restore_results_args(linked)
    assert (a.follow, a.track_min_frames) == ("none", 1) and cli._follow(a) is None
    assert cli._follow(cli.parse_restore_results_args(linked + ["--follow", "mass"])) == {"rule": "mass", "min_frames": 1}
    assert cli._follow(cli.parse_restore_results_args(linked + ["--follow", "all", "--track_min_frames", "5"])) == {"rule": "all", "min_frames": 5}
    assert cli._follow(cli.parse_restore_results_args(linked + ["--instances", "--follow", "best_gt"])) == {"rule": "best_gt", "min_frames": 1}
    for bad, said in ((["--detections", "--follow", "mass"], "it needs --tracks"), (["--follow", "length"], "it needs --tracks"),
                      (["--detections", "--tracks", "--follow", "mass", "--component", "largest"], "pass --component none"),
                      (["--detections", "--tracks", "--follow", "best_gt"], "it needs --instances"),
                      (["--detections", "--tracks", "--instances", "--follow", "best_gt", "--dataset", "FRAMES"], "has no annotations"),
                      (["--detections", "--tracks", "--track_min_frames", "2"], "it needs --follow"),
                      (["--detections", "--tracks", "--follow", "mass", "--track_min_frames", "0"], "--track_min_frames")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    with pytest.raises(SystemExit):
        cli.parse_restore_results_args(linked + ["--follow", "largest"])  # argparse: not one of the choices
    d = default_flags()
    assert (d.follow, d.track_min_frames) == ("none", 1)
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--detections", "--tracks"]
    f = parse_flags(native + ["--follow", "area", "--track_min_frames", "3"])
    cli.check_native_flags(f)
    assert cli._follow(f) == {"rule": "area", "min_frames": 3}
    for more, said in ((["--follow", "mass", "--component", "largest"], "pass --component none"), (["--follow", "biggest"], "--follow")):
        with pytest.raises(SystemExit) as e:
            cli.check_native_flags(parse_flags(native + more))
        assert said in str(e.value), more
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R", "--detections", "--tracks"]
    assert cli._follow(cli.parse_post_process_args(pp + ["--follow", "length", "--component", "none"])) == {"rule": "length", "min_frames": 1}
    with pytest.raises(SystemExit) as e:
        cli.parse_post_process_args(pp + ["--follow", "length"])  # post_process's --component defaults to best_gt
    assert "pass --component none" in str(e.value)
    for flag in ("--follow", "--track_min_frames"):
        assert flag in cli.__doc__
    assert "one consistently followed object" in cli.__doc__.replace("\n", " ")
