"""CPU: the host side of scoring tracks against multi-object annotations (native_objects.object_overlaps / match_tracks,
csrc/objects.hip) -- the numpy restatement of the header's sentences, the hand-built cases with every table written out,
what the random inputs of the GPU comparison promise, match_tracks by hand and against brute force, the C entry point's argument checks,
the wrappers' host validation, the loader's mode rule, restore_results_dir(objects=...) on numpy stand-ins, the command-line flags and
the header's and the documents' sentences.

object_overlaps_np restates include/udet.h sentence by sentence; tests/test_objects_gpu.py compares the kernels with it for exact
equality.  The tables are integers: no tolerance anywhere but the 1e-12 of the float64 sums of the brute-force comparison."""
import itertools
import json
import os
import re
import warnings

import numpy as np
import pytest

from test_components import DENSITIES, _tree_files
from test_detections import detect_np, select_labels_np
from test_instances import never, sequences
from test_native_results import SEQS, frame_hw
from test_tracks import inputs_np, link_np, rects, run_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_OBJECTS = 32


# ------------------------------------------------------------------------------------------------------------ restatement ----
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def object_overlaps_np(labels_list, dets, counts, objects_list, num_objects):
    """include/udet.h, udet_track_object_overlaps_ragged, written as its sentences.  labels_list: per frame the [H, W] labels; dets
    [n, k, 9], counts [n, 3]; objects_list: per frame the [H, W] object bytes; num_objects: O.  Returns (row_obj int64 [n, k, O], obj_area
    int64 [n, O], frame_stats int64 [n, 2])."""
    dets, counts = _np(dets).astype(np.int64), _np(counts).astype(np.int64)
    n, k, O = dets.shape[0], dets.shape[1], int(num_objects)
    row_obj, area, stats = np.zeros((n, k, O), np.int64), np.zeros((n, O), np.int64), np.zeros((n, 2), np.int64)
    for i in range(n):
        lab, obj = np.asarray(labels_list[i]).astype(np.int64), np.asarray(objects_list[i]).astype(np.int64)
        rows = min(max(int(counts[i, 2]), 0), k)
        inside = (lab >= 1) & (lab <= lab.size)                      # outside the range is background
        area[i] = np.bincount(obj.ravel(), minlength=256)[1:O + 1]   # the pixels with object byte o + 1, whatever their label
        for r in range(rows):                                        # entries for r >= rows_i are 0
            comp = inside & (lab - 1 == dets[i, r, 0])               # the pixels whose label is the root of row r ...
            row_obj[i, r] = np.bincount(obj[comp], minlength=256)[1:O + 1]   # ... by their object byte
        stats[i] = [int(((obj >= 1) & (obj <= O)).sum()), int((obj > O).sum())]
    return row_obj, area, stats


def random_objects(frames, num_objects, seed=5):
    """One object map per frame: a coarse grid of 3 x 5 patches of random bytes in 0..O (so that a wave sees runs of every length and a
    component lies under several objects), 4 % of the pixels redrawn from 0..255 -- bytes above O, the void label 255 among them."""
    rng = np.random.default_rng(seed + 31 * num_objects)
    out = []
    for f in frames:
        h, w = np.asarray(f).shape
        coarse = rng.integers(0, num_objects + 1, ((h + 2) // 3, (w + 4) // 5))
        m = np.kron(coarse, np.ones((3, 5), np.int64))[:h, :w].astype(np.uint8)
        speck = rng.random((h, w)) < 0.04
        m[speck] = rng.integers(0, 256, int(speck.sum()), dtype=np.uint8)
        if h * w > 20:
            m.reshape(-1)[int(rng.integers(0, h * w))] = 255
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------------------- hand-built cases ----
def test_the_hand_built_cases_are_what_they_claim():
    s = (8, 18)
    big, third = (1, 1, 5, 7), (1, 10, 4, 15)  # 24 and 15 pixels: ranks 0 and 1
    f = rects(s, big, third)
    labels, dets, counts = inputs_np([f], 4)
    assert counts[0].tolist() == [2, 2, 2] and dets[0, :2, 1].tolist() == [24, 15]
    # two components over three objects; object 2 is split over the two components
    obj = np.zeros(s, np.uint8)
    obj[:, 0:4], obj[:, 4:12], obj[:, 12:18] = 1, 2, 3
    row_obj, area, stats = object_overlaps_np(labels, dets, counts, [obj], 3)
    assert row_obj[0].tolist() == [[12, 12, 0], [0, 6, 9], [0, 0, 0], [0, 0, 0]]  # rows < k: the rows past the frame's are zeros
    assert area[0].tolist() == [32, 64, 48] and stats[0].tolist() == [144, 0]
    # a component under no object
    bare = obj.copy()
    bare[:, 9:] = 0
    row_obj, area, stats = object_overlaps_np(labels, dets, counts, [bare], 3)
    assert row_obj[0].tolist() == [[12, 12, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]] and area[0].tolist() == [32, 40, 0] and stats[0].tolist() == [72, 0]
    # void bytes: above O, 255 among them -- on a component and off it
    void = obj.copy()
    void[1:3, 1:3], void[0, 17], void[7, 5] = 200, 255, 4
    row_obj, area, stats = object_overlaps_np(labels, dets, counts, [void], 3)
    assert row_obj[0].tolist() == [[8, 12, 0], [0, 6, 9], [0, 0, 0], [0, 0, 0]] and area[0].tolist() == [28, 63, 47] and stats[0].tolist() == [138, 6]
    # ... and with O = 4 the byte 4 is an object of one pixel that no row touches; with O = 1 objects 2 and 3 are void
    row_obj, area, stats = object_overlaps_np(labels, dets, counts, [void], 4)
    assert row_obj[0, :, 3].tolist() == [0, 0, 0, 0] and area[0].tolist() == [28, 63, 47, 1] and stats[0].tolist() == [139, 5]
    row_obj, area, stats = object_overlaps_np(labels, dets, counts, [void], 1)
    assert row_obj[0].tolist() == [[8], [0], [0], [0]] and area[0].tolist() == [28] and stats[0].tolist() == [28, 116]
    # k = 1: only the largest component has a row
    labels1, dets1, counts1 = inputs_np([f], 1)
    row_obj, _, _ = object_overlaps_np(labels1, dets1, counts1, [obj], 3)
    assert row_obj[0].tolist() == [[12, 12, 0]]
    # a label outside 1..H*W is background, and counts past k are clamped
    lab = labels[0].copy()
    lab[1:5, 1:7] = 8 * 18 + 1
    wild = counts.copy()
    wild[0, 2] = 99
    row_obj, area, _ = object_overlaps_np([lab], dets, wild, [obj], 3)
    assert row_obj[0, 0].tolist() == [0, 0, 0] and row_obj[0, 1].tolist() == [0, 6, 9] and area[0].tolist() == [32, 64, 48]


def test_the_random_inputs_exercise_what_they_are_meant_to():
    """What tests/test_objects_gpu.py compares on, asserted on the restatement so that the comparison cannot pass vacuously."""
    for density in DENSITIES:
        frames, _ = sequences(density)
        two = False
        for k, min_area, conn, O in ((16, 2, 4, 3), (64, 1, 8, 32), (1, 1, 8, 1)):
            labels, dets, counts = inputs_np(frames, k, min_area, conn)
            objs = random_objects(frames, O)
            row_obj, area, stats = object_overlaps_np(labels, dets, counts, objs, O)
            assert stats[:, 1].sum() > 0, (density, O)                               # every density has some void pixels
            assert any(int(m.max()) == 255 for m in objs) and all(int(m.max()) >= 0 for m in objs)
            if O > 1:
                assert 2 * sum(bool(row_obj[i, :, 1:].any()) for i in range(len(frames))) >= len(frames), (density, k, O)
                two = two or bool(((row_obj != 0).sum(axis=2) >= 2).any())          # some row touches two objects
            for i in range(len(frames)):
                rows = int(counts[i, 2])
                assert (row_obj[i].sum(axis=1)[:rows] <= dets[i, :rows, 1]).all() and not row_obj[i, rows:].any()
                assert (row_obj[i].sum(axis=0) <= area[i]).all() and stats[i].sum() == (objs[i] != 0).sum() and area[i].sum() == stats[i, 0]
        assert two, density


# ------------------------------------------------------------------------------------------------------------- the match ----
def rec(area):
    return {"area": area}


def tables(frames):
    """frames: per frame ({track: (area, [inter per object])}, [object areas]) -> the arguments of match_tracks (rows in the dict's order)."""
    records = [[rec(a) for a, _ in rows.values()] for rows, _ in frames]
    ids = [list(rows) for rows, _ in frames]
    row_obj = [[list(inter) for _, inter in rows.values()] for rows, _ in frames]
    return records, ids, row_obj, [list(a) for _, a in frames]


def stats_of(values, skip_ends):
    from unsupervised_detection_amd.evaluation import davis_statistics
    return davis_statistics(values, skip_ends)


def test_match_tracks_by_hand():
    from unsupervised_detection_amd.native_results import match_tracks
    # two objects and two crossing tracks: greedy per object picks track 0 twice (6/14 > 5/15 and 4/16 > 1/19); one-to-one, 5/15 + 4/16
    # beats 6/14 + 1/19
    frame = ({0: (10, [6, 4]), 1: (10, [5, 1])}, [10, 10])
    got = match_tracks(*tables([frame] * 3), [True, False, False], False)
    assert len(got) == 1 and got[0]["frames"] == 3 and list(got[0]) == ["frames", "objects", "J_mean", "unmatched_tracks"]
    assert {o: v["track"] for o, v in got[0]["objects"].items()} == {1: 1, 2: 0} and got[0]["unmatched_tracks"] == []
    assert got[0]["objects"][1]["J"] == stats_of([5 / 15] * 3, False) and got[0]["objects"][2]["J"] == stats_of([4 / 16] * 3, False)
    assert got[0]["J_mean"] == float(np.mean([got[0]["objects"][1]["J"]["mean"], 0.25])) and got[0]["objects"][1]["frames_annotated"] == 3
    assert list(got[0]["objects"][1]) == ["track", "J", "frames_annotated"] and list(got[0]["objects"][1]["J"]) == ["mean", "recall", "decay"]
    # more objects than tracks: the one track goes where it adds most, the others score the empty prediction
    frame = ({4: (12, [2, 6, 1])}, [5, 8, 3])
    got = match_tracks(*tables([frame] * 2), [True, False], False)[0]
    assert {o: v["track"] for o, v in got["objects"].items()} == {1: None, 2: 4, 3: None}
    assert got["objects"][2]["J"]["mean"] == 6 / 14 and got["objects"][1]["J"]["mean"] == 0.0 and got["J_mean"] == float(np.mean([0.0, 6 / 14, 0.0]))
    # an object absent in some frames: a missing row scores 1 there, a row scores 0 (its pixels are all wrong); unmatched scores 1 there
    frames = [({0: (10, [5, 0])}, [10, 4]), ({0: (8, [0, 0])}, [0, 4]), ({}, [0, 4]), ({0: (10, [10, 0])}, [10, 0])]
    got = match_tracks(*tables(frames), [True, False, False, False], False)[0]
    assert got["objects"][1]["track"] == 0 and got["objects"][1]["J"] == stats_of([5 / 15, 0.0, 1.0, 1.0], False) and got["objects"][1]["frames_annotated"] == 2
    assert got["objects"][2]["track"] is None and got["objects"][2]["J"] == stats_of([0.0, 0.0, 0.0, 1.0], False) and got["objects"][2]["frames_annotated"] == 3
    # skip_ends: the first and the last frame leave, as in the DAVIS table -- here the only frames in which track 0 meets object 1
    got = match_tracks(*tables(frames), [True, False, False, False], True)[0]
    assert got["objects"][1]["track"] is None and got["objects"][1]["J"] == stats_of([0.0, 1.0, 1.0, 0.0], True) and got["objects"][1]["J"]["mean"] == 1.0
    assert got["unmatched_tracks"] == [0]
    # a track with no overlap is never matched, whatever is left; an object without a pixel in the sequence takes no part
    frame = ({0: (10, [7, 0, 0]), 3: (6, [0, 0, 0])}, [9, 0, 5])
    got = match_tracks(*tables([frame] * 3), [True, False, False], False)[0]
    assert sorted(got["objects"]) == [1, 3] and got["objects"][1]["track"] == 0 and got["objects"][3]["track"] is None
    assert got["unmatched_tracks"] == [3] and got["objects"][3]["J"]["mean"] == 0.0
    # two sequences; a sequence of two frames counts no frame under skip_ends: NaN, which the means ignore
    got = match_tracks(*tables([frame] * 5), [True, False, True, False, False], True)
    assert [s["frames"] for s in got] == [2, 3] and np.isnan(got[0]["objects"][1]["J"]["mean"]) and np.isnan(got[0]["J_mean"])
    assert got[0]["objects"][1]["track"] is None and got[1]["objects"][1]["track"] == 0 and got[1]["objects"][1]["J"]["mean"] == 7 / 12
    # a row without an id belongs to no track
    got = match_tracks([[rec(10)]] * 3, [[-1]] * 3, [[[7]]] * 3, [[9]] * 3, [True, False, False], False)[0]
    assert got["objects"][1]["track"] is None and got["unmatched_tracks"] == []
    with pytest.raises(ValueError, match="per frame"):
        match_tracks([[]], [[]], [[]], [[1]], [True, False], False)
    with pytest.raises(ValueError, match="more records than rows"):
        match_tracks([[rec(1), rec(1)]], [[0]], [[[1], [1]]], [[1]], [True], False)


def frame_j(inter, area_t, area_o):
    return 1.0 if area_t + area_o - inter == 0 else inter / (area_t + area_o - inter)


def test_match_tracks_against_brute_force():
    """200 seeded random integer tables, at most 5 tracks and 4 objects: the total of the objects' means is the maximum over all injective
    assignments of objects to tracks (an object may stay unmatched and then scores the empty prediction), and the assignment is valid."""
    from unsupervised_detection_amd.native_results import match_tracks
    rng = np.random.default_rng(2017)
    matched = 0
    for case in range(200):
        T, O, F = int(rng.integers(0, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 7))
        skip = bool(case % 2) and F >= 3
        frames = []
        for _ in range(F):
            area_o = [int(rng.integers(0, 30)) * int(rng.random() < 0.8) for _ in range(O)]
            rows = {}
            for t in rng.permutation(T):
                if rng.random() < 0.7:
                    a = int(rng.integers(1, 40))
                    inter = [int(rng.integers(0, min(a // O, area_o[o]) + 1)) * int(rng.random() < 0.6) for o in range(O)]
                    rows[int(t)] = (a, inter)
            frames.append((rows, area_o))
        got = match_tracks(*tables(frames), [True] + [False] * (F - 1), skip)[0]
        counted = list(range(F))[1:-1] if skip else list(range(F))
        objs = [o for o in range(O) if any(fr[1][o] for fr in frames)]
        assert sorted(got["objects"]) == [o + 1 for o in objs], case

        def mean_j(t, o):
            return float(np.mean([frame_j(*((fr[0][t][1][o], fr[0][t][0]) if t in fr[0] else (0, 0)), fr[1][o]) for fr in (frames[f] for f in counted)]))
        best = -1.0
        for pick in itertools.product([None] + list(range(T)), repeat=len(objs)):
            used = [t for t in pick if t is not None]
            if len(used) == len(set(used)):
                best = max(best, sum(mean_j(t, o) for t, o in zip(pick, objs)))
        total = sum(v["J"]["mean"] for v in got["objects"].values())
        assert abs(total - best) <= 1e-12, (case, total, best)
        taken = [v["track"] for v in got["objects"].values() if v["track"] is not None]
        assert len(taken) == len(set(taken)) and set(taken) <= set(range(T)), case
        for o, v in got["objects"].items():
            if v["track"] is not None:
                assert sum(frames[f][0][v["track"]][1][o - 1] for f in counted if v["track"] in frames[f][0]) > 0, case
            assert v["J"]["mean"] == float(np.mean([mean_j(v["track"], o - 1)])) or abs(v["J"]["mean"] - mean_j(v["track"], o - 1)) <= 1e-15
        seen = {t for fr in frames for t in fr[0]}
        assert got["unmatched_tracks"] == sorted(seen - set(taken)), case
        matched += len(taken)
    assert matched > 150


# ------------------------------------------------------------------------------------------------ arguments and the header ----
OBJ_OK = dict(labels=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, dets=256, counts=512, k=16, objects=65, O=8, row_obj=1024,
              area=2048, stats=4096, ws=64, ws_bytes=1 << 20, stream=None)
OBJ_ORDER = "labels n offsets hw max_h max_w total dets counts k objects O row_obj area stats ws ws_bytes stream".split()
OBJ_BAD = ([dict(**{p: None}) for p in ("labels", "offsets", "hw", "dets", "counts", "objects", "row_obj", "area", "stats", "ws")] +
           [dict(n=0), dict(n=65536), dict(k=0), dict(k=65), dict(O=0), dict(O=33), dict(O=-1), dict(max_h=0), dict(max_w=0), dict(total=0),
            dict(ws_bytes=64), dict(ws_bytes=4 * 3180 - 1), dict(ws=66), dict(labels=66), dict(dets=260), dict(counts=516), dict(row_obj=1028),
            dict(area=2052), dict(stats=4100)])


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    ws = lib.udet_track_object_overlaps_workspace_bytes
    assert ws(1000, 2, 16) == 4 * 1000 and ws(1, 1, 1) == 4 and ws(3180, 65535, 64) == 4 * 3180  # 4 bytes per pixel
    for bad in ((0, 2, 16), (1000, 0, 16), (1000, 65536, 16), (1000, 2, 0), (1000, 2, 65), (1000, -1, 16)):
        assert ws(*bad) == 0, bad
    for change in OBJ_BAD:
        a = dict(OBJ_OK, **change)
        assert lib.udet_track_object_overlaps_ragged(*[a[p] for p in OBJ_ORDER]) == -5 and b"track_object_overlaps_ragged" in lib.udet_last_error(), change


def test_the_header_and_the_documents_say_what_the_symbols_do():
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert re.search(r"\bsize_t udet_track_object_overlaps_workspace_bytes\(size_t total_pixels, int n, int k\);", hdr)
    assert re.search(r"\bint udet_track_object_overlaps_ragged\(const int\* labels, int n, const long long\* offsets, const int\* hw,", hdr)
    assert re.search(r"#define UDET_MAX_OBJECTS 32\b", hdr)
    for sentence in ("0 background, 1..num_objects an annotated object, anything above num_objects \"void\"", "whatever their label",
                     "0 for r >= rows_i", "{pixels with byte in 1..O, pixels with byte > O}", "A label outside 1..H_i*W_i is background",
                     "integer atomics only", "one LDS atomic per horizontal run of a wave", "one coalesced byte load per lane",
                     "Nothing is written per pixel", "num_objects outside 1..UDET_MAX_OBJECTS", "identical from run to run"):
        assert sentence in flat, sentence
    src = open(os.path.join(ROOT, "unsupervised_detection_amd", "csrc", "objects.hip")).read()
    assert "asm" not in src and "det_run_length" in src and "link_enter_roots" in src and "extern __shared__" in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7.13" in design and "udet_track_object_overlaps_ragged" in design and "match_tracks" in design and "obj_count_kernel" in design
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "--objects" in text or "udet_track_object_overlaps_ragged" in text, doc
    assert "--objects_max" in open(os.path.join(ROOT, "README.md")).read()
    assert "udet_track_object_overlaps_ragged" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "objects_bench" in open(os.path.join(ROOT, "profiles", "NOTES.md")).read()


def test_wrappers_validate_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd import native_results
    from unsupervised_detection_amd.native_results import (ComponentSelection, Detections, GtBatch, ObjectOverlaps, check_object_arguments,
                                                           object_overlaps, object_params)
    from unsupervised_detection_amd.ragged import PackedLayout
    assert native_results.object_overlaps.__module__.endswith("native_objects") and native_results.MAX_OBJECTS == MAX_OBJECTS
    hw = [(30, 53), (30, 53)]
    total, k = 2 * 30 * 53, 4
    layout = PackedLayout.packed(hw)
    lab = torch.zeros(total, dtype=torch.int32)  # host tensors: anything that got past the validation would fail on them, not launch
    det = Detections(torch.zeros((2, k, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, k)
    obj = torch.zeros(total, dtype=torch.uint8)

    def bad(match, labels=lab, detections=det, objects=obj, num_objects=3):
        with pytest.raises(ValueError, match=match):
            object_overlaps(labels, detections, objects, num_objects)
    other = ComponentSelection(None, torch.zeros(total + 7, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int64), [7, 7 + 30 * 53], hw)
    bad("packed like the detections", labels=other)
    bad("int32", labels=lab.long())
    bad("dets must be", detections=Detections(det.dets[:, :, :8], det.counts, layout, 1, k))
    bad("objects", objects=None)
    bad("objects", objects=obj[:-1])
    bad("objects", objects=obj.int())
    bad("packed like the labels", objects=GtBatch(torch.zeros(total + 7, dtype=torch.uint8), [7, 7 + 30 * 53], hw))
    for n in (0, 33, -1, 2.0, "3", True, None):
        bad("num_objects", num_objects=n)
    bad("CUDA")  # everything valid but the host tensors: refused before any call into the library
    bad("CUDA", objects=GtBatch(obj, layout))
    assert check_object_arguments(layout, det, obj, 32)[1] == 32 and check_object_arguments(layout, det, GtBatch(obj, layout), np.int64(1))[0] is obj
    wide = Detections(torch.zeros((2, 65, 9), dtype=torch.int64), det.counts, layout, 1, 65)
    with pytest.raises(ValueError, match="k in 1..64"):
        check_object_arguments(layout, wide, obj, 3)
    got = ObjectOverlaps(torch.zeros((2, k, 3), dtype=torch.int64), torch.ones((2, 3), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64), layout, 3)
    assert [t.shape for t in got.host()] == [(2, k, 3), (2, 3), (2, 2)] and got.host() is got.host() and got.host()[1].sum() == 6
    assert object_params(None) == object_params({}) == {"max": 16, "dir": None} and object_params({"max": 32, "dir": "D"}) == {"max": 32, "dir": "D"}
    assert object_params({"max": np.int64(1), "dir": None}) == {"max": 1, "dir": None}
    for v in ({"max": 0}, {"max": 33}, {"max": "4"}, {"max": 2.0}, {"max": True}, {"dir": 3}, {"most": 4}, [4], "yes"):
        with pytest.raises(ValueError, match="objects"):
            object_params(v)


def test_the_loader_reads_ids_and_refuses_other_modes(tmp_path):
    from PIL import Image
    from unsupervised_detection_amd.native_objects import OBJECT_RULES, ObjectRule, read_object_ids
    ids = np.array([[0, 1, 2, 255], [3, 3, 40, 0]], np.uint8)
    p = Image.fromarray(ids, "P")
    p.putpalette([(7 * i) % 256 for i in range(768)])
    p.save(str(tmp_path / "p.png"))
    Image.fromarray(ids, "L").save(str(tmp_path / "l.png"))
    Image.fromarray(np.stack([ids] * 3, axis=2), "RGB").save(str(tmp_path / "rgb.png"))
    for name in ("p.png", "l.png"):
        got = read_object_ids(str(tmp_path / name), 1)
        assert got.dtype == np.uint8 and got.shape == (2, 4, 1) and np.array_equal(got[..., 0], ids), name  # raw indices / values: not binarised
    with pytest.raises(ValueError, match="rgb.png"):
        read_object_ids(str(tmp_path / "rgb.png"), 1)
    assert set(OBJECT_RULES) == {"DAVIS2016", "SEGTRACK", "FBMS"} and all(isinstance(r, ObjectRule) for r in OBJECT_RULES.values())


# ------------------------------------------------------------------------------------------------------ restore_results_dir ----
class ObjectsNp(object):
    """Stand-in for load_objects_device's result."""

    def __init__(self, arrays):
        self.arrays = arrays
        self.max_id = [int(np.max(a, initial=0, where=a != 255)) for a in arrays]

    def sample(self, i):
        return self.arrays[i]


def load_objects_np(calls):
    def load(paths, rule):
        from PIL import Image
        calls.append(list(paths))
        arrays = []
        for p in paths:
            with Image.open(p) as im:
                assert im.mode in ("P", "L"), p
                arrays.append(np.array(im, np.uint8))
        return ObjectsNp(arrays)
    return load


class OverlapsNp(object):
    def __init__(self, tables):
        self.tables = tables

    def host(self):
        return self.tables


def overlaps_np(calls):
    """Stand-in for object_overlaps over the stand-ins of test_detections / test_tracks."""
    def overlaps(labelled, det, ann, num_objects):
        got = object_overlaps_np(labelled.labels, det.dets, det.counts, [ann.sample(i) for i in range(len(det))], num_objects)
        calls.append((len(det), num_objects, got))
        return OverlapsNp(got)
    return overlaps


def write_object_tree(folder, mixed=True, frames=7):
    """<folder>/<sequence>/<frame>.png for the tree of test_native_results.make_davis_tree: the annotated blob cut into object 1 (left) and
    object 2 (right), object 3 in a corner, a void pixel, and in goat's frame 2 a block of id 7; bear as indexed, goat as grey PNGs."""
    from PIL import Image
    for si, seq in enumerate(SEQS):
        os.makedirs(os.path.join(folder, seq))
        for k in range(frames):
            H, W = frame_hw(seq, k, mixed)
            m = np.zeros((H, W), np.uint8)
            x0, x1 = 6 + 5 * k + 3 * si, 30 + 5 * k
            m[4 + 2 * k:20 + k, x0:(x0 + x1) // 2], m[4 + 2 * k:20 + k, (x0 + x1) // 2:x1] = 1, 2
            m[H - 4:H, 0:6], m[0, 1] = 3, 255
            if seq == "goat" and k == 2:
                m[0:2, W - 3:W] = 7
            im = Image.fromarray(m, "P" if si == 0 else "L")
            if si == 0:
                im.putpalette([(37 * i) % 256 for i in range(768)])
            im.save(os.path.join(folder, seq, "%05d.png" % k))


def base_options():
    return dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3}, tracks={"min_iou": 0.2},
                link=link_np([]))


def test_restore_results_dir_with_objects(tmp_path):
    from unsupervised_detection_amd.native_results import match_tracks, objects_summary
    folder = str(tmp_path / "ids")
    write_object_tree(folder)
    loaded, counted, counted7 = [], [], []
    out0, js0, _ = run_tree(tmp_path, "trk", True, 3, **base_options())
    with pytest.warns(UserWarning, match=r"goat.*--objects_max") as caught:
        out, js, _ = run_tree(tmp_path, "obj", True, 3, objects={"max": 4, "dir": folder}, load_objects=load_objects_np(loaded),
                              overlaps=overlaps_np(counted), **base_options())
    assert len([w for w in caught if "objects_max" in str(w.message)]) == 1  # goat's frame 2 alone: one line for its sequence, none for bear
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out7, js7, _ = run_tree(tmp_path, "obj7", True, 7, objects={"max": 4, "dir": folder}, load_objects=load_objects_np([]),
                                overlaps=overlaps_np(counted7), **base_options())
    assert [c[:2] for c in counted] == [(3, 4), (3, 4), (1, 4)] * 2 and [c[:2] for c in counted7] == [(7, 4)] * 2
    assert loaded[0] == [os.path.join(folder, "bear", "%05d.png" % k) for k in range(3)] and len(loaded) == 6
    # batch 3 against batch 7: byte for byte
    f3, f7 = _tree_files(out), _tree_files(out7)
    assert sorted(f3) == sorted(f7) and all(f3[k] == f7[k] for k in f3)
    assert json.loads(json.dumps(js)) == json.loads(json.dumps(js7)) or str(js) == str(js7)
    # against the run without the option: the new files, the changed files, everything else byte for byte
    f0 = _tree_files(out0)
    new = sorted(os.path.join("objects", s + ".json") for s in SEQS)
    changed = {"native_eval.json"} | {os.path.join("tracks", s + ".json") for s in SEQS}
    assert sorted(set(f3) - set(f0)) == new and not set(f0) - set(f3)
    assert all(f0[k] == f3[k] for k in f0 if k not in changed) and all(f0[k] != f3[k] for k in changed)
    # the existing keys keep their order, the new one follows
    assert list(js)[:len(js0)] == list(js0) and list(js)[len(js0):] == ["objects"] and {k: v for k, v in js.items() if k != "objects"} == js0
    assert list(js["objects"]) == ["max", "J", "sequences"] and js["objects"]["max"] == 4 and list(js["objects"]["J"]) == ["mean", "recall", "decay"]
    every = []
    for si, seq in enumerate(SEQS):
        with open(os.path.join(out, "objects", seq + ".json")) as f:
            got = json.load(f)
        with open(os.path.join(out, "tracks", seq + ".json")) as f:
            summary = json.load(f)
        with open(os.path.join(out0, "tracks", seq + ".json")) as f:
            plain = json.load(f)
        with open(os.path.join(out, "detections", seq + ".json")) as f:
            recs = list(json.load(f).values())
        tabs = counted7[si][2]
        starts = [k == 0 or frame_hw(seq, k, True) != frame_hw(seq, k - 1, True) for k in range(7)]
        ids = [[d["track"] for d in r] for r in recs]
        want = match_tracks(recs, ids, [tabs[0][i][:len(r)].tolist() for i, r in enumerate(recs)], tabs[1].tolist(), starts, True)
        assert len(got) == len(want) == len(summary) == len(plain) and sum(s["frames"] for s in got) == 7
        lo = 0
        for g, w, s, p in zip(got, want, summary, plain):
            assert list(g) == ["frames", "objects", "J_mean", "void_pixels", "unmatched_tracks"]
            assert g["void_pixels"] == int(tabs[2][lo:lo + g["frames"], 1].sum()) and g["void_pixels"] >= g["frames"]
            lo += g["frames"]
            assert json.loads(json.dumps({str(o): v for o, v in w["objects"].items()})) == g["objects"] or str(w["objects"]) == str(g["objects"])
            assert g["unmatched_tracks"] == w["unmatched_tracks"]
            taken = {v["track"]: int(o) for o, v in g["objects"].items() if v["track"] is not None}
            assert list(s) == list(p)
            for t, q in zip(s["tracks"], p["tracks"]):
                assert list(t) == list(q) + ["object"] and {k: v for k, v in t.items() if k != "object"} == q
                assert t["object"] == taken.get(t["id"])
            every += [v["J"] for v in w["objects"].values()]
        means = [v["J"]["mean"] for w in want for v in w["objects"].values()]
        assert js["objects"]["sequences"][seq] == float(np.nanmean(means))
        assert any(v["track"] is not None and v["J"]["mean"] > 0.2 for g in got for v in g["objects"].values()), seq
    for key in ("mean", "recall", "decay"):
        vals = np.array([j[key] for j in every], np.float64)
        assert js["objects"]["J"][key] == float(vals[~np.isnan(vals)].mean())
    assert 0 < js["objects"]["J"]["mean"] < 1
    assert np.isnan(objects_summary({"max": 4}, {"a": []})["sequences"]["a"])  # a category without an object: NaN, which the means ignore
    # the frame list's own annotations (no dir): grey files with 255 (void, warns nothing) and one pixel of 20
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, own, _ = run_tree(tmp_path, "own", False, 3, objects={"max": 32}, load_objects=load_objects_np(loaded), overlaps=overlaps_np([]),
                             **base_options())
    assert loaded[-1][0].endswith(os.path.join("Annotations", "480p", "goat", "00006.png")) and own["objects"]["max"] == 32
    with open(os.path.join(str(tmp_path), "own", "native", "objects", "bear.json")) as f:
        got = json.load(f)
    assert list(got[0]["objects"]) == ["20"] and got[0]["objects"]["20"]["frames_annotated"] == 7 and got[0]["void_pixels"] > 7
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        run_tree(tmp_path, "own4", False, 3, objects={"max": 4}, load_objects=load_objects_np([]), overlaps=overlaps_np([]), **base_options())
    lines = [str(w.message) for w in said if "--objects_max" in str(w.message)]
    assert len(lines) == 2 and lines[0].startswith("bear: object ids up to 20") and lines[1].startswith("goat:")  # one line per sequence
    # with instances and follow beside it: the same objects files
    from test_follow import keep_np
    from test_instances import paint_np
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out8, js8, _ = run_tree(tmp_path, "all", True, 3, objects={"max": 4, "dir": folder}, load_objects=load_objects_np([]),
                                overlaps=overlaps_np([]), instances={}, paint=paint_np([]), follow={"rule": "mass"}, keep=keep_np([]),
                                **base_options())
    f8 = _tree_files(out8)
    assert all(f8[k] == f3[k] for k in new) and list(js8)[-1] == "objects" and js8["objects"] == js["objects"]


def test_objects_none_changes_nothing_and_every_refusal_raises(tmp_path):
    """objects=None (the default): neither callable runs and every file equals a run without the argument."""
    from unsupervised_detection_amd.native_results import restore_results_dir
    out0, js0, _ = run_tree(tmp_path, "a", True, 3, **base_options())
    out1, js1, _ = run_tree(tmp_path, "b", True, 3, objects=None, load_objects=never, overlaps=never, **base_options())
    f0, f1 = _tree_files(out0), _tree_files(out1)
    assert js0 == js1 and list(js0) == list(js1) and "objects" not in js0
    assert sorted(f0) == sorted(f1) and all(f0[k] == f1[k] for k in f0) and not os.path.exists(os.path.join(out1, "objects"))
    no_tracks = {k: v for k, v in base_options().items() if k not in ("tracks", "link")}
    with pytest.raises(ValueError, match="needs tracks"):
        run_tree(tmp_path, "c", False, 3, objects={}, load_objects=never, overlaps=never, **no_tracks)
    with pytest.raises(ValueError, match="needs annotations"):
        restore_results_dir("nowhere", {"a": [("a/0.jpg", None), ("a/1.jpg", None)]}, str(tmp_path / "free"), objects={}, load_objects=never,
                            overlaps=never, verbose=False, **base_options())
    for bad in ({"max": 0}, {"max": 33}, {"max": "4"}, {"dirs": "x"}, [4]):
        with pytest.raises(ValueError, match="objects"):
            run_tree(tmp_path, "d%d" % len(str(bad)), False, 3, objects=bad, load_objects=never, overlaps=never, **base_options())
    # objects_dir: a missing file is an error that names it
    folder = str(tmp_path / "ids")
    write_object_tree(folder, mixed=False)
    os.remove(os.path.join(folder, "goat", "00004.png"))
    with pytest.raises(IOError, match=r"goat.00004\.png"):
        run_tree(tmp_path, "e", False, 3, objects={"max": 4, "dir": folder}, load_objects=load_objects_np([]), overlaps=overlaps_np([]),
                 **base_options())


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    linked = base + ["--detections", "--tracks"]
    a = cli.parse_restore_results_args(linked)
    assert (a.objects, a.objects_max, a.objects_dir) == (False, 16, None) and cli._objects(a) is None
    assert cli._objects(cli.parse_restore_results_args(linked + ["--objects"])) == {"max": 16, "dir": None}
    assert cli._objects(cli.parse_restore_results_args(linked + ["--objects", "--objects_max", "32", "--objects_dir", "X"])) == {"max": 32, "dir": "X"}
    for more in (["--instances"], ["--follow", "mass"], ["--track_max_gap", "2"], ["--track_motion"], ["--instances", "--follow", "best_gt"]):
        assert cli._objects(cli.parse_restore_results_args(linked + ["--objects"] + more)) == {"max": 16, "dir": None}, more
    for bad, said in ((["--detections", "--objects"], "it needs --tracks"), (["--objects"], "it needs --tracks"),
                      (["--detections", "--tracks", "--objects_max", "4"], "they need --objects"),
                      (["--detections", "--tracks", "--objects_dir", "X"], "they need --objects"),
                      (["--detections", "--tracks", "--objects", "--objects_max", "0"], "1..32"),
                      (["--detections", "--tracks", "--objects", "--objects_max", "33"], "1..32"),
                      (["--detections", "--tracks", "--objects", "--dataset", "FRAMES"], "no annotations")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    d = default_flags()
    assert (d.objects, d.objects_max, d.objects_dir) == (False, 16, "")
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--detections", "--tracks"]
    f = parse_flags(native + ["--objects", "--objects_max", "8"])
    cli.check_native_flags(f)
    assert cli._objects(f) == {"max": 8, "dir": None}
    with pytest.raises(SystemExit) as e:
        cli.check_native_flags(parse_flags(["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--detections", "--objects"]))
    assert "it needs --tracks" in str(e.value)
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R", "--detections", "--tracks"]
    assert cli._objects(cli.parse_post_process_args(pp + ["--objects", "--objects_dir", "X"])) == {"max": 16, "dir": "X"}
    with pytest.raises(SystemExit) as e:
        cli.parse_post_process_args(pp[:-1] + ["--objects"])
    assert "it needs --tracks" in str(e.value)
    for flag in ("--objects", "--objects_max", "--objects_dir"):
        assert flag in cli.__doc__
    assert "one-to-one" in cli.__doc__.replace("\n", " ")
