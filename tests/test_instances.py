"""CPU: the host side of the per-track instance maps (native_results.instance_maps / track_gt_scores, visualize.overlay_instances,
csrc/instances.hip) -- the numpy / scipy restatements of the header's sentences, the hand-built cases, what the random
inputs of the GPU comparison promise, the C entry points' argument checks, the wrappers' host validation, the score arithmetic,
restore_results_dir(instances=...) on numpy stand-ins, the command-line flags and the header's sentences.

instance_maps_np and overlay_instances_np restate include/udet.h sentence by sentence; tests/test_instances_gpu.py compares the kernels
with them for exact equality.  Everything is integers and bytes: no tolerance anywhere."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from test_components import DENSITIES, _tree_files, components_np, ragged_masks
from test_detections import DetectionsNp, detect_np, select_labels_np
from test_native_results import SEQS, frame_hw
from test_track_gaps import bridge_np, link_gap_np
from test_tracks import inputs_np, link_np, links_np, moving_sequence, rects, run_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAP, OTHER = 252, 255
PALETTE = [(166, 206, 227), (31, 120, 180), (178, 223, 138), (51, 160, 44), (251, 154, 153), (227, 26, 28),
           (253, 191, 111), (255, 127, 0), (202, 178, 214), (106, 61, 154), (255, 255, 153), (177, 89, 40)]  # visualize.TRACK_PALETTE, written out


# ------------------------------------------------------------------------------------------------------------ restatement ----
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def instance_maps_np(labels_list, dets, counts, ids, gts=None):
    """include/udet.h, udet_track_instance_maps_ragged, written as its sentences.  labels_list: per frame the [H, W] labels; dets
    [n, k, 9], counts [n, 3], ids [n, k]; gts: None or per frame the [H, W] annotation (foreground where != 0).  Returns (maps: a list of
    uint8 [H, W], row_gt int64 [n, k], frame_stats int64 [n, 3])."""
    dets, counts, ids = _np(dets).astype(np.int64), _np(counts).astype(np.int64), _np(ids).astype(np.int64)
    n, k = ids.shape
    maps, row_gt, stats = [], np.zeros((n, k), np.int64), np.zeros((n, 3), np.int64)
    for i in range(n):
        lab = np.asarray(labels_list[i]).astype(np.int64)
        rows = min(max(int(counts[i, 2]), 0), k)
        inside = (lab >= 1) & (lab <= lab.size)                      # outside the range is background
        m = np.where(inside, OTHER, 0).astype(np.uint8)             # foreground of a component that has no row ... unless:
        g = None if gts is None else np.asarray(gts[i]) != 0
        for r in range(rows):
            comp = inside & (lab - 1 == dets[i, r, 0])
            if ids[i, r] >= 0:
                m[comp] = 1 + ids[i, r] % WRAP
            if g is not None:
                row_gt[i, r] = int((comp & g).sum())
        stats[i] = [int(((m >= 1) & (m <= WRAP)).sum()), int((m == OTHER).sum()), 0 if g is None else int(g.sum())]
        maps.append(m)
    return maps, row_gt, stats


def colour_table(palette=PALETTE, other=(128, 128, 128)):
    """[256, 3]: the colour of every value of the map -- none (zeros) for 0, palette[(v - 1) mod len] for 1..252, `other` for 253..255."""
    lut = np.zeros((256, 3), np.uint8)
    for v in range(1, WRAP + 1):
        lut[v] = palette[(v - 1) % len(palette)]
    lut[WRAP + 1:] = other
    return lut


def overlay_instances_np(img, m, alpha=0.5, beta=0.4, edge=2, palette=PALETTE, other=(128, 128, 128)):
    """include/udet.h, udet_overlay_instances_ragged: two float32 products and a float32 sum, np.rint, saturation, with the pixel's own
    colour; the contour is (v != 0) & ((minimum_filter != v) | (maximum_filter != v)) in mode "nearest", written unblended in the pixel's
    own colour.  Returns (picture, contour)."""
    from scipy.ndimage import maximum_filter, minimum_filter
    m = np.asarray(m, np.uint8)
    own = colour_table(palette, other)[m]
    with np.errstate(over="ignore"):
        a, b = img.astype(np.float32) * np.float32(alpha), own.astype(np.float32) * np.float32(beta)
        t = np.rint(a + b)
    assert a.dtype == b.dtype == t.dtype == np.float32
    out = np.clip(t, 0, 255).astype(np.uint8)
    contour = np.zeros(m.shape, bool)
    if edge >= 1:
        size = 2 * edge + 1
        contour = (m != 0) & ((minimum_filter(m, size, mode="nearest") != m) | (maximum_filter(m, size, mode="nearest") != m))
        out[contour] = own[contour]
    return out, contour


def random_gts(frames, seed=3):
    """One annotation per frame: the frame's own mask rolled by a pixel or two with a block knocked out (so that rows overlap it partly),
    values 0 / 1 / 200 -- anything non-zero is foreground."""
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        g = np.roll(np.asarray(f, np.uint8), (int(rng.integers(0, 2)), int(rng.integers(0, 3))), (0, 1)) * np.uint8(200 if len(out) % 2 else 1)
        h, w = g.shape
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        g[y:y + max(1, h // 4), x:x + max(1, w // 4)] = 0
        out.append(g)
    return out


# ------------------------------------------------------------------------------------------------------- hand-built cases ----
def paint(frames, k, min_area=1, conn=8, ids=None, gts=None):
    labels, dets, counts = inputs_np(frames, k, min_area, conn)
    if ids is None:
        ids = links_np(labels, dets, counts, [1] * len(frames), 100).ids
    return instance_maps_np(labels, dets, counts, np.asarray(ids), gts) + (dets, counts)


def test_the_hand_built_cases_are_what_they_claim():
    s = (8, 18)
    big, small, third = (1, 1, 5, 7), (6, 12, 8, 14), (1, 10, 4, 15)
    f = rects(s, big, small, third)  # 24, 4 and 15 pixels
    # a component below min_area has no row: 255
    maps, _, stats, dets, counts = paint([f], 4, min_area=5)
    assert counts[0].tolist() == [3, 2, 2] and (maps[0][6:8, 12:14] == 255).all() and (maps[0][1:5, 1:7] == 1).all() and (maps[0][1:4, 10:15] == 2).all()
    assert stats[0].tolist() == [24 + 15, 4, 0] and (maps[0][f == 0] == 0).all()
    # more components than k: the extras are 255
    maps, _, stats, dets, counts = paint([f], 2)
    assert counts[0].tolist() == [3, 3, 2] and (maps[0][6:8, 12:14] == 255).all() and stats[0].tolist() == [39, 4, 0]
    maps, _, stats, _, _ = paint([f], 1)
    assert (maps[0][1:4, 10:15] == 255).all() and stats[0].tolist() == [24, 19, 0]
    # a row without an id: 255, and its row_gt is still counted
    gt = rects(s, (0, 0, 3, 12))
    maps, row_gt, stats, dets, _ = paint([f], 4, ids=[[0, -1, 7, -1]], gts=[gt])
    assert (maps[0][1:4, 10:15] == 255).all() and (maps[0][6:8, 12:14] == 8).all() and dets[0, :3, 1].tolist() == [24, 15, 4]
    assert row_gt[0].tolist() == [2 * 6, 2 * 2, 0, 0] and stats[0].tolist() == [28, 15, 36]
    # ids 251, 252, 253 and 504 give 252, 1, 2 and 1
    four = rects(s, (0, 0, 3, 4), (0, 6, 3, 9), (0, 11, 2, 14), (5, 0, 7, 2))
    maps, _, _, dets, _ = paint([four], 4, ids=[[251, 252, 253, 504]])
    assert [int(maps[0].reshape(-1)[int(r)]) for r in dets[0, :, 0]] == [252, 1, 2, 1]
    assert all(colour_table()[1 + i % WRAP].tolist() == list(PALETTE[i % 12]) for i in (0, 11, 12, 251, 252, 253, 504, 100000))  # 252 = 21 * 12
    # a label outside 1..H*W is background
    labels, dets, counts = inputs_np([f], 4)
    lab = labels[0].copy()
    lab[1:5, 1:7] = 8 * 18 + 1
    lab[6:8, 12:14] = -3
    maps, _, stats = instance_maps_np([lab], dets, counts, np.array([[0, 1, 2, -1]]))
    assert (maps[0][1:5, 1:7] == 0).all() and (maps[0][6:8, 12:14] == 0).all() and stats[0].tolist() == [15, 0, 0]
    # two instances that touch diagonally (4-connected labelling): a contour on both sides at edge = 1
    touch = rects((8, 10), (1, 1, 4, 4), (4, 4, 7, 8))
    maps, _, _, dets, counts = paint([touch], 4, conn=4, ids=[[3, 5, -1, -1]])
    m = maps[0]
    assert counts[0, 0] == 2 and m[3, 3] == 6 and m[4, 4] == 4 and dets[0, :2, 1].tolist() == [12, 9]
    img = np.full((8, 10, 3), 100, np.uint8)
    pic, contour = overlay_instances_np(img, m, edge=1)
    assert contour[3, 3] and contour[4, 4] and (pic[3, 3] == PALETTE[5]).all() and (pic[4, 4] == PALETTE[3]).all()
    both = np.array(m, copy=True)
    both[both == 6] = 4  # the same two blobs as ONE value: their inner corners stay a contour (background is a neighbour) ...
    assert overlay_instances_np(img, both, edge=1)[1][3, 3]
    solid = rects((8, 10), (1, 1, 7, 8)).astype(np.uint8)
    solid[solid != 0] = 4
    solid[1:4, 1:4] = 6
    _, c = overlay_instances_np(img, solid, edge=1)
    assert c[3, 2] and c[4, 2] and c[2, 4] and c[2, 3] and not c[5, 5]  # ... and an inner border between two values is a line on both sides
    one = np.where(solid != 0, 4, 0)
    assert not overlay_instances_np(img, one, edge=1)[1][3, 2]          # which one value alone does not have
    assert pic[5, 5].tolist() == [int(np.rint(np.float32(100) * np.float32(0.5) + np.float32(c) * np.float32(0.4))) for c in PALETTE[3]]
    assert pic[0, 0].tolist() == [50, 50, 50]
    # an object on the frame border gets no line along the border
    edge_on = np.zeros((9, 13), np.uint8)
    edge_on[0:6, 0:9] = 7
    _, c = overlay_instances_np(np.zeros((9, 13, 3), np.uint8), edge_on, edge=2)
    assert not c[0, :6].any() and not c[:3, 0].any() and c[5, :9].all() and c[:6, 8].all() and c[3, 7] and not c[3, 6]
    assert not overlay_instances_np(img, m, edge=0)[1].any()
    # 253..255 take the other colour
    assert colour_table()[253].tolist() == colour_table()[254].tolist() == colour_table()[255].tolist() == [128, 128, 128] and not colour_table()[0].any()


def sequences(density):
    """test_tracks_gpu.sequences without its GPU imports: one sequence per size of the GPU test, cut from the largest random frame."""
    sizes = [(1, 1), (1, 70), (67, 1), (9, 13), (33, 65), (130, 259)]
    base = ragged_masks(density)[5]
    frames, link = [], []
    for j, (h, w) in enumerate(sizes):
        seq = moving_sequence(base[:h, :w], 3 + j % 2, 10 + j)
        frames += seq
        link += [0] + [1] * (len(seq) - 1)
    return frames, link


def test_the_random_inputs_exercise_what_they_are_meant_to():
    """What tests/test_instances_gpu.py compares on, asserted on the restatement so that the comparison cannot pass vacuously."""
    hits = 0
    for density in DENSITIES:
        frames, link = sequences(density)
        gts = random_gts(frames)
        for k, min_area, conn in ((1, 1, 8), (16, 2, 4), (64, 1, 4)):
            labels, dets, counts = inputs_np(frames, k, min_area, conn)
            ids = links_np(labels, dets, counts, link, 100).ids
            maps, row_gt, stats = instance_maps_np(labels, dets, counts, ids, gts)
            if k == 1 or min_area == 2:
                assert sum(int((m == OTHER).sum()) for m in maps) >= 1, (density, k)
            if k == 64:
                assert max(len(np.unique(m[m != 0])) for m in maps) >= 3, density
            hits += int((row_gt != 0).sum())
            for i, (m, lab) in enumerate(zip(maps, labels)):
                rows = int(counts[i, 2])
                assert stats[i, 0] == dets[i, :rows, 1].sum(), (density, k, i)
                assert stats[i, 0] + stats[i, 1] == ((lab >= 1) & (lab <= lab.size)).sum(), (density, k, i)
                assert stats[i, 2] == (gts[i] != 0).sum() and (row_gt[i, :rows] <= dets[i, :rows, 1]).all() and not row_gt[i, rows:].any()
            assert not instance_maps_np(labels, dets, counts, ids)[1].any()
    assert hits > 20


# ------------------------------------------------------------------------------------------------ arguments and the header ----
MAPS_OK = dict(labels=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, dets=256, counts=512, k=16, ids=64, gt=None, map=65,
               row_gt=1024, stats=2048, ws=64, ws_bytes=1 << 20, stream=None)
MAPS_ORDER = "labels n offsets hw max_h max_w total dets counts k ids gt map row_gt stats ws ws_bytes stream".split()
MAPS_BAD = ([dict(**{p: None}) for p in ("labels", "offsets", "hw", "dets", "counts", "ids", "map", "row_gt", "stats", "ws")] +
            [dict(n=0), dict(n=65536), dict(k=0), dict(k=65), dict(max_h=0), dict(max_w=0), dict(total=0), dict(ws_bytes=64),
             dict(ws_bytes=4 * 3180 - 1), dict(ws=66), dict(labels=66), dict(ids=65), dict(dets=260), dict(counts=516), dict(row_gt=1028),
             dict(stats=2052)])
OVER_OK = dict(image=64, map=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, alpha=0.5, beta=0.4, palette=64, p=12, other=0x808080,
               edge=2, out=64, stream=None)
OVER_ORDER = "image map n offsets hw max_h max_w total alpha beta palette p other edge out stream".split()
OVER_BAD = ([dict(**{p: None}) for p in ("image", "map", "offsets", "hw", "palette", "out")] +
            [dict(n=0), dict(n=65536), dict(max_h=0), dict(max_w=-3), dict(total=0), dict(edge=-1), dict(alpha=-1.0), dict(alpha=float("nan")),
             dict(alpha=float("inf")), dict(beta=-1e-9), dict(beta=float("nan")), dict(beta=float("inf")), dict(p=0), dict(p=65), dict(palette=66),
             dict(other=0x1000000)])


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    ws = lib.udet_track_instance_maps_workspace_bytes
    assert ws(1000, 2, 16) == 4 * 1000 and ws(1, 1, 1) == 4 and ws(3180, 65535, 64) == 4 * 3180  # at most 4 bytes per pixel
    for bad in ((0, 2, 16), (1000, 0, 16), (1000, 65536, 16), (1000, 2, 0), (1000, 2, 65), (1000, -1, 16)):
        assert ws(*bad) == 0, bad
    for change in MAPS_BAD:
        a = dict(MAPS_OK, **change)
        assert lib.udet_track_instance_maps_ragged(*[a[p] for p in MAPS_ORDER]) == -5 and b"track_instance_maps_ragged" in lib.udet_last_error(), change
    for change in OVER_BAD:
        a = dict(OVER_OK, **change)
        assert lib.udet_overlay_instances_ragged(*[a[p] for p in OVER_ORDER]) == -5 and b"overlay_instances_ragged" in lib.udet_last_error(), change
    assert lib.udet_overlay_instances_ragged(*[dict(OVER_OK, edge=9)[p] for p in OVER_ORDER]) == -4  # UDET_ERR_UNSUPPORTED
    assert b"UDET_OVERLAY_MAX_EDGE" in lib.udet_last_error()


def test_the_header_and_the_documents_say_what_the_symbols_do():
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert re.search(r"\bsize_t udet_track_instance_maps_workspace_bytes\(size_t total_pixels, int n, int k\);", hdr)
    assert re.search(r"\bint udet_track_instance_maps_ragged\(const int\* labels, int n, const long long\* offsets, const int\* hw,", hdr)
    assert re.search(r"\bint udet_overlay_instances_ragged\(const unsigned char\* image_rgb, const unsigned char\* map, int n,", hdr)
    assert re.search(r"#define UDET_INSTANCE_WRAP 252\b", hdr) and re.search(r"#define UDET_INSTANCE_UNASSIGNED 255\b", hdr)
    for sentence in ("map = 1 + (ids[i][r] mod UDET_INSTANCE_WRAP)", "map = UDET_INSTANCE_UNASSIGNED", "outside the range is background",
                     "the values 253 and 254 stay unused", "252 is a multiple of the twelve colours", "Bytes of map between the samples are not written",
                     "integer atomics only", "one LDS atomic per horizontal run of a wave", "aligned 32-bit words of four pixels",
                     "palette[(v - 1) mod palette_size] for v in 1..252 and other_rgb for 253..255", "positions outside the frame never count",
                     "a contour pixel is written in its own colour, unblended", "gets no line along the border", "edge = 0: no contour, no neighbour is read",
                     "One launch, no workspace, no atomics", "rows then columns"):
        assert sentence in flat, sentence
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7.10" in design and "udet_track_instance_maps_ragged" in design and "udet_overlay_instances_ragged" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--instances" in readme and "--overlay_instances" in readme


def test_wrappers_validate_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd import native_results
    from unsupervised_detection_amd.native_results import (INSTANCE_PALETTE_BYTES, ComponentSelection, Detections, InstanceMaps, GtBatch,
                                                           check_instance_arguments, instance_maps, instance_params)
    from unsupervised_detection_amd.ragged import PackedLayout
    from unsupervised_detection_amd.visualize import TRACK_PALETTE, overlay_instances
    assert native_results.instance_maps.__module__.endswith("native_instances") and native_results.INSTANCE_WRAP == WRAP
    assert [tuple(c) for c in TRACK_PALETTE] == PALETTE
    pal = np.frombuffer(INSTANCE_PALETTE_BYTES, np.uint8).reshape(256, 3)
    assert len(INSTANCE_PALETTE_BYTES) == 768 and np.array_equal(pal[:253], colour_table()[:253])  # the picture's colours, but for 253 / 254
    assert not pal[0].any() and not pal[253].any() and not pal[254].any() and pal[255].tolist() == [128, 128, 128] and pal[13].tolist() == list(PALETTE[0])
    hw = [(30, 53), (30, 53)]
    total, k = 2 * 30 * 53, 4
    layout = PackedLayout.packed(hw)
    lab = torch.zeros(total, dtype=torch.int32)  # host tensors: anything that got past the validation would fail on them, not launch
    det = Detections(torch.zeros((2, k, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, k)
    trk = SimpleNamespace(ids=torch.zeros((2, k), dtype=torch.int32))

    def bad(match, labels=lab, detections=det, tracks=trk, **kw):
        with pytest.raises(ValueError, match=match):
            instance_maps(labels, detections, tracks, **kw)
    other = ComponentSelection(None, torch.zeros(total + 7, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int64), [7, 7 + 30 * 53], hw)
    bad("packed like the detections", labels=other)
    bad("int32", labels=lab.long())
    bad("dets must be", detections=Detections(det.dets[:, :, :8], det.counts, layout, 1, k))
    bad("tracks.ids must be", tracks=SimpleNamespace(ids=trk.ids[:, :3]))
    bad("tracks.ids", tracks=SimpleNamespace(ids=trk.ids.long()))
    bad("gt", gt=torch.zeros(total - 1, dtype=torch.uint8))
    bad("gt", gt=torch.zeros(total, dtype=torch.int32))
    bad("packed like the labels", gt=GtBatch(torch.zeros(total + 7, dtype=torch.uint8), [7, 7 + 30 * 53], hw))
    bad("CUDA")  # everything valid but the host tensors: refused before any call into the library
    bad("CUDA", gt=torch.zeros(total, dtype=torch.uint8))
    assert check_instance_arguments(layout, det, trk.ids, None) is None
    wide = Detections(torch.zeros((2, 65, 9), dtype=torch.int64), det.counts, layout, 1, 65)
    with pytest.raises(ValueError, match="k in 1..64"):
        check_instance_arguments(layout, wide, torch.zeros((2, 65), dtype=torch.int32))
    assert instance_params(None) == instance_params({}) == {"overlay": False} and instance_params({"overlay": True}) == {"overlay": True}
    for v in ({"overlay": 1}, {"draw": True}, [True], "yes"):
        with pytest.raises(ValueError, match="instances"):
            instance_params(v)
    # overlay_instances: host tensors throughout
    maps = InstanceMaps(torch.zeros(total, dtype=torch.uint8), torch.zeros((2, k), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout)
    assert tuple(maps.sample(1).shape) == (30, 53) and maps.host()[0].shape == (2, k) and maps.host() is maps.host()
    rgb = SimpleNamespace(data=torch.zeros(3 * total, dtype=torch.uint8), layout=PackedLayout(3 * layout.offsets, hw, 3 * total, 3))
    for match, kw in (("edge", dict(edge=9)), ("alpha", dict(alpha=-1.0)), ("1..64 colours", dict(palette=[])), ("1..64 colours", dict(palette=[(0, 0, 0)] * 65)),
                      ("0..255", dict(other_colour=(0, 0, 256))), ("CUDA", {})):
        with pytest.raises(ValueError, match=match):
            overlay_instances(rgb, maps, **kw)
    with pytest.raises(ValueError, match="three times their offsets"):
        overlay_instances(SimpleNamespace(data=rgb.data[:total], layout=layout), maps)
    with pytest.raises(ValueError, match="no packed instance map"):
        overlay_instances(rgb, SimpleNamespace(layout=layout))


# ------------------------------------------------------------------------------------------------------------ the scores ----
def test_track_gt_scores_by_hand():
    from unsupervised_detection_amd.native_results import track_gt_scores
    rec = lambda t, area: {"track": t, "area": area}
    records = [[rec(0, 10), rec(1, 4)], [rec(1, 6)], [], [rec(0, 5)], [rec(0, 8), rec(2, 2)]]
    row_gt = [[5, 0, 0], [3, 0, 0], [0, 0, 0], [5, 0, 0], [2, 2, 0]]
    gt_area = [10, 6, 0, 5, 4]
    got = track_gt_scores(records, row_gt, gt_area, [True, False, False, True, False])
    # sequence 1, frames 0..2: track 0 = (5 / 15, 0 (no row, gt there), 1 (no row, no gt)); track 1 = (0 / 14, 3 / 9, 1)
    assert got[0] == {"frames": 3, "gt_j_mean": {0: float(np.mean(np.array([5 / 15, 0.0, 1.0]))), 1: float(np.mean(np.array([0.0, 3 / 9, 1.0])))},
                      "best_track": {"id": 0, "gt_j_mean": float(np.mean(np.array([5 / 15, 0.0, 1.0])))}, "best_j": float(np.mean(np.array([5 / 15, 0.0, 1.0])))}
    assert got[0]["gt_j_mean"][0] == got[0]["gt_j_mean"][1]  # (1/3 + 1) / 3 twice: the tie goes to the smaller id
    # sequence 2, frames 3..4: track 0 = (5 / 5, 2 / 10), track 2 = (0, 2 / 4): the first and the last frame count
    assert got[1]["gt_j_mean"] == {0: float(np.mean(np.array([1.0, 0.2]))), 2: 0.25} and got[1]["best_track"] == {"id": 0, "gt_j_mean": 0.6}
    none = track_gt_scores([[], []], [[0], [0]], [0, 3], [True, False])
    assert none == [{"frames": 2, "gt_j_mean": {}, "best_track": None, "best_j": 0.5}]
    with pytest.raises(ValueError, match="per frame"):
        track_gt_scores(records, row_gt[:4], gt_area, [True] * 5)
    with pytest.raises(ValueError, match="more records than rows"):
        track_gt_scores([[rec(0, 1), rec(1, 1)]], [[1]], [1], [True])
    assert "not skipped" in track_gt_scores.__doc__


# ------------------------------------------------------------------------------------------------------ restore_results_dir ----
class InstanceMapsNp(object):
    """instance_maps_np's result with the interface of native_results.InstanceMaps that restore_results_dir uses."""

    def __init__(self, maps, row_gt, stats):
        self.maps, self.row_gt, self.frame_stats = maps, row_gt, stats

    def sample(self, i):
        return self.maps[i]

    def host(self):
        return self.row_gt, self.frame_stats


def paint_np(calls):
    """Stand-in for instance_maps over the stand-ins of test_detections / test_tracks."""
    def paint(labelled, det, trk, gt=None):
        calls.append((len(det), gt is not None))
        return InstanceMapsNp(*instance_maps_np(labelled.labels, det.dets, det.counts, trk.host()[2],
                                                None if gt is None else [gt.sample(i) for i in range(len(det))]))
    return paint


class FramesNp(object):
    """Stand-in for load_images_device: the frames decoded as the device loader decodes them."""

    def __init__(self, paths):
        from unsupervised_detection_amd.data import _read_image
        self.images = [_read_image(p, 3) for p in paths]

    def sample(self, i):
        return self.images[i]


class DrawnNp(object):
    def __init__(self, images):
        self.images = images

    def sample(self, i):
        return self.images[i]


def draw_instances_np(calls):
    def draw(frames, maps, overlay):
        calls.append(len(frames.images))
        return DrawnNp([overlay_instances_np(im, maps.sample(i), overlay["alpha"], overlay["beta"], overlay["edge"])[0]
                        for i, im in enumerate(frames.images)])
    return draw


def never(*a, **k):
    raise AssertionError("must not be called")


def stand_ins(painted, drawn, max_gap=1):
    return dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3},
                tracks={"min_iou": 0.2, "max_gap": max_gap} if max_gap else {"min_iou": 0.2}, link=link_gap_np([]) if max_gap else link_np([]),
                paint=paint_np(painted), draw_instances=draw_instances_np(drawn), load_images=FramesNp, draw=never)


def test_restore_results_dir_with_instances(tmp_path):
    from PIL import Image
    from test_components import speckled_restore_np
    from unsupervised_detection_amd.native_results import INSTANCE_PALETTE_BYTES, track_gt_scores
    painted, drawn = [], []
    base = {k: v for k, v in stand_ins([], [], 0).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    out0, js0, masks = run_tree(tmp_path, "trk", True, 3, **base)
    out, js, _ = run_tree(tmp_path, "inst", True, 3, instances={}, **dict(base, paint=paint_np(painted), draw_instances=never))
    assert painted == [(3, True), (3, True), (1, True)] * 2 and js["instances"] == {"overlay": False}
    f0, f1 = _tree_files(out0), _tree_files(out)
    new = sorted(os.path.join("instances", s, "%05d.png" % k) for s in SEQS for k in range(7))
    changed = {"native_eval.json"} | {os.path.join("tracks", s + ".json") for s in SEQS}
    assert sorted(set(f1) - set(f0)) == new and not set(f0) - set(f1)
    assert all(f0[k] == f1[k] for k in f0 if k not in changed) and all(f0[k] != f1[k] for k in changed)
    # the existing keys keep their order, the new ones follow
    assert list(js)[:len(js0)] == list(js0) and list(js)[len(js0):] == ["instances", "best_track_J"]
    assert {k: v for k, v in js.items() if k not in ("instances", "best_track_J", "sequences")} == {k: v for k, v in js0.items() if k != "sequences"}
    best = []
    for seq in SEQS:
        frames = [speckled_restore_np(masks[seq][k][None], [frame_hw(seq, k, True)], 0.9, 0.5).binary_sample(0) for k in range(7)]
        labels, dets, counts = inputs_np(frames, 3, 2, 4)
        r = links_np(labels, dets, counts, [0] + [1] * 6, 200)
        gts = []
        for k in range(7):
            with Image.open(os.path.join(str(tmp_path), "inst", "DAVIS", "Annotations", "480p", seq, "%05d.png" % k)) as im:
                gts.append((np.asarray(im) / 255.0 > 0.1).astype(np.uint8))
        maps, row_gt, stats = instance_maps_np(labels, dets, counts, r.ids, gts)
        assert (row_gt != 0).sum() >= 5 and sum(int((m == OTHER).sum()) for m in maps) > 0 and stats[:, 2].all()
        for k in range(7):
            with Image.open(os.path.join(out, "instances", seq, "%05d.png" % k)) as im:
                assert im.mode == "P" and bytes(bytearray(im.getpalette())) == INSTANCE_PALETTE_BYTES, (seq, k)
                assert np.array_equal(np.array(im), maps[k]), (seq, k)
        with open(os.path.join(out, "tracks", seq + ".json")) as f:
            summary = json.load(f)
        with open(os.path.join(out0, "tracks", seq + ".json")) as f:
            plain = json.load(f)
        with open(os.path.join(out, "detections", seq + ".json")) as f:
            recs = list(json.load(f).values())
        starts = [not v for v in r.linked]
        want = track_gt_scores(recs, [row_gt[i, :counts[i, 2]].tolist() for i in range(7)], stats[:, 2].tolist(), starts)
        assert len(summary) == len(want) == len(plain)
        for s, p, w in zip(summary, plain, want):
            assert list(s) == list(p) + ["best_track"] and s["best_track"] == w["best_track"] and "wrapped" not in s
            for t, q in zip(s["tracks"], p["tracks"]):
                assert list(t) == list(q) + ["gt_j_mean"] and {k: v for k, v in t.items() if k != "gt_j_mean"} == q
                i0 = int(s["first"])  # the stems are the frames' numbers
                j = np.array([0.0 if stats[i, 2] else 1.0 for i in range(i0, i0 + s["frames"])])
                for i, b in [(i, b) for i in range(i0, i0 + s["frames"]) for b in range(counts[i, 2]) if r.ids[i, b] == t["id"]]:
                    j[i - i0] = row_gt[i, b] / (dets[i, b, 1] + stats[i, 2] - row_gt[i, b])
                assert t["gt_j_mean"] == float(np.mean(j)), (seq, t["id"])
        got = js["sequences"][seq]
        assert list(got)[:len(js0["sequences"][seq])] == list(js0["sequences"][seq]) and list(got)[-2:] == ["unassigned_mean", "best_track_j"]
        assert got["unassigned_mean"] == float(np.mean([u / (a + u) if a + u else 0.0 for a, u, _ in stats.tolist()])) and got["unassigned_mean"] > 0
        assert got["best_track_j"] == float(sum(w["frames"] * w["best_j"] for w in want) / 7)
        best.append(got["best_track_j"])
    assert js["best_track_J"] == float(np.mean(best)) and 0 < js["best_track_J"] < 1
    # with the overlay: draw_instances takes the place of draw, boxes still go on top; with max_gap the maps follow the bridged ids
    painted, drawn, boxed = [], [], []

    def boxes_on_top(overlays, det, trk, boxes):
        boxed.append(len(det))
        return overlays
    out2, js2, _ = run_tree(tmp_path, "drawn", True, 3, instances={"overlay": True}, overlay={"edge": 1, "boxes": {}}, draw_track_boxes=boxes_on_top,
                            **stand_ins(painted, drawn))
    assert drawn == boxed == [3, 3, 1] * 2 and js2["instances"] == {"overlay": True} and js2["overlay"]["edge"] == 1
    with Image.open(os.path.join(out2, "overlay", "bear", "00003.png")) as im:
        pic = np.array(im)
    with Image.open(os.path.join(out2, "instances", "bear", "00003.png")) as im:
        m = np.array(im)
    frame = FramesNp([os.path.join(str(tmp_path), "drawn", "DAVIS", "JPEGImages", "480p", "bear", "00003.jpg")]).images[0]
    assert np.array_equal(pic, overlay_instances_np(frame, m, edge=1)[0]) and len(np.unique(m)) >= 3
    # a wrapped sequence is flagged
    def link_from_252(labelled, det, **kw):
        t = link_np([])(labelled, det, **kw)
        t.r.ids[t.r.ids >= 0] += 252
        return t
    out3, _, _ = run_tree(tmp_path, "wrap", False, 7, instances={}, **dict(base, link=link_from_252, paint=paint_np([])))
    with open(os.path.join(out3, "tracks", "bear.json")) as f:
        assert all(s.get("wrapped") is True for s in json.load(f))


def test_instances_none_changes_nothing(tmp_path):
    """instances=None (the default): neither callable runs and every file equals a run without the argument; instances needs tracks."""
    base = {k: v for k, v in stand_ins([], [], 0).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    out0, js0, _ = run_tree(tmp_path, "a", True, 3, component="largest", **base)
    out1, js1, _ = run_tree(tmp_path, "b", True, 3, component="largest", instances=None, paint=never, draw_instances=never, **base)
    f0, f1 = _tree_files(out0), _tree_files(out1)
    assert js0 == js1 and list(js0) == list(js1) and "instances" not in js0 and "best_track_J" not in js0
    assert sorted(f0) == sorted(f1) and all(f0[k] == f1[k] for k in f0) and not os.path.exists(os.path.join(out1, "instances"))
    no_tracks = {k: v for k, v in base.items() if k not in ("tracks", "link")}
    with pytest.raises(ValueError, match="needs tracks"):
        run_tree(tmp_path, "c", False, 3, instances={}, paint=never, **no_tracks)
    with pytest.raises(ValueError, match="needs overlay"):
        run_tree(tmp_path, "d", False, 3, instances={"overlay": True}, paint=never, **base)
    with pytest.raises(ValueError, match="instances"):
        run_tree(tmp_path, "e", False, 3, instances={"overlay": "yes"}, paint=never, **base)


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    linked = base + ["--detections", "--tracks"]
    a = cli.parse_restore_results_args(linked)
    assert (a.instances, a.overlay_instances) == (False, False) and cli._instances(a) is None
    assert cli._instances(cli.parse_restore_results_args(linked + ["--instances"])) == {"overlay": False}
    assert cli._instances(cli.parse_restore_results_args(linked + ["--instances", "--overlay", "--overlay_instances"])) == {"overlay": True}
    for bad, said in ((["--detections", "--instances"], "it needs --tracks"), (["--instances"], "it needs --tracks"),
                      (["--detections", "--tracks", "--overlay_instances"], "it needs --overlay and --instances"),
                      (["--detections", "--tracks", "--overlay", "--overlay_instances"], "it needs --overlay and --instances"),
                      (["--detections", "--tracks", "--instances", "--overlay_instances"], "it needs --overlay and --instances")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    d = default_flags()
    assert (d.instances, d.overlay_instances) == (False, False)
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--detections", "--tracks"]
    f = parse_flags(native + ["--instances", "--overlay", "--overlay_instances"])
    cli.check_native_flags(f)
    assert cli._instances(f) == {"overlay": True}
    with pytest.raises(SystemExit) as e:
        cli.check_native_flags(parse_flags(["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--detections", "--instances"]))
    assert "it needs --tracks" in str(e.value)
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R", "--detections", "--tracks"]
    assert cli._instances(cli.parse_post_process_args(pp + ["--instances"])) == {"overlay": False}
    with pytest.raises(SystemExit) as e:
        cli.parse_post_process_args(pp + ["--overlay_instances"])
    assert "it needs --overlay and --instances" in str(e.value)
    for flag in ("--instances", "--overlay_instances"):
        assert flag in cli.__doc__
    assert "removed from the exported binary mask" in cli.__doc__.replace("\n", " ")
