"""GPU: udet_component_boxes_ragged and udet_draw_boxes_ragged (csrc/detections.hip) through native_results.component_boxes and
visualize.draw_boxes -- dets and counts against the scipy restatement of tests/test_detections.py, the painted frames against its numpy
restatement.  Everything is integer: every comparison is exact equality.  The labels come from the existing labelling call; the frames
are those of tests/test_components_gpu.py (the largest 130 x 259): degenerate and ragged frames in one call, thousands of components
against k = 16 / 64, ties at the cut, a component through every tile, labels that are out of range."""
import json
import os

import numpy as np
import pytest
import torch

from test_components import DENSITIES, checkerboard, corner_blobs, ragged_masks, serpentine
from test_components_gpu import pack
from test_detections import boxes_np, draw_boxes_np, rank_rows, records_np, rows_np, scores_for

pytestmark = pytest.mark.gpu

KS = (1, 16, 64)
MIN_AREAS = (1, 4, 10 ** 6)  # 10^6: more than any frame here has pixels -- nothing is kept, every row is -1, 0, ...


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


_rows = {}


def want(key, masks, scores, conn, min_area, k):
    """The restatement of a batch, (dets [n, k, 9], counts [n, 3]): every component's row computed once per (key, conn) and shared,
    ranked per (min_area, k)."""
    if (key, conn) not in _rows:
        _rows[(key, conn)] = [rows_np(m, s, conn) for m, s in zip(masks, scores if scores is not None else [None] * len(masks))]
    out = [rank_rows(r, min_area, k) for r in _rows[(key, conn)]]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64)


def labelled(masks, conn, gap=0):
    from unsupervised_detection_amd.native_results import select_components
    binary, off, hw = pack(masks, gap)
    return select_components(binary, off, hw, mode="label", connectivity=conn, want_labels=True)


def check_batch(key, masks, conns=(4, 8), ks=KS, min_areas=MIN_AREAS, gap=0):
    from unsupervised_detection_amd.native_results import component_boxes
    scores = scores_for(masks)
    score = pack(scores, gap, 0xA5)[0]
    for conn in conns:
        sel = labelled(masks, conn, gap)
        for k in ks:
            for min_area in min_areas:
                d, c = want(key, masks, scores, conn, min_area, k)
                for sc in (score, None):
                    got = component_boxes(sel, score=sc, min_area=min_area, max_detections=k)
                    dd = d.copy()
                    if sc is None:
                        dd[:, :, 8] = 0
                    assert got.dets.dtype == torch.int64 and tuple(got.dets.shape) == (len(masks), k, 9)
                    assert np.array_equal(got.counts.cpu().numpy(), c), (key, conn, k, min_area)
                    assert np.array_equal(got.dets.cpu().numpy(), dd), (key, conn, k, min_area, sc is None)
                    for i in range(len(masks)):
                        assert np.array_equal(got.rows(i), dd[i, :c[i, 2]])
                if min_area == 10 ** 6:
                    assert (d[:, :, 0] == -1).all() and not d[:, :, 1:].any() and not c[:, 1:].any()


@pytest.mark.parametrize("density", DENSITIES)
def test_degenerate_and_ragged_frames_in_one_call(gpu, density):
    check_batch(("ragged", density), ragged_masks(density))


def test_flat_frames_and_the_hand_built_ones(gpu):
    from unsupervised_detection_amd.native_results import COMPONENT_TILE
    s = serpentine()
    masks = [checkerboard(), s, s.T.copy(), np.ones((67, 131), np.uint8), np.zeros((37, 53), np.uint8), np.zeros((1, 1), np.uint8)] + corner_blobs(*COMPONENT_TILE)
    check_batch("flat", masks)
    d, c = want("flat", masks, None, 4, 1, 64)
    assert c[:6].tolist() == [[980, 980, 64], [1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0]] and c[6:].tolist() == [[2, 2, 2]] * 2
    assert d[1, 0, :6].tolist() == [0, int(s.sum()), 0, 0, 67, 131] and d[3, 0, :6].tolist() == [0, 67 * 131, 0, 0, 67, 131]  # the whole frame
    assert want("flat", masks, None, 8, 1, 64)[1][[0, 6, 7]].tolist() == [[1, 1, 1]] * 3


def test_first_row_is_the_largest_component_of_the_existing_call(gpu):
    from unsupervised_detection_amd.native_results import component_boxes, select_components
    for density in (0.3, 0.593):
        binary, off, hw = pack(ragged_masks(density))
        for conn in (4, 8):
            sel = select_components(binary, off, hw, mode="largest", connectivity=conn, want_labels=True)
            for k in (1, 16):
                got = component_boxes(sel, min_area=1, max_detections=k)
                info = sel.info.cpu().numpy()
                assert np.array_equal(got.dets[:, 0, :2].cpu().numpy(), info[:, 1:3]) and np.array_equal(got.counts[:, 0].cpu().numpy(), info[:, 0])


def test_alone_in_another_order_with_guards_and_twice(gpu):
    from unsupervised_detection_amd.native_results import component_boxes
    masks = ragged_masks(0.593)
    scores = scores_for(masks)
    sel = labelled(masks, 8)
    ref = component_boxes(sel, score=pack(scores)[0], min_area=2, max_detections=16)
    again = component_boxes(sel, score=pack(scores)[0], min_area=2, max_detections=16)
    assert torch.equal(ref.dets, again.dets) and torch.equal(ref.counts, again.counts)
    d, c = want(("ragged", 0.593), masks, scores, 8, 2, 16)
    assert np.array_equal(ref.dets.cpu().numpy(), d) and np.array_equal(ref.counts.cpu().numpy(), c)
    for i in (3, 5):  # a sample alone
        one = component_boxes(labelled([masks[i]], 8), score=pack([scores[i]])[0], min_area=2, max_detections=16)
        assert torch.equal(one.dets[0], ref.dets[i]) and torch.equal(one.counts[0], ref.counts[i])
    order = [5, 0, 3, 2, 4, 1]
    other = component_boxes(labelled([masks[i] for i in order], 8), score=pack([scores[i] for i in order])[0], min_area=2, max_detections=16)
    assert torch.equal(other.dets, ref.dets[order]) and torch.equal(other.counts, ref.counts[order])
    # odd offsets, guard elements between the samples: garbage in the labels' guards is not read
    gap = 37
    g = labelled(masks, 8, gap)
    guard = np.ones(g.labels.numel(), bool)
    for o, (h, w) in zip(g.offsets, g.hw):
        guard[o:o + h * w] = False
    lab = g.labels.cpu().numpy()
    lab[guard] = np.resize(np.array([1, 7, -3, 2 ** 31 - 1, -2 ** 31, 40000], np.int32), int(guard.sum()))
    got = component_boxes(torch.from_numpy(lab).cuda(), score=pack(scores, gap, 0xA5)[0], min_area=2, max_detections=16, offsets=g.layout)
    assert torch.equal(got.dets, ref.dets) and torch.equal(got.counts, ref.counts)


def test_labels_out_of_range_are_background(gpu):
    """Whole components (and background pixels) overwritten with values outside 0..H*W: they vanish, nothing else changes."""
    from unsupervised_detection_amd.native_results import component_boxes
    masks = ragged_masks(0.45)
    scores = scores_for(masks)
    sel = labelled(masks, 4)
    lab = sel.labels.cpu().numpy()
    poison = np.array([2 ** 31 - 1, -1, -2 ** 31], np.int32)
    kept = []
    for i, (o, (h, w)) in enumerate(zip(sel.offsets, sel.hw)):
        v = lab[o:o + h * w]
        roots = np.unique(v[v > 0])
        gone = roots[::3]  # every third component, the first one among them
        m = masks[i].copy().reshape(-1)
        for j, r in enumerate(gone):
            v[v == r] = h * w + 1 if j % 4 == 0 else poison[j % 3]  # H*W + 1: the first value past the range
        m[np.isin(sel.labels.cpu().numpy()[o:o + h * w], gone)] = 0
        bg = np.flatnonzero(v == 0)[::5]
        v[bg] = poison[i % 3]
        kept.append(m.reshape(h, w))
    assert sum(int(a.sum()) for a in kept) < sum(int(a.sum()) for a in masks)
    got = component_boxes(torch.from_numpy(lab).cuda(), score=pack(scores)[0], min_area=1, max_detections=64, offsets=sel.layout)
    out = [boxes_np(m, s, 1, 64, 4) for m, s in zip(kept, scores)]
    assert np.array_equal(got.dets.cpu().numpy(), np.stack([o[0] for o in out]))
    assert got.counts.cpu().numpy().tolist() == [o[1] for o in out]


def test_refused_calls_leave_the_outputs_untouched(gpu):
    from unsupervised_detection_amd._ffi import lib
    masks = ragged_masks(0.45)[3:5]
    sel = labelled(masks, 8)
    n, total = len(sel), sel.labels.numel()
    dets = torch.full((n, 16, 9), -77, dtype=torch.int64, device="cuda")
    counts = torch.full((n, 3), -77, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.udet_component_boxes_workspace_bytes(total, n, 16) // 8 + 1, dtype=torch.int64, device="cuda")
    ok = dict(labels=sel.labels.data_ptr(), score=None, n=n, offsets=sel.dev_offsets.data_ptr(), hw=sel.dev_hw.data_ptr(), max_h=67, max_w=131,
              total=total, min_area=1, k=16, dets=dets.data_ptr(), counts=counts.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 8,
              stream=torch.cuda.current_stream().cuda_stream)
    for change in (dict(labels=None), dict(offsets=None), dict(hw=None), dict(n=0), dict(n=65536), dict(k=0), dict(k=65), dict(min_area=0),
                   dict(ws=None), dict(ws_bytes=ok["ws_bytes"] // 2), dict(ws=ok["ws"] + 4), dict(labels=ok["labels"] + 2), dict(dets=ok["dets"] + 4)):
        a = dict(ok, **change)
        rc = lib.udet_component_boxes_ragged(a["labels"], a["score"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"],
                                             a["min_area"], a["k"], a["dets"], a["counts"], a["ws"], a["ws_bytes"], a["stream"])
        assert rc == -5, change
    torch.cuda.synchronize()
    assert (dets == -77).all() and (counts == -77).all()
    a = ok
    assert lib.udet_component_boxes_ragged(a["labels"], a["score"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"],
                                           a["min_area"], a["k"], a["dets"], a["counts"], a["ws"], a["ws_bytes"], a["stream"]) == 0
    d = [boxes_np(m, None, 1, 16, 8) for m in masks]
    assert np.array_equal(dets.cpu().numpy(), np.stack([o[0] for o in d])) and counts.cpu().numpy().tolist() == [o[1] for o in d]


# ------------------------------------------------------------------------------------------------------------- draw_boxes ----
DRAW_SIZES = [(1, 1), (1, 70), (40, 150), (33, 65), (9, 13), (67, 1)]
GUARD = 0xA5


def hand_boxes():
    """Per sample of DRAW_SIZES a list of (y0, x0, y1, x1): boxes on every border of their frame, narrower than 2 t for t = 2 and 8,
    overlapping, the whole frame; sample 4 has none."""
    return [[(0, 0, 1, 1)],
            [(0, 0, 1, 70), (0, 3, 1, 9)],
            [(0, 0, 40, 150), (0, 10, 12, 30), (28, 120, 40, 150), (5, 0, 35, 20), (8, 5, 25, 60), (20, 40, 38, 140), (10, 70, 13, 75), (30, 2, 31, 149),
             (17, 100, 34, 103)],
            [(0, 0, 33, 65), (16, 32, 33, 65), (0, 64, 33, 65), (32, 0, 33, 65)],
            [],
            [(0, 0, 67, 1), (60, 0, 67, 1)]]


def hand_detections(k, offsets=None, total=None):
    from unsupervised_detection_amd.native_results import Detections
    from unsupervised_detection_amd.ragged import PackedLayout
    boxes = hand_boxes()
    layout = PackedLayout.packed(DRAW_SIZES) if offsets is None else PackedLayout(offsets, DRAW_SIZES, total)
    dets = np.zeros((len(boxes), k, 9), np.int64)
    dets[:, :, 0] = -1
    counts = np.zeros((len(boxes), 3), np.int64)
    for i, bs in enumerate(boxes):
        counts[i] = len(bs)
        for j, (y0, x0, y1, x1) in enumerate(bs):
            dets[i, j, :6] = [y0 * DRAW_SIZES[i][1] + x0, (y1 - y0) * (x1 - x0), y0, x0, y1, x1]
    # a row past the written ones is not drawn, whatever it holds
    dets[4, 0, :6] = [0, 9, 0, 0, 3, 3]
    return Detections(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), layout, 1, k), dets, counts


class Frames(object):
    def __init__(self, images, layout):
        from unsupervised_detection_amd.ragged import PackedLayout
        self.layout = PackedLayout(3 * layout.offsets, layout.hw, 3 * layout.numel, 3)
        buf = np.full(3 * layout.numel, GUARD, np.uint8)
        for o, im in zip(layout.offsets, images):
            buf[3 * o:3 * o + im.size] = im.reshape(-1)
        self.host, self.data = buf, torch.from_numpy(buf).cuda()

    def sample(self, i):
        return self.layout.view(self.data, i)


@pytest.mark.parametrize("thickness", [1, 2, 8])
def test_draw_boxes_equals_the_numpy_restatement(gpu, thickness):
    from unsupervised_detection_amd.visualize import draw_boxes
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in DRAW_SIZES]
    sizes = np.array([h * w for h, w in DRAW_SIZES])
    off = 5 + np.concatenate([[0], np.cumsum(sizes + 5)[:-1]])  # odd offsets, guard bytes before, between and after
    det, dets, counts = hand_detections(16, off, int(off[-1] + sizes[-1] + 5))
    frames = Frames(images, det.layout)
    assert draw_boxes(frames, det, thickness=thickness, colour=(250, 3, 128)) is frames
    got = frames.data.cpu().numpy()
    touched = np.zeros(len(got), bool)
    for i, im in enumerate(images):
        painted = draw_boxes_np(im, dets[i, :counts[i, 2]], thickness, (250, 3, 128))
        assert np.array_equal(frames.sample(i).cpu().numpy(), painted), (i, thickness)
        o = 3 * int(off[i])
        touched[o:o + im.size] = True
        if i == 2:
            line = (painted != im).any(2)
            assert line[0].all() and line[:, 0].all() and line[30, 2:149].all()  # the frame's border; a box one row high
            if thickness == 1:
                assert not line[11, 71:74].any() and not line[21:30, 101].any()  # 3 x 5 and 17 x 3 boxes: a hole at t = 1 ...
            else:
                assert line[10:13, 70:75].all() and line[17:34, 100:103].all()   # ... narrower than 2 t: filled
            if thickness < 8:
                assert not line[20, 12:18].any()
    assert np.array_equal(frames.sample(4).cpu().numpy(), images[4])  # no detection: untouched
    assert (got[~touched] == GUARD).all() and (~touched).sum() == 3 * 5 * 7


def test_draw_boxes_of_real_detections(gpu):
    from unsupervised_detection_amd.native_results import component_boxes
    from unsupervised_detection_amd.visualize import draw_boxes
    masks = ragged_masks(0.3)  # 4-connected: hundreds of components of three pixels or more on the three larger frames
    det = component_boxes(labelled(masks, 4), min_area=3, max_detections=64)
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, m.shape + (3,), dtype=np.uint8) for m in masks]
    frames = Frames(images, det.layout)
    draw_boxes(frames, det)
    for i, im in enumerate(images):
        assert np.array_equal(frames.sample(i).cpu().numpy(), draw_boxes_np(im, det.rows(i))), i
    assert sum(len(det.rows(i)) for i in range(len(masks))) > 64


# ------------------------------------------------------------------------------------------------------------- end to end ----
def test_restore_results_dir_with_detections_and_boxes(gpu, tmp_path):
    """The annotation-free stage on the small tree of test_frames_folder_gpu.py: component "largest", detections and boxes on the
    overlays; the json and the overlay files against the numpy path on what the stage itself restored."""
    import scipy.io as sio
    from PIL import Image
    from test_frames_folder import frames_flags, raises
    from test_frames_folder_gpu import HW, make_tree
    from test_overlay_native_gpu import Packed
    from unsupervised_detection_amd import data
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_masks, restore_results_dir, select_components
    from unsupervised_detection_amd.visualize import overlay_native
    root = make_tree(str(tmp_path / "clips"))
    saved, native = str(tmp_path / "saved"), str(tmp_path / "saved" / "native")
    rng = np.random.default_rng(2)
    for seq in HW:
        os.makedirs(os.path.join(saved, seq))
        for k in range(4):
            m = (0.2 * rng.random((24, 32))).astype(np.float32)
            m[3 + k:12, 4:14 + k] += 0.7    # three blobs of different sizes, one of them small
            m[15:21, 18 + k:27] += 0.7
            m[4:6, 22:25] += 0.7
            sio.savemat(os.path.join(saved, seq, "result_%d.mat" % (k + 1)), {"pred_mask": m})
    seen = []

    def restore(*a, **kw):
        seen.append([restore_masks(*a, **kw)])
        return seen[-1][0]

    def select(pred, **kw):
        seen[-1].append((pred.binary.clone(), kw))
        return select_components(pred, **kw)
    lists = frame_lists_from_reader(frames_flags(root))
    js = restore_results_dir(saved, lists, native, mask_key="pred_mask", batch=3, component="largest", connectivity=4, restore=restore, select=select,
                             detections={"min_area": 12, "max_detections": 2}, overlay={"boxes": {"thickness": 1, "colour": (9, 8, 7)}},
                             load_gt=raises, score=raises, verbose=False, gt_rule="FRAMES")
    assert js["detections"] == {"min_area": 12, "max_detections": 2, "connectivity": 4} and js["overlay"]["boxes"] == {"thickness": 1, "colour": (9, 8, 7)}
    assert all(len(b) == 2 and b[1][1] == {"gt": None, "mode": "largest", "connectivity": 4, "want_labels": True} for b in seen)  # labelled once
    assert sorted(os.listdir(os.path.join(native, "detections"))) == ["a.json", "b.json"]
    batches = iter(seen)
    for seq, sizes in HW.items():
        with open(os.path.join(native, "detections", seq + ".json")) as f:
            got = json.load(f)
        assert list(got) == ["frame_%d" % (k + 9) for k in range(4)]
        counts = []
        for k, (h, w) in enumerate(sizes):
            if k % 3 == 0:
                res, (binary, _) = next(batches)
            stem, i = "frame_%d" % (k + 9), k % 3
            b = res.layout.view(binary, i).cpu().numpy()
            rows, c = boxes_np(b, res.sample(i).cpu().numpy(), 12, 2, 4)
            assert c[0] >= 3 and c[2] == 2 and b.shape == (h, w)  # three blobs, the two largest reported
            assert got[stem] == json.loads(json.dumps(records_np(rows[:c[2]], int(res.amax[i])))), (seq, stem)
            counts.append(int(c[2]))
            with Image.open(os.path.join(native, seq, stem + ".png")) as im:
                mask = np.array(im)
            assert int((mask != 0).sum()) == rows[0, 1]  # the mask is the first detection: the largest component
            frame = data._read_image(os.path.join(root, seq, stem + ".png"), 3)
            p = Packed([frame], [mask])
            base = overlay_native(p.frames, p).sample(0).cpu().numpy()
            with Image.open(os.path.join(native, "overlay", seq, stem + ".png")) as im:
                assert np.array_equal(np.array(im), draw_boxes_np(base, rows[:c[2]], 1, (9, 8, 7))), (seq, stem)
        assert js["sequences"][seq]["detections_mean"] == float(np.mean(counts))
    with open(os.path.join(native, "native_eval.json")) as f:
        assert json.load(f) == json.loads(json.dumps(js))
