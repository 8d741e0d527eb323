"""GPU: udet_link_detections_ragged and udet_draw_track_boxes_ragged (csrc/tracks.hip) through native_results.link_detections and
visualize.draw_track_boxes -- inter, match, ids, linked and seq_tracks against the numpy restatement of tests/test_tracks.py, the painted
frames against its numpy restatement.  Everything is integer: every comparison is exact equality.  The labels come from the existing
labelling call and the dets from component_boxes; the largest frame is 130 x 259."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_components import DENSITIES, _tree_files, ragged_masks
from test_components_gpu import pack
from test_detections import DetectionsNp
from test_detections_gpu import DRAW_SIZES, GUARD, Frames, hand_detections
from test_tracks import (LINK_OK, LINK_ORDER, TracksNp, draw_track_boxes_np, hand_cases, links_np, moving_sequence, run_case)

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 70), (67, 1), (9, 13), (33, 65), (130, 259)]
FIELDS = ("inter", "match", "ids", "linked", "seq_tracks")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def inputs(frames, k, min_area=1, conn=8, gap=0):
    """(ComponentSelection with labels, Detections) of binary frames, from the existing calls."""
    from unsupervised_detection_amd.native_results import component_boxes, select_components
    binary, off, hw = pack(frames, gap)
    sel = select_components(binary, off, hw, mode="label", connectivity=conn, want_labels=True)
    return sel, component_boxes(sel, min_area=min_area, max_detections=k)


def host_labels(sel):
    return [sel.labels_sample(i).cpu().numpy() for i in range(len(sel))]


def equal(got, want, where=()):
    for f, g in zip(FIELDS, got.host()):
        w = getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), where + (f,)
    assert int(got.next_id.cpu()[0]) == want.next_id, where


def sequences(density):
    """One sequence of 4 frames per size, cut from the largest random frame of that density; the flags that keep them apart."""
    base = ragged_masks(density)[5]
    frames, link = [], []
    for j, (h, w) in enumerate(SIZES):
        seq = moving_sequence(base[:h, :w], 3 + j % 2, 10 + j)
        frames += seq
        link += [0] + [1] * (len(seq) - 1)
    return frames, link


@pytest.mark.parametrize("density", DENSITIES)
def test_overlap_match_and_ids_equal_the_restatement(gpu, density):
    from unsupervised_detection_amd.native_results import link_detections
    frames, link = sequences(density)
    matched = 0
    for conn in (4, 8):
        for k in (1, 16, 64):
            sel, det = inputs(frames, k, 1, conn)
            labels, (dets, counts) = host_labels(sel), det.host()
            for permille in (1, 100, 1000):
                got = link_detections(sel, det, link=link, min_iou=permille / 1000)
                want = links_np(labels, dets, counts, link, permille)
                equal(got, want, (density, conn, k, permille))
                matched += int((want.match >= 0).sum())
                assert tuple(got.inter.shape) == (len(frames), k, k) and got.inter.dtype == torch.int64 and got.ids.dtype == torch.int32
            assert want.linked.tolist() == link  # every sequence keeps its size
            # link = None: every frame continues the one before it, so only the size changes cut
            equal(link_detections(sel, det, min_iou=0.1), links_np(labels, dets, counts, [1] * len(frames), 100), (density, conn, k, "None"))
    assert matched > 100


def test_the_hand_built_cases(gpu):
    from unsupervised_detection_amd.native_results import link_detections
    for name, (frames, k, permille) in hand_cases().items():
        sel, det = inputs(frames, k)
        want, dets, counts = run_case(name)
        assert np.array_equal(det.host()[0], dets) and np.array_equal(det.host()[1], counts), name
        equal(link_detections(sel, det, min_iou=permille / 1000), want, (name,))
    sel, det = inputs(hand_cases()["tie"][0], 4)
    labels, (dets, counts) = host_labels(sel), det.host()
    equal(link_detections(sel, det, link=[1, 0, 1]), links_np(labels, dets, counts, [1, 0, 1], 100), ("cut",))
    equal(link_detections(sel.labels, det, link=torch.tensor([0, 1, 1], dtype=torch.int32, device="cuda")),
          links_np(labels, dets, counts, [0, 1, 1], 100), ("device link",))


def test_carry_a_sequence_in_pieces_and_inside_a_batch(gpu):
    from unsupervised_detection_amd.native_results import link_detections
    frames = moving_sequence(ragged_masks(0.45)[3], 7, 1)
    sel, det = inputs(frames, 16, 2, 4)
    labels, (dets, counts) = host_labels(sel), det.host()
    whole = link_detections(sel, det)
    want = links_np(labels, dets, counts, [1] * 7, 100)
    equal(whole, want)
    assert (want.match >= 0).sum() > 20 and want.next_id > 16
    ref = whole.host()
    for cuts in ((3, 3, 1), (1,) * 7):
        carry, s = None, 0
        for c in cuts:
            part = link_detections(*inputs(frames[s:s + c], 16, 2, 4), carry=carry)
            got = part.host()
            for f, g, r in zip(FIELDS, got, ref):
                w = r[s:s + c].copy()
                if f == "seq_tracks":  # the piece's last frame ends the sequence within its call
                    w[:] = 0
                    w[-1] = int(part.next_id.cpu()[0])
                assert np.array_equal(g, w), (cuts, s, f)
            carry = part.tail()
            assert carry.hw == frames[0].shape and torch.equal(carry.ids, part.ids[-1]) and carry.ids.data_ptr() != part.ids[-1].data_ptr()
            s += c
        assert int(part.next_id.cpu()[0]) == want.next_id
        # the restatement takes the device tail as it is
        last = links_np(labels[-1:], dets[-1:], counts[-1:], [1], 100, link_detections(*inputs(frames[:6], 16, 2, 4)).tail())
        assert np.array_equal(last.ids[0], ref[2][6]) and np.array_equal(last.inter[0], ref[0][6])
    # the sequence inside a batch of several, and a carried frame of another size
    a, b = moving_sequence(ragged_masks(0.45)[4][:33, :65], 3, 5), moving_sequence(ragged_masks(0.3)[3][:9, :13], 4, 6)
    link = [0, 1, 1] + [0] + [1] * 6 + [0, 1, 1, 1]
    batch = link_detections(*inputs(a + frames + b, 16, 2, 4), link=link)
    for f, g, r in zip(FIELDS, batch.host(), ref):
        assert np.array_equal(g[3:10], r), f
    assert batch.host()[3].tolist() == link
    other = link_detections(*inputs(a, 16, 2, 4)).tail()
    alone = link_detections(sel, det, carry=other)
    equal(alone, want)  # link[0] = 1, but the carried frame has another size: frame 0 starts a sequence


def test_odd_offsets_guards_twice_and_labels_out_of_range(gpu):
    from unsupervised_detection_amd.native_results import component_boxes, link_detections
    frames, link = sequences(0.593)
    sel, det = inputs(frames, 16, 2, 8)
    ref = link_detections(sel, det, link=link)
    again = link_detections(sel, det, link=link)
    for a, b in zip(ref.host(), again.host()):
        assert np.array_equal(a, b)
    want = links_np(host_labels(sel), *det.host(), link, 100)
    equal(ref, want)
    # odd offsets, guard elements between the samples: garbage in the labels' guards is not read and nothing is written
    g, gdet = inputs(frames, 16, 2, 8, gap=37)
    guard = np.ones(g.labels.numel(), bool)
    for o, (h, w) in zip(g.offsets, g.hw):
        guard[o:o + h * w] = False
    lab = g.labels.cpu().numpy()
    lab[guard] = np.resize(np.array([1, 7, -3, 2 ** 31 - 1, -2 ** 31, 40000], np.int32), int(guard.sum()))
    dev = torch.from_numpy(lab).cuda()
    gdet2 = component_boxes(dev, min_area=2, max_detections=16, offsets=g.layout)
    assert torch.equal(gdet2.dets, det.dets)
    equal(link_detections(dev, gdet2, link=link), want, ("guards",))
    assert np.array_equal(dev.cpu().numpy(), lab)
    # whole components (and background pixels) overwritten with values outside 0..H*W: they vanish, nothing else changes
    lab = sel.labels.cpu().numpy().copy()
    poison = np.array([2 ** 31 - 1, -1, -2 ** 31], np.int32)
    for i, (o, (h, w)) in enumerate(zip(sel.offsets, sel.hw)):
        v = lab[o:o + h * w]
        for j, r in enumerate(np.unique(v[v > 0])[::3]):
            v[v == r] = h * w + 1 if j % 4 == 0 else poison[j % 3]
        v[np.flatnonzero(v == 0)[::5]] = poison[i % 3]
    dev = torch.from_numpy(lab).cuda()
    pdet = component_boxes(dev, min_area=2, max_detections=16, offsets=sel.layout)
    plabels = [sel.layout.view(dev, i).cpu().numpy() for i in range(len(sel))]
    pwant = links_np(plabels, *pdet.host(), link, 100)
    equal(link_detections(dev, pdet, link=link), pwant, ("poison",))
    assert not np.array_equal(pwant.inter, want.inter)


def test_refused_calls_leave_the_outputs_untouched(gpu):
    from unsupervised_detection_amd._ffi import lib
    frames = hand_cases()["split"][0]
    sel, det = inputs(frames, 4)
    n, k, total = 2, 4, sel.labels.numel()
    out = {"inter": torch.full((n, k, k), -77, dtype=torch.int64, device="cuda")}
    for f, shape in (("match", (n, k)), ("ids", (n, k)), ("linked", (n,)), ("seq", (n,)), ("next_id", (1,))):
        out[f] = torch.full(shape, -77, dtype=torch.int32, device="cuda")
    link = torch.ones(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.udet_link_detections_workspace_bytes(total, n, k, 0, 0) // 4 + 1, dtype=torch.int32, device="cuda")
    ok = dict(LINK_OK, labels=sel.labels.data_ptr(), n=n, offsets=sel.dev_offsets.data_ptr(), hw=sel.dev_hw.data_ptr(), max_h=8, max_w=18,
              total=total, dets=det.dets.data_ptr(), counts=det.counts.data_ptr(), k=k, link=link.data_ptr(), ws=ws.data_ptr(),
              ws_bytes=ws.numel() * 4, stream=torch.cuda.current_stream().cuda_stream, **{f: t.data_ptr() for f, t in out.items()})
    for change in (dict(labels=None), dict(link=None), dict(n=0), dict(k=0), dict(k=65), dict(permille=0), dict(permille=1001), dict(ws=None),
                   dict(ws_bytes=ok["ws_bytes"] // 2), dict(ws=ok["ws"] + 2), dict(inter=ok["inter"] + 4), dict(ids=None),
                   dict(c_labels=sel.labels.data_ptr()), dict(c_h=8, c_w=18)):
        a = dict(ok, **change)
        assert lib.udet_link_detections_ragged(*[a[p] for p in LINK_ORDER]) == -5, change
    torch.cuda.synchronize()
    assert all(bool((t == -77).all()) for t in out.values())
    assert lib.udet_link_detections_ragged(*[ok[p] for p in LINK_ORDER]) == 0
    want = run_case("split")[0]
    assert np.array_equal(out["inter"].cpu().numpy(), want.inter) and np.array_equal(out["match"].cpu().numpy(), want.match)
    assert np.array_equal(out["ids"].cpu().numpy(), want.ids) and out["linked"].tolist() == [0, 1] and out["seq"].tolist() == [0, 2]
    assert out["next_id"].tolist() == [2]


# ------------------------------------------------------------------------------------------------------- draw_track_boxes ----
def hand_ids(dets, counts):
    """Track ids for the rows of test_detections_gpu.hand_boxes: distinct, some past the palette's length, one row of sample 2 without."""
    ids = np.full(dets.shape[:2], -1, np.int32)
    for i in range(len(dets)):
        ids[i, :counts[i, 2]] = (7 * np.arange(counts[i, 2]) + 3 * i) % 29
    ids[2, 1] = -1   # a written row without an id: not painted, and it hides nothing
    ids[4, 0] = 5    # a row past the written ones: not painted whatever its id
    return ids


@pytest.mark.parametrize("thickness", [1, 2, 8])
def test_draw_track_boxes_equals_the_numpy_restatement(gpu, thickness):
    from unsupervised_detection_amd.visualize import TRACK_PALETTE, draw_track_boxes
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in DRAW_SIZES]
    sizes = np.array([h * w for h, w in DRAW_SIZES])
    off = 5 + np.concatenate([[0], np.cumsum(sizes + 5)[:-1]])  # odd offsets, guard bytes before, between and after
    det, dets, counts = hand_detections(16, off, int(off[-1] + sizes[-1] + 5))
    ids = hand_ids(dets, counts)
    trk = SimpleNamespace(ids=torch.from_numpy(ids).cuda())
    for palette in (TRACK_PALETTE, [(250, 3, 128)]):
        frames = Frames(images, det.layout)
        assert draw_track_boxes(frames, det, trk, thickness=thickness, palette=palette) is frames
        got = frames.data.cpu().numpy()
        touched = np.zeros(len(got), bool)
        for i, im in enumerate(images):
            painted = draw_track_boxes_np(im, dets[i, :counts[i, 2]], ids[i], thickness, palette)
            assert np.array_equal(frames.sample(i).cpu().numpy(), painted), (i, thickness, len(palette))
            touched[3 * int(off[i]):3 * int(off[i]) + im.size] = True
        assert np.array_equal(frames.sample(4).cpu().numpy(), images[4])  # no detection: untouched
        assert (got[~touched] == GUARD).all() and (~touched).sum() == 3 * 5 * 7
    # what the inputs promise: boxes of different tracks overlap and the lower rank's colour is what remains
    im = draw_track_boxes_np(images[2], dets[2, :counts[2, 2]], ids[2], thickness, TRACK_PALETTE)
    assert (im[0, 15] == TRACK_PALETTE[ids[2, 0] % 12]).all()
    assert (im[8, 19] == TRACK_PALETTE[ids[2, 3] % 12]).all() and ids[2, 3] % 12 != ids[2, 4] % 12  # on the lines of rows 3 and 4: row 3's colour
    assert len({int(v) % 12 for v in ids[2, :9] if v >= 0}) >= 6 and (ids[2, :9] >= 12).any()
    if thickness < 8:
        assert (im[5, 10] == TRACK_PALETTE[ids[2, 3] % 12]).all()  # on the lines of row 1 (no id) and row 3: row 1 hides nothing


def test_draw_track_boxes_of_real_tracks(gpu):
    from unsupervised_detection_amd.native_results import link_detections
    from unsupervised_detection_amd.visualize import TRACK_PALETTE, draw_track_boxes
    frames, link = sequences(0.3)
    sel, det = inputs(frames, 64, 3, 4)  # 4-connected: hundreds of components of three pixels or more on the larger frames
    trk = link_detections(sel, det, link=link)
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, m.shape + (3,), dtype=np.uint8) for m in frames]
    rgb = Frames(images, det.layout)
    draw_track_boxes(rgb, det, trk)
    ids = trk.host()[2]
    for i, im in enumerate(images):
        assert np.array_equal(rgb.sample(i).cpu().numpy(), draw_track_boxes_np(im, det.rows(i), ids[i], 2, TRACK_PALETTE)), i
    assert ids.max() > 12  # more tracks than colours: the palette is taken modulo its length


# ------------------------------------------------------------------------------------------------------------- end to end ----
def test_restore_results_dir_with_tracks_and_boxes(gpu, tmp_path):
    """The annotation-free stage on the small tree of test_frames_folder_gpu.py: component "largest", detections, tracks and boxes on the
    overlays; tracks/<category>.json and the overlay files against the numpy path on what the stage itself labelled."""
    import scipy.io as sio
    from PIL import Image
    from test_frames_folder import frames_flags, raises
    from test_frames_folder_gpu import HW, make_tree
    from test_overlay_native_gpu import Packed
    from unsupervised_detection_amd import data
    from unsupervised_detection_amd.native_results import (detection_records, frame_lists_from_reader, link_detections, restore_results_dir,
                                                           summarise_tracks, track_records)
    from unsupervised_detection_amd.visualize import TRACK_PALETTE, overlay_native
    root = make_tree(str(tmp_path / "clips"))
    saved = str(tmp_path / "saved")
    rng = np.random.default_rng(2)
    for seq in HW:
        os.makedirs(os.path.join(saved, seq))
        for k in range(4):
            m = (0.2 * rng.random((24, 32))).astype(np.float32)
            m[3 + k:12, 4:14 + k] += 0.7    # three blobs of different sizes, two of them moving
            m[15:21, 18 + k:27] += 0.7
            m[4:6, 22:25] += 0.7
            sio.savemat(os.path.join(saved, seq, "result_%d.mat" % (k + 1)), {"pred_mask": m})
    seen = []

    def link(labelled, det, **kw):
        seen.append((labelled, det, kw, link_detections(labelled, det, **kw)))
        return seen[-1][3]
    lists = frame_lists_from_reader(frames_flags(root))
    kw = dict(mask_key="pred_mask", batch=3, component="largest", connectivity=4, detections={"min_area": 12, "max_detections": 3},
              overlay={"boxes": {"thickness": 1}}, load_gt=raises, score=raises, verbose=False, gt_rule="FRAMES")
    native = str(tmp_path / "native")
    js = restore_results_dir(saved, lists, native, tracks={"min_iou": 0.3}, link=link, **kw)
    assert js["tracks"] == {"min_iou": 0.3} and sorted(os.listdir(os.path.join(native, "tracks"))) == ["a.json", "b.json"]
    assert [(s[2]["link"], s[2]["carry"] is not None, s[2]["min_iou"]) for s in seen] == [([0, 1, 1], False, 0.3), ([1], True, 0.3)] * 2
    batches = iter(seen)
    for seq, sizes in HW.items():
        stems = ["frame_%d" % (k + 9) for k in range(4)]
        parts = [next(batches), next(batches)]
        labels = [p[0].labels_sample(i).cpu().numpy() for p in parts for i in range(len(p[0]))]
        dets, counts = (np.concatenate([p[1].host()[j] for p in parts]) for j in (0, 1))
        want = links_np(labels, dets, counts, [0, 1, 1, 1], 300)
        assert want.linked.tolist() == [0] + [int(sizes[k] == sizes[k - 1]) for k in range(1, 4)] and (want.match >= 0).sum() >= 2
        for f, w in zip(FIELDS, (want.inter, want.match, want.ids, want.linked)):
            assert np.array_equal(np.concatenate([p[3].host()[FIELDS.index(f)] for p in parts]), w), (seq, f)
        with open(os.path.join(native, "detections", seq + ".json")) as f:
            got = json.load(f)
        plain = [[{k: v for k, v in d.items() if k not in ("track", "prev", "iou")} for d in got[s]] for s in stems]
        recs = track_records(plain, TracksNp(want, labels, DetectionsNp(dets, counts), None))
        assert [got[s] for s in stems] == json.loads(json.dumps(recs)), seq
        with open(os.path.join(native, "tracks", seq + ".json")) as f:
            assert json.load(f) == json.loads(json.dumps(summarise_tracks(stems, recs, [not v for v in want.linked]))), seq
        assert js["sequences"][seq]["tracks"] == int(want.seq_tracks.sum())
        for k, stem in enumerate(stems):
            with Image.open(os.path.join(native, seq, stem + ".png")) as im:
                mask = np.array(im)
            frame = data._read_image(os.path.join(root, seq, stem + ".png"), 3)
            p = Packed([frame], [mask])
            base = overlay_native(p.frames, p).sample(0).cpu().numpy()
            with Image.open(os.path.join(native, "overlay", seq, stem + ".png")) as im:
                assert np.array_equal(np.array(im), draw_track_boxes_np(base, dets[k, :counts[k, 2]], want.ids[k], 1, TRACK_PALETTE)), (seq, stem)
    # tracks=None: every file equals what it is without the argument
    none, plain = str(tmp_path / "none"), str(tmp_path / "plain")
    js_none = restore_results_dir(saved, lists, none, tracks=None, link=raises, draw_track_boxes=raises, **kw)
    js_plain = restore_results_dir(saved, lists, plain, **kw)
    f0, f1 = _tree_files(plain), _tree_files(none)
    assert js_none == js_plain and "tracks" not in js_none and sorted(f0) == sorted(f1) and all(f0[k] == f1[k] for k in f0)
    assert not os.path.exists(os.path.join(none, "tracks")) and len(f0) == len(_tree_files(native)) - 2
