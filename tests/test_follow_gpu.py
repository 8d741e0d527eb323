"""GPU: udet_follow_tracks_ragged (csrc/follow.hip) through native_results.follow_tracks -- selected and stats against the numpy
restatement of tests/test_follow.py.  Everything is integers and bytes: every comparison is exact equality.  The labels come from the
existing labelling call, the dets from component_boxes and the ids from link_detections; the largest frame is 130 x 259."""
import json

import numpy as np
import pytest
import torch

from test_components import DENSITIES, _tree_files, ragged_masks
from test_follow import FOLLOW_OK, FOLLOW_ORDER, ONES, follow_np, hand_cases, held_bytes, keep_cases, keep_np, stand_ins
from test_instances import random_gts, sequences
from test_instances_gpu import GUARD, pack_like
from test_tracks import moving_sequence, run_tree
from test_tracks_gpu import host_labels, inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def equal(got, want, where=()):
    masks, stats = want
    for i, m in enumerate(masks):
        g = got.binary_sample(i)
        assert g.dtype == torch.uint8 and tuple(g.shape) == m.shape and np.array_equal(g.cpu().numpy(), m), where + ("selected", i)
    assert got.host().dtype == np.int64 and np.array_equal(got.host(), stats), where + ("stats",)


@pytest.mark.parametrize("density", DENSITIES)
def test_selected_and_stats_equal_the_restatement(gpu, density):
    from unsupervised_detection_amd.native_results import follow_tracks, link_detections
    frames, link = sequences(density)
    gts = random_gts(frames)
    kept = dropped = hit = 0
    for conn in (4, 8):
        for k in (1, 16, 64):
            sel, det = inputs(frames, k, 2 if k == 16 else 1, conn)
            labels, (dets, counts) = host_labels(sel), det.host()
            gt = pack_like(sel, gts)
            rows = np.clip(counts[:, 2], 0, k)
            for max_gap in (0, 3):
                trk = link_detections(sel, det, link=link, max_gap=max_gap)
                ids, linked = trk.host()[2], trk.host()[3]
                for name, (words, _) in keep_cases(dets, counts, ids, linked, labels, gts, seed=k + max_gap).items():
                    want = follow_np(labels, dets, counts, words, gts)
                    got = follow_tracks(sel, det, words, gt=gt)
                    equal(got, want, (density, conn, k, max_gap, name, "gt"))
                    # without the annotation; the labels as a bare tensor, the words already on the device
                    dev = torch.from_numpy(words.view(np.int64)).cuda()
                    equal(follow_tracks(sel.labels, det, dev), follow_np(labels, dets, counts, words), (density, conn, k, max_gap, name, "no gt"))
                    # consistency with the detections: the kept pixels are the kept rows' areas, kept + dropped is the labelled foreground
                    stats = got.host()
                    assert all(stats[i, 0] == sum(int(dets[i, b, 1]) for b in range(rows[i]) if int(words[i]) >> b & 1) for i in range(len(frames)))
                    assert np.array_equal(stats[:, 0] + stats[:, 1], [int((lab > 0).sum()) for lab in labels])
                    kept, dropped, hit = kept + int(stats[:, 0].sum()), dropped + int(stats[:, 1].sum()), hit + int(stats[:, 2].sum())
    assert kept > 1000 and dropped > 1000 and hit > 100


def test_the_hand_built_cases_through_the_kernel(gpu):
    """The cases of tests/test_follow.py with their masks and counts written out by hand, one call each and all of them in one batch."""
    from unsupervised_detection_amd.native_results import Detections, follow_tracks
    from unsupervised_detection_amd.ragged import PackedLayout
    cases = hand_cases()
    dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()
    for name, lab, dets, counts, word, gt, mask, st in cases:
        layout = PackedLayout.packed([lab.shape])
        det = Detections(dev(dets, np.int64), dev(counts, np.int64), layout, 1, dets.shape[1])
        got = follow_tracks(dev(lab.reshape(-1), np.int32), det, [word], gt=None if gt is None else dev(gt.reshape(-1), np.uint8))
        assert np.array_equal(got.binary_sample(0).cpu().numpy(), mask) and got.host()[0].tolist() == st, name
    batch = [c for c in cases if c[2].shape[1] == 4]  # one k per call; a frame without gt gets an all-zero one
    layout = PackedLayout.packed([c[1].shape for c in batch])
    det = Detections(dev(np.concatenate([c[2] for c in batch]), np.int64), dev(np.concatenate([c[3] for c in batch]), np.int64), layout, 1, 4)
    gts = np.concatenate([(np.zeros(c[1].shape, np.uint8) if c[5] is None else c[5]).reshape(-1) for c in batch])
    got = follow_tracks(dev(np.concatenate([c[1].reshape(-1) for c in batch]), np.int32), det, np.array([c[4] for c in batch], np.uint64), gt=dev(gts, np.uint8))
    for i, (name, lab, dets, counts, word, gt, mask, st) in enumerate(batch):
        assert np.array_equal(got.binary_sample(i).cpu().numpy(), mask) and got.host()[i, :2].tolist() == st[:2], name
        assert got.host()[i, 2:].tolist() == (st[2:] if gt is not None else [0, 0]), name


def call_follow(labels, layout, det, keep, gt, out, stats):
    from unsupervised_detection_amd._ffi import lib
    from unsupervised_detection_amd.ragged import workspace
    d_off, d_hw = layout.device_tables(labels.device)
    ws = workspace(lib.udet_follow_tracks_workspace_bytes(layout.numel, layout.n, det.k), 4, labels.device)
    return lib.udet_follow_tracks_ragged(labels.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w, layout.numel,
                                         det.dets.data_ptr(), det.counts.data_ptr(), det.k, keep.data_ptr(), None if gt is None else gt.data_ptr(),
                                         out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)


def test_guards_a_sample_alone_twice_and_a_misaligned_output(gpu):
    from unsupervised_detection_amd.native_results import follow_tracks, link_detections
    frames, link = sequences(0.593)
    gts = random_gts(frames)
    sel, det = inputs(frames, 16, 2, 8)
    trk = link_detections(sel, det, link=link)
    labels, (dets, counts) = host_labels(sel), det.host()
    words = keep_cases(dets, counts, trk.host()[2], trk.host()[3], seed=5)["random"][0]
    ref = follow_tracks(sel, det, words, gt=pack_like(sel, gts))
    again = follow_tracks(sel, det, words, gt=pack_like(sel, gts))
    assert torch.equal(ref.selected, again.selected) and torch.equal(ref.stats, again.stats)
    want = follow_np(labels, dets, counts, words, gts)
    equal(ref, want)
    assert want[1][:, 0].sum() > 0 and want[1][:, 1].sum() > 0
    # odd offsets and guard bytes before, between and after the samples: none of them is written, whatever the output's own alignment
    g, gdet = inputs(frames, 16, 2, 8, gap=37)
    assert torch.equal(gdet.dets, det.dets) and len({int(o) % 4 for o in g.offsets}) >= 3
    gt = pack_like(g, gts, GUARD)
    dev_words = torch.from_numpy(words.view(np.int64)).cuda()
    total = g.layout.numel
    for shift in (0, 1, 2, 3):
        buf = torch.full((total + 8,), GUARD, dtype=torch.uint8, device="cuda")
        out = buf[shift:shift + total]
        stats = torch.full((len(frames), 4), -7, dtype=torch.int64, device="cuda")
        assert call_follow(g.labels, g.layout, gdet, dev_words, gt, out, stats) == 0
        host = buf.cpu().numpy()
        written = np.zeros(total + 8, bool)
        for i, (o, m) in enumerate(zip(g.offsets, want[0])):
            written[shift + o:shift + o + m.size] = True
            assert np.array_equal(host[shift + o:shift + o + m.size].reshape(m.shape), m), (shift, i)
        assert (host[~written] == GUARD).all() and (~written).sum() == 8 + 37 * (len(frames) + 1)
        assert np.array_equal(stats.cpu().numpy(), want[1])
    # a sample alone equals the same sample inside the batch
    for i in (0, 4, 9, 13, len(frames) - 1):
        s1, d1 = inputs(frames[i:i + 1], 16, 2, 8)
        alone = follow_tracks(s1, d1, words[i:i + 1], gt=pack_like(s1, gts[i:i + 1]))
        assert torch.equal(alone.binary_sample(0), ref.binary_sample(i)) and torch.equal(alone.stats[0], ref.stats[i]), i


def test_labels_out_of_range_and_garbage_counts(gpu):
    from unsupervised_detection_amd.native_results import Detections, follow_tracks
    frames = moving_sequence(ragged_masks(0.45)[3], 7, 1)
    gts = random_gts(frames, 5)
    sel, det = inputs(frames, 16, 2, 4)
    dets, counts = det.host()
    words = np.full(7, ONES, np.uint64)
    words[3] = 0b101
    lab = sel.labels.cpu().numpy().copy()
    poison = np.array([2 ** 31 - 1, -1, -2 ** 31], np.int32)
    for i, (o, (h, w)) in enumerate(zip(sel.offsets, sel.hw)):
        v = lab[o:o + h * w]
        for j, r in enumerate(np.unique(v[v > 0])[::3]):
            v[v == r] = h * w + 1 if j % 2 == 0 else poison[j % 3]
        v[np.flatnonzero(v == 0)[::5]] = poison[i % 3]
    dev = torch.from_numpy(lab).cuda()
    plabels = [sel.layout.view(dev, i).cpu().numpy() for i in range(7)]
    want = follow_np(plabels, dets, counts, words, gts)
    equal(follow_tracks(dev, det, words, gt=pack_like(sel, gts)), want, ("poison",))
    assert any(not np.array_equal(a, b) for a, b in zip(want[0], follow_np(host_labels(sel), dets, counts, words)[0]))
    # counts that claim more rows than k, or fewer than none: clamped, and the rows past the written ones hold root = -1
    wild = counts.copy()
    wild[0, 2], wild[1, 2], wild[2, 2] = 99, -5, 2 ** 40
    wdet = Detections(det.dets, torch.from_numpy(wild).cuda(), det.layout, det.min_area, det.k)
    equal(follow_tracks(sel, wdet, words), follow_np(host_labels(sel), dets, wild, words), ("wild counts",))


def test_refused_calls_leave_the_outputs_untouched(gpu):
    from unsupervised_detection_amd._ffi import lib
    frames = moving_sequence(ragged_masks(0.45)[3], 2, 1)
    sel, det = inputs(frames, 4)
    total = sel.layout.numel
    out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    stats = torch.full((2, 4), -7, dtype=torch.int64, device="cuda")
    keep = torch.tensor([0b11, 0b10], dtype=torch.int64, device="cuda")
    ws = torch.empty(total + 1, dtype=torch.int32, device="cuda")
    ok = dict(FOLLOW_OK, labels=sel.labels.data_ptr(), n=2, offsets=sel.dev_offsets.data_ptr(), hw=sel.dev_hw.data_ptr(), max_h=sel.layout.max_h,
              max_w=sel.layout.max_w, total=total, dets=det.dets.data_ptr(), counts=det.counts.data_ptr(), k=4, keep=keep.data_ptr(),
              selected=out.data_ptr(), stats=stats.data_ptr(), ws=ws.data_ptr(), ws_bytes=4 * total, stream=torch.cuda.current_stream().cuda_stream)
    for change in (dict(labels=None), dict(keep=None), dict(selected=None), dict(stats=None), dict(n=0), dict(n=65536), dict(k=0), dict(k=65),
                   dict(ws=None), dict(ws_bytes=4 * total - 1), dict(ws=ok["ws"] + 2), dict(stats=ok["stats"] + 4), dict(keep=ok["keep"] + 4),
                   dict(max_h=0), dict(total=0), dict(total=-1)):
        a = dict(ok, **change)
        assert lib.udet_follow_tracks_ragged(*[a[p] for p in FOLLOW_ORDER]) == -5, change
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((stats == -7).all())
    assert lib.udet_follow_tracks_ragged(*[ok[p] for p in FOLLOW_ORDER]) == 0
    want = follow_np(host_labels(sel), *det.host(), [0b11, 0b10])
    assert all(np.array_equal(sel.layout.view(out, i).cpu().numpy(), m) for i, m in enumerate(want[0]))
    assert np.array_equal(stats.cpu().numpy(), want[1]) and want[1][:, 0].all()


def test_restore_results_dir_with_follow_end_to_end(gpu, tmp_path, monkeypatch):
    """The stage with its real callables on the small mixed tree equals the run on the numpy stand-ins, file for file; between the passes
    it holds 5 bytes per pixel and frame."""
    from test_components_gpu import speckled_restore_gpu
    from unsupervised_detection_amd import native_results as nr
    seen, real = [], nr._follow_category

    def spy(cat, held, *a):
        if held and isinstance(held[0][5], nr.Tracks):  # the run on the device
            total, least = sum(h[3].layout.numel for h in held), 17 * 40  # (the smallest frame of the tree: nothing per row is that large)
            seen.append((held_bytes([x for h in held for x in h[3:]], least), total))
            assert all(h[5].carry is None and h[5].inter is None and h[5].gap_inter is None and h[6].binary is None for h in held)
        return real(cat, held, *a)
    monkeypatch.setattr(nr, "_follow_category", spy)
    from unsupervised_detection_amd.native_results import (component_boxes, follow_tracks, link_detections, load_gt_device, score_device,
                                                           select_components)
    kw = dict(follow={"rule": "mass", "min_frames": 2})
    base = {k: v for k, v in stand_ins([], [], 1).items() if k not in ("paint", "draw_instances", "load_images", "draw")}
    ref, want, _ = run_tree(tmp_path, "ref", True, 3, keep=keep_np([]), **dict(base, **kw))
    out, got, _ = run_tree(tmp_path, "dev", True, 3, restore=speckled_restore_gpu, load_gt=load_gt_device, score=score_device,
                           select=select_components, detect=component_boxes, link=link_detections, keep=follow_tracks,
                           detections={"min_area": 2, "max_detections": 3}, tracks={"min_iou": 0.2, "max_gap": 1}, **kw)
    assert json.loads(json.dumps(got)) == json.loads(json.dumps(want)) and got["follow"] == {"rule": "mass", "min_frames": 2}
    assert len(seen) == 2 and all(held == 5 * total for held, total in seen)  # per category: every tensor of a frame's size or more that the held batches keep alive, over their pixels
    assert all(0 < got["sequences"][s]["kept_mean"] < 1 for s in got["sequences"])
    a, b = _tree_files(out), _tree_files(ref)
    assert sorted(a) == sorted(b) and len(a) == 2 * 14 + 2 + 2 + 1
    for name in a:
        if name == "native_eval.json":
            assert json.loads(a[name]) == json.loads(b[name]) == json.loads(json.dumps(got))
        else:
            assert a[name] == b[name], name
