"""GPU: udet_link_detections_gap_ragged (csrc/tracks.hip) through native_results.link_detections(max_gap=...) and through
the C entry point -- every output against bridge_np, the numpy restatement of tests/test_track_gaps.py, for exact equality: everything is
integer.  The labels come from the existing labelling call and the dets from component_boxes; the largest frame is 130 x 259."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_components import RAGGED_SHAPES, ragged_masks
from test_detections import DetectionsNp
from test_track_gaps import (GAP_FIELDS, GAP_OK, GAP_ORDER, TracksGapNp, bridge_np, bridges, claimed_once, flicker, gap_cases, hand_checks,
                             no_id_twice, run_gap_case)
from test_tracks import moving_sequence
from test_tracks_gpu import host_labels, inputs

pytestmark = pytest.mark.gpu

GUARD = 64  # elements of FILL on both sides of every output of a raw call
FILL = -77


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def fields(got):
    """A Tracks linked with max_gap > 0 -> bridge_np's namespace, on the host."""
    out = SimpleNamespace(**dict(zip(GAP_FIELDS, got.host() + got.host_gaps())))
    out.next_id = int(got.next_id.cpu()[0])
    out.hist_open = None if got.hist_open is None else got.hist_open.cpu().numpy()
    return out


def equal(got, want, where=()):
    for f in GAP_FIELDS + ("hist_open",):
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None and w is None) or (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)), where + (f,)
    assert got.next_id == want.next_id, where


def sequences(density):
    """One flickering sequence of 7 frames per size, and the flags that keep them apart."""
    frames = [f for base in ragged_masks(density) for f in flicker(moving_sequence(base, 7, 1), 5)]
    return frames, ([0] + [1] * 6) * len(RAGGED_SHAPES)


@pytest.mark.parametrize("density", [0.3, 0.45, 0.6])
def test_every_output_equals_the_restatement(gpu, density):
    """Six sequences in one call, for every (connectivity, k) with every max_gap and every threshold (each pair of the two once per
    density), and one of the sequences alone."""
    from unsupervised_detection_amd.native_results import link_detections
    frames, link = sequences(density)
    bridged, combo = {}, 0
    for conn in (4, 8):
        for k in (1, 16, 64):
            sel, det = inputs(frames, k, 2, conn)
            labels, (dets, counts) = host_labels(sel), det.host()
            for j, max_gap in enumerate((1, 3, 8)):
                permille = (1, 100, 1000)[(j + combo) % 3]
                got = link_detections(sel, det, link=link, min_iou=permille / 1000, max_gap=max_gap)
                want = bridge_np(labels, dets, counts, link, permille, max_gap)
                equal(fields(got), want, (density, conn, k, max_gap, permille))
                assert tuple(got.gap_inter.shape) == (len(frames), max_gap, k, k) and got.gap_inter.dtype == torch.int64 and got.back.dtype == torch.int32
                assert no_id_twice(got.host()[2])
                old = link_detections(sel, det, link=link, min_iou=permille / 1000)  # stage 1 is the old entry's, entry for entry
                assert all(np.array_equal(a, b) for a, b in zip(old.host()[:2] + old.host()[3:4], got.host()[:2] + got.host()[3:4]))
                for d, v in bridges(want).items():
                    bridged[d] = bridged.get(d, 0) + v
            combo += 1
            if k == 16:  # the 37 x 53 sequence alone: what it gives inside the batch
                alone = fields(link_detections(*inputs(frames[21:28], k, 2, conn), min_iou=permille / 1000, max_gap=8))
                for f in GAP_FIELDS:
                    w = getattr(want, f)[21:28]
                    assert np.array_equal(getattr(alone, f), w), (density, conn, "alone", f)
    assert set(bridged) >= {2, 3, 4} and sum(bridged.values()) > 50, bridged


def test_the_inputs_bridge_at_every_distance(gpu):
    """The two cases counted on the restatement: bridges at every distance 2..4 at max_gap = 3, and the device agrees."""
    from unsupervised_detection_amd.native_results import link_detections
    for size_index, density, k, conn in ((3, 0.3, 64, 8), (5, 0.45, 16, 4)):
        frames = flicker(moving_sequence(ragged_masks(density)[size_index], 7, 1), 5)
        sel, det = inputs(frames, k, 2, conn)
        want = bridge_np(host_labels(sel), *det.host(), [1] * 7, 100, 3)
        assert set(bridges(want)) == {2, 3, 4}
        got = link_detections(sel, det, max_gap=3)
        equal(fields(got), want, (size_index,))
        assert want.next_id < int(link_detections(sel, det).next_id.cpu()[0])


def device_run(labels, dets, counts, link, permille, max_gap, history=None, k=None):
    """bridge_np's signature on the device: the labels are packed as they are, dets / counts go up unchanged."""
    from unsupervised_detection_amd.native_results import Detections, link_detections
    from unsupervised_detection_amd.ragged import PackedLayout
    layout = PackedLayout.packed([np.asarray(l).shape for l in labels])
    lab = torch.from_numpy(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in labels])).cuda()
    dets, counts = np.asarray(dets, np.int64), np.asarray(counts, np.int64)
    det = Detections(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), layout, 1, dets.shape[1])
    got = link_detections(lab, det, link=link, carry=history, min_iou=permille / 1000, max_gap=max_gap)
    out = fields(got)
    out.tracks = got
    return out


def test_the_hand_built_cases(gpu):
    from test_tracks import inputs_np

    def run(name, max_gap):
        frames, k, permille, link = gap_cases()[name]
        labels, dets, counts = inputs_np(frames, k)
        got = device_run(labels, dets, counts, link or [1] * len(frames), permille, max_gap)
        equal(got, run_gap_case(name, max_gap)[0], (name, max_gap))
        return got
    hand_checks(run)
    for name in gap_cases():
        for max_gap in (1, 2, 8):
            run(name, max_gap)
    # the frames through the labelling and the boxes of the device give the same inputs
    frames, k, permille, _ = gap_cases()["c two orphans"]
    sel, det = inputs(frames, k)
    labels, dets, counts = inputs_np(frames, k)
    assert np.array_equal(det.host()[0], dets) and np.array_equal(det.host()[1], counts) and all(np.array_equal(a, b) for a, b in zip(host_labels(sel), labels))


@pytest.mark.parametrize("max_gap", [1, 3])
def test_history_a_sequence_in_pieces_and_inside_a_batch(gpu, max_gap):
    from unsupervised_detection_amd.native_results import TrackHistory, link_detections
    frames = flicker(moving_sequence(ragged_masks(0.3)[3], 7, 1), 5)
    sel, det = inputs(frames, 64, 2, 8)
    labels, (dets, counts) = host_labels(sel), det.host()
    whole = link_detections(sel, det, max_gap=max_gap)
    want = bridge_np(labels, dets, counts, [1] * 7, 100, max_gap)
    equal(fields(whole), want)
    assert (want.back >= 2).sum() >= 20
    ref = fields(whole)
    for cuts in ((3, 3, 1), (1,) * 7):
        hist, s = None, 0
        for c in cuts:
            part = link_detections(*inputs(frames[s:s + c], 64, 2, 8), carry=hist, max_gap=max_gap)
            got = fields(part)
            for f in GAP_FIELDS:
                w = getattr(ref, f)[s:s + c].copy()
                if f == "seq_tracks":  # the piece's last frame ends the sequence within its call
                    w[:] = 0
                    w[-1] = got.next_id
                if f == "open":  # so far: rows that later pieces close are still open
                    w = None
                assert w is None or np.array_equal(getattr(got, f), w), (cuts, s, f)
            before = None if hist is None else hist.open.clone()
            hist = part.tail()
            assert before is None or torch.equal(before, part.carry.open)  # the call closed rows in its own copy
            s += c
            assert isinstance(hist, TrackHistory) and (hist.m, hist.k, hist.max_gap, hist.hw) == (min(max_gap + 1, s), 64, max_gap, frames[0].shape)
            assert torch.equal(hist.ids, whole.ids[s - hist.m:s]) and hist.ids.data_ptr() != part.ids.data_ptr()
            opened = np.array(ref.open[s - hist.m:s])  # the whole's flags, without what the frames from s on closed
            for c2 in range(s, 7):
                for b in range(64):
                    d = int(ref.back[c2, b])
                    if d and s - hist.m <= c2 - d < s:
                        opened[c2 - d - (s - hist.m), ref.prev[c2, b]] = 1
            assert np.array_equal(hist.open.cpu().numpy(), opened), (cuts, s)
        assert got.next_id == want.next_id
    # the sequence inside a batch of several
    a, b = moving_sequence(ragged_masks(0.45)[4][:33, :65], 3, 5), flicker(moving_sequence(ragged_masks(0.3)[3][:9, :13], 5, 6), 2)
    link = [0, 1, 1] + [0] + [1] * 6 + [0, 1, 1, 1, 1]
    batch = fields(link_detections(*inputs(a + frames + b, 64, 2, 8), link=link, max_gap=max_gap))
    for f in GAP_FIELDS:
        assert np.array_equal(getattr(batch, f)[3:10], getattr(ref, f)), f
    assert batch.linked.tolist() == link


def test_a_history_row_is_claimed_once(gpu):
    claimed_once(device_run, lambda r, labels, dets, counts, max_gap, history: r.tracks.tail())


def raw_call(sel, det, link, permille, max_gap, hist=None, ws_fill=None, change=None):
    """One call of the C entry point on guarded outputs -> (status, {name: numpy array}, guards intact).  change: arguments replaced
    after everything is set up (("+", v): the pointer moved by v bytes)."""
    from unsupervised_detection_amd._ffi import lib
    n, k, total = len(sel), det.k, sel.labels.numel()
    shapes = dict(inter=(n, k, k), match=(n, k), ids=(n, k), linked=(n,), seq=(n,), next_id=(1,), gap_inter=(n, max_gap, k, k), back=(n, k),
                  prev=(n, k), open=(n, k))
    bufs = {f: torch.full((2 * GUARD + int(np.prod(s)),), FILL, dtype=torch.int64 if "inter" in f else torch.int32, device="cuda")
            for f, s in shapes.items()}
    m, (hh, hw) = (hist.m, hist.hw) if hist is not None else (0, (0, 0))
    words = lib.udet_link_detections_gap_workspace_bytes(total, n, k, max_gap, m, hh, hw) // 4
    assert words == total + m * hh * hw
    ws = torch.empty(words + 1, dtype=torch.int32, device="cuda")
    if ws_fill is not None:
        ws.copy_(torch.from_numpy(np.resize(np.asarray(ws_fill, np.int32), words + 1)))
    d_link = torch.tensor(link, dtype=torch.int32, device="cuda")
    hist_open = None if hist is None else hist.open.clone()
    a = dict(GAP_OK, labels=sel.labels.data_ptr(), n=n, offsets=sel.dev_offsets.data_ptr(), hw=sel.dev_hw.data_ptr(),
             max_h=int(max(h for h, _ in sel.hw)), max_w=int(max(w for _, w in sel.hw)), total=total, dets=det.dets.data_ptr(),
             counts=det.counts.data_ptr(), k=k, link=d_link.data_ptr(), max_gap=max_gap, m=m, h_h=hh, h_w=hw, permille=permille, ws=ws.data_ptr(),
             ws_bytes=words * 4, stream=torch.cuda.current_stream().cuda_stream,
             **{f: t.data_ptr() + GUARD * t.element_size() for f, t in bufs.items()})
    if hist is not None:
        a.update(h_labels=hist.labels.data_ptr(), h_dets=hist.dets.data_ptr(), h_counts=hist.counts.data_ptr(), h_ids=hist.ids.data_ptr(),
                 h_open=hist_open.data_ptr(), h_next=hist.next_id.data_ptr())
    a.update({p: (a[p] + v[1] if isinstance(v, tuple) else v) for p, v in (change or {}).items()})
    rc = lib.udet_link_detections_gap_ragged(*[a[p] for p in GAP_ORDER])
    torch.cuda.synchronize()
    host = {f: t.cpu().numpy() for f, t in bufs.items()}
    intact = all((v[:GUARD] == FILL).all() and (v[-GUARD:] == FILL).all() for v in host.values())
    out = {("seq_tracks" if f == "seq" else f): host[f][GUARD:-GUARD].reshape(s) for f, s in shapes.items()}
    out["hist_open"] = None if hist is None else hist_open.cpu().numpy()
    return rc, out, intact


def as_fields(out):
    r = SimpleNamespace(**{f: out[f] for f in GAP_FIELDS}, hist_open=out["hist_open"])
    r.next_id = int(out["next_id"][0])
    return r


def test_guards_twice_garbage_in_the_workspace_and_labels_out_of_range(gpu):
    from unsupervised_detection_amd.native_results import component_boxes, link_detections
    frames, link = sequences(0.6)
    sel, det = inputs(frames, 16, 2, 8)
    labels = host_labels(sel)
    want = bridge_np(labels, *det.host(), link, 100, 3)
    garbage = [0, 15, 16, -1, 2 ** 31 - 1, -2 ** 31, 3, 70000]
    for fill in (None, garbage, garbage[::-1]):  # whatever the workspace holds, twice over: the same outputs, the guards as they were
        rc, out, intact = raw_call(sel, det, link, 100, 3, ws_fill=fill)
        assert rc == 0 and intact
        equal(as_fields(out), want, ("workspace", fill is None))
    # a history with garbage in its flags and ids beyond its rows, and in the workspace
    seq = flicker(moving_sequence(ragged_masks(0.3)[3], 7, 1), 5)  # 37 x 53: 64, 56 and 48 rows in the first three frames
    head = link_detections(*inputs(seq[:3], 64, 2, 8), max_gap=3)
    hist = head.tail()
    rows = hist.counts[:, 2].clamp(0, 64)
    beyond = torch.arange(64, device="cuda")[None, :] >= rows[:, None]
    hist.open[beyond] = 7
    hist.ids[beyond] = 2 ** 31 - 1
    tsel, tdet = inputs(seq[3:], 64, 2, 8)
    rc, out, intact = raw_call(tsel, tdet, [1] * 4, 100, 3, hist=hist, ws_fill=garbage)
    assert rc == 0 and intact and int(beyond.sum()) == 8 + 16 and (out["hist_open"][beyond.cpu().numpy()] == 7).all()  # not read, not written
    out["hist_open"][beyond.cpu().numpy()] = 0
    tail = bridge_np(host_labels(tsel), *tdet.host(), [1] * 4, 100, 3, head.tail())
    equal(as_fields(out), tail, ("history",))
    reach = [(c, d) for c in range(4) for d in tail.back[c] if d > c + 1]
    assert len(reach) >= 10 and {d for _, d in reach} == {2, 3, 4} and not tail.hist_open[:, :8].all()  # bridges into the history, at every distance
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
    pwant = bridge_np(plabels, *pdet.host(), link, 100, 3)
    equal(fields(link_detections(dev, pdet, link=link, max_gap=3)), pwant, ("poison",))
    assert not np.array_equal(pwant.gap_inter, want.gap_inter) and (pwant.back >= 2).any()


def test_refused_calls_leave_the_outputs_untouched(gpu):
    frames, k, permille, _ = gap_cases()["a vanish and return"]
    sel, det = inputs(frames, k)
    for change in (dict(labels=None), dict(link=None), dict(n=0), dict(k=0), dict(k=65), dict(permille=0), dict(max_gap=0), dict(max_gap=9), dict(m=1),
                   dict(m=-1), dict(ws=None), dict(ws_bytes=16), dict(ws=("+", 2)), dict(gap_inter=("+", 4)), dict(back=None), dict(prev=("+", 2)),
                   dict(open=None), dict(h_labels=sel.labels.data_ptr()), dict(h_h=8, h_w=18)):
        rc, out, intact = raw_call(sel, det, [1, 1, 1], permille, 1, change=change)
        assert rc == -5 and intact and all((v == FILL).all() for f, v in out.items() if v is not None), change
    rc, out, intact = raw_call(sel, det, [1, 1, 1], permille, 1)
    assert rc == 0 and intact
    equal(as_fields(out), run_gap_case("a vanish and return", 1)[0])


# ------------------------------------------------------------------------------------------------------------- end to end ----
def test_restore_results_dir_with_max_gap_and_boxes(gpu, tmp_path):
    """The annotation-free stage on the small tree of test_frames_folder_gpu.py with detections, tracks, max_gap = 2 and boxes: a blob is
    missing from one frame of each sequence; detections/ and tracks/<sequence>.json against the restatement on what the stage labelled."""
    import scipy.io as sio
    from test_frames_folder import frames_flags, raises
    from test_frames_folder_gpu import HW, make_tree
    from unsupervised_detection_amd.native_results import (frame_lists_from_reader, link_detections, restore_results_dir, summarise_tracks,
                                                           track_records)
    root = make_tree(str(tmp_path / "clips"))
    saved = str(tmp_path / "saved")
    rng = np.random.default_rng(2)
    for seq in HW:
        os.makedirs(os.path.join(saved, seq))
        for k in range(4):
            m = (0.2 * rng.random((24, 32))).astype(np.float32)
            m[3 + k:12, 4:14 + k] += 0.7    # three blobs of different sizes, two of them moving
            if k != 1:
                m[15:21, 18 + k:27] += 0.7  # ... and one of those missing from the second frame
            m[4:6, 22:25] += 0.7
            sio.savemat(os.path.join(saved, seq, "result_%d.mat" % (k + 1)), {"pred_mask": m})
    seen = []

    def link(labelled, det, **kw):
        seen.append((labelled, det, kw, link_detections(labelled, det, **kw)))
        return seen[-1][3]
    lists = frame_lists_from_reader(frames_flags(root))
    native = str(tmp_path / "native")
    js = restore_results_dir(saved, lists, native, tracks={"min_iou": 0.3, "max_gap": 2}, link=link, mask_key="pred_mask", batch=3,
                             component="largest", connectivity=4, detections={"min_area": 12, "max_detections": 3},
                             overlay={"boxes": {"thickness": 1}}, load_gt=raises, score=raises, verbose=False, gt_rule="FRAMES")
    assert js["tracks"] == {"min_iou": 0.3, "max_gap": 2}
    assert [(s[2]["link"], None if s[2]["carry"] is None else s[2]["carry"].m, s[2]["max_gap"]) for s in seen] == [
        ([0, 1, 1], None, 2), ([1], 1, 2), ([0, 1, 1], None, 2), ([1], 3, 2)]  # "a" changes its size at its third frame: a history of one
    batches = iter(seen)
    for seq in HW:
        stems = ["frame_%d" % (k + 9) for k in range(4)]
        parts = [next(batches), next(batches)]
        labels = [p[0].labels_sample(i).cpu().numpy() for p in parts for i in range(len(p[0]))]
        dets, counts = (np.concatenate([p[1].host()[j] for p in parts]) for j in (0, 1))
        want = bridge_np(labels, dets, counts, [0, 1, 1, 1], 300, 2)
        for f in ("inter", "match", "ids", "linked", "gap_inter", "back", "prev"):
            assert np.array_equal(np.concatenate([getattr(fields(p[3]), f) for p in parts]), getattr(want, f)), (seq, f)
        with open(os.path.join(native, "detections", seq + ".json")) as f:
            got = json.load(f)
        plain = [[{k: v for k, v in d.items() if k not in ("track", "prev", "iou", "back")} for d in got[s]] for s in stems]
        recs = track_records(plain, TracksGapNp(want, labels, DetectionsNp(dets, counts), None, 2))
        assert [got[s] for s in stems] == json.loads(json.dumps(recs)), seq
        with open(os.path.join(native, "tracks", seq + ".json")) as f:
            summary = json.load(f)
        assert summary == json.loads(json.dumps(summarise_tracks(stems, recs, [not v for v in want.linked], gaps=True))), seq
        assert js["sequences"][seq]["tracks"] == int(want.seq_tracks.sum())
        if seq == "b":  # one size throughout: the blob missing from the second frame keeps its id
            assert [s["bridged"] for s in summary] == [1] and (want.back == 2).sum() == 1 and want.linked.tolist() == [0, 1, 1, 1]
            assert (3, 4, 1) in [(t["frames"], t["span"], t["gaps"]) for t in summary[0]["tracks"]]
        assert len(os.listdir(os.path.join(native, "overlay", seq))) == 4
