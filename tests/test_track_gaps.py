"""CPU: gap bridging of the tracks (native_results.link_detections(max_gap=...), udet_link_detections_gap_ragged, csrc/tracks.hip,
DESIGN.md 7.9) -- the numpy restatement of the definition, the hand-built cases on it, the C entry point's argument checks, the
wrapper's host validation, the parameters and flags, the records' and the summary's arithmetic, restore_results_dir(tracks={"max_gap":
...}) on numpy stand-ins and the header's sentences.

bridge_np restates include/udet.h's definition on top of test_tracks.links_np (stage 1): one bincount per distance for gap_inter, a
sorted candidate list for the greedy choice, a plain Python walk.  tests/test_track_gaps_gpu.py compares the kernels with it for exact
equality."""
import functools
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from test_components import _tree_files, ragged_masks
from test_detections import DetectionsNp, detect_np, select_labels_np
from test_tracks import LINK_OK, TracksNp, _np, hand_cases, inputs_np, link_np, links_np, moving_sequence, rank_map, rects, run_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_FIELDS = ("inter", "match", "ids", "linked", "seq_tracks", "gap_inter", "back", "prev", "open")


# ------------------------------------------------------------------------------------------------------------ restatement ----
def bridge_np(labels_list, dets, counts, link, permille, max_gap, history=None):
    """include/udet.h, udet_link_detections_gap_ragged, written as its sentences.  labels_list / dets / counts / link / permille: as for
    links_np; history: None or an object with labels [m, h * w] / hw / dets / counts / ids / open / next_id (native_results.TrackHistory).
    Returns a namespace of the nine outputs (arrays of the kernels' dtypes), next_id and hist_open (the history's flags after the call)."""
    dets, counts = _np(dets).astype(np.int64), _np(counts).astype(np.int64)
    n, k = dets.shape[:2]
    rows = [min(max(int(c[2]), 0), k) for c in counts]
    seq, next_id, hist_open = [], 0, None  # seq: the frames of the current sequence so far, oldest first, at most max_gap + 1
    carry = None
    if history is not None:
        m, hw = len(_np(history.dets)), tuple(history.hw)
        hl, hd, hc, hi = _np(history.labels).reshape((m,) + hw), _np(history.dets).astype(np.int64), _np(history.counts), _np(history.ids)
        hist_open = np.array(_np(history.open), np.int32)
        next_id = int(_np(history.next_id).reshape(-1)[0])
        carry = SimpleNamespace(labels=hl[-1], hw=hw, dets=hd[-1], counts=hc[-1], ids=hi[-1], next_id=history.next_id)
        seq = [SimpleNamespace(dets=hd[j], rows=min(max(int(hc[j][2]), 0), k), ids=hi[j], open=hist_open[j]) for j in range(m)]
        for j, f in enumerate(seq):
            f.rank = rank_map(hl[j], f.dets, f.rows).ravel()
    s1 = links_np(labels_list, dets, counts, link, permille, carry)  # stage 1 is today's link, unchanged
    out = SimpleNamespace(inter=s1.inter, match=s1.match, linked=s1.linked, ids=np.full((n, k), -1, np.int32), seq_tracks=np.zeros(n, np.int32),
                          gap_inter=np.zeros((n, max_gap, k, k), np.int64), back=np.zeros((n, k), np.int32), prev=np.full((n, k), -1, np.int32),
                          open=np.zeros((n, k), np.int32), hist_open=hist_open)

    def order(p, q):  # the larger inter / union, then the smaller d, then the smaller a, then the smaller b
        l, r = p[0] * q[1], q[0] * p[1]
        if l != r:
            return -1 if l > r else 1
        return -1 if p[2:] < q[2:] else 1
    for c in range(n):
        rb = rank_map(labels_list[c], dets[c], rows[c]).ravel()  # per pixel the rank of its row, or -1
        if not s1.linked[c]:
            if c:
                out.seq_tracks[c - 1] = next_id
            seq = []
            out.ids[c, :rows[c]] = np.arange(rows[c])
            next_id = rows[c]
        else:
            orphans = []
            for b in range(rows[c]):
                a = int(s1.match[c, b])
                if a >= 0:  # stage 1 comes first and is never undone
                    out.ids[c, b], out.back[c, b], out.prev[c, b] = seq[-1].ids[a], 1, a
                    seq[-1].open[a] = 0
                else:
                    orphans.append(b)
            cands = []
            for d in range(2, min(max_gap + 1, len(seq)) + 1):
                f = seq[-d]
                both = (f.rank >= 0) & (rb >= 0)
                out.gap_inter[c, d - 2] = np.bincount(f.rank[both] * k + rb[both], minlength=k * k).reshape(k, k)
                for a in range(f.rows):
                    for b in orphans:
                        it = int(out.gap_inter[c, d - 2, a, b])
                        union = int(f.dets[a, 1]) + int(dets[c, b, 1]) - it
                        if f.open[a] and it > 0 and 1000 * it >= permille * union:
                            cands.append((it, union, d, a, b))
            for it, union, d, a, b in sorted(cands, key=functools.cmp_to_key(order)):
                if seq[-d].open[a] and out.back[c, b] == 0:
                    out.ids[c, b], out.back[c, b], out.prev[c, b] = seq[-d].ids[a], d, a
                    seq[-d].open[a] = 0
            for b in orphans:
                if out.back[c, b] == 0:
                    out.ids[c, b] = next_id
                    next_id += 1
        out.open[c, :rows[c]] = 1
        seq = (seq + [SimpleNamespace(rank=rb, dets=dets[c], rows=rows[c], ids=out.ids[c], open=out.open[c])])[-(max_gap + 1):]
    out.seq_tracks[n - 1] = out.next_id = next_id
    return out


def history_np(r, labels_list, dets, counts, max_gap, history=None):
    """What Tracks.tail() returns for a bridge_np result: the last max_gap + 1 frames of the call's last sequence, the history's included."""
    from unsupervised_detection_amd.native_results import TrackHistory
    n = len(labels_list)
    first = n - 1
    while first > 0 and r.linked[first]:
        first -= 1
    lo = max(first, n - 1 - max_gap)
    hw = np.asarray(labels_list[-1]).shape
    parts = [[np.stack([np.asarray(l, np.int32).reshape(-1) for l in labels_list[lo:]])], [_np(dets)[lo:]], [_np(counts)[lo:]], [r.ids[lo:]], [r.open[lo:]]]
    if first == 0 and r.linked[0]:
        m = len(_np(history.dets))
        keep = slice(max(0, m - (max_gap - (n - 1))), m)
        old = (_np(history.labels).reshape(m, -1), _np(history.dets), _np(history.counts), _np(history.ids), r.hist_open)
        parts = [[o[keep]] + p for o, p in zip(old, parts)]
    lab, d, c, ids, opn = (np.concatenate(p) for p in parts)
    return TrackHistory(lab.astype(np.int32), hw, d.astype(np.int64), c.astype(np.int64), ids.astype(np.int32), opn.astype(np.int32),
                        np.array([r.next_id], np.int32), max_gap)


def flicker(frames, seed):
    """Copies of the frames with one H // 2 x W // 2 block zeroed at a seeded position in every inner frame: components go missing."""
    rng = np.random.default_rng(seed)
    out = [np.array(f, np.uint8) for f in frames]
    H, W = out[0].shape
    for f in out[1:-1]:
        y, x = int(rng.integers(0, H - H // 2 + 1)), int(rng.integers(0, W - W // 2 + 1))
        f[y:y + H // 2, x:x + W // 2] = 0
    return out


def bridges(r):
    """{distance: rows bridged at it} of a bridge_np result."""
    return {int(d): int((r.back == d).sum()) for d in np.unique(r.back) if d >= 2}


def no_id_twice(ids):
    return all(len(set(row[row >= 0].tolist())) == int((row >= 0).sum()) for row in np.asarray(ids))


# ------------------------------------------------------------------------------------------------------- hand-built cases ----
def gap_cases():
    """{name: (frames, k, permille, link)}: one short sequence per property (8 x 18, 8-connected, min_area 1); hand_checks says what each
    must give."""
    s = (8, 18)
    old = hand_cases()
    empty = rects(s)
    A, B = (1, 1, 6, 7), (2, 10, 5, 14)
    big = (1, 1, 5, 9)                                # 32 pixels
    two, bridge = old["tie"][0][0], old["tie"][0][1]  # two blobs of 6; a bridge of 8 that shares 2 pixels with each
    on, below = old["on the threshold"][0], old["below the threshold"][0]
    cut = old["past the cut"][0]
    return {
        "a vanish and return": (old["vanish and return"][0], 4, 100, None),
        "b gone for two": ([rects(s, A, B), rects(s, A), rects(s, A), rects(s, A, B)], 4, 100, None),
        # P (20 pixels, 20 / 32) and Q (35 pixels, the larger: rank 0; 8 / 59) both overlap the one open row
        "c two orphans": ([rects(s, big), empty, rects(s, (1, 1, 5, 6), (1, 7, 8, 12))], 4, 100, None),
        # X shares 4 of its 12 pixels with the row of frame 0 (d = 3) and 4 with the row of frame 1 (d = 2), both of 8 pixels
        "d tie in d": ([rects(s, (1, 1, 3, 5)), rects(s, (1, 7, 3, 11)), empty, rects(s, (1, 3, 3, 9))], 4, 100, None),
        "d tie in a": ([two, empty, bridge], 4, 100, None),
        "d tie in b": ([bridge, empty, two], 4, 100, None),
        # X continues T at 4 / 52 in stage 1 although it shares 32 / 40 with the open row of frame 0
        "e stage 1 wins": ([rects(s, big), rects(s, (1, 10, 5, 14)), rects(s, (1, 1, 5, 11))], 4, 50, None),
        # Y overlaps the row of frame 0, whose track went on into frame 1
        "f not open": ([rects(s, big), rects(s, (1, 1, 5, 5)), rects(s, (1, 1, 5, 5), (1, 6, 5, 9))], 4, 100, None),
        "g chain": ([rects(s, A), empty, rects(s, A), empty, rects(s, A)], 4, 100, None),
        "h link 0": (old["vanish and return"][0], 4, 100, [1, 0, 1]),
        "h size change": ([rects(s, A, B), rects((9, 18), A), rects((9, 18), A, B)], 4, 100, None),
        "i on the threshold": ([on[0], empty, on[1]], 4, 250, None),
        "i below the threshold": ([below[0], empty, below[1]], 4, 250, None),
        # k = 2: Y loses its row to Z for a frame and has one again
        "j past the cut": ([cut[0], cut[1], cut[0]], 2, 100, None),
    }


def run_gap_case(name, max_gap):
    frames, k, permille, link = gap_cases()[name]
    labels, dets, counts = inputs_np(frames, k)
    return bridge_np(labels, dets, counts, link or [1] * len(frames), permille, max_gap), dets, counts


def hand_checks(run):
    """The table of the hand-built cases, asserted on run(name, max_gap) -> a result with bridge_np's fields."""
    r = run("a vanish and return", 1)
    assert r.ids[:, :2].tolist() == [[0, 1], [0, -1], [0, 1]] and r.back[2, :2].tolist() == [1, 2] and r.prev[2, :2].tolist() == [0, 1]
    assert r.next_id == 2 and r.open[:, :2].tolist() == [[0, 0], [0, 0], [1, 1]] and r.gap_inter[2, 0, 1, 1] == 12
    r = run("b gone for two", 1)
    assert r.ids[3, :2].tolist() == [0, 2] and r.back[3, :2].tolist() == [1, 0] and r.next_id == 3
    r = run("b gone for two", 2)
    assert r.ids[3, :2].tolist() == [0, 1] and r.back[3, :2].tolist() == [1, 3] and r.next_id == 2 and r.gap_inter[3, 1, 1, 1] == 12
    r = run("c two orphans", 1)  # the larger IoU takes the row although it is the lower rank
    assert r.gap_inter[2, 0, 0, :2].tolist() == [8, 20] and r.ids[2, :2].tolist() == [1, 0] and r.back[2, :2].tolist() == [0, 2]
    r = run("d tie in d", 2)
    assert r.gap_inter[3, :, 0, 0].tolist() == [4, 4] and r.back[3, 0] == 2 and r.ids[3, 0] == 1 and r.open[:2, 0].tolist() == [1, 0]
    r = run("d tie in a", 1)
    assert r.gap_inter[2, 0, :2, 0].tolist() == [2, 2] and r.prev[2, 0] == 0 and r.ids[2, 0] == 0 and r.open[0, :2].tolist() == [0, 1]
    r = run("d tie in b", 1)
    assert r.gap_inter[2, 0, 0, :2].tolist() == [2, 2] and r.back[2, :2].tolist() == [2, 0] and r.ids[2, :2].tolist() == [0, 1]
    r = run("e stage 1 wins", 1)
    assert r.match[2, 0] == 0 and r.inter[2, 0, 0] == 4 and r.gap_inter[2, 0, 0, 0] == 32
    assert r.back[2, 0] == 1 and r.ids[:, 0].tolist() == [0, 1, 1] and r.open[0, 0] == 1
    r = run("f not open", 1)
    assert r.gap_inter[2, 0, 0, 1] == 12 and r.back[2, :2].tolist() == [1, 0] and r.ids[2, :2].tolist() == [0, 1] and r.open[0, 0] == 0
    r = run("g chain", 1)
    assert r.ids[:, 0].tolist() == [0, -1, 0, -1, 0] and r.back[:, 0].tolist() == [0, 0, 2, 0, 2] and r.open[:, 0].tolist() == [0, 0, 0, 0, 1]
    assert r.next_id == 1
    for name in ("h link 0", "h size change"):
        r = run(name, 2)
        assert r.linked.tolist() == [0, 0, 1] and not r.gap_inter.any() and r.back[2, :2].tolist() == [1, 0] and (r.back < 2).all(), name
        assert r.seq_tracks.tolist() == [2, 0, 2]
    r = run("i on the threshold", 1)
    assert r.gap_inter[2, 0, 0, 0] == 2 and r.back[2, 0] == 2 and r.ids[2, 0] == 0 and r.next_id == 1
    r = run("i below the threshold", 1)
    assert r.gap_inter[2, 0, 0, 0] == 2 and r.back[2, 0] == 0 and r.ids[2, 0] == 1 and r.next_id == 2
    r = run("j past the cut", 1)
    assert r.ids.tolist() == [[0, 1], [0, 2], [0, 1]] and r.back[2].tolist() == [1, 2] and r.prev[2].tolist() == [0, 1]


def test_the_hand_built_cases_on_the_restatement():
    hand_checks(lambda name, g: run_gap_case(name, g)[0])
    # without gaps the same frames come back under new ids: what links_np says
    frames, k, permille, _ = gap_cases()["a vanish and return"]
    labels, dets, counts = inputs_np(frames, k)
    plain = links_np(labels, dets, counts, [1] * 3, permille)
    assert plain.ids[2, :2].tolist() == [0, 2] and plain.next_id == 3
    for name in gap_cases():
        for g in (1, 2, 8):
            r, dets, counts = run_gap_case(name, g)
            frames, k, permille, link = gap_cases()[name]
            s1 = links_np(inputs_np(frames, k)[0], dets, counts, link or [1] * len(frames), permille)
            assert all(np.array_equal(getattr(r, f), getattr(s1, f)) for f in ("inter", "match", "linked")) and no_id_twice(r.ids), (name, g)


def sequence_inputs(size_index, density, k, conn, min_area=2):
    frames = flicker(moving_sequence(ragged_masks(density)[size_index], 7, 1), 5)
    return (frames,) + inputs_np(frames, k, min_area, conn)


def test_the_random_inputs_bridge_at_every_distance():
    """What the GPU comparison relies on: at max_gap = 3 the restatement bridges at every distance 2..4, and fewer tracks remain."""
    for size_index, density, k, conn in ((3, 0.3, 64, 8), (5, 0.45, 16, 4)):
        _, labels, dets, counts = sequence_inputs(size_index, density, k, conn)
        r = bridge_np(labels, dets, counts, [1] * 7, 100, 3)
        got = bridges(r)
        assert set(got) == {2, 3, 4} and all(got.values()), (size_index, got)
        assert r.next_id < links_np(labels, dets, counts, [1] * 7, 100).next_id and no_id_twice(r.ids)
        assert int((r.back >= 2).sum()) == links_np(labels, dets, counts, [1] * 7, 100).next_id - r.next_id  # one track fewer per bridge


@pytest.mark.parametrize("max_gap", [1, 3])
def test_history_restated_a_sequence_in_pieces_is_the_sequence(max_gap):
    _, labels, dets, counts = sequence_inputs(3, 0.3, 64, 8)
    whole = bridge_np(labels, dets, counts, [1] * 7, 100, max_gap)
    assert (whole.back >= 2).sum() >= 20
    for cuts in ((3, 3, 1), (1,) * 7):
        hist, s = None, 0
        for c in cuts:
            part = bridge_np(labels[s:s + c], dets[s:s + c], counts[s:s + c], [1] * c, 100, max_gap, hist)
            lo = 1 if s == 0 else 0
            for f in ("inter", "match", "ids", "gap_inter", "back", "prev"):
                assert np.array_equal(getattr(part, f)[lo:], getattr(whole, f)[s + lo:s + c]), (cuts, s, f)
            assert part.linked.tolist() == whole.linked[s:s + c].tolist() and part.seq_tracks[-1] == part.next_id
            hist = history_np(part, labels[s:s + c], dets[s:s + c], counts[s:s + c], max_gap, hist)
            s += c
            assert hist.m == min(max_gap + 1, s) and np.array_equal(hist.ids, whole.ids[s - hist.m:s])
            want = np.array(whole.open[s - hist.m:s])  # the open flags so far: those of the whole, without what later frames closed
            for c2 in range(s, 7):
                for b in range(64):
                    d = int(whole.back[c2, b])
                    if d and s - hist.m <= c2 - d < s:
                        want[c2 - d - (s - hist.m), whole.prev[c2, b]] = 1
            assert np.array_equal(hist.open, want), (cuts, s)
        assert part.next_id == whole.next_id
    claimed_once(lambda labels, dets, counts, link, permille, max_gap, history=None: bridge_np(labels, dets, counts, link, permille, max_gap, history),
                 history_np)


def claimed_once(run, tail):
    """A history row bridged to in one call cannot be claimed again in the next, and a history of another size is left alone.  run: bridge_np
    or the device behind its signature; tail(result, labels, dets, counts, max_gap, history) -> the next call's history."""
    s, A = (8, 18), (1, 1, 6, 7)
    # B (12 pixels) is missing in frame 1; its left half comes back in frame 2 and takes the open row of frame 0 (6 / 12); the right half,
    # alone in frame 3, overlaps that row just as well -- but it is closed, in the history's flags
    frames = [rects(s, A, (2, 10, 5, 14)), rects(s, A), rects(s, A, (2, 10, 5, 12)), rects(s, A, (2, 12, 5, 14))]
    labels, dets, counts = inputs_np(frames, 4)
    first = run(labels[:3], dets[:3], counts[:3], [1] * 3, 100, 2)
    assert first.back[2, :2].tolist() == [1, 2] and first.ids[2, :2].tolist() == [0, 1] and first.open[0, :2].tolist() == [0, 0]
    hist = tail(first, labels[:3], dets[:3], counts[:3], 2, None)
    assert hist.m == 3 and _np(hist.open)[:, :2].tolist() == [[0, 0], [0, 0], [1, 1]]
    last = run(labels[3:], dets[3:], counts[3:], [1], 100, 2, hist)
    assert last.gap_inter[0, 1, 1, 1] == 6 and last.back[0, :2].tolist() == [1, 0] and last.ids[0, :2].tolist() == [0, 2] and last.next_id == 3
    assert _np(last.hist_open)[:, :2].tolist() == [[0, 0], [0, 0], [0, 1]] and _np(hist.open)[2, 0] == 1  # closed in the call's copy
    whole = run(labels, dets, counts, [1] * 4, 100, 2)
    assert np.array_equal(whole.ids[3], last.ids[0]) and np.array_equal(whole.back[3], last.back[0])
    # a history of another size: frame 0 starts a sequence and the history stays as it is
    other = inputs_np([rects((9, 18), A)], 4)
    alone = run(other[0], other[1], other[2], [1], 100, 2, hist)
    assert alone.linked.tolist() == [0] and alone.ids[0, 0] == 0 and np.array_equal(_np(alone.hist_open), _np(hist.open)) and alone.next_id == 1
    assert not alone.gap_inter.any()


# ------------------------------------------------------------------------------------------------ arguments and the header ----
GAP_OK = dict(LINK_OK, max_gap=2, m=0, h_labels=None, h_h=0, h_w=0, h_dets=None, h_counts=None, h_ids=None, h_open=None, h_next=None,
              gap_inter=2048, back=576, prev=640, open=704)
GAP_ORDER = ("labels n offsets hw max_h max_w total dets counts k link max_gap m h_labels h_h h_w h_dets h_counts h_ids h_open h_next permille "
             "inter match ids linked seq next_id gap_inter back prev open ws ws_bytes stream").split()
HIST_OK = dict(m=2, h_labels=64, h_h=30, h_w=53, h_dets=256, h_counts=512, h_ids=64, h_open=128, h_next=64)
GAP_BAD = ([dict(**{p: None}) for p in ("labels", "offsets", "hw", "dets", "counts", "link", "inter", "match", "ids", "linked", "seq", "next_id", "ws",
                                        "gap_inter", "back", "prev", "open")] +
           [dict(n=0), dict(n=65536), dict(k=0), dict(k=65), dict(permille=0), dict(permille=1001), dict(max_h=0), dict(max_w=0), dict(total=0),
            dict(max_gap=0), dict(max_gap=9), dict(max_gap=-1), dict(m=1), dict(m=-1), dict(HIST_OK, m=0), dict(HIST_OK, m=4), dict(HIST_OK, m=-2),
            dict(HIST_OK, h_open=None), dict(HIST_OK, h_next=None), dict(HIST_OK, h_labels=None), dict(HIST_OK, h_h=0), dict(h_h=30, h_w=53),
            dict(ws_bytes=64), dict(ws=66), dict(labels=66), dict(link=65), dict(dets=260), dict(counts=516), dict(inter=1028), dict(ids=130),
            dict(gap_inter=2052), dict(back=578), dict(prev=641), dict(open=706), dict(HIST_OK, h_dets=260), dict(HIST_OK, h_counts=516),
            dict(HIST_OK, h_ids=66), dict(HIST_OK, h_open=130), dict(HIST_OK, h_labels=65), dict(HIST_OK, ws_bytes=4 * (3180 + 30 * 53))])


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    ws = lib.udet_link_detections_gap_workspace_bytes
    assert ws(1000, 2, 16, 1, 0, 0, 0) == 4 * 1000 and ws(1000, 2, 16, 8, 0, 0, 0) == 4 * 1000
    assert ws(1000, 2, 16, 2, 3, 10, 20) == 4 * 1600 and ws(1000, 2, 16, 8, 9, 10, 20) == 4 * 2800  # one int32 per pixel, the history's too
    for bad in ((0, 2, 16, 1, 0, 0, 0), (1000, 0, 16, 1, 0, 0, 0), (1000, 2, 0, 1, 0, 0, 0), (1000, 2, 65, 1, 0, 0, 0), (1000, 2, 16, 0, 0, 0, 0),
                (1000, 2, 16, 9, 0, 0, 0), (1000, 2, 16, 2, 4, 10, 20), (1000, 2, 16, 2, -1, 10, 20), (1000, 2, 16, 2, 0, 10, 20),
                (1000, 2, 16, 2, 1, 0, 20), (1000, 2, 16, 2, 1, 10, -1)):
        assert ws(*bad) == 0, bad
    for change in GAP_BAD:
        a = dict(GAP_OK, **change)
        assert lib.udet_link_detections_gap_ragged(*[a[p] for p in GAP_ORDER]) == -5 and b"link_detections_gap_ragged" in lib.udet_last_error(), change


def test_the_header_says_what_the_symbols_do():
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert re.search(r"\bsize_t udet_link_detections_gap_workspace_bytes\(size_t total_pixels, int n, int k, int max_gap, int m, int hist_h, int hist_w\);", hdr)
    assert re.search(r"\bint udet_link_detections_gap_ragged\(const int\* labels, int n, const long long\* offsets, const int\* hw,", hdr)
    assert re.search(r"#define UDET_TRACK_MAX_GAP 8\b", hdr)
    for sentence in ("linked, inter and match are equal to it entry for entry", "is open while no row of any later frame continues it",
                     "an orphan is a row b < rows_c with match[c][b] = -1", "gap_inter[c][d - 2][a][b] (device int64 [n][max_gap][k][k])",
                     "1000 gap_inter >= min_iou_permille (area_a + area_b - gap_inter)",
                     "ties to the smaller d, then the smaller a, then the smaller b", "back[c][b] = d, prev[c][b] = a, ids[c][b] = ids[c - d][a]",
                     "a stage-1 match is never undone by a better bridge", "Within a frame no id occurs twice", "is closed in hist_open in place",
                     "Six launches whatever n", "integer atomics only", "nothing enqueued", "a history that is neither absent nor whole",
                     "Every index a kernel forms is bounded"):
        assert sentence in flat, sentence
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7.9" in design and "udet_link_detections_gap_ragged" in design and "now §7.9" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--track_max_gap" in readme


def test_wrapper_validates_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd.native_results import Detections, TrackHistory, Tracks, TrackTail, link_detections
    from unsupervised_detection_amd.ragged import PackedLayout
    hw = [(30, 53), (30, 53)]
    total, k = 2 * 30 * 53, 4
    layout = PackedLayout.packed(hw)
    lab = torch.zeros(total, dtype=torch.int32)  # host tensors: anything that got past the validation would fail on them, not launch
    det = Detections(torch.zeros((2, k, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, k)

    def history(m=2, k=k, max_gap=2, **kw):
        a = dict(labels=torch.zeros((m, 30 * 53), dtype=torch.int32), hw=(30, 53), dets=torch.zeros((m, k, 9), dtype=torch.int64),
                 counts=torch.zeros((m, 3), dtype=torch.int64), ids=torch.zeros((m, k), dtype=torch.int32),
                 open=torch.zeros((m, k), dtype=torch.int32), next_id=torch.zeros(1, dtype=torch.int32), max_gap=max_gap)
        a.update(kw)
        return TrackHistory(**a)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            link_detections(lab, det, **kw)
    for v in (-1, 9, 1.0, True, "2", None):
        bad("max_gap", max_gap=v)
    tail = TrackTail(torch.zeros(30 * 53, dtype=torch.int32), (30, 53), torch.zeros((k, 9), dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
                     torch.zeros(k, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    bad("same k = 4 and max_gap = 2", max_gap=2, carry=tail)                 # the carried frame of a link without gaps
    bad("tail\\(\\)", max_gap=0, carry=history())                             # and the other way round
    bad("same k = 4 and max_gap = 3", max_gap=3, carry=history())
    bad("same k = 4 and max_gap = 2", max_gap=2, carry=history(k=3))
    bad("1..max_gap \\+ 1 frames", max_gap=2, carry=history(m=4))
    bad("1..max_gap \\+ 1 frames", max_gap=2, carry=history(open=torch.zeros((2, 3), dtype=torch.int32)))
    bad("1..max_gap \\+ 1 frames", max_gap=2, carry=history(labels=torch.zeros((2, 30 * 53 - 1), dtype=torch.int32)))
    bad("one 0 / 1 per frame", max_gap=2, link=[1])
    bad("min_iou", max_gap=2, min_iou=0)
    bad("CUDA", max_gap=2)  # everything valid but the host tensors: refused before any call into the library
    bad("CUDA", max_gap=2, carry=history(), link=[1, 1])
    bad("CUDA", max_gap=8, carry=history(m=9, max_gap=8))
    # the positional constructor keeps working, and host() keeps returning its five arrays
    z = [torch.zeros(s, dtype=d) for s, d in (((2, k, k), torch.int64), ((2, k), torch.int32), ((2, k), torch.int32), (2, torch.int32),
                                              (2, torch.int32), (1, torch.int32))]
    old = Tracks(*z, lab, det)
    assert old.max_gap == 0 and old.back is None and len(old.host()) == 5 and isinstance(old.tail(), TrackTail)
    new = Tracks(*z, lab, det, None, back=torch.ones((2, k), dtype=torch.int32), prev=z[1], gap_inter=torch.zeros((2, 2, k, k), dtype=torch.int64),
                 open=torch.ones((2, k), dtype=torch.int32), max_gap=2)
    assert len(new.host()) == 5 and [a.shape for a in new.host_gaps()] == [(2, 2, k, k), (2, k), (2, k), (2, k)]
    t = new.tail()  # linked = [0, 0]: the last sequence is the last frame
    assert isinstance(t, TrackHistory) and (t.m, t.k, t.max_gap, t.hw) == (1, k, 2, (30, 53)) and tuple(t.labels.shape) == (1, 30 * 53)
    new.linked[1] = 1
    new._host = None
    assert new.tail().m == 2 and tuple(new.tail().open.shape) == (2, k)


def test_parameters_and_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    from unsupervised_detection_amd.native_results import track_params
    assert track_params(None) == track_params({}) == track_params({"max_gap": 0}) == track_params({"max_gap": None}) == {"min_iou": 0.1}
    assert track_params({"max_gap": 3}) == {"min_iou": 0.1, "max_gap": 3} and track_params({"min_iou": 0.5, "max_gap": 8}) == {"min_iou": 0.5, "max_gap": 8}
    for v in (-1, 9, 2.0, True, "1"):
        with pytest.raises(ValueError, match="tracks: max_gap"):
            track_params({"max_gap": v})
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    a = cli.parse_restore_results_args(base + ["--detections", "--tracks"])
    assert a.track_max_gap == 0 and cli._tracks(a) == {"min_iou": 0.1}
    assert cli._tracks(cli.parse_restore_results_args(base + ["--detections", "--tracks", "--track_max_gap", "0"])) == {"min_iou": 0.1}
    assert cli._tracks(cli.parse_restore_results_args(base + ["--detections", "--tracks", "--track_max_gap", "3", "--track_min_iou", "0.25"])) == \
        {"min_iou": 0.25, "max_gap": 3}
    for bad, said in ((["--track_max_gap", "2"], "it needs --tracks"), (["--detections", "--track_max_gap", "2"], "it needs --tracks"),
                      (["--tracks", "--track_max_gap", "2"], "it needs --detections"),
                      (["--detections", "--tracks", "--track_max_gap", "9"], "--track_max_gap"),
                      (["--detections", "--tracks", "--track_max_gap", "-1"], "--track_max_gap")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    assert default_flags().track_max_gap == 0
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D"]
    f = parse_flags(native + ["--detections", "--tracks", "--track_max_gap", "2"])
    cli.check_native_flags(f)
    assert cli._tracks(f) == {"min_iou": 0.1, "max_gap": 2}
    with pytest.raises(SystemExit) as e:
        cli.check_native_flags(parse_flags(native + ["--detections", "--track_max_gap", "2"]))
    assert "it needs --tracks" in str(e.value)
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R"]
    assert cli._tracks(cli.parse_post_process_args(pp + ["--detections", "--tracks", "--track_max_gap", "1"])) == {"min_iou": 0.1, "max_gap": 1}
    with pytest.raises(SystemExit) as e:
        cli.parse_post_process_args(pp + ["--track_max_gap", "1"])
    assert "it needs --tracks" in str(e.value)
    assert "--track_max_gap" in cli.__doc__


# ------------------------------------------------------------------------------------------------- records and the summary ----
class TracksGapNp(TracksNp):
    """bridge_np's result with the interface of native_results.Tracks that restore_results_dir and track_records use."""

    def __init__(self, r, labels, detections, carry, max_gap):
        TracksNp.__init__(self, r, labels, detections, carry)
        self.max_gap = max_gap

    def host_gaps(self):
        return self.r.gap_inter, self.r.back, self.r.prev, self.r.open

    def tail(self):
        return history_np(self.r, self.labels, self.detections.dets, self.detections.counts, self.max_gap, self.carry)


def link_gap_np(calls):
    """Stand-in for link_detections(max_gap=...) over the stand-ins of test_detections."""
    def link(labelled, det, link=None, carry=None, min_iou=0.1, max_gap=0):
        from unsupervised_detection_amd.native_results import min_iou_permille
        calls.append((list(link), None if carry is None else carry.m, min_iou, max_gap))
        r = bridge_np(labelled.labels, det.dets, det.counts, link, min_iou_permille(min_iou), max_gap, carry)
        return TracksGapNp(r, labelled.labels, det, carry, max_gap)
    return link


def test_track_records_and_summary_arithmetic():
    from unsupervised_detection_amd.native_results import detection_records, summarise_tracks, track_records
    frames, k, permille, _ = gap_cases()["b gone for two"]
    labels, dets, counts = inputs_np(frames, k)
    det = DetectionsNp(dets, counts)
    recs = detection_records(det, [255] * 4)
    r = bridge_np(labels, dets, counts, [1] * 4, permille, 2)
    got = track_records(recs, TracksGapNp(r, labels, det, None, 2))
    assert [[(d["track"], d["back"], d["prev"], d["iou"]) for d in f] for f in got] == [
        [(0, 0, None, None), (1, 0, None, None)], [(0, 1, 0, 1.0)], [(0, 1, 0, 1.0)], [(0, 1, 0, 1.0), (1, 3, 1, 1.0)]]
    assert all(set(d) == set(recs[0][0]) | {"track", "prev", "iou", "back"} for f in got for d in f)
    json.dumps(got)
    # the last frame alone against the history of the first three: the bridged row's area comes from the history
    hist = history_np(bridge_np(labels[:3], dets[:3], counts[:3], [1] * 3, permille, 2), labels[:3], dets[:3], counts[:3], 2)
    last = bridge_np(labels[3:], dets[3:], counts[3:], [1], permille, 2, hist)
    alone = track_records(recs[3:], TracksGapNp(last, labels[3:], DetectionsNp(dets[3:], counts[3:]), hist, 2))
    assert alone == got[3:] and last.hist_open[:, :2].tolist() == [[0, 0], [0, 0], [0, 0]] and hist.open[0, 1] == 1
    # an IoU below 1 through a gap: gap_inter, not inter
    frames, k, permille, _ = gap_cases()["c two orphans"]
    labels, dets, counts = inputs_np(frames, k)
    r = bridge_np(labels, dets, counts, [1] * 3, permille, 1)
    got = track_records(detection_records(DetectionsNp(dets, counts), [255] * 3), TracksGapNp(r, labels, DetectionsNp(dets, counts), None, 1))
    assert [(d["track"], d["back"], d["prev"], d["iou"]) for d in got[2]] == [(1, 0, None, None), (0, 2, 0, 20 / 32)]
    # without max_gap the records are what they were
    plain = track_records(detection_records(DetectionsNp(dets, counts), [255] * 3), TracksNp(links_np(labels, dets, counts, [1] * 3, permille),
                                                                                           labels, DetectionsNp(dets, counts), None))
    assert all("back" not in d for f in plain for d in f)
    rec = lambda t, back, area=4, score=0.5: {"track": t, "back": back, "area": area, "score": score, "box": [0, 0, 1, 1]}
    s = summarise_tracks(list("abcdef"), [[rec(0, 0), rec(1, 0)], [rec(0, 1)], [rec(0, 1), rec(1, 3)], [], [rec(0, 0)], [rec(0, 2)]],
                         [True, False, False, False, True, False])
    assert [(q["first"], q["frames"], q["bridged"]) for q in s] == [("a", 4, 1), ("e", 2, 1)] and list(s[0]) == ["first", "frames", "tracks", "bridged"]
    assert [(t["id"], t["frames"], t["span"], t["gaps"]) for t in s[0]["tracks"]] == [(0, 3, 3, 0), (1, 2, 3, 1)]
    assert [(t["id"], t["first"], t["last"], t["frames"], t["span"], t["gaps"]) for t in s[1]["tracks"]] == [(0, "e", "f", 2, 2, 0)]
    old = summarise_tracks(["a"], [[{k: v for k, v in rec(0, 0).items() if k != "back"}]], [True])
    assert list(old[0]) == ["first", "frames", "tracks"] and "span" not in old[0]["tracks"][0]
    assert summarise_tracks(["a"], [[]], [True], gaps=True) == [{"first": "a", "frames": 1, "tracks": [], "bridged": 0}]


# ------------------------------------------------------------------------------------------------------ restore_results_dir ----
def test_restore_results_dir_with_max_gap(tmp_path):
    calls, calls7, calls0 = [], [], []
    det = dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3})
    out, js, masks = run_tree(tmp_path, "gap", False, 3, tracks={"min_iou": 0.2, "max_gap": 2}, link=link_gap_np(calls), **det)
    out7, js7, _ = run_tree(tmp_path, "gap7", False, 7, tracks={"min_iou": 0.2, "max_gap": 2}, link=link_gap_np(calls7), **det)
    assert calls == [([0, 1, 1], None, 0.2, 2), ([1, 1, 1], 3, 0.2, 2), ([1], 3, 0.2, 2)] * 2 and calls7 == [([0] + [1] * 6, None, 0.2, 2)] * 2
    assert js["tracks"] == {"min_iou": 0.2, "max_gap": 2} and js == js7
    f3, f7 = _tree_files(out), _tree_files(out7)
    assert sorted(f3) == sorted(f7) and all(f3[k] == f7[k] for k in f3)  # batch 3 and batch 7: the same files, byte for byte
    with open(os.path.join(out, "tracks", "bear.json")) as f:
        summary = json.load(f)
    assert all("bridged" in s and all(t["gaps"] == t["span"] - t["frames"] for t in s["tracks"]) for s in summary)
    with open(os.path.join(out, "detections", "bear.json")) as f:
        assert all("back" in d for recs in json.load(f).values() for d in recs)
    # max_gap absent or 0: the existing stand-in, which does not take the argument, and every byte of a run without the key
    outs = [run_tree(tmp_path, name, False, 3, tracks=t, link=link_np(calls0), **det) for name, t in
            (("none", {"min_iou": 0.2}), ("zero", {"min_iou": 0.2, "max_gap": 0}), ("null", {"min_iou": 0.2, "max_gap": None}))]
    assert outs[0][1] == outs[1][1] == outs[2][1] and outs[0][1]["tracks"] == {"min_iou": 0.2}
    f0, f1, f2 = (_tree_files(o[0]) for o in outs)
    assert sorted(f0) == sorted(f1) == sorted(f2) and all(f0[k] == f1[k] == f2[k] for k in f0)
    with pytest.raises(ValueError, match="needs detections"):
        run_tree(tmp_path, "bad", False, 3, tracks={"max_gap": 2}, link=link_gap_np([]), select=select_labels_np([]))
    with pytest.raises(ValueError, match="max_gap"):
        run_tree(tmp_path, "bad2", False, 3, tracks={"max_gap": 9}, link=link_gap_np([]), **det)
