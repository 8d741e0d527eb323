"""Time native_results.link_detections (udet_link_detections_ragged: four launches per batch) on labels and detections that are already
on the device, next to the only alternative there was before it: .cpu() of the packed labels, dets and counts, the overlap of every pair
of consecutive frames by np.bincount and the matching and the id walk in Python.  16 consecutive frames of 480 x 854 hold moving blobs
(discs that drift, grow, appear and vanish, over specks below min_area); they are labelled (select_components, mode "label") and boxed
(component_boxes, k = 16, min_area 64) once, outside the timing.  The device path goes through its Python wrapper, as a user calls it,
and is timed with HIP events around `--iters` back-to-back calls; the host path is timed with a host clock around the copies (which
synchronise) and the loop.  They alternate over `--rounds` rounds after a warm-up in which the two must be equal in every entry; the
figures are the per-batch median and the min .. max over the rounds.

    python tools/tracks_bench.py [--n 16 --h 480 --w 854 --k 16 --min_area 64 --blobs 12 --iters 10 --rounds 5]

--max_gap G [G ...] measures the link with gap bridging (udet_link_detections_gap_ragged: six launches) as well: every
blob is then blanked on one or two frames inside its span, and each G is timed through the wrapper in the same rounds as G = 0 (the
old entry) and next to .cpu() + the numpy restatement with that G (tests/test_track_gaps.py, bridge_np), with which it must be equal in
every entry first.  The JSON line gains "max_gap": per G the two timings, the rows bridged and the tracks that remain.

    python tools/tracks_bench.py --max_gap 1 2 8
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

LAUNCHES = 4  # csrc/tracks.hip: init, overlap, match, ids


def moving_blobs(n, h, w, blobs, rng, blank=False):
    """n binary frames [h, w]: `blobs` discs that drift a few pixels per frame and change their radius, each present over its own span of
    frames, plus a few single-pixel specks per frame.  blank: every blob is also missing from one or two consecutive frames inside its
    span (drawn after everything else, so that the frames without it are what they were)."""
    y, x = np.mgrid[:h, :w]
    cy, cx = rng.uniform(0.1 * h, 0.9 * h, blobs), rng.uniform(0.1 * w, 0.9 * w, blobs)
    vy, vx = rng.uniform(-4, 4, blobs), rng.uniform(-6, 6, blobs)
    r0, dr = rng.uniform(0.03 * h, 0.12 * h, blobs), rng.uniform(-1, 1, blobs)
    first, last = rng.integers(0, n // 3 + 1, blobs), rng.integers(2 * n // 3, n + 1, blobs)
    frames = []
    for t in range(n):
        m = np.zeros((h, w), np.uint8)
        for b in range(blobs):
            if first[b] <= t < last[b]:
                m[(y - cy[b] - vy[b] * t) ** 2 + (x - cx[b] - vx[b] * t) ** 2 <= (r0[b] + dr[b] * t) ** 2] = 1
        m[rng.integers(0, h, 200), rng.integers(0, w, 200)] = 1
        frames.append(m)
    if blank:
        at, length = rng.integers(first + 1, np.maximum(first + 2, last - 2)), rng.integers(1, 3, blobs)
        for t in range(n):
            gone = [b for b in range(blobs) if at[b] <= t < at[b] + length[b]]
            if gone:
                m = np.zeros((h, w), np.uint8)
                for b in range(blobs):
                    if first[b] <= t < last[b] and b not in gone:
                        m[(y - cy[b] - vy[b] * t) ** 2 + (x - cx[b] - vx[b] * t) ** 2 <= (r0[b] + dr[b] * t) ** 2] = 1
                frames[t] = m | (frames[t] & (np.add.reduce([(y - cy[b] - vy[b] * t) ** 2 + (x - cx[b] - vx[b] * t) ** 2 <= (r0[b] + dr[b] * t) ** 2
                                                             for b in gone]) == 0))  # the specks outside the blanked discs stay
    return frames


def links_host(labels, hw, dets, counts, link, permille):
    """The alternative, on host arrays: per pair of consecutive frames the ranks of both frames' pixels through a root -> rank table, inter
    by np.bincount, the greedy matching over the candidates sorted by exact fractions, the id walk -> (inter, match, ids, linked,
    seq_tracks, next_id) as udet_link_detections_ragged defines them."""
    from fractions import Fraction
    n, k = dets.shape[:2]
    inter, match, ids = np.zeros((n, k, k), np.int64), np.full((n, k), -1, np.int32), np.full((n, k), -1, np.int32)
    linked, seq_tracks, next_id = np.zeros(n, np.int32), np.zeros(n, np.int32), 0
    rows = np.clip(counts[:, 2], 0, k).astype(int)
    pos = np.concatenate([[0], np.cumsum([H * W for H, W in hw])])
    ranks = []
    for i, (H, W) in enumerate(hw):
        v = labels[pos[i]:pos[i + 1]].astype(np.int64)
        table = np.full(H * W + 1, -1, np.int64)
        table[dets[i, :rows[i], 0] + 1] = np.arange(rows[i])
        ranks.append(table[np.where((v >= 1) & (v <= H * W), v, 0)])
    for i in range(n):
        if not (i and link[i] and tuple(hw[i]) == tuple(hw[i - 1])):
            if i:
                seq_tracks[i - 1] = next_id
            ids[i, :rows[i]] = np.arange(rows[i])
            next_id = rows[i]
            continue
        linked[i] = 1
        both = (ranks[i - 1] >= 0) & (ranks[i] >= 0)
        inter[i] = np.bincount(ranks[i - 1][both] * k + ranks[i][both], minlength=k * k).reshape(k, k)
        cands = []
        for a, b in zip(*np.nonzero(inter[i])):
            it = int(inter[i, a, b])
            union = int(dets[i - 1, a, 1]) + int(dets[i, b, 1]) - it
            if 1000 * it >= permille * union:
                cands.append((-Fraction(it, union), int(a), int(b)))
        for _, a, b in sorted(cands):
            if match[i, b] < 0 and a not in match[i]:
                match[i, b] = a
        for b in range(rows[i]):
            if match[i, b] >= 0:
                ids[i, b] = ids[i - 1, match[i, b]]
            else:
                ids[i, b], next_id = next_id, next_id + 1
    seq_tracks[n - 1] = next_id
    return inter, match, ids, linked, seq_tracks, next_id


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("h", 480), ("w", 854), ("k", 16), ("min_area", 64), ("blobs", 12), ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--min_iou", type=float, default=0.1)
    ap.add_argument("--max_gap", type=int, nargs="*", default=[], help="also measure the link with gap bridging for these G (1..8)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_detections import component_boxes
    from unsupervised_detection_amd.native_tracks import link_detections, min_iou_permille
    from unsupervised_detection_amd.ragged import PackedLayout
    frames = moving_blobs(a.n, a.h, a.w, a.blobs, np.random.default_rng(0), blank=bool(a.max_gap))
    hw = [(a.h, a.w)] * a.n
    layout = PackedLayout.packed(hw)
    binary = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    sel = select_components(binary, layout, mode="label", connectivity=8, want_labels=True)
    det = component_boxes(sel, min_area=a.min_area, max_detections=a.k)
    link = [0] + [1] * (a.n - 1)
    d_link = torch.tensor(link, dtype=torch.int32, device="cuda")
    permille = min_iou_permille(a.min_iou)

    def device():
        return link_detections(sel, det, link=d_link, min_iou=a.min_iou)

    def host():
        return links_host(sel.labels.cpu().numpy(), hw, det.dets.cpu().numpy(), det.counts.cpu().numpy(), link, permille)
    got, want = device(), host()  # warm-up of both, and they must be equal in every entry before either is timed
    for g, w in zip(got.host(), want[:5]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert int(got.next_id.cpu()[0]) == want[5]
    torch.cuda.synchronize()
    gaps = {}
    if a.max_gap:  # the restatement of the tests is the alternative: .cpu() of the same three buffers, then numpy and Python
        sys.path.append(os.path.join(ROOT, "tests"))
        from test_track_gaps import GAP_FIELDS, bridge_np

        def host_gap(g):
            lab = sel.labels.cpu().numpy().reshape(a.n, a.h, a.w)
            return bridge_np(list(lab), det.dets.cpu().numpy(), det.counts.cpu().numpy(), link, permille, g)
        for g in a.max_gap:
            got_g, want_g = link_detections(sel, det, link=d_link, min_iou=a.min_iou, max_gap=g), host_gap(g)
            for f, v in zip(GAP_FIELDS, got_g.host() + got_g.host_gaps()):
                assert np.array_equal(v, getattr(want_g, f)), (g, f)
            gaps[g] = {"bridged": int((want_g.back >= 2).sum()), "tracks": int(want_g.next_id), "device": [], "host": []}
        torch.cuda.synchronize()
    t = {"device": [], "host": []}
    for _ in range(a.rounds):
        for g, rec in gaps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                link_detections(sel, det, link=d_link, min_iou=a.min_iou, max_gap=g)
            e1.record()
            torch.cuda.synchronize()
            rec["device"].append(e0.elapsed_time(e1) / a.iters)
            t0 = time.perf_counter()
            host_gap(g)
            rec["host"].append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            device()
        e1.record()
        torch.cuda.synchronize()
        t["device"].append(e0.elapsed_time(e1) / a.iters)
        t0 = time.perf_counter()
        host()
        t["host"].append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    counts = det.counts.cpu().numpy()
    print(json.dumps({"shape": [a.n, a.h, a.w], "k": a.k, "min_area": a.min_area, "min_iou": a.min_iou, "iters": a.iters, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "rows_mean": float(counts[:, 2].mean()),
                      "matched": int((want[1] >= 0).sum()), "tracks": int(want[5]), "link_detections": stat(t["device"]),
                      "host": stat(t["host"]), "ratio_host_over_link_detections": float(np.median(t["host"]) / np.median(t["device"])),
                      **({"max_gap": {str(g): {"launches": 6, "bridged": r["bridged"], "tracks": r["tracks"], "link_detections": stat(r["device"]),
                                               "host": stat(r["host"])} for g, r in gaps.items()}} if gaps else {})}))


if __name__ == "__main__":
    main()
