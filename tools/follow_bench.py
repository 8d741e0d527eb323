"""Time native_results.follow_tracks (udet_follow_tracks_ragged: two launches per batch) on labels and detections that are already on the
device, next to the only alternative there was before it: .cpu() of the packed labels, dets, counts and annotations and numpy over every
frame for the masks and the four counts.  16 consecutive frames of 480 x 854 hold the moving blobs of tools/tracks_bench.py; they are
labelled, boxed (k = 16, min_area 64) and linked once, outside the timing, and the keep words are those of the track native_results.choose_tracks
follows under `--rule`; the annotation is the first frame's mask shifted along.  The device path goes through its Python wrapper, as a user
calls it, and is timed with HIP events around `--iters` back-to-back calls; the host path with a host clock around the copies (which
synchronise) and the loop.  They alternate over `--rounds` rounds after a warm-up in which device and host must be equal in every byte; the
figures are the per-batch median and the min .. max over the rounds.

    python tools/follow_bench.py [--n 16 --h 480 --w 854 --k 16 --min_area 64 --blobs 12 --rule mass --iters 10 --rounds 5]
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


def follow_host(labels, hw, dets, counts, words, gt):
    """The alternative, on host arrays: per frame a root -> kept table and one gather -> (selected [total] uint8, stats [n, 4]) as
    udet_follow_tracks_ragged defines them."""
    n, k = dets.shape[:2]
    out, stats = np.zeros(len(labels), np.uint8), np.zeros((n, 4), np.int64)
    rows = np.clip(counts[:, 2], 0, k).astype(int)
    pos = np.concatenate([[0], np.cumsum([H * W for H, W in hw])])
    for i, (H, W) in enumerate(hw):
        v = labels[pos[i]:pos[i + 1]].astype(np.int64)
        g = gt[pos[i]:pos[i + 1]] != 0
        table = np.zeros(H * W + 1, bool)
        r = np.arange(rows[i])
        table[dets[i, r, 0] + 1] = np.array([(int(words[i]) >> int(b)) & 1 for b in r], bool)
        inside = (v >= 1) & (v <= H * W)
        kept = table[np.where(inside, v, 0)]
        out[pos[i]:pos[i + 1]] = kept
        stats[i] = [kept.sum(), (inside & ~kept).sum(), (kept & g).sum(), g.sum()]
    return out, stats


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("h", 480), ("w", 854), ("k", 16), ("min_area", 64), ("blobs", 12), ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--rule", default="mass", choices=("mass", "area", "length", "all"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from tracks_bench import moving_blobs
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_detections import component_boxes
    from unsupervised_detection_amd.native_follow import choose_tracks, follow_tracks, keep_words
    from unsupervised_detection_amd.native_tracks import link_detections
    from unsupervised_detection_amd.ragged import PackedLayout
    rng = np.random.default_rng(0)
    frames = moving_blobs(a.n, a.h, a.w, a.blobs, rng)
    hw = [(a.h, a.w)] * a.n
    layout = PackedLayout.packed(hw)
    binary = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    score = torch.from_numpy(rng.integers(1, 256, layout.numel, dtype=np.uint8)).cuda()
    gt = torch.from_numpy(np.concatenate([np.roll(frames[0], (2 * t, 3 * t), (0, 1)).reshape(-1) for t in range(a.n)])).cuda()
    sel = select_components(binary, layout, mode="label", connectivity=8, want_labels=True)
    det = component_boxes(sel, score=score, min_area=a.min_area, max_detections=a.k)
    trk = link_detections(sel, det, link=[0] + [1] * (a.n - 1))
    dets, counts, ids = det.dets.cpu().numpy(), det.counts.cpu().numpy(), trk.ids.cpu().numpy()
    records = [[{"track": int(ids[i, r]), "area": int(dets[i, r, 1])} for r in range(int(counts[i, 2]))] for i in range(a.n)]
    sums = [[int(v) for v in dets[i, :len(r), 8]] for i, r in enumerate(records)]
    ranks, followed = choose_tracks(records, sums, [True] + [False] * (a.n - 1), a.rule, 1)
    words = keep_words(ranks, a.n)
    keep = torch.from_numpy(words.view(np.int64)).cuda()

    def device():
        return follow_tracks(sel, det, keep, gt=gt)

    def host():
        return follow_host(sel.labels.cpu().numpy(), hw, det.dets.cpu().numpy(), det.counts.cpu().numpy(), words, gt.cpu().numpy())
    got, want = device(), host()  # warm-up of both, and device and host must be equal in every byte before either is timed
    assert np.array_equal(got.selected.cpu().numpy(), want[0]) and np.array_equal(got.host(), want[1])
    torch.cuda.synchronize()
    t = {"device": [], "host": []}
    for _ in range(a.rounds):
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
    stats = got.host()
    print(json.dumps({"shape": [a.n, a.h, a.w], "k": a.k, "min_area": a.min_area, "rule": a.rule, "iters": a.iters, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0), "rows_mean": float(counts[:, 2].mean()), "tracks": int(trk.next_id.cpu()[0]),
                      "followed": followed, "frames_with_a_kept_row": int((stats[:, 0] > 0).sum()), "kept_pixels": int(stats[:, 0].sum()),
                      "dropped_pixels": int(stats[:, 1].sum()), "kept_gt_pixels": int(stats[:, 2].sum()),
                      "follow_tracks": dict(stat(t["device"]), launches=2), "follow_tracks_host": stat(t["host"]),
                      "ratio_host_over_follow_tracks": float(np.median(t["host"]) / np.median(t["device"]))}))


if __name__ == "__main__":
    main()
