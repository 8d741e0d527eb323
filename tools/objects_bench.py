"""Time native_results.object_overlaps (udet_track_object_overlaps_ragged: two launches per batch) on labels, detections and object
annotations that are already on the device, next to the only alternative there was before it: .cpu() of the packed labels, dets, counts
and object bytes and numpy over every frame for row_obj, obj_area and frame_stats.  16 consecutive frames of 480 x 854 hold the moving
blobs of tools/tracks_bench.py; they are labelled and boxed (k = 16, min_area 64) once, outside the timing; the object annotation cuts
every frame into O = 8 vertical bands of objects that drift along with the frames, with a strip of void bytes.  The device path goes
through its Python wrapper, as a user calls it, and is timed with HIP events around `--iters` back-to-back calls; the host path with a host
clock around the copies (which synchronise) and the loop.  They alternate over `--rounds` rounds after a warm-up in which every table of
the device must equal the numpy restatement; the figures are the per-batch median and the min .. max over the rounds.

    python tools/objects_bench.py [--n 16 --h 480 --w 854 --k 16 --objects 8 --min_area 64 --blobs 12 --iters 10 --rounds 5]
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


def overlaps_host(labels, hw, dets, counts, objects, O):
    """The alternative, on host arrays: per frame a root -> rank table, a gather and two bincounts -> (row_obj [n, k, O], obj_area [n, O],
    frame_stats [n, 2]) as udet_track_object_overlaps_ragged defines them."""
    n, k = dets.shape[:2]
    row_obj, area, stats = np.zeros((n, k, O), np.int64), np.zeros((n, O), np.int64), np.zeros((n, 2), np.int64)
    rows = np.clip(counts[:, 2], 0, k).astype(int)
    pos = np.concatenate([[0], np.cumsum([H * W for H, W in hw])])
    for i, (H, W) in enumerate(hw):
        v = labels[pos[i]:pos[i + 1]].astype(np.int64)
        b = objects[pos[i]:pos[i + 1]].astype(np.int64)
        rank = np.full(H * W + 1, -1, np.int64)
        r = np.arange(rows[i])
        rank[dets[i, r, 0] + 1] = r
        hit = rank[np.where((v >= 1) & (v <= H * W), v, 0)]
        named = (b >= 1) & (b <= O)
        both = named & (hit >= 0)
        row_obj[i] = np.bincount(hit[both] * O + b[both] - 1, minlength=k * O).reshape(k, O)
        area[i] = np.bincount(b[named] - 1, minlength=O)
        stats[i] = [named.sum(), (b > O).sum()]
    return row_obj, area, stats


def banded_objects(n, h, w, O, rng):
    """n object maps: O vertical bands of the ids 1..O with background gaps between them, shifted by three columns per frame, a strip of
    the void label and a few ids above O."""
    cols = np.zeros(w, np.uint8)
    edges = np.linspace(0, w, O + 1).astype(int)
    for o in range(O):
        cols[edges[o]:edges[o + 1] - max(1, (edges[o + 1] - edges[o]) // 6)] = o + 1
    out = []
    for t in range(n):
        m = np.tile(np.roll(cols, 3 * t), (h, 1))
        m[:4] = 255
        m[rng.integers(0, h, 50), rng.integers(0, w, 50)] = O + 1
        out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("h", 480), ("w", 854), ("k", 16), ("objects", 8), ("min_area", 64), ("blobs", 12), ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from tracks_bench import moving_blobs
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_detections import component_boxes
    from unsupervised_detection_amd.native_objects import object_overlaps
    from unsupervised_detection_amd.ragged import PackedLayout
    rng = np.random.default_rng(0)
    frames = moving_blobs(a.n, a.h, a.w, a.blobs, rng)
    hw = [(a.h, a.w)] * a.n
    layout = PackedLayout.packed(hw)
    binary = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    objects = torch.from_numpy(np.concatenate([m.reshape(-1) for m in banded_objects(a.n, a.h, a.w, a.objects, rng)])).cuda()
    sel = select_components(binary, layout, mode="label", connectivity=8, want_labels=True)
    det = component_boxes(sel, min_area=a.min_area, max_detections=a.k)

    def device():
        return object_overlaps(sel, det, objects, a.objects)

    def host():
        return overlaps_host(sel.labels.cpu().numpy(), hw, det.dets.cpu().numpy(), det.counts.cpu().numpy(), objects.cpu().numpy(), a.objects)
    got, want = device().host(), host()  # warm-up of both, and every table must equal the numpy restatement before either is timed
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
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
    print(json.dumps({"shape": [a.n, a.h, a.w], "k": a.k, "objects": a.objects, "min_area": a.min_area, "iters": a.iters, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0), "rows_mean": float(det.counts.cpu().numpy()[:, 2].mean()),
                      "row_obj_nonzero": int((want[0] != 0).sum()), "object_pixels": int(want[2][:, 0].sum()), "void_pixels": int(want[2][:, 1].sum()),
                      "object_overlaps": dict(stat(t["device"]), launches=2), "object_overlaps_host": stat(t["host"]),
                      "ratio_host_over_object_overlaps": float(np.median(t["host"]) / np.median(t["device"]))}))


if __name__ == "__main__":
    main()
