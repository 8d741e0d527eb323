"""Time native_results.component_boxes (udet_component_boxes_ragged: four launches per batch), alone on labels that are already on the
device and together with the labelling call that writes them (select_components in mode "label": five launches), next to the only
alternative there was before it: .cpu() of the packed binary masks and scores, scipy.ndimage.label / find_objects per frame and the
ranking in numpy.  16 masks 192 x 384 are restored to 480 x 854 (native_results.restore_masks) from two kinds of soft mask -- "random"
(uniform noise: thousands of small components per frame) and "blobs" (a few smooth blobs over weak noise: what a generator's output
looks like) -- for both connectivities, min_area 64 and k = 16.  The device paths go through their Python wrappers, as a user calls
them, and are timed with HIP events around `--iters` back-to-back calls; the host path is timed with a host clock around the copies
(which synchronise) and the loop.  They alternate over `--rounds` rounds after a warm-up in which their results must agree; the
figures are the per-batch median and the min .. max over the rounds.

    python tools/detections_bench.py [--n 16 --mh 192 --mw 384 --h 480 --w 854 --k 16 --min_area 64 --iters 10 --rounds 5]
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

LAUNCHES = 4  # csrc/detections.hip: init, area + kept roots, rank, box / sums


def boxes_host(binary, score, hw, conn, min_area, k):
    """The alternative: scipy.ndimage.label / find_objects per frame, sums by np.bincount (float64 weights: exact below 2^53), the
    ranking by np.lexsort -> (dets [n, k, 9], counts [n, 3])."""
    from scipy import ndimage
    st = np.ones((3, 3), int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    dets = np.zeros((len(hw), k, 9), np.int64)
    dets[:, :, 0] = -1
    counts = np.zeros((len(hw), 3), np.int64)
    pos = 0
    for i, (H, W) in enumerate(hw):
        b, s = binary[pos:pos + H * W].reshape(H, W), score[pos:pos + H * W]
        pos += H * W
        lab, nc = ndimage.label(b, structure=st)
        if nc == 0:
            continue
        flat = lab.ravel()
        area = np.bincount(flat, minlength=nc + 1)[1:]
        keep = np.flatnonzero(area >= min_area)
        fg = np.flatnonzero(flat)
        first = np.full(nc + 1, H * W, np.int64)
        np.minimum.at(first, flat[fg][::-1], fg[::-1])  # the root: the smallest index of each component
        order = keep[np.lexsort((first[1:][keep], -area[keep]))][:k]
        yy, xx = np.divmod(np.arange(H * W), W)
        sums = [np.bincount(flat, weights=v, minlength=nc + 1)[1:] for v in (yy, xx, s)]
        objs = ndimage.find_objects(lab)
        for r, c in enumerate(order):
            sl = objs[c]
            dets[i, r] = [first[c + 1], area[c], sl[0].start, sl[1].start, sl[0].stop, sl[1].stop] + [int(v[c]) for v in sums]
        counts[i] = [nc, len(keep), len(order)]
    return dets, counts


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("mh", 192), ("mw", 384), ("h", 480), ("w", 854), ("k", 16), ("min_area", 64), ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from components_bench import soft_masks
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_detections import component_boxes
    from unsupervised_detection_amd.native_restore import restore_masks
    rng = np.random.default_rng(0)
    sizes = [(a.h, a.w)] * a.n
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    res = {"shape": [a.n, a.mh, a.mw, a.h, a.w], "k": a.k, "min_area": a.min_area, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "cases": []}
    for kind in ("random", "blobs"):
        restored = restore_masks(torch.from_numpy(soft_masks(kind, a.n, a.mh, a.mw, rng)).cuda(), sizes, 0.9, 0.5)
        for conn in (4, 8):
            sel = select_components(restored, mode="label", connectivity=conn, want_labels=True)

            def boxes():
                return component_boxes(sel, score=restored, min_area=a.min_area, max_detections=a.k)

            def label_and_boxes():
                s = select_components(restored, mode="label", connectivity=conn, want_labels=True)
                return component_boxes(s, score=restored, min_area=a.min_area, max_detections=a.k)

            def host():
                return boxes_host(restored.binary.cpu().numpy(), restored.data.cpu().numpy(), sizes, conn, a.min_area, a.k)
            got, both, (dets, counts) = boxes(), label_and_boxes(), host()  # warm-up of all, and they must agree before any is timed
            for g in (got, both):
                assert np.array_equal(g.dets.cpu().numpy(), dets) and np.array_equal(g.counts.cpu().numpy(), counts), (kind, conn)
            torch.cuda.synchronize()
            t = {"boxes": [], "label_and_boxes": [], "host": []}
            for _ in range(a.rounds):
                for name, fn in (("boxes", boxes), ("label_and_boxes", label_and_boxes)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    t[name].append(e0.elapsed_time(e1) / a.iters)
                t0 = time.perf_counter()
                host()
                t["host"].append((time.perf_counter() - t0) * 1e3)
            res["cases"].append({"masks": kind, "connectivity": conn, "components_mean": float(counts[:, 0].mean()),
                                 "kept_mean": float(counts[:, 1].mean()), "written_mean": float(counts[:, 2].mean()),
                                 "boxes": stat(t["boxes"]), "label_and_boxes": stat(t["label_and_boxes"]), "host": stat(t["host"]),
                                 "ratio_host_over_label_and_boxes": float(np.median(t["host"]) / np.median(t["label_and_boxes"]))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
