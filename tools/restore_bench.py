"""Time native_results.restore_masks (udet_restore_masks_ragged: at most three launches per batch) on one batch of benchmark-sized
masks next to the per-frame composition the soft-score stage already had (post_processing._imresize_window + udet_post_place: four
launches per frame, two of them on a single workgroup).  Both go through their Python wrappers, as a user calls them.  Device time:
HIP events around `--iters` back-to-back batches, the two paths alternating over `--rounds` rounds after a warm-up; the figures are
the per-batch median and the min .. max over the rounds (the run-to-run spread on this box).

    python tools/restore_bench.py [--n 16 --mh 192 --mw 384 --h 480 --w 854 --crop 0.9 --iters 20 --rounds 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("mh", 192), ("mw", 384), ("h", 480), ("w", 854), ("iters", 20), ("rounds", 7)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--crop", type=float, default=0.9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from unsupervised_detection_amd.native_restore import restore_box, restore_masks
    from unsupervised_detection_amd.post_processing import _imresize_window, _stream, check, lib
    rng = np.random.default_rng(0)
    masks = torch.from_numpy(rng.random((a.n, a.mh, a.mw), dtype=np.float32)).cuda()
    sizes = [(a.h, a.w)] * a.n
    y0, x0, h, w = restore_box(a.h, a.w, a.crop)

    def batched():
        return restore_masks(masks, sizes, a.crop, 0.5)

    def per_frame():
        out = []
        for i in range(a.n):
            patch = _imresize_window(masks[i].double(), 0, 0, a.mh, a.mw, h, w)
            canvas = torch.empty((a.h, a.w), dtype=torch.float64, device="cuda")
            check(lib.udet_post_place(patch.data_ptr(), h, w, y0, x0, a.h, a.w, canvas.data_ptr(), _stream()))
            out.append((patch, canvas))
        return out
    got, want = batched(), per_frame()  # warm-up of both paths, and the two must agree before either is timed
    for i in range(a.n):
        assert torch.equal(got.sample(i)[y0:y0 + h, x0:x0 + w], want[i][0]), "the two paths differ at sample {}".format(i)
    for _ in range(3):
        batched(), per_frame()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    tb, tp = [], []
    for _ in range(a.rounds):
        tb.append(timed(batched))
        tp.append(timed(per_frame))
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    res = {"shape": [a.n, a.mh, a.mw, a.h, a.w], "box": [y0, x0, h, w], "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "batched": stat(tb), "per_frame": stat(tp),
           "ratio_per_frame_over_batched": float(np.median(tp) / np.median(tb))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
