"""Time native_results.select_components (udet_select_components_ragged: five launches per batch) on one batch of benchmark-sized
masks next to the only alternative there was before it: .cpu() of the packed buffer, scipy.ndimage.label per frame and the same rule in
numpy.  16 masks 192 x 384 are restored to 480 x 854 (native_results.restore_masks) from two kinds of soft mask -- "random" (uniform
noise: thousands of small components per frame) and "blobs" (a few smooth blobs over weak noise: what a generator's output looks like)
-- and the selection is timed for both modes and both connectivities.  The device path goes through its Python wrapper, as a user
calls it, and is timed with HIP events around `--iters` back-to-back calls; the host path is timed with a host clock around the copy
(which synchronises) and the loop.  The two alternate over `--rounds` rounds after a warm-up in which their results must agree; the
figures are the per-batch median and the min .. max over the rounds.

    python tools/components_bench.py [--n 16 --mh 192 --mw 384 --h 480 --w 854 --iters 10 --rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

LAUNCHES = 5  # csrc/components.hip: tile, border, flatten, partial, select


def soft_masks(kind, n, mh, mw, rng):
    if kind == "random":
        return rng.random((n, mh, mw), dtype=np.float32)
    y, x = np.mgrid[:mh, :mw].astype(np.float32)
    out = 0.3 * rng.random((n, mh, mw), dtype=np.float32)
    for i in range(n):
        for _ in range(5):
            cy, cx, s = rng.uniform(0, mh), rng.uniform(0, mw), rng.uniform(6, 30)
            out[i] += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s)).astype(np.float32)
    return out


def select_host(binary, gt, hw, mode, conn):
    """The alternative: scipy.ndimage.label per frame and the rule in numpy -> (selected [n] arrays, info [n,4])."""
    from scipy import ndimage
    st = np.ones((3, 3), int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    sel, info, pos = [], [], 0
    for H, W in hw:
        b, g = binary[pos:pos + H * W].reshape(H, W), gt[pos:pos + H * W].reshape(H, W) != 0
        pos += H * W
        lab, k = ndimage.label(b, structure=st)
        if k == 0:
            sel.append(np.zeros((H, W), np.uint8))
            info.append([0, -1, 0, 0])
            continue
        flat = lab.ravel()
        area = np.bincount(flat, minlength=k + 1)[1:].astype(np.int64)
        inter = np.bincount(flat[g.ravel()], minlength=k + 1)[1:].astype(np.int64)
        if mode == "best_gt":  # IoU as exact integers: rank by cross-multiplication against the running best
            union = area + int(g.sum()) - inter
            best = 0
            for c in range(1, k):
                l, r = int(inter[c]) * int(union[best]), int(inter[best]) * int(union[c])
                if l > r or (l == r and area[c] > area[best]):
                    best = c
        else:
            best = int(np.argmax(area))  # the first of equal areas: scipy numbers components by their first pixel
        idx = np.flatnonzero(flat == best + 1)
        sel.append((lab == best + 1).astype(np.uint8))
        info.append([k, int(idx[0]), int(area[best]), int(inter[best])])
    return sel, np.array(info, np.int64)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("mh", 192), ("mw", 384), ("h", 480), ("w", 854), ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_restore import restore_masks
    from unsupervised_detection_amd.native_results import GtBatch
    rng = np.random.default_rng(0)
    sizes = [(a.h, a.w)] * a.n
    gtm = np.zeros((a.n, a.h, a.w), np.uint8)
    gtm[:, a.h // 4:3 * a.h // 4, a.w // 4:3 * a.w // 4] = 1
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    res = {"shape": [a.n, a.mh, a.mw, a.h, a.w], "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "launches": LAUNCHES, "cases": []}
    for kind in ("random", "blobs"):
        restored = restore_masks(torch.from_numpy(soft_masks(kind, a.n, a.mh, a.mw, rng)).cuda(), sizes, 0.9, 0.5)
        gt = GtBatch(torch.from_numpy(gtm.reshape(-1)).cuda(), restored.offsets, restored.hw)
        for mode in ("largest", "best_gt"):
            for conn in (4, 8):
                def device():
                    return select_components(restored, gt=gt, mode=mode, connectivity=conn)

                def host():
                    return select_host(restored.binary.cpu().numpy(), gt.data.cpu().numpy(), sizes, mode, conn)
                got, (sel, info) = device(), host()  # warm-up of both, and the two must agree before either is timed
                assert got.info.cpu().numpy().tolist() == info.tolist(), (kind, mode, conn)
                for i in range(a.n):
                    assert np.array_equal(got.binary_sample(i).cpu().numpy(), sel[i]), (kind, mode, conn, i)
                torch.cuda.synchronize()
                td, th = [], []
                for _ in range(a.rounds):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        device()
                    e1.record()
                    torch.cuda.synchronize()
                    td.append(e0.elapsed_time(e1) / a.iters)
                    t0 = time.perf_counter()
                    host()
                    th.append((time.perf_counter() - t0) * 1e3)
                res["cases"].append({"masks": kind, "mode": mode, "connectivity": conn, "components_mean": float(info[:, 0].mean()),
                                     "foreground": float(restored.binary.float().mean()), "device": stat(td), "host": stat(th),
                                     "ratio_host_over_device": float(np.median(th) / np.median(td))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
