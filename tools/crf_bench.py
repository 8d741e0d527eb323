"""Time the two dense-CRF implementations on the same inputs in one process: udet_post_dense_crf (csrc/postproc.hip: one thread per
pixel, one frame per call, three launches per iteration) and udet_dense_crf_ragged (csrc/crf.hip: LDS strips, several targets per
thread, the whole batch in iters + 2 launches).  Both go through their Python wrappers, as a user calls them
(post_processing.dense_crf once per frame, post_processing.dense_crf_ragged once per batch), and are timed with HIP events around the
calls; they alternate over `--rounds` rounds after a warm-up in which their marginals must agree (below).
The frames are structured pictures (a bright ellipse on a darker ground plus noise, the soft mask a shifted copy of the ellipse): on
noise pictures the field collapses and every frame costs the same anyway, but the agreement check would be vacuous.  --skip_old: time
the new kernel alone (the first kernel at sxy = 60 on a 480 x 854 frame takes far longer than anyone would wait for).

    python tools/crf_bench.py --shape 192 384 --sxy 25 --radius 75 --iters 50 --batch 16 [--srgb 5 --compat 5 --rounds 3] [--skip_old]

Agreement.  The first kernel adds a pixel's N = (2R + 1)^2 taps one after the other in float32: a rounding error of about
sqrt(N) 2^-24 of the sum per filter pass (the new kernel adds eight taps, then columns, then strips: far less).  A message is
compat * n K n <= compat, the softmax's slope is at most 1/4, and in the worst case the error of every update is carried into the next
one, so the two may differ by up to iters * compat / 4 * sqrt(N) 2^-24: 5.6e-4 at R = 75, 50 iterations, 4.9e-6 at R = 6, 5 iterations
(the size of the tests, whose bound against the oracle is 1e-5).  The check is max(1e-5, that); the difference found is printed.

One JSON line: per-frame milliseconds (median, min .. max over the rounds), the kernel evaluations per frame (pairs inside the clipped
windows x filter passes) and evaluations per second."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def scene(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx, ry, rx = 0.5 * h, 0.45 * w, 0.3 * h, 0.25 * w
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
    base = np.where(inside, 170.0, 60.0)[..., None] + np.array([0.0, 12.0, -9.0])
    img = np.clip(base + rng.normal(0, 4.0, (h, w, 3)), 0, 255).astype(np.uint8)
    d = ((yy - cy - max(1, h // 12)) / ry) ** 2 + ((xx - cx - max(1, w // 12)) / rx) ** 2
    soft = 1.0 / (1.0 + np.exp(4.0 * (d - 1.0))) + 0.05 * rng.random((h, w))
    return img, (soft / soft.max()).astype(np.float64)


def unary_of(soft):
    U = np.clip(soft / (soft.max() + 1e-8), 1e-6, 1.0 - 1e-6)
    return np.float32(-np.log(np.stack([1.0 - U, U], 0)))


def window_pairs(h, w, r):
    """Pairs (i, j != i) with |dy|, |dx| <= r inside an h x w frame."""
    ny = sum(min(y + r, h - 1) - max(y - r, 0) + 1 for y in range(h))
    nx = sum(min(x + r, w - 1) - max(x - r, 0) + 1 for x in range(w))
    return ny * nx - h * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=(192, 384), metavar=("H", "W"))
    ap.add_argument("--sxy", type=float, default=25.0)
    ap.add_argument("--srgb", type=float, default=5.0)
    ap.add_argument("--compat", type=float, default=5.0)
    ap.add_argument("--radius", type=int, default=0, help="0: ceil(3 sxy)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip_old", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from unsupervised_detection_amd._ffi import lib
    from unsupervised_detection_amd.post_processing import dense_crf, dense_crf_ragged
    H, W = a.shape
    R = a.radius if a.radius > 0 else int(math.ceil(3.0 * a.sxy))
    frames = [scene(H, W, 1000 + i) for i in range(a.batch)]
    imgs = [torch.from_numpy(f[0]).cuda() for f in frames]
    unaries = [torch.from_numpy(unary_of(f[1])).cuda() for f in frames]
    un_packed = torch.cat([u.view(2, -1) for u in unaries], 1).contiguous()
    im_packed = torch.cat([i.view(-1) for i in imgs]).contiguous()
    off, hw = np.arange(a.batch, dtype=np.int64) * H * W, np.array([(H, W)] * a.batch, np.int64)

    def new():
        return dense_crf_ragged(un_packed, im_packed, off, hw, a.sxy, a.srgb, a.compat, a.iters, R, want_q=True, want_labels=True)

    def old():
        return [dense_crf(u, i, a.sxy, a.srgb, a.compat, a.iters, R) for u, i in zip(unaries, imgs)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    q1, labels = new()  # warm-up of both; they must agree before either is timed
    torch.cuda.synchronize()
    res = {"shape": [H, W], "batch": a.batch, "sxy": a.sxy, "srgb": a.srgb, "compat": a.compat, "radius": R, "iters": a.iters,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "launches_new": a.iters + 2,
           "rows_per_thread": int(lib.udet_dense_crf_rows_per_thread(a.batch, H, W)),
           "launches_old_per_frame": 6 + 3 * a.iters, "foreground": float(labels.float().mean())}
    if not a.skip_old:
        qo = old()
        torch.cuda.synchronize()
        res["max_abs_diff_q1"] = max(float((q1[i * H * W:(i + 1) * H * W].view(H, W) - qo[i][1]).abs().max()) for i in range(a.batch))
        res["max_abs_diff_bound"] = max(1e-5, a.iters * a.compat / 4.0 * (2 * R + 1) * 2.0 ** -24)
        assert res["max_abs_diff_q1"] < res["max_abs_diff_bound"], (res["max_abs_diff_q1"], res["max_abs_diff_bound"])
    tn, to = [], []
    for _ in range(a.rounds):
        tn.append(timed(new))
        if not a.skip_old:
            to.append(timed(old))
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    evals = window_pairs(H, W, R) * (a.iters + 2)
    res["evaluations_per_frame"] = evals
    res["new_per_frame"] = stat(tn)
    res["new_evaluations_per_s"] = evals / (np.median(tn) * 1e-3)
    if to:
        res["old_per_frame"] = stat(to)
        res["old_evaluations_per_s"] = evals / (np.median(to) * 1e-3)
        res["ratio_old_over_new"] = float(np.median(to) / np.median(tn))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
