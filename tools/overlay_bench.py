"""Time visualize.overlay_native (udet_overlay_native_ragged: one launch per batch) on one batch of benchmark-sized frames next to
what a user would otherwise write with torch on the device, frame by frame: `where` for the mask's colour, two products, a sum,
`round` and `clamp` for the blend, `max_pool2d` of the background for the erosion, `where` for the contour.  16 frames 480 x 854 with
a few blobs each, edge = 2.  Both paths start from the same packed device buffers, both are timed with HIP events around `--iters`
back-to-back batches, and they alternate over `--rounds` rounds after a warm-up in which their results must be equal byte for byte; the
figures are the per-batch median and the min .. max over the rounds.  --notes FILE appends them as a markdown paragraph (the form they
have in profiles/NOTES.md).

    python tools/overlay_bench.py [--n 16 --h 480 --w 854 --edge 2 --iters 200 --rounds 5] [--notes profiles/NOTES.md]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def blob_masks(n, h, w, rng):
    y, x = np.mgrid[:h, :w].astype(np.float32)
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        for _ in range(4):
            cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(20, h / 3), rng.uniform(20, w / 3)
            out[i][((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 1
    return out


def overlay_torch(frame, mask, alpha, beta, colour, edge, edge_colour):
    """One frame [H,W,3] uint8 and its mask [H,W] uint8 on the device -> [H,W,3] uint8, the definition of udet_overlay_native_ragged:
    every product and the sum are float32 operations of their own, round is half to even."""
    fg = mask != 0
    m = torch.where(fg[..., None], colour, torch.zeros_like(colour))
    out = torch.round(frame.to(torch.float32) * alpha + m * beta).clamp_(0.0, 255.0).to(torch.uint8)
    if edge >= 1:  # a background pixel of the frame within the window: max_pool2d pads with -inf, never background
        near = torch.nn.functional.max_pool2d((~fg).to(torch.float32)[None, None], 2 * edge + 1, 1, edge)[0, 0] > 0
        out = torch.where((fg & near)[..., None], edge_colour, out)
    return out


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("h", 480), ("w", 854), ("edge", 2), ("iters", 200), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--notes", default="", help="append the figures to this markdown file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.rounds >= 5, "at least five rounds"
    from unsupervised_detection_amd.ragged import PackedLayout, PackedSamples
    from unsupervised_detection_amd.visualize import OVERLAY_DEFAULTS, overlay_native
    rng = np.random.default_rng(0)
    layout = PackedLayout.packed([(a.h, a.w)] * a.n)
    frames = PackedSamples(PackedLayout.packed([(a.h, a.w)] * a.n, 3), torch.device("cuda", 0))
    frames.data = torch.from_numpy(rng.integers(0, 256, 3 * layout.numel, dtype=np.uint8)).cuda()
    masks = PackedSamples(layout, frames.device)
    masks.binary = torch.from_numpy(blob_masks(a.n, a.h, a.w, rng).reshape(-1)).cuda()
    p = dict(OVERLAY_DEFAULTS, edge=a.edge)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=frames.device)
    alpha, beta, colour = f32(p["alpha"]), f32(p["beta"]), f32(p["colour"])
    edge_colour = torch.tensor(p["edge_colour"], dtype=torch.uint8, device=frames.device)
    out = torch.zeros_like(frames.data)

    def device():
        return overlay_native(frames, masks, out=out, **p)

    def composed():
        return [overlay_torch(frames.layout.view(frames.data, i), layout.view(masks.binary, i), alpha, beta, colour, a.edge, edge_colour)
                for i in range(a.n)]
    got, want = device(), composed()  # warm-up of both, and the two must agree before either is timed
    for i in range(a.n):
        assert torch.equal(got.sample(i), want[i]), i
    contour = float(np.mean([(w == edge_colour).all(-1).float().mean().item() for w in want]))
    torch.cuda.synchronize()
    td, tt = [], []
    for _ in range(a.rounds):
        for fn, times in ((device, td), (composed, tt)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.iters)
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    nbytes = 7 * layout.numel  # frame in, mask in, picture out
    res = {"shape": [a.n, a.h, a.w], "edge": a.edge, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "foreground": float(masks.binary.float().mean()), "contour": contour, "one_call": stat(td), "torch_per_frame": stat(tt),
           "ratio_torch_over_one_call": float(np.median(tt) / np.median(td)), "one_call_gb_per_s": nbytes / np.median(td) / 1e6}
    print(json.dumps(res))
    if a.notes:
        with open(a.notes, "a") as f:
            f.write("\n`tools/overlay_bench.py` on {device}: {n} frames {h} x {w}, edge {edge}, foreground {fg:.2f}, {iters} batches per round, "
                    "{rounds} rounds, HIP events, the two paths alternating after a warm-up in which their pictures were equal byte for "
                    "byte.  One call of `udet_overlay_native_ragged` through `visualize.overlay_native`: median {d[median_ms]:.4f} ms per batch "
                    "({d[min_ms]:.4f} .. {d[max_ms]:.4f}), {bw:.0f} GB/s over the 7 bytes per pixel it must move.  The per-frame composition "
                    "in torch (`where`, two products, a sum, `round`, `clamp`, `max_pool2d`, `where`): median {t[median_ms]:.4f} ms per batch "
                    "({t[min_ms]:.4f} .. {t[max_ms]:.4f}).  Ratio of the medians {r:.1f}.  Recorded, not gated.\n".format(
                        device=res["device"], n=a.n, h=a.h, w=a.w, edge=a.edge, fg=res["foreground"], iters=a.iters, rounds=a.rounds,
                        d=res["one_call"], t=res["torch_per_frame"], bw=res["one_call_gb_per_s"], r=res["ratio_torch_over_one_call"]))


if __name__ == "__main__":
    main()
