"""Time the per-frame and the batched sequence stage on the same inputs in one process: synthetic data of DAVIS-2016
val's shape -- 192 x 384 frames, 20 sequences of the lengths generate_soft_score_from_buffer.py:14 lists (1376 frames).

  propagation   flows given (device tensors): post_processing.propagate per sequence (one udet_post_remap x 2 + udet_post_blend x 2 chain
                per frame and direction) against ONE post_processing.propagate_sequences call; HIP events around each, so the gaps in
                which the device waits for the host's next launch count, as they do for a user.  The two must agree byte for byte.
  flows         PWCFlow per pair against PWCFlow.batch(--flow_batch) on --flow_pairs pairs (seeded random weights: the time does not
                depend on them); HIP events.
  crf           the device part of run_crf on --crf_frames frames: select_candidate + refine per frame (three host round trips, then
                udet_post_dense_crf) against post_processing._run_crf_group (one upload, udet_post_select_unary, udet_dense_crf_ragged,
                one copy back); host clock around calls that end in a device-to-host copy.
  soft_score    synthetic ensemble masks of DAVIS's shape (2 shifts x 4 crops x 2 directions per frame) on the device, --score_frames frames:
                post_processing.soft_score per frame (about a hundred launches and a host wait each) against post_processing.soft_score_batch
                on --score_batch frames per call (udet_post_soft_score_batch: four launches); host clock, both sides ending in a device
                synchronise, because the per-frame path waits on the host.  The two must agree byte for byte.

    python tools/sequence_bench.py [--rounds 3] [--flow_batch 8] [--flow_pairs 64] [--crf_batch 16] [--crf_frames 16]
                                   [--score_frames 64] [--score_batch 16] [--skip crf,flows,soft_score]

The paths alternate over --rounds rounds after a warm-up.  One JSON line: milliseconds per path (median, min .. max) and the ratios."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

DAVIS_VAL_LENGTHS = [99, 43, 100, 80, 40, 49, 50, 50, 90, 50, 52, 60, 90, 104, 40, 75, 90, 84, 80, 50]
H, W = 192, 384


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def bench_propagation(PP, lens, rounds):
    total = sum(lens)
    gen = torch.Generator(device="cuda").manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    c = torch.rand((total, 2), generator=gen, device="cuda") * 0.4 + 0.3
    masks = torch.exp(-(((yy[None] - c[:, :1, None] * H) / (0.2 * H)) ** 2 + ((xx[None] - c[:, 1:, None] * W) / (0.15 * W)) ** 2))
    masks = (masks + 0.05 * torch.rand(masks.shape, generator=gen, device="cuda")).float().contiguous()
    fp = (torch.randn((total, H, W, 2), generator=gen, device="cuda") * 3.0).contiguous()
    fn = (torch.randn((total, H, W, 2), generator=gen, device="cuda") * 3.0).contiguous()
    starts = np.concatenate([[0], np.cumsum(lens)])

    def old():
        out = []
        for s, n in zip(starts, lens):
            frames = [np.array([k]) for k in range(n)]

            def flow_fn(a, b, s=int(s)):
                ka, kb = int(a[0]), int(b[0])
                return (fp if kb == ka - 1 else fn)[s + ka]
            out.append(PP.propagate(list(masks[int(s):int(s) + n]), frames, flow_fn))
        return out

    def new():
        return PP.propagate_sequences(masks, fp, fn, lens)
    o, (nf, nb) = old(), new()
    torch.cuda.synchronize()
    for s, (f, b) in zip(starts, o):  # byte for byte
        assert torch.equal(torch.stack(f), nf[int(s):int(s) + len(f)]) and torch.equal(torch.stack(b), nb[int(s):int(s) + len(b)])
    del o
    to, tn = [], []
    for _ in range(rounds):
        tn.append(event_ms(new)[0])
        to.append(event_ms(old)[0])
    return {"frames": total, "sequences": len(lens), "per_step": stat(to), "one_call": stat(tn), "identical": True,
            "steps": 2 * (total - len(lens)), "ratio_per_step_over_one_call": float(np.median(to) / np.median(tn))}


def bench_flows(PP, pairs, batch, rounds):
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(pairs + 1)]
    flow = PP.PWCFlow()
    a, b = imgs[:-1], imgs[1:]
    dev_a, dev_b = [torch.from_numpy(x).cuda() for x in a], [torch.from_numpy(x).cuda() for x in b]

    def old():
        return [flow(x, y) for x, y in zip(dev_a, dev_b)]

    def new():
        return flow.batch(dev_a, dev_b, batch)
    o, n = old(), new()
    torch.cuda.synchronize()
    diff = max(float((n[i] - o[i]).abs().max() / o[i].abs().max()) for i in range(pairs))
    to, tn = [], []
    for _ in range(rounds):
        tn.append(event_ms(new)[0] / pairs)
        to.append(event_ms(old)[0] / pairs)
    return {"pairs": pairs, "flow_batch": batch, "per_pair": stat(to), "batched_per_pair": stat(tn), "max_rel_diff": diff,
            "ratio_per_pair_over_batched": float(np.median(to) / np.median(tn))}


def bench_crf(PP, frames_n, batch, rounds, sxy, srgb, compat, iters):
    from crf_bench import scene
    frames = []
    for i in range(frames_n):
        img, soft = scene(H, W, 1000 + i)
        soft = soft.astype(np.float32)
        frames.append((soft, np.roll(soft, 3, 1), np.roll(soft, -4, 0), (soft > 0.5).astype(np.float32), img))

    def old():
        out = []
        for pm, pf, pb, gt, img in frames:
            mask, _ = PP.select_candidate(pm, pf, pb, gt)
            out.append(PP.refine(mask, img, 0.1, sxy, srgb, compat, gt, iters))
        return out

    def new():
        return [PP._run_crf_group(frames[k:k + batch], sxy, srgb, compat, 0.1, iters, None) for k in range(0, frames_n, batch)]
    o, n = old(), new()
    labels_new = np.concatenate([g[1] for g in n])
    differ = [int((labels_new[i] != o[i][0]).sum()) for i in range(frames_n)]
    to, tn = [], []
    for _ in range(rounds):
        tn.append(host_ms(new)[0] / frames_n)
        to.append(host_ms(old)[0] / frames_n)
    return {"frames": frames_n, "crf_batch": batch, "sxy": sxy, "srgb": srgb, "compat": compat, "iters": iters, "per_frame": stat(to),
            "batched_per_frame": stat(tn), "labels_differing_pixels_max": max(differ), "foreground": float(labels_new.mean()),
            "ratio_per_frame_over_batched": float(np.median(to) / np.median(tn))}


def bench_soft_score(PP, frames_n, batch, rounds):
    ns, crops = 2, (85, 90, 95, 100)
    gen = torch.Generator(device="cuda").manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    c = torch.rand((frames_n * 2 * ns * len(crops), 2), generator=gen, device="cuda") * 0.2 + 0.4
    m = torch.exp(-(((yy[None] - c[:, :1, None] * H) / (0.2 * H)) ** 2 + ((xx[None] - c[:, 1:, None] * W) / (0.15 * W)) ** 2))
    m = m + 0.05 * torch.rand(m.shape, generator=gen, device="cuda")
    preds = (m / m.amax((1, 2), keepdim=True)).float().view(frames_n, 2, ns, len(crops), H, W).contiguous()
    preds[1::7, 0, 0, 2] = 1.0  # a mask that fails the sanity rule now and then: its slot takes the partner
    preds[3::11, :, 1, 1] = 1.0  # ... and a pair that fails together
    per_frame_args = [([list(r) for r in preds[i, 0]], [list(r) for r in preds[i, 1]]) for i in range(frames_n)]

    def old():
        return [PP.soft_score(pb, pf, crops, 90.0, (H, W)) for pb, pf in per_frame_args]

    def new():
        return [PP.soft_score_batch(preds[k:k + batch], crops, 90.0) for k in range(0, frames_n, batch)]
    o, n = old(), new()
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(o), torch.cat(n))  # byte for byte
    del o, n
    to, tn = [], []
    for _ in range(rounds):
        tn.append(host_ms(new)[0] / frames_n)
        to.append(host_ms(old)[0] / frames_n)
    davis = sum(DAVIS_VAL_LENGTHS)
    return {"frames": frames_n, "score_batch": batch, "ensemble": [2, ns, len(crops)], "per_frame": stat(to), "batched_per_frame": stat(tn),
            "identical": True, "batched_median_below_per_frame_min": bool(np.median(tn) < min(to)),
            "ratio_per_frame_over_batched": float(np.median(to) / np.median(tn)),
            "davis_val_frames": davis, "davis_val_per_frame_s": float(np.median(to) * davis / 1e3),
            "davis_val_batched_s": float(np.median(tn) * davis / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--flow_batch", type=int, default=8)
    ap.add_argument("--flow_pairs", type=int, default=64)
    ap.add_argument("--crf_batch", type=int, default=16)
    ap.add_argument("--crf_frames", type=int, default=16)
    ap.add_argument("--score_frames", type=int, default=64)
    ap.add_argument("--score_batch", type=int, default=16)
    ap.add_argument("--sxy", type=float, default=25.0)
    ap.add_argument("--srgb", type=float, default=5.0)
    ap.add_argument("--compat", type=float, default=5.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sequences", type=int, default=len(DAVIS_VAL_LENGTHS), help="the first so many of DAVIS val's 20 lengths")
    ap.add_argument("--skip", default="", help="comma-separated: propagation, flows, crf, soft_score")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from unsupervised_detection_amd import post_processing as PP
    skip = set(filter(None, a.skip.split(",")))
    res = {"shape": [H, W], "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    if "propagation" not in skip:
        res["propagation"] = bench_propagation(PP, DAVIS_VAL_LENGTHS[:a.sequences], a.rounds)
    if "flows" not in skip:
        res["flows"] = bench_flows(PP, a.flow_pairs, a.flow_batch, a.rounds)
    if "crf" not in skip:
        res["crf"] = bench_crf(PP, a.crf_frames, a.crf_batch, a.rounds, a.sxy, a.srgb, a.compat, a.iters)
    if "soft_score" not in skip:
        res["soft_score"] = bench_soft_score(PP, a.score_frames, a.score_batch, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
