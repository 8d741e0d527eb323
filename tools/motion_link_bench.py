"""Time the motion-compensated link on labels and detections that are already on the device: flow_displacements
(udet_flow_displacements_ragged, one launch), link_detections with and without `disp` on the same labels (four launches each), and the
only alternative there was before them: .cpu() of the labels, dets, counts and the flow, and numpy for the displacements and the link.
16 consecutive frames of 480 x 854 hold square blobs that move further than their own extent per frame; the flow is synthetic, at 384 x
640: minus each blob's step (in grid pixels) over the blob's box grown by `--pad` grid cells, zero elsewhere.  The frames are labelled and
boxed (k = 16) once, outside the timing.  Before anything is timed the device's displacements and every output of the motion link must
equal the numpy restatements of tests/test_motion_link.py.  The device calls go through their Python wrappers, as a user calls them, and
are timed with HIP events around `--iters` back-to-back calls; the host path with a host clock around the copies (which synchronise) and
the arithmetic.  They alternate over `--rounds` rounds; the figures are the per-batch median and the min .. max over the rounds.  The
comparison that matters is the motion link against the co-located link of the same build on the same labels.

    python tools/motion_link_bench.py [--n 16 --h 480 --w 854 --fh 384 --fw 640 --k 16 --blobs 8 --side 24 --pad 3 --iters 10 --rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]


def fast_blobs(n, h, w, fh, fw, blobs, side, pad, rng):
    """n binary frames [h, w] of `blobs` side x side squares, each moving by a constant step of more than `side` pixels per frame on its
    own lane (so that no two ever touch), and the backward flow [n, fh, fw, 2] of every frame in grid pixels."""
    frames, flow = np.zeros((n, h, w), np.uint8), np.zeros((n, fh, fw, 2), np.float32)
    lane = h // blobs
    assert lane >= side + 8, "too many blobs for the frame's height"
    for b in range(blobs):
        sx = int(rng.integers(side + 2, 2 * side)) * (1 if b % 2 == 0 else -1)
        sy = int(rng.integers(-3, 4))
        x0 = 4 if sx > 0 else w - side - 4
        y0 = b * lane + (lane - side) // 2
        for t in range(n):
            x, y = x0 + t * sx, min(max(y0 + t * sy, b * lane + 4), (b + 1) * lane - side - 4)
            if x < 0 or x + side > w:
                break
            frames[t, y:y + side, x:x + side] = 1
            if t:
                py = min(max(y0 + (t - 1) * sy, b * lane + 4), (b + 1) * lane - side - 4)
                gy0, gy1 = int(y * fh / h) - pad, int((y + side) * fh / h) + pad + 1
                gx0, gx1 = int(x * fw / w) - pad, int((x + side) * fw / w) + pad + 1
                flow[t, max(gy0, 0):gy1, max(gx0, 0):gx1] = (-sx * fw / w, (py - y) * fh / h)
    return list(frames), flow


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("h", 480), ("w", 854), ("fh", 384), ("fw", 640), ("k", 16), ("blobs", 8), ("side", 24), ("pad", 3),
                          ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from test_motion_link import displacements_np, links_motion_np
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_detections import component_boxes
    from unsupervised_detection_amd.native_motion import flow_displacements
    from unsupervised_detection_amd.native_tracks import link_detections
    from unsupervised_detection_amd.ragged import PackedLayout
    frames, flow = fast_blobs(a.n, a.h, a.w, a.fh, a.fw, a.blobs, a.side, a.pad, np.random.default_rng(0))
    hw = [(a.h, a.w)] * a.n
    layout = PackedLayout.packed(hw)
    binary = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    d_flow = torch.from_numpy(flow).cuda()
    sel = select_components(binary, layout, mode="label", connectivity=8, want_labels=True)
    det = component_boxes(sel, min_area=a.side, max_detections=a.k)
    link = [0] + [1] * (a.n - 1)

    def host():
        labels = sel.labels.cpu().numpy().reshape(a.n, a.h, a.w)
        dets, counts, f = det.dets.cpu().numpy(), det.counts.cpu().numpy(), d_flow.cpu().numpy()
        disps = [displacements_np(f[i], a.h, a.w) for i in range(a.n)]
        return disps, links_motion_np(list(labels), dets, counts, link, 100, disps)
    disp = flow_displacements(d_flow, layout)
    moved, plain = link_detections(sel, det, link=link, disp=disp), link_detections(sel, det, link=link)
    disps, want = host()  # device and restatement must be equal in every entry before either is timed
    assert np.array_equal(disp.cpu().numpy(), np.concatenate([d.reshape(-1) for d in disps]))
    for g, f in zip(moved.host(), ("inter", "match", "ids", "linked", "seq_tracks")):
        assert np.array_equal(g, getattr(want, f)), f
    assert int(moved.next_id.cpu()[0]) == want.next_id
    calls = {"flow_displacements": lambda: flow_displacements(d_flow, layout), "link_motion": lambda: link_detections(sel, det, link=link, disp=disp),
             "link_co_located": lambda: link_detections(sel, det, link=link)}
    t = {name: [] for name in list(calls) + ["host"]}
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1) / a.iters)
        t0 = time.perf_counter()
        host()
        t["host"].append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    print(json.dumps({"shape": [a.n, a.h, a.w], "flow": [a.fh, a.fw], "k": a.k, "blobs": a.blobs, "side": a.side, "iters": a.iters, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0), "rows_mean": float(det.counts.cpu().numpy()[:, 2].mean()),
                      "tracks_co_located": int(plain.next_id.cpu()[0]), "tracks_motion": int(moved.next_id.cpu()[0]),
                      "flow_displacements": dict(stat(t["flow_displacements"]), launches=1),
                      "link_motion": dict(stat(t["link_motion"]), launches=4), "link_co_located": dict(stat(t["link_co_located"]), launches=4),
                      "host_cpu_numpy": stat(t["host"]),
                      "ratio_link_motion_over_co_located": float(np.median(t["link_motion"]) / np.median(t["link_co_located"])),
                      "ratio_host_over_device": float(np.median(t["host"]) / (np.median(t["flow_displacements"]) + np.median(t["link_motion"])))}))


if __name__ == "__main__":
    main()
