"""Time native_results.instance_maps (udet_track_instance_maps_ragged: two launches per batch) and visualize.overlay_instances
(udet_overlay_instances_ragged: one launch) on labels, detections and track ids that are already on the device, next to the only
alternative there was before them: .cpu() of the packed labels, dets, counts, ids and annotations and numpy over every frame for the maps,
row_gt and frame_stats; .cpu() of the frames and the maps and numpy / scipy (two windowed filters per frame) for the picture.  16
consecutive frames of 480 x 854 hold the moving blobs of tools/tracks_bench.py; they are labelled, boxed (k = 16, min_area 64) and
linked once, outside the timing; the annotation is the first frame's mask shifted along.  The device paths go through their Python
wrappers, as a user calls them, and are timed with HIP events around `--iters` back-to-back calls; the host paths with a host clock around
the copies (which synchronise) and the loops.  They alternate over `--rounds` rounds after a warm-up in which device and host must be
equal in every byte; the figures are the per-batch median and the min .. max over the rounds.

    python tools/instances_bench.py [--n 16 --h 480 --w 854 --k 16 --min_area 64 --blobs 12 --edge 2 --iters 10 --rounds 5]
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

WRAP, OTHER = 252, 255


def maps_host(labels, hw, dets, counts, ids, gt):
    """The alternative for the maps, on host arrays: per frame a root -> value table and a root -> rank table, two gathers and a bincount
    -> (maps [total] uint8, row_gt [n, k], frame_stats [n, 3]) as udet_track_instance_maps_ragged defines them."""
    n, k = ids.shape
    out, row_gt, stats = np.zeros(len(labels), np.uint8), np.zeros((n, k), np.int64), np.zeros((n, 3), np.int64)
    rows = np.clip(counts[:, 2], 0, k).astype(int)
    pos = np.concatenate([[0], np.cumsum([H * W for H, W in hw])])
    for i, (H, W) in enumerate(hw):
        v = labels[pos[i]:pos[i + 1]].astype(np.int64)
        g = gt[pos[i]:pos[i + 1]] != 0
        value, rank = np.full(H * W + 1, OTHER, np.uint8), np.full(H * W + 1, -1, np.int64)
        value[0] = 0
        r = np.arange(rows[i])
        rank[dets[i, r, 0] + 1] = r
        has = ids[i, r] >= 0
        value[dets[i, r[has], 0] + 1] = 1 + ids[i, r[has]] % WRAP
        at = np.where((v >= 1) & (v <= H * W), v, 0)
        m = value[at]
        out[pos[i]:pos[i + 1]] = m
        hit = rank[at]
        row_gt[i] = np.bincount(hit[(hit >= 0) & g], minlength=k)
        stats[i] = [((m >= 1) & (m <= WRAP)).sum(), (m == OTHER).sum(), g.sum()]
    return out, row_gt, stats


def overlay_host(frames, maps, hw, lut, alpha, beta, edge):
    """The alternative for the picture, on host arrays: the float32 blend with the pixel's own colour, the contour from scipy's windowed
    minimum and maximum -> the packed rgb bytes as udet_overlay_instances_ragged defines them."""
    from scipy.ndimage import maximum_filter, minimum_filter
    out = np.empty_like(frames)
    pos = np.concatenate([[0], np.cumsum([H * W for H, W in hw])])
    for i, (H, W) in enumerate(hw):
        m = maps[pos[i]:pos[i + 1]].reshape(H, W)
        img = frames[3 * pos[i]:3 * pos[i + 1]].reshape(H, W, 3)
        own = lut[m]
        pic = np.clip(np.rint(img.astype(np.float32) * np.float32(alpha) + own.astype(np.float32) * np.float32(beta)), 0, 255).astype(np.uint8)
        if edge >= 1:
            c = (m != 0) & ((minimum_filter(m, 2 * edge + 1, mode="nearest") != m) | (maximum_filter(m, 2 * edge + 1, mode="nearest") != m))
            pic[c] = own[c]
        out[3 * pos[i]:3 * pos[i + 1]] = pic.reshape(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("n", 16), ("h", 480), ("w", 854), ("k", 16), ("min_area", 64), ("blobs", 12), ("edge", 2), ("iters", 10), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from tracks_bench import moving_blobs
    from unsupervised_detection_amd.native_components import select_components
    from unsupervised_detection_amd.native_detections import component_boxes
    from unsupervised_detection_amd.native_instances import instance_maps
    from unsupervised_detection_amd.native_tracks import link_detections
    from unsupervised_detection_amd.ragged import PackedLayout
    from unsupervised_detection_amd.visualize import TRACK_PALETTE, NativeOverlays, overlay_instances
    rng = np.random.default_rng(0)
    frames = moving_blobs(a.n, a.h, a.w, a.blobs, rng)
    hw = [(a.h, a.w)] * a.n
    layout = PackedLayout.packed(hw)
    binary = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    gt = torch.from_numpy(np.concatenate([np.roll(frames[0], (2 * t, 3 * t), (0, 1)).reshape(-1) for t in range(a.n)])).cuda()
    sel = select_components(binary, layout, mode="label", connectivity=8, want_labels=True)
    det = component_boxes(sel, min_area=a.min_area, max_detections=a.k)
    trk = link_detections(sel, det, link=[0] + [1] * (a.n - 1))
    rgb = NativeOverlays(torch.from_numpy(rng.integers(0, 256, 3 * layout.numel, dtype=np.uint8)).cuda(), PackedLayout(3 * layout.offsets, hw, 3 * layout.numel, 3))
    canvas = torch.zeros(3 * layout.numel, dtype=torch.uint8, device="cuda")
    lut = np.zeros((256, 3), np.uint8)
    lut[1:WRAP + 1] = [TRACK_PALETTE[j % len(TRACK_PALETTE)] for j in range(WRAP)]
    lut[WRAP + 1:] = (128, 128, 128)

    def device_maps():
        return instance_maps(sel, det, trk, gt=gt)

    def host_maps():
        return maps_host(sel.labels.cpu().numpy(), hw, det.dets.cpu().numpy(), det.counts.cpu().numpy(), trk.ids.cpu().numpy(), gt.cpu().numpy())
    inst = device_maps()

    def device_overlay():
        return overlay_instances(rgb, inst, edge=a.edge, out=canvas)

    def host_overlay():
        return overlay_host(rgb.data.cpu().numpy(), inst.map.cpu().numpy(), hw, lut, 0.5, 0.4, a.edge)
    want = host_maps()  # warm-up of all four, and device and host must be equal in every byte before either is timed
    assert np.array_equal(inst.map.cpu().numpy(), want[0]) and np.array_equal(inst.host()[0], want[1]) and np.array_equal(inst.host()[1], want[2])
    assert np.array_equal(device_overlay().data.cpu().numpy(), host_overlay())
    torch.cuda.synchronize()
    t = {"maps": [], "maps_host": [], "overlay": [], "overlay_host": []}
    for _ in range(a.rounds):
        for name, dev, host in (("maps", device_maps, host_maps), ("overlay", device_overlay, host_overlay)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                dev()
            e1.record()
            torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1) / a.iters)
            t0 = time.perf_counter()
            host()
            t[name + "_host"].append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
    stats = inst.host()[1]
    print(json.dumps({"shape": [a.n, a.h, a.w], "k": a.k, "min_area": a.min_area, "edge": a.edge, "iters": a.iters, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0), "rows_mean": float(det.counts.cpu().numpy()[:, 2].mean()),
                      "tracks": int(trk.next_id.cpu()[0]), "assigned_pixels": int(stats[:, 0].sum()), "unassigned_pixels": int(stats[:, 1].sum()),
                      "row_gt_nonzero": int((want[1] != 0).sum()),
                      "instance_maps": dict(stat(t["maps"]), launches=2), "instance_maps_host": stat(t["maps_host"]),
                      "overlay_instances": dict(stat(t["overlay"]), launches=1), "overlay_instances_host": stat(t["overlay_host"]),
                      "ratio_host_over_instance_maps": float(np.median(t["maps_host"]) / np.median(t["maps"])),
                      "ratio_host_over_overlay_instances": float(np.median(t["overlay_host"]) / np.median(t["overlay"]))}))


if __name__ == "__main__":
    main()
