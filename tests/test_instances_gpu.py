"""GPU: udet_track_instance_maps_ragged and udet_overlay_instances_ragged (csrc/instances.hip) through native_results.instance_maps and
visualize.overlay_instances -- map, row_gt and frame_stats against the numpy restatement of tests/test_instances.py, the pictures
against its numpy / scipy restatement.  Everything is integers and bytes: every comparison is exact equality.  The labels come from the
existing labelling call, the dets from component_boxes and the ids from link_detections; the largest frame is 130 x 259."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_components import DENSITIES, _tree_files, ragged_masks
from test_instances import (MAPS_OK, MAPS_ORDER, OTHER, OVER_OK, OVER_ORDER, PALETTE, instance_maps_np, never,
                            overlay_instances_np, random_gts, sequences, stand_ins)
from test_overlay_native_gpu import Packed
from test_tracks import moving_sequence, run_tree
from test_tracks_gpu import host_labels, inputs

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 70), (67, 1), (9, 13), (33, 65), (130, 259)]
GUARD = 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def pack_like(sel, arrays, fill=0):
    """Host arrays packed like sel's labels, on the device (uint8)."""
    buf = np.full(sel.layout.numel, fill, np.uint8)
    for o, a in zip(sel.offsets, arrays):
        buf[o:o + a.size] = np.asarray(a, np.uint8).reshape(-1)
    return torch.from_numpy(buf).cuda()


def equal(got, want, where=()):
    maps, row_gt, stats = want
    for i, m in enumerate(maps):
        g = got.sample(i)
        assert g.dtype == torch.uint8 and tuple(g.shape) == m.shape and np.array_equal(g.cpu().numpy(), m), where + ("map", i)
    h_row, h_stats = got.host()
    assert h_row.dtype == np.int64 and np.array_equal(h_row, row_gt), where + ("row_gt",)
    assert h_stats.dtype == np.int64 and np.array_equal(h_stats, stats), where + ("frame_stats",)


# -------------------------------------------------------------------------------------------------------------------- maps ----
@pytest.mark.parametrize("density", DENSITIES)
def test_maps_row_gt_and_stats_equal_the_restatement(gpu, density):
    from unsupervised_detection_amd.native_results import instance_maps, link_detections
    frames, link = sequences(density)
    gts = random_gts(frames)
    seen = set()
    for conn in (4, 8):
        for k in (1, 16, 64):
            sel, det = inputs(frames, k, 2 if k == 16 else 1, conn)
            labels, (dets, counts) = host_labels(sel), det.host()
            gt = pack_like(sel, gts)
            for max_gap in (0, 3):
                trk = link_detections(sel, det, link=link, max_gap=max_gap)
                ids = trk.host()[2]
                want = instance_maps_np(labels, dets, counts, ids, gts)
                equal(instance_maps(sel, det, trk, gt=gt), want, (density, conn, k, max_gap, "gt"))
                equal(instance_maps(sel.labels, det, trk), instance_maps_np(labels, dets, counts, ids), (density, conn, k, max_gap, "no gt"))
                seen |= {int(v) for m in want[0] for v in np.unique(m)}
                assert (want[1] != 0).any()
    assert 0 in seen and OTHER in seen and len(seen) > 20


def call_maps(labels, layout, det, ids, gt, out, row_gt, stats):
    from unsupervised_detection_amd._ffi import lib
    from unsupervised_detection_amd.ragged import workspace
    d_off, d_hw = layout.device_tables(labels.device)
    ws = workspace(lib.udet_track_instance_maps_workspace_bytes(layout.numel, layout.n, det.k), 4, labels.device)
    return lib.udet_track_instance_maps_ragged(labels.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w,
                                               layout.numel, det.dets.data_ptr(), det.counts.data_ptr(), det.k, ids.data_ptr(),
                                               None if gt is None else gt.data_ptr(), out.data_ptr(), row_gt.data_ptr(), stats.data_ptr(),
                                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)


def test_guards_a_sample_alone_twice_and_a_misaligned_map(gpu):
    from unsupervised_detection_amd.native_results import instance_maps, link_detections
    frames, link = sequences(0.593)
    gts = random_gts(frames)
    sel, det = inputs(frames, 16, 2, 8)
    trk = link_detections(sel, det, link=link)
    ref = instance_maps(sel, det, trk, gt=pack_like(sel, gts))
    again = instance_maps(sel, det, trk, gt=pack_like(sel, gts))
    assert torch.equal(ref.map, again.map) and torch.equal(ref.row_gt, again.row_gt) and torch.equal(ref.frame_stats, again.frame_stats)
    want = instance_maps_np(host_labels(sel), *det.host(), trk.host()[2], gts)
    equal(ref, want)
    # odd offsets and guard bytes before, between and after the samples: none of them is written, whatever the map's own alignment
    g, gdet = inputs(frames, 16, 2, 8, gap=37)
    assert torch.equal(gdet.dets, det.dets) and len({int(o) % 4 for o in g.offsets}) >= 3
    gt = pack_like(g, gts, GUARD)
    total = g.layout.numel
    for shift in (0, 1, 2, 3):
        buf = torch.full((total + 8,), GUARD, dtype=torch.uint8, device="cuda")
        out = buf[shift:shift + total]
        row_gt, stats = torch.full((len(frames), 16), -7, dtype=torch.int64, device="cuda"), torch.full((len(frames), 3), -7, dtype=torch.int64, device="cuda")
        assert call_maps(g.labels, g.layout, gdet, trk.ids, gt, out, row_gt, stats) == 0
        host = buf.cpu().numpy()
        written = np.zeros(total + 8, bool)
        for i, (o, m) in enumerate(zip(g.offsets, want[0])):
            written[shift + o:shift + o + m.size] = True
            assert np.array_equal(host[shift + o:shift + o + m.size].reshape(m.shape), m), (shift, i)
        assert (host[~written] == GUARD).all() and (~written).sum() == 8 + 37 * (len(frames) + 1)
        assert np.array_equal(row_gt.cpu().numpy(), want[1]) and np.array_equal(stats.cpu().numpy(), want[2])
    # a sample alone equals the same sample inside the batch
    for i in (0, 4, 9, 13, len(frames) - 1):
        s1, d1 = inputs(frames[i:i + 1], 16, 2, 8)
        alone = instance_maps(s1, d1, SimpleNamespace(ids=trk.ids[i:i + 1].contiguous()), gt=pack_like(s1, gts[i:i + 1]))
        assert torch.equal(alone.sample(0), ref.sample(i)) and torch.equal(alone.row_gt[0], ref.row_gt[i]) and torch.equal(alone.frame_stats[0], ref.frame_stats[i])


def test_a_sequence_in_pieces_and_ids_set_by_hand(gpu):
    from unsupervised_detection_amd.native_results import instance_maps, link_detections
    frames = moving_sequence(ragged_masks(0.45)[3], 7, 1)
    gts = random_gts(frames, 5)
    sel, det = inputs(frames, 16, 2, 4)
    whole = instance_maps(sel, det, link_detections(sel, det), gt=pack_like(sel, gts))
    assert int(whole.map.max()) == OTHER and len(torch.unique(whole.map)) > 10
    for max_gap in (0, 2):
        ref = whole if max_gap == 0 else instance_maps(sel, det, link_detections(sel, det, max_gap=max_gap), gt=pack_like(sel, gts))
        carry, s = None, 0
        for c in (3, 3, 1):
            s1, d1 = inputs(frames[s:s + c], 16, 2, 4)
            part = link_detections(s1, d1, carry=carry, max_gap=max_gap)
            got = instance_maps(s1, d1, part, gt=pack_like(s1, gts[s:s + c]))
            for i in range(c):
                assert torch.equal(got.sample(i), ref.sample(s + i)), (max_gap, s, i)
            assert torch.equal(got.row_gt, ref.row_gt[s:s + c]) and torch.equal(got.frame_stats, ref.frame_stats[s:s + c])
            carry, s = part.tail(), s + c
    # ids set by hand: -1 and values at and past the wrap
    labels, (dets, counts) = host_labels(sel), det.host()
    ids = np.full((7, 16), -1, np.int32)
    vals = np.array([251, 252, 253, 504, -1, 0, 2 ** 31 - 1, 755, 12, -1], np.int32)
    for i in range(7):
        ids[i] = np.resize(np.roll(vals, i), 16)
    want = instance_maps_np(labels, dets, counts, ids, gts)
    equal(instance_maps(sel, det, SimpleNamespace(ids=torch.from_numpy(ids).cuda()), gt=pack_like(sel, gts)), want, ("by hand",))
    seen = {int(v) for m in want[0] for v in np.unique(m)}
    assert {252, 1, 2, OTHER, 1 + (2 ** 31 - 1) % 252} <= seen
    # labels out of range are background; garbage in dets beyond the rows and in counts changes nothing outside its sample
    lab = sel.labels.cpu().numpy().copy()
    poison = np.array([2 ** 31 - 1, -1, -2 ** 31], np.int32)
    for i, (o, (h, w)) in enumerate(zip(sel.offsets, sel.hw)):
        v = lab[o:o + h * w]
        for j, r in enumerate(np.unique(v[v > 0])[::3]):
            v[v == r] = h * w + 1 if j % 2 == 0 else poison[j % 3]
        v[np.flatnonzero(v == 0)[::5]] = poison[i % 3]
    dev = torch.from_numpy(lab).cuda()
    plabels = [sel.layout.view(dev, i).cpu().numpy() for i in range(7)]
    pwant = instance_maps_np(plabels, dets, counts, ids, gts)
    equal(instance_maps(dev, det, SimpleNamespace(ids=torch.from_numpy(ids).cuda()), gt=pack_like(sel, gts)), pwant, ("poison",))
    assert any(not np.array_equal(a, b) for a, b in zip(pwant[0], want[0]))


def test_refused_map_calls_leave_the_outputs_untouched(gpu):
    from unsupervised_detection_amd._ffi import lib
    from unsupervised_detection_amd.native_results import link_detections
    frames = moving_sequence(ragged_masks(0.45)[3], 2, 1)
    sel, det = inputs(frames, 4)
    trk = link_detections(sel, det)
    total = sel.layout.numel
    out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    row_gt, stats = torch.full((2, 4), -7, dtype=torch.int64, device="cuda"), torch.full((2, 3), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(total + 1, dtype=torch.int32, device="cuda")
    ok = dict(MAPS_OK, labels=sel.labels.data_ptr(), n=2, offsets=sel.dev_offsets.data_ptr(), hw=sel.dev_hw.data_ptr(), max_h=sel.layout.max_h,
              max_w=sel.layout.max_w, total=total, dets=det.dets.data_ptr(), counts=det.counts.data_ptr(), k=4, ids=trk.ids.data_ptr(),
              map=out.data_ptr(), row_gt=row_gt.data_ptr(), stats=stats.data_ptr(), ws=ws.data_ptr(), ws_bytes=4 * total,
              stream=torch.cuda.current_stream().cuda_stream)
    for change in (dict(labels=None), dict(ids=None), dict(map=None), dict(row_gt=None), dict(stats=None), dict(n=0), dict(k=0), dict(k=65),
                   dict(ws=None), dict(ws_bytes=4 * total - 1), dict(ws=ok["ws"] + 2), dict(row_gt=ok["row_gt"] + 4), dict(ids=ok["ids"] + 2),
                   dict(max_h=0), dict(total=0)):
        a = dict(ok, **change)
        assert lib.udet_track_instance_maps_ragged(*[a[p] for p in MAPS_ORDER]) == -5, change
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((row_gt == -7).all()) and bool((stats == -7).all())
    assert lib.udet_track_instance_maps_ragged(*[ok[p] for p in MAPS_ORDER]) == 0
    want = instance_maps_np(host_labels(sel), *det.host(), trk.host()[2])
    assert all(np.array_equal(sel.layout.view(out, i).cpu().numpy(), m) for i, m in enumerate(want[0]))
    assert np.array_equal(row_gt.cpu().numpy(), want[1]) and np.array_equal(stats.cpu().numpy(), want[2])


# ----------------------------------------------------------------------------------------------------------------- overlay ----
def make_maps():
    """One frame and one instance map per size: patches of a coarse random grid of values -- background, tracks (the values 1, 12, 13, 252
    among them), 253, 254 and 255 -- so that different values touch along straight and ragged borders and at the frame's border."""
    rng = np.random.default_rng(21)
    values = np.array([0, 0, 0, 1, 2, 5, 12, 13, 100, 252, 253, 254, 255, 255], np.uint8)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    images[5].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    maps = []
    for h, w in SIZES:
        coarse = values[rng.integers(0, len(values), ((h + 6) // 7, (w + 8) // 9))]
        m = np.kron(coarse, np.ones((7, 9), np.uint8))[:h, :w].copy()
        speck = rng.random((h, w)) < 0.03
        m[speck] = values[rng.integers(0, len(values), int(speck.sum()))]
        maps.append(m)
    maps[4][32, 64] = 9  # one pixel of another value one past a tile's edge and corner
    return images, maps


class PackedMaps(Packed):
    """test_overlay_native_gpu.Packed with the masks' buffer under the name overlay_instances looks for: `data` there is the frames'."""

    @property
    def maps(self):
        return SimpleNamespace(map=self.binary, layout=self.layout)


@pytest.fixture(scope="module")
def samples(gpu):
    images, maps = make_maps()
    return images, maps, PackedMaps(images, maps)


def test_the_overlay_inputs_exercise_what_they_are_meant_to():
    images, maps = make_maps()
    seen = {int(v) for m in maps for v in np.unique(m)}
    assert {0, 1, 12, 13, 252, 253, 254, 255} <= seen
    for e in (1, 2, 8):
        _, c = overlay_instances_np(images[5], maps[5], edge=e)
        assert c.any() and not (c & (maps[5] == 0)).any() and (e > 1 or ((maps[5] != 0) & ~c).any()), e
    _, c = overlay_instances_np(images[4], maps[4], edge=1)
    assert c[32, 64] and c[31, 63] == (maps[4][31, 63] != 0)  # decided across the tile's edge and corner


@pytest.mark.parametrize("edge", [0, 1, 2, 8])
def test_overlay_against_the_restatement(samples, edge):
    from unsupervised_detection_amd.visualize import overlay_instances
    images, maps, p = samples
    rng = np.random.default_rng(6)
    palettes = ([(250, 3, 128)], PALETTE, [tuple(int(v) for v in c) for c in rng.integers(0, 256, (64, 3))])
    for palette in palettes:
        for alpha, beta in ((0.5, 0.4), (1.0, 0.0)):
            got = overlay_instances(p.frames, p.maps, alpha=alpha, beta=beta, edge=edge, palette=palette, other_colour=(90, 91, 92))
            assert len(got) == len(SIZES)
            for i, (im, m) in enumerate(zip(images, maps)):
                want, _ = overlay_instances_np(im, m, alpha, beta, edge, palette, (90, 91, 92))
                g = got.sample(i)
                assert g.dtype == torch.uint8 and tuple(g.shape) == im.shape
                assert np.array_equal(g.cpu().numpy(), want), (edge, len(palette), alpha, i, SIZES[i])
    # the defaults are the track palette and grey; a saturating blend
    got = overlay_instances(p.frames, p.maps, edge=edge)
    sat = overlay_instances(p.frames, p.maps, alpha=1.0, beta=1.0, edge=edge)
    for i, (im, m) in enumerate(zip(images, maps)):
        assert np.array_equal(got.sample(i).cpu().numpy(), overlay_instances_np(im, m, edge=edge)[0]), (edge, i)
        assert np.array_equal(sat.sample(i).cpu().numpy(), overlay_instances_np(im, m, 1.0, 1.0, edge)[0]), (edge, i)


def test_overlay_guards_order_and_a_misaligned_base(samples):
    from unsupervised_detection_amd.visualize import overlay_instances
    images, maps, p = samples
    base = overlay_instances(p.frames, p.maps, edge=2)
    assert torch.equal(base.data, overlay_instances(p.frames, p.maps, edge=2).data)
    order = [5, 0, 3, 1, 4, 2]
    sizes = [SIZES[i][0] * SIZES[i][1] for i in order]
    offsets, at = [], 5
    for k, s in enumerate(sizes):
        offsets.append(at)
        at += s + (3, 1, 8, 2, 5, 9)[k]
    assert {o % 4 for o in offsets} == {0, 1, 2, 3}
    q = PackedMaps(images, maps, offsets, at, order)
    out = torch.full((3 * at,), GUARD, dtype=torch.uint8, device="cuda")
    got = overlay_instances(q.frames, q.maps, edge=2, out=out)
    assert got.data.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    written = np.zeros(3 * at, bool)
    for k, i in enumerate(order):
        o, n = 3 * offsets[k], 3 * sizes[k]
        written[o:o + n] = True
        assert np.array_equal(host[o:o + n], base.sample(i).cpu().numpy().reshape(-1)), (k, i)
    assert (~written).sum() == 3 * (5 + 3 + 1 + 8 + 2 + 5 + 9) and (host[~written] == GUARD).all()
    # image_rgb / out_rgb at a base pointer one byte off alignment: the byte-by-byte path
    for i in (3, 4, 5):
        alone = PackedMaps([images[i]], [maps[i]])
        assert torch.equal(overlay_instances(alone.frames, alone.maps, edge=2).sample(0), base.sample(i)), i
        shifted = torch.full((alone.data.numel() + 1,), GUARD, dtype=torch.uint8, device="cuda")
        shifted[1:] = alone.data
        f = Packed._Frames()
        f.data, f.layout = shifted[1:], alone.frames_layout
        dst = torch.full((alone.data.numel() + 2,), GUARD, dtype=torch.uint8, device="cuda")
        assert f.data.data_ptr() % 4 == 1
        got = overlay_instances(f, alone.maps, edge=2, out=dst[1:-1])
        assert torch.equal(got.sample(0), base.sample(i)) and int(dst[0]) == GUARD and int(dst[-1]) == GUARD, i


def test_refused_overlay_calls_leave_the_output_untouched(samples):
    from unsupervised_detection_amd._ffi import lib
    images, maps, p = samples
    total = p.layout.numel
    out = torch.full((3 * total,), GUARD, dtype=torch.uint8, device="cuda")
    d_off, d_hw = p.layout.device_tables(out.device)
    pal = torch.tensor([(r << 16) | (g << 8) | b for r, g, b in PALETTE], dtype=torch.int32, device="cuda")
    ok = dict(OVER_OK, image=p.data.data_ptr(), map=p.binary.data_ptr(), n=p.layout.n, offsets=d_off.data_ptr(), hw=d_hw.data_ptr(),
              max_h=p.layout.max_h, max_w=p.layout.max_w, total=total, palette=pal.data_ptr(), p=12, out=out.data_ptr(),
              stream=torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    for change in (dict(n=0), dict(n=65536), dict(image=None), dict(map=None), dict(offsets=None), dict(hw=None), dict(out=None), dict(palette=None),
                   dict(max_h=0), dict(max_w=0), dict(edge=-1), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf), dict(beta=nan), dict(beta=inf),
                   dict(p=0), dict(p=65), dict(palette=ok["palette"] + 2), dict(other=0x1000000)):
        a = dict(ok, **change)
        assert lib.udet_overlay_instances_ragged(*[a[k] for k in OVER_ORDER]) == -5 and b"overlay_instances_ragged" in lib.udet_last_error(), change
    assert lib.udet_overlay_instances_ragged(*[dict(ok, edge=9)[k] for k in OVER_ORDER]) == -4  # UDET_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())
    assert lib.udet_overlay_instances_ragged(*[ok[k] for k in OVER_ORDER]) == 0
    torch.cuda.synchronize()
    for i, (im, m) in enumerate(zip(images, maps)):
        assert np.array_equal(p.frames_layout.view(out, i).cpu().numpy(), overlay_instances_np(im, m)[0]), i


# -------------------------------------------------------------------------------------------------------------- end to end ----
def test_restore_results_dir_with_instances_end_to_end(gpu, tmp_path):
    """The stage with its real callables on the small mixed tree equals the run on the numpy stand-ins, file for file."""
    from test_components_gpu import speckled_restore_gpu
    from unsupervised_detection_amd.native_results import (component_boxes, draw_instance_overlays, instance_maps, link_detections,
                                                           load_gt_device, load_images_device, score_device, select_components)
    kw = dict(instances={"overlay": True}, overlay={"edge": 1})
    ref, want, _ = run_tree(tmp_path, "ref", True, 3, **dict(stand_ins([], [], 1), **kw))
    out, got, _ = run_tree(tmp_path, "dev", True, 3, restore=speckled_restore_gpu, load_gt=load_gt_device, score=score_device,
                           select=select_components, detect=component_boxes, link=link_detections, paint=instance_maps,
                           draw_instances=draw_instance_overlays, load_images=load_images_device, draw=never,
                           detections={"min_area": 2, "max_detections": 3}, tracks={"min_iou": 0.2, "max_gap": 1}, **kw)
    assert json.loads(json.dumps(got)) == json.loads(json.dumps(want)) and got["instances"] == {"overlay": True} and 0 < got["best_track_J"] < 1
    a, b = _tree_files(out), _tree_files(ref)
    assert sorted(a) == sorted(b) and sum(name.startswith("instances" + os.sep) for name in a) == 14
    for name in a:
        if name != "native_eval.json":
            assert a[name] == b[name], name
