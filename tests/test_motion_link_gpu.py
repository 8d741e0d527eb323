"""GPU: udet_flow_displacements_ragged (csrc/motion.hip), udet_link_detections_motion_ragged and udet_link_detections_gap_motion_ragged
(csrc/tracks.hip) through native_motion.flow_displacements, native_results.link_detections(disp=...) and the C ABI, the driver with
tracks={"motion": ...} and the BackwardFlow provider -- against the numpy restatements of tests/test_motion_link.py.  The displacements
are float32 arithmetic pinned operation by operation and the link is integer work: every comparison is exact equality.  The largest
frame is 130 x 259, the smallest that spans more than one 4096-pixel pass of the overlap kernel."""
import json
import os

import numpy as np
import pytest
import torch

from test_components import DENSITIES, ragged_masks
from test_detections import DetectionsNp
from test_motion_link import (BLOB_IDS, DISP_OK, DISP_ORDER, F32, MOTION_ORDER, SIZES, bridge_motion_np, displacements_np, links_motion_np,
                              onto_root, pack_np, random_fields, sequences, smooth_fields, translating_blobs, unpack_np)
from test_track_gaps import TracksGapNp, sequence_inputs
from test_track_gaps_gpu import equal as equal_gaps
from test_track_gaps_gpu import fields as gap_fields
from test_tracks import LINK_OK, links_np, moving_sequence
from test_tracks_gpu import equal, host_labels, inputs

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (2, 3), (8, 16), (64, 128)]
GUARD, FILL = 64, -77
GARBAGE = np.array([0x7fff7fff, -1, -2 ** 31, 0x00010001, 123456789, -77], np.int64).astype(np.int32)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def layout_of(hw, gap=0):
    """The PackedLayout of samples hw with `gap` guard elements before, between and after them (0: back to back)."""
    from unsupervised_detection_amd.ragged import PackedLayout
    sizes = np.array([h * w for h, w in hw])
    off = gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]])
    return PackedLayout(off, hw, int(off[-1] + sizes[-1] + gap))


def pack_disp(disps, layout, linked=None):
    """Per-frame packed [H, W] displacements -> the device int32 buffer of `layout`; the guard elements, and the frames that are not
    linked (linked: per frame 0 / 1), hold garbage."""
    buf = np.resize(GARBAGE, layout.numel).copy()
    for i, (o, (h, w)) in enumerate(zip(layout.offsets, layout.hw)):
        if linked is None or linked[i]:
            buf[o:o + h * w] = np.asarray(disps[i], np.int32).reshape(-1)
    return torch.from_numpy(buf).cuda()


def samples(buf, layout):
    host = buf.cpu().numpy()
    return [host[o:o + h * w].reshape(h, w) for o, (h, w) in zip(layout.offsets, layout.hw)]


# ----------------------------------------------------------------------------------------------------------- displacements ----
def raw_displacements(flow, layout, change=None):
    """One call of the C entry point on a buffer of FILL -> (status, the buffer on the host)."""
    from unsupervised_detection_amd._ffi import lib
    d_flow = torch.from_numpy(np.ascontiguousarray(flow, F32)).cuda()
    d_off, d_hw = layout.device_tables(torch.device("cuda", torch.cuda.current_device()))
    disp = torch.full((layout.numel,), FILL, dtype=torch.int32, device="cuda")
    a = dict(DISP_OK, flow=d_flow.data_ptr(), n=layout.n, fh=flow.shape[1], fw=flow.shape[2], offsets=d_off.data_ptr(), hw=d_hw.data_ptr(),
             max_h=layout.max_h, max_w=layout.max_w, total=layout.numel, disp=disp.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    a.update({p: (a[p] + v[1] if isinstance(v, tuple) else v) for p, v in (change or {}).items()})
    rc = lib.udet_flow_displacements_ragged(*[a[p] for p in DISP_ORDER])
    torch.cuda.synchronize()
    return rc, disp.cpu().numpy()


def random_flows(grid, seed, special=False):
    """One flow field per size of SIZES on `grid`, in grid pixels, with magnitudes up to the frame's size; special: NaN, infinities and
    values beyond the 16-bit range sprinkled in."""
    rng = np.random.default_rng(seed)
    fh, fw = grid
    out = np.empty((len(SIZES), fh, fw, 2), F32)
    for i, (H, W) in enumerate(SIZES):
        out[i] = rng.uniform(-1, 1, (fh, fw, 2)).astype(F32) * np.array([fw, fh], F32)  # times W / fw, H / fh: up to W, H native pixels
    if special:
        flat = out.reshape(-1)
        flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = np.resize(np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 4e4, -4e4, 32767.5], F32),
                                                                               max(2, flat.size // 7))
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_displacements_equal_the_restatement(gpu, grid):
    from unsupervised_detection_amd.native_motion import flow_displacements
    tight, odd = layout_of(SIZES), layout_of(SIZES, 37)
    for special in (False, True):
        flow = random_flows(grid, 3 + special, special)
        want = [displacements_np(flow[i], H, W) for i, (H, W) in enumerate(SIZES)]
        d_flow = torch.from_numpy(flow).cuda()
        got = flow_displacements(d_flow, tight)
        assert got.dtype == torch.int32 and tuple(got.shape) == (tight.numel,) and got.device == d_flow.device
        for i, (g, w) in enumerate(zip(samples(got, tight), want)):
            bad = np.argwhere(g != w)
            assert not len(bad), (grid, special, i, bad[:3].tolist(), [unpack_np(v[tuple(bad[0])]) for v in (g, w)])
        assert torch.equal(flow_displacements(d_flow, tight), got)  # twice
        # odd sample offsets with guard words on both sides of every sample: they stay what they were
        rc, host = raw_displacements(flow, odd)
        assert rc == 0
        guard = np.ones(odd.numel, bool)
        for i, (o, (h, w)) in enumerate(zip(odd.offsets, odd.hw)):
            assert np.array_equal(host[o:o + h * w].reshape(h, w), want[i]), (grid, special, i)
            guard[o:o + h * w] = False
        assert (host[guard] == FILL).all() and guard.sum() == 37 * 7
        # a sample alone is what it is inside the batch
        for i in (3, 5):
            alone = flow_displacements(d_flow[i:i + 1].contiguous(), layout_of(SIZES[i:i + 1]))
            assert np.array_equal(alone.cpu().numpy().reshape(SIZES[i]), want[i]), (grid, special, i)
    dx, dy = unpack_np(np.concatenate([w.reshape(-1) for w in want]))  # of the run with the special values: a NaN's 0 and the clamp occur
    assert ((dx == 0) | (dy == 0)).any() and (grid == (1, 1) or (dx == -32768).any() or (dx == 32767).any() or (dy == -32768).any() or (dy == 32767).any())


def test_displacements_on_a_grid_of_the_samples_size_and_a_constant_flow(gpu):
    from unsupervised_detection_amd.native_motion import flow_displacements
    rng = np.random.default_rng(8)
    for H, W in SIZES:  # the centres coincide and every ratio is 1: disp = rint(flow), ties to even
        flow = (rng.integers(-40, 41, (1, H, W, 2)) + rng.choice([0.0, 0.5, 0.25, -0.5], (1, H, W, 2))).astype(F32)
        got = flow_displacements(torch.from_numpy(flow).cuda(), layout_of([(H, W)])).cpu().numpy().reshape(H, W)
        r = np.rint(flow[0]).astype(np.int64)
        assert np.array_equal(got, pack_np(r[..., 0], r[..., 1])) and np.array_equal(got, displacements_np(flow[0], H, W)), (H, W)
    assert (np.abs(flow - np.trunc(flow)) == 0.5).any()
    const = np.broadcast_to(np.array([2.5, -1.25], F32), (len(SIZES), 8, 16, 2)).copy()
    layout = layout_of(SIZES)
    got = samples(flow_displacements(torch.from_numpy(const).cuda(), layout), layout)
    for (H, W), g in zip(SIZES, got):
        dx, dy = unpack_np(g)
        assert (dx == int(np.rint(F32(2.5) * (F32(W) / F32(16))))).all() and (dy == int(np.rint(F32(-1.25) * (F32(H) / F32(8))))).all(), (H, W)


def test_displacements_refused_calls_write_nothing(gpu):
    layout = layout_of(SIZES, 5)
    flow = random_flows((8, 16), 1)
    for change in (dict(flow=None), dict(offsets=None), dict(hw=None), dict(disp=None), dict(n=0), dict(n=65536), dict(fh=0), dict(fw=0),
                   dict(fh=32768), dict(fw=32768), dict(max_h=0), dict(max_w=0), dict(total=0), dict(flow=("+", 4)), dict(disp=("+", 2))):
        rc, host = raw_displacements(flow, layout, change)
        assert rc == -5 and (host == FILL).all(), change
    rc, host = raw_displacements(flow, layout)
    assert rc == 0 and (host != FILL).any()


# -------------------------------------------------------------------------------------------------------------------- link ----
def shapes_of(frames):
    return [f.shape for f in frames]


@pytest.mark.parametrize("density", DENSITIES)
def test_the_motion_link_equals_the_restatement(gpu, density):
    """The six sequences in one ragged call, both connectivities, k 1 / 16 / 64, every threshold: smooth fields, and per-pixel random
    fields whose sources leave the frame on every side (the extremes of the 16-bit range among them); zero displacement against the
    co-located entry itself.  The frames that are not linked carry garbage in their disp."""
    from unsupervised_detection_amd.native_results import link_detections
    frames, link = sequences(density)
    smooth, wild = smooth_fields(shapes_of(frames), 21)[1], random_fields(shapes_of(frames), 5)
    zero = [np.zeros(s, np.int32) for s in shapes_of(frames)]
    matched = differ = 0
    for conn in (4, 8):
        for k in (1, 16, 64):
            sel, det = inputs(frames, k, 1, conn)
            labels, (dets, counts) = host_labels(sel), det.host()
            d_smooth, d_wild, d_zero = (pack_disp(d, sel.layout, link) for d in (smooth, wild, zero))
            for permille in (1, 100, 1000):
                got = link_detections(sel, det, link=link, min_iou=permille / 1000, disp=d_smooth)
                want = links_motion_np(labels, dets, counts, link, permille, smooth)
                equal(got, want, (density, conn, k, permille, "smooth"))
                assert got.motion and tuple(got.inter.shape) == (len(frames), k, k) and got.inter.dtype == torch.int64
                matched += int((want.match >= 0).sum())
                plain = link_detections(sel, det, link=link, min_iou=permille / 1000)
                differ += int(not np.array_equal(plain.host()[0], want.inter))
                still = link_detections(sel, det, link=link, min_iou=permille / 1000, disp=d_zero)
                for f, a, b in zip(("inter", "match", "ids", "linked", "seq_tracks"), still.host(), plain.host()):
                    assert np.array_equal(a, b), (density, conn, k, permille, "zero", f)
                assert torch.equal(still.next_id, plain.next_id) and not plain.motion
            equal(link_detections(sel, det, link=link, disp=d_wild), links_motion_np(labels, dets, counts, link, 100, wild), (density, conn, k, "wild"))
    assert matched > 100 and differ >= 9  # of 18 combinations: the fields change the overlap (tests/test_motion_link.py counts the frames)


def test_extremes_a_frame_onto_one_pixel_and_the_translating_blobs(gpu):
    from unsupervised_detection_amd.native_results import link_detections
    frames, link = sequences(0.593)
    sel, det = inputs(frames, 16, 1, 8)
    labels, (dets, counts) = host_labels(sel), det.host()
    for j, (dx, dy) in enumerate(((32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 0), (0, 32767))):  # every source is outside
        far = [np.full(s, pack_np(dx, dy), np.int32) for s in shapes_of(frames)]
        got = link_detections(sel, det, link=link, disp=pack_disp(far, sel.layout))
        equal(got, links_motion_np(labels, dets, counts, link, 100, far), ("far", j))
        assert not got.host()[0].any() and (got.host()[1] == -1).all()
    a = int(counts[-2, 2]) - 1  # the whole last frame onto the root of its predecessor's smallest row: inter > area_a
    onto = [np.zeros(s, np.int32) for s in shapes_of(frames[:-1])] + [onto_root(frames[-1].shape, dets[-2, a, 0])]
    got = link_detections(sel, det, link=link, min_iou=0.001, disp=pack_disp(onto, sel.layout))
    want = links_motion_np(labels, dets, counts, link, 1, onto)
    equal(got, want, ("onto",))
    assert want.inter[-1, a, 0] > dets[-2, a, 1] and want.match[-1, 0] == a
    # three blobs that move further than their extent: 18 tracks without the flow, 3 with it, the ids written out by hand
    frames, disps, _ = translating_blobs()
    sel, det = inputs(frames, 4)
    got = link_detections(sel, det, disp=pack_disp(disps, sel.layout))
    equal(got, links_motion_np(host_labels(sel), *det.host(), [1] * 6, 100, disps), ("blobs",))
    assert got.host()[2][:, :3].tolist() == BLOB_IDS and int(got.next_id.cpu()[0]) == 3
    assert int(link_detections(sel, det).next_id.cpu()[0]) == 18


def test_carry_pieces_a_batch_twice_and_labels_out_of_range(gpu):
    from unsupervised_detection_amd.native_results import component_boxes, link_detections
    frames = moving_sequence(ragged_masks(0.45)[3], 7, 1)
    disps = smooth_fields(shapes_of(frames), 9)[1]
    sel, det = inputs(frames, 16, 2, 4)
    labels, (dets, counts) = host_labels(sel), det.host()
    whole = link_detections(sel, det, disp=pack_disp(disps, sel.layout))
    want = links_motion_np(labels, dets, counts, [1] * 7, 100, disps)
    equal(whole, want)
    assert (want.match >= 0).sum() > 20 and not np.array_equal(want.inter, links_np(labels, dets, counts, [1] * 7, 100).inter)
    again = link_detections(sel, det, disp=pack_disp(disps, sel.layout))
    assert all(np.array_equal(a, b) for a, b in zip(whole.host(), again.host()))  # twice
    ref = whole.host()
    for cuts in ((3, 3, 1), (1,) * 7):  # the carried frame: frame 0's own displacement reaches into it
        carry, s = None, 0
        for c in cuts:
            psel, pdet = inputs(frames[s:s + c], 16, 2, 4)
            part = link_detections(psel, pdet, carry=carry, disp=pack_disp(disps[s:s + c], psel.layout))
            for f, g, r in zip(("inter", "match", "ids", "linked", "seq_tracks"), part.host(), ref):
                w = r[s:s + c].copy()
                if f == "seq_tracks":  # the piece's last frame ends the sequence within its call
                    w[:] = 0
                    w[-1] = int(part.next_id.cpu()[0])
                assert np.array_equal(g, w), (cuts, s, f)
            carry = part.tail()
            s += c
        assert int(part.next_id.cpu()[0]) == want.next_id
    # the sequence inside a batch of several (odd offsets: guard elements with garbage), and a carried frame of another size
    a, b = moving_sequence(ragged_masks(0.45)[4][:33, :65], 3, 5), moving_sequence(ragged_masks(0.3)[3][:9, :13], 4, 6)
    link = [0, 1, 1] + [0] + [1] * 6 + [0, 1, 1, 1]
    every = smooth_fields(shapes_of(a), 1)[1] + disps + smooth_fields(shapes_of(b), 2)[1]
    bsel, bdet = inputs(a + frames + b, 16, 2, 4, gap=37)
    batch = link_detections(bsel.labels, bdet, link=link, disp=pack_disp(every, bsel.layout, link))
    for f, g, r in zip(("inter", "match", "ids", "linked", "seq_tracks"), batch.host(), ref):
        assert np.array_equal(g[3:10], r), f
    equal(batch, links_motion_np(host_labels(bsel), *bdet.host(), link, 100, every), ("batch",))
    other = link_detections(*inputs(a, 16, 2, 4)).tail()
    equal(link_detections(sel, det, carry=other, disp=pack_disp(disps, sel.layout)), want, ("another size",))  # frame 0 starts a sequence
    # whole components (and background pixels) overwritten with values outside 0..H*W: they vanish, nothing else changes
    lab = sel.labels.cpu().numpy().copy()
    poison = np.array([2 ** 31 - 1, -1, -2 ** 31], np.int32)
    for i, (o, (h, w)) in enumerate(zip(sel.offsets, sel.hw)):
        v = lab[o:o + h * w]
        for j, r in enumerate(np.unique(v[v > 0])[::3]):
            v[v == r] = h * w + 1 if j % 4 == 0 else poison[j % 3]
        v[np.flatnonzero(v == 0)[::5]] = poison[i % 3]
    dev = torch.from_numpy(lab).cuda()
    pdet = component_boxes(dev, min_area=2, max_detections=16, offsets=sel.layout)
    plabels = [sel.layout.view(dev, i).cpu().numpy() for i in range(len(sel))]
    pwant = links_motion_np(plabels, *pdet.host(), [1] * 7, 100, disps)
    equal(link_detections(dev, pdet, disp=pack_disp(disps, sel.layout)), pwant, ("poison",))
    assert not np.array_equal(pwant.inter, want.inter)


def raw_link(sel, det, link, permille, disp, change=None):
    """One call of udet_link_detections_motion_ragged on guarded outputs -> (status, {name: numpy array}, guards intact)."""
    from unsupervised_detection_amd._ffi import lib
    n, k, total = len(sel), det.k, sel.labels.numel()
    shapes = dict(inter=(n, k, k), match=(n, k), ids=(n, k), linked=(n,), seq=(n,), next_id=(1,))
    bufs = {f: torch.full((2 * GUARD + int(np.prod(s)),), FILL, dtype=torch.int64 if f == "inter" else torch.int32, device="cuda")
            for f, s in shapes.items()}
    words = lib.udet_link_detections_workspace_bytes(total, n, k, 0, 0) // 4
    ws = torch.empty(words + 1, dtype=torch.int32, device="cuda")
    d_link = torch.tensor(link, dtype=torch.int32, device="cuda")
    a = dict(LINK_OK, labels=sel.labels.data_ptr(), n=n, offsets=sel.dev_offsets.data_ptr(), hw=sel.dev_hw.data_ptr(),
             max_h=int(max(h for h, _ in sel.hw)), max_w=int(max(w for _, w in sel.hw)), total=total, dets=det.dets.data_ptr(),
             counts=det.counts.data_ptr(), k=k, link=d_link.data_ptr(), permille=permille, disp=disp.data_ptr(), ws=ws.data_ptr(),
             ws_bytes=words * 4, stream=torch.cuda.current_stream().cuda_stream,
             **{f: t.data_ptr() + GUARD * t.element_size() for f, t in bufs.items()})
    a.update({p: (a[p] + v[1] if isinstance(v, tuple) else v) for p, v in (change or {}).items()})
    rc = lib.udet_link_detections_motion_ragged(*[a[p] for p in MOTION_ORDER])
    torch.cuda.synchronize()
    host = {f: t.cpu().numpy() for f, t in bufs.items()}
    intact = all((v[:GUARD] == FILL).all() and (v[-GUARD:] == FILL).all() for v in host.values())
    return rc, {("seq_tracks" if f == "seq" else f): host[f][GUARD:-GUARD].reshape(s) for f, s in shapes.items()}, intact


def test_guards_around_every_output_and_refused_calls(gpu):
    frames, link = sequences(0.45)
    sel, det = inputs(frames, 16, 2, 8)
    wild = random_fields(shapes_of(frames), 11)
    disp = pack_disp(wild, sel.layout, link)
    before = disp.clone()
    want = links_motion_np(host_labels(sel), *det.host(), link, 100, wild)
    rc, out, intact = raw_link(sel, det, link, 100, disp)
    assert rc == 0 and intact and torch.equal(disp, before)
    for f in ("inter", "match", "ids", "linked", "seq_tracks"):
        assert np.array_equal(out[f], getattr(want, f)), f
    assert int(out["next_id"][0]) == want.next_id
    for change in (dict(disp=None), dict(disp=("+", 2)), dict(labels=None), dict(link=None), dict(n=0), dict(k=65), dict(permille=0),
                   dict(ws=None), dict(ws_bytes=16), dict(inter=("+", 4)), dict(ids=None), dict(c_h=8, c_w=18)):
        rc, out, intact = raw_link(sel, det, link, 100, disp, change)
        assert rc == -5 and intact and all((v == FILL).all() for v in out.values()), change


# ---------------------------------------------------------------------------------------------------------------- gap form ----
@pytest.mark.parametrize("max_gap", [1, 3])
def test_the_gap_form_warps_stage_one_only(gpu, max_gap):
    from unsupervised_detection_amd.native_results import link_detections
    for size_index, density, k, conn in ((3, 0.3, 64, 8), (5, 0.45, 16, 4)):
        frames = sequence_inputs(size_index, density, k, conn)[0]
        sel, det = inputs(frames, k, 2, conn)
        labels, (dets, counts) = host_labels(sel), det.host()
        disps = smooth_fields(shapes_of(frames), 3)[1]
        d = pack_disp(disps, sel.layout)
        got = link_detections(sel, det, max_gap=max_gap, disp=d)
        want = bridge_motion_np(labels, dets, counts, [1] * 7, 100, max_gap, disps)
        equal_gaps(gap_fields(got), want, (size_index, "smooth"))
        assert got.motion and (want.back >= 2).any()
        stage1, plain = link_detections(sel, det, disp=d), link_detections(sel, det, max_gap=max_gap)
        assert all(np.array_equal(a, b) for a, b in zip(stage1.host()[:2] + stage1.host()[3:4], got.host()[:2] + got.host()[3:4]))
        assert torch.equal(got.gap_inter, plain.gap_inter) and not torch.equal(got.inter, plain.inter)
        still = link_detections(sel, det, max_gap=max_gap, disp=torch.zeros_like(d))  # zero displacement: the co-located entry, entry for entry
        equal_gaps(gap_fields(still), gap_fields(plain), (size_index, "zero"))
        # the sequence in pieces: the history's newest frame is what frame 0's displacement reaches into
        hist, s = None, 0
        for c in (3, 3, 1):
            psel, pdet = inputs(frames[s:s + c], k, 2, conn)
            part = link_detections(psel, pdet, carry=hist, max_gap=max_gap, disp=pack_disp(disps[s:s + c], psel.layout))
            for f in ("inter", "match", "ids", "gap_inter", "back", "prev"):
                assert np.array_equal(getattr(gap_fields(part), f), getattr(want, f)[s:s + c]), (size_index, s, f)
            hist = part.tail()
            s += c


# ------------------------------------------------------------------------------------------------------------------ driver ----
def test_restore_results_dir_with_motion(gpu, tmp_path):
    """The annotation-free stage on the small tree of test_frames_folder_gpu.py with detections, tracks, max_gap = 1 and motion: a
    synthetic provider (a seeded constant flow per frame), the real flow_displacements and link_detections; detections/ and
    tracks/<sequence>.json against the restatement on what the stage itself labelled.  No flow network runs."""
    import scipy.io as sio
    from test_frames_folder import frames_flags, raises
    from test_frames_folder_gpu import HW, make_tree
    from unsupervised_detection_amd.native_results import (flow_displacements, frame_lists_from_reader, link_detections, restore_results_dir,
                                                           summarise_tracks, track_records)
    root = make_tree(str(tmp_path / "clips"))
    saved = str(tmp_path / "saved")
    rng = np.random.default_rng(2)
    for seq in HW:
        os.makedirs(os.path.join(saved, seq))
        for k in range(4):
            m = (0.2 * rng.random((24, 32))).astype(np.float32)
            m[3 + k:12, 4:14 + k] += 0.7
            m[15:21, 18 + k:27] += 0.7
            m[4:6, 22:25] += 0.7
            sio.savemat(os.path.join(saved, seq, "result_%d.mat" % (k + 1)), {"pred_mask": m})
    seen, flows, resets = [], [], []

    class Provider(object):
        def reset(self):
            resets.append(len(flows))

        def __call__(self, frames):
            n = len(frames)
            f = np.random.default_rng(len(flows)).uniform(-10, 10, (n, 1, 1, 2)).astype(F32) * np.ones((n, 64, 128, 2), F32)
            flows.append(f)
            return torch.from_numpy(f).cuda()

    def link(labelled, det, **kw):
        seen.append((labelled, det, kw, link_detections(labelled, det, **kw)))
        return seen[-1][3]
    lists = frame_lists_from_reader(frames_flags(root))
    native = str(tmp_path / "native")
    kw = dict(mask_key="pred_mask", batch=3, component="largest", connectivity=4, detections={"min_area": 12, "max_detections": 3},
              load_gt=raises, score=raises, verbose=False, gt_rule="FRAMES")
    js = restore_results_dir(saved, lists, native, tracks={"min_iou": 0.1, "max_gap": 1, "motion": {"size": (64, 128)}}, link=link,
                             motion_flow=Provider(), **kw)
    assert js["tracks"] == {"min_iou": 0.1, "max_gap": 1} and js["track_motion"] == {"size": [64, 128]} and list(js)[-1] == "track_motion"
    assert resets == [0, 2] and [len(f) for f in flows] == [3, 1, 3, 1] and all(s[2]["disp"].dtype == torch.int32 for s in seen)
    batches, fl = iter(seen), iter(flows)
    for seq in HW:
        stems = ["frame_%d" % (k + 9) for k in range(4)]
        parts = [next(batches), next(batches)]
        flow = np.concatenate([next(fl), next(fl)])
        labels = [p[0].labels_sample(i).cpu().numpy() for p in parts for i in range(len(p[0]))]
        dets, counts = (np.concatenate([p[1].host()[j] for p in parts]) for j in (0, 1))
        disps = [displacements_np(flow[i], *labels[i].shape) for i in range(4)]
        for p, lo in zip(parts, (0, 3)):  # the stage's displacements are the restatement's
            for i in range(len(p[0])):
                assert np.array_equal(p[0].layout.view(p[2]["disp"], i).cpu().numpy(), disps[lo + i]), (seq, lo + i)
        want = bridge_motion_np(labels, dets, counts, [0, 1, 1, 1], 100, 1, disps)
        for f in ("inter", "match", "ids", "linked", "gap_inter", "back", "prev"):
            assert np.array_equal(np.concatenate([getattr(gap_fields(p[3]), f) for p in parts]), getattr(want, f)), (seq, f)
        with open(os.path.join(native, "detections", seq + ".json")) as f:
            got = json.load(f)
        plain = [[{k: v for k, v in d.items() if k not in ("track", "prev", "iou", "back")} for d in got[s]] for s in stems]
        trk = TracksGapNp(want, labels, DetectionsNp(dets, counts), None, 1)
        trk.motion = True
        recs = track_records(plain, trk)
        assert [got[s] for s in stems] == json.loads(json.dumps(recs)), seq
        with open(os.path.join(native, "tracks", seq + ".json")) as f:
            assert json.load(f) == json.loads(json.dumps(summarise_tracks(stems, recs, [not v for v in want.linked], gaps=True))), seq
        assert (want.match >= 0).sum() >= 2
    # without the key: no provider call, no disp=, the files of a run that never heard of motion
    plain_dir, none_dir = str(tmp_path / "plain"), str(tmp_path / "none")
    js0 = restore_results_dir(saved, lists, plain_dir, tracks={"min_iou": 0.1, "max_gap": 1}, **kw)
    js1 = restore_results_dir(saved, lists, none_dir, tracks={"min_iou": 0.1, "max_gap": 1, "motion": None}, motion_flow=raises, displace=raises, **kw)
    from test_components import _tree_files
    f0, f1 = _tree_files(plain_dir), _tree_files(none_dir)
    assert js0 == js1 and "track_motion" not in js0 and sorted(f0) == sorted(f1) and all(f0[k] == f1[k] for k in f0)
    assert sorted(f0) == sorted(_tree_files(native))


# ---------------------------------------------------------------------------------------------------------------- provider ----
def test_backward_flow_provider(gpu):
    """The only test that runs the flow network, at its smallest legal size: four 70 x 90 frames at 64 x 128 with seeded weights."""
    from unsupervised_detection_amd.native_motion import BackwardFlow
    from unsupervised_detection_amd.post_processing import PWCFlow
    from test_overlay_native_gpu import Packed
    flow_fn = PWCFlow()
    rng = np.random.default_rng(6)
    images = [rng.integers(0, 256, (70, 90, 3), dtype=np.uint8) for _ in range(4)]
    masks = [np.zeros((70, 90), np.uint8)] * 4
    whole = BackwardFlow(flow_fn, size=(64, 128), flow_batch=2)
    flow = whole(Packed(images, masks).frames)
    assert tuple(flow.shape) == (4, 64, 128, 2) and flow.dtype == torch.float32 and flow.is_cuda
    assert not flow[0].any() and flow[1:].abs().sum() > 0 and torch.isfinite(flow).all()
    pieces = BackwardFlow(flow_fn, size=(64, 128), flow_batch=2)
    head = pieces(Packed(images[:2], masks[:2]).frames)
    tail = pieces(Packed(images[2:], masks[2:]).frames)
    print("max|pieces - whole|:", [float((a - b).abs().max()) for a, b in ((head[1], flow[1]), (tail[0], flow[2]), (tail[1], flow[3]))])
    assert not head[0].any() and torch.equal(head[1], flow[1])
    assert torch.equal(tail[0], flow[2]) and torch.equal(tail[1], flow[3])  # row 0 of the second call: the pair across the calls
    pieces.reset()
    assert not pieces(Packed(images[2:], masks[2:]).frames)[0].any()
