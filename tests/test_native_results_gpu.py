"""GPU: udet_restore_masks_ragged (csrc/restore.hip) and the native-resolution output stage built on it
(native_results.restore_masks / restore_results_dir), byte for byte against the Pillow restatement of tests/test_native_results.py
and against the per-frame composition of the soft-score stage (post_processing._imresize_window).  Everything is integer: every
comparison is exact equality."""
import json
import os

import numpy as np
import pytest
import torch

from test_native_results import SEQS, SIZES, davis_flags, make_davis_tree, random_masks, restore_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


@pytest.fixture(scope="module")
def batch(gpu):
    """The ragged batch of the issue: four native sizes, 12 x 24 masks, crop 0.9; restored once per threshold, shared."""
    from unsupervised_detection_amd.native_results import restore_masks
    masks = random_masks(len(SIZES), seed=11)
    dev = torch.from_numpy(masks).cuda()
    return masks, dev, {t: restore_masks(dev, SIZES, 0.9, t) for t in (0.1, 0.5)}


def _assert_equals_np(got, want, binary=True):
    assert got.amax.cpu().tolist() == want.amax.tolist()
    for i in range(len(want.frames)):
        assert np.array_equal(got.sample(i).cpu().numpy(), want.sample(i)), i
        if binary:
            assert np.array_equal(got.binary_sample(i).cpu().numpy(), want.binary_sample(i)), i


def test_bit_exact_against_pillow(batch):
    from unsupervised_detection_amd.native_results import restore_masks
    masks, dev, got = batch
    for t in (0.1, 0.5):
        _assert_equals_np(got[t], restore_np(masks, SIZES, 0.9, t))
        assert got[t].data.numel() == sum(h * w for h, w in SIZES)
    assert got[0.1].binary.sum() > got[0.5].binary.sum() > 0
    # crop 1.0 at the mask's own size: both passes skipped, the bytes are the bytescale itself
    for t in (0.1, 0.5):
        _assert_equals_np(restore_masks(dev[:2], [(12, 24), (12, 24)], 1.0, t), restore_np(masks[:2], [(12, 24), (12, 24)], 1.0, t))
    # [n,mh,mw,1] input, no binary mask
    r = restore_masks(dev[..., None].contiguous(), SIZES, 0.9)
    assert r.binary is None
    _assert_equals_np(r, restore_np(masks, SIZES, 0.9), binary=False)
    # the benchmark's own shape
    big = random_masks(1, 192, 384, seed=5)
    _assert_equals_np(restore_masks(torch.from_numpy(big).cuda(), [(480, 854)], 0.9, 0.5), restore_np(big, [(480, 854)], 0.9, 0.5))


def test_tile_reads_more_than_one_strip(gpu):
    """A tenfold vertical shrink: the 16 patch rows of one tile read about 160 mask rows, three 64-row strips of the horizontal
    intermediate (every other shape here stays inside the first)."""
    from unsupervised_detection_amd.native_results import restore_masks
    masks, sizes = random_masks(2, 200, 40, seed=23), [(20, 30), (23, 31)]
    _assert_equals_np(restore_masks(torch.from_numpy(masks).cuda(), sizes, 1.0, 0.5), restore_np(masks, sizes, 1.0, 0.5))


def test_bit_exact_against_per_frame_path(batch):
    from unsupervised_detection_amd.native_results import restore_box
    from unsupervised_detection_amd.post_processing import _imresize_window
    masks, dev, got = batch
    r = got[0.5]
    amax = r.amax.cpu().numpy()
    for i, (H, W) in enumerate(SIZES):
        y0, x0, h, w = restore_box(H, W, 0.9)
        patch = _imresize_window(dev[i].double(), 0, 0, 12, 24, h, w)
        canvas = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        canvas[y0:y0 + h, x0:x0 + w] = patch
        assert torch.equal(r.sample(i), canvas), i
        assert int(amax[i]) == int(patch.max())
        soft = r.soft(i)
        assert soft.dtype == torch.float64
        assert np.array_equal(soft.cpu().numpy(), canvas.cpu().numpy().astype(np.float64) / (np.float64(amax[i]) + 1e-8))


def test_constant_mask_single_sample_and_order(gpu):
    from unsupervised_detection_amd.native_results import restore_masks
    const = torch.full((1, 12, 24), 0.37, device="cuda")
    r = restore_masks(const, [(30, 53)], 0.9, 0.5)  # n = 1
    assert r.amax.cpu().tolist() == [0] and not r.data.any() and not r.binary.any()
    rng = np.random.default_rng(19)
    masks = random_masks(19, seed=19)
    masks[7] = -2.5  # a constant mask in the middle of a batch
    sizes = [SIZES[k] for k in rng.integers(0, len(SIZES), 19)]
    dev = torch.from_numpy(masks).cuda()
    r = restore_masks(dev, sizes, 0.9, 0.5)
    assert int(r.amax[7]) == 0 and not r.sample(7).any()
    for i in range(19):
        one = restore_masks(dev[i:i + 1], [sizes[i]], 0.9, 0.5)
        assert torch.equal(one.sample(0), r.sample(i)) and torch.equal(one.binary_sample(0), r.binary_sample(i)), i
        assert int(one.amax[0]) == int(r.amax[i])
    _assert_equals_np(r, restore_np(masks, sizes, 0.9, 0.5))


def test_sentinel_bytes_untouched(batch):
    from unsupervised_detection_amd.native_results import restore_masks
    masks, dev, got = batch
    G = 64
    sizes = [h * w for h, w in SIZES]
    offsets, pos = [], G
    for s in sizes:
        offsets.append(pos)
        pos += s + G
    out = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    binary = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    r = restore_masks(dev, SIZES, 0.9, 0.5, offsets=offsets, out=out, binary_out=binary)
    torch.cuda.synchronize()
    for buf in (out.cpu().numpy(), binary.cpu().numpy()):
        guard = np.ones(pos, bool)
        for o, s in zip(offsets, sizes):
            guard[o:o + s] = False
        assert guard.sum() == G * (len(sizes) + 1) and (buf[guard] == 0xA5).all()
    for i in range(len(SIZES)):
        assert torch.equal(r.sample(i), got[0.5].sample(i)) and torch.equal(r.binary_sample(i), got[0.5].binary_sample(i))


def test_native_scores(gpu):
    from test_davis_metrics_gpu import oracle_counts, oracle_f, oracle_j
    from unsupervised_detection_amd.evaluation import boundary_radius, evaluate_batch_davis
    from unsupervised_detection_amd.native_results import restore_box, restore_masks
    H, W = 30, 53
    y0, x0, h, w = restore_box(H, W, 0.9)
    rng = np.random.default_rng(2)
    masks = (0.1 * rng.random((3, 12, 24))).astype(np.float32)
    masks[0, 3:9, 0:10] += 0.8   # touches the crop's left edge
    masks[1, 2:7, 8:20] += 0.8
    masks[2, 0:12, 15:24] += 0.8  # touches three edges
    gts = np.zeros((3, H, W), bool)
    gts[0, 8:22, 0:22] = True    # the object runs on through the strip to the frame's edge
    gts[1, 6:16, 20:45] = True
    gts[2, :, 33:] = True
    r = restore_masks(torch.from_numpy(masks).cuda(), [(H, W)] * 3, 0.9, 0.5)
    pred = r.stack(range(3))
    assert pred.shape == (3, H, W, 1) and pred.dtype == torch.float32 and set(pred.unique().tolist()) <= {0.0, 1.0}
    gt = torch.from_numpy(gts.astype(np.float32)[..., None]).cuda().contiguous()
    _, _, flip, j, f = evaluate_batch_davis(gt, pred, 0.5, disambiguate=False)
    assert not flip.any()
    p = pred.cpu().numpy()[..., 0] > 0.5
    assert not p[:, :y0].any() and not p[:, :, :x0].any() and not p[:, y0 + h:].any() and not p[:, :, x0 + w:].any()
    rad = boundary_radius(H, W)
    for i in range(3):
        assert j[i] == oracle_j(p[i], gts[i]) and f[i] == oracle_f(oracle_counts(p[i], gts[i], rad)[0]), i
    # the strip outside the crop counts: scored on the full frame the mask loses against the same mask scored inside the crop
    inside = lambda t: t[:, y0:y0 + h, x0:x0 + w].contiguous()
    _, _, _, j_crop, _ = evaluate_batch_davis(inside(gt), inside(pred), 0.5, disambiguate=False)
    assert j_crop[0] == oracle_j(p[0, y0:y0 + h, x0:x0 + w], gts[0, y0:y0 + h, x0:x0 + w])
    assert 0 < j[0] < j_crop[0] and 0 < j[2] < j_crop[2]


@pytest.mark.parametrize("mixed", [False, True])
def test_restore_results_dir_end_to_end(gpu, tmp_path, mixed):
    from test_native_results import load_gt_np, score_np
    from unsupervised_detection_amd.evaluation import evaluate_results_dir
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, _ = make_davis_tree(tmp_path, mixed)
    lists = frame_lists_from_reader(davis_flags(root))
    ref_dir, out = str(tmp_path / "ref"), str(tmp_path / "native")
    want = restore_results_dir(res, lists, ref_dir, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False)
    got = restore_results_dir(res, lists, out, batch=2, verbose=False)
    for seq in SEQS:
        names = sorted(os.listdir(os.path.join(out, seq)))
        assert names == sorted(os.listdir(os.path.join(ref_dir, seq))) and len(names) == 6
        for n in names:
            skip = 128 if n.endswith(".mat") else 0  # a MAT-file's 128-byte header carries the time it was written
            with open(os.path.join(out, seq, n), "rb") as a, open(os.path.join(ref_dir, seq, n), "rb") as b:
                assert a.read()[skip:] == b.read()[skip:], (seq, n)
    assert json.loads(json.dumps(got)) == json.loads(json.dumps(want))  # the device's J and F equal the numpy / scipy restatement's
    ev = evaluate_results_dir(out, "mask", 0.5, verbose=False)
    assert ev["J"] == got["J"] and ev["F"] == got["F"] and ev["J&F"] == got["J&F"]
    for seq in SEQS:
        assert ev["sequences"][seq] == got["sequences"][seq]


RAGGED3 = [(30, 53), (13, 26), (9, 70)]  # the shapes of tests/test_ragged.py


def _count_table_uploads(monkeypatch):
    """Counts the uploads of a layout's own (offsets int64 [n], hw int32 [n,2]) pair; the restore tables' tab / coef upload is separate."""
    from unsupervised_detection_amd import ragged
    calls, real = [], ragged.upload_tables

    def counting(arrays, device):
        if len(arrays) == 2 and arrays[0].dtype == np.int64 and arrays[1].dtype == np.int32 and arrays[1].shape == (len(arrays[0]), 2):
            calls.append(arrays)
        return real(arrays, device)
    monkeypatch.setattr(ragged, "upload_tables", counting)
    return calls


def test_chain_by_layout_equals_chain_by_raw_tables(gpu, monkeypatch):
    """restore -> unary -> dense CRF -> select on three ragged samples with gaps and guard bytes, once handing the restored batch's
    layout along and once passing raw offsets / hw to every call: the same bytes everywhere, the guards untouched, and in the first form
    one upload of the layout's tables for the whole chain."""
    from test_crf_native import COMPAT, scene
    from unsupervised_detection_amd import native_restore
    from unsupervised_detection_amd.native_results import RestoredMasks, restore_masks, select_components
    monkeypatch.setattr(native_restore, "_restore_tables", {})  # the counts below start from a cold restore cache
    from unsupervised_detection_amd.post_processing import dense_crf_ragged, unary_from_restored
    masks = np.stack([scene(12, 24, 500 + k)[1] for k in range(3)])
    masks[1] = 0.25  # constant: restores to zeros, amax = 0
    areas = [h * w for h, w in RAGGED3]
    offsets = [40, 40 + areas[0] + 72, 40 + areas[0] + 72 + areas[1]]  # a gap in front, one between samples 0 and 1, a tail
    numel = offsets[2] + areas[2] + 24
    guard = np.ones(numel, bool)
    for o, a in zip(offsets, areas):
        guard[o:o + a] = False
    rgb = np.zeros(3 * numel, np.uint8)
    for (H, W), o in zip(RAGGED3, offsets):
        rgb[3 * o:3 * (o + H * W)] = scene(H, W, H * W)[0].reshape(-1)
    images, dev = torch.from_numpy(rgb).cuda(), torch.from_numpy(masks).cuda()
    uploads = _count_table_uploads(monkeypatch)

    def chain(by_layout):
        out, binary, labels = (torch.full((numel,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3))
        q = torch.full((numel,), -7.0, dtype=torch.float32, device="cuda")
        res = restore_masks(dev, RAGGED3, 0.9, 0.5, offsets=offsets, out=out, binary_out=binary)
        tables = (res.layout, None) if by_layout else (offsets, RAGGED3)
        unary = unary_from_restored(res.data, tables[0], tables[1], res.amax, 0.1)
        q1, lab = dense_crf_ragged(unary, images, tables[0], tables[1], 3, 5, COMPAT, iters=2, radius=5, q_out=q, labels_out=labels)
        if by_layout:
            sel = select_components(RestoredMasks(res.data, lab, res.layout, None, res.amax), mode="largest")
        else:
            sel = select_components(lab, offsets, RAGGED3, mode="largest")
        torch.cuda.synchronize()
        return res, unary, q1, lab, sel
    first = chain(True)
    assert len(uploads) == 1 and uploads[0][0] is first[0].layout.offsets and uploads[0][1] is first[0].layout.hw
    assert first[4].layout is first[0].layout
    second = chain(False)
    assert len(uploads) == 4  # the restore tables are cached with their layout; unary, CRF and selection each upload their raw tables
    (res, unary, q1, lab, sel), (res2, unary2, q2, lab2, sel2) = first, second
    assert torch.equal(res.data, res2.data) and torch.equal(res.binary, res2.binary) and torch.equal(res.amax, res2.amax)
    assert torch.equal(unary, unary2) and torch.equal(q1, q2) and torch.equal(lab, lab2) and torch.equal(sel.info, sel2.info)
    assert res.amax.cpu().tolist()[1] == 0 and lab.sum() > 0
    for i in range(3):
        assert torch.equal(sel.binary_sample(i), sel2.binary_sample(i)), i
        assert not (sel.binary_sample(i).bool() & ~res.layout.view(lab, i).bool()).any()
    for buf in (res.data, res.binary, lab, res2.data, res2.binary, lab2):
        assert (buf.cpu().numpy()[guard] == 0xA5).all()
    for buf in (q1, q2):
        assert (buf.cpu().numpy()[guard] == -7.0).all() and (buf.cpu().numpy()[~guard] >= 0).all()
    assert not unary.cpu().numpy()[:, guard].any()


def test_loader_batch_uploads_no_tables(gpu, tmp_path, monkeypatch):
    """A RaggedLoader batch's layout hands out the device tables that travelled with the pixels: nothing is uploaded for them."""
    from PIL import Image
    from unsupervised_detection_amd import data
    from unsupervised_detection_amd.native_results import GtBatch, select_components
    rng = np.random.default_rng(3)
    arrs = [(rng.random((h, w)) > 0.5).astype(np.uint8) * 255 for h, w in RAGGED3]
    paths = []
    for k, a in enumerate(arrs):
        paths.append(str(tmp_path / ("%d.png" % k)))
        Image.fromarray(a, "L").save(paths[-1])
    uploads = _count_table_uploads(monkeypatch)
    rb = data.RaggedLoader().load(paths, 1)
    d_off, d_hw = rb.layout.device_tables(rb.data.device)
    assert d_off is rb.dev_offsets and d_hw is rb.dev_hw
    assert d_off.data_ptr() + 16 * len(paths) == rb.data.data_ptr() and d_hw.data_ptr() == d_off.data_ptr() + 8 * len(paths)
    assert d_off.cpu().tolist() == rb.offsets.tolist() and d_hw.cpu().view(-1, 2).tolist() == rb.hw.tolist() == [list(s) for s in RAGGED3]
    got = rb.resize(12, 24, None, True, 255.0, 0.0)  # the input stage's launch reads them
    for i, a in enumerate(arrs):
        one = data.crop_flip_resize(torch.from_numpy(a[None, :, :, None].copy()).cuda(), 12, 24, None, True, 255.0, 0.0)
        assert torch.equal(got[i:i + 1], one), i
    gt = GtBatch((rb.data > 127).to(torch.uint8), rb.layout)  # and so does whatever the annotations' layout is handed to
    sel = select_components(gt.data, gt.layout, mode="label", want_labels=True)
    assert sel.layout is rb.layout and int(sel.info[:, 0].min()) >= 1
    torch.cuda.synchronize()
    assert uploads == []
