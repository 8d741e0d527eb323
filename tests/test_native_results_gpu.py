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
