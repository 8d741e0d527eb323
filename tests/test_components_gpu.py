"""GPU: udet_select_components_ragged (csrc/components.hip) through native_results.select_components -- labels, selected and info
against the scipy restatement of tests/test_components.py, for both connectivities and the three modes.  Everything is integer: every
comparison is exact equality.  The shapes are the smallest at which a tiled union-find can go wrong: degenerate and ragged frames in
one call, components that span many tiles on thin bridges, a chain through every tile boundary, a connection at a tile corner only."""
import json
import os

import numpy as np
import pytest
import torch

from test_components import (DENSITIES, MODES, best_gt_case, checkerboard, components_np, corner_blobs, ragged_masks, run_component_tree,
                             select_np, serpentine, tie_cases, _tree_files)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def pack(arrays, gap=0, fill=0):
    """Host arrays -> (packed device uint8, offsets, hw); gap: that many guard bytes (of `fill`) before, between and after the samples."""
    hw = np.array([a.shape for a in arrays], np.int64)
    sizes = hw[:, 0] * hw[:, 1]
    off = gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]])
    buf = np.full(int(off[-1] + sizes[-1] + gap), fill, np.uint8)
    for a, o, s in zip(arrays, off, sizes):
        buf[o:o + s] = np.asarray(a, np.uint8).reshape(-1)
    return torch.from_numpy(buf).cuda(), off, hw


_want = {}


def want_np(key, masks, gts, mode, conn):
    """The restatement of a batch, computed once per (key, mode, conn) and shared."""
    k = (key, mode, conn)
    if k not in _want:
        _want[k] = [components_np(m, None if gts is None else g, mode, conn) for m, g in zip(masks, gts if gts is not None else masks)]
    return _want[k]


def check_batch(key, masks, gts=None, modes=MODES, conns=(4, 8), gap=0):
    from unsupervised_detection_amd.native_results import select_components
    binary, off, hw = pack(masks, gap)
    gt = None if gts is None else pack(gts, gap)[0]
    for conn in conns:
        for mode in modes:
            if mode == "best_gt" and gt is None:
                continue
            got = select_components(binary, off, hw, gt=gt, mode=mode, connectivity=conn, want_labels=True)
            want = want_np(key, masks, gts, mode, conn)
            info = got.info.cpu().numpy()
            assert info.dtype == np.int64 and info.tolist() == [w[2] for w in want], (key, mode, conn)
            for i, w in enumerate(want):
                assert np.array_equal(got.labels_sample(i).cpu().numpy(), w[0]), (key, mode, conn, i)
                if mode == "label":
                    assert got.selected is None
                else:
                    assert np.array_equal(got.binary_sample(i).cpu().numpy(), w[1]), (key, mode, conn, i)
    return binary, off, hw, gt


def rect_gts(masks, seed=5):
    """An annotation per frame: a rectangle over the frame's middle, with holes."""
    rng = np.random.default_rng(seed)
    out = []
    for m in masks:
        h, w = m.shape
        g = np.zeros((h, w), np.uint8)
        g[h // 4:max(h // 4 + 1, 3 * h // 4), w // 5:max(w // 5 + 1, 4 * w // 5)] = 1
        out.append(g * (rng.random((h, w)) < 0.9))
    return out


@pytest.mark.parametrize("density", DENSITIES)
def test_degenerate_and_ragged_frames_in_one_call(gpu, density):
    masks = ragged_masks(density)
    check_batch(("ragged", density), masks, rect_gts(masks))


def test_guard_bytes_between_samples_stay_untouched(gpu):
    """Samples at odd offsets with guard bytes around them: the same results, and nothing written outside a sample."""
    from unsupervised_detection_amd.native_results import select_components
    masks = ragged_masks(0.593)
    gts = rect_gts(masks)
    check_batch(("ragged", 0.593), masks, gts, gap=37)
    binary, off, hw = pack(masks, 37)
    gt = pack(gts, 37)[0]
    got = select_components(binary, off, hw, gt=gt, mode="best_gt", connectivity=8, want_labels=True)
    sel, lab = got.selected.clone(), got.labels.clone()
    sel2 = torch.full_like(sel, 0xA5)
    lab2 = torch.full_like(lab, -7)
    # run again into poisoned buffers: what the kernels do not write keeps the poison
    from unsupervised_detection_amd import native_results as nr
    from unsupervised_detection_amd._ffi import check, lib
    d_off, d_hw = torch.from_numpy(off).cuda(), torch.from_numpy(hw.astype(np.int32)).cuda()
    info = torch.empty((len(off), 4), dtype=torch.int64, device="cuda")
    ws = torch.empty((lib.udet_components_workspace_bytes(binary.numel(), len(off)) + 7) // 8, dtype=torch.int64, device="cuda")
    check(lib.udet_select_components_ragged(binary.data_ptr(), gt.data_ptr(), len(off), d_off.data_ptr(), d_hw.data_ptr(), int(hw[:, 0].max()),
                                            int(hw[:, 1].max()), binary.numel(), 8, nr.COMPONENT_MODES["best_gt"], lab2.data_ptr(),
                                            sel2.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    guard = np.ones(binary.numel(), bool)
    for o, (h, w) in zip(off, hw):
        guard[o:o + h * w] = False
    assert guard.sum() == 37 * (len(off) + 1)
    assert (sel2.cpu().numpy()[guard] == 0xA5).all() and (lab2.cpu().numpy()[guard] == -7).all()
    assert np.array_equal(sel2.cpu().numpy()[~guard], sel.cpu().numpy()[~guard]) and np.array_equal(lab2.cpu().numpy()[~guard], lab.cpu().numpy()[~guard])
    assert torch.equal(info, got.info)


def test_zeros_ones_and_checkerboard(gpu):
    masks = [np.zeros((37, 53), np.uint8), np.ones((37, 53), np.uint8), checkerboard(), np.ones((67, 131), np.uint8), np.zeros((1, 1), np.uint8)]
    check_batch("flat", masks, rect_gts(masks))
    assert want_np("flat", masks, None, "label", 4)[2][2][0] == 980 and want_np("flat", masks, None, "label", 8)[2][2][0] == 1


def test_serpentine(gpu):
    s = serpentine()
    check_batch("serpentine", [s, s[:, ::-1].copy(), s.T.copy()], modes=("label", "largest"))
    assert want_np("serpentine", None, None, "largest", 4)[0][2] == [1, 0, int(s.sum()), 0]


def test_connection_at_a_tile_corner_only(gpu):
    from unsupervised_detection_amd.native_results import COMPONENT_TILE
    masks = corner_blobs(*COMPONENT_TILE)
    check_batch("corner", masks, modes=("label", "largest"))
    for i in range(2):
        assert want_np("corner", None, None, "label", 4)[i][2][0] == 2 and want_np("corner", None, None, "label", 8)[i][2][0] == 1


def test_best_gt_differs_from_largest_and_every_tie_break(gpu):
    m, gt = best_gt_case()
    check_batch("best_gt", [m], [gt], modes=("largest", "best_gt"))
    assert want_np("best_gt", None, None, "largest", 4)[0][2][1] != want_np("best_gt", None, None, "best_gt", 4)[0][2][1]
    cases = tie_cases()
    check_batch("ties", [c[1] for c in cases], [c[2] for c in cases], modes=("largest", "best_gt"))
    for conn in (4, 8):
        for mode in ("largest", "best_gt"):
            assert [w[2][1] for w in want_np("ties", None, None, mode, conn)] == [c[3][mode] for c in cases]


def test_benchmark_size_frame_straight_from_restore(gpu):
    """480 x 854 restored from a 192 x 384 mask; RestoredMasks goes into select_components as it is (no host copy in between)."""
    from unsupervised_detection_amd.native_results import GtBatch, restore_masks, select_components
    rng = np.random.default_rng(3)
    soft = rng.random((1, 192, 384)).astype(np.float32)
    soft[0, 60:140, 100:300] += 0.35  # a blob under the noise: many small components and a large one
    res = restore_masks(torch.from_numpy(soft).cuda(), [(480, 854)], 0.9, 0.62)
    gtm = np.zeros((480, 854), np.uint8)
    gtm[150:330, 250:700] = 1
    gt = GtBatch(torch.from_numpy(gtm.reshape(-1)).cuda(), res.offsets, res.hw)
    binary = res.binary_sample(0).cpu().numpy()
    for conn in (4, 8):
        for mode in ("largest", "best_gt"):
            got = select_components(res, gt=gt, mode=mode, connectivity=conn, want_labels=True)
            labels, sel, info = components_np(binary, gtm, mode, conn)
            assert info[0] > 100 and got.info.cpu().numpy().tolist() == [info], (mode, conn)
            assert np.array_equal(got.labels_sample(0).cpu().numpy(), labels) and np.array_equal(got.binary_sample(0).cpu().numpy(), sel)
            assert got.stack([0]).shape == (1, 480, 854, 1) and got.stack([0]).dtype == torch.float32


def test_two_calls_are_byte_identical(gpu):
    from unsupervised_detection_amd.native_results import select_components
    masks = ragged_masks(0.593) + [serpentine()]
    binary, off, hw = pack(masks)
    gt = pack(rect_gts(masks))[0]
    for conn in (4, 8):
        a = select_components(binary, off, hw, gt=gt, mode="best_gt", connectivity=conn, want_labels=True)
        b = select_components(binary, off, hw, gt=gt, mode="best_gt", connectivity=conn, want_labels=True)
        assert torch.equal(a.labels, b.labels) and torch.equal(a.selected, b.selected) and torch.equal(a.info, b.info)


def speckled_restore_gpu(masks, native_hw, crop=0.9, threshold=None):
    """restore_masks plus the specks of test_components.speckled_restore_np, set on the device."""
    from unsupervised_detection_amd.native_results import restore_masks
    r = restore_masks(masks, native_hw, crop, threshold)
    for i in range(len(r)):
        b = r.binary_sample(i)
        if min(b.shape) >= 12:
            b[2, 4] = b[b.shape[0] - 3, b.shape[1] - 5] = 1
            b[b.shape[0] - 5:b.shape[0] - 3, 5:8] = 1
    return r


@pytest.mark.parametrize("mixed", [False, True])
def test_restore_results_dir_best_gt_end_to_end(gpu, tmp_path, mixed):
    ref, want, _ = run_component_tree(tmp_path, "ref", mixed, component="best_gt", connectivity=4, select=select_np)
    from unsupervised_detection_amd.native_results import load_gt_device, score_device, select_components
    out, got, _ = run_component_tree(tmp_path, "dev", mixed, component="best_gt", connectivity=4, restore=speckled_restore_gpu,
                                     load_gt=load_gt_device, score=score_device, select=select_components)
    assert json.loads(json.dumps(got)) == json.loads(json.dumps(want))
    assert got["component"] == "best_gt" and got["sequences"]["bear"]["components_mean"] >= 3
    a, b = _tree_files(out), _tree_files(ref)
    assert sorted(a) == sorted(b) and len(a) == 13
    for name in a:
        if name != "native_eval.json":
            assert a[name] == b[name], name
    with open(os.path.join(out, "native_eval.json")) as f:
        assert json.load(f) == json.loads(json.dumps(want))
