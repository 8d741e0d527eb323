"""CPU: the host side of the dense CRF at native resolution -- check_crf_tables, the unary table, restore_results_dir
with crf={...} on numpy stand-ins (restore, image reader, CRF, select and score injected as in tests/test_native_results.py), the --crf
flags of both subcommands and run_crf_original_resolution's forwarding.  Also the inputs tests/test_crf_native_gpu.py shares: `scene`
(a picture with structure the mask can snap to: on noise pictures compat = 5 collapses the field to background and hides every error)
and CASES."""
import json
import os

import numpy as np
import pytest

from test_native_results import SEQS, davis_flags, frame_hw, load_gt_np, make_davis_tree, restore_np, score_np

# (H, W, radius, sxy, srgb, iters); compat = 5, seed = H * W
CASES = [(24, 32, 6, 3, 13, 5),    # the shape of tests/test_post_processing.py: both kernels and the oracle on one input
         (37, 53, 20, 7, 5, 5),    # odd sizes, a window wider than a tile, several strips
         (5, 70, 9, 3, 5, 5),      # fewer rows than the radius and than a tile
         (33, 17, 40, 14, 5, 3),   # the radius exceeds both dimensions: every pixel sees the whole frame
         (16, 16, 3, 1, 5, 5),     # one tile or less, tiny window
         (70, 130, 12, 4, 5, 4)]   # several tiles in both directions, interior tiles with no border
COMPAT = 5.0


def scene(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx, ry, rx = 0.5 * h, 0.45 * w, 0.3 * h, 0.25 * w
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
    base = np.where(inside, 170.0, 60.0)[..., None] + np.array([0.0, 12.0, -9.0])
    img = np.clip(base + rng.normal(0, 4.0, (h, w, 3)), 0, 255).astype(np.uint8)
    sy, sx = max(1, h // 12), max(1, w // 12)
    d = ((yy - cy - sy) / ry) ** 2 + ((xx - cx - sx) / rx) ** 2
    soft = 1.0 / (1.0 + np.exp(4.0 * (d - 1.0))) + 0.05 * rng.random((h, w))
    return img, (soft / soft.max()).astype(np.float32)


def test_check_crf_tables():
    from unsupervised_detection_amd.native_results import check_crf_tables
    off, hw = check_crf_tables([0, 12], [(3, 4), (2, 5)], 22)
    assert off.dtype == np.int64 and hw.dtype == np.int32 and off.tolist() == [0, 12] and hw.tolist() == [[3, 4], [2, 5]]
    check_crf_tables([14, 2], [(2, 5), (3, 4)], 24)  # any order, gaps allowed
    with pytest.raises(ValueError, match="overlap"):
        check_crf_tables([0, 11], [(3, 4), (2, 5)], 30)
    with pytest.raises(ValueError, match="outside"):
        check_crf_tables([0, 12], [(3, 4), (2, 5)], 21)
    with pytest.raises(ValueError, match="outside"):
        check_crf_tables([-1], [(3, 4)], 30)
    with pytest.raises(ValueError, match="2\\^31"):
        check_crf_tables([0], [(1 << 16, 1 << 15)], 1 << 40)
    with pytest.raises(ValueError):
        check_crf_tables([0], [(0, 4)], 30)
    with pytest.raises(ValueError):
        check_crf_tables([0, 1], [(1, 1)], 30)  # one size per offset
    with pytest.raises(ValueError, match="65535"):
        check_crf_tables(np.arange(65536), np.ones((65536, 2), np.int64), 65536)


@pytest.mark.parametrize("amax", [0, 1, 37, 254, 255])
def test_unary_table_equals_the_oracle(amax):
    """The table's entry of a byte = oracle_post.unary_from_mask of the float64 soft mask at a pixel of that byte, bit for bit."""
    from oracle.oracle_post import unary_from_mask
    from unsupervised_detection_amd.post_processing import unary_table
    rng = np.random.default_rng(amax)
    canvas = rng.integers(0, amax + 1, (9, 11)).astype(np.uint8)
    canvas[4, 5] = amax
    want = unary_from_mask(canvas.astype(np.float64) / (np.float64(amax) + 1e-8), 0.1)
    tab = unary_table([amax, 255])
    assert tab.shape == (2, 2, 256) and tab.dtype == np.float32
    got = tab[0][:, canvas]
    assert got.tobytes() == want.tobytes()
    if amax == 0:
        assert np.array_equal(got[1], np.full((9, 11), np.float32(-np.log(1e-6))))


def test_crf_params():
    from unsupervised_detection_amd.native_results import crf_params
    p = crf_params({"sxy": 60, "srgb": 5, "compat": 5, "gauss_k": 0.1})
    assert p == {"sxy": 60.0, "srgb": 5.0, "compat": 5.0, "gauss_k": 0.1, "iters": 50, "radius": 180}
    assert crf_params({"sxy": 2.5, "srgb": 5, "compat": 5, "gauss_k": 0.1, "iters": 0, "radius": 3})["radius"] == 3
    assert crf_params({"sxy": 2.5, "srgb": 5, "compat": 5, "gauss_k": 0.1, "radius": None})["radius"] == 8
    for bad in ({"sxy": 60}, {"sxy": 0, "srgb": 5, "compat": 5, "gauss_k": 0.1}, {"sxy": 1, "srgb": 5, "compat": 5, "gauss_k": 0.1, "radius": 0},
                {"sxy": 1, "srgb": 5, "compat": 5, "gauss_k": 0.1, "iters": -1}, {"sxy": 1, "srgb": 5, "compat": 5, "gauss_k": 0.1, "sigma": 2}):
        with pytest.raises(ValueError):
            crf_params(bad)


class ImagesNp(object):
    def __init__(self, arrays):
        self.arrays = arrays
        self.hw = np.array([a.shape[:2] for a in arrays], np.int32)


class RefinedNp(object):
    """What the stand-in CRF returns: the restored batch with `labels` as its binary masks."""

    def __init__(self, res, labels):
        self.res, self.labels, self.hw = res, labels, res.hw

    def binary_sample(self, i):
        return self.labels[i]

    def stack(self, idx):
        return np.stack([self.labels[i] for i in idx]).astype(np.float32)[..., None]


def crf_np(img, soft):
    """A stand-in with the CRF's inputs and none of its cost: foreground where the frame's red channel is bright and the restored mask
    is not empty there -- it depends on the frame, so a wrong frame <-> mask pairing shows, and differs from soft > 0.5."""
    return ((img[..., 0] > 120) & (soft > 0.05)).astype(np.uint8)


@pytest.mark.parametrize("mixed", [False, True])
def test_restore_results_dir_with_crf_host_logic(tmp_path, mixed):
    import scipy.io as sio
    from PIL import Image
    from unsupervised_detection_amd.data import _read_image
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_davis_tree(tmp_path, mixed)
    lists = frame_lists_from_reader(davis_flags(root))
    calls = []

    def load_images_np(paths):
        return ImagesNp([_read_image(p, 3) for p in paths])

    def refine_np(restored, images, crf):
        calls.append((len(images.arrays), [a.shape[:2] for a in images.arrays], dict(crf)))
        assert np.array_equal(images.hw, restored.hw)
        return RefinedNp(restored, [crf_np(a, restored.soft(i)) for i, a in enumerate(images.arrays)])

    def select_np(pred, gt=None, mode="largest", connectivity=8):
        assert isinstance(pred, RefinedNp)  # the selection sees the CRF's labels, not the thresholded masks
        sel = RefinedNp(pred.res, [np.where(np.arange(l.shape[1])[None] < l.shape[1] // 2, l, 0).astype(np.uint8) for l in pred.labels])
        sel.info = np.array([[2, 0, int(l.sum()), 0] for l in sel.labels], np.int64)
        return sel

    crf = {"sxy": 4, "srgb": 5, "compat": 5, "gauss_k": 0.1, "iters": 3}
    out = str(tmp_path / "native_crf")
    got = restore_results_dir(res, lists, out, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False, crf=crf,
                              load_images=load_images_np, refine=refine_np)
    # once per batch (3 frames, batch 2: 2 + 1 per sequence), the batch's frames in the reader's order, the parameters filled in
    assert [c[0] for c in calls] == [2, 1, 2, 1]
    want_crf = {"sxy": 4.0, "srgb": 5.0, "compat": 5.0, "gauss_k": 0.1, "iters": 3, "radius": 12}
    assert all(c[2] == want_crf for c in calls)
    order = [frame_hw(seq, k, mixed) for seq in SEQS for k in range(3)]
    assert [hw for c in calls for hw in c[1]] == order
    js_j = {}
    for seq in SEQS:
        for k in range(3):
            H, W = frame_hw(seq, k, mixed)
            r = restore_np(masks[seq][k][None], [(H, W)], 0.9, 0.5)
            img = _read_image(os.path.join(root, "JPEGImages", "480p", seq, "%05d.jpg" % k), 3)
            want = crf_np(img, r.soft(0))
            assert want.any() and not np.array_equal(want, r.binary_sample(0))  # the check below tells the two apart
            with Image.open(os.path.join(out, seq, "%05d.png" % k)) as im:
                assert np.array_equal(np.asarray(im), want * 255)
            mat = sio.loadmat(os.path.join(out, seq, "result_%d.mat" % (k + 1)))
            assert np.array_equal(mat["mask"], want) and np.array_equal(mat["soft_mask"], r.soft(0).astype(np.float32))
            with Image.open(os.path.join(root, "Annotations", "480p", seq, "%05d.png" % k)) as im:
                g = (np.asarray(im) / 255.0 > 0.1).astype(np.uint8)
            js_j.setdefault(seq, []).append(score_np(g[None, ..., None], want[None, ..., None], 0.008)[0][0])
    with open(os.path.join(out, "native_eval.json")) as f:
        js = json.load(f)
    assert js == json.loads(json.dumps(got)) and js["crf"] == want_crf
    for seq in SEQS:  # the CRF's labels are what is scored
        assert js["category_iou"][seq] == pytest.approx(float(np.mean(js_j[seq])), abs=1e-12)
    # with a component selection: it is fed the CRF's labels, and its choice is what is written
    out2 = str(tmp_path / "native_crf_sel")
    got2 = restore_results_dir(res, lists, out2, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=3, verbose=False, crf=crf,
                               load_images=load_images_np, refine=refine_np, component="largest", select=select_np)
    assert got2["crf"] == want_crf and got2["component"] == "largest"
    mat = sio.loadmat(os.path.join(out2, "bear", "result_1.mat"))
    H, W = frame_hw("bear", 0, mixed)
    r = restore_np(masks["bear"][0][None], [(H, W)], 0.9, 0.5)
    want = crf_np(_read_image(os.path.join(root, "JPEGImages", "480p", "bear", "00000.jpg"), 3), r.soft(0))
    want[:, W // 2:] = 0
    assert np.array_equal(mat["mask"], want)
    with pytest.raises(ValueError):
        restore_results_dir(res, lists, str(tmp_path / "n3"), restore=restore_np, load_gt=load_gt_np, score=score_np, verbose=False,
                            crf={"sxy": 4}, load_images=load_images_np, refine=refine_np)


def _tree(d):
    return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}


def test_crf_none_changes_nothing(tmp_path):
    """crf=None: the outputs are byte-identical to a call that does not know the argument, and neither the image reader nor the CRF is
    touched."""
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, _ = make_davis_tree(tmp_path, True)
    lists = frame_lists_from_reader(davis_flags(root))

    def never(*a, **k):
        raise AssertionError("called without crf")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ja = restore_results_dir(res, lists, a, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False)
    jb = restore_results_dir(res, lists, b, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False, crf=None,
                             load_images=never, refine=never)
    assert ja == jb and "crf" not in ja and _tree(a) == _tree(b) and len(_tree(a)) == 13


def test_cli_crf_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    a = cli.parse_restore_results_args(base)
    assert a.crf is False and cli._crf(a) is None
    assert (a.sxy, a.srgb, a.scomp, a.gauss_k, a.crf_iters) == (60.0, 5.0, 5.0, 0.1, 50)  # post_processing.py:24-28,40
    a = cli.parse_restore_results_args(base + ["--crf"])
    assert cli._crf(a) == {"sxy": 60.0, "srgb": 5.0, "compat": 5.0, "gauss_k": 0.1, "iters": 50, "radius": None}
    from unsupervised_detection_amd.native_results import crf_params
    assert crf_params(cli._crf(a))["radius"] == 180
    a = cli.parse_restore_results_args(base + ["--crf", "--sxy", "25", "--srgb", "4", "--scomp", "3", "--gauss_k", "0.5", "--crf_iters", "10",
                                               "--crf_radius", "40", "--mask_key", "soft_mask", "--component", "best_gt"])
    assert cli._crf(a) == {"sxy": 25.0, "srgb": 4.0, "compat": 3.0, "gauss_k": 0.5, "iters": 10, "radius": 40}
    assert (a.mask_key, a.component) == ("soft_mask", "best_gt")
    d = default_flags()
    assert (d.crf, d.sxy, d.srgb, d.scomp, d.gauss_k, d.crf_iters) == (False, 60.0, 5.0, 5.0, 0.1, 50) and cli._crf(d) is None
    f = parse_flags(["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--crf", "--sxy", "30"])
    cli.check_native_flags(f)
    assert cli._crf(f) == {"sxy": 30.0, "srgb": 5.0, "compat": 5.0, "gauss_k": 0.1, "iters": 50, "radius": None}


def test_run_crf_original_resolution_forwards(monkeypatch):
    from unsupervised_detection_amd import native_results, post_processing
    seen = {}

    def fake(results_dir, frame_lists, out_dir, **kw):
        seen.update(results_dir=results_dir, frame_lists=frame_lists, out_dir=out_dir, **kw)
        return {"J": 1}
    monkeypatch.setattr(native_results, "restore_results_dir", fake)
    lists = {"bear": [("a.jpg", "a.png")]}
    assert post_processing.run_crf_original_resolution("soft", lists, 60.0, 5.0, 4.0, 0.1, "out", component="best_gt", crf_iters=7) == {"J": 1}
    assert seen == {"results_dir": "soft", "frame_lists": lists, "out_dir": "out", "mask_key": "soft_mask", "component": "best_gt",
                    "crf": {"sxy": 60.0, "srgb": 5.0, "compat": 4.0, "gauss_k": 0.1, "iters": 7, "radius": None}}
    post_processing.run_crf_original_resolution("soft", lists, 25.0, 5.0, 5.0, 0.1)
    assert seen["out_dir"] == "./post_processed_davis_original" and seen["crf"]["sxy"] == 25.0 and seen["crf"]["iters"] == 50
