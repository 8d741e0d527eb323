"""CPU: the host side of the native-resolution output stage (unsupervised_detection_amd/native_results.py) -- restore_box, the
table builder and its validation, restore_results_dir on numpy stand-ins, the restore_results subcommand's arguments.

restore_np below restates the restore from two things only: oracle_post.bytescale (on the mask widened to float64: the project's
pinned definition) and the real Pillow resize.  tests/test_native_results_gpu.py compares the kernel with it byte for byte."""
import json
import os

import numpy as np
import pytest

SIZES = [(30, 53), (17, 40), (13, 26), (9, 70)]  # (13, 26): ksize 5 horizontally, odd offset; (9, 70): shrinks in y, grows in x, y0 = 0


# ------------------------------------------------------------------------------------------------------------ restatement ----
def restore_patch_np(mask, h, w):
    """scipy.misc.imresize(mask, (h, w)) = bytescale + Pillow's 8-bit bilinear resize."""
    from PIL import Image
    from oracle.oracle_post import bytescale
    return np.asarray(Image.fromarray(bytescale(np.asarray(mask, dtype=np.float64))).resize((w, h), resample=Image.BILINEAR))


class RestoredNp(object):
    def __init__(self, frames, binaries, amax):
        self.frames, self.binaries, self.amax = frames, binaries, np.asarray(amax, np.int32)
        self.hw = np.array([f.shape for f in frames], np.int32)

    def sample(self, i):
        return self.frames[i]

    def binary_sample(self, i):
        return self.binaries[i]

    def soft(self, i):
        return self.frames[i].astype(np.float64) / (np.float64(self.amax[i]) + 1e-8)

    def stack(self, idx):
        return np.stack([self.binaries[i] for i in idx]).astype(np.float32)[..., None]


def restore_np(masks, native_hw, crop=0.9, threshold=None):
    from unsupervised_detection_amd.native_results import restore_box
    masks = np.asarray(masks)
    masks = masks[..., 0] if masks.ndim == 4 else masks
    frames, binaries, amax = [], [], []
    for m, (H, W) in zip(masks, np.asarray(native_hw).reshape(-1, 2)):
        y0, x0, h, w = restore_box(H, W, crop)
        patch = restore_patch_np(m, h, w)
        canvas = np.zeros((H, W), np.uint8)
        canvas[y0:y0 + h, x0:x0 + w] = patch
        frames.append(canvas)
        amax.append(int(patch.max()))
        soft = canvas.astype(np.float64) / (np.float64(amax[-1]) + 1e-8)
        binaries.append(None if threshold is None else (soft > threshold).astype(np.uint8))
    return RestoredNp(frames, binaries, amax)


def random_masks(n, mh=12, mw=24, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, mh, mw)) * rng.uniform(0.2, 3.0, (n, 1, 1)) - rng.uniform(0, 1, (n, 1, 1))).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- fixtures ----
class GtNp(object):
    def __init__(self, arrays):
        self.arrays = arrays
        self.hw = np.array([a.shape for a in arrays], np.int32)

    def sample(self, i):
        return self.arrays[i]

    def stack(self, idx):
        return np.stack([self.arrays[i] for i in idx]).astype(np.float32)[..., None]


def load_gt_np(paths, rule):
    from unsupervised_detection_amd.data import _read_image
    load = rule.loader or _read_image
    return GtNp([(load(p, 1)[..., 0] / 255.0 > rule.threshold).astype(np.uint8) for p in paths])


def score_np(gt_stack, pred_stack, bound_th):
    from test_davis_metrics_gpu import oracle_counts, oracle_f, oracle_j
    from unsupervised_detection_amd.evaluation import boundary_radius
    g, p = np.asarray(gt_stack)[..., 0] > 0.5, np.asarray(pred_stack)[..., 0] > 0.5
    r = boundary_radius(g.shape[1], g.shape[2], bound_th)
    return (np.array([oracle_j(a, b) for a, b in zip(p, g)]), np.array([oracle_f(oracle_counts(a, b, r)[0]) for a, b in zip(p, g)]))


SEQS = ("bear", "goat")
ODD = {("goat", 1): (17, 40)}  # mixed=True: one frame of another size inside a batch, the ragged path of restore_results_dir


def frame_hw(seq, k, mixed=False, hw=(30, 53)):
    return ODD.get((seq, k), hw) if mixed else hw


def make_davis_tree(tmp_path, mixed=False, frames=3, hw=(30, 53), mhw=(12, 24)):
    """A DAVIS-layout dataset (two sequences of `frames` hw frames; mixed: one frame of ODD's size among them) and a results folder of mhw
    masks; frame k of a sequence carries a blob whose place depends on k, so a wrong k <-> frame mapping shows.  Returns (root,
    results_dir, {seq: [mask, ...]})."""
    import scipy.io as sio
    from PIL import Image
    root, res = str(tmp_path / "DAVIS"), str(tmp_path / "results")
    rng = np.random.default_rng(7)
    lines, masks = [], {}
    for si, seq in enumerate(SEQS):
        for sub in ("JPEGImages", "Annotations"):
            os.makedirs(os.path.join(root, sub, "480p", seq))
        os.makedirs(os.path.join(res, seq))
        masks[seq] = []
        for k in range(frames):
            H, W = frame_hw(seq, k, mixed, hw)
            gt = np.zeros((H, W), np.uint8)
            gt[4 + 2 * k:20 + k, 6 + 5 * k + 3 * si:30 + 5 * k] = 255
            gt[0, 0] = 20  # 20 / 255 < 0.1: background by the DAVIS rule, foreground by a bare != 0
            Image.fromarray(gt, "L").save(os.path.join(root, "Annotations", "480p", seq, "%05d.png" % k))
            Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8), "RGB").save(os.path.join(root, "JPEGImages", "480p", seq, "%05d.jpg" % k))
            lines.append("/JPEGImages/480p/{0}/{1:05d}.jpg /Annotations/480p/{0}/{1:05d}.png".format(seq, k))
            m = (0.2 * rng.random(mhw)).astype(np.float32)
            m[2 + k:9, 2 + 2 * k + si:12 + 2 * k] += 0.7
            masks[seq].append(m)
            sio.savemat(os.path.join(res, seq, "result_%d.mat" % (k + 1)), {"mask": m, "gt_mask": np.zeros(mhw, np.float32)})
    os.makedirs(os.path.join(root, "ImageSets", "480p"))
    with open(os.path.join(root, "ImageSets", "480p", "val.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return root, res, masks


def davis_flags(root):
    from unsupervised_detection_amd.config import default_flags
    flags = default_flags()
    flags.root_dir, flags.dataset = root, "DAVIS2016"
    return flags


# ----------------------------------------------------------------------------------------------------------------- tests ----
def test_restore_box():
    from unsupervised_detection_amd.native_results import restore_box
    assert restore_box(480, 854, 0.9) == (24, 43, 432, 768)
    assert restore_box(30, 53, 0.9) == (1, 3, 27, 47)
    assert restore_box(13, 26, 0.9) == (1, 1, 11, 23)
    assert restore_box(9, 70, 0.9) == (0, 3, 8, 63)
    assert restore_box(30, 53, 1.0) == (0, 0, 30, 53) and restore_box(30, 53, 1.25) == (0, 0, 30, 53)
    with pytest.raises(ValueError):
        restore_box(1, 1, 0.9)
    with pytest.raises(ValueError):
        restore_box(0, 5, 1.0)


def test_tables_layout_and_coefficients_are_pillows():
    from oracle.oracle_post import _coeffs
    from unsupervised_detection_amd.native_results import build_restore_tables, check_restore_tables
    hw = SIZES + [(30, 53)]
    off, tab, coef = build_restore_tables(hw, 12, 24, 0.9)
    assert off.tolist() == np.concatenate([[0], np.cumsum([h * w for h, w in hw])[:-1]]).tolist()
    check_restore_tables(off, tab, coef, sum(h * w for h, w in hw), 12, 24)
    assert tab[0].tolist() == tab[4].tolist()  # one table per distinct (in, out) length
    for row in tab:
        h, w = int(row[2]), int(row[3])
        for (k0, b0, ks), n_in, n_out in ((row[6:9], 24, w), (row[9:12], 12, h)):
            kk, bounds, ksize = _coeffs(n_in, n_out)
            assert ks == ksize and coef[k0:k0 + n_out * ks].tolist() == kk.reshape(-1).tolist()
            assert coef[b0:b0 + 2 * n_out].tolist() == bounds.reshape(-1).tolist()
    assert tab[2][8] == 5 and tab[3][11] == 5 and tab[3][8] == 3  # (13,26): 24 -> 23 has ksize 5; (9,70): 12 -> 8 has 5, 24 -> 63 has 3
    # crop 1.0 at the mask's own size: both passes skipped
    _, t1, _ = build_restore_tables([(12, 24)], 12, 24, 1.0)
    assert t1[0].tolist() == [0, 0, 12, 24, 12, 24, -1, -1, 0, -1, -1, 0]


def test_table_validation_refuses_bad_tables():
    from unsupervised_detection_amd.native_results import build_restore_tables, check_restore_tables
    hw = [(30, 53), (13, 26)]
    total = 30 * 53 + 13 * 26
    off, tab, coef = build_restore_tables(hw, 12, 24, 0.9)
    check_restore_tables(off, tab, coef, total, 12, 24)

    def bad(off=off, tab=tab, coef=coef, numel=total, match=""):
        with pytest.raises(ValueError, match=match):
            check_restore_tables(off, tab, coef, numel, 12, 24)
    bad(off=[0, 30 * 53 + 1], match="outside the output buffer")
    bad(off=[-1, 30 * 53], match="outside the output buffer")
    bad(numel=total - 1, match="outside the output buffer")
    bad(off=[0, 30 * 53 - 1], match="overlap")
    bad(off=[13 * 26 - 5, 0], match="overlap")
    t = tab.copy(); t[0, 0] = 4  # y0 + h = 31 > 30
    bad(tab=t, match="box outside")
    t = tab.copy(); t[1, 1] = -1
    bad(tab=t, match="box outside")
    t = tab.copy(); t[1, 3] = 26; t[1, 1] = 1
    bad(tab=t, match="box outside")
    t = tab.copy(); t[1, 6] = len(coef) - 3
    bad(tab=t, match="coefficient index")
    t = tab.copy(); t[0, 10] = len(coef) - 2
    bad(tab=t, match="coefficient index")
    t = tab.copy(); t[0, 6] = -1  # a kk index without its bounds index
    bad(tab=t, match="coefficient index")
    t = tab.copy(); t[0, 6] = t[0, 7] = -1  # 24 -> 47 cannot be skipped
    bad(tab=t, match="cannot be skipped")
    c = coef.copy(); c[tab[0, 7] + 1] = 99  # a tap count beyond the mask
    bad(coef=c, match="tap")
    c = coef.copy(); c[tab[0, 10]] = 11; c[tab[0, 10] + 1] = 3  # first tap 11 + 3 taps > 12 mask rows
    bad(coef=c, match="tap")
    # restore_masks validates before it touches the device: these raise without a GPU
    from unsupervised_detection_amd.native_results import restore_masks
    with pytest.raises(ValueError):
        restore_masks(np.zeros((2, 12, 24), np.float32), hw, offsets=[0, 30 * 53 - 1])
    with pytest.raises(ValueError):
        restore_masks(np.zeros((2, 12, 24), np.float32), [(30, 53), (1, 1)])
    with pytest.raises(ValueError):
        restore_masks(np.zeros((2, 12, 24), np.float32), [(30, 53)])


def test_c_entry_point_refuses_bad_scalars_and_pointers():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd import native_results  # noqa: F401  (declares the argument types)
    from unsupervised_detection_amd._ffi import lib
    assert lib.udet_restore_workspace_bytes(16) >= 16 * 2 * 4 and lib.udet_restore_workspace_bytes(0) == 0
    ok = dict(masks=64, n=2, mh=12, mw=24, offsets=64, tab=64, coef=64, max_h=30, max_w=53, data=64, amax=64, binary=128, threshold=0.5,
              ws=64, ws_bytes=1 << 20, stream=None)
    for change in (dict(n=0), dict(n=65536), dict(mh=0), dict(mw=-1), dict(max_h=0), dict(max_w=0), dict(masks=None), dict(offsets=None),
                   dict(tab=None), dict(coef=None), dict(data=None), dict(amax=None), dict(threshold=-0.1), dict(threshold=float("nan")),
                   dict(threshold=float("inf")), dict(binary=64), dict(ws=None), dict(ws_bytes=8), dict(ws=66)):
        a = dict(ok, **change)
        rc = lib.udet_restore_masks_ragged(a["masks"], a["n"], a["mh"], a["mw"], a["offsets"], a["tab"], a["coef"], a["max_h"], a["max_w"],
                                           a["data"], a["amax"], a["binary"], a["threshold"], a["ws"], a["ws_bytes"], a["stream"])
        assert rc == -5 and b"restore_masks_ragged" in lib.udet_last_error(), change


def test_restatement_equals_the_fixed_point_oracle():
    from oracle.oracle_post import bytescale, pil_bilinear_u8
    from unsupervised_detection_amd.native_results import restore_box
    masks = random_masks(6, seed=3)
    for m, (H, W) in zip(masks, SIZES + [(12, 24), (24, 12)]):
        _, _, h, w = restore_box(H, W, 0.9 if (H, W) != (12, 24) else 1.0)
        got = restore_patch_np(m, h, w)
        assert got.dtype == np.uint8 and got.shape == (h, w)
        assert np.array_equal(got, pil_bilinear_u8(bytescale(m.astype(np.float64)), h, w)), (H, W)
    big = random_masks(1, 192, 384, seed=4)[0]
    assert np.array_equal(restore_patch_np(big, 432, 768), pil_bilinear_u8(bytescale(big.astype(np.float64)), 432, 768))
    r = restore_np(np.ones((1, 12, 24), np.float32), [(30, 53)], 0.9, 0.5)  # a constant mask restores to zeros
    assert r.amax.tolist() == [0] and not r.sample(0).any() and not r.binary_sample(0).any()


@pytest.mark.parametrize("mixed", [False, True])
def test_restore_results_dir_host_logic(tmp_path, mixed):
    import scipy.io as sio
    from PIL import Image
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_davis_tree(tmp_path, mixed)
    lists = frame_lists_from_reader(davis_flags(root))
    assert list(lists) == list(SEQS) and [os.path.basename(i) for i, _ in lists["goat"]] == ["00000.jpg", "00001.jpg", "00002.jpg"]
    assert all("Annotations" in a for _, a in lists["bear"])
    out = str(tmp_path / "native")
    got = restore_results_dir(res, lists, out, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False)
    for seq in SEQS:
        assert sorted(os.listdir(os.path.join(out, seq))) == ["00000.png", "00001.png", "00002.png", "result_1.mat", "result_2.mat", "result_3.mat"]
        for k in range(3):
            H, W = frame_hw(seq, k, mixed)
            want = restore_np(masks[seq][k][None], [(H, W)], 0.9, 0.5)
            with Image.open(os.path.join(out, seq, "%05d.png" % k)) as im:
                assert im.mode == "L" and im.size == (W, H)
                png = np.asarray(im)
            assert set(np.unique(png)) <= {0, 255} and png.any()
            assert np.array_equal(png, want.binary_sample(0) * 255)  # result_<k+1>.mat <-> frame k
            mat = sio.loadmat(os.path.join(out, seq, "result_%d.mat" % (k + 1)))
            assert {"mask", "soft_mask", "gt_mask"} <= set(mat)
            assert mat["soft_mask"].dtype == np.float32 and mat["soft_mask"].shape == (H, W)
            assert np.array_equal(mat["mask"], want.binary_sample(0)) and np.array_equal(mat["soft_mask"], want.soft(0).astype(np.float32))
            with Image.open(os.path.join(root, "Annotations", "480p", seq, "%05d.png" % k)) as im:
                assert np.array_equal(mat["gt_mask"], (np.asarray(im) / 255.0 > 0.1).astype(np.uint8))
            assert mat["gt_mask"][0, 0] == 0
    with open(os.path.join(out, "native_eval.json")) as f:
        js = json.load(f)
    assert js == json.loads(json.dumps(got))
    assert set(js) >= {"mask_key", "threshold", "crop", "bound_th", "skip_ends", "sequences", "J", "F", "J&F", "category_iou", "sequence_iou"}
    assert set(js["sequences"]) == set(SEQS) and js["sequences"]["bear"]["frames"] == 3 and js["skip_ends"] is True
    assert set(js["J"]) == {"mean", "recall", "decay"} and set(js["sequences"]["goat"]["F"]) == {"mean", "recall", "decay"}
    assert 0.0 < js["category_iou"]["bear"] < 1.0 and js["J&F"] == (js["J"]["mean"] + js["F"]["mean"]) / 2
    # a category whose .mat count differs from its list is an IOError naming it
    os.remove(os.path.join(res, "goat", "result_3.mat"))
    with pytest.raises(IOError, match="goat"):
        restore_results_dir(res, lists, str(tmp_path / "n2"), restore=restore_np, load_gt=load_gt_np, score=score_np, verbose=False)
    with pytest.raises(IOError, match="ghost"):
        restore_results_dir(res, {"ghost": lists["bear"]}, str(tmp_path / "n3"), restore=restore_np, load_gt=load_gt_np, score=score_np, verbose=False)


def test_cli_arguments():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    a = cli.parse_restore_results_args(["--results_dir", "D", "--out_dir", "O", "--dataset", "FBMS", "--root_dir", "/data/FBMS"])
    assert (a.results_dir, a.out_dir, a.dataset, a.root_dir) == ("D", "O", "FBMS", "/data/FBMS")
    assert (a.test_partition, a.test_temporal_shift, a.mask_key, a.crop, a.threshold, a.keep_ends) == ("val", 1, "mask", 0.9, 0.5, False)
    assert a.max_temporal_len == default_flags().max_temporal_len  # the reader's flags ride along
    a = cli.parse_restore_results_args(["--results_dir", "D", "--out_dir", "O", "--root_dir", "R", "--mask_key", "pred_mask", "--crop", "1.0",
                                        "--threshold", "0.3", "--keep_ends", "--test_temporal_shift", "-1"])
    assert (a.mask_key, a.crop, a.threshold, a.keep_ends, a.test_temporal_shift, a.dataset) == ("pred_mask", 1.0, 0.3, True, -1, "DAVIS2016")
    with pytest.raises(SystemExit):
        cli.parse_restore_results_args(["--results_dir", "D"])
    assert default_flags().native_resolution is False and parse_flags([]).native_resolution is False
    with pytest.raises(SystemExit):
        cli.main(["test_generator", "--native_resolution", "--generate_visualization"])  # no --test_save_dir
    with pytest.raises(SystemExit):
        cli.main(["test_generator", "--native_resolution", "--test_save_dir", "D"])  # no --generate_visualization
    cli.check_native_flags(parse_flags(["--native_resolution", "--generate_visualization", "--test_save_dir", "D"]))
