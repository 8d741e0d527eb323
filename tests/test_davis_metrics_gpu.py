"""GPU: udet_boundary_stats and the DAVIS-2016 measures built on it (evaluation.boundary_stats / evaluate_batch_davis /
evaluate_masks(davis_metrics=True) / the davis_eval subcommand).

The oracle below restates the published DAVIS measure db_eval_boundary in numpy: the boundary map of include/udet.h and matching by
scipy.ndimage.binary_dilation with a disk -- another formulation than the kernel's per-pixel window search over bit-packed rows.
Counts are integers: every comparison of counts, boundary maps and F is exact equality."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import binary_dilation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


# ---------------------------------------------------------------------------------------------------------------- oracle ----
def boundary_map(seg):
    seg = np.asarray(seg, dtype=bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def oracle_counts(fg, gt, r):
    """(n_fg, n_gt, fg_match, gt_match) and the two boundary maps of one pair of boolean masks"""
    bf, bg = boundary_map(fg), boundary_map(gt)
    d = disk(r)
    return [int(bf.sum()), int(bg.sum()), int((bf & binary_dilation(bg, d)).sum()), int((bg & binary_dilation(bf, d)).sum())], bf, bg


def oracle_f(c):
    n_fg, n_gt, m_fg, m_gt = (float(x) for x in c)
    if n_fg == 0 and n_gt > 0:
        p, r = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        p, r = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        p, r = 1.0, 1.0
    else:
        p, r = m_fg / n_fg, m_gt / n_gt
    return 0.0 if p + r == 0 else 2 * p * r / (p + r)


def oracle_j(fg, gt):
    u = int((fg | gt).sum())
    return 1.0 if u == 0 else int((fg & gt).sum()) / u


def oracle_stats(v, skip_ends=True):
    v = np.asarray(v, dtype=np.float64)
    if skip_ends:
        v = v[1:-1]
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(int)
    bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return {"mean": np.nanmean(v), "recall": np.nanmean(v > 0.5), "decay": np.nanmean(bins[0]) - np.nanmean(bins[3])}


# ------------------------------------------------------------------------------------------------------------- contents ----
def _tile_rows(r):  # rows of the kernel's tile (metrics.hip); its columns: 256, words: 64
    return 32 if r <= 16 else 64


def _rects_noise(h, w, r, k):
    """two overlapping rectangles, ~3 % salt noise in the ground truth: partial matches at every radius"""
    rng = np.random.default_rng(100 + k)
    fg, gt = np.zeros((h, w), bool), np.zeros((h, w), bool)
    fg[h // 4:3 * h // 4 + 1, w // 5 + k:3 * w // 5 + 1] = True
    gt[h // 3:2 * h // 3 + 2, w // 3:w - 2 - k] = True
    gt ^= rng.random((h, w)) < 0.03
    return fg, gt


def _borders(h, w, r, k):
    """a mask that touches all four image borders against an interior one"""
    fg = np.ones((h, w), bool)
    fg[h // 3:h // 3 + 3 + k, w // 4:w // 2] = False
    gt = np.zeros((h, w), bool)
    gt[max(h // 3 - r, 0):h // 3 + 2, w // 4 + k:w // 2 + r // 2] = True
    return fg, gt


def _single_pixel(h, w, r, k):
    fg, gt = np.zeros((h, w), bool), np.zeros((h, w), bool)
    y, x = h // 2, min(w // 2 + 20 * k, w - 1)
    fg[y, x] = True
    gt[min(y + (r * 3) // 5, h - 1), max(x - (r * 4) // 5 - k, 0)] = True  # (3, 4, 5): on the disk's edge when 5 divides r
    return fg, gt


def _checkerboard(h, w, r, k):
    yy, xx = np.mgrid[:h, :w]
    return (yy + xx + k) % 2 == 0, np.random.default_rng(200 + k).random((h, w)) < 0.5


def _edges(h, w, r, k):
    """single pixels (2 x 2 boundary blocks) whose nearest boundary pixels lie exactly r and r + 1 apart across a 64-column word
    edge, across the 256-column tile edge where the frame has one, and across the tile's row edge where it fits"""
    fg, gt = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for edge in (64, 256):
        xa = edge - 1 if edge + r + 1 <= w - 1 else None
        if xa is not None:
            y = min(5 + 3 * k + (edge // 64), h - 1)
            fg[y, xa] = True          # boundary columns xa - 1, xa
            gt[y, xa + r + 1] = True  # boundary columns xa + r, xa + r + 1
    ya = min(_tile_rows(r) - 1, h - 2 - r)
    if ya >= 1:
        x = min(10 + k, w - 1)
        gt[ya, x] = True              # and the other direction: ground truth above, prediction below
        fg[ya + r + 1, x] = True
    return fg, gt


CONTENTS = {"rects_noise": _rects_noise, "borders": _borders, "single_pixel": _single_pixel, "checkerboard": _checkerboard,
            "edges": _edges}
# (n, h, w, bound_th): radii 1, 3, 8, 18, 36 and the benchmark's own frame at the default 0.008 -> 8
CASES = [(3, 37, 83, 1), (3, 37, 83, 3), (2, 70, 150, 8), (2, 21, 200, 18), (1, 90, 130, 36), (1, 480, 854, 0.008)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)[..., None]).cuda().contiguous()


def _run(fgs, gts, bound_th, **kw):
    from unsupervised_detection_amd.evaluation import boundary_stats
    c, bp, bg = boundary_stats(_dev(np.stack(fgs)), _dev(np.stack(gts)), bound_th, threshold=0.5, gt_threshold=0.5, return_maps=True, **kw)
    assert c.dtype == np.int64 and c.shape == (len(fgs), 4)
    return c, bp.cpu().numpy(), bg.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("content", sorted(CONTENTS))
@pytest.mark.parametrize("n,h,w,bound_th", CASES)
def test_counts_and_maps_match_the_oracle(gpu, n, h, w, bound_th, content):
    from unsupervised_detection_amd.evaluation import boundary_radius, f_from_counts
    r = boundary_radius(h, w, bound_th)
    assert r == (8 if bound_th == 0.008 else bound_th)
    pairs = [CONTENTS[content](h, w, r, k) for k in range(n)]
    got, bp, bg = _run([p[0] for p in pairs], [p[1] for p in pairs], bound_th)
    for k, (fg, gt) in enumerate(pairs):
        want, wf, wg = oracle_counts(fg, gt, r)
        print(content, (n, h, w, r), k, "counts", got[k].tolist(), "oracle", want)
        assert np.array_equal(bp[k], wf.astype(np.uint8)) and np.array_equal(bg[k], wg.astype(np.uint8))
        assert got[k].tolist() == want
        assert float(f_from_counts(got[k])[0]) == oracle_f(want)


def test_largest_supported_radius(gpu):
    r = 63
    fg, gt = _rects_noise(40, 300, r, 0)
    got, _, _ = _run([fg], [gt], r)
    assert got[0].tolist() == oracle_counts(fg, gt, r)[0]


def test_hand_derived_anchors(gpu):
    from unsupervised_detection_amd.evaluation import compute_boundary_f, f_from_counts
    rect = np.zeros((40, 60), bool)
    rect[10:30, 15:45] = True  # 20 x 30: a closed contour of 2 * (20 + 30) = 100 boundary pixels
    shifted = [np.roll(rect, d, axis=1) for d in (0, 2, 3, 4)]
    got, _, _ = _run([rect] * 4, shifted, 3)
    assert got.tolist() == [[100, 100, 100, 100]] * 3 + [[100, 100, 66, 66]]
    f = f_from_counts(got)[0]
    assert f[:3].tolist() == [1.0, 1.0, 1.0] and abs(f[3] - 0.66) < 1e-15
    ones, zeros = np.ones((40, 60), bool), np.zeros((40, 60), bool)
    got, _, _ = _run([ones, zeros, zeros, ones], [rect, zeros, ones, rect], 3)
    assert got.tolist() == [[0, 100, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 100, 0, 0]]
    assert f_from_counts(got)[0].tolist() == [0.0, 1.0, 1.0, 0.0]
    # identical masks: F = 1 whatever the content; the single-image form
    fg, _ = _rects_noise(37, 83, 2, 1)
    noisy = fg ^ (np.random.default_rng(5).random(fg.shape) < 0.05)
    assert compute_boundary_f(noisy, noisy.astype(np.float32), bound_th=2) == (1.0, 1.0, 1.0)
    f, p, rc = compute_boundary_f(rect, np.roll(rect, 4, axis=1).astype(np.float32), bound_th=3)
    assert (p, rc) == (0.66, 0.66) and f == oracle_f([100, 100, 66, 66])


def test_flip_follows_the_border_statistics(gpu):
    """A prediction that hugs the image borders is scored as its complement when the border statistics of udet_mask_stats are
    passed, as itself when they are not; one flipped and one unflipped sample share a batch.  (The boundary map of a mask and of its
    complement coincide -- every term is an XOR of two pixels of the mask -- so the counts agree; the maps are checked too.)"""
    from unsupervised_detection_amd.evaluation import boundary_stats, mask_stats_device
    h, w, r = 50, 90, 4
    hug = np.ones((h, w), bool)
    hug[15:35, 20:70] = False
    inner, gt = _rects_noise(h, w, r, 0)
    pm, gm = _dev(np.stack([hug, inner])), _dev(np.stack([gt, gt]))
    st = mask_stats_device(pm, gm, 0.5, 0.5)
    score = st.cpu().numpy()[:, 0] / (4 * w + 4 * h)
    assert score[0] >= 0.6 > score[1]  # sample 0 is complemented, sample 1 is not
    flipped, bp, _ = boundary_stats(pm, gm, r, 0.5, 0.5, stats=st, return_maps=True)
    plain, bq, _ = boundary_stats(pm, gm, r, 0.5, 0.5, return_maps=True)
    want_c, map_c, _ = oracle_counts(~hug, gt, r)
    want_own, map_own, _ = oracle_counts(hug, gt, r)
    want_inner, map_inner, _ = oracle_counts(inner, gt, r)
    assert flipped.tolist() == [want_c, want_inner] and plain.tolist() == [want_own, want_inner]
    assert np.array_equal(bp.cpu().numpy(), np.stack([map_c, map_inner]).astype(np.uint8))
    assert np.array_equal(bq.cpu().numpy(), np.stack([map_own, map_inner]).astype(np.uint8))
    # the statistics may come from the host as well
    assert boundary_stats(pm, gm, r, 0.5, 0.5, stats=st.cpu().numpy()).tolist() == flipped.tolist()


def test_thresholds_are_strict(gpu):
    from unsupervised_detection_amd.evaluation import boundary_stats
    h, w, r = 37, 83, 3
    fg, gt = _rects_noise(h, w, r, 2)
    t, g = np.float32(0.1), np.float32(0.25)
    # outside the mask: exactly the threshold (excluded by >); inside: the next float above it
    pv = np.where(fg, np.nextafter(t, np.float32(1)), t).astype(np.float32)
    gv = np.where(gt, np.nextafter(g, np.float32(1)), g).astype(np.float32)
    got = boundary_stats(_dev(pv[None]), _dev(gv[None]), r, threshold=float(t), gt_threshold=float(g))
    assert got[0].tolist() == oracle_counts(fg, gt, r)[0]
    # the defaults: prediction > 0.1, ground truth > 0
    got = boundary_stats(_dev(np.where(fg, 0.11, 0.1)[None]), _dev(np.where(gt, 1e-6, 0.0)[None]), r)
    assert got[0].tolist() == oracle_counts(fg, gt, r)[0]


def test_samples_of_a_batch_are_independent(gpu):
    r = 5
    pairs = [_rects_noise(70, 150, r, 0), _checkerboard(70, 150, r, 1), _edges(70, 150, r, 2)]
    both, _, _ = _run([p[0] for p in pairs], [p[1] for p in pairs], r)
    for k, (fg, gt) in enumerate(pairs):
        alone, _, _ = _run([fg], [gt], r)
        assert alone[0].tolist() == both[k].tolist()


def test_bad_radius_is_an_error(gpu):
    from unsupervised_detection_amd._ffi import UdetError
    from unsupervised_detection_amd.evaluation import boundary_stats
    z = _dev(np.zeros((1, 16, 16)))
    with pytest.raises(ValueError, match="radius"):
        boundary_stats(z, z, bound_th=0.0)  # radius 0
    with pytest.raises(UdetError, match="maximum"):
        boundary_stats(z, z, bound_th=64)
    assert boundary_stats(z, z, bound_th=63).tolist() == [[0, 0, 0, 0]]


def test_evaluate_batch_davis(gpu):
    from unsupervised_detection_amd.evaluation import evaluate_batch, evaluate_batch_davis
    h, w = 48, 100
    hug = np.ones((h, w), bool)
    hug[10:30, 20:70] = False
    fg, gt = _rects_noise(h, w, 1, 0)
    pm, gm = _dev(np.stack([hug, fg, np.zeros((h, w), bool)])), _dev(np.stack([gt, gt, np.zeros((h, w), bool)]))
    iou, mae, flip, j, f = evaluate_batch_davis(gm, pm)
    iou0, mae0, flip0 = evaluate_batch(gm, pm)
    assert np.array_equal(iou, iou0) and np.array_equal(mae, mae0) and np.array_equal(flip, flip0) and flip.tolist() == [True, False, False]
    r = 1  # ceil(0.008 * sqrt(48^2 + 100^2)) = ceil(0.887)
    assert j.tolist() == [oracle_j(~hug, gt), oracle_j(fg, gt), 1.0]
    assert f.tolist() == [oracle_f(oracle_counts(~hug, gt, r)[0]), oracle_f(oracle_counts(fg, gt, r)[0]), 1.0]


class _SrcGt:
    """reader-style batches with an annotation, two categories (tests/test_learner_gpu.py's sources, with category names)"""

    def __init__(self, batch, n, hw=(128, 192)):
        self.batch, self.n, self.hw = batch, n, hw

    def __iter__(self):
        g = torch.Generator().manual_seed(1)
        for i in range(self.n):
            a = torch.rand(self.batch, *self.hw, 3, generator=g) - 0.5
            b = torch.rand(self.batch, *self.hw, 3, generator=g) - 0.5
            m = (torch.rand(self.batch, self.hw[0] // 8, self.hw[1] // 8, 1, generator=g) > 0.5).float()
            yield {"img1": a.cuda(), "img2": b.cuda(), "gt_mask": m.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous().cuda(),
                   "fname": [b"root/seq%d/f%d" % (i // 2, i * self.batch + j) for j in range(self.batch)]}


def test_evaluate_masks_davis_metrics(gpu, monkeypatch, capsys):
    from unsupervised_detection_amd import learner as Lr
    from unsupervised_detection_amd.config import default_flags
    from unsupervised_detection_amd.evaluation import evaluate_masks
    monkeypatch.setattr(Lr, "_engine_config", lambda config, batch=None, in_hw=(128, 192): Lr.EngineConfig(
        batch_size=batch or config.batch_size, in_height=128, in_width=192, img_height=config.img_height, img_width=config.img_width))

    def run(**kw):
        c = default_flags()
        c.img_height, c.img_width, c.batch_size, c.synthetic, c.autotune = 64, 128, 2, True, False
        c.data_source = _SrcGt(2, 4)
        lr = Lr.AdversarialLearner()
        lr.setup_inference(c, aug_test=False)
        capsys.readouterr()
        return evaluate_masks(lr, **kw), capsys.readouterr().out

    plain, text_plain = run()
    davis, text_davis = run(davis_metrics=True)
    assert set(plain) == {"category_iou", "category_mae", "dataset_iou", "dataset_mae", "sequence_iou", "frames"}
    assert set(davis) == set(plain) | {"category_f", "category_davis", "davis"}
    assert davis["category_iou"] == plain["category_iou"] and davis["frames"] == plain["frames"] == 8
    assert set(plain["category_iou"]) == {"seq0", "seq1"}
    assert "DAVIS" not in text_plain and text_davis.startswith(text_plain) and "J&F mean is" in text_davis[len(text_plain):]
    assert set(davis["category_f"]) == set(davis["category_davis"]) == {"seq0", "seq1"}
    vals = [davis["davis"]["J&F"]] + list(davis["category_f"].values())
    for d in [davis["davis"]] + list(davis["category_davis"].values()):
        assert set(d) - {"J&F"} == {"J", "F"} and all(set(d[m]) == {"mean", "recall", "decay"} for m in ("J", "F"))
        vals += [d[m][k] for m in ("J", "F") for k in d[m]]
    assert len(vals) == 21 and all(np.isfinite(v) and -1.0 <= v <= 1.0 for v in vals)
    assert davis["davis"]["J&F"] == (davis["davis"]["J"]["mean"] + davis["davis"]["F"]["mean"]) / 2


def test_davis_eval_subcommand(gpu, tmp_path, capsys):
    import scipy.io as sio
    from unsupervised_detection_amd import cli
    rng = np.random.default_rng(7)
    shapes = {"bear": [(24, 40)] * 5, "camel": [(24, 40), (30, 50), (24, 40), (30, 50), (30, 50), (24, 40)], "cows": [(33, 70)] * 3}
    want = {}
    for seq, shp in shapes.items():
        os.makedirs(tmp_path / seq)
        js, fs = [], []
        for k, (h, w) in enumerate(shp):
            gt = np.zeros((h, w), bool)
            gt[h // 4:3 * h // 4, w // 4:3 * w // 4] = True
            soft = np.clip(gt * 0.8 + rng.normal(0, 0.25, (h, w)) + 0.02 * k, 0, 1).astype(np.float32)
            pred = soft > 0.5
            sio.savemat(str(tmp_path / seq / "result_{}.mat".format(k + 1)),
                        {"pred_mask": pred, "soft_mask": soft, "gt_mask": gt.astype(np.float32)[..., None]})
            r = int(np.ceil(0.008 * np.sqrt(h * h + w * w)))
            js.append(oracle_j(pred, gt))
            fs.append(oracle_f(oracle_counts(pred, gt, r)[0]))
        want[seq] = {"J": oracle_stats(js), "F": oracle_stats(fs)}
    (tmp_path / "notes.txt").write_text("not a sequence")
    assert cli.main(["davis_eval", "--results_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    assert "J mean" in out and "F decay" in out and all(s in out for s in shapes) and "J&F mean is" in out
    res = json.load(open(tmp_path / "davis_eval.json"))
    assert set(res["sequences"]) == set(shapes) and res["mask_key"] == "pred_mask" and res["skip_ends"] is True
    for seq in shapes:
        assert res["sequences"][seq]["frames"] == len(shapes[seq])
        for m in ("J", "F"):
            for k in ("mean", "recall", "decay"):
                assert res["sequences"][seq][m][k] == pytest.approx(want[seq][m][k], abs=1e-12), (seq, m, k)
    for m in ("J", "F"):
        for k in ("mean", "recall", "decay"):
            assert res[m][k] == pytest.approx(np.mean([want[s][m][k] for s in shapes]), abs=1e-12)
    assert res["J&F"] == pytest.approx((res["J"]["mean"] + res["F"]["mean"]) / 2, abs=1e-15)
    # the soft scores at another threshold: the same frames, scored through the other key
    assert cli.main(["davis_eval", "--results_dir", str(tmp_path), "--mask_key", "soft_mask", "--threshold", "0.5", "--keep_ends"]) == 0
    res2 = json.load(open(tmp_path / "davis_eval.json"))
    assert res2["mask_key"] == "soft_mask" and res2["skip_ends"] is False and res2["sequences"]["bear"]["frames"] == 5
