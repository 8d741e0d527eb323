"""GPU: flow / mask visualisation and training summaries (csrc/visualize.hip, visualize.py) against the reference's own images
(tests/golden/visualize.npz), numpy restatements written here, and through the training loop and the command line."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "visualize.npz")))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------ flow_to_image ----
@pytest.mark.parametrize("name", ["a", "b", "hi", "lo"])
def test_flow_to_image_matches_the_reference(gpu, golden, name):
    """No element off by more than one level, at most 1 in 1e5 elements different at all (room for a last-bit atan2 difference
    flipping a floor, nothing else: the reference restatement with atan2 perturbed by 2 ulp differs in 0 elements here)."""
    from unsupervised_detection_amd.visualize import flow_to_image
    flow, ref = golden["flow_" + name], golden["img_" + name]
    out = flow_to_image(_dev(flow))
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == ref.shape
    d = np.abs(out.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
    print(name, "max level difference", d.max(), "elements differing", int((d > 0).sum()), "of", d.size)
    assert d.max() <= 1
    assert (d > 0).sum() <= 1e-5 * d.size


def test_flow_to_image_nan_and_unknown(gpu):
    from unsupervised_detection_amd.visualize import flow_to_image
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((2, 9, 11, 2)) * 4).astype(np.float32)
    zeroed = f.copy()
    zeroed[0, 3, 4] = 0
    zeroed[0, 6, 2] = 0
    base = flow_to_image(_dev(zeroed)).cpu().numpy()
    bad = f.copy()
    bad[0, 3, 4] = (np.nan, 50.0)  # the finite component would be the batch maximum: a NaN pixel is left out of it entirely
    bad[0, 6, 2] = (1.0, 3e7)      # |v| > 1e7: both components are unknown and count as zero
    out = flow_to_image(_dev(bad)).cpu().numpy()
    assert out[0, 3, 4].tolist() == [0, 0, 0]
    assert out[0, 6, 2].tolist() == [255, 255, 255] and base[0, 6, 2].tolist() == [255, 255, 255]
    keep = np.ones(out.shape[:3], bool)
    keep[0, 3, 4] = False
    assert np.array_equal(out[keep], base[keep])  # sample 1 included: nothing is poisoned


def test_flow_to_image_with_mask(gpu):
    """A border-hugging mask (score >= 0.6) is complemented, a central one is not; object pixels are exactly 127, the rest is the
    unmasked image.  The border statistics never leave the device."""
    from unsupervised_detection_amd.visualize import flow_to_image
    rng = np.random.default_rng(6)
    f = (rng.standard_normal((2, 14, 18, 2)) * 2).astype(np.float32)
    mask = np.full((2, 14, 18, 1), 0.05, np.float32)
    mask[0] = 0.9
    mask[0, 5:9, 6:12] = 0.05  # sample 0: everything but a hole -> covers the borders -> the hole is the object
    mask[1, 4:10, 3:9] = 0.9   # sample 1: a central blob -> the blob is the object
    obj = np.zeros((2, 14, 18), bool)
    obj[0, 5:9, 6:12] = True
    obj[1, 4:10, 3:9] = True
    plain = flow_to_image(_dev(f)).cpu().numpy()
    out = flow_to_image(_dev(f), _dev(mask)).cpu().numpy()
    assert np.all(out[obj] == 127)
    assert np.array_equal(out[~obj], plain[~obj])


# ------------------------------------------------------------------------------------------------------- overlay_mask ----
def _taps(n_out, n_in):
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= n_in - 1
    f[lo | hi] = 0
    s[lo] = 0
    s[hi] = n_in - 1
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    c1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s, np.minimum(s + 1, n_in - 1), c0, c1


def _overlay_np(image, mask, oh, ow, threshold=0.1):
    """The definition in include/udet.h restated: postprocess_image, postprocess_mask of the disambiguated mask, addWeighted in
    float32 rounded half to even, OpenCV's 8-bit INTER_LINEAR."""
    h, w, _ = image.shape
    binm = mask[..., 0] > np.float32(threshold)
    border = binm[:2].sum() + binm[-2:].sum() + binm[:, :2].sum() + binm[:, -2:].sum()
    obj = ~binm if border / (4.0 * w + 4.0 * h) >= 0.6 else binm
    img = np.trunc(np.clip((image + np.float32(0.5)) * np.float32(255), 0, 255)).astype(np.float32)
    m = np.zeros((h, w, 3), np.float32)
    m[..., 1] = obj * np.float32(255)
    b = img * np.float32(0.5) + m * np.float32(0.4)
    assert b.dtype == np.float32
    blended = np.clip(np.rint(b), 0, 255).astype(np.int32)
    y0, y1, b0, b1 = _taps(oh, h)
    x0, x1, a0, a1 = _taps(ow, w)
    S = blended[:, x0] * a0[None, :, None] + blended[:, x1] * a1[None, :, None]
    r = (((b0[:, None, None] * (S[y0] >> 4)) >> 16) + ((b1[:, None, None] * (S[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(r, 0, 255).astype(np.uint8), blended


@pytest.mark.parametrize("hw,out_hw", [((7, 9), (13, 17)), ((6, 10), (6, 10)), ((192, 384), (384, 640))])
def test_overlay_mask(gpu, hw, out_hw):
    from unsupervised_detection_amd.visualize import overlay_mask
    h, w = hw
    rng = np.random.default_rng(7)
    # levels -20 .. 275: odd levels give the .5 ties of the 0.5 / 0.4 blend, the ends are clamped to 0 and 255
    level = rng.integers(-20, 276, (2, h, w, 3))
    image = ((level + 0.25) / 255.0 - 0.5).astype(np.float32)
    mask = np.full((2, h, w, 1), 0.05, np.float32)
    mask[0] = 0.9
    mask[0, h // 3:2 * h // 3, w // 3:2 * w // 3] = 0.0  # complemented (covers the borders)
    mask[1, h // 4:h // 2, w // 4:3 * w // 4] = 0.7      # kept
    out = overlay_mask(_dev(image), _dev(mask), out_hw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, out_hw[0], out_hw[1], 3)
    for i in range(2):
        ref, blended = _overlay_np(image[i], mask[i], *out_hw)
        # the inputs do exercise what they are meant to: clamps at both ends, ties, both mask polarities
        pi = np.clip(level[i], 0, 255)
        assert (level[i] < 0).any() and (level[i] > 255).any() and (pi % 2 == 1).any()
        assert np.array_equal(blended[..., 0], np.rint(pi[..., 0] * 0.5).astype(np.int32))
        assert 0 < (blended[..., 1] > np.rint(pi[..., 1] * 0.5)).sum() < h * w
        assert torch.equal(out[i].cpu(), torch.from_numpy(ref)), (hw, i)
        if hw == out_hw:
            assert np.array_equal(ref, blended.astype(np.uint8))  # identity resize


# ----------------------------------------------------------------------------------------------------- grad_histogram ----
def test_grad_histogram(gpu):
    from unsupervised_detection_amd.visualize import bucket_limits, segment_histograms
    lim = bucket_limits()
    lens = [1, 63, 64, 1000, 70001]
    off = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(off[-1]) * 1e-3).astype(np.float32)
    x[0] = np.float32(1e-40)                       # a float32 subnormal, alone in its segment
    x[off[1] + 5] = 0.0
    x[off[3] + 17:off[3] + 21] = 0.0               # planted exact zeros
    x[off[3] + 30], x[off[3] + 31] = 0.2, -0.2
    x[off[3] + 40] = np.inf                        # no limit above it: last bucket
    x[off[4] + 5], x[off[4] + 60000] = 0.2, -0.2
    x[off[4] + 100] = np.float32(lim[776 + 100])   # float32 roundings of three limits: the comparison must be made in double
    x[off[4] + 101] = np.float32(lim[776 + 250])
    x[off[4] + 102] = np.float32(lim[775 - 200])
    assert 0 < x[0] < np.finfo(np.float32).tiny
    g = _dev(x)
    stats, counts = segment_histograms(g, off)
    stats2, counts2 = segment_histograms(g, off)
    assert stats.shape == (5, 5) and counts.shape == (5, 1551) and counts.dtype == np.uint32
    assert np.array_equal(counts, counts2) and stats.tobytes() == stats2.tobytes()  # identical across two calls
    for s in range(5):
        seg = x[off[s]:off[s + 1]].astype(np.float64)
        idx = np.minimum(np.searchsorted(lim, seg, side="right"), 1550)  # (+inf: searchsorted says 1551, the last bucket is 1550)
        assert np.array_equal(counts[s], np.bincount(idx, minlength=1551)), s
        assert stats[s, 0] == seg.min() and stats[s, 1] == seg.max() and stats[s, 2] == len(seg)
        for k, want in ((3, seg.sum()), (4, (seg * seg).sum())):
            print("segment", s, "stat", k, stats[s, k], want)
            if np.isinf(want):
                assert stats[s, k] == want
            else:
                assert abs(stats[s, k] - want) <= 1e-12 * abs(want)
    assert counts[0, 776] == 1 and stats[0, 3] == np.float64(np.float32(1e-40))


def test_grad_histograms_by_variable(gpu):
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd.visualize import grad_histograms
    g = torch.randn(W.param_total(W.NET_GEN), generator=torch.Generator().manual_seed(9)) * 1e-2
    h = grad_histograms(g.cuda(), W.NET_GEN)
    tab = W.param_table(W.NET_GEN)
    assert list(h) == [n for n, _, _ in tab]
    for n, shape, o in tab[:3] + tab[-2:]:
        cnt = int(np.prod(shape))
        st, c = h[n]
        seg = g[o:o + cnt].numpy().astype(np.float64)
        assert st[2] == cnt and int(c.sum()) == cnt and st[0] == seg.min() and st[1] == seg.max()
    with pytest.raises(ValueError):
        grad_histograms(g[:-1].cuda(), W.NET_GEN)


# ------------------------------------------------------------------------------------------------------------ training ----
class _Src:
    def __init__(self, batch, n, hw=(128, 192)):
        self.batch, self.n, self.hw = batch, n, hw

    def __iter__(self):
        g = torch.Generator().manual_seed(1)
        for i in range(self.n):
            a = torch.rand(self.batch, *self.hw, 3, generator=g) - 0.5
            b = torch.rand(self.batch, *self.hw, 3, generator=g) - 0.5
            yield {"img1": a.cuda(), "img2": b.cuda(), "gt_mask": None, "fname": [b"f%d" % (i * self.batch + j) for j in range(self.batch)]}


def _cfg(**kw):
    from unsupervised_detection_amd.config import default_flags
    c = default_flags()
    c.img_height, c.img_width, c.batch_size = 64, 128, 2
    c.synthetic, c.autotune = True, False
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _small_engine(monkeypatch):
    from unsupervised_detection_amd import learner as Lr
    monkeypatch.setattr(Lr, "_engine_config", lambda config, batch=None, in_hw=(128, 192): Lr.EngineConfig(
        batch_size=batch or config.batch_size, in_height=128, in_width=192, img_height=config.img_height, img_width=config.img_width))
    return Lr


def test_training_summaries_do_not_disturb_the_run(gpu, monkeypatch, tmp_path):
    from PIL import Image
    from unsupervised_detection_amd import weights as W
    Lr = _small_engine(monkeypatch)
    final = []
    for summary_dir in ("", str(tmp_path / "sum")):
        lr = Lr.AdversarialLearner()
        lr.train(_cfg(data_source=_Src(2, 12), num_samples_train=24, max_epochs=1, summary_freq=4, summary_dir=summary_dir))
        assert lr.engine.adam_step == 12
        final.append((lr.state.w_gen.clone(), lr.state.w_rec.clone()))
    assert torch.equal(final[0][0], final[1][0]) and torch.equal(final[0][1], final[1][1])
    d = tmp_path / "sum"
    lines = [json.loads(l) for l in (d / "scalars.jsonl").read_text().splitlines()]
    assert [l["step"] for l in lines] == [4, 8, 12]
    assert len(lines[0]) == 9 and all(np.isfinite(v) for v in lines[-1].values())
    tags = ("input_image", "next_image", "PWC_Flow", "masked_flow", "Rec_flow", "Rec_flow_compl")
    assert sorted(os.listdir(d / "images")) == sorted("step_%08d_%s.png" % (s, t) for s in (4, 8, 12) for t in tags)
    for name in os.listdir(d / "images"):
        with Image.open(d / "images" / name) as im:
            assert im.size == (128, 64) and im.mode == "RGB"
    # steps 4, 8, 12 of the 1 recover + 3 generator schedule train the recover network
    assert sorted(os.listdir(d / "histograms")) == ["step_%08d_recover.npz" % s for s in (4, 8, 12)]
    z = np.load(d / "histograms" / "step_00000012_recover.npz")
    tab = W.param_table(W.NET_REC)
    assert list(z["names"]) == [n for n, _, _ in tab]
    assert np.array_equal(z["stats"][:, 2], [float(np.prod(s)) for _, s, _ in tab])
    assert np.array_equal(z["counts"].sum(1), z["stats"][:, 2])
    assert z["stats"][:, 1].max() <= np.float32(0.2) and z["stats"][:, 0].min() >= -np.float32(0.2)  # the clipped gradient udet_apply left


def test_cli_test_generator_writes_visualisation(gpu, monkeypatch, tmp_path):
    import scipy.io as sio
    from PIL import Image
    from unsupervised_detection_amd import cli
    Lr = _small_engine(monkeypatch)
    monkeypatch.setattr(Lr._data, "synthetic_davis_pairs", lambda b, seed, h=128, w=192, max_disp=8.0:
                        tuple(np.random.default_rng(seed + k).integers(0, 255, (b, 128, 192, 3), dtype=np.uint8) for k in (0, 1)))
    monkeypatch.setattr(Lr._data, "READER_H", 128)
    monkeypatch.setattr(Lr._data, "READER_W", 192)
    monkeypatch.setattr(Lr._data, "preprocess_image", lambda f, out_h=128, out_w=192: Lr._data.crop_flip_resize(f, 128, 192, None, False, 255.0, -0.5))
    common = ["test_generator", "--img_height", "64", "--img_width", "128", "--batch_size", "2", "--root_dir", "/nonexistent",
              "--synthetic"]
    off, on = tmp_path / "off", tmp_path / "on"
    off.mkdir()
    on.mkdir()
    assert cli.main(common + ["--test_save_dir", str(off)]) == 0
    assert os.listdir(off) == []
    assert cli.main(common + ["--generate_visualization", "--test_save_dir", str(on)]) == 0
    (cat,) = os.listdir(on)
    files = sorted(os.listdir(on / cat))
    assert files == sorted(["frame_%08d.png" % k for k in range(1, 9)] + ["result_%d.mat" % k for k in range(1, 9)])
    with Image.open(on / cat / "frame_00000001.png") as im:
        assert np.asarray(im).shape == (384, 640, 3)
    m = sio.loadmat(str(on / cat / "result_8.mat"))
    assert {"flow", "img1", "pred_mask", "gt_mask"} <= set(m)
    assert m["flow"].shape == (64, 128, 2) and m["img1"].shape == (64, 128, 3) and m["img1"].dtype == np.uint8
    assert m["pred_mask"].shape[:2] == (64, 128) and m["gt_mask"].shape[:2] == (64, 128)  # (.mat drops a trailing unit axis)
