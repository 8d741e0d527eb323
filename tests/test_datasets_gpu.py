"""GPU: the ragged input stage (udet_crop_flip_resize_ragged) bit for bit against crop_flip_resize on each sample alone and
against the numpy oracle; the FBMS-59 / SegTrackV2 readers on mixed-resolution trees against the image-by-image path; the
learner's inference, evaluation and training on both trees."""

import numpy as np
import pytest
import torch

from oracle import oracle_np as ON
from test_datasets import FBMS_SPEC, make_fbms, make_segtrack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


# one pixel tall, an odd size, 720p, an upsampled small one, a tall narrow one
SIZES = [(1, 45), (259, 327), (720, 1280), (20, 30), (97, 13)]


def _pack(arrays):
    off = np.cumsum([0] + [a.size for a in arrays])[:-1].astype(np.int64)
    hw = np.array([a.shape[:2] for a in arrays], np.int32)
    return np.concatenate([a.reshape(-1) for a in arrays]), off, hw


def _windows(rng, sizes, flips):
    out = []
    for h, w in sizes:
        ch, cw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        out.append([int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1)), ch, cw] +
                   ([int(rng.integers(0, 2)), int(rng.integers(0, 2))] if flips else [0, 0]))
    return np.array(out, np.int32)


def _oracle(x, prm, oh, ow, nearest, div, add):
    """Per-sample restatement with oracle_np: convert each value, flip, crop window, legacy resize."""
    v = x.astype(np.float32)
    if div != 1.0:
        v = v / np.float32(div)
    v = (v + np.float32(add))[None]
    if prm is not None:
        y0, x0, ch, cw, flr, ftd = (int(t) for t in prm)
        if ftd:
            v = v[:, ::-1]
        if flr:
            v = v[:, :, ::-1]
        v = np.ascontiguousarray(v[:, y0:y0 + ch, x0:x0 + cw])
    return (ON.resize_nearest_legacy(v, oh, ow) if nearest else ON.resize_bilinear_legacy(v, oh, ow))[0]


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("with_params", [False, True])
def test_ragged_kernel_matches_single_sample_path(gpu, u8, nearest, c, with_params):
    from unsupervised_detection_amd import data
    rng = np.random.default_rng(11 + 8 * u8 + 4 * nearest + 2 * c + with_params)
    arrays = [(rng.random((h, w, c)) * 255).astype(np.uint8) if u8 else (rng.standard_normal((h, w, c))).astype(np.float32)
              for h, w in SIZES]
    div, add = (255.0, -0.5) if u8 else (1.0, 0.0)
    prm = _windows(rng, SIZES, True) if with_params else None
    oh, ow = 48, 80
    flat, off, hw = _pack(arrays)
    out = data.crop_flip_resize_ragged(torch.from_numpy(flat).cuda(), off, hw, c, oh, ow, prm, nearest, div, add)
    assert out.shape == (len(SIZES), oh, ow, c)
    for i, a in enumerate(arrays):
        single = data.crop_flip_resize(torch.from_numpy(a[None]).cuda(), oh, ow, None if prm is None else prm[i:i + 1], nearest, div, add)
        assert torch.equal(out[i], single[0]), (i, a.shape)
        assert np.array_equal(out[i].cpu().numpy(), _oracle(a, None if prm is None else prm[i], oh, ow, nearest, div, add)), i


def test_ragged_kernel_full_reader_size_and_single_sample(gpu):
    from unsupervised_detection_amd import data
    rng = np.random.default_rng(5)
    arrays = [(rng.random((h, w, 3)) * 255).astype(np.uint8) for h, w in SIZES]
    flat, off, hw = _pack(arrays)
    out = data.crop_flip_resize_ragged(torch.from_numpy(flat).cuda(), off, hw, 3, 384, 640, None, False, 255.0, -0.5)
    for i, a in enumerate(arrays):
        assert torch.equal(out[i], data.preprocess_image(torch.from_numpy(a[None]).cuda())[0]), i
    # n = 1, with flips
    prm = np.array([[3, 5, 200, 301, 1, 1]], np.int32)
    one = data.crop_flip_resize_ragged(torch.from_numpy(arrays[1].reshape(-1)).cuda(), [0], [arrays[1].shape[:2]], 3, 64, 96, prm)
    assert torch.equal(one[0], data.crop_flip_resize(torch.from_numpy(arrays[1][None]).cuda(), 64, 96, prm)[0])


def test_ragged_entry_point_rejects_bad_scalar_arguments(gpu):
    from unsupervised_detection_amd import _ffi
    lib = _ffi.lib
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(64, dtype=torch.float32, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    hw = torch.ones(2, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda **kw: lib.udet_crop_flip_resize_ragged(
        kw.get("src", src.data_ptr()), 1, 0, kw.get("n", 1), kw.get("c", 1), kw.get("off", off.data_ptr()), kw.get("hw", hw.data_ptr()),
        None, kw.get("dst", dst.data_ptr()), kw.get("oh", 4), kw.get("ow", 4), 1.0, 0.0, s)
    assert call() == 0
    torch.cuda.synchronize()
    assert dst[:16].eq(0).all()
    for bad in ({"n": 0}, {"c": 0}, {"oh": 0}, {"ow": -1}, {"src": None}, {"dst": None}, {"off": None}, {"hw": None}):
        assert call(**bad) == -5, bad  # UDET_ERR_ARG
        assert b"crop_flip_resize_ragged" in lib.udet_last_error()


# ---------------------------------------------------------------------------------------------------------------- readers ----

def _single(path, channels, loader=None):
    from unsupervised_detection_amd import data
    a = (loader or data._read_image)(path, channels)
    return torch.from_numpy(np.array(a[None])).cuda()


def _replay_train(filenames, table, lo, hi, loader, seed, batch, crop, n_batches):
    """The reader's draws replayed with the per-sample path: decode -> preprocess_image -> augment_pair."""
    from unsupervised_detection_amd import data
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(table))
    out = []
    for k in range(n_batches):
        rows = table[order[k * batch:(k + 1) * batch]]
        shift = rng.integers(lo, hi + 1, len(rows))
        i1 = rows[:, 0].astype(np.int32)
        i2 = (shift.astype(np.float32) * rows[:, 1] + rows[:, 0]).astype(np.int32)
        a = torch.cat([data.preprocess_image(_single(f, 3, loader)) for f in filenames[i1]])
        b = torch.cat([data.preprocess_image(_single(f, 3, loader)) for f in filenames[i2]])
        out.append(data.augment_pair(a, b, crop, rng) + ([f.encode() for f in filenames[i1]],))
    return out


def test_fbms_reader_matches_the_per_sample_path(gpu, tmp_path, capsys):
    from unsupervised_detection_amd import data, datasets as D
    root = make_fbms(str(tmp_path / "FBMS"))
    rd = D.FBMS59Reader(root, seed=3)
    src = rd.image_inputs(batch_size=3, partition="trainval", train_crop=0.8)
    got = [next(src) for _ in range(2)]  # two consecutive batches through one reader: the staging slots are reused
    fl, _ = rd.get_filenames_list("trainval")
    assert len({tuple(a.shape[:2]) for a in (data._read_image(s[0], 3) for s in fl)}) >= 3  # mixed resolutions
    table = data.pair_table([len(f) for f in fl], 3, True)
    ref = _replay_train(np.concatenate(fl), table, 2, 3, None, 3, 3, 0.8, 2)
    for g, (a, b, names) in zip(got, ref):
        assert g["img1"].shape == (3, 384, 640, 3) and g["fname"] == names
        assert torch.equal(g["img1"], a) and torch.equal(g["img2"], b)

    tuples = rd.get_test_tuples("val", 1)
    batches = list(rd.test_inputs(batch_size=4, partition="val", t_len=1, test_crop=0.9))
    assert [len(b["fname"]) for b in batches] == [4, 4, 2]
    for s, batch in zip(range(0, len(tuples), 4), batches):
        rows = tuples[s:s + 4]
        a = torch.cat([data.central_cropping(data.preprocess_image(_single(r[0], 3)), 0.9) for r in rows])
        b = torch.cat([data.central_cropping(data.preprocess_image(_single(r[1], 3)), 0.9) for r in rows])
        g = torch.cat([data.central_cropping(data.preprocess_mask(_single(r[2], 1, rd.gt_loader)), 0.9) for r in rows])
        assert torch.equal(batch["img1"], a) and torch.equal(batch["img2"], b) and torch.equal(batch["gt_mask"], g)
        assert batch["fname"] == [r[0].encode() for r in rows]
        assert batch["samples_per_cat"].tolist() == [float(r[3]) for r in rows]
    assert float(batches[0]["gt_mask"].min()) >= 0 and float(batches[0]["gt_mask"].max()) <= 1

    crops = [0.85, 0.9, 0.95, 1.0]
    aug = list(rd.augmented_inputs(partition="val", t_len=1, test_crops=crops))
    assert len(aug) == len(tuples)
    d, fname = aug[0]
    assert fname == tuples[0][0].encode() and all(set(d[k]) == set(crops) for k in ("img_1s", "img_2s", "seg_1s"))
    first = next(iter(rd.test_inputs(batch_size=1, partition="val", t_len=1, test_crop=1.0)))
    assert torch.equal(d["img_1s"][1.0], first["img1"][0]) and torch.equal(d["seg_1s"][0.85], data.central_cropping(first["gt_mask"], 0.85)[0])
    assert d["img_2s"][0.9].shape == (384, 640, 3) and d["seg_1s"][0.9].shape == (384, 640, 1)


def test_segtrack_reader_matches_the_per_sample_path(gpu, tmp_path, capsys):
    from unsupervised_detection_amd import data, datasets as D
    root = make_segtrack(str(tmp_path / "segtrack"))
    rd = D.SegTrackV2Reader(root, seed=4)
    src = rd.image_inputs(batch_size=4, train_crop=0.9)
    got = [next(src) for _ in range(2)]
    fl, al = rd.get_filenames_list()
    table = data.pair_table([len(f) for f in fl], 3, True)
    ref = _replay_train(np.concatenate(fl), table, 2, 3, D.read_decode_jpeg, 4, 4, 0.9, 2)
    for g, (a, b, names) in zip(got, ref):
        assert g["fname"] == names and torch.equal(g["img1"], a) and torch.equal(g["img2"], b)

    files, anns = np.concatenate(fl), np.concatenate(al)
    table = data.pair_table([len(f) for f in fl], 2, False)
    batches = list(rd.test_inputs(batch_size=5, t_len=2, test_crop=0.85))
    assert sum(len(b["fname"]) for b in batches) == len(files) == 18
    for s, batch in zip(range(0, len(table), 5), batches):
        rows = table[s:s + 5]
        i1 = rows[:, 0].astype(np.int32)
        i2 = (np.float32(2) * rows[:, 1] + rows[:, 0]).astype(np.int32)
        a = torch.cat([data.central_cropping(data.preprocess_image(_single(files[i], 3, D.read_decode_jpeg)), 0.85) for i in i1])
        b = torch.cat([data.central_cropping(data.preprocess_image(_single(files[i], 3, D.read_decode_jpeg)), 0.85) for i in i2])
        g = torch.cat([data.central_cropping(data.preprocess_mask(_single(anns[i], 1, D.read_decode_jpeg)), 0.85) for i in i1])
        assert torch.equal(batch["img1"], a) and torch.equal(batch["img2"], b) and torch.equal(batch["gt_mask"], g)
    d, fname = next(rd.augmented_inputs(t_len=2, test_crops=[0.85, 0.9, 0.95, 1.0]))
    assert len(d["img_1s"]) == 4 and d["seg_1s"][0.95].shape == (384, 640, 1) and fname == files[0].encode()


# ------------------------------------------------------------------------------------------------------------- end to end ----

def _small_engine(monkeypatch):
    """The engine-size monkeypatches of tests/test_learner_gpu.py: 128 x 192 reader frames, a 64 x 128 working size."""
    from unsupervised_detection_amd import learner as Lr
    monkeypatch.setattr(Lr, "_engine_config", lambda config, batch=None, in_hw=(128, 192): Lr.EngineConfig(
        batch_size=batch or config.batch_size, in_height=128, in_width=192, img_height=config.img_height, img_width=config.img_width))
    monkeypatch.setattr(Lr._data, "READER_H", 128)
    monkeypatch.setattr(Lr._data, "READER_W", 192)
    return Lr


def _flags(dataset, root, **kw):
    from unsupervised_detection_amd.config import default_flags
    c = default_flags()
    c.dataset, c.root_dir = dataset, root
    c.img_height, c.img_width, c.batch_size = 64, 128, 2
    c.synthetic = True  # seeded random weights (no checkpoint); the data come from the reader
    c.autotune = False
    c.test_partition, c.test_temporal_shift, c.test_crop = "val", 1, 0.9
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("dataset", ["FBMS", "SEGTRACK"])
def test_inference_evaluation_and_training_on_mixed_trees(gpu, tmp_path, monkeypatch, capsys, dataset):
    from unsupervised_detection_amd import cli, evaluation
    Lr = _small_engine(monkeypatch)
    if dataset == "FBMS":
        root = make_fbms(str(tmp_path / "FBMS59"))
        names = {n for n, *_ in FBMS_SPEC["Testset"]}
        frames = 10
    else:
        root = make_segtrack(str(tmp_path / "SegTrackv2"))
        names = {"birdfall", "worm", "frog", "drift"}
        frames = 18

    cfg = _flags(dataset, root)
    cli.dataset_sources(cfg, "test")
    assert cfg.data_source[0]["img1"].shape == (2, 128, 192, 3)
    lr = Lr.AdversarialLearner()
    lr.setup_inference(cfg, aug_test=False)
    res = evaluation.evaluate_masks(lr, verbose=False)
    assert set(res["category_iou"]) == names and res["frames"] == frames
    assert all(0.0 <= v <= 1.0 for v in res["category_iou"].values())

    cfg = _flags(dataset, root)
    cli.dataset_sources(cfg, "ensemble")
    lr = Lr.AdversarialLearner()
    lr.setup_inference(cfg, aug_test=True)
    res = evaluation.evaluate_ensemble(lr, verbose=False)
    assert set(res["category_iou"]) == names and res["frames"] == frames

    cfg = _flags(dataset, root, num_samples_train=6, max_epochs=1, summary_freq=1)
    cli.dataset_sources(cfg, "train")
    lr = Lr.AdversarialLearner()
    lr.train(cfg)
    out = capsys.readouterr().out
    assert "Training completed successfully" in out and "Validation IoU" in out
    assert lr.engine.adam_step == 3 and all(np.isfinite(v) for v in lr.engine.losses().values())
