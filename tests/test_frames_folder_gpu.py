"""GPU: a plain folder of frames end to end -- datasets.FrameFolderReader against the image-by-image path, then the test pass with
seeded weights, the annotation-free native-resolution stage with CRF, component selection and overlays, one ensemble step and two
training steps without a validation source."""
import json
import os

import numpy as np
import pytest
import torch

from test_datasets_gpu import _flags, _replay_train, _single, _small_engine
from test_frames_folder import raises
from test_overlay_native_gpu import Packed

pytestmark = pytest.mark.gpu

# two sequences of different frame sizes, and one frame of a third size inside the first (a ragged batch)
HW = {"a": [(48, 64), (48, 64), (36, 52), (48, 64)], "b": [(60, 40)] * 4}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def make_tree(root):
    from PIL import Image
    rng = np.random.default_rng(21)
    for seq, sizes in HW.items():
        os.makedirs(os.path.join(root, seq))
        for k, (h, w) in enumerate(sizes):
            y, x = np.mgrid[:h, :w]
            img = rng.integers(0, 60, (h, w, 3)) + 90
            img[((y - h / 2 - k) / (h / 4)) ** 2 + ((x - w / 2 - 2 * k) / (w / 5)) ** 2 <= 1] += 100  # a moving blob
            Image.fromarray(img.astype(np.uint8), "RGB").save(os.path.join(root, seq, "frame_%d.png" % (k + 9)))  # 9, 10, 11, 12: natural order
    return root


def test_reader_matches_the_per_sample_path(gpu, tmp_path, capsys):
    from unsupervised_detection_amd import data, datasets as D
    root = make_tree(str(tmp_path / "clips"))
    rd = D.FrameFolderReader(root, 2, 1, seed=5)
    fl, anns = rd.get_filenames_list()
    assert [os.path.basename(f) for f in fl[0]] == ["frame_9.png", "frame_10.png", "frame_11.png", "frame_12.png"]
    files = np.concatenate(fl)
    table = data.pair_table([4, 4], 1, False)
    batches = list(rd.test_inputs(batch_size=3, t_len=1, with_fname=True, test_crop=0.9))
    assert [len(b["fname"]) for b in batches] == [3, 3, 2] and all(b["gt_mask"] is None for b in batches)
    for s, batch in zip(range(0, len(table), 3), batches):
        rows = table[s:s + 3]
        i1 = rows[:, 0].astype(np.int32)
        i2 = (np.float32(1) * rows[:, 1] + rows[:, 0]).astype(np.int32)
        a = torch.cat([data.central_cropping(data.preprocess_image(_single(files[i], 3)), 0.9) for i in i1])
        b = torch.cat([data.central_cropping(data.preprocess_image(_single(files[i], 3)), 0.9) for i in i2])
        assert batch["img1"].shape == (len(rows), 384, 640, 3)
        assert torch.equal(batch["img1"], a) and torch.equal(batch["img2"], b)
        assert batch["fname"] == [files[i].encode() for i in i1]
    src = rd.image_inputs(batch_size=3, train_crop=0.8)
    got = [next(src) for _ in range(2)]
    ref = _replay_train(files, data.pair_table([4, 4], 2, True), 1, 2, None, 5, 3, 0.8, 2)
    for g, (a, b, names) in zip(got, ref):
        assert g["fname"] == names and torch.equal(g["img1"], a) and torch.equal(g["img2"], b)
    d, fname = next(iter(rd.augmented_inputs(t_len=1, test_crops=[0.9, 1.0])))
    assert d["seg_1s"] == {0.9: None, 1.0: None} and d["img_1s"][0.9].shape == (384, 640, 3) and fname == files[0].encode()


def test_end_to_end_with_seeded_weights(gpu, tmp_path, monkeypatch, capsys):
    import scipy.io as sio
    from PIL import Image
    from unsupervised_detection_amd import cli, data, evaluation
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    from unsupervised_detection_amd.visualize import overlay_native
    Lr = _small_engine(monkeypatch)
    root = make_tree(str(tmp_path / "clips"))
    saved, native = str(tmp_path / "saved"), str(tmp_path / "saved" / "native")

    cfg = _flags("FRAMES", root)
    cli.dataset_sources(cfg, "test")
    assert cfg.data_source[0]["img1"].shape == (2, 128, 192, 3) and cfg.data_source[0]["gt_mask"] is None
    lr = Lr.AdversarialLearner()
    lr.setup_inference(cfg, aug_test=False)
    res = evaluation.evaluate_masks(lr, verbose=False, save_dir=saved)
    assert set(res["category_iou"]) == {"a", "b"} and res["frames"] == 8

    lists = frame_lists_from_reader(cfg)
    crf = {"sxy": 3.0, "srgb": 5.0, "compat": 5.0, "gauss_k": 0.1, "iters": 2, "radius": 4}
    js = restore_results_dir(saved, lists, native, mask_key="pred_mask", crop=cfg.test_crop, batch=3, component="largest", crf=crf,
                             overlay={}, load_gt=raises, score=raises, verbose=False, gt_rule="FRAMES")
    for seq, sizes in HW.items():
        stems = ["frame_%d" % (k + 9) for k in range(4)]
        assert sorted(os.listdir(os.path.join(native, seq))) == sorted([s + ".png" for s in stems] + ["result_%d.mat" % k for k in range(1, 5)])
        assert sorted(os.listdir(os.path.join(native, "overlay", seq))) == sorted(s + ".png" for s in stems)
        fg = []
        for k, (stem, (h, w)) in enumerate(zip(stems, sizes)):
            with Image.open(os.path.join(native, seq, stem + ".png")) as im:
                assert im.mode == "L" and im.size == (w, h)  # each frame's own size
                mask = np.array(im)
            assert set(np.unique(mask)) <= {0, 255}
            mat = sio.loadmat(os.path.join(native, seq, "result_%d.mat" % (k + 1)))
            assert {n for n in mat if not n.startswith("__")} == {"mask", "soft_mask"} and np.array_equal(mat["mask"] * 255, mask)
            fg.append(int((mask == 255).sum()) / (h * w))
            frame = data._read_image(os.path.join(root, seq, stem + ".png"), 3)
            with Image.open(os.path.join(native, "overlay", seq, stem + ".png")) as im:
                assert im.mode == "RGB" and im.size == (w, h)
                drawn = np.array(im)
            p = Packed([frame], [mask])
            assert np.array_equal(drawn, overlay_native(p.frames, p).sample(0).cpu().numpy()), (seq, stem)
        assert set(js["sequences"][seq]) == {"frames", "foreground_mean", "components_mean"} and js["sequences"][seq]["frames"] == 4
        assert js["sequences"][seq]["foreground_mean"] == float(np.mean(fg)) and js["sequences"][seq]["components_mean"] >= 0.0
    with open(os.path.join(native, "native_eval.json")) as f:
        assert json.load(f) == json.loads(json.dumps(js))
    assert js["annotations"] is False and js["component"] == "largest" and js["crf"]["iters"] == 2
    assert js["overlay"] == {"alpha": 0.5, "beta": 0.4, "colour": (0, 255, 0), "edge": 2, "edge_colour": (255, 255, 255)}
    assert not {"J", "F", "J&F", "category_iou", "sequence_iou"} & set(js)

    cfg = _flags("FRAMES", root)
    cli.dataset_sources(cfg, "ensemble")
    lr = Lr.AdversarialLearner()
    lr.setup_inference(cfg, aug_test=True)
    res = evaluation.evaluate_ensemble(lr, n_steps=1, verbose=False)
    assert res["frames"] == 1 and set(res["category_iou"]) == {"a"}

    cfg = _flags("FRAMES", root, num_samples_train=4, max_epochs=1, summary_freq=1)
    cli.dataset_sources(cfg, "train")
    assert cfg.val_source is None
    capsys.readouterr()
    lr = Lr.AdversarialLearner()
    lr.train(cfg)
    out = capsys.readouterr().out
    assert "Training completed successfully" in out and "Validation IoU" not in out
    assert lr.engine.adam_step == 2 and all(np.isfinite(v) for v in lr.engine.losses().values())
