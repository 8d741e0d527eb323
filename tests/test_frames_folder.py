"""CPU: a plain folder of frames without annotations -- datasets.FrameFolderReader (natural order, layouts, pair tables, errors,
shards), the annotation-free mode of native_results.restore_results_dir on the numpy stand-ins of test_native_results.py, the
--dataset FRAMES / --overlay arguments and the new symbol."""
import json
import os
import re

import numpy as np
import pytest
import torch

from test_native_results import SEQS, davis_flags, load_gt_np, make_davis_tree, restore_np, score_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_frames(d, names, hw=(12, 16), seed=0):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    for n in names:
        path = os.path.join(d, n)
        if n.lower().endswith((".jpg", ".jpeg", ".png", ".bmp")):
            Image.fromarray(rng.integers(0, 255, hw + (3,), dtype=np.uint8), "RGB").save(path)
        else:
            with open(path, "w") as f:
                f.write("not a frame\n")


def frames_flags(root, **kw):
    from unsupervised_detection_amd.config import default_flags
    flags = default_flags()
    flags.root_dir, flags.dataset = root, "FRAMES"
    for k, v in kw.items():
        setattr(flags, k, v)
    return flags


# ----------------------------------------------------------------------------------------------------------------- reader ----
def test_natural_order_is_a_pure_function():
    from unsupervised_detection_amd.datasets import frame_files, natural_key
    names = ["f10.png", "f2.png", "f1.jpg", "F3.PNG", ".hidden.png", "notes.txt"]
    # digits as integers, the rest as plain strings ("F" < "f"); dot-files and other files ignored; any case of the extension
    assert frame_files(names) == ["F3.PNG", "f1.jpg", "f2.png", "f10.png"]
    assert names == ["f10.png", "f2.png", "f1.jpg", "F3.PNG", ".hidden.png", "notes.txt"]
    assert sorted(["frame_10", "frame_2", "frame_02", "frame_1"], key=natural_key) == ["frame_1", "frame_02", "frame_2", "frame_10"]
    assert sorted(["a2b10.bmp", "a2b9.bmp", "a10b1.bmp", "b.JPEG", "7.jpeg"], key=natural_key) == ["7.jpeg", "a2b9.bmp", "a2b10.bmp", "a10b1.bmp", "b.JPEG"]
    assert frame_files(["x.gif", "x.txt", "x.png.bak"]) == []


def test_layouts(tmp_path, capsys):
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.datasets import FrameFolderReader, frame_folder_sequences
    from unsupervised_detection_amd.native_results import frame_lists_from_reader
    # sub-directories: every one that holds images is a sequence, by name; others are ignored
    root = str(tmp_path / "clips")
    write_frames(os.path.join(root, "walk"), ["w_10.jpg", "w_9.jpg", "w_11.jpg", "readme.txt"])
    write_frames(os.path.join(root, "dog"), ["2.png", "1.png", "10.png", ".1.png"])
    write_frames(os.path.join(root, "notes"), ["a.txt"])
    write_frames(os.path.join(root, ".cache"), ["1.png", "2.png"])
    write_frames(root, ["stray.png"])  # sub-directories hold images: the root's own are not a sequence
    seqs = frame_folder_sequences(root)
    assert [n for n, _ in seqs] == ["dog", "walk"]
    assert [os.path.basename(f) for f in seqs[0][1]] == ["1.png", "2.png", "10.png"]
    assert [os.path.basename(f) for f in seqs[1][1]] == ["w_9.jpg", "w_10.jpg", "w_11.jpg"]
    rd = cli._reader(frames_flags(root), 0, 1)
    assert isinstance(rd, FrameFolderReader)
    imgs, anns = rd.get_filenames_list()
    assert [len(s) for s in imgs] == [3, 3] and anns == [[None] * 3, [None] * 3] and rd.val_samples == 6
    lists = frame_lists_from_reader(frames_flags(root))
    assert list(lists) == ["dog", "walk"] and all(a is None for v in lists.values() for _, a in v)
    assert [os.path.basename(i) for i, _ in lists["walk"]] == ["w_9.jpg", "w_10.jpg", "w_11.jpg"]
    assert all(i.split("/")[-2] == c for c, v in lists.items() for i, _ in v)  # the category evaluate_masks derives from fname
    # the frames in the root itself: one sequence named after it (also through a relative path)
    flat = str(tmp_path / "myvideo")
    write_frames(flat, ["frame2.bmp", "frame1.bmp", "frame10.bmp"])
    os.makedirs(os.path.join(flat, "empty"))
    seqs = frame_folder_sequences(flat + "/")
    assert [n for n, _ in seqs] == ["myvideo"] and [os.path.basename(f) for f in seqs[0][1]] == ["frame1.bmp", "frame2.bmp", "frame10.bmp"]
    cwd = os.getcwd()
    os.chdir(flat)
    try:
        lists = frame_lists_from_reader(frames_flags("."))
    finally:
        os.chdir(cwd)
    assert list(lists) == ["myvideo"] and len(lists["myvideo"]) == 3 and lists["myvideo"][0][0].split("/")[-2] == "myvideo"


def test_pair_tables_of_a_short_sequence(tmp_path, monkeypatch, capsys):
    from unsupervised_detection_amd import data
    from unsupervised_detection_amd import datasets as D
    want = [[0, 1], [1, -1], [2, -1]]
    assert data.pair_table([3], 2, False).tolist() == want and data.pair_table([3], -1, False).tolist() == want
    root = str(tmp_path / "v")
    write_frames(os.path.join(root, "a"), ["0.png", "1.png", "2.png"])
    write_frames(os.path.join(root, "b"), ["0.png", "1.png", "2.png", "3.png"])
    seen = []

    def pairs(self, p1, p2):
        seen.append(([os.path.relpath(p, root) for p in p1], [os.path.relpath(p, root) for p in p2]))
        return torch.zeros(len(p1), 1, 1, 3), torch.zeros(len(p2), 1, 1, 3)
    monkeypatch.setattr(D._RaggedReader, "_image_pairs", pairs)
    rd = D.FrameFolderReader(root, 2, 1)
    batches = list(rd.test_inputs(batch_size=4, t_len=2, with_fname=True, test_crop=1.0))
    assert [len(b["fname"]) for b in batches] == [4, 3] and all(b["gt_mask"] is None for b in batches)
    first = sum((s[0] for s in seen), [])
    second = sum((s[1] for s in seen), [])
    # pair_table([3, 4], 2, False): the +2 rows of both sequences, then the -2 rows; a's middle frame has neither neighbour: clamped into a
    assert first == ["a/0.png", "b/0.png", "b/1.png", "a/1.png", "a/2.png", "b/2.png", "b/3.png"]
    assert second == ["a/2.png", "b/2.png", "b/3.png", "a/0.png", "a/0.png", "b/0.png", "b/1.png"]
    assert [f.decode() for b in batches for f in b["fname"]] == [os.path.join(root, f) for f in first]
    del seen[:]
    list(rd.test_inputs(batch_size=7, t_len=-1))
    assert seen[0][0] == ["a/0.png", "b/0.png", "a/1.png", "a/2.png", "b/1.png", "b/2.png", "b/3.png"]
    assert seen[0][1] == ["a/1.png", "b/1.png", "a/0.png", "a/1.png", "b/0.png", "b/1.png", "b/2.png"]
    # augmented_inputs: per frame, seg_1s[crop] is None
    d, fname = next(iter(rd.augmented_inputs(t_len=1, test_crops=(1.0,))))
    assert d["seg_1s"] == {1.0: None} and tuple(d["img_1s"][1.0].shape) == (1, 1, 3) and fname.decode().endswith("a/0.png")


def test_reader_errors(tmp_path, capsys):
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.datasets import FrameFolderReader
    root = str(tmp_path / "v")
    write_frames(os.path.join(root, "long"), ["0.png", "1.png", "2.png", "3.png"])
    write_frames(os.path.join(root, "short"), ["0.png", "1.png"])
    rd = FrameFolderReader(root, 2, 1)
    with pytest.raises(IOError, match="'short'.*2 frame.*3 are needed"):
        rd.test_inputs(t_len=2)
    with pytest.raises(IOError, match="'short'"):
        rd.test_inputs(t_len=-2)
    with pytest.raises(IOError, match="'short'"):
        rd.image_inputs(batch_size=2)  # training needs max_temporal_len + 1
    rd.test_inputs(t_len=1), rd.test_inputs(t_len=-1)  # |t_len| + 1 = 2 frames are enough
    empty = str(tmp_path / "empty")
    write_frames(os.path.join(empty, "sub"), ["notes.txt"])
    with pytest.raises(IOError, match="FRAMES layout"):
        FrameFolderReader(empty, 2, 1).get_filenames_list()
    with pytest.raises(IOError, match="FRAMES layout"):
        cli._reader(frames_flags(str(tmp_path / "missing")), 0, 1)
    with pytest.raises(IOError, match="FRAMES"):
        cli._reader(frames_flags(root, dataset="KITTI"), 0, 1)  # the unsupported-dataset message names it


def test_two_shards_are_disjoint(tmp_path, monkeypatch, capsys):
    from unsupervised_detection_amd import data
    from unsupervised_detection_amd import datasets as D
    root = str(tmp_path / "v")
    write_frames(os.path.join(root, "a"), ["%d.png" % k for k in range(6)])
    write_frames(os.path.join(root, "b"), ["%d.png" % k for k in range(5)])
    monkeypatch.setattr(D._RaggedReader, "_image_pairs", lambda self, p1, p2: (torch.zeros(len(p1), 1, 1, 3), torch.zeros(len(p2), 1, 1, 3)))
    monkeypatch.setattr(data, "augment_pair", lambda a, b, crop, rng: (a, b))
    picked = []
    for rank in (0, 1):
        rd = D.FrameFolderReader(root, 2, 1, seed=7, shard=(rank, 2))
        src = rd.image_inputs(batch_size=2, train_crop=0.9)
        picked.append([next(src) for _ in range(3)])
    assert all(b["gt_mask"] is None for r in picked for b in r)
    files = np.concatenate(D.FrameFolderReader(root).get_filenames_list()[0])
    table = data.pair_table([6, 5], 2, True)
    assert len(table) == 14  # 3 global batches of 4 rows, the last two rows dropped
    order = np.random.default_rng(7).permutation(len(table))
    for k in range(3):
        a, b = picked[0][k]["fname"], picked[1][k]["fname"]
        rows = order[4 * k:4 * k + 4]  # rank 0 takes the first two rows of the global batch, rank 1 the other two: disjoint rows
        assert len(set(rows)) == 4 and a + b == [f.encode() for f in files[table[rows][:, 0].astype(np.int32)]]
    with pytest.raises(AssertionError):
        D.FrameFolderReader(root, 2, 1, shard=(0, 2))  # a sharded reader needs a seed


def test_dataset_sources(tmp_path, monkeypatch, capsys):
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd import datasets as D
    root = str(tmp_path / "v")
    write_frames(os.path.join(root, "a"), ["0.png", "1.png", "2.png"])
    monkeypatch.setattr(D._RaggedReader, "_image_pairs", lambda self, p1, p2: (torch.zeros(len(p1), 1, 1, 3), torch.zeros(len(p2), 1, 1, 3)))
    flags = frames_flags(root, batch_size=2, test_crop=1.0)
    flags.val_source = "untouched"
    cli.dataset_sources(flags, "train")
    assert flags.val_source is None and hasattr(flags.data_source, "__next__")  # no validation IoU, no model.best
    cli.dataset_sources(flags, "test")
    assert flags.data_source.n == 2 and [len(b["fname"]) for b in flags.data_source] == [2, 1]
    cli.dataset_sources(flags, "ensemble")
    assert flags.data_source.n == 3 and all(b["gt_mask"] is None for b in flags.data_source)


# ------------------------------------------------------------------------------------------- annotation-free restore ----
def raises(*a, **k):
    raise AssertionError("must not be called without annotations")


FRAME_HW = {("clip", 0): (37, 53), ("clip", 1): (20, 64), ("clip", 2): (37, 53), ("other", 0): (20, 64), ("other", 1): (20, 64)}


def make_frames_tree(tmp_path, mhw=(12, 24)):
    """Two sequences of frames (two sizes inside `clip`) and a results folder of mhw masks; returns (root, results, {seq: [mask]})."""
    import scipy.io as sio
    from PIL import Image
    root, res = str(tmp_path / "frames"), str(tmp_path / "results")
    rng = np.random.default_rng(3)
    masks = {}
    for (seq, k), (H, W) in sorted(FRAME_HW.items()):
        os.makedirs(os.path.join(root, seq), exist_ok=True)
        os.makedirs(os.path.join(res, seq), exist_ok=True)
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8), "RGB").save(os.path.join(root, seq, "f%d.png" % k))
        m = (0.2 * rng.random(mhw)).astype(np.float32)
        m[2 + k:9, 3 + 2 * k:13 + 2 * k] += 0.7
        masks.setdefault(seq, []).append(m)
        sio.savemat(os.path.join(res, seq, "result_%d.mat" % (k + 1)), {"pred_mask": m, "gt_mask": np.zeros(mhw, np.float32)})
    return root, res, masks


def test_annotation_free_restore(tmp_path, capsys):
    import scipy.io as sio
    from PIL import Image
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_frames_tree(tmp_path)
    lists = frame_lists_from_reader(frames_flags(root))
    assert {c: len(v) for c, v in lists.items()} == {"clip": 3, "other": 2}
    out = str(tmp_path / "native")
    got = restore_results_dir(res, lists, out, mask_key="pred_mask", restore=restore_np, load_gt=raises, score=raises, batch=2, verbose=False,
                              gt_rule="FRAMES")
    want_fg = {}
    for (seq, k), (H, W) in sorted(FRAME_HW.items()):
        want = restore_np(masks[seq][k][None], [(H, W)], 0.9, 0.5)
        with Image.open(os.path.join(out, seq, "f%d.png" % k)) as im:
            assert im.mode == "L" and im.size == (W, H)  # each frame's own size, read from its header
            png = np.asarray(im)
        assert png.any() and np.array_equal(png, want.binary_sample(0) * 255)
        mat = sio.loadmat(os.path.join(out, seq, "result_%d.mat" % (k + 1)))
        assert {n for n in mat if not n.startswith("__")} == {"mask", "soft_mask"}
        assert np.array_equal(mat["mask"], want.binary_sample(0)) and np.array_equal(mat["soft_mask"], want.soft(0).astype(np.float32))
        want_fg.setdefault(seq, []).append(int((png == 255).sum()) / (H * W))  # counted by hand from the written file
    assert sorted(os.listdir(os.path.join(out, "clip"))) == ["f0.png", "f1.png", "f2.png", "result_1.mat", "result_2.mat", "result_3.mat"]
    assert sorted(os.listdir(out)) == ["clip", "native_eval.json", "other"]  # no overlay folder without overlay=
    with open(os.path.join(out, "native_eval.json")) as f:
        js = json.load(f)
    assert js == json.loads(json.dumps(got)) and js["annotations"] is False
    assert not {"J", "F", "J&F", "category_iou", "sequence_iou"} & set(js)
    assert {"mask_key", "threshold", "crop", "sequences"} <= set(js) and "component" not in js
    for seq in ("clip", "other"):
        assert set(js["sequences"][seq]) == {"frames", "foreground_mean"} and js["sequences"][seq]["frames"] == len(want_fg[seq])
        assert js["sequences"][seq]["foreground_mean"] == float(np.mean(want_fg[seq])) and 0.0 < js["sequences"][seq]["foreground_mean"] < 1.0


def test_annotation_free_components_and_refusals(tmp_path, capsys):
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_frames_tree(tmp_path)
    lists = frame_lists_from_reader(frames_flags(root))
    kw = dict(mask_key="pred_mask", restore=restore_np, load_gt=raises, score=raises, verbose=False)
    seen = []

    class Selected(object):
        def __init__(self, pred):
            self.pred, self.info = pred, np.tile(np.array([[3, 0, 1, 0]], np.int64), (len(pred.hw), 1))

        def binary_sample(self, i):
            return self.pred.binary_sample(i)

    def select(pred, gt=None, mode="largest", connectivity=8):
        seen.append((gt, mode, connectivity))
        return Selected(pred)
    js = restore_results_dir(res, lists, str(tmp_path / "n1"), component="largest", connectivity=4, select=select, **kw)
    assert seen and all(s == (None, "largest", 4) for s in seen)
    assert js["component"] == "largest" and js["connectivity"] == 4 and js["annotations"] is False
    assert all(set(v) == {"frames", "foreground_mean", "components_mean"} and v["components_mean"] == 3.0 for v in js["sequences"].values())
    with pytest.raises(ValueError, match="best_gt"):
        restore_results_dir(res, lists, str(tmp_path / "n2"), component="best_gt", select=select, **kw)
    mixed = {"clip": [(lists["clip"][0][0], None), (lists["clip"][1][0], lists["clip"][1][0]), lists["clip"][2]], "other": lists["other"]}
    with pytest.raises(ValueError, match="mixes"):
        restore_results_dir(res, mixed, str(tmp_path / "n3"), **kw)
    with pytest.raises(ValueError, match="overlay"):
        restore_results_dir(res, lists, str(tmp_path / "n4"), overlay={"edge": 9}, **kw)
    with pytest.raises(ValueError, match="overlay"):
        restore_results_dir(res, lists, str(tmp_path / "n5"), overlay={"width": 2}, **kw)
    # injected sizes are what the frames are restored to
    sizes = []

    def load_sizes(paths):
        sizes.extend(paths)
        return [(10, 11)] * len(paths)
    restore_results_dir(res, {"other": lists["other"]}, str(tmp_path / "n6"), load_sizes=load_sizes, **kw)
    from PIL import Image
    with Image.open(os.path.join(str(tmp_path / "n6"), "other", "f1.png")) as im:
        assert im.size == (11, 10)
    assert sizes == [i for i, _ in lists["other"]]


def test_annotated_lists_write_what_they_wrote(tmp_path):
    """The same call with annotated lists: the files and the json of tests/test_native_results.py, key for key (no "annotations")."""
    import scipy.io as sio
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_davis_tree(tmp_path, mixed=True)
    lists = frame_lists_from_reader(davis_flags(root))
    out = str(tmp_path / "native")
    js = restore_results_dir(res, lists, out, restore=restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False, load_sizes=raises)
    assert list(js) == ["mask_key", "threshold", "crop", "bound_th", "skip_ends", "sequences", "J", "F", "J&F", "category_iou", "sequence_iou"]
    for seq in SEQS:
        assert sorted(os.listdir(os.path.join(out, seq))) == ["00000.png", "00001.png", "00002.png", "result_1.mat", "result_2.mat", "result_3.mat"]
        mat = sio.loadmat(os.path.join(out, seq, "result_1.mat"))
        assert [n for n in mat if not n.startswith("__")] == ["mask", "soft_mask", "gt_mask"]
    assert sorted(os.listdir(out)) == sorted(SEQS + ("native_eval.json",))


# -------------------------------------------------------------------------------------------------------------- arguments ----
def test_arguments():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--dataset", "FRAMES", "--root_dir", "V"]
    a = cli.parse_restore_results_args(base)
    assert a.dataset == "FRAMES" and a.overlay is False and cli._overlay(a) is None and cli._component(a) is None
    assert (a.overlay_edge, a.overlay_alpha, a.overlay_beta, a.overlay_colour, a.overlay_edge_colour) == (2, 0.5, 0.4, "0,255,0", "255,255,255")
    a = cli.parse_restore_results_args(base + ["--component", "largest", "--overlay"])
    assert cli._overlay(a) == {"alpha": 0.5, "beta": 0.4, "colour": (0, 255, 0), "edge": 2, "edge_colour": (255, 255, 255)}
    a = cli.parse_restore_results_args(base + ["--overlay", "--overlay_edge", "0", "--overlay_alpha", "0.7", "--overlay_beta", "0.25",
                                               "--overlay_colour", "255,0,10", "--overlay_edge_colour", "1,2,3"])
    assert cli._overlay(a) == {"alpha": 0.7, "beta": 0.25, "colour": (255, 0, 10), "edge": 0, "edge_colour": (1, 2, 3)}
    for bad in (["--overlay_edge", "9"], ["--overlay_colour", "green"], ["--overlay_colour", "0,300,0"], ["--overlay_alpha", "-1"],
                ["--overlay_edge_colour", "1,2"]):
        with pytest.raises(SystemExit):
            cli.parse_restore_results_args(base + ["--overlay"] + bad)
    # no annotations: best_gt cannot be honoured, whether asked for or the default
    with pytest.raises(SystemExit, match="largest"):
        cli.parse_restore_results_args(base + ["--component", "best_gt"])
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--dataset", "FRAMES", "--root_dir", "V"]
    with pytest.raises(SystemExit, match="largest"):
        cli.parse_post_process_args(pp + ["--benchmark"])  # --component defaults to best_gt there
    a = cli.parse_post_process_args(pp + ["--benchmark", "--component", "largest", "--overlay", "--overlay_edge", "3"])
    assert a.dataset == "FRAMES" and cli._component(a) == "largest" and cli._overlay(a)["edge"] == 3
    assert cli.parse_post_process_args(pp).dataset == "FRAMES"  # without --benchmark the component is not used
    # test_generator --native_resolution
    d = default_flags()
    assert (d.overlay, d.overlay_edge, d.overlay_alpha, d.overlay_beta, d.overlay_colour, d.overlay_edge_colour) == (False, 2, 0.5, 0.4, "0,255,0", "255,255,255")
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D", "--dataset", "FRAMES", "--root_dir", "V"]
    f = parse_flags(native + ["--component", "largest", "--overlay", "--overlay_edge", "1"])
    cli.check_native_flags(f)  # FRAMES goes through
    assert cli._overlay(f)["edge"] == 1
    with pytest.raises(SystemExit, match="largest"):
        cli.check_native_flags(parse_flags(native + ["--component", "best_gt"]))
    with pytest.raises(SystemExit):
        cli.check_native_flags(parse_flags(native + ["--overlay", "--overlay_edge", "12"]))
    # the defaults of the existing flags are what they were
    assert cli.parse_restore_results_args(["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]).dataset == "DAVIS2016"
    assert cli.parse_post_process_args(["--buffer_dir", "B", "--out_dir", "O"]).component == "best_gt"


def test_post_process_on_a_folder_of_frames(tmp_path, monkeypatch):
    """post_process --dataset FRAMES: "iou_resized": null, the overlay parameters reach the native-resolution pass."""
    from unsupervised_detection_amd import cli, native_results, post_processing as PP
    d = tmp_path / "buf" / "davis_shift_1" / "clip"
    d.mkdir(parents=True)
    (d / "result_1.mat").write_bytes(b"")
    seen = []
    monkeypatch.setattr(PP, "buffer_to_soft_score", lambda *a, **k: None)
    monkeypatch.setattr(PP, "run_crf", lambda *a, **k: np.float32(0.0) / np.float32(0.0))  # what an all-zero gt_mask gives; no warning
    monkeypatch.setattr(PP, "run_crf_original_resolution", lambda *a, **k: seen.append(k) or {"annotations": False})
    monkeypatch.setattr(native_results, "frame_lists_from_reader", lambda flags: {"clip": []})
    out = str(tmp_path / "out")
    args = ["post_process", "--buffer_dir", str(tmp_path / "buf"), "--out_dir", out, "--dataset", "FRAMES", "--root_dir", "V"]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert cli.main(args) == 0
    with open(os.path.join(out, "post_process.json")) as f:
        js = json.load(f)
    assert js["iou_resized"] is None and "benchmark" not in js
    with pytest.raises(SystemExit, match="largest"):
        cli.main(args + ["--benchmark"])
    assert cli.main(args + ["--benchmark", "--component", "largest", "--overlay", "--overlay_edge", "1"]) == 0
    assert seen == [{"out_path": os.path.join(out, "crf_original"), "component": "largest", "gt_rule": "FRAMES",
                     "overlay": {"alpha": 0.5, "beta": 0.4, "colour": (0, 255, 0), "edge": 1, "edge_colour": (255, 255, 255)}}]
    with open(os.path.join(out, "post_process.json")) as f:
        js = json.load(f)
    assert js["iou_resized"] is None and js["benchmark"] == {"annotations": False}


def test_overlay_parameters():
    from unsupervised_detection_amd.visualize import OVERLAY_MAX_EDGE, overlay_params
    assert overlay_params() == overlay_params({}) == {"alpha": 0.5, "beta": 0.4, "colour": (0, 255, 0), "edge": 2, "edge_colour": (255, 255, 255)}
    assert overlay_params({"edge": 8, "alpha": 0})["edge"] == OVERLAY_MAX_EDGE == 8
    for bad in ({"edge": 9}, {"edge": -1}, {"edge": 1.5}, {"alpha": float("nan")}, {"beta": float("inf")}, {"beta": -0.5}, {"colour": (0, 0)},
                {"edge_colour": (0, 0, 256)}, {"thickness": 2}, "green"):
        with pytest.raises(ValueError):
            overlay_params(bad)


def test_symbol_is_declared_exported_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) / UDET_ERR_UNSUPPORTED (-4) before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    assert re.search(r"#define UDET_OVERLAY_MAX_EDGE 8\b", hdr)
    assert re.search(r"\bint udet_overlay_native_ragged\(const unsigned char\* image_rgb, const unsigned char\* mask, int n,", hdr)
    assert hasattr(lib, "udet_overlay_native_ragged") and lib.udet_overlay_native_ragged.argtypes is not None
    ok = dict(image=64, mask=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=4000, alpha=0.5, beta=0.4, mask_rgb=0x00FF00, edge=2,
              edge_rgb=0xFFFFFF, out=128)

    def call(**change):
        a = dict(ok, **change)
        return lib.udet_overlay_native_ragged(a["image"], a["mask"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"],
                                              a["alpha"], a["beta"], a["mask_rgb"], a["edge"], a["edge_rgb"], a["out"], None)
    for change in (dict(n=0), dict(n=65536), dict(image=None), dict(mask=None), dict(offsets=None), dict(hw=None), dict(out=None),
                   dict(max_h=0), dict(max_w=0), dict(edge=-1), dict(alpha=-0.5), dict(alpha=float("nan")), dict(beta=float("inf")),
                   dict(beta=-1.0)):
        assert call(**change) == -5 and b"overlay_native_ragged" in lib.udet_last_error(), change
    assert call(edge=9) == -4 and b"overlay_native_ragged" in lib.udet_last_error()
