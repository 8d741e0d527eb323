"""FBMS-59 / SegTrackV2 readers (datasets.py) and the ragged wrapper's host checks, on CPU: directory layouts, test tuples,
ground-truth conversion, PNG decoding, shard selection.  The trees are tiny synthetic ones written with Pillow; the builders
are shared with tests/test_datasets_gpu.py."""
import os

import numpy as np
import pytest
import torch

from unsupervised_detection_amd import data, datasets as D

# (sequence, frame count, frame size, GT naming rule, annotated frame numbers) per FBMS partition directory
FBMS_SPEC = {
    "Trainingset": [("cars1", 6, (40, 56), "suffix", (1, 3, 6)), ("marple2", 5, (33, 47), "regex", (2, 4))],
    "Testset": [("marple7", 6, (24, 72), "suffix", (1, 3, 6)), ("people1", 7, (50, 38), "weird", (10, 12, 13, 16)),
                ("tennis", 5, (61, 29), "regex", (0, 1, 4))],
}
# (sequence, frame count, frame size); a 1-pixel-tall sequence among them
SEGTRACK_SPEC = [("birdfall", 5, (45, 64)), ("worm", 4, (30, 40)), ("frog", 4, (1, 37)), ("drift", 5, (52, 27))]


def _frame(rng, h, w):
    return (rng.random((h, w, 3)) * 255).astype(np.uint8)


def _mask(rng, h, w, colour=False):
    """Blocks of grey levels on both sides of every threshold the conversion uses, white included."""
    levels = np.array([0, 12, 13, 25, 26, 102, 103, 200, 252, 253, 255], np.uint8)
    m = levels[rng.integers(0, len(levels), (h, w))]
    if colour:
        return np.stack([m, np.roll(m, 1, 1), m // 2], -1)
    return m


def make_fbms(root, spec=FBMS_SPEC, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for part, seqs in spec.items():
        for name, n, (h, w), rule, gts in seqs:
            d = os.path.join(root, part, name)
            os.makedirs(os.path.join(d, "GroundTruth"))
            names = ["%s_%02d.pgm" % (name, i + 1) for i in range(n)]
            with open(os.path.join(d, name + ".bmf"), "w") as f:
                f.write("%d 1\n" % n + "\n".join(names) + "\n")
            for nm in names:
                Image.fromarray(_frame(rng, h, w)).save(os.path.join(d, nm.split(".")[0] + ".jpg"), quality=90)
            for k in gts:
                gt_name = {"suffix": "%s_%03d.pgm" % (name, k), "regex": "gt%03d.pgm" % k, "weird": "%s_%02d_gt.ppm" % (name, k)}[rule]
                Image.fromarray(_mask(rng, h, w, rule == "weird")).save(os.path.join(d, "GroundTruth", gt_name))
                if rule == "weird":  # probability maps beside the annotations: never read
                    Image.fromarray(_mask(rng, h, w, True)).save(os.path.join(d, "GroundTruth", "%s_%02d_PROB.ppm" % (name, k)))
    return root


def make_segtrack(root, spec=SEGTRACK_SPEC, seed=1):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "ImageSets"))
    with open(os.path.join(root, "ImageSets", "all.txt"), "w") as f:
        f.write("\n".join("*" + name for name, _, _ in spec) + "\n")
    for name, n, (h, w) in spec:
        os.makedirs(os.path.join(root, "JPEGImages", name))
        os.makedirs(os.path.join(root, "GroundTruth", name))
        stems = ["%05d" % i for i in range(n)]
        with open(os.path.join(root, "ImageSets", name + ".txt"), "w") as f:
            f.write(name + "\n" + "\n".join(stems) + "\n")
        for st in stems:
            Image.fromarray(_frame(rng, h, w)).save(os.path.join(root, "JPEGImages", name, st + ".png"))
            Image.fromarray(((rng.random((h, w)) > 0.5) * 255).astype(np.uint8)).save(os.path.join(root, "GroundTruth", name, st + ".png"))
    return root


# --------------------------------------------------------------------------------------------------------------------- FBMS ----

def test_fbms_training_lists_and_partitions(tmp_path, capsys):
    root = make_fbms(str(tmp_path))
    it = D.FBMS59DirectoryIterator(root, "train")
    assert it.num_experiments == 2 and it.samples == 11 and [len(s) for s in it.image_filenames] == [6, 5]
    assert it.image_filenames[0][0] == os.path.join(root, "Trainingset", "cars1", "cars1_01.jpg")  # header skipped, pgm -> jpg
    assert D.FBMS59DirectoryIterator(root, "val").samples == 18
    tv = D.FBMS59DirectoryIterator(root, "trainval")
    assert tv.samples == 29 and [os.path.basename(s[0]) for s in tv.image_filenames] == \
        ["cars1_01.jpg", "marple2_01.jpg", "marple7_01.jpg", "people1_01.jpg", "tennis_01.jpg"]  # sorted sequence order
    with pytest.raises(IOError):
        D.FBMS59DirectoryIterator(str(tmp_path / "nope"), "val")
    os.remove(os.path.join(root, "Trainingset", "marple2", "marple2.bmf"))
    with pytest.raises(IOError):
        D.FBMS59DirectoryIterator(root, "train")


def test_fbms_find_gt_rules(tmp_path):
    d = tmp_path / "gt"
    d.mkdir()
    for n in ("seq_10.pgm", "seq_2.pgm", "seq_7.pgm", "seq_2.jpg"):
        (d / n).write_bytes(b"")
    assert D.FBMS59DirectoryIterator.find_gt(str(d)) == (["seq_2.pgm", "seq_7.pgm", "seq_10.pgm"], [2, 7, 10], False)
    d = tmp_path / "gt2"
    d.mkdir()
    for n in ("a12b_gt.pgm", "a3b_gt.pgm", "a5b_gt.pgm"):  # no numeric _N: first run of digits
        (d / n).write_bytes(b"")
    assert D.FBMS59DirectoryIterator.find_gt(str(d)) == (["a3b_gt.pgm", "a5b_gt.pgm", "a12b_gt.pgm"], [3, 5, 12], False)
    d = tmp_path / "gt3"
    d.mkdir()
    for n in ("s_20_gt.ppm", "s_4_gt.ppm", "s_4_PROB.ppm", "s_9_x.ppm", "s_1.pgm"):  # any .ppm: the "weird" layout
        (d / n).write_bytes(b"")
    assert D.FBMS59DirectoryIterator.find_gt(str(d)) == (["s_4_gt.ppm", "s_9_x.ppm", "s_20_gt.ppm"], [4, 9, 20], True)


def _tuples(root, t, seq):
    it = D.FBMS59DirectoryIterator(root, "val", for_testing=True, test_temporal_t=t)
    frame = lambda p: int(os.path.basename(p).split(".")[0].split("_")[-1]) - 1
    return [(frame(a), frame(b)) for a, b, g, _ in it.test_tuples if os.sep + seq + os.sep in a], it


def test_fbms_test_tuples_at_both_ends(tmp_path, capsys):
    root = make_fbms(str(tmp_path))
    # marple7: GT at frames 1, 3, 6 of 6 -> numbers 0, 2, 5 (normalised), clamp bound 5
    assert _tuples(root, 1, "marple7")[0] == [(0, 1), (2, 3), (5, 4)]     # last: 6 > 5 -> 6 - 2
    assert _tuples(root, 2, "marple7")[0] == [(0, 2), (2, 4), (5, 3)]     # last: 7 -> 7 - 4
    assert _tuples(root, -1, "marple7")[0] == [(0, 1), (2, 1), (5, 4)]    # first: -1 -> -1 + 2
    # tennis: GT at 0, 1, 4 of 5 frames; people1 ("weird"): GT 10, 12, 13, 16 -> 0, 2, 3, 6 of 7 frames
    assert _tuples(root, -1, "tennis")[0] == [(0, 1), (1, 0), (4, 3)]
    assert _tuples(root, 2, "people1")[0] == [(0, 2), (2, 4), (3, 5), (6, 4)]     # last: 8 -> 8 - 4
    t, it = _tuples(root, -2, "people1")
    assert t == [(0, 2), (2, 0), (3, 1), (6, 4)]                           # first: -2 -> 2; second: 0 stays
    assert it.samples_per_cat == {"marple7": 3, "people1": 4, "tennis": 3} and it.num_experiments == 3 and it.samples == 10
    assert all(r[3] == str(it.samples_per_cat[r[0].split(os.sep)[-2]]) for r in it.test_tuples)
    assert all(r[2].endswith(".ppm") and "PROB" not in r[2] for r in it.test_tuples if "people1" in r[0])


def test_fbms_offsets_clamp_to_the_largest_gt_number_not_the_frame_count(tmp_path, capsys):
    spec = {"Testset": [("clip", 8, (20, 30), "suffix", (1, 3, 4))]}  # numbers 0, 2, 3 of 8 frames: clamp bound 3
    root = make_fbms(str(tmp_path), spec)
    assert _tuples(root, 2, "clip")[0] == [(0, 2), (2, 3), (3, 1)]       # 2 + 2 = 4 exists but is clamped to 3; last 5 -> 1


def test_fbms_reader_tables(tmp_path, capsys):
    root = make_fbms(str(tmp_path))
    rd = D.FBMS59Reader(root)
    assert (rd.min_temporal_len, rd.max_temporal_len) == (2, 3)  # the reference's defaults
    tt = rd.get_test_tuples("val", 1)
    assert len(tt) == 10 and rd.val_samples == 10 and rd.num_categories == 3
    assert rd.samples_per_cat == {"marple7": 3, "people1": 4, "tennis": 3}
    rd.get_filenames_list("train")
    assert rd.val_samples == 11
    with pytest.raises(AssertionError):
        D.FBMS59Reader(root, max_temporal_len=2, min_temporal_len=2)


def test_fbms_gt_conversion():
    # OpenCV's BGR2GRAY fixed point, hand-computed: (1868 B + 9617 G + 4899 R + 8192) >> 14
    rgb = np.array([[[200, 10, 30], [0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255], [77, 77, 77]]], np.uint8)
    assert D.bgr2gray_u8(rgb).tolist() == [[69, 29, 150, 76, 255, 77]]
    grey = lambda v: np.repeat(np.array(v, np.uint8)[None, :, None], 3, 2)
    assert D.fbms_binarize(grey([12, 13, 102, 103]), "marple7", False).tolist() == [[0, 255, 255, 255]]   # > 0.05
    assert D.fbms_binarize(grey([12, 13, 102, 103]), "marple2", False).tolist() == [[0, 0, 0, 255]]       # > 0.4
    assert D.fbms_binarize(grey([25, 26, 102, 255]), "cars1", False).tolist() == [[0, 255, 255, 255]]     # > 0.1
    assert D.fbms_binarize(grey([25, 26, 252, 253, 255]), "people1", True).tolist() == [[0, 255, 255, 0, 0]]  # weird: white -> 0
    # a coloured .ppm pixel goes through the grey formula first: (255, 0, 0) -> 76 -> 0.298 > 0.1
    assert D.fbms_binarize(np.array([[[255, 0, 0], [0, 0, 30]]], np.uint8), "people1", True).tolist() == [[255, 0]]
    # the JPEG round trip of a binary mask: flat regions survive exactly, the result is one channel
    m = np.zeros((32, 32), np.uint8)
    m[8:24, 8:24] = 255
    r = D.jpeg_roundtrip(m)
    assert r.shape == (32, 32) and r.dtype == np.uint8 and r[0, 0] <= 2 and r[16, 16] >= 253


def test_fbms_gt_mask_from_files(tmp_path):
    from PIL import Image
    d = tmp_path / "marple7" / "GroundTruth"
    d.mkdir(parents=True)
    m = np.zeros((16, 16), np.uint8)
    m[:, 8:] = 13  # just above marple7's threshold
    Image.fromarray(m).save(str(d / "marple7_001.pgm"))
    p = str(d / "marple7_001.pgm")
    out = D.fbms_gt_mask(p, data._read_image(p, 3))
    assert out.shape == (16, 16, 1) and out[4, 2, 0] <= 2 and out[4, 13, 0] >= 253
    assert np.array_equal(out[..., 0], D.jpeg_roundtrip(D.fbms_binarize(data._read_image(p, 3), "marple7", False)))


# ---------------------------------------------------------------------------------------------------------------- SegTrackV2 ----

def test_segtrack_layout(tmp_path, capsys):
    root = make_segtrack(str(tmp_path))
    it = D.SegTrackV2DirectoryIterator(root)
    assert it.components == ["birdfall", "worm", "frog", "drift"]  # first character of each all.txt line dropped
    assert [len(s) for s in it.image_filenames] == [5, 4, 4, 5] and it.samples == 18 and it.num_experiments == 4
    assert it.image_filenames[1][0] == os.path.join(root, "JPEGImages", "worm", "00000.png")  # header row skipped
    assert it.annotation_filenames[1][3] == os.path.join(root, "GroundTruth", "worm", "00003.png")
    rd = D.SegTrackV2Reader(root)
    f, a = rd.get_filenames_list()
    assert rd.val_samples == 18 and len(f) == 4
    with pytest.raises(IOError):
        D.SegTrackV2DirectoryIterator(str(tmp_path / "nope"))
    os.remove(os.path.join(root, "GroundTruth", "frog", "00002.png"))
    with pytest.raises(IOError):
        D.SegTrackV2DirectoryIterator(root)
    os.remove(os.path.join(root, "ImageSets", "frog.txt"))
    with pytest.raises(IOError):
        D.SegTrackV2DirectoryIterator(root)


def test_segtrack_png_decoding(tmp_path):
    from PIL import Image
    rgba = np.zeros((2, 3, 4), np.uint8)
    rgba[..., 0], rgba[..., 1], rgba[..., 2], rgba[..., 3] = 200, 10, 30, 7
    rgba[1, 2, :3] = 90  # equal channels
    Image.fromarray(rgba, "RGBA").save(str(tmp_path / "c.png"))
    assert D.read_decode_jpeg(str(tmp_path / "c.png"), 3)[0, 0].tolist() == [200, 10, 30]  # alpha dropped, not composited
    g = D.read_decode_jpeg(str(tmp_path / "c.png"), 1)
    # libpng 8-bit rgb_to_gray with TF's 0.299 / 0.587: (9797 R + 19234 G + 9737 B) >> 15, equal channels kept exactly
    assert g.shape == (2, 3, 1) and g[0, 0, 0] == (9797 * 200 + 19234 * 10 + 9737 * 30) >> 15 == 74 and g[1, 2, 0] == 90
    Image.fromarray(np.full((2, 2), 77, np.uint8)).save(str(tmp_path / "g.png"))
    assert D.read_decode_jpeg(str(tmp_path / "g.png"), 3).tolist() == [[[77] * 3] * 2] * 2
    Image.fromarray(np.full((2, 2), 4000, np.uint16)).save(str(tmp_path / "w.png"))
    with pytest.raises(ValueError, match="16-bit"):
        D.read_decode_jpeg(str(tmp_path / "w.png"), 1)


# ---------------------------------------------------------------------------------------------------------------- both readers ----

def test_shard_batches_are_disjoint_and_cover_each_global_batch():
    order = np.random.default_rng(0).permutation(23)
    r0, r1 = list(D.shard_batches(order, 3, 0, 2)), list(D.shard_batches(order, 3, 1, 2))
    assert len(r0) == len(r1) == 3  # 23 // 6 global batches, the remainder dropped
    for k, (a, b) in enumerate(zip(r0, r1)):
        assert len(a) == len(b) == 3 and not set(a) & set(b)
        assert sorted(np.concatenate([a, b])) == sorted(order[6 * k:6 * k + 6])
    assert [list(x) for x in D.shard_batches(order, 4)] == [list(order[i:i + 4]) for i in range(0, 20, 4)]


@pytest.mark.parametrize("which", ["fbms", "segtrack"])
def test_readers_shard_rows(tmp_path, monkeypatch, capsys, which):
    """The training rows the two ranks of shard=(r, 2) draw: disjoint, together the global batch of the shared shuffle."""
    root = make_fbms(str(tmp_path)) if which == "fbms" else make_segtrack(str(tmp_path))
    monkeypatch.setattr(D._RaggedReader, "_image_pairs", lambda self, p1, p2: (torch.zeros(len(p1), 1, 1, 3), torch.zeros(len(p2), 1, 1, 3)))
    monkeypatch.setattr(data, "augment_pair", lambda a, b, crop, rng: (a, b))
    picked = []
    for rank in (0, 1):
        rd = (D.FBMS59Reader if which == "fbms" else D.SegTrackV2Reader)(root, 2, 1, seed=7, shard=(rank, 2))
        src = rd.image_inputs(batch_size=2, train_crop=0.9, **({"partition": "train"} if which == "fbms" else {}))
        picked.append([next(src)["fname"] for _ in range(2)])
    files = np.concatenate((D.FBMS59Reader(root).get_filenames_list("train") if which == "fbms" else
                            D.SegTrackV2Reader(root).get_filenames_list())[0])
    lens = [len(s) for s in (D.FBMS59DirectoryIterator(root, "train") if which == "fbms" else D.SegTrackV2DirectoryIterator(root)).image_filenames]
    table = data.pair_table(lens, 2, True)
    order = np.random.default_rng(7).permutation(len(table))
    for k in range(2):
        a, b = picked[0][k], picked[1][k]
        assert len(a) == len(b) == 2
        rows = table[order[4 * k:4 * k + 4]]
        assert a + b == [f.encode() for f in files[rows[:, 0].astype(np.int32)]]


def test_ragged_wrapper_validates_tables_on_the_host():
    buf = torch.zeros(100, dtype=torch.uint8)  # two samples: 4x4x3 at 0, 3x5x3 at 48 (ends at 93)
    ok = dict(offsets=[0, 48], hw=[[4, 4], [3, 5]], c=3)
    data.check_ragged_tables(ok["offsets"], ok["hw"], 3, 100, [[0, 0, 4, 4, 0, 0], [1, 2, 2, 3, 1, 1]])
    with pytest.raises(ValueError, match="window"):
        data.crop_flip_resize_ragged(buf, **ok, out_h=8, out_w=8, params=[[0, 0, 4, 4, 0, 0], [1, 2, 3, 3, 0, 0]])  # 1 + 3 > 3
    with pytest.raises(ValueError, match="window"):
        data.crop_flip_resize_ragged(buf, **ok, out_h=8, out_w=8, params=[[0, 1, 4, 4, 0, 0], [0, 0, 3, 5, 0, 0]])  # 1 + 4 > 4
    with pytest.raises(ValueError, match="buffer"):
        data.crop_flip_resize_ragged(buf, [0, 60], ok["hw"], 3, 8, 8)  # 60 + 45 > 100
    with pytest.raises(ValueError, match="buffer"):
        data.crop_flip_resize_ragged(buf, [0, 48], [[4, 4], [4, 5]], 3, 8, 8)
    with pytest.raises(ValueError, match="flip"):
        data.crop_flip_resize_ragged(buf, **ok, out_h=8, out_w=8, params=[[0, 0, 4, 4, 2, 0], [0, 0, 3, 5, 0, 0]])
    with pytest.raises(ValueError, match="1x1"):
        data.crop_flip_resize_ragged(buf, [0, 48], [[4, 4], [0, 5]], 3, 8, 8)
