"""FBMS-59 and SegTrackV2 readers (data/fbms_data_utils.py, data/segtrackv2_data_utils.py of the reference) on the ragged
input stage of data.py.

Both datasets mix frame sizes inside a batch (FBMS sequences come at several sizes, SegTrackV2 from a few hundred pixels on a
side up to 720p), so a batch is decoded on the host (Pillow), packed into one pinned buffer, copied once, and brought to
READER_H x READER_W by one udet_crop_flip_resize_ragged launch.  Everything after that point -- the augmentation (flip + equal
random crop) and the central crops -- runs on the uniform crop_flip_resize, exactly as in the DAVIS reader.  Same class,
method and argument names as the reference; `shard`, `seed`, `loader` and `device` have the contract of
data.Davis2016Reader, and the draws of a training batch come in the DAVIS order: temporal shifts, then flips, then crops.

  FBMS59 DirectoryIterator(directory, part, for_testing, test_temporal_t)   fbms_data_utils.py:19-170
  FBMS59Reader.get_filenames_list / get_test_tuples / image_inputs / test_inputs / augmented_inputs   :172-392
  SegTrackV2 DirectoryIterator(directory)                                    segtrackv2_data_utils.py:11-69
  SegTrackV2Reader.get_filenames_list / image_inputs / test_inputs / augmented_inputs                 :72-330
  FrameFolderReader (natural_key, frame_files, frame_folder_sequences)       a plain folder of frames without annotations: the
                                                                             use of scripts/create_data_frvideo.py + test_video.sh

Batches are the dicts {"img1","img2","gt_mask","fname"} AdversarialLearner consumes; FBMS test batches also carry
"samples_per_cat" (float32 per row, the number of annotated frames of the row's sequence)."""
from __future__ import annotations

import io
import os
import re

import numpy as np
import torch

from . import data

# ---------------------------------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------------------------------


def shard_batches(order, batch_size, rank=0, world=1):
    """Row indices of one epoch of a sharded training reader: global batches of batch_size * world rows of `order` (the pair
    table's shuffle, identical on every rank), rank r taking rows [r*batch_size, (r+1)*batch_size) of each; an incomplete last
    global batch is dropped (drop_remainder=True).  The same selection as data.Davis2016Reader.image_inputs."""
    gb = batch_size * world
    for s in range(0, len(order) - gb + 1, gb):
        yield order[s + rank * batch_size:s + (rank + 1) * batch_size]


def _loadtxt_column(path, skiprows=0):
    """np.loadtxt(path, dtype=str, skiprows=skiprows) of a one-column list: `skiprows` first lines dropped, '#' comments and
    blank lines ignored, first whitespace-separated token of each remaining line."""
    with open(path) as f:
        lines = f.read().splitlines()[skiprows:]
    out = []
    for ln in lines:
        tok = ln.split("#", 1)[0].split()
        if tok:
            out.append(tok[0])
    return out


class _RaggedReader(object):
    """The sharding / seeding contract of data.Davis2016Reader plus the ragged loader and the batch assembly both readers share."""

    def __init__(self, root_dir, max_temporal_len, min_temporal_len, num_threads, device, seed, loader, shard):
        self.root_dir, self.max_temporal_len, self.min_temporal_len = root_dir, max_temporal_len, min_temporal_len
        self.num_threads, self.device = num_threads, device
        self.rank, self.world = int(shard[0]), max(1, int(shard[1]))
        assert 0 <= self.rank < self.world, "shard = (rank, world)"
        assert self.world == 1 or seed is not None, "a sharded reader (world > 1) needs an explicit seed, the same on every rank"
        self.order_rng = np.random.default_rng(seed)  # identical on every rank: the shuffle of the pair table
        self.rng = self.order_rng if self.world == 1 else np.random.default_rng(None if seed is None else seed + 1 + self.rank)
        self.loader = loader or self.default_loader  # (path, channels) -> uint8 [H,W,C]
        self._ragged = None

    default_loader = staticmethod(data._read_image)

    @property
    def ragged(self):
        if self._ragged is None:  # created on first use: the CPU-side parsing needs no device
            self._ragged = data.RaggedLoader(self.loader, self.num_threads, self.device)
        return self._ragged

    def _image_pairs(self, paths_1, paths_2):
        """Both frames of every pair through one ragged load + one launch: preprocess_image -> (img1s, img2s) [B,H,W,3]."""
        x = self.ragged.load(list(paths_1) + list(paths_2), 3).preprocess_image()
        return x[:len(paths_1)], x[len(paths_1):]

    def _train_batches(self, filenames, table, batch_size, train_crop):
        """image_inputs (:270-311): an endless stream; per batch the temporal shifts, then augment_pair's flips and crops."""
        while True:
            order = self.order_rng.permutation(len(table))
            for idx in shard_batches(order, batch_size, self.rank, self.world):
                rows = table[idx]
                shift = self.rng.integers(self.min_temporal_len, self.max_temporal_len + 1, len(rows))
                i1 = rows[:, 0].astype(np.int32)
                i2 = (shift.astype(np.float32) * rows[:, 1] + rows[:, 0]).astype(np.int32)
                a, b = self._image_pairs(filenames[i1], filenames[i2])
                a, b = data.augment_pair(a, b, train_crop, self.rng)
                yield {"img1": a, "img2": b, "gt_mask": None, "fname": [f.encode() for f in filenames[i1]]}

    def _test_batch(self, paths_1, paths_2, gt_paths, test_crop, gt_loader=None):
        """test_dataset_map: preprocess_image / preprocess_mask (nearest), then central_cropping of all three with the
        bilinear resize, the mask included."""
        a, b = self._image_pairs(paths_1, paths_2)
        g = self.ragged.load(gt_paths, 1, gt_loader).preprocess_mask()
        return {"img1": data.central_cropping(a, test_crop), "img2": data.central_cropping(b, test_crop),
                "gt_mask": data.central_cropping(g, test_crop), "fname": [f.encode() for f in paths_1]}

    @staticmethod
    def _augment(test_batches, test_crops):
        """augmented_inputs: per frame a dict of centrally cropped versions for the ensemble, batch size 1."""
        for batch in test_batches:
            d = {"img_1s": {}, "img_2s": {}, "seg_1s": {}}
            for crop in test_crops:
                d["img_1s"][crop] = data.central_cropping(batch["img1"], crop)[0]
                d["img_2s"][crop] = data.central_cropping(batch["img2"], crop)[0]
                d["seg_1s"][crop] = None if batch["gt_mask"] is None else data.central_cropping(batch["gt_mask"], crop)[0]
            yield d, batch["fname"][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# FBMS-59
# ---------------------------------------------------------------------------------------------------------------------------------

FBMS_PARTITIONS = {"train": ["Trainingset"], "val": ["Testset"], "trainval": ["Trainingset", "Testset"]}


def fbms_threshold(folder_name):
    """The per-sequence binarisation threshold of the ground-truth conversion (fbms_data_utils.py:115-120)."""
    return 0.05 if folder_name == "marple7" else 0.4 if folder_name == "marple2" else 0.1


def bgr2gray_u8(rgb):
    """OpenCV's 8-bit COLOR_BGR2GRAY in fixed point: (1868 B + 9617 G + 4899 R + 8192) >> 14.  rgb uint8 [H,W,3] in RGB order
    (cv2.imread would hand the same pixels over as BGR)."""
    x = np.asarray(rgb, dtype=np.int32)
    return ((1868 * x[..., 2] + 9617 * x[..., 1] + 4899 * x[..., 0] + 8192) >> 14).astype(np.uint8)


def fbms_binarize(rgb, folder_name, type_weird):
    """fbms_data_utils.py:110-124 up to the cv2.imwrite: grey (bgr2gray_u8) / 255; the "weird" (.ppm) annotations lose their
    white (> 0.99 -> 0); threshold per sequence (fbms_threshold); * 255 -> uint8 {0, 255} [H,W]."""
    mask = bgr2gray_u8(rgb) / 255.0
    if type_weird:
        mask[mask > 0.99] = 0.0
    mask = mask > fbms_threshold(folder_name)
    return np.asarray(mask * 255, dtype=np.uint8)


def jpeg_roundtrip(mask_u8, quality=95):
    """The reference writes the binarised mask as <frame>.jpg (cv2.imwrite, default quality 95) and its test graph decodes that
    JPEG with one channel: here the same round trip in memory through Pillow's encoder at quality 95.  The JPEG encoder of the
    reference's OpenCV build is not pinned here (OpenCV is not a dependency of this port), so the ringing around the mask's
    edges can differ from its files by the encoders' quantisation / DCT choices; the decoded values stay within a few levels."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(mask_u8), "L").save(buf, "JPEG", quality=quality)
    buf.seek(0)
    with Image.open(buf) as im:
        return np.asarray(im.convert("L"), dtype=np.uint8)


def fbms_gt_mask(path, rgb):
    """The test graph's view of one FBMS annotation: fbms_binarize (sequence = the directory above GroundTruth, "weird" = a
    .ppm annotation) then the JPEG round trip, as uint8 [H,W,1].  Restated in memory: nothing is written to the dataset tree."""
    folder = os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(path))))
    return jpeg_roundtrip(fbms_binarize(rgb, folder, path.endswith("ppm")))[..., None]


class FBMS59DirectoryIterator(object):
    """fbms_data_utils.py:19-170.  Training: image_filenames = per-sequence frame lists from <seq>/<seq>.bmf (header row
    skipped, x.pgm -> x.jpg).  Testing: test_tuples (frame_k, frame_offset, gt, samples_per_cat) at the annotated frames only.

    Divergences from the reference: the sequence (and annotation-file) order is that of sorted(os.listdir), not the
    filesystem's own order (which differs between machines); `gt` is the source annotation (.pgm / .ppm), converted in
    memory by fbms_gt_mask instead of the <frame>.jpg the reference writes into the dataset tree.  Kept as in the reference:
    the per-directory reset of test_tuples (for_testing on 'trainval' keeps the Testset tuples while `samples` counts
    both), the clamp of the offsets to the largest GT number rather than to the frame count."""

    def __init__(self, directory, part="train", for_testing=False, test_temporal_t=1):
        self.directory = directory
        self.num_experiments = 0
        self.samples_per_cat = {}
        self.test_tuples = []
        data_dirs = [os.path.join(directory, d) for d in FBMS_PARTITIONS.get(part, ())]
        for d in data_dirs:
            if not os.path.isdir(d):
                raise IOError("Directory {} file not found".format(d))
        self.samples = 0
        self.image_filenames = []
        self.annotation_filenames = []
        for d in data_dirs:
            if for_testing:
                self._parse_testtime_dir(d, test_temporal_t)
            else:
                self._parse_data_dir(d)
        if self.samples == 0:
            raise IOError("Did not find any file in the dataset folder")
        if not for_testing:
            self.num_experiments = len(self.image_filenames)
        print("Found {} images belonging to {} experiments.".format(self.samples, self.num_experiments))

    @staticmethod
    def _frame_list(data_dir, folder_name):
        bmf = os.path.join(data_dir, folder_name, folder_name + ".bmf")
        if not os.path.isfile(bmf):
            raise IOError("Not found file {}".format(bmf))
        names = [f.split(".")[0] + ".jpg" for f in _loadtxt_column(bmf, skiprows=1)]  # correct from pgm to jpg
        return [os.path.join(data_dir, folder_name, f) for f in names]

    def _parse_data_dir(self, data_dir):
        for folder_name in sorted(os.listdir(data_dir)):
            frames = self._frame_list(data_dir, folder_name)
            self.samples += len(frames)
            self.image_filenames.append(frames)

    def _parse_testtime_dir(self, data_dir, test_temporal_t=1):
        self.test_tuples = []  # (sic: per directory, fbms_data_utils.py:88)
        for folder_name in sorted(os.listdir(data_dir)):
            frames = self._frame_list(data_dir, folder_name)
            gt_dir = os.path.join(data_dir, folder_name, "GroundTruth")
            annotation_fnames, numbers, _ = self.find_gt(gt_dir)
            annotation_fnames = [os.path.join(gt_dir, f) for f in annotation_fnames]
            numbers = np.array(numbers) - np.min(numbers)
            seq_len = np.max(numbers)
            offsets = numbers + test_temporal_t
            if offsets[0] < numbers[0]:  # test was negative, needs to increase
                offsets[0] += 2 * abs(test_temporal_t)
            if offsets[-1] > numbers[-1]:  # test was positive, needs to decrease
                offsets[-1] -= 2 * abs(test_temporal_t)
            offsets = np.minimum(np.maximum(offsets, 0), seq_len)
            for i, k in enumerate(numbers):
                self.test_tuples.append((frames[k], frames[offsets[i]], annotation_fnames[i], "{}".format(len(annotation_fnames))))
            self.samples += len(annotation_fnames)
            self.samples_per_cat[folder_name] = len(annotation_fnames)
            self.num_experiments += 1

    @staticmethod
    def find_gt(directory):
        """(annotation file names, frame numbers, type_weird) of a GroundTruth directory (fbms_data_utils.py:151-170): .pgm
        files sorted by their trailing _N, or by the first run of digits when a name has no numeric _N; if any file ends in
        "ppm" the "weird" layout: the .ppm files without PROB in their name, numbered by split('_')[1]."""
        all_files = sorted(os.listdir(directory))
        type_weird = any(f.endswith("ppm") for f in all_files)
        if not type_weird:
            all_files = [f for f in all_files if f.endswith("pgm")]
            try:
                all_files = sorted(all_files, key=lambda x: int(x.split(".")[0].split("_")[-1]))
                numbers = [int(f.split(".")[0].split("_")[-1]) for f in all_files]
            except ValueError:
                all_files = sorted(all_files, key=lambda x: int(re.search(r"\d+", x).group()))
                numbers = [int(re.search(r"\d+", f).group()) for f in all_files]
            return all_files, numbers, type_weird
        all_files = [f for f in all_files if f.endswith("ppm") and "PROB" not in f]
        all_files = sorted(all_files, key=lambda x: int(x.split("_")[1]))
        numbers = [int(f.split("_")[1]) for f in all_files]
        return all_files, numbers, type_weird




class FBMS59Reader(_RaggedReader):
    """data/fbms_data_utils.py:172-392 as Python iterables of device batches."""

    def __init__(self, root_dir, max_temporal_len=3, min_temporal_len=2, num_threads=6, device="cuda", seed=None, loader=None,
                 shard=(0, 1)):
        assert min_temporal_len < max_temporal_len, "Temporal lenghts are not consistent"
        assert min_temporal_len > 0, "Min temporal len should be positive"
        super().__init__(root_dir, max_temporal_len, min_temporal_len, num_threads, device, seed, loader, shard)

    def get_filenames_list(self, partition):
        it = FBMS59DirectoryIterator(self.root_dir, partition)
        self.val_samples = it.samples
        return it.image_filenames, it.annotation_filenames

    def get_test_tuples(self, partition, test_temporal_t=1):
        it = FBMS59DirectoryIterator(self.root_dir, partition, for_testing=True, test_temporal_t=test_temporal_t)
        self.val_samples = it.samples
        self.samples_per_cat = it.samples_per_cat
        self.num_categories = len(it.samples_per_cat.keys())
        return it.test_tuples

    def gt_loader(self, path, channels):
        """An annotation as the test graph decodes it (fbms_gt_mask of the loader's RGB decode)."""
        return fbms_gt_mask(path, self.loader(path, 3))

    def image_inputs(self, batch_size=32, partition="train", train_crop=1.0):
        """Endless training batches {"img1","img2"} (:270-311): img2 = img1 +- U{min..max} frames, augmented."""
        file_list, _ = self.get_filenames_list(partition)
        filenames = np.concatenate(file_list)
        table = data.pair_table([len(f) for f in file_list], self.max_temporal_len, True)
        return self._train_batches(filenames, table, batch_size, train_crop)

    def test_inputs(self, batch_size=32, partition="val", t_len=2, with_fname=False, test_crop=1.0):
        """One pass over the annotated frames (:313-368), in tuple order; batches also carry samples_per_cat."""
        tuples = self.get_test_tuples(partition, t_len)

        def gen():
            for s in range(0, len(tuples), batch_size):  # drop_remainder=False
                rows = tuples[s:s + batch_size]
                batch = self._test_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], test_crop, self.gt_loader)
                batch["samples_per_cat"] = np.array([float(r[3]) for r in rows], np.float32)
                yield batch
        return gen()

    def augmented_inputs(self, partition="val", t_len=2, test_crops=(1.0,)):
        """Per annotated frame a dict of centrally cropped versions for the ensemble (:370-392), batch size 1."""
        return self._augment(self.test_inputs(batch_size=1, partition=partition, t_len=t_len, with_fname=True, test_crop=1.0),
                             test_crops)


# ---------------------------------------------------------------------------------------------------------------------------------
# SegTrackV2
# ---------------------------------------------------------------------------------------------------------------------------------

_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def read_decode_jpeg(path, channels):
    """tf.image.decode_jpeg(contents, channels) of a SegTrackV2 frame / annotation (PNG files; TF-1.13's decode_jpeg decodes
    PNG too, through libpng).  channels=3: RGB, alpha dropped without compositing, grey and palette expanded.  channels=1 of
    a colour PNG: libpng's png_set_rgb_to_gray(png, 1, 0.299, 0.587) as TF's png_io sets it -- fixed-point weights
    9797 R + 19234 G + 9737 B (/32768, from 0.299 / 0.587 / the remainder), truncated, and a pixel with equal channels kept
    as that channel.  16-bit PNGs are refused: TF would reduce them to 8 bits in its own way."""
    from PIL import Image
    with open(path, "rb") as f:
        head = f.read(26)
    if head[:8] == _PNG_SIGNATURE and len(head) > 24 and head[24] == 16:
        raise ValueError("{}: 16-bit PNG is not supported (only 8-bit frames and annotations)".format(path))
    with Image.open(path) as im:
        if channels == 3:
            return np.asarray(im.convert("RGB"), dtype=np.uint8).reshape(im.size[1], im.size[0], 3)
        if im.mode in ("L", "LA", "1", "I", "I;16"):
            return np.asarray(im.convert("L"), dtype=np.uint8).reshape(im.size[1], im.size[0], 1)
        return png_rgb_to_gray(np.asarray(im.convert("RGB"), dtype=np.uint8))[..., None]


def png_rgb_to_gray(rgb):
    """libpng's 8-bit rgb_to_gray without gamma: equal channels -> that channel, else (9797 R + 19234 G + 9737 B) >> 15."""
    x = np.asarray(rgb, dtype=np.int64)
    g = (9797 * x[..., 0] + 19234 * x[..., 1] + 9737 * x[..., 2]) >> 15
    equal = (x[..., 0] == x[..., 1]) & (x[..., 0] == x[..., 2])
    return np.where(equal, x[..., 0], g).astype(np.uint8)


class SegTrackV2DirectoryIterator(object):
    """segtrackv2_data_utils.py:11-69: ImageSets/all.txt lists the sequences (first character of each name dropped);
    ImageSets/<seq>.txt the frame stems (header row skipped); frames JPEGImages/<seq>/<stem>.png, annotations
    GroundTruth/<seq>/<stem>.png.  A missing list or frame is an IOError (the reference asserts)."""

    def __init__(self, directory):
        self.directory = directory
        all_files = os.path.join(directory, "ImageSets", "all.txt")
        self.image_dirs = os.path.join(directory, "JPEGImages")
        self.annotation_dir = os.path.join(directory, "GroundTruth")
        if not os.path.isfile(all_files):
            raise IOError("Division file not found")
        self.components = [c[1:] for c in _loadtxt_column(all_files)]
        self.samples = 0
        self.num_experiments = 0
        self.image_filenames = []
        self.annotation_filenames = []
        for experiment in self.components:
            self._parse_experiment(experiment)
            self.num_experiments += 1
        if self.samples == 0:
            raise IOError("Did not find any file in the dataset folder")
        print("Found {} images belonging to {} experiments.".format(self.samples, self.num_experiments))

    def _parse_experiment(self, experiment):
        experiment_file = os.path.join(self.directory, "ImageSets", experiment + ".txt")
        if not os.path.isfile(experiment_file):
            raise IOError("Experiment {} not found".format(experiment_file))
        frames, annotations = [], []
        for stem in _loadtxt_column(experiment_file, skiprows=1):
            frames.append(os.path.join(self.image_dirs, experiment, stem + ".png"))
            annotations.append(os.path.join(self.annotation_dir, experiment, stem + ".png"))
            for p in (frames[-1], annotations[-1]):
                if not os.path.isfile(p):
                    raise IOError("Not found image {}".format(p))
            self.samples += 1
        self.image_filenames.append(frames)
        self.annotation_filenames.append(annotations)


class SegTrackV2Reader(_RaggedReader):
    """data/segtrackv2_data_utils.py:72-330 as Python iterables of device batches.  No partition: every method works on
    every sequence listed in all.txt (the test_partition flag does not apply to this dataset, as in the reference)."""

    default_loader = staticmethod(read_decode_jpeg)

    def __init__(self, root_dir, max_temporal_len=3, min_temporal_len=2, num_threads=6, device="cuda", seed=None, loader=None,
                 shard=(0, 1)):
        super().__init__(root_dir, max_temporal_len, min_temporal_len, num_threads, device, seed, loader, shard)

    def get_filenames_list(self):
        it = SegTrackV2DirectoryIterator(self.root_dir)
        self.val_samples = it.samples
        return it.image_filenames, it.annotation_filenames

    def image_inputs(self, batch_size=32, train_crop=1.0, num_threads=6):
        """Endless training batches {"img1","img2"} (:180-226): img2 = img1 +- U{min..max} frames, augmented."""
        file_list, _ = self.get_filenames_list()
        filenames = np.concatenate(file_list)
        table = data.pair_table([len(f) for f in file_list], self.max_temporal_len, True)
        return self._train_batches(filenames, table, batch_size, train_crop)

    def test_inputs(self, batch_size=32, t_len=2, with_fname=False, test_crop=1.0):
        """One pass over every frame (:228-304): time(img2) - time(img1) = t_len except at sequence ends."""
        file_list, ann_list = self.get_filenames_list()
        filenames, annotations = np.concatenate(file_list), np.concatenate(ann_list)
        table = data.pair_table([len(f) for f in file_list], t_len, False)

        def gen():
            for s in range(0, len(table), batch_size):  # drop_remainder=False
                rows = table[s:s + batch_size]
                i1 = rows[:, 0].astype(np.int32)
                i2 = (np.float32(abs(t_len)) * rows[:, 1] + rows[:, 0]).astype(np.int32)
                yield self._test_batch(filenames[i1], filenames[i2], annotations[i1], test_crop)
        return gen()

    def augmented_inputs(self, t_len=2, test_crops=(1.0,)):
        """Per frame a dict of centrally cropped versions for the ensemble (:306-330), batch size 1."""
        return self._augment(self.test_inputs(batch_size=1, t_len=t_len, with_fname=True, test_crop=1.0), test_crops)


# ---------------------------------------------------------------------------------------------------------------------------------
# A plain folder of frames (no annotations)
# ---------------------------------------------------------------------------------------------------------------------------------

FRAME_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp")


def natural_key(name):
    """Sort key of the natural order of file names: runs of digits compare as integers (frame_2 < frame_10), everything between them
    as plain strings, ties (frame_02 / frame_2) broken by the plain string."""
    return [int(t) if i & 1 else t for i, t in enumerate(re.split(r"(\d+)", name))], name


def frame_files(names):
    """The frames among the file names of one directory, in natural order: names ending in .jpg / .jpeg / .png / .bmp (any case);
    dot-files and everything else are ignored."""
    return sorted((n for n in names if not n.startswith(".") and n.lower().endswith(FRAME_EXTENSIONS)), key=natural_key)


def frame_folder_sequences(root_dir):
    """[(sequence name, [frame paths in natural order]), ...] of a folder of frames: every sub-directory of root_dir that holds images is
    a sequence, sorted by name; if none does and root_dir itself holds images, it is one sequence named basename(root_dir).  No image
    at all (or no such directory) is an IOError."""
    root = os.path.abspath(root_dir) if root_dir else ""  # (a frame's category is the directory above it: "." would not name one)
    layout = "FRAMES layout: <root_dir>/<sequence>/<frame>.jpg|.jpeg|.png|.bmp, or the frames in <root_dir> itself"
    if not (root and os.path.isdir(root)):
        raise IOError("Directory {!r} not found ({})".format(root_dir, layout))
    seqs = []
    for name in sorted(os.listdir(root)):
        d = os.path.join(root, name)
        if name.startswith(".") or not os.path.isdir(d):
            continue
        frames = frame_files(os.listdir(d))
        if frames:
            seqs.append((name, [os.path.join(d, f) for f in frames]))
    if not seqs:
        frames = frame_files(os.listdir(root))
        if frames:
            seqs.append((os.path.basename(root), [os.path.join(root, f) for f in frames]))
    if not seqs:
        raise IOError("Did not find any image under {!r} ({})".format(root_dir, layout))
    return seqs


class FrameFolderReader(_RaggedReader):
    """A reader for one's own footage: frames on disk (frame_folder_sequences), no annotation anywhere -- the job of the reference's
    scripts/create_data_frvideo.py + scripts/test_video.sh without the faked DAVIS tree.  Batches carry "gt_mask": None, which
    learner.inference, evaluate_masks and evaluate_ensemble take.  No partition argument, like SegTrackV2Reader.  A sequence must hold
    max_temporal_len + 1 frames to train on and |t_len| + 1 to test on (IOError naming it); in a test sequence shorter than 2 |t_len|
    the second frame of a pair is clamped into its own sequence."""

    def __init__(self, root_dir, max_temporal_len=3, min_temporal_len=2, num_threads=6, device="cuda", seed=None, loader=None,
                 shard=(0, 1)):
        super().__init__(root_dir, max_temporal_len, min_temporal_len, num_threads, device, seed, loader, shard)

    def get_filenames_list(self, min_frames=1):
        """(per-sequence frame lists, per-sequence lists of None); a sequence of fewer than min_frames frames is an IOError."""
        seqs = frame_folder_sequences(self.root_dir)
        for name, frames in seqs:
            if len(frames) < min_frames:
                raise IOError("Sequence {!r} under {!r} holds {} frame(s), {} are needed".format(name, self.root_dir, len(frames), min_frames))
        self.val_samples = sum(len(f) for _, f in seqs)
        print("Found {} images belonging to {} experiments.".format(self.val_samples, len(seqs)))
        return [f for _, f in seqs], [[None] * len(f) for _, f in seqs]

    def image_inputs(self, batch_size=32, train_crop=1.0, num_threads=6):
        """Endless training batches {"img1","img2"}: img2 = img1 +- U{min..max} frames, augmented (the other readers' image_inputs)."""
        file_list, _ = self.get_filenames_list(self.max_temporal_len + 1)
        filenames = np.concatenate(file_list)
        table = data.pair_table([len(f) for f in file_list], self.max_temporal_len, True)
        return self._train_batches(filenames, table, batch_size, train_crop)

    def test_inputs(self, batch_size=32, t_len=2, with_fname=False, test_crop=1.0):
        """One pass over every frame: time(img2) - time(img1) = t_len except at sequence ends; "gt_mask" is None."""
        file_list, _ = self.get_filenames_list(abs(t_len) + 1)
        filenames = np.concatenate(file_list)
        lengths = [len(f) for f in file_list]
        table = data.pair_table(lengths, t_len, False)
        first = np.repeat(np.cumsum([0] + lengths[:-1]), lengths)  # per frame: the first and the last frame of its sequence
        last = first + np.repeat(lengths, lengths) - 1

        def gen():
            for s in range(0, len(table), batch_size):  # drop_remainder=False
                rows = table[s:s + batch_size]
                i1 = rows[:, 0].astype(np.int32)
                i2 = (np.float32(abs(t_len)) * rows[:, 1] + rows[:, 0]).astype(np.int32)
                i2 = np.clip(i2, first[i1], last[i1])
                a, b = self._image_pairs(filenames[i1], filenames[i2])
                yield {"img1": data.central_cropping(a, test_crop), "img2": data.central_cropping(b, test_crop), "gt_mask": None,
                       "fname": [f.encode() for f in filenames[i1]]}
        return gen()

    def augmented_inputs(self, t_len=2, test_crops=(1.0,)):
        """Per frame a dict of centrally cropped versions for the ensemble, batch size 1; seg_1s[crop] is None."""
        return self._augment(self.test_inputs(batch_size=1, t_len=t_len, with_fname=True, test_crop=1.0), test_crops)
