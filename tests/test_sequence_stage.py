"""CPU: the host side of the batched sequence stage -- check_sequence_tables, the chunking of PWCFlow.batch, the
post_process subcommand's parser and sequence discovery, the unchanged defaults of propagate / buffer_to_soft_score / run_crf, and the
new exports of libudet.so.  Also the inputs tests/test_sequence_stage_gpu.py shares."""
import inspect
import os

import numpy as np
import pytest


def soft_mask(h, w, seed):
    """A blob plus a little noise, max 1 (the shape of tests/test_post_processing.py's masks)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w
    m = np.exp(-(((yy - cy) / (0.2 * h)) ** 2 + ((xx - cx) / (0.15 * w)) ** 2)) + 0.05 * rng.random((h, w))
    return (m / m.max()).astype(np.float32)


def test_check_sequence_tables():
    from unsupervised_detection_amd.post_processing import check_sequence_tables
    first, length = check_sequence_tables([0, 1, 3], [1, 2, 5], 8)
    assert first.dtype == np.int32 and length.dtype == np.int32 and first.tolist() == [0, 1, 3] and length.tolist() == [1, 2, 5]
    check_sequence_tables([6, 0], [2, 3], 9)  # any order, gaps allowed
    check_sequence_tables([0], [1], 1)
    with pytest.raises(ValueError, match="overlap"):
        check_sequence_tables([0, 2], [3, 2], 8)
    with pytest.raises(ValueError, match="overlap"):
        check_sequence_tables([4, 0], [2, 5], 8)  # unsorted and overlapping
    with pytest.raises(ValueError, match="overlap"):
        check_sequence_tables([3, 3], [1, 1], 8)
    with pytest.raises(ValueError, match="outside"):
        check_sequence_tables([0, 3], [3, 6], 8)
    with pytest.raises(ValueError, match="outside"):
        check_sequence_tables([-1], [2], 8)
    with pytest.raises(ValueError, match="outside"):
        check_sequence_tables([8], [1], 8)
    with pytest.raises(ValueError, match="length"):
        check_sequence_tables([0, 3], [3, 0], 8)
    with pytest.raises(ValueError, match="length"):
        check_sequence_tables([0], [-2], 8)
    with pytest.raises(ValueError):
        check_sequence_tables([0, 1], [1], 8)  # one length per sequence
    with pytest.raises(ValueError):
        check_sequence_tables([], [], 8)
    with pytest.raises(ValueError, match="65535"):
        check_sequence_tables(np.arange(65536), np.ones(65536, np.int64), 65536)
    with pytest.raises(ValueError):
        check_sequence_tables([0], [1], 0)


@pytest.mark.parametrize("n, batch", [(3, 8), (8, 8), (9, 8), (1, 8), (1, 1), (5, 2), (16, 8)])
def test_flow_chunks_pad_and_trim(n, batch):
    from unsupervised_detection_amd.post_processing import flow_chunks
    chunks = flow_chunks(n, batch)
    assert len(chunks) == -(-n // batch)
    kept = []
    for idx, keep in chunks:
        assert len(idx) == batch and 1 <= keep <= batch  # one engine shape
        assert idx[:keep] == list(range(idx[0], idx[0] + keep))  # consecutive: the results land in one slice
        assert all(i == idx[keep - 1] for i in idx[keep:])  # padded by repeating the last pair
        assert all(0 <= i < n for i in idx)
        kept += idx[:keep]
    assert kept == list(range(n))  # every pair once, in order
    assert all(keep == batch for _, keep in chunks[:-1])


def test_flow_chunks_known_answers():
    from unsupervised_detection_amd.post_processing import flow_chunks
    assert flow_chunks(3, 2) == [([0, 1], 2), ([2, 2], 1)]
    assert flow_chunks(1, 4) == [([0, 0, 0, 0], 1)]
    assert flow_chunks(4, 4) == [([0, 1, 2, 3], 4)]
    assert flow_chunks(5, 4) == [([0, 1, 2, 3], 4), ([4, 4, 4, 4], 1)]
    for bad in ((0, 4), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            flow_chunks(*bad)


def test_pwcflow_batch_signature_and_argument_errors():
    """The arrays of PWCFlow.batch go through the device helper, so its results are checked on the GPU; here: its signature and the
    errors it raises before it touches the model."""
    from unsupervised_detection_amd import post_processing as PP
    assert list(inspect.signature(PP.PWCFlow.batch).parameters) == ["self", "imgs_from", "imgs_to", "batch"]
    assert inspect.signature(PP.PWCFlow.batch).parameters["batch"].default == 8
    with pytest.raises(ValueError):
        PP.PWCFlow(model=object()).batch([], [], 2)
    with pytest.raises(ValueError):
        PP.PWCFlow(model=object()).batch([np.zeros((4, 4, 3), np.uint8)], [], 2)


def test_post_process_parser_defaults():
    from unsupervised_detection_amd import cli
    a = cli.parse_post_process_args(["--buffer_dir", "B", "--out_dir", "O"])
    # post_processing/post_processing.py:24-27 (sxy, srgb, scomp, gauss_k) and :40 (the CRF at original resolution)
    assert (a.sxy, a.srgb, a.scomp, a.gauss_k, a.native_sxy) == (25.0, 5.0, 5.0, 0.1, 60.0)
    assert (a.dprefix, a.max_shift, a.crf_batch, a.flow_batch) == ("davis_shift", 2, 16, 8)
    assert a.benchmark is False and a.component == "best_gt" and a.dataset == "DAVIS2016" and a.test_partition == "val"
    assert (a.buffer_dir, a.out_dir) == ("B", "O")
    a = cli.parse_post_process_args(["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R", "--dataset", "FBMS", "--sxy", "20",
                                     "--crf_batch", "0", "--flow_batch", "4", "--component", "largest", "--native_sxy", "50"])
    assert a.benchmark and (a.root_dir, a.dataset, a.sxy, a.crf_batch, a.flow_batch, a.component, a.native_sxy) == \
        ("R", "FBMS", 20.0, 0, 4, "largest", 50.0)
    assert cli._component(a) == "largest"
    for bad in (["--out_dir", "O"], ["--buffer_dir", "B", "--out_dir", "O", "--benchmark"],
                ["--buffer_dir", "B", "--out_dir", "O", "--crf_batch", "-1"], ["--buffer_dir", "B", "--out_dir", "O", "--max_shift", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_post_process_args(bad)


def test_discover_sequences(tmp_path):
    from unsupervised_detection_amd import cli
    root = tmp_path / "buf"
    for name, n in (("camel", 3), ("bear", 11), ("empty", 0)):
        d = root / "davis_shift_1" / name
        d.mkdir(parents=True)
        for k in range(1, n + 1):
            (d / ("result_%d.mat" % k)).write_bytes(b"")
        (d / "notes.txt").write_bytes(b"")
    (root / "davis_shift_1" / "stray.mat").write_bytes(b"")
    (root / "davis_shift_-1" / "other").mkdir(parents=True)
    names, lengths = cli.discover_sequences(str(root))
    assert names == ["bear", "camel"] and lengths == [11, 3]  # by name; 11 frames are counted, not sorted as text
    os.remove(str(root / "davis_shift_1" / "bear" / "result_4.mat"))
    with pytest.raises(IOError, match="hole"):
        cli.discover_sequences(str(root))
    with pytest.raises(IOError):
        cli.discover_sequences(str(root), "fbms_shift")
    (root / "x_1").mkdir()
    with pytest.raises(IOError):
        cli.discover_sequences(str(root), "x")


def test_post_process_calls_the_three_stages(tmp_path, monkeypatch):
    import json
    from unsupervised_detection_amd import cli, native_results, post_processing as PP
    d = tmp_path / "buf" / "davis_shift_1" / "bear"
    d.mkdir(parents=True)
    for k in (1, 2):
        (d / ("result_%d.mat" % k)).write_bytes(b"")
    seen = []
    monkeypatch.setattr(PP, "buffer_to_soft_score", lambda *a, **k: seen.append(("soft", a, k)))
    monkeypatch.setattr(PP, "run_crf", lambda *a, **k: seen.append(("crf", a, k)) or np.float32(0.5))
    monkeypatch.setattr(PP, "run_crf_original_resolution", lambda *a, **k: seen.append(("orig", a, k)) or {"J": {"mean": 0.25}})
    monkeypatch.setattr(native_results, "frame_lists_from_reader", lambda flags: {"bear": []})
    out = str(tmp_path / "out")
    assert cli.main(["post_process", "--buffer_dir", str(tmp_path / "buf"), "--out_dir", out]) == 0
    assert [s[0] for s in seen] == ["soft", "crf"]
    assert seen[0][1] == (str(tmp_path / "buf"), os.path.join(out, "soft"), ["bear"], [2])
    assert seen[0][2] == {"max_shift": 2, "dprefix": "davis_shift", "flow_batch": 8}
    assert seen[1][1] == (os.path.join(out, "soft"), 25.0, 5.0, 5.0, 0.1) and seen[1][2] == {"out_path": os.path.join(out, "crf_resized"), "batch": 16}
    with open(os.path.join(out, "post_process.json")) as f:
        js = json.load(f)
    assert js["iou_resized"] == 0.5 and js["sequences"] == {"bear": 2} and "benchmark" not in js
    del seen[:]
    assert cli.main(["post_process", "--buffer_dir", str(tmp_path / "buf"), "--out_dir", out, "--benchmark", "--root_dir", "R", "--crf_batch", "0",
                     "--flow_batch", "0"]) == 0
    assert [s[0] for s in seen] == ["soft", "crf", "orig"]
    assert seen[0][2]["flow_batch"] is None and seen[1][2]["batch"] is None  # 0: the per-frame paths
    assert seen[2][1] == (os.path.join(out, "crf_resized"), {"bear": []}, 60.0, 5.0, 5.0, 0.1)
    assert seen[2][2] == {"out_path": os.path.join(out, "crf_original"), "component": "best_gt", "gt_rule": "DAVIS2016"}
    with open(os.path.join(out, "post_process.json")) as f:
        assert json.load(f)["benchmark"] == {"J": {"mean": 0.25}}


def test_defaults_keep_the_per_frame_paths():
    from unsupervised_detection_amd import post_processing as PP
    sig = inspect.signature(PP.run_crf).parameters
    assert sig["batch"].default is None and sig["crf_iters"].default == 50 and sig["crf_radius"].default is None
    assert sig["out_path"].default == "./post_processed_davis"
    assert list(sig)[:5] == ["path_soft", "sxy", "srgb", "scomp", "gauss_k"]
    sig = inspect.signature(PP.propagate).parameters
    assert sig["flow_batch"].default is None and sig["w_r"].default == 0.85 and list(sig)[:3] == ["pred_masks", "images_u8", "flow_fn"]
    assert inspect.signature(PP.buffer_to_soft_score).parameters["flow_batch"].default is None
    assert inspect.signature(PP.select_unary_batch).parameters["gauss_k"].default == 0.1
    assert inspect.signature(PP.propagate_sequences).parameters["w_r"].default == 0.85
    with pytest.raises(ValueError):  # a wider Gaussian is not the batched kernel's case
        PP.select_unary_batch(None, None, None, None, gauss_k=1.0)
    with pytest.raises(ValueError):
        PP.run_crf("nowhere", 25.0, 5.0, 5.0, 0.1, batch=0)


def test_new_exports_are_in_the_library():
    from unsupervised_detection_amd._ffi import lib
    for name in ("udet_post_propagate_workspace_bytes", "udet_post_propagate_sequences", "udet_post_select_unary"):
        assert hasattr(lib, name), name
    import unsupervised_detection_amd.post_processing  # noqa: F401  (declares the argument types)
    need = lib.udet_post_propagate_workspace_bytes
    assert need(1, 1) > 0 and need(1376, 20) == 1376 * need(1, 1)  # O(frames) scalars, no per-pixel intermediate
    assert need(1376, 20) < 192 * 384 * 4 * 2  # less than two frames' worth of pixels for the whole of DAVIS val
    assert need(0, 1) == 0 and need(1, 0) == 0
    # argument errors are decided before the device is touched: they can be checked without one
    assert lib.udet_post_propagate_sequences(None, None, None, 1, None, None, 1, 4, 4, 0.15, 0.85, None, None, None, 0, None) == -5
    assert lib.udet_post_select_unary(None, None, None, None, 1, 16, None, None, None, None, None) == -5
    assert b"post_select_unary" in lib.udet_last_error()
