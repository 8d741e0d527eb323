"""CPU: the host side of the connected-component candidate selection (native_results.select_components, csrc/components.hip,
DESIGN.md 7.3) -- the numpy / scipy restatement of the rule and its tie-breaks, the C entry point's argument checks, the wrapper's table
validation, restore_results_dir(component=...) on numpy stand-ins, the two command-line flags.

components_np below restates the definition from scipy.ndimage.label alone: a component's root is the smallest row-major index among
its pixels, labels are root + 1, and the choice is made in Python integers.  tests/test_components_gpu.py compares the kernels with it
for exact equality; the mask builders of that comparison live here too, so that what they promise (component counts, which modes they
tell apart) is checked without a GPU."""
import json
import os

import numpy as np
import pytest

from test_native_results import SEQS, davis_flags, load_gt_np, make_davis_tree, restore_np, score_np

MODES = ("label", "largest", "best_gt")
RAGGED_SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (67, 131), (130, 259)]
DENSITIES = (0.3, 0.45, 0.593, 0.7)  # 0.593: the 4-connected site-percolation threshold -- components that span many tiles on thin bridges


# ------------------------------------------------------------------------------------------------------------ restatement ----
def structure(connectivity):
    return np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def roots_of(lab, k):
    """roots[c - 1] = the smallest row-major index of scipy's component c."""
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    comp, first = np.unique(flat[idx], return_index=True)
    assert comp.tolist() == list(range(1, k + 1))
    return idx[first].astype(np.int64)


def better(mode, a, b, G):
    """Candidate a = (root, area, inter) wins over b; None: no candidate.  Python integers: no overflow, no rounding."""
    if a is None:
        return False
    if b is None:
        return True
    if mode == "best_gt":
        l, r = a[2] * (b[1] + G - b[2]), b[2] * (a[1] + G - a[2])  # IoU = inter / (area + G - inter), cross-multiplied
        if l != r:
            return l > r
    if a[1] != b[1]:
        return a[1] > b[1]
    return a[0] < b[0]


def components_np(binary, gt=None, mode="largest", connectivity=8):
    """(labels int32 [H,W], selected uint8 [H,W], info [4]) of one frame."""
    from scipy import ndimage
    fg = np.asarray(binary) != 0
    lab, k = ndimage.label(fg, structure=structure(connectivity))
    roots = roots_of(lab, k)
    labels = np.where(fg, np.concatenate([[0], roots + 1])[lab], 0).astype(np.int32)
    area = np.bincount(lab.ravel(), minlength=k + 1)[1:]
    g = np.zeros_like(fg) if gt is None else np.asarray(gt) != 0
    inter = np.bincount(lab.ravel()[g.ravel()], minlength=k + 1)[1:]
    if mode == "best_gt" and gt is None:
        raise ValueError("best_gt needs the annotation")
    best = None
    if mode != "label":
        for c in range(k):
            cand = (int(roots[c]), int(area[c]), int(inter[c]))
            if better(mode, cand, best, int(g.sum())):
                best = cand
    selected = np.zeros(fg.shape, np.uint8) if best is None else (labels == best[0] + 1).astype(np.uint8)
    return labels, selected, [k] + (list(best) if best else [-1, 0, 0])


class SelectionNp(object):
    def __init__(self, binaries, info):
        self.binaries, self.info = binaries, np.asarray(info, np.int64)
        self.hw = np.array([b.shape for b in binaries], np.int32)

    def binary_sample(self, i):
        return self.binaries[i]

    def stack(self, idx):
        return np.stack([self.binaries[i] for i in idx]).astype(np.float32)[..., None]


def select_np(res, gt=None, mode="largest", connectivity=8):
    """Stand-in for select_components over the stand-ins of test_native_results (RestoredNp, GtNp)."""
    out = [components_np(res.binary_sample(i), None if gt is None else gt.sample(i), mode, connectivity) for i in range(len(res.hw))]
    return SelectionNp([o[1] for o in out], [o[2] for o in out])


# ---------------------------------------------------------------------------------------------------------- mask builders ----
def ragged_masks(density, seed=0):
    rng = np.random.default_rng([seed, int(density * 1000)])
    return [(rng.random(s) < density).astype(np.uint8) for s in RAGGED_SHAPES]


def checkerboard(h=37, w=53):
    y, x = np.mgrid[:h, :w]
    return ((y + x) % 2 == 1).astype(np.uint8)  # 980 of the 1961 pixels


def serpentine(h=67, w=131):
    """Every other row full, the full rows joined alternately at the right and the left end: one component whose union chain crosses
    every tile boundary of the frame."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def corner_blobs(tile_h, tile_w):
    """Two blobs in a (2 tile_h + 5) x (2 tile_w + 7) frame that touch only diagonally, at the pixel pairs that straddle the corner
    shared by the first four tiles: frame 0 joins NW-SE, frame 1 NE-SW.  Separate under 4-connectivity, one under 8."""
    h, w = 2 * tile_h + 5, 2 * tile_w + 7
    a, b = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    a[tile_h - 4:tile_h, tile_w - 6:tile_w] = 1
    a[tile_h:tile_h + 3, tile_w:tile_w + 9] = 1
    b[tile_h - 3:tile_h, tile_w:tile_w + 5] = 1
    b[tile_h:tile_h + 6, tile_w - 8:tile_w] = 1
    return [a, b]


def best_gt_case():
    """The 130 x 259 random mask at density 0.45 and a rectangle annotation: under 4-connectivity the largest component and the
    best-IoU component differ."""
    m = ragged_masks(0.45)[5]
    gt = np.zeros_like(m)
    gt[70:118, 30:110] = 1
    return m, gt


def tie_cases():
    """Hand-built (name, binary, gt, {mode: chosen root}): one case per tie-break of the rule."""
    out = []
    m = np.zeros((7, 12), np.uint8)
    m[1:3, 1:4] = 1   # root 13, area 6
    m[4:6, 6:9] = 1   # root 54, area 6
    g = np.zeros_like(m)
    g[2, 2:4] = 1     # inter 2 with the first
    g[4, 6:8] = 1     # inter 2 with the second: equal IoU, equal area
    out.append(("equal area", m, g, {"largest": 13, "best_gt": 13}))
    # equal IoU, different area: a = (area 3, inter 1), b = (area 10, inter 2), G = 4 (one annotated pixel lies on the background):
    # 1 * (10 + 4 - 2) = 12 = 2 * (3 + 4 - 1).  The larger area wins, whichever comes first.
    m = np.zeros((8, 16), np.uint8)
    m[1, 1:4] = 1      # root 17, area 3
    m[4:6, 5:10] = 1   # root 69, area 10
    g = np.zeros_like(m)
    g[1, 1] = 1
    g[4, 5:7] = 1
    g[7, 15] = 1
    out.append(("equal IoU, different area", m, g, {"largest": 69, "best_gt": 69}))
    m = np.zeros((8, 16), np.uint8)
    m[1, 1:11] = 1     # root 17, area 10: the larger area comes first this time
    m[4, 5:8] = 1      # root 69, area 3
    g = np.zeros_like(m)
    g[1, 1:3] = 1
    g[4, 5] = 1
    g[7, 15] = 1
    out.append(("equal IoU, larger area first", m, g, {"largest": 17, "best_gt": 17}))
    m = np.zeros((6, 10), np.uint8)
    m[0, 0:2] = 1      # root 0, area 2
    m[2:4, 3:6] = 1    # root 23, area 6
    m[5, 8:10] = 1     # root 58, area 2
    g = np.zeros_like(m)
    g[0, 9] = 1        # touches nothing: every IoU is 0, the largest wins
    out.append(("all inter 0", m, g, {"largest": 23, "best_gt": 23}))
    out.append(("empty annotation", m, np.zeros_like(m), {"largest": 23, "best_gt": 23}))
    m = np.zeros((5, 9), np.uint8)
    g = np.zeros_like(m)
    g[1:3, 2:5] = 1
    out.append(("empty mask", m, g, {"largest": -1, "best_gt": -1}))
    # the smaller component has the better IoU: the two modes differ
    m = np.zeros((10, 20), np.uint8)
    m[1:7, 1:9] = 1    # root 21, area 48, inter 2
    m[8, 12:16] = 1    # root 172, area 4, inter 4
    g = np.zeros_like(m)
    g[6, 7:9] = 1
    g[8, 12:16] = 1
    out.append(("modes differ", m, g, {"largest": 21, "best_gt": 172}))
    return out


# ----------------------------------------------------------------------------------------------------------------- tests ----
def test_roots_in_ascending_order_are_scipys_numbering():
    from scipy import ndimage
    for density in DENSITIES:
        for m in ragged_masks(density):
            for conn in (4, 8):
                lab, k = ndimage.label(m, structure=structure(conn))
                roots = roots_of(lab, k)
                assert (np.diff(roots) > 0).all(), (m.shape, conn)  # scipy's component c has the c-th smallest root
                labels, _, info = components_np(m, None, "label", conn)
                assert info == [k, -1, 0, 0] and np.array_equal(np.unique(labels[labels > 0]), roots + 1)
                rank = np.searchsorted(roots + 1, labels[labels > 0]) + 1
                assert np.array_equal(rank, lab[lab > 0])
                assert ((labels > 0) == (m != 0)).all() and (labels.ravel()[roots] == roots + 1).all()


def test_builders_keep_their_promises():
    counts = []
    for d in DENSITIES:
        for m in ragged_masks(d):
            for conn in (4, 8):
                counts.append(components_np(m, None, "label", conn)[2][0])
                assert counts[-1] >= 1 or m.size == 1, (d, m.shape, conn)  # only the 1 x 1 frame may be empty
    assert max(counts) > 1000 and min(c for c in counts if c) < 10
    assert components_np(checkerboard(), None, "label", 4)[2][0] == 980 and components_np(checkerboard(), None, "label", 8)[2][0] == 1
    s = serpentine()
    assert components_np(s, None, "largest", 4)[2] == [1, 0, int(s.sum()), 0] and components_np(s, None, "label", 8)[2][0] == 1
    from unsupervised_detection_amd.native_results import COMPONENT_TILE
    th, tw = COMPONENT_TILE
    for m in corner_blobs(th, tw):
        assert components_np(m, None, "label", 4)[2][0] == 2 and components_np(m, None, "label", 8)[2][0] == 1
    a, b = corner_blobs(th, tw)
    assert a[th - 1, tw - 1] and a[th, tw] and not a[th - 1, tw] and not a[th, tw - 1]   # NW - SE across the corner of four tiles
    assert b[th - 1, tw] and b[th, tw - 1] and not b[th - 1, tw - 1] and not b[th, tw]   # NE - SW
    m, gt = best_gt_case()
    largest, best = components_np(m, gt, "largest", 4)[2], components_np(m, gt, "best_gt", 4)[2]
    assert largest[1] != best[1] and largest[2] > best[2] and best[3] * (largest[2] + int(gt.sum()) - largest[3]) > largest[3] * (best[2] + int(gt.sum()) - best[3])


def test_every_tie_break():
    names = [c[0] for c in tie_cases()]
    assert {"equal area", "equal IoU, different area", "equal IoU, larger area first", "all inter 0", "empty mask", "modes differ"} <= set(names)
    for name, m, g, want in tie_cases():
        for conn in (4, 8):
            for mode in ("largest", "best_gt"):
                labels, sel, info = components_np(m, g, mode, conn)
                assert info[1] == want[mode], (name, mode, conn, info)
                if info[1] < 0:
                    assert info == [0, -1, 0, 0] and not sel.any()
                else:
                    assert sel.sum() == info[2] and sel.ravel()[info[1]] == 1 and (sel & (g != 0)).sum() == info[3]
                    assert np.array_equal(sel, (labels == info[1] + 1).astype(np.uint8))
    # the ties are ties: the two candidates of each case really have the equal quantities the rule then breaks
    _, m, g, _ = [c for c in tie_cases() if c[0] == "equal IoU, different area"][0]
    G = int(g.sum())
    assert 1 * (10 + G - 2) == 2 * (3 + G - 1)
    assert components_np(m, None, "largest", 8)[2] == [2, 69, 10, 0]  # without gt: inter 0
    with pytest.raises(ValueError):
        components_np(m, None, "best_gt", 8)


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd import native_results  # noqa: F401  (declares the argument types)
    from unsupervised_detection_amd._ffi import lib
    assert hasattr(lib, "udet_select_components_ragged") and hasattr(lib, "udet_components_workspace_bytes")
    assert lib.udet_components_workspace_bytes(1000, 2) >= 3 * 4 * 1000 and lib.udet_components_workspace_bytes(1000, 0) == 0
    ok = dict(binary=64, gt=128, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, connectivity=8, mode=2, labels=256, selected=512,
              info=64, ws=64, ws_bytes=1 << 20, stream=None)
    for change in (dict(connectivity=6), dict(connectivity=0), dict(mode=3), dict(mode=-1), dict(gt=None), dict(binary=None), dict(n=0),
                   dict(n=-3), dict(n=65536), dict(offsets=None), dict(hw=None), dict(info=None), dict(max_h=0), dict(max_w=0), dict(total=0),
                   dict(selected=None), dict(selected=64), dict(mode=1, selected=None), dict(ws=None), dict(ws_bytes=64), dict(ws=68),
                   dict(labels=258)):
        a = dict(ok, **change)
        rc = lib.udet_select_components_ragged(a["binary"], a["gt"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"],
                                               a["connectivity"], a["mode"], a["labels"], a["selected"], a["info"], a["ws"], a["ws_bytes"],
                                               a["stream"])
        assert rc == -5 and b"select_components_ragged" in lib.udet_last_error(), change


def test_wrapper_validates_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd.native_results import GtBatch, check_component_tables, select_components
    hw = [(30, 53), (13, 26)]
    total = 30 * 53 + 13 * 26
    off, size = check_component_tables([0, 30 * 53], hw, total)
    assert off.dtype == np.int64 and size.dtype == np.int32 and size.tolist() == [[30, 53], [13, 26]]
    buf = torch.zeros(total, dtype=torch.uint8)  # a host tensor: anything that got past the validation would fail on it, not launch

    def bad(match, **kw):
        args = dict(binary=buf, offsets=[0, 30 * 53], hw=hw)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            select_components(**args)
    bad("overlap", offsets=[0, 30 * 53 - 1])
    bad("overlap", offsets=[13 * 26 - 5, 0])
    bad("outside the packed buffer", offsets=[0, 30 * 53 + 1])
    bad("outside the packed buffer", offsets=[-1, 30 * 53])
    bad("outside the packed buffer", binary=buf[:-1])
    bad("at least 1x1", hw=[(30, 53), (0, 26)])
    bad("one \\(H, W\\) per offset", hw=[(30, 53)])
    bad("mode", mode="smallest")
    bad("connectivity", connectivity=6)
    bad("best_gt", mode="best_gt")
    bad("packed like binary", gt=buf[:-1])
    bad("packed like the masks", gt=GtBatch(buf, np.array([0, 30 * 53]), np.array([(30, 53), (26, 13)])))
    bad("uint8", binary=buf.float())
    bad("offsets and sizes", offsets=None)
    bad("CUDA", mode="largest")  # everything valid but the host tensor: refused before any call into the library


def _tree_files(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                data = fh.read()
            out[os.path.relpath(os.path.join(d, f), root)] = data[128:] if f.endswith(".mat") else data  # the MAT header carries the time
    return out


def speckled_restore_np(masks, native_hw, crop=0.9, threshold=None):
    """restore_np plus specks: every restored binary mask gets a few isolated pixels and a small second blob inside the crop, so that a
    frame has several components and the selection has something to remove."""
    r = restore_np(masks, native_hw, crop, threshold)
    for b in r.binaries:
        if b is not None and min(b.shape) >= 12:
            b[2, 4] = b[b.shape[0] - 3, b.shape[1] - 5] = 1
            b[b.shape[0] - 5:b.shape[0] - 3, 5:8] = 1
    return r


def run_component_tree(tmp_path, name, mixed=False, **kw):
    from unsupervised_detection_amd.native_results import frame_lists_from_reader, restore_results_dir
    root, res, masks = make_davis_tree(tmp_path / name, mixed)
    out = str(tmp_path / name / "native")
    args = dict(restore=speckled_restore_np, load_gt=load_gt_np, score=score_np, batch=2, verbose=False)
    args.update(kw)
    return out, restore_results_dir(res, frame_lists_from_reader(davis_flags(root)), out, **args), masks


@pytest.mark.parametrize("mixed", [False, True])
def test_restore_results_dir_with_selection(tmp_path, mixed):
    import scipy.io as sio
    from PIL import Image
    from test_native_results import frame_hw
    out0, js0, masks = run_component_tree(tmp_path, "plain", mixed)
    out1, js1, _ = run_component_tree(tmp_path, "largest", mixed, component="largest", select=select_np)
    out2, js2, _ = run_component_tree(tmp_path, "best", mixed, component="best_gt", connectivity=4, select=select_np)
    assert "component" not in js0 and "components_mean" not in js0["sequences"]["bear"]
    for out, js, mode, conn in ((out1, js1, "largest", 8), (out2, js2, "best_gt", 4)):
        assert js["component"] == mode and js["connectivity"] == conn
        with open(os.path.join(out, "native_eval.json")) as f:
            assert json.load(f) == json.loads(json.dumps(js))
        for seq in SEQS:
            ncs = []
            for k in range(3):
                H, W = frame_hw(seq, k, mixed)
                r = speckled_restore_np(masks[seq][k][None], [(H, W)], 0.9, 0.5)
                with Image.open(os.path.join(os.path.dirname(out), "DAVIS", "Annotations", "480p", seq, "%05d.png" % k)) as im:
                    gt = (np.asarray(im) / 255.0 > 0.1).astype(np.uint8)
                _, want, info = components_np(r.binary_sample(0), gt, mode, conn)
                ncs.append(info[0])
                assert info[0] >= 3 and want.sum() == info[2] < r.binary_sample(0).sum()  # the specks are gone
                with Image.open(os.path.join(out, seq, "%05d.png" % k)) as im:
                    assert np.array_equal(np.asarray(im), want * 255)
                mat = sio.loadmat(os.path.join(out, seq, "result_%d.mat" % (k + 1)))
                plain = sio.loadmat(os.path.join(out0, seq, "result_%d.mat" % (k + 1)))
                assert np.array_equal(mat["mask"], want) and mat["mask"].dtype == np.uint8
                assert components_np(mat["mask"], None, "label", conn)[2][0] == 1  # only the chosen component
                assert np.array_equal(mat["soft_mask"], plain["soft_mask"]) and np.array_equal(mat["gt_mask"], plain["gt_mask"])
            assert js["sequences"][seq]["components_mean"] == float(np.mean(ncs))
        assert js["J"]["mean"] >= js0["J"]["mean"]  # the specks lie outside the annotation: dropping them cannot lower J


def test_component_none_changes_nothing(tmp_path):
    """component=None (the default): nothing is called and every file equals a run of the same call without the argument."""
    def never(*a, **k):
        raise AssertionError("select called with component=None")
    out0, js0, _ = run_component_tree(tmp_path, "a", True)
    out1, js1, _ = run_component_tree(tmp_path, "b", True, component=None, connectivity=4, select=never)
    assert js0 == js1
    f0, f1 = _tree_files(out0), _tree_files(out1)
    assert sorted(f0) == sorted(f1) and len(f0) == 13 and all(f0[k] == f1[k] for k in f0)
    with pytest.raises(ValueError):
        run_component_tree(tmp_path, "c", component="smallest", select=select_np)
    with pytest.raises(ValueError):
        run_component_tree(tmp_path, "d", component="largest", connectivity=6, select=select_np)


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    a = cli.parse_restore_results_args(base)
    assert (a.component, a.connectivity) == ("none", 8) and cli._component(a) is None
    a = cli.parse_restore_results_args(base + ["--component", "best_gt", "--connectivity", "4"])
    assert (a.component, a.connectivity) == ("best_gt", 4) and cli._component(a) == "best_gt"
    assert cli._component(cli.parse_restore_results_args(base + ["--component", "largest"])) == "largest"
    for bad in (["--component", "smallest"], ["--connectivity", "6"]):
        with pytest.raises(SystemExit):
            cli.parse_restore_results_args(base + bad)
    assert (default_flags().component, default_flags().connectivity) == ("none", 8)
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D"]
    f = parse_flags(native + ["--component", "largest", "--connectivity", "4"])
    assert (f.component, f.connectivity) == ("largest", 4)
    cli.check_native_flags(f)
    for bad in (["--component", "smallest"], ["--connectivity", "5"]):
        with pytest.raises(SystemExit):
            cli.check_native_flags(parse_flags(native + bad))
    assert "--component" in cli.__doc__ and "--connectivity" in cli.__doc__
