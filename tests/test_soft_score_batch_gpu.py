"""GPU: udet_post_soft_score_batch (csrc/soft_score.hip) through the C ABI -- bit for bit against the per-frame path
(post_processing.soft_score) and against the CPU oracle with the real Pillow (oracle_post.soft_score), at sizes below, at and across the
64 x 16 tile; other ensemble sizes; independence of the batch, its order and the run; argument errors that enqueue nothing; and
buffer_to_soft_score(score_batch=) against the per-frame driver, file for file."""
import os

import numpy as np
import pytest

from oracle import oracle_post as P
from test_soft_score_batch import CROPS, ensemble

pytestmark = pytest.mark.gpu

GUARD = 64  # float64 elements on both sides of pred_mask
FILL = -7.0


@pytest.fixture(scope="module")
def PP():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import post_processing as pp
    return pp


def call_abi(PP, preds, crops=CROPS, base_crop=90.0, san_t=0.6, **change):
    """One udet_post_soft_score_batch call on a guarded output buffer -> (status, whole buffer as numpy, n * H * W).  change: arguments
    replaced after everything valid was set up (the argument-error cases)."""
    import torch
    from unsupervised_detection_amd._ffi import lib
    t = torch.from_numpy(np.ascontiguousarray(preds)).cuda()
    n, _, ns, nc, H, W = t.shape
    geom, coef = PP._soft_score_tables(ns, crops, base_crop, H, W, t.device)
    buf = torch.full((2 * GUARD + n * H * W,), FILL, dtype=torch.float64, device="cuda")
    ws = PP.workspace(lib.udet_post_soft_score_workspace_bytes(n, ns, nc, H, W), 16, t.device)
    a = dict(masks=t.data_ptr(), n=n, ns=ns, nc=nc, h=H, w=W, geom=geom.data_ptr(), coef=coef.data_ptr(), san_t=san_t,
             pred=buf.data_ptr() + 8 * GUARD, ws=ws.data_ptr(), ws_bytes=ws.numel())
    for k, v in change.items():
        a[k] = v(a[k]) if callable(v) else v
    status = lib.udet_post_soft_score_batch(a["masks"], a["n"], a["ns"], a["nc"], a["h"], a["w"], a["geom"], a["coef"], a["san_t"], a["pred"],
                                            a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, buf.cpu().numpy(), n * H * W


def batch(PP, preds, crops=CROPS, base_crop=90.0):
    """The call's result [n, H, W] (numpy float64), with the guard elements checked."""
    status, buf, size = call_abi(PP, preds, crops, base_crop)
    assert status == 0
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + size:] == FILL).all()  # nothing outside pred_mask
    return buf[GUARD:GUARD + size].reshape(preds.shape[0], preds.shape[4], preds.shape[5])


def branches(n):
    """Slots (frame, direction, shift index, crop index) that cover the sanity rule's four branches within frames 0 and 1 (the batch of 2 at
    192 x 384 has no more): all-ones masks (border mean 1) and one constant mask (border mean 0.25: clean, cscale == 0)."""
    edges = [(0, 0, 0, 1),                 # backward-only bad on the identity row
             (0, 1, 1, 1),                 # forward-only bad on shift 2 / crop 90 (bytescale only)
             (0, 0, 1, 3),                 # backward-only bad, crop 100
             (1, 0, 0, 0), (1, 1, 0, 0),   # both bad, crop 85
             (1, 1, 0, 1),                 # forward-only bad on the identity row
             (1, 0, 1, 1), (1, 1, 1, 1),   # both bad on shift 2 / crop 90
             (1, 0, 1, 2)]                 # backward-only bad, crop 95
    const = [(0, 1, 0, 2)]
    if n > 2:
        edges += [(2, 0, 0, 1), (2, 1, 0, 1)]  # both bad on the identity row
        const += [(2, 0, 1, 1), (2, 1, 0, 3)]
    return edges, const


@pytest.mark.parametrize("H, W, n", [(17, 23, 3), (24, 40, 3), (70, 131, 3), (192, 384, 2)])
def test_equals_the_per_frame_path_and_the_oracle(PP, H, W, n):
    """17 x 23: patches narrower than a tile, a zero row offset; 70 x 131: tile edges crossed in both directions at odd sizes; 192 x 384: the
    real tile counts."""
    import torch
    edges, const = branches(n)
    preds = ensemble(n, 2, 4, H, W, seed=H, edges=edges, const=const)
    got = batch(PP, preds)
    high = PP.soft_score_batch(preds)  # the Python entry point: the same call
    assert high.dtype == torch.float64 and tuple(high.shape) == (n, H, W) and np.array_equal(high.cpu().numpy(), got)
    for i in range(n):
        pb, pf = [list(row) for row in preds[i, 0]], [list(row) for row in preds[i, 1]]
        assert torch.equal(high[i], PP.soft_score(pb, pf, CROPS, 90.0, (H, W))), i
        assert np.array_equal(got[i], P.soft_score(pb, pf, CROPS, 90.0, base_hw=(H, W))), i
        assert got[i].min() == 0.0 and abs(got[i].max() - 1.0) < 1e-5


@pytest.mark.parametrize("ns, crops", [(1, (85, 100)), (3, (90,))])
def test_other_ensemble_sizes(PP, ns, crops):
    """One shift without the base crop: no identity row.  Three shifts of the base crop alone: one identity row, two bytescale-only rows."""
    H, W, n = 24, 40, 2
    preds = ensemble(n, ns, len(crops), H, W, seed=7 + ns, edges=[(0, 0, 0, 0), (1, 1, ns - 1, len(crops) - 1)], const=[(1, 0, 0, 0)])
    got = batch(PP, preds, crops)
    for i in range(n):
        ref = P.soft_score([list(r) for r in preds[i, 0]], [list(r) for r in preds[i, 1]], crops, 90.0, base_hw=(H, W))
        assert np.array_equal(got[i], ref), i


def test_tile_reads_more_than_one_strip(PP):
    """Crop 20 against base crop 90 shrinks 96 rows to int(96 * 20 / 90) = 21: the 16 patch rows of the first tile read more than 64 window
    rows, a second strip of the horizontal intermediate (every other shape here stays inside the first)."""
    import torch
    H, W, n, crops = 96, 40, 2, (20, 90)
    preds = ensemble(n, 1, 2, H, W, seed=31)
    got = batch(PP, preds, crops)
    high = PP.soft_score_batch(preds, crops)
    for i in range(n):
        pb, pf = [list(row) for row in preds[i, 0]], [list(row) for row in preds[i, 1]]
        assert np.array_equal(got[i], P.soft_score(pb, pf, crops, 90.0, base_hw=(H, W))), i
        assert torch.equal(high[i], PP.soft_score(pb, pf, crops, 90.0, (H, W))), i


def test_independent_of_the_batch_and_the_run(PP):
    H, W, n = 24, 40, 5
    edges, const = branches(3)
    preds = ensemble(n, 2, 4, H, W, seed=3, edges=edges + [(4, 1, 1, 0)], const=const)
    whole = batch(PP, preds)
    assert np.array_equal(batch(PP, preds), whole)  # the same call twice
    assert np.array_equal(batch(PP, np.ascontiguousarray(preds[::-1]))[::-1], whole)
    for i in range(n):
        assert np.array_equal(batch(PP, preds[i:i + 1])[0], whole[i]), i


def test_argument_errors_enqueue_nothing(PP):
    from unsupervised_detection_amd._ffi import lib
    preds = ensemble(2, 2, 4, 24, 40, seed=5)
    cases = [dict(n=0), dict(ns=0), dict(nc=0), dict(h=0), dict(w=0), dict(n=-1), dict(h=3), dict(w=3), dict(masks=None), dict(geom=None),
             dict(coef=None), dict(pred=None), dict(ws=None), dict(san_t=float("nan")), dict(san_t=float("-inf")),
             dict(ws_bytes=lambda b: lib.udet_post_soft_score_workspace_bytes(2, 2, 4, 24, 40) - 1), dict(ws=lambda p: p + 4)]
    for change in cases:
        status, buf, _ = call_abi(PP, preds, **change)
        assert status == -5 and b"post_soft_score_batch" in lib.udet_last_error(), change
        assert (buf == FILL).all(), change
    status, buf, size = call_abi(PP, preds)  # ... and the call they were derived from is a good one
    assert status == 0 and (buf[GUARD:GUARD + size] != FILL).all()


def test_buffer_to_soft_score_in_groups(PP, tmp_path):
    """Two sequences of 3 and 2 frames, score_batch=2: groups of 2 + 1 and 2.  The same files, and every array of every file equal."""
    import scipy.io as sio
    H, W, crops = 24, 40, list(range(85, 101, 5))
    seqs, rng = {"bear": 3, "camel": 2}, np.random.default_rng(11)
    buf = tmp_path / "buf"
    for s, (name, num) in enumerate(seqs.items()):
        preds = ensemble(num, 2, 4, H, W, seed=20 + s, edges=[(0, 0, 0, 1), (1, 1, 1, 1), (1, 0, 0, 3), (1, 1, 0, 3)], const=[(0, 1, 1, 2)])
        for k in range(num):
            for d, sign in ((0, -1), (1, 1)):
                for si in (0, 1):
                    folder = buf / ("davis_shift_%d" % (sign * (si + 1))) / name
                    folder.mkdir(parents=True, exist_ok=True)
                    mat = {}
                    for ci, c in enumerate(crops):
                        mat["pred_mask_%03d" % c] = preds[k, d, si, ci][None, :, :, None]
                        mat["img_1_%03d" % c] = (rng.random((H, W, 3)) - 0.5).astype(np.float32)
                        mat["gt_mask_%03d" % c] = (preds[k, d, si, ci] > 0.5).astype(np.float32)
                    sio.savemat(str(folder / ("result_%d.mat" % (k + 1))), mat)
    flow = np.stack([np.full((H, W), 0.75, np.float32), np.full((H, W), -0.5, np.float32)], -1)
    outs = []
    for score_batch in (None, 2):
        out = tmp_path / ("soft_%s" % score_batch)
        PP.buffer_to_soft_score(str(buf), str(out), list(seqs), list(seqs.values()), max_shift=2, flow_fn=lambda a, b: flow, score_batch=score_batch)
        outs.append(out)
    listing = [sorted(os.path.relpath(os.path.join(d, f), str(o)) for d, _, fs in os.walk(str(o)) for f in fs) for o in outs]
    assert listing[0] == listing[1] and len(listing[0]) == 5
    for rel in listing[0]:
        a, b = sio.loadmat(str(outs[0] / rel)), sio.loadmat(str(outs[1] / rel))
        keys = sorted(k for k in a if not k.startswith("__"))
        assert keys == sorted(k for k in b if not k.startswith("__")) == ["gt_mask", "img1", "pred_mask", "running_avg_b", "running_avg_f"]
        for k in keys:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (rel, k)
