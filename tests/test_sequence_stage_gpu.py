"""GPU: the batched sequence stage (csrc/sequence.hip) against oracle.oracle_post and against the per-frame paths it
stands beside.

Bounds.  Propagation: bytes -- the kernels share every expression with udet_post_remap / udet_post_blend (csrc/post_remap.h), which
tests/test_post_processing.py already holds to the oracle bit for bit; max is exact in any order.  Unary: 2 float32 ulp -- both sides
round a float64 -log to float32 and the two log implementations differ (measured: see profiles/NOTES.md).  run_crf: labels equal to
oracle_post.refine's on every pixel where the oracle's |Q1 - 0.5| > 1e-5, at most 1e-3 H W pixels excluded (the conditions of
tests/test_crf_native_gpu.py; on these inputs the oracle alone excludes none, checked on the CPU when the inputs were chosen and
asserted below).  PWCFlow.batch: 2e-3 max|flow| against the per-pair call (each side within the project's 1e-3 parity bound of the
oracle)."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle_post as P
from test_crf_native import scene
from test_sequence_stage import soft_mask

pytestmark = pytest.mark.gpu

ERR_ARG = -5


@pytest.fixture(scope="module")
def PP():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import post_processing as pp
    return pp


# ------------------------------------------------------------------------------------------------------------ propagation ----
def make_sequences(H, W, lens, seed):
    """masks [total,H,W], flow_prev, flow_next [total,H,W,2]: flows of sigma 3 px, the first rows of every third frame shifted by +40 (they
    sample outside), the second frame's mask all zero (max = 0)."""
    rng = np.random.default_rng(seed)
    total = sum(lens)
    masks = np.stack([soft_mask(H, W, seed + k) for k in range(total)])
    if total > 1:
        masks[1] = 0.0
    fp, fn = (rng.normal(0, 3.0, (total, H, W, 2)).astype(np.float32) for _ in range(2))
    fp[::3, :5] += 40.0
    fn[1::3, :5] += 40.0
    return masks, fp, fn


def oracle_chain(masks, fp, fn, w_r=0.85):
    """oracle_post.propagate_step along one sequence, both directions."""
    n = len(masks)
    f, b = [None] * n, [None] * n
    f[0] = masks[0]
    for k in range(1, n):
        f[k] = P.propagate_step(f[k - 1], masks[k - 1], fp[k], w_r)
    b[n - 1] = masks[n - 1]
    for k in range(n - 2, -1, -1):
        b[k] = P.propagate_step(b[k + 1], masks[k + 1], fn[k], w_r)
    return np.stack(f).astype(np.float32), np.stack(b).astype(np.float32)


_cases = {}


def case(name):
    """(masks, flow_prev, flow_next, lens, oracle avg_f, oracle avg_b) of a case, built once and shared."""
    if name not in _cases:
        H, W, lens, seed = {"mixed": (37, 53, [1, 2, 5], 11), "frame": (192, 384, [4], 23)}[name]
        m, fp, fn = make_sequences(H, W, lens, seed)
        want_f, want_b, base = [], [], 0
        for n in lens:
            f, b = oracle_chain(m[base:base + n], fp[base:base + n], fn[base:base + n])
            want_f.append(f), want_b.append(b)
            base += n
        _cases[name] = (m, fp, fn, lens, np.concatenate(want_f), np.concatenate(want_b))
    return _cases[name]


def run_sequences(PP, m, fp, fn, lens):
    f, b = PP.propagate_sequences(torch.from_numpy(m).cuda(), torch.from_numpy(fp).cuda(), torch.from_numpy(fn).cuda(), lens)
    return f.cpu().numpy(), b.cpu().numpy()


@pytest.mark.parametrize("name", ["mixed", "frame"])
def test_propagation_equals_the_oracle_and_the_per_frame_path_bit_for_bit(PP, name):
    m, fp, fn, lens, want_f, want_b = case(name)
    got_f, got_b = run_sequences(PP, m, fp, fn, lens)
    assert got_f.dtype == np.float32 and got_f.shape == m.shape == got_b.shape
    print(name, "max|avg_f - oracle| %.3g" % np.abs(got_f - want_f).max(), "max|avg_b - oracle| %.3g" % np.abs(got_b - want_b).max())
    assert got_f.tobytes() == want_f.tobytes() and got_b.tobytes() == want_b.tobytes()
    assert np.isfinite(got_f).all() and got_f.max() > 0.5  # something is propagated
    if name == "mixed":
        assert got_f[0].tobytes() == m[0].tobytes() == got_b[0].tobytes()  # a sequence of one frame: the output is the input
        assert not got_f[1].any() and not got_f[2].any() and got_b[1].any()  # the all-zero mask starts the second sequence: every max is 0
    # the existing per-step path with the same flows
    base = 0
    for n in lens:
        imgs = [np.array([k]) for k in range(n)]

        def flow_fn(a, b, base=base):
            ka, kb = int(a[0]), int(b[0])
            return (fp if kb == ka - 1 else fn)[base + ka]
        fwd, bwd = PP.propagate(list(m[base:base + n]), imgs, flow_fn)
        for k in range(n):
            assert fwd[k].cpu().numpy().tobytes() == got_f[base + k].tobytes(), (name, base, k)
            assert bwd[k].cpu().numpy().tobytes() == got_b[base + k].tobytes(), (name, base, k)
        base += n


def test_propagation_does_not_depend_on_the_batch_or_the_run(PP):
    m, fp, fn, lens, want_f, want_b = case("mixed")
    got_f, got_b = run_sequences(PP, m, fp, fn, lens)
    again_f, again_b = run_sequences(PP, m, fp, fn, lens)
    assert again_f.tobytes() == got_f.tobytes() and again_b.tobytes() == got_b.tobytes()
    base = 0
    for n in lens:
        s = slice(base, base + n)
        f1, b1 = run_sequences(PP, m[s], fp[s], fn[s], [n])
        assert f1.tobytes() == got_f[s].tobytes() and b1.tobytes() == got_b[s].tobytes(), n
        base += n
    # in another order
    order = [2, 0, 1]
    starts = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([np.arange(starts[i], starts[i + 1]) for i in order])
    f2, b2 = run_sequences(PP, m[idx], fp[idx], fn[idx], [lens[i] for i in order])
    assert f2.tobytes() == got_f[idx].tobytes() and b2.tobytes() == got_b[idx].tobytes()


def test_propagation_argument_errors_enqueue_nothing(PP):
    from unsupervised_detection_amd._ffi import lib
    m, fp, fn, lens, want_f, _ = case("mixed")
    total, H, W = m.shape
    dm, dfp, dfn = (torch.from_numpy(a).cuda() for a in (m, fp, fn))
    first = torch.tensor([0, 1, 3], dtype=torch.int32, device="cuda")
    length = torch.tensor(lens, dtype=torch.int32, device="cuda")
    guard = 64
    outs = [torch.full((4 * (total * H * W + guard),), 0xA5, dtype=torch.uint8, device="cuda").view(torch.float32) for _ in range(2)]
    need = int(lib.udet_post_propagate_workspace_bytes(total, 3))
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    good = dict(masks=dm.data_ptr(), fp=dfp.data_ptr(), fn=dfn.data_ptr(), n_seq=3, first=first.data_ptr(), length=length.data_ptr(), total=total,
                h=H, w=W, avg_f=outs[0].data_ptr(), avg_b=outs[1].data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.udet_post_propagate_sequences(a["masks"], a["fp"], a["fn"], a["n_seq"], a["first"], a["length"], a["total"], a["h"], a["w"],
                                                 float(np.float32(1 - 0.85)), float(np.float32(0.85)), a["avg_f"], a["avg_b"], a["ws"],
                                                 a["ws_bytes"], None)
    bad = [dict(n_seq=0), dict(n_seq=65536), dict(h=0), dict(w=0), dict(total=0), dict(h=1 << 16, w=1 << 15), dict(masks=None), dict(fp=None),
           dict(fn=None), dict(first=None), dict(length=None), dict(avg_f=None), dict(avg_b=None), dict(ws=None), dict(ws_bytes=need - 1),
           dict(ws=ws.data_ptr() + 4), dict(avg_b=outs[0].data_ptr()), dict(fp=dfp.data_ptr() + 4), dict(fn=dfn.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
        assert lib.udet_last_error()
    torch.cuda.synchronize()
    assert all((o.view(torch.uint8) == 0xA5).all() for o in outs) and (ws == 0xA5).all()
    assert call() == 0
    torch.cuda.synchronize()
    for o in outs:  # the guard words after the outputs are untouched, the outputs written
        assert (o[total * H * W:].view(torch.uint8) == 0xA5).all()
    assert (ws[need:] == 0xA5).all()
    assert outs[0][:total * H * W].cpu().numpy().tobytes() == want_f.tobytes()
    # the Python entry validates the tables and shapes on the host
    with pytest.raises(ValueError):
        PP.propagate_sequences(dm, dfp, dfn, [1, 2, 4])
    with pytest.raises(ValueError):
        PP.propagate_sequences(dm, dfp, dfn, [1, 2, 5, 0])
    with pytest.raises(ValueError):
        PP.propagate_sequences(dm, dfp[:, :, :, :1].contiguous(), dfn, lens)


# ----------------------------------------------------------------------------------------------------- choice and unary ----
def select_frames():
    """pred, avg_f, avg_b, gt [5,24,32] and the choices they are built for."""
    H, W = 24, 32
    a = soft_mask(H, W, 3)
    gt = (a > 0.5).astype(np.float32)
    mid, low = np.roll(a, 5, 1), np.roll(a, 11, 1)  # the same blob further and further from the annotation
    z = np.zeros_like(a)
    frames = [(low, mid, a, gt, 2),      # three different scores, the backward average wins
              (a, low, mid, gt, 0),      # three different scores, the raw mask wins
              (mid, mid, mid, gt, 0),    # identical arrays: identical scores, the first rule holds
              (low, a, a, gt, 1),        # f == b above m: the second rule holds before the third
              (z, a, mid, z, 0)]         # an empty annotation: every score is 0, the raw mask -- constant zero -- is taken
    return tuple(np.stack([f[i] for f in frames]) for i in range(4)) + ([f[4] for f in frames],)


def test_select_unary_batch(PP):
    pred, af, ab, gt, built = select_frames()
    n, H, W = pred.shape
    choice, scores, soft, unary = PP.select_unary_batch(*(torch.from_numpy(x).cuda() for x in (pred, af, ab, gt)))
    assert choice.dtype == torch.int32 and scores.dtype == torch.float64 and soft.dtype == torch.float32 and unary.dtype == torch.float32
    assert tuple(scores.shape) == (n, 3) and tuple(soft.shape) == (n, H, W) and tuple(unary.shape) == (2, n * H * W)
    choice, scores, soft, unary = choice.cpu().numpy(), scores.cpu().numpy(), soft.cpu().numpy(), unary.cpu().numpy().reshape(2, n, H, W)
    worst = 0
    for i in range(n):
        want_mask, want = P.select_candidate(pred[i], af[i], ab[i], gt[i])
        s = [float(np.sum(p * gt[i]) / (np.sum(p) + 1e-8)) for p in (pred[i], af[i], ab[i])]
        if i in (0, 1):
            assert min(abs(s[0] - s[1]), abs(s[0] - s[2]), abs(s[1] - s[2])) > 1e-3, s
        if i == 3:
            assert s[1] == s[2] and s[1] - s[0] > 1e-3
        assert choice[i] == want == built[i], (i, choice[i], want, s)
        assert np.abs(scores[i] - s).max() < 1e-5
        assert soft[i].tobytes() == want_mask.tobytes()
        ref = P.unary_from_mask(soft[i], 0.1)
        ulp = int(np.abs(unary[:, i].view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max())
        worst = max(worst, ulp)
    print("select_unary_batch: worst unary difference against oracle_post.unary_from_mask: %d float32 ulp" % worst)
    assert worst <= 2
    assert scores[2, 0] == scores[2, 1] == scores[2, 2] and (scores[4] == 0).all()
    # a constant-zero candidate: U = 1e-6 everywhere
    assert (unary[1, 4] == np.float32(-np.log(1e-6))).all() and (unary[0, 4] == np.float32(-np.log(1.0 - 1e-6))).all()
    with pytest.raises(ValueError):
        PP.select_unary_batch(*(torch.from_numpy(x).cuda() for x in (pred, af, ab, gt[:4])))


def test_select_unary_argument_errors_enqueue_nothing(PP):
    from unsupervised_detection_amd._ffi import lib
    pred, af, ab, gt, _ = select_frames()
    n, hw = pred.shape[0], pred.shape[1] * pred.shape[2]
    d = [torch.from_numpy(x).cuda() for x in (pred, af, ab, gt)]

    def guarded(count, dtype):
        return torch.full((count * torch.empty(0, dtype=dtype).element_size(),), 0xA5, dtype=torch.uint8, device="cuda").view(dtype)
    choice, scores, soft, unary = guarded(n + 8, torch.int32), guarded(3 * n + 8, torch.float64), guarded(n * hw + 8, torch.float32), \
        guarded(2 * n * hw + 8, torch.float32)
    good = dict(pred=d[0].data_ptr(), af=d[1].data_ptr(), ab=d[2].data_ptr(), gt=d[3].data_ptr(), n=n, hw=hw, choice=choice.data_ptr(),
                scores=scores.data_ptr(), soft=soft.data_ptr(), unary=unary.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.udet_post_select_unary(a["pred"], a["af"], a["ab"], a["gt"], a["n"], a["hw"], a["choice"], a["scores"], a["soft"], a["unary"],
                                          None)
    for kw in [dict(n=0), dict(n=65536), dict(hw=0), dict(pred=None), dict(af=None), dict(ab=None), dict(gt=None), dict(choice=None),
               dict(scores=None), dict(soft=None), dict(unary=None), dict(scores=scores.data_ptr() + 4)]:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    outs = (choice, scores, soft, unary)
    assert all((o.view(torch.uint8) == 0xA5).all() for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    for o, used in zip(outs, (n, 3 * n, n * hw, 2 * n * hw)):
        assert (o[used:].view(torch.uint8) == 0xA5).all() and not (o[:used].view(torch.uint8) == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------------ run_crf ----
CRF = dict(sxy=3.0, srgb=13.0, scomp=5.0, gauss_k=0.1, iters=5, radius=6)
_folder = {}


def crf_folder(tmp_path_factory):
    """A soft-score folder of 2 sequences x 3 frames at 24 x 32 and, per frame, the oracle's (choice mask, labels, sure pixels)."""
    if not _folder:
        import scipy.io as sio
        H, W = 24, 32
        root = str(tmp_path_factory.mktemp("soft"))
        want = {}
        for si, seq in enumerate(("bear", "camel")):
            os.makedirs(os.path.join(root, seq))
            for k in range(3):
                img, soft = scene(H, W, 100 * si + k + 1)
                gt = (soft > 0.5).astype(np.float32)
                cands = [soft, np.roll(soft, 3, 1), np.roll(soft, -4, 0)]
                pm, pf, pb = (cands[(j + k) % 3] for j in range(3))  # the winner is another candidate in every frame
                sio.savemat(os.path.join(root, seq, "result_%d.mat" % (k + 1)),
                            {"pred_mask": pm, "running_avg_f": pf, "running_avg_b": pb, "gt_mask": gt, "img1": img})
                mask, c = P.select_candidate(pm, pf, pb, gt)
                Q = P.dense_crf(P.unary_from_mask(mask, CRF["gauss_k"]), img, CRF["sxy"], CRF["srgb"], CRF["scomp"], CRF["iters"], CRF["radius"])
                labels, _ = P.refine(mask, img, CRF["gauss_k"], CRF["sxy"], CRF["srgb"], CRF["scomp"], gt, CRF["iters"], CRF["radius"])
                want[(seq, k + 1)] = (mask, c, labels, np.abs(Q[1] - 0.5) > 1e-5, gt)
        _folder.update(root=root, want=want, hw=(H, W))
    return _folder


@pytest.mark.parametrize("batch", [4, None])
def test_run_crf_batched_and_per_frame_against_the_oracle(PP, tmp_path_factory, tmp_path, batch):
    import scipy.io as sio
    folder = crf_folder(tmp_path_factory)
    H, W = folder["hw"]
    out = str(tmp_path / "out")
    avg = PP.run_crf(folder["root"], CRF["sxy"], CRF["srgb"], CRF["scomp"], CRF["gauss_k"], out_path=out, batch=batch, crf_iters=CRF["iters"],
                     crf_radius=CRF["radius"])
    ious, choices = [], set()
    for (seq, k), (mask, c, labels, sure, gt) in folder["want"].items():
        mat = sio.loadmat(os.path.join(out, seq, "result_%d.mat" % k))
        assert set(mat) >= {"gt_mask", "soft_mask", "mask"}
        assert all(mat[key].dtype == np.float32 and mat[key].shape == (H, W) for key in ("gt_mask", "soft_mask", "mask"))
        assert mat["soft_mask"].tobytes() == mask.tobytes(), (seq, k)  # the oracle's choice
        assert np.array_equal(mat["gt_mask"], gt)
        assert (~sure).sum() <= 1e-3 * H * W  # the oracle alone stays inside the cap on these inputs
        assert set(np.unique(mat["mask"])) <= {0.0, 1.0} and 0 < mat["mask"].mean() < 1
        assert np.array_equal(mat["mask"][sure], labels[sure]), (seq, k, int((mat["mask"] != labels).sum()))
        g, bm = mat["gt_mask"] > 0.1, mat["mask"] > 0.1
        ious.append(float(np.sum(g & bm)) / float(np.sum(g | bm)))
        choices.add(c)
    assert choices == {0, 1, 2}
    print("run_crf(batch=%s): average IoU %.6f" % (batch, float(avg)))
    assert abs(float(avg) - float(np.mean(ious))) < 1e-6


# --------------------------------------------------------------------------------------------------------------------- flows ----
def test_pwcflow_batch_and_propagate_with_flow_batch(PP):
    rng = np.random.default_rng(41)
    H, W = 64, 128
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    flow = PP.PWCFlow()
    a, b = imgs[:3], imgs[1:]
    got = flow.batch(a, b, batch=2)
    assert tuple(got.shape) == (3, H, W, 2) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    for i in range(3):
        one = flow(a[i], b[i])
        scale = float(one.abs().max())
        err = float((got[i] - one).abs().max())
        print("pair %d: max|flow| %.4g, max|batch - single| %.3g" % (i, scale, err))
        assert scale > 0 and err <= 2e-3 * scale, (i, err, scale)
    masks = [soft_mask(H, W, 50 + k) for k in range(3)]
    fwd, bwd = PP.propagate(masks, imgs[:3], flow, flow_batch=2)
    assert len(fwd) == len(bwd) == 3
    for t in fwd + bwd:
        assert tuple(t.shape) == (H, W) and t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert fwd[0].cpu().numpy().tobytes() == masks[0].tobytes() and bwd[2].cpu().numpy().tobytes() == masks[2].tobytes()
    with pytest.raises(ValueError):  # a plain function has no batch method
        PP.propagate(masks, imgs[:3], lambda x, y: None, flow_batch=2)
