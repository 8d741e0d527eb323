"""GPU: udet_dense_crf_ragged / udet_crf_unary_lookup (csrc/crf.hip) through post_processing.dense_crf_ragged and
native_results.crf_refine_restored, against oracle_post.dense_crf and, as a second witness, the existing udet_post_dense_crf.

Bounds.  |q1 - oracle Q1| < 1e-5 is the project's bound for the CRF marginals (tests/test_post_processing.py); on
the cases below the float32 oracle is within 1.3e-6 of a float64 restatement of itself, which leaves the kernel about 8x of room.
Labels must equal the oracle's argmax wherever the oracle's |Q1 - Q0| >= 1e-4 (ten times the marginal bound), and at most 0.1 % of a
case's pixels may be excluded that way (the oracle alone excludes none on these inputs).  Batch against single sample, run against
run and guard bytes: exact.  The cases (test_crf_native.CASES) are the smallest at which a tiled, strip-walking kernel can go wrong."""
import numpy as np
import pytest
import torch

from test_crf_native import CASES, COMPAT, scene
from test_native_results import restore_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


_inputs, _oracle = {}, {}


def case_inputs(case):
    """(image uint8 [H,W,3], unary float32 [2,H,W]) of a case, built once."""
    if case not in _inputs:
        from oracle.oracle_post import unary_from_mask
        H, W = case[:2]
        img, soft = scene(H, W, H * W)
        _inputs[case] = (img, unary_from_mask(soft, 0.1))
    return _inputs[case]


def oracle_q(case):
    """oracle_post.dense_crf of a case, computed once and shared."""
    if case not in _oracle:
        from oracle.oracle_post import dense_crf
        img, un = case_inputs(case)
        _, _, R, sxy, srgb, iters = case
        _oracle[case] = dense_crf(un, img, sxy, srgb, COMPAT, iters, R)
    return _oracle[case]


def pack(samples, gap=0):
    """[(image, unary), ...] -> (unary float32 [2,total], images uint8 [3 total], offsets, hw) on the device, `gap` elements before,
    between and after the samples (unary 0, image 0xA5 there)."""
    hw = np.array([u.shape[1:] for _, u in samples], np.int64)
    sizes = hw[:, 0] * hw[:, 1]
    off = gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]])
    total = int(off[-1] + sizes[-1] + gap)
    un, im = np.zeros((2, total), np.float32), np.full(3 * total, 0xA5, np.uint8)
    for (img, u), o, s in zip(samples, off, sizes):
        un[:, o:o + s] = u.reshape(2, -1)
        im[3 * o:3 * (o + s)] = img.reshape(-1)
    return torch.from_numpy(un).cuda(), torch.from_numpy(im).cuda(), off, hw


def guarded(total, dtype):
    """A device buffer of `total` elements whose every byte is 0xA5 (as float32 a small negative number no marginal equals)."""
    return torch.full((total * torch.empty(0, dtype=dtype).element_size(),), 0xA5, dtype=torch.uint8, device="cuda").view(dtype)


def run(samples, R, sxy, srgb, iters, gap=0, **kw):
    from unsupervised_detection_amd.post_processing import dense_crf_ragged
    un, im, off, hw = pack(samples, gap)
    q1, labels = dense_crf_ragged(un, im, off, hw, sxy, srgb, COMPAT, iters, R, **kw)
    return q1, labels, off, hw


def sample_of(buf, off, hw, i):
    H, W = (int(v) for v in hw[i])
    return buf[int(off[i]):int(off[i]) + H * W].view(H, W).cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_single_sample_against_the_oracle_and_the_first_kernel(gpu, case):
    from unsupervised_detection_amd.post_processing import dense_crf
    H, W, R, sxy, srgb, iters = case
    img, un = case_inputs(case)
    q1, labels, off, hw = run([(img, un)], R, sxy, srgb, iters)
    q1, labels = sample_of(q1, off, hw, 0), sample_of(labels, off, hw, 0)
    Q = oracle_q(case)
    fg = float(np.mean(Q[1] > Q[0]))
    changed = int(np.sum((Q[1] > Q[0]) != (un[1] < un[0])))
    err = float(np.abs(q1 - Q[1]).max())
    old = dense_crf(un, img, sxy, srgb, COMPAT, iters, R).cpu().numpy()
    err_old = float(np.abs(q1 - old[1]).max())
    sure = np.abs(Q[1] - Q[0]) >= 1e-4
    print("case", case, "foreground share %.3f" % fg, "labels changed by the CRF", changed, "max|q1 - oracle| %.3g" % err,
          "max|q1 - first kernel| %.3g" % err_old, "pixels below 1e-4:", int((~sure).sum()))
    assert 0.1 < fg < 0.4 and changed > 0  # the CRF does something on this input
    assert err < 1e-5
    assert err_old < 1e-5
    assert (~sure).sum() <= 1e-3 * H * W
    assert labels.dtype == np.uint8 and np.array_equal(labels[sure], (Q[1] > Q[0]).astype(np.uint8)[sure])


def test_ragged_batch_is_bit_identical_to_single_samples(gpu):
    from unsupervised_detection_amd.post_processing import dense_crf_ragged
    R, sxy, srgb, iters = 9, 3, 5, 5
    samples = [case_inputs(c) for c in CASES[:4]]
    un, im, off, hw = pack(samples, gap=37)
    total = un.shape[1]
    q_buf, l_buf = guarded(total, torch.float32), guarded(total, torch.uint8)
    q1, labels = dense_crf_ragged(un, im, off, hw, sxy, srgb, COMPAT, iters, R, q_out=q_buf, labels_out=l_buf)
    assert q1 is q_buf and labels is l_buf
    q_host, l_host = q1.cpu().numpy().copy(), labels.cpu().numpy().copy()
    # the same call twice: bit-identical
    q2, l2 = dense_crf_ragged(un, im, off, hw, sxy, srgb, COMPAT, iters, R, q_out=guarded(total, torch.float32),
                              labels_out=guarded(total, torch.uint8))
    assert q2.cpu().numpy().tobytes() == q_host.tobytes() and l2.cpu().numpy().tobytes() == l_host.tobytes()
    # guard elements before, between and after the samples are untouched
    written = np.zeros(total, bool)
    for o, (H, W) in zip(off, hw):
        written[int(o):int(o) + int(H) * int(W)] = True
    assert (~written).sum() == 37 * 5
    assert (q_host.view(np.uint8).reshape(-1, 4)[~written] == 0xA5).all() and (l_host[~written] == 0xA5).all()
    # every sample equals the same sample run alone, bit for bit (another grid, another tile <-> sample mapping, other neighbours)
    for i, s in enumerate(samples):
        qa, la, oa, ha = run([s], R, sxy, srgb, iters)
        assert sample_of(q1, off, hw, i).tobytes() == sample_of(qa, oa, ha, 0).tobytes(), i
        assert np.array_equal(sample_of(labels, off, hw, i), sample_of(la, oa, ha, 0)), i
        assert 0 < sample_of(la, oa, ha, 0).mean() < 1
    # in another order and with other gaps: still the same
    order = [2, 0, 3, 1]
    q3, l3, o3, h3 = run([samples[i] for i in order], R, sxy, srgb, iters, gap=5)
    for k, i in enumerate(order):
        assert sample_of(q3, o3, h3, k).tobytes() == sample_of(q1, off, hw, i).tobytes(), i


@pytest.mark.parametrize("n, rows", [(60, 2), (128, 4)])
def test_rows_per_thread_variants_are_bit_identical(gpu, n, rows):
    """The kernel holds 1, 2 or 4 rows of a tile per thread, by the size of the grid: batches large enough for the 2- and the 4-row
    form (the single samples above run the 1-row form) give every sample what it gives alone, bit for bit."""
    from unsupervised_detection_amd._ffi import lib
    R, sxy, srgb, iters = 9, 3, 5, 3
    kinds = [case_inputs(c) for c in (CASES[0], (32, 53, 0, 0, 0, 0), CASES[2])]  # 24 x 32, 32 x 53, 5 x 70: the grid is sized for 32 x 70
    assert lib.udet_dense_crf_rows_per_thread(1, 32, 70) == 1 and lib.udet_dense_crf_rows_per_thread(n, 32, 70) == rows
    q1, labels, off, hw = run([kinds[i % 3] for i in range(n)], R, sxy, srgb, iters, gap=3)
    for k, s in enumerate(kinds):
        qa, la, oa, ha = run([s], R, sxy, srgb, iters)
        qa, la = sample_of(qa, oa, ha, 0), sample_of(la, oa, ha, 0)
        for i in (k, k + 3, k + 3 * ((n - 1 - k) // 3)):  # the first two and the last sample of this kind
            assert sample_of(q1, off, hw, i).tobytes() == qa.tobytes() and np.array_equal(sample_of(labels, off, hw, i), la), (k, i)


def test_iters_zero_and_single_outputs(gpu):
    case = CASES[1]
    img, un = case_inputs(case)
    _, _, R, sxy, srgb, iters = case
    q1, labels, off, hw = run([(img, un)], R, sxy, srgb, 0)
    e = -un.astype(np.float64)
    want = np.exp(e[1]) / (np.exp(e[0]) + np.exp(e[1]))
    assert np.abs(sample_of(q1, off, hw, 0) - want).max() <= 1e-6
    assert np.array_equal(sample_of(labels, off, hw, 0), (un[1] < un[0]).astype(np.uint8))
    both = run([(img, un)], R, sxy, srgb, iters)
    q_only = run([(img, un)], R, sxy, srgb, iters, want_labels=False)
    l_only = run([(img, un)], R, sxy, srgb, iters, want_q=False)
    assert q_only[1] is None and l_only[0] is None
    assert torch.equal(q_only[0], both[0]) and torch.equal(l_only[1], both[1])
    with pytest.raises(ValueError):
        run([(img, un)], R, sxy, srgb, iters, want_q=False, want_labels=False)


def test_argument_errors_enqueue_nothing(gpu):
    from unsupervised_detection_amd._ffi import lib
    import unsupervised_detection_amd.post_processing  # noqa: F401  (declares the argument types)
    img, un = case_inputs(CASES[4])
    u, im, off, hw = pack([(img, un)])
    total = u.shape[1]
    d_off, d_hw = torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(hw.astype(np.int32)).cuda()
    q, lab = guarded(total, torch.float32), guarded(total, torch.uint8)
    need = int(lib.udet_dense_crf_workspace_bytes(total, 1))
    assert need >= 16 * total and lib.udet_dense_crf_workspace_bytes(0, 1) == 0 and lib.udet_dense_crf_workspace_bytes(total, 0) == 0
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    good = dict(unary=u.data_ptr(), image=im.data_ptr(), n=1, offsets=d_off.data_ptr(), hw=d_hw.data_ptr(), max_h=16, max_w=16, total=total,
                sxy=1.0, srgb=5.0, compat=5.0, iters=2, radius=3, q1=q.data_ptr(), labels=lab.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.udet_dense_crf_ragged(a["unary"], a["image"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"], a["sxy"],
                                         a["srgb"], a["compat"], a["iters"], a["radius"], a["q1"], a["labels"], a["ws"], a["ws_bytes"], None)
    bad = [dict(n=0), dict(n=65536), dict(iters=-1), dict(radius=0), dict(sxy=0.0), dict(sxy=-1.0), dict(srgb=0.0), dict(srgb=-2.0),
           dict(unary=None), dict(image=None), dict(offsets=None), dict(hw=None), dict(q1=None, labels=None), dict(ws=None),
           dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == -5, kw  # UDET_ERR_ARG
        assert lib.udet_last_error()
    torch.cuda.synchronize()
    assert (q.view(torch.uint8) == 0xA5).all() and (lab == 0xA5).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (q.view(torch.uint8) == 0xA5).all() and (lab <= 1).all()


def test_stage_restore_unary_crf_select(gpu):
    """Restored bytes -> unary (bit-equal to the oracle's, a constant mask included) -> one dense-CRF call -> labels equal to the
    oracle's composed from bytescale + Pillow + placement (test_native_results.restore_np), unary_from_mask and dense_crf -> the
    component selection takes them unchanged."""
    from oracle.oracle_post import dense_crf, unary_from_mask
    from unsupervised_detection_amd.native_results import crf_refine_restored, restore_masks, select_components
    from unsupervised_detection_amd.post_processing import unary_from_restored
    sizes = [(30, 44), (27, 40), (30, 44)]
    masks = np.stack([scene(12, 20, 240 + k)[1] for k in range(3)])
    masks[1] = 0.25  # constant: restores to zeros, amax = 0
    images = [scene(H, W, H * W)[0] for H, W in sizes]
    res = restore_masks(masks, sizes, 0.9, 0.5)
    ref = restore_np(masks, sizes, 0.9, 0.5)
    assert res.amax.cpu().tolist() == ref.amax.tolist() and ref.amax[1] == 0
    unary = unary_from_restored(res.data, res.offsets, res.hw, res.amax, 0.1)
    want_un = []
    for i, (H, W) in enumerate(sizes):
        canvas = res.soft(i).cpu().numpy()
        assert canvas.dtype == np.float64 and np.array_equal(canvas, ref.soft(i))
        want_un.append(unary_from_mask(canvas, 0.1))
        o = int(res.offsets[i])
        assert unary[:, o:o + H * W].cpu().numpy().tobytes() == want_un[-1].tobytes(), i
    assert (want_un[1][1] == np.float32(-np.log(1e-6))).all()

    class Frames(object):
        data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in images])).cuda()
        offsets, hw = 3 * np.asarray(res.offsets), np.asarray(sizes, np.int32)
    crf = {"sxy": 3, "srgb": 5, "compat": COMPAT, "gauss_k": 0.1, "iters": 5, "radius": 6}
    out = crf_refine_restored(res, Frames, crf)
    assert out.data is res.data and out.binary is not res.binary
    for i in range(3):
        Q = dense_crf(want_un[i], images[i], 3, 5, COMPAT, 5, 6)
        assert np.array_equal(out.binary_sample(i).cpu().numpy(), (Q[1] > Q[0]).astype(np.uint8)), i
    assert out.binary_sample(0).any() and not out.binary_sample(1).any()
    sel = select_components(out, mode="largest")
    info = sel.info.cpu().numpy()
    assert info[1].tolist() == [0, -1, 0, 0] and info[0, 0] >= 1 and info[0, 2] == int(sel.binary_sample(0).sum()) > 0
    assert not (sel.binary_sample(0).cpu().numpy() & ~out.binary_sample(0).cpu().numpy().astype(bool)).any()
    with pytest.raises(ValueError):  # frames of other sizes than the restored masks
        Frames.hw = np.asarray([(30, 44), (27, 41), (30, 44)], np.int32)
        crf_refine_restored(res, Frames, crf)
