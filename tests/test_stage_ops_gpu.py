"""GPU parity of the per-stage entry points of the loss / optimizer tail (include/udet.h: udet_flow_normalize,
udet_charbonnier_loss, udet_losses_forward / _backward, udet_generator_backward / udet_recover_backward, udet_grad_absmean,
udet_clip_or_noise, udet_adam_step) and of the function-level Python surface (functional.py) against the CPU oracle.
Tolerance 1e-3 relative (north_star) unless the arithmetic allows tighter."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_torch as O  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel(a, ref):
    return float((a - ref).abs().max()) / max(1e-6, float(ref.abs().max()))


def test_flow_normalize(ops):
    """preprocess_flow_batch (flow_utils.py:5-12)"""
    f = rnd(3, 64, 128, 2, seed=1, scale=2.0) + torch.tensor([0.7, -1.3])
    got = ops.preprocess_flow_batch(f.cuda()).cpu()
    ref = O.preprocess_flow_batch(f.double()).float()
    assert rel(got, ref) < 1e-5
    assert abs(float(got.mean())) < 1e-5 and abs(float(got[0, ..., 0].std(unbiased=False)) - 1.0) < 1e-4


@pytest.mark.parametrize("cbn", [0.5, 0.4, 1.0])
@pytest.mark.parametrize("mc", [None, 1, 2])
def test_charbonnier_loss(ops, cbn, mc):
    """charbonnier_loss (loss_utils.py:34-51) incl. the cbn values of the reference's experiments and the three mask forms"""
    gt, pr = rnd(2, 48, 64, 2, seed=2), rnd(2, 48, 64, 2, seed=3)
    m = None if mc is None else torch.rand(2, 48, 64, mc, generator=torch.Generator().manual_seed(4))
    got = ops.charbonnier_loss(gt.cuda(), pr.cuda(), None if m is None else m.cuda(), cbn).cpu()
    ref = O.charbonnier_loss(gt.double(), pr.double(), torch.ones(1).double() if m is None else m.double(), cbn).float()
    assert rel(got, ref) < 1e-5


def _step_tensors(B=2, H=64, W=128, seed=5):
    flow = rnd(B, H, W, 2, seed=seed, scale=0.3)
    mask = torch.rand(B, H, W, 1, generator=torch.Generator().manual_seed(seed + 1))
    pred3 = rnd(3 * B, H, W, 2, seed=seed + 2, scale=0.3)
    return flow, mask, pred3


def _oracle_losses(flow, mask, pred3, cbn, eps):
    B = flow.shape[0]
    p, pc, pi = pred3[:B], pred3[B:2 * B], pred3[2 * B:]
    cm = 1.0 - mask
    rec = O.charbonnier_loss(flow, p, mask, cbn)
    rec_c = O.charbonnier_loss(flow, pc, cm, cbn)
    prior = O.charbonnier_loss(flow, pi, torch.ones_like(flow), cbn)
    npx = float(flow.shape[1] * flow.shape[2] * B)
    den = O.charbonnier_loss(flow, pi, mask, cbn) + eps
    den_c = O.charbonnier_loss(flow, pi, cm, cbn) + eps
    red, red_c = (1.0 - rec / den).mean(), (1.0 - rec_c / den_c).mean()
    return {"generator": red + red_c, "recover": (rec.sum() + rec_c.sum() + prior.sum()) / npx, "red_rate": red, "red_rate_compl": red_c,
            "reconstruction_loss": rec[0], "reconstruction_compl_loss": rec_c[0], "denominator_red_rate": den[0],
            "denominator_red_rate_compl": den_c[0]}


@pytest.mark.parametrize("cbn", [0.5, 0.4])
def test_losses_forward_and_backward(ops, cbn):
    """losses{} (adversarial_learner.py:141-204) and tf.gradients of both losses w.r.t. the predictions / the mask"""
    flow, mask, pred3 = _step_tensors()
    eps = 75.0
    L, coef = ops.losses_forward(flow.cuda(), mask.cuda(), pred3.cuda(), cbn, eps)
    fd, md, pd = flow.double(), mask.double().requires_grad_(True), pred3.double().requires_grad_(True)
    ref = _oracle_losses(fd, md, pd, cbn, eps)
    for k, v in zip(ops.LOSS_KEYS, L.cpu().tolist()):
        assert abs(v - float(ref[k])) < 1e-4 * max(1.0, abs(float(ref[k]))), (k, v, float(ref[k]))
    gp, = torch.autograd.grad(ref["recover"], [pd], retain_graph=True)
    dpred = ops.losses_backward(flow.cuda(), mask.cuda(), pred3.cuda(), "recover", cbn=cbn).cpu()
    assert rel(dpred, gp.float()) < 1e-4
    gp, gm = torch.autograd.grad(ref["generator"], [pd, md])
    dpred, dmask = ops.losses_backward(flow.cuda(), mask.cuda(), pred3.cuda(), "generator", coef, cbn=cbn)
    B = flow.shape[0]
    assert rel(dpred.cpu(), gp[:2 * B].float()) < 1e-4
    assert rel(dmask.cpu(), gm.float()) < 1e-4


def test_clip_or_noise_and_adam_step_equal_the_fused_apply(ops):
    """train_op's second half stage by stage (loss_utils.py:22-32) == the step's fused clip+Adam kernel, bit for bit; and the
    oracle's TF Adam with shared beta powers."""
    n = 100003
    w0, g0 = rnd(n, seed=7), rnd(n, seed=8, scale=0.3)
    opt = O.TFAdam()
    params = {"x": w0.clone()}
    w, m, v = w0.cuda().clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for t in (1, 2, 3):
        g = (g0 * t).cuda()
        ops.clip_or_noise_(g, 0.2, None)
        clipped, _ = O.clip_or_noise({"x": g0 * t}, 0.2, False)
        assert torch.equal(g.cpu(), clipped["x"])
        ops.adam_step_(w, g, m, v, t)
        opt.apply(params, clipped)
        assert float((w.cpu() - params["x"]).abs().max()) < 1e-6
    # noise branch: flag set -> |U(-clip, clip)| from the counter-based stream of (seed, step, index)
    flag = torch.tensor([0.0, 1.0], device="cuda")
    a = ops.clip_or_noise_(torch.full((n,), 1e-9, device="cuda"), 0.2, flag, seed=8964, step=5).cpu()
    b = ops.clip_or_noise_(torch.full((n,), 1e-9, device="cuda"), 0.2, flag, seed=8964, step=5).cpu()
    assert torch.equal(a, b) and float(a.min()) >= 0.0 and float(a.max()) <= 0.2 and abs(float(a.mean()) - 0.1) < 2e-3


# ---- the same entry points at the shapes, masks and values where the kernels take another path (oracle/oracle_glue.py holds the cases and
# the measured tolerances G.TOL; tests/test_glue_oracle.py re-measures them on the CPU) ---------------------------------------------------
from oracle import oracle_glue as G  # noqa: E402


@pytest.mark.parametrize("cbn", G.LOSS_CBN)
@pytest.mark.parametrize("B,H,W", G.LOSS_SHAPES)
def test_losses_at_small_and_odd_shapes(ops, B, H, W, cbn):
    """losses_forward, both losses_backward forms and charbonnier_loss at B = 1 and 3, HW = 15 (below one block), 257 (one past a block)
    and 33 x 40; masks all 0, all 1 and random; epsilon 75 and 1e-3 (small enough for the denominators to matter).  All eight losses at
    1e-4; coef ITSELF against float64 autograd through the four per-sample sums (G.coef_f64), each derivative relative to its own
    largest value, at G.TOL['coef'] (measured 3.74e-7, allowed 4 x); the gradients at 1e-4."""
    for kind in G.LOSS_MASKS:
        for eps in G.LOSS_EPS:
            flow, mask, pred3 = G.loss_case(B, H, W, kind, 80 + G.LOSS_SHAPES.index((B, H, W)))
            L, coef = ops.losses_forward(flow.cuda(), mask.cuda(), pred3.cuda(), cbn, eps)
            fd, md, pd = flow.double(), mask.double().requires_grad_(True), pred3.double().requires_grad_(True)
            ref, _ = G.losses(fd, md, pd, cbn, eps)
            for k, v in zip(ops.LOSS_KEYS, L.cpu().tolist()):
                assert abs(v - float(ref[k])) < 1e-4 * max(1.0, abs(float(ref[k]))), (kind, eps, k, v, float(ref[k]))
            c64 = G.coef_f64(flow, mask, pred3, cbn, eps)
            for j in range(4):
                assert G.relmax(coef.cpu()[:, j], c64[:, j]) <= G.TOL["coef"], (kind, eps, j, coef.cpu()[:, j], c64[:, j])
            gp, = torch.autograd.grad(ref["recover"], [pd], retain_graph=True)
            dpred = ops.losses_backward(flow.cuda(), mask.cuda(), pred3.cuda(), "recover", cbn=cbn).cpu()
            assert rel(dpred, gp.float()) < 1e-4, (kind, eps)
            gp, gm = torch.autograd.grad(ref["generator"], [pd, md])
            dpred, dmask = ops.losses_backward(flow.cuda(), mask.cuda(), pred3.cuda(), "generator", coef, cbn=cbn)
            assert rel(dpred.cpu(), gp[:2 * B].float()) < 1e-4, (kind, eps)
            assert rel(dmask.cpu(), gm.float()) < 1e-4, (kind, eps)
            got = ops.charbonnier_loss(flow.cuda(), pred3[:B].cuda(), mask.cuda(), cbn).cpu()
            assert rel(got, O.charbonnier_loss(fd, pd[:B].detach(), md.detach(), cbn).float()) < 1e-5, (kind, eps)


@pytest.mark.parametrize("cbn", G.LOSS_CBN)
@pytest.mark.parametrize("B,H,W", G.LOSS_SHAPES)
def test_losses_where_the_prediction_equals_the_flow(ops, B, H, W, cbn):
    """pred3[:B] == flow: every pixel's loss term is 2 * 0.001^(2 cbn) * mask, and the Charbonnier derivative is exactly 0"""
    for kind in G.LOSS_MASKS:
        flow, mask, pred3 = G.loss_case(B, H, W, kind, 90, equal_pred=True)
        want = 2.0 * 0.001 ** (2 * cbn) * mask.double().sum(dim=(1, 2, 3))  # (= 2 HW 0.001^(2 cbn) mask for a constant mask)
        got = ops.charbonnier_loss(flow.cuda(), pred3[:B].cuda(), mask.cuda(), cbn).cpu()
        assert rel(got, want.float()) < 1e-5, kind
        L, coef = ops.losses_forward(flow.cuda(), mask.cuda(), pred3.cuda(), cbn, 75.0)
        assert abs(float(L[4]) - float(want[0])) < 1e-4 * max(1.0, float(want[0])), kind
        dpred = ops.losses_backward(flow.cuda(), mask.cuda(), pred3.cuda(), "recover", cbn=cbn).cpu()
        assert float(dpred[:B].abs().max()) == 0.0, kind
        dpred, _ = ops.losses_backward(flow.cuda(), mask.cuda(), pred3.cuda(), "generator", coef, cbn=cbn)
        assert float(dpred[:B].abs().max()) == 0.0, kind


@pytest.mark.parametrize("t", G.ADAM_T)
@pytest.mark.parametrize("n", G.ADAM_N)
def test_clip_and_adam_state_against_tf_adam(ops, n, t):
    """g after the clip bit for bit, then m and v -- not only w -- against O.TFAdam in float64 after every apply, for gradients that hold
    exactly +-clip, +-(clip + 1 ulp), 0 and 1e-20, at applies t and t + 1 (lr_t from the float64 closed form, as udet_adam_step computes
    it) and at n = 1, 255, 257 and one past the 2048-workgroup grid cap.  w at the project's 1e-6; m and v at G.TOL (measured 2.04e-6 /
    1.63e-7 relative over the two applies, allowed 4 x)."""
    w0, g0, m0, v0 = G.adam_case(n, 70 + G.ADAM_N.index(n))
    w, m, v = w0.cuda(), m0.cuda(), v0.cuda()
    rw, rm, rv = w0.double(), m0.double(), v0.double()
    for k, gk in enumerate(G.adam_gradients(g0)):
        tt, g = t + k, gk.cuda()
        want_g = G.clip_f32(g.cpu(), G.ADAM_CLIP)
        ops.clip_or_noise_(g, G.ADAM_CLIP, None)
        assert torch.equal(g.cpu(), want_g)
        if k == 0 and n >= 7:
            assert torch.equal(g.cpu()[:4].abs(), torch.full((4,), G.ADAM_CLIP))  # +-clip stay, +-(clip + 1 ulp) land on +-clip
        ops.adam_step_(w, g, m, v, tt)
        rw, rm, rv = G.adam_f64(rw, want_g, rm, rv, tt)
        assert float((w.cpu().double() - rw).abs().max()) < 1e-6
        assert G.relmax(m.cpu(), rm) <= G.TOL["adam_m"] and G.relmax(v.cpu(), rv) <= G.TOL["adam_v"]


@pytest.fixture(scope="module")
def tail_engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd.engine import Engine, EngineConfig
    return Engine(EngineConfig(batch_size=2, in_height=128, in_width=192, img_height=64, img_width=128)), W


@pytest.mark.parametrize("t", G.ADAM_T)
@pytest.mark.parametrize("net", ["gen", "rec"])
def test_fused_apply_equals_clip_then_adam_at_the_edge_values(ops, tail_engine, net, t):
    """eng.apply (adam_kernel mode 0) == clip (mode 1) followed by Adam (mode 2), bit for bit in w, g, m and v, on a gradient with the
    edge values at its front and at applies 1, 2, 1000 and 100000; both nets' flat buffers are longer than the grid: the stride loop runs"""
    eng, W = tail_engine
    nid = W.NET_GEN if net == "gen" else W.NET_REC
    n = W.param_total(nid)
    assert n > 2048 * 256
    w0, g0, m0, v0 = G.adam_case(n, 75)
    fused = [x.cuda() for x in (w0, g0, m0, v0)]
    eng.adam_step = t - 1
    eng.apply(nid, *fused)
    assert eng.adam_step == t
    if nid == W.NET_GEN:
        assert float(eng.buffer("noise_flag").view(-1)[1]) == 0.0
    w, g, m, v = (x.cuda() for x in (w0, g0, m0, v0))
    ops.clip_or_noise_(g, G.ADAM_CLIP, None)
    ops.adam_step_(w, g, m, v, t)
    for a, b in zip(fused, (w, g, m, v)):
        assert torch.equal(a, b)
    assert torch.equal(g.cpu(), G.clip_f32(g0, G.ADAM_CLIP))


@pytest.fixture(scope="module")
def small_step():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import functional as F
    from unsupervised_detection_amd import weights as W
    F.set_seed(77)
    gen = torch.Generator().manual_seed(9)
    i1 = (torch.rand(2, 128, 192, 3, generator=gen) - 0.5).cuda()
    i2 = (torch.rand(2, 128, 192, 3, generator=gen) - 0.5).cuda()
    return dict(F=F, W=W, i1=i1, i2=i2)


def test_functional_networks_match_the_oracle(small_step):
    """generator_net / recover_net / ModelPWCNet.predict_from_img_pairs with the reference's own argument contract"""
    F, W = small_step["F"], small_step["W"]
    pp, pg, pr = (W.as_dict(F.variables(n).cpu(), n) for n in (W.NET_PWC, W.NET_GEN, W.NET_REC))
    i1, i2 = small_step["i1"], small_step["i2"]
    flow = F.ModelPWCNet().predict_from_img_pairs(i1, i2)
    ref, _ = O.pwc_forward(pp, i1.cpu(), i2.cpu())
    assert rel(flow.cpu(), ref) < 1e-3
    nn_flow, _ = F.ModelPWCNet().nn(F.ModelPWCNet().adapt_x(i1, i2))
    assert rel(nn_flow.cpu(), ref) < 1e-3
    image = (torch.rand(2, 64, 128, 3, generator=torch.Generator().manual_seed(10)) - 0.5)
    fl = rnd(2, 64, 128, 2, seed=11, scale=0.2)
    fstd = F.preprocess_flow_batch(fl.cuda())
    mask = F.generator_net(image.cuda(), fstd, "MaskNet/")
    mref = O.generator_net(pg, image, O.preprocess_flow_batch(fl))
    assert float((mask.cpu() - mref).abs().max()) < 1e-3
    pred = F.recover_net(image.cuda(), (fl * (1 - mref)).cuda(), mref.cuda(), "FlownetS/")
    pref = O.recover_net(pr, image, fl * (1 - mref), mref)
    assert rel(pred.cpu(), pref) < 1e-3


def test_train_op_equals_the_fused_step(small_step):
    """loss_utils.train_op built from the per-stage entry points (backward of ONE loss, |g| mean, clip / noise, Adam) leaves
    the same weights, bit for bit, as trainer.train_step's fused path (udet_backward + udet_apply), for the reference's
    schedule REC, GEN, GEN (adversarial_learner.py:376-397) with the shared optimizer."""
    F, W = small_step["F"], small_step["W"]
    from unsupervised_detection_amd.engine import GEN, REC, Engine, EngineConfig
    from unsupervised_detection_amd.trainer import TrainState, train_step
    i1, i2 = small_step["i1"], small_step["i2"]
    w0 = {n: F.variables(n).clone() for n in (W.NET_PWC, W.NET_GEN, W.NET_REC)}
    graph = F.AdversarialGraph(2, img_hw=(64, 128), in_hw=(128, 192))
    opt = F.AdamOptimizer(1e-4, beta1=0.9)
    for which in (REC, GEN, GEN):
        losses = graph.run(i1, i2)
        if which == REC:
            op, gv = F.train_op(losses["recover"], "FlownetS/", opt, gradient_clip_value=0.2, can_change=False)
        else:
            op, gv = F.train_op(losses["generator"], "MaskNet/", opt, gradient_clip_value=0.2, can_change=True)
        op()
    assert len(gv) == len(W.param_table(W.NET_GEN)) and float(gv[0][0].abs().max()) <= 0.2
    torch.cuda.synchronize()
    st = TrainState(Engine(EngineConfig(batch_size=2, in_height=128, in_width=192, img_height=64, img_width=128)), w_pwc=w0[W.NET_PWC],
                    w_gen=w0[W.NET_GEN].clone(), w_rec=w0[W.NET_REC].clone())
    for which in (REC, GEN, GEN):
        train_step(st, i1, i2, which)
    torch.cuda.synchronize()
    assert torch.equal(st.w_gen, F.variables(W.NET_GEN)) and torch.equal(st.w_rec, F.variables(W.NET_REC))
    assert opt.t == 3 and st.engine.adam_step == 3
