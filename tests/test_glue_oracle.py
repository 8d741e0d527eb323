"""The restatements of oracle/oracle_glue.py held to each other and to autograd, on the CPU (no GPU needed): the float32 forms against the
float64 forms, the written-out resize adjoint against autograd of O.resize_bilinear_legacy, the fold as the adjoint of the share, the
mean-of-means rule against O.clip_or_noise, and the conditions the GPU tests rely on for their constructed gradients and their measured
tolerances.  tests/test_glue_gpu.py and tests/test_stage_ops_gpu.py hold the kernels of csrc/elementwise.hip to these forms."""
import numpy as np
import pytest
import torch

from oracle import oracle_glue as G
from oracle import oracle_torch as O


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=G.gen(seed)) * scale


def test_measured_tolerances():
    """every measured tolerance is (about) four times the float32 restatement's own deviation on the GPU tests' inputs, and under the cap"""
    worst = G.measure_tolerances()
    assert set(worst) == set(G.TOL)
    for k, tol in G.TOL.items():
        print(k, "measured", worst[k], "allowed", tol)
        assert tol <= G.TOL_CAP, k
        # nominally tol = 4 x measured; another libm may move the measurement a little, never by a factor of two
        assert tol / 8 <= worst[k] <= tol / 2, (k, worst[k], tol)


@pytest.mark.parametrize("copies", [1, 2, 3])
@pytest.mark.parametrize("ld,coff,C", [(8, 0, 8), (8, 4, 4), (6, 1, 2), (12, 0, 12), (5, 4, 1)])
def test_fold_is_the_adjoint_of_share(copies, ld, coff, C):
    P = 7
    x, y = rnd(3 * P, ld, seed=1).double(), rnd(3 * P, ld, seed=2).double()
    sx, fy = G.share(x, P, coff, C, copies), G.fold(y, P, coff, C, copies)
    w = slice(coff, coff + C)
    lhs = (sx[:copies * P, w] * y[:copies * P, w]).sum()
    rhs = (x[:P, w] * fy[:P, w]).sum()
    assert abs(float(lhs - rhs)) < 1e-12 * max(1.0, abs(float(lhs)))
    # nothing outside the window or past copies * P moves, the fold leaves its sources
    keep = torch.ones_like(x, dtype=torch.bool)
    keep[:copies * P, w] = False
    assert torch.equal(sx[keep], x[keep]) and torch.equal(fy[keep], y[keep]) and torch.equal(fy[P:], y[P:])
    # float32 order (x0 + x1) + x2, not x0 + (x1 + x2)
    y32 = rnd(3 * P, ld, seed=3)
    f32 = G.fold(y32, P, coff, C, copies)[:P, w]
    want = y32[:P, w]
    for k in range(1, copies):
        want = want + y32[k * P:(k + 1) * P, w]
    assert torch.equal(f32, want)
    assert G.relmax(f32, G.fold(y32.double(), P, coff, C, copies)[:P, w]) < 3e-7


def test_packs():
    i1, i2 = rnd(5, 3, seed=4), rnd(5, 3, seed=5)
    x = G.pack_pwc_input(i1, i2)
    assert x.shape == (10, 4) and torch.equal(x[:5, :3], i1 + 0.5) and torch.equal(x[5:, :3], i2 + 0.5) and float(x[:, 3].abs().max()) == 0.0
    im = G.pack_imgin(i1, 3)
    assert im.shape == (15, 4) and all(torch.equal(im[k * 5:(k + 1) * 5, :3], i1) for k in range(3)) and float(im[:, 3].abs().max()) == 0.0


@pytest.mark.parametrize("act,alpha", [(G.ACT_NONE, 0.0), (G.ACT_LEAKY, 0.1), (G.ACT_LEAKY, 0.2), (G.ACT_ELU, 1.0)])
def test_emit_du_forms(act, alpha):
    """the derivative taken from the stored output equals autograd of the activation at the pre-activation that produced it"""
    x = rnd(40, 6, seed=6).double()
    x.view(-1)[::7] = 0.0
    x.requires_grad_(True)
    y = {G.ACT_NONE: lambda v: v * 1.0, G.ACT_LEAKY: lambda v: O.leaky_relu(v, alpha), G.ACT_ELU: torch.nn.functional.elu}[act](x)
    d = rnd(40, 6, seed=7).double()
    ref, = torch.autograd.grad(y, [x], d)
    if act != G.ACT_NONE:  # at x == 0 the kernels take the negative branch (a > 0 ? 1 : ...), autograd's choice there is its own
        ref = torch.where(x.detach() == 0, d * (alpha if act == G.ACT_LEAKY else 1.0), ref)
    u64 = G.emit_du(d, y.detach(), 1, 4, act, alpha, torch.zeros(40, 6))
    assert G.relmax(u64[:, 1:5], ref[:, 1:5]) < 1e-7  # (alpha is a float32 constant in both forms)
    assert float(u64[:, 0].abs().max()) == 0.0 and float(u64[:, 5].abs().max()) == 0.0
    u32 = G.emit_du(d.float(), y.detach().float(), 1, 4, act, alpha, torch.zeros(40, 6))
    assert G.relmax(u32, u64) < 3e-7


@pytest.mark.parametrize("hw,ohw", [((7, 9), (11, 5)), ((5, 3), (12, 10)), ((12, 10), (5, 3)), ((3, 5), (6, 10)), ((1, 4), (2, 8)), ((4, 1), (8, 2)),
                                    ((1, 1), (2, 2))])
def test_resize_adjoint_forms(hw, ohw):
    """the written-out adjoint Ay^T dy Ax == float64 autograd of O.resize_bilinear_legacy; the float32 forward against the float64 one"""
    (h, w), (oh, ow) = hw, ohw
    dy = rnd(2, oh, ow, 3, seed=8)
    assert float((G.resize_bwd_matrix(dy, h, w) - G.resize_bwd_f64(dy, h, w)).abs().max()) < 1e-12
    x = rnd(2, h, w, 3, seed=9)
    assert G.relmax(G.resize_fwd_f32(x, oh, ow, 4.0, 3.0), O.resize_bilinear_legacy(x.double(), oh, ow) * 4.0 / 3.0) < 1e-6
    # dot-product identity of forward and adjoint
    lhs = (O.resize_bilinear_legacy(x.double(), oh, ow) * dy.double()).sum()
    rhs = (x.double() * G.resize_bwd_f64(dy, h, w)).sum()
    assert abs(float(lhs - rhs)) < 1e-10 * max(1.0, abs(float(lhs)))


def test_exact_2x_adjoint_weights():
    """the weights resize2x_bwd4_kernel hard-codes: 1 at 2a, 1/2 at 2a - 1, w+ at 2a + 1 with w+ = 1/2, and 1 in the last row, where both taps
    fall on the same source pixel -- a one-pixel source takes 1 + 1"""
    for n in (1, 2, 5):
        A = G.interp_matrix(n, 2 * n)
        for a in range(n):
            col = A[:, a]
            assert float(col[2 * a]) == 1.0 and float(col[2 * a + 1]) == (1.0 if a == n - 1 else 0.5)
            if a > 0:
                assert float(col[2 * a - 1]) == 0.5
            assert int((col != 0).sum()) == (2 if a == 0 else 3)
        assert float(A.sum()) == 2.0 * n  # every output row's two taps add up to 1


@pytest.mark.parametrize("B,HW", [(1, 15), (3, 257), (3, 1320)])
def test_flow_standardise_forms(B, HW):
    f = G.flow_case(B, HW, 10 + B)
    mean, std = f.mean(1), f.std(1, unbiased=False)
    assert float((mean.abs() / std).max()) <= 4.0  # the issue's condition on the inputs
    ref = G.flow_standardise_f64(f)
    assert G.relmax(G.flow_standardise_f32(f), ref) < 1e-5
    gin = G.gen_input_f64(rnd(B, HW, 3, seed=11), f)
    assert torch.equal(gin[..., 3:5], ref) and float(gin[..., 5:].abs().max()) == 0.0


def test_mask_composite_forms_and_saturation():
    logits, f, dmask, dfin = G.mask_bwd_case(189, 12)
    for comp in (G.mask_composite_f32, G.mask_composite_f64):
        m, fin = comp(logits[:, :2], f)
        # (float64 keeps exp(-400) = 1.9e-174 where float32 has exactly 0)
        assert float(m[0]) == 0.5 and float(m[1]) == 1.0 and (float(m[2]) == 0.0 if m.dtype == torch.float32 else 0.0 <= float(m[2]) < 1e-170)
        assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(fin).all())
        assert float((fin[:, :, 2] - 1.0).abs().max()) == 0.0
        assert torch.equal(fin[2], torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=fin.dtype).expand(189, 4))
    m64, _ = G.mask_composite_f64(logits[:, :2], f)
    g64 = G.mask_bwd_f64(logits[:, :2], f, dmask, dfin)
    assert float(g64[1].abs().max()) < 1e-170 and float(g64[2].abs().max()) < 1e-170  # saturated mask: no gradient
    sat = G.mask_bwd_f32(m64.float(), f, dmask, dfin)
    assert float(sat[1].abs().max()) == 0.0 and float(sat[2].abs().max()) == 0.0  # exactly none from the stored float32 mask
    assert G.relmax(g64[:, 1], -g64[:, 0]) < 1e-12  # (autograd's softmax backward rounds the two columns on their own)
    g32 = G.mask_bwd_f32(m64.float(), f, dmask, dfin)
    assert G.relmax(g32, g64) < 1e-6


@pytest.mark.parametrize("cbn", G.LOSS_CBN)
def test_coef_forms_and_equal_prediction(cbn):
    """coef from autograd through the four sums == the closed form; pred == flow: the loss term is 2 HW 0.001^(2 cbn) mask, zero derivative"""
    flow, mask, pred3 = G.loss_case(3, 7, 9, "random", 13, equal_pred=True)
    assert G.relmax(G.coef_f32(flow, mask, pred3, cbn, 75.0), G.coef_f64(flow, mask, pred3, cbn, 75.0)) < 1e-5
    fd, md, pd = flow.double(), mask.double(), pred3.double().requires_grad_(True)
    L, (R, D, Rc, Dc) = G.losses(fd, md, pd, cbn, 75.0)
    want = 2.0 * 0.001 ** (2 * cbn) * md.sum(dim=(1, 2, 3))
    assert float((R.detach() - want).abs().max()) < 1e-12
    g, = torch.autograd.grad(L["generator"], [pd], retain_graph=True)
    assert float(g[:3].abs().max()) == 0.0
    g, = torch.autograd.grad(L["recover"], [pd])
    assert float(g[:3].abs().max()) == 0.0


def _tables():
    from unsupervised_detection_amd import weights as W
    return {"gen": W.param_table(W.NET_GEN), "rec": W.param_table(W.NET_REC)}


@pytest.mark.parametrize("net", ["gen", "rec"])
def test_rule_discrimination_cases_separate_the_two_statistics(net):
    """the two constructed gradients put the mean of means and the global mean of |g| on opposite sides of 1e-5; O.clip_or_noise follows
    the mean of means.  'means_high' holds with a factor of at least 4 on each side.  'means_low' cannot: for any gradient the global mean
    is at most max_len * nvars / total times the mean of means (6.9 generator, 14.9 recover net; asserted below), less than the ratio of
    16 that a factor of 4 on each side needs -- the widest power-of-two margin is taken and held to a factor of 2 on each side."""
    table = _tables()[net]
    cases = G.rule_cases(table)
    bound = G.rule_ratio_bound(table)
    assert bound < 16.0
    rng = np.random.default_rng(3)
    for _ in range(20):  # the bound itself, on arbitrary gradients
        grads = {k: torch.from_numpy(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0)) for k, n in zip(range(len(table)), G.table_lens(table))}
        assert G.global_absmean(grads) <= bound * G.mean_of_means(grads) * (1 + 1e-12)
    for name, (consts, mom, glob) in cases.items():
        assert all(c == 0.0 or np.log2(c) == round(np.log2(c)) for c in consts)
        grads = G.as_dict(G.flat_from_constants(table, consts), table)
        assert abs(G.mean_of_means(grads) - mom) < 1e-12 and abs(G.global_absmean(grads) - glob) < 1e-12
        print(net, name, "mean of means", mom, "global mean", glob)
        if name == "means_high":
            assert mom >= 4e-5 and glob <= 2.5e-6
        else:
            assert mom <= 5e-6 and glob >= 2e-5 and glob / mom > 0.99 * bound
        _, changed = O.clip_or_noise(grads, 0.2, True, noise_fn=lambda k, s: torch.zeros(s))
        assert changed == (name == "means_low")
        _, changed = O.clip_or_noise(grads, 0.2, False)
        assert not changed


@pytest.mark.parametrize("net", ["gen", "rec"])
def test_threshold_gradients(net):
    """constant gradients just below / above 1e-5 flip O.clip_or_noise; the exact-threshold gradient replays to float32(1e-5) exactly"""
    table = _tables()[net]
    lens = G.table_lens(table)
    assert max(lens) < 2 ** 24  # float32 sums of ones are exact
    for sign, want in ((-1, True), (1, False)):
        c = 1e-5 * (1 + sign * 2.0 ** -10)
        grads = G.as_dict(G.flat_from_constants(table, [c] * len(lens)), table)
        _, changed = O.clip_or_noise(grads, 0.2, True, noise_fn=lambda k, s: torch.zeros(s))
        assert changed == want
    g, replay = G.exact_threshold_gradient(table)
    assert replay == G.THRESH and not (replay < G.THRESH)
    assert int((g != 0).sum()) == 1
    # the float32 flag stage against the float64 rule
    sums = [float(v.double().abs().sum()) for v in G.as_dict(g, table).values()]
    assert abs(float(G.flag_stage_f32(sums, lens)) - G.mean_of_means(G.as_dict(g, table))) < 1e-11


@pytest.mark.parametrize("t", G.ADAM_T)
def test_adam_forms(t):
    w, g, m, v = G.adam_case(257, 14)
    assert {float(x) for x in g[:7].abs()} >= {0.0, float(np.float32(0.2)), float(np.float32(1e-20))}
    gc = G.clip_f32(g, G.ADAM_CLIP)
    assert float(gc.abs().max()) == float(np.float32(0.2)) and torch.equal(gc[:4].abs(), torch.full((4,), 0.2))
    w32, m32, v32 = G.adam_f32(w, gc, m, v, t)
    w64, m64, v64 = G.adam_f64(w, gc, m, v, t)
    assert float((w32 - w64).abs().max()) < 1e-6
    assert G.relmax(m32, m64) < G.TOL["adam_m"] and G.relmax(v32, v64) < G.TOL["adam_v"]
    # the closed form of lr_t equals the running beta powers of the shared optimizer
    opt = O.TFAdam()
    for _ in range(min(t, 1000) - 1):
        opt.b1p *= opt.b1
        opt.b2p *= opt.b2
    if t <= 1000:
        assert abs(opt.b1p - 0.9 ** t) < 1e-12 and abs(opt.b2p - 0.999 ** t) < 1e-12
