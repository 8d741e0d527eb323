"""The glue kernels of csrc/elementwise.hip one by one, each through one launch (the udet_debug_launch_* hooks of include/udet_debug.h, or the
entry point the kernel already has), against the restatements of oracle/oracle_glue.py: bit for bit where the float32 form has the kernel's
order, against float64 at the project's tolerance for that operation, or at a tolerance measured on these very inputs (G.TOL: four times
the float32 restatement's own deviation from float64, re-measured by tests/test_glue_oracle.py).  Shapes are tiny; every output sits in a
buffer whose other channels, rows and guard bands hold a sentinel that must survive."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_glue as G  # noqa: E402
from oracle import oracle_torch as O  # noqa: E402

S = G.SENTINEL
PIX = (1, 15, 257, 189)  # one pixel, below one block, one past a block (2 P no multiple of 256 either), odd


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import _devel
    return _devel


class Guarded:
    """a device tensor between two guard bands of 64 sentinel floats (the tensor itself starts 256-byte aligned)"""

    def __init__(self, init):
        n = init.numel()
        self.raw = torch.full((n + 128,), S, device="cuda")
        self.t = self.raw[64:64 + n].view(init.shape)
        self.t.copy_(init)

    def intact(self):
        return bool((self.raw[:64] == S).all()) and bool((self.raw[-64:] == S).all())


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=G.gen(seed)) * scale


def err_vs(got, ref, scale_ref=None):
    """max |got - ref| relative to the largest value of scale_ref (default: ref)"""
    s = float((ref if scale_ref is None else scale_ref).double().abs().max())
    return float((got.double() - ref.double()).abs().max()) / s


# ---------------------------------------------------------------------------------------------------------------------------------
# copies and packs: torch.equal
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PIX)
def test_pack_pwc_input(dev, P):
    i1, i2 = rnd(P, 3, seed=1) * 0.3, rnd(P, 3, seed=2) * 0.3
    x8 = Guarded(torch.full((2 * P, 4), S))
    dev.launch("pack_pwc_input", i1.cuda(), i2.cuda(), x8.t, P)
    got = x8.t.cpu()
    assert torch.equal(got, G.pack_pwc_input(i1, i2)) and x8.intact()
    assert float(got[:, 3].abs().max()) == 0.0  # the padding channel is exactly 0


@pytest.mark.parametrize("ncalls", [0, 1, 2, 3])
@pytest.mark.parametrize("P", PIX)
def test_pack_imgin(dev, P, ncalls):
    img = rnd(P, 3, seed=3)
    out = Guarded(torch.full((3 * P, 4), S))
    dev.launch("pack_imgin", img.cuda(), out.t, P, ncalls)
    want = torch.full((3 * P, 4), S)
    want[:ncalls * P] = G.pack_imgin(img, ncalls)
    assert torch.equal(out.t.cpu(), want) and out.intact()  # the rows of the calls not asked for are untouched


# (ld, coff, C): the float4 form needs all three to be multiples of 4; then each of them breaks it in turn; C = 1, 2, 4, 12
FORMS = [(8, 0, 8), (12, 4, 4), (16, 4, 12), (6, 0, 4), (8, 1, 4), (8, 4, 2), (8, 0, 1), (13, 0, 12)]


@pytest.mark.parametrize("copies", [1, 2, 3])
@pytest.mark.parametrize("ld,coff,C", FORMS)
@pytest.mark.parametrize("P", (1, 15, 257))
def test_share_samples(dev, P, ld, coff, C, copies):
    buf0 = torch.full((3 * P + 2, ld), S)  # (rows past copies * P, and two more than any call uses, hold the sentinel)
    buf0[:P] = rnd(P, ld, seed=4)
    buf = Guarded(buf0)
    dev.launch("share_samples", buf.t, P, ld, coff, C, copies)
    assert torch.equal(buf.t.cpu(), G.share(buf0, P, coff, C, copies)) and buf.intact()


@pytest.mark.parametrize("copies", [1, 2, 3])
@pytest.mark.parametrize("ld,coff,C", FORMS)
@pytest.mark.parametrize("P", (1, 15, 257))
def test_fold_samples(dev, P, ld, coff, C, copies):
    """bit-equal to (x0 + x1) + x2; sources, other channels and later rows unchanged; <share(x), y> == <x, fold(y)> on the GPU results"""
    buf0 = torch.full((3 * P + 2, ld), S)
    # magnitudes spread over several binades, so that x0 + (x1 + x2) rounds differently from (x0 + x1) + x2 on many elements
    buf0[:copies * P] = rnd(copies * P, ld, seed=5) * torch.pow(10.0, rnd(copies * P, ld, seed=6))
    buf = Guarded(buf0)
    dev.launch("fold_samples", buf.t, P, ld, coff, C, copies)
    got = buf.t.cpu()
    assert torch.equal(got, G.fold(buf0, P, coff, C, copies)) and buf.intact()
    assert torch.equal(got[P:], buf0[P:])
    x0 = torch.full((3 * P + 2, ld), S)
    x0[:P] = rnd(P, ld, seed=7)
    x = Guarded(x0)
    dev.launch("share_samples", x.t, P, ld, coff, C, copies)
    w = slice(coff, coff + C)
    lhs = (x.t.cpu()[:copies * P, w].double() * buf0[:copies * P, w].double()).sum()
    rhs = (x0[:P, w].double() * got[:P, w].double()).sum()
    scale = (x0[:P, w].double().abs().max() * buf0[:copies * P, w].double().abs()).sum()
    assert abs(float(lhs - rhs)) <= 2.0 ** -22 * float(scale)  # (the fold's two float32 roundings per element)


@pytest.mark.parametrize("act,alpha", [(G.ACT_NONE, 0.0), (G.ACT_LEAKY, 0.1), (G.ACT_LEAKY, 0.2), (G.ACT_ELU, G.ELU_ALPHA)])
@pytest.mark.parametrize("case", range(len(G.EMIT_CASES)))
def test_emit_du(dev, case, act, alpha):
    """u = d * act'(a) with the derivative from the stored output, on a channel window inside a wider row"""
    P, ld, coff, C = G.EMIT_CASES[case]
    d, a = G.emit_case(P, ld, 60 + case)
    assert P == 1 or (bool((a > 0).any()) and bool((a < 0).any()) and bool((a == 0).any()))
    u0 = torch.full((P, ld), S)
    u = Guarded(u0)
    dev.launch("emit_du", d.cuda(), a.cuda(), u.t, P, ld, coff, C, act, alpha)
    got = u.t.cpu()
    assert u.intact()
    if act == G.ACT_ELU:
        ref = G.emit_du(d.double(), a.double(), coff, C, act, alpha, u0)
        w = slice(coff, coff + C)
        assert err_vs(got[:, w], ref[:, w]) <= G.TOL["emit_elu"]  # measured 4.24e-8, allowed 4 x
        keep = torch.ones(P, ld, dtype=torch.bool)
        keep[:, w] = False
        assert bool((got[keep] == S).all())
    else:
        assert torch.equal(got, G.emit_du(d, a, coff, C, act, alpha, u0))


# ---------------------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------------------
def _windowed(x, ld, coff, seed):
    """x [n,h,w,c] placed at channels [coff, coff + c) of a [n,h,w,ld] tensor of other random values"""
    n, h, w, c = x.shape
    full = rnd(n, h, w, ld, seed=seed) * 3.0
    full[..., coff:coff + c] = x
    return full


def _resize_fwd(dev, x, ldx, x_coff, ldy, y_coff, oh, ow, mul, div):
    n, h, w, c = x.shape
    y = Guarded(torch.full((n, oh, ow, ldy), S))
    dev.launch("resize_bilinear_fwd", _windowed(x, ldx, x_coff, 11).cuda(), ldx, x_coff, n, h, w, y.t, ldy, y_coff, oh, ow, c, mul, div)
    assert y.intact()
    return y.t.cpu()


# (n, h, w, oh, ow, c, ldx, x_coff, ldy, y_coff, mul, div); C % 4 == 0 with aligned windows selects resize_bilinear_fwd4_kernel
RESIZE_FWD = [(1, 3, 5, 6, 12, 2, 2, 0, 2, 0, 4.0, 1.0),     # the step's flow up-scale: mul 4
              (2, 7, 9, 11, 5, 3, 5, 1, 4, 1, 4.0, 1.0),
              # (mul = 4 is a power of two: (v * 4) / d == (v / d) * 4 and 4 (a + b) == 4 a + 4 b exactly, so a kernel that scaled in another
              # order would pass with it -- 1.7 and 0.3 hold the order as well)
              (3, 6, 12, 33, 40, 4, 8, 4, 12, 8, 1.7, 3.0),  # float4 form, both windows inside wider rows, div != 1
              (2, 1, 257, 7, 9, 8, 8, 0, 12, 4, 4.0, 7.0),   # float4 form, C = ld on the source side
              (1, 257, 1, 3, 5, 1, 3, 2, 2, 1, 0.3, 3.0),
              (3, 1, 1, 3, 5, 5, 7, 1, 6, 0, 4.0, 1.0),
              (1, 7, 9, 1, 1, 4, 4, 0, 5, 0, 1.0, 80.0)]     # C % 4 == 0 but ldy % 4 != 0: generic kernel


@pytest.mark.parametrize("case", RESIZE_FWD)
def test_resize_forward_strided(dev, case):
    n, h, w, oh, ow, c, ldx, x_coff, ldy, y_coff, mul, div = case
    x = rnd(n, h, w, c, seed=12)
    got = _resize_fwd(dev, x, ldx, x_coff, ldy, y_coff, oh, ow, mul, div)
    want = torch.full((n, oh, ow, ldy), S)
    want[..., y_coff:y_coff + c] = G.resize_fwd_f32(x, oh, ow, mul, div)
    assert torch.equal(got, want)


@pytest.mark.parametrize("mul,div", [(4.0, 1.0), (1.7, 3.0)])
@pytest.mark.parametrize("hw,ohw", [((3, 5), (6, 12)), ((7, 9), (11, 5)), ((6, 12), (33, 40)), ((1, 1), (3, 5))])
def test_resize_forward_float4_equals_generic(dev, hw, ohw, mul, div):
    """the same content through resize_bilinear_fwd4_kernel (aligned windows) and through the generic kernel (x_coff = 1): bit for bit"""
    x = rnd(2, hw[0], hw[1], 8, seed=13)
    fast = _resize_fwd(dev, x, 12, 4, 8, 0, ohw[0], ohw[1], mul, div)
    slow = _resize_fwd(dev, x, 12, 1, 9, 1, ohw[0], ohw[1], mul, div)
    assert torch.equal(fast, slow[..., 1:9]) and torch.equal(fast, G.resize_fwd_f32(x, ohw[0], ohw[1], mul, div))


def _resize_bwd(dev, dy, ldy, y_coff, h, w, ldx, x_coff, accumulate, dx0):
    n, oh, ow, c = dy.shape
    dx = Guarded(dx0)
    dev.launch("resize_bilinear_bwd", _windowed(dy, ldy, y_coff, 14).cuda(), ldy, y_coff, n, oh, ow, dx.t, ldx, x_coff, h, w, c, accumulate)
    assert dx.intact()
    return dx.t.cpu()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("hw,ohw", [((7, 9), (11, 5)), ((5, 3), (12, 10)), ((12, 10), (5, 3)), ((3, 5), (6, 10)), ((1, 257), (3, 5))])
@pytest.mark.parametrize("c,ldy,y_coff,ldx,x_coff", [(3, 5, 1, 4, 1), (4, 8, 4, 12, 8), (2, 2, 0, 2, 0)])
def test_resize_backward(dev, hw, ohw, c, ldy, y_coff, ldx, x_coff, accumulate):
    """against float64 autograd of O.resize_bilinear_legacy at the project's tolerance for this adjoint (1e-5 absolute, unit-scale inputs);
    channel windows on both sides, accumulate onto a non-zero dx; (3, 5) -> (6, 10) with c = 4 is the exact-2x float4 kernel"""
    (h, w), (oh, ow) = hw, ohw
    dy = rnd(2, oh, ow, c, seed=15)
    dx0 = rnd(2, h, w, ldx, seed=16)
    got = _resize_bwd(dev, dy, ldy, y_coff, h, w, ldx, x_coff, accumulate, dx0)
    want = dx0.double().clone()
    adj = G.resize_bwd_f64(dy, h, w)
    want[..., x_coff:x_coff + c] = adj + (want[..., x_coff:x_coff + c] if accumulate else 0.0)
    assert float((got.double() - want).abs().max()) < 1e-5
    keep = torch.ones_like(dx0, dtype=torch.bool)
    keep[..., x_coff:x_coff + c] = False
    assert torch.equal(got[keep], dx0[keep])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n,h,w", [(2, 3, 5), (1, 1, 4), (1, 4, 1), (3, 1, 1), (1, 7, 9), (2, 6, 12)])
def test_resize_backward_exact_2x_equals_generic(dev, n, h, w, accumulate):
    """the same dy through resize2x_bwd4_kernel (aligned windows, C % 4 == 0) and through the generic gather kernel (coff = 1 breaks the
    fast path): 1e-6 relative on the common channels, both within 1e-5 of float64 autograd.  H = 1, W = 1 and 1 x 1 sources: the last row
    or column is also the first, both taps of the odd output fall on the same source pixel."""
    dy = rnd(n, 2 * h, 2 * w, 4, seed=17)
    dx0 = rnd(n, h, w, 4, seed=18)
    fast = _resize_bwd(dev, dy, 8, 4, h, w, 8, 4, accumulate, _windowed(dx0, 8, 4, 19))[..., 4:8]
    slow = _resize_bwd(dev, dy, 8, 1, h, w, 8, 1, accumulate, _windowed(dx0, 8, 1, 19))[..., 1:5]
    ref = G.resize_bwd_f64(dy, h, w) + (dx0.double() if accumulate else 0.0)
    assert err_vs(fast, slow) <= 1e-6
    assert float((fast.double() - ref).abs().max()) < 1e-5 and float((slow.double() - ref).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# generator input / flow standardisation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(3, 5), (1, 257), (33, 40)])
def test_gen_input_and_flow_normalize(dev, B, H, W):
    """pack_gen_input (what the step launches) and flow_normalize produce bit-identical standardised flow; both within 1e-5 relative of
    O.preprocess_flow_batch in float64; image channels copied exactly, the three padding channels exactly 0"""
    from unsupervised_detection_amd import ops
    HW = H * W
    f = G.flow_case(B, HW, 20 + B)
    img = rnd(B, HW, 3, seed=21)
    ws = torch.empty(int(dev.dbg.udet_debug_gen_input_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
    gin = Guarded(torch.full((B, HW, 8), S))
    dev.launch("gen_input", img.cuda(), f.cuda(), gin.t, B, HW, ws, ws.numel())
    got = gin.t.cpu()
    fn = ops.preprocess_flow_batch(f.view(B, H, W, 2).cuda()).cpu().view(B, HW, 2)
    assert gin.intact()
    assert torch.equal(got[..., 3:5], fn)
    ref = G.flow_standardise_f64(f)
    assert err_vs(fn, ref) < 1e-5 and err_vs(got[..., 3:5], ref) < 1e-5
    assert torch.equal(got[..., :3], img) and float(got[..., 5:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# mask, recover inputs and their backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncalls", [0, 1, 2, 3])
@pytest.mark.parametrize("case", range(len(G.BHW_CASES)))
def test_mask_rec_inputs(dev, case, ncalls):
    B, H, W = G.BHW_CASES[case]
    P = B * H * W
    logits, f = G.mask_case(P, 40 + case)
    mask, fin = Guarded(torch.full((P,), S)), Guarded(torch.full((3, P, 4), S))
    dev.launch("mask_rec_inputs", logits.cuda(), f.cuda(), mask.t, fin.t, P, ncalls)
    m, fi = mask.t.cpu(), fin.t.cpu()
    assert mask.intact() and fin.intact()
    m64, fin64 = G.mask_composite_f64(logits[:, :2], f)
    assert err_vs(m, m64) <= G.TOL["mask"]  # measured 1.077e-7, allowed 4 x
    assert bool(torch.isfinite(m).all())
    assert float(m[0]) == 0.5  # equal logits
    if P > 2:
        assert float(m[1]) == 1.0 and float(m[2]) == 0.0  # logits of +-2000
    if ncalls:
        assert err_vs(fi[:ncalls], fin64[:ncalls], fin64) <= G.TOL["fin"]  # measured 8.70e-8, allowed 4 x
        assert bool(torch.isfinite(fi[:ncalls]).all())
        assert float((fi[:ncalls, :, 2] - 1.0).abs().max()) == 0.0  # channel 2 of every written call is exactly 1
    if ncalls == 3:
        assert torch.equal(fi[2], torch.tensor([0.0, 0.0, 1.0, 0.0]).expand(P, 4))
    assert bool((fi[ncalls:] == S).all())  # the rows of the calls not asked for


@pytest.mark.parametrize("case", range(len(G.BHW_CASES)))
def test_mask_bwd(dev, case):
    """dlogits against autograd of the float64 composite with random dmask / dfin; exactly 0 where the mask is exactly 0 or 1"""
    B, H, W = G.BHW_CASES[case]
    P = B * H * W
    logits, f, dmask, dfin = G.mask_bwd_case(P, 40 + case)
    m64, _ = G.mask_composite_f64(logits[:, :2], f)
    out = Guarded(torch.full((P, 8), S))
    dev.launch("mask_bwd", dmask.cuda(), dfin.cuda(), f.cuda(), m64.float().cuda(), out.t, P)
    got = out.t.cpu()
    assert out.intact()
    ref = G.mask_bwd_f64(logits[:, :2], f, dmask, dfin)
    if float(ref.abs().max()) > 1e-100:
        assert err_vs(got[:, :2], ref) <= G.TOL["mask_bwd"]  # measured 1.523e-7, allowed 4 x
    else:  # (one pixel with equal logits aside, the smallest cases are all saturated)
        assert float(got[:, :2].abs().max()) == 0.0
    assert torch.equal(got[:, 1], -got[:, 0])
    assert bool((got[:, 2:] == S).all())  # channels 2..7 of the ld-8 rows
    if P > 2:
        assert float(got[1:3, :2].abs().max()) == 0.0


def test_hooks_refuse_bad_arguments_before_any_launch(dev):
    """a channel window outside its row, a misaligned pointer, an ncalls / copies out of range: an error code, never a launch"""
    buf = torch.zeros(64, device="cuda")
    L = dev.launch
    with pytest.raises(ValueError):
        L("share_samples", buf, 2, 8, 6, 4, 2)            # window 6 + 4 of 8
    with pytest.raises(ValueError):
        L("share_samples", buf[1:], 2, 8, 0, 4, 2)        # float4 form on a pointer that is not 16-byte aligned
    with pytest.raises(ValueError):
        L("fold_samples", buf, 2, 8, 0, 4, 4)             # copies
    with pytest.raises(ValueError):
        L("emit_du", buf, buf, buf, 2, 8, -1, 4, 1, 0.2)  # negative coff
    with pytest.raises(ValueError):
        L("emit_du", buf, buf, buf, 2, 8, 0, 4, 7, 0.2)   # unknown act
    with pytest.raises(ValueError):
        L("resize_bilinear_fwd", buf, 2, 1, 1, 2, 2, buf, 2, 0, 2, 2, 2, 1.0, 1.0)   # x window 1 + 2 of 2
    with pytest.raises(ValueError):
        L("resize_bilinear_bwd", buf, 2, 0, 1, 2, 2, buf, 2, 0, 2, 2, 3, 0)          # c = 3 of ld 2
    with pytest.raises(ValueError):
        L("resize_bilinear_bwd", buf, 2, 0, 1, 2, 2, None, 2, 0, 2, 2, 2, 0)         # NULL
    with pytest.raises(ValueError):
        L("pack_pwc_input", buf, buf, buf[1:], 2)         # x8 not 16-byte aligned
    with pytest.raises(ValueError):
        L("mask_rec_inputs", buf, buf, buf, buf, 2, 4)    # ncalls
    with pytest.raises(ValueError):
        L("mask_rec_inputs", buf, buf[1:], buf, buf, 2, 1)  # flow not 8-byte aligned
    with pytest.raises(ValueError):
        L("mask_bwd", buf, buf[2:], buf, buf, buf, 2)     # dfin not 16-byte aligned
    with pytest.raises(ValueError):
        L("pack_imgin", buf, buf, 0, 1)                   # no pixels
    with pytest.raises(ValueError):
        L("gen_input", buf, buf, buf, 1, 2, buf, 8)       # workspace too small
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the escape rule: grad_absmean_kernel + grad_flag_kernel through udet_grad_absmean and through eng.apply
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd._ffi import check, lib
    from unsupervised_detection_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(batch_size=2, in_height=128, in_width=192, img_height=64, img_width=128))

    def absmean(net, g):
        out = torch.full((2,), S, device="cuda")
        check(lib.udet_grad_absmean(eng._h, net, g.data_ptr(), out.data_ptr(), eng.ws.data_ptr(), eng._stream()))
        return out.cpu().numpy()

    return dict(eng=eng, W=W, absmean=absmean, nets={"gen": W.NET_GEN, "rec": W.NET_REC})


NETS = ["gen", "rec"]


@pytest.mark.parametrize("net", NETS)
def test_absmean_of_all_ones_is_exactly_one(env, net):
    """every per-variable mean is exactly 1 (each variable is far shorter than 2^24: the float32 sums are exact), so any element lost or
    counted twice at a slice or tail boundary shows"""
    W, nid = env["W"], env["nets"][net]
    assert max(G.table_lens(W.param_table(nid))) < 2 ** 24
    out = env["absmean"](nid, torch.ones(W.param_total(nid), device="cuda"))
    assert float(out[0]) == 1.0 and float(out[1]) == 0.0


def _handful(lens):
    """the shortest, the longest, one whose length is no multiple of 8, one shorter than 8 (distinct where the table has them)"""
    order = sorted(range(len(lens)), key=lambda i: lens[i])
    pick = [order[0], order[-1]]
    pick += [i for i in order if lens[i] % 8 and lens[i] >= 8][:1]
    pick += [i for i in order if lens[i] < 8 and i not in pick][:1]
    return sorted(set(pick))


@pytest.mark.parametrize("net", NETS)
def test_absmean_of_one_element(env, net):
    """a single 1.0 at the first, last and a middle index of a handful of variables: out2[0] == 1 / (len_v nvars) to float32 rounding
    (two correctly rounded divisions: 3 ulp allowed)"""
    W, nid = env["W"], env["nets"][net]
    table = W.param_table(nid)
    lens = G.table_lens(table)
    g = torch.zeros(W.param_total(nid), device="cuda")
    for v in _handful(lens):
        off = table[v][2]
        for pos in sorted({0, lens[v] // 2 + (lens[v] > 2), lens[v] - 1} & set(range(lens[v]))):
            g[off + pos] = 1.0
            out = env["absmean"](nid, g)
            g[off + pos] = 0.0
            want = 1.0 / (lens[v] * len(lens))
            assert abs(float(out[0]) - want) <= 3 * 2.0 ** -24 * want, (table[v][0], pos, float(out[0]), want)
            assert float(out[1]) == (1.0 if want < 1e-5 else 0.0)


@pytest.mark.parametrize("net", NETS)
def test_flag_follows_the_mean_of_means_not_the_global_mean(env, net):
    """two constructed gradients (per-variable powers of two) with the mean of means and the global mean of |g| on opposite sides of 1e-5
    (conditions and margins: tests/test_glue_oracle.py, G.rule_cases); the flag must follow the mean of means in both"""
    W, nid = env["W"], env["nets"][net]
    table = W.param_table(nid)
    for name, (consts, mom, glob) in G.rule_cases(table).items():
        flat = G.flat_from_constants(table, consts)
        grads = W.as_dict(flat, nid)
        mom, glob = G.mean_of_means(grads), G.global_absmean(grads)  # both statistics on the CPU, before the GPU flag is looked at
        _, ref_changed = O.clip_or_noise(grads, 0.2, True, noise_fn=lambda k, s: torch.zeros(s))
        if name == "means_high":
            assert mom >= 4e-5 and glob <= 2.5e-6 and not ref_changed
        else:
            assert mom <= 5e-6 and glob >= 2e-5 and ref_changed  # (the widest margin that exists: G.rule_ratio_bound)
        out = env["absmean"](nid, flat.cuda())
        assert abs(float(out[0]) - mom) <= 1e-6 * mom
        assert float(out[1]) == (1.0 if ref_changed else 0.0), (name, float(out[0]), mom, glob)


@pytest.mark.parametrize("net", NETS)
def test_flag_threshold(env, net):
    """constant gradients with avg = 1e-5 (1 -+ 2^-10) flip the flag; avg == 1e-5f exactly does not set it (strict comparison)"""
    W, nid = env["W"], env["nets"][net]
    n = W.param_total(nid)
    for sign, want in ((-1, 1.0), (1, 0.0)):
        c = 1e-5 * (1 + sign * 2.0 ** -10)
        out = env["absmean"](nid, torch.full((n,), c, device="cuda"))
        assert abs(float(out[0]) - c) <= 1e-4 * c and float(out[1]) == want
    g, replay = G.exact_threshold_gradient(W.param_table(nid))
    assert replay == G.THRESH
    out = env["absmean"](nid, g.cuda())
    assert out[0] == G.THRESH and float(out[1]) == 0.0


def test_apply_escapes_for_the_generator_only(env):
    """through eng.apply: the generator's gradient is replaced when the mean of means is below 1e-5 (and only then), the recover net's
    never, whatever its gradient"""
    eng, W = env["eng"], env["W"]
    for net, name in ((W.NET_GEN, "means_low"), (W.NET_GEN, "means_high"), (W.NET_REC, "means_low"), (W.NET_REC, "means_high")):
        table = W.param_table(net)
        consts, _, _ = G.rule_cases(table)[name]
        g0 = G.flat_from_constants(table, consts)
        n = g0.numel()
        g = g0.cuda()
        eng.buffer("noise_flag").fill_(S)
        eng.apply(net, torch.zeros(n, device="cuda"), g, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"))
        flag = eng.buffer("noise_flag").view(-1).cpu()
        if net == W.NET_GEN and name == "means_low":
            assert float(flag[1]) == 1.0
            got = g.cpu()
            assert float(got.min()) >= 0.0 and float(got.max()) <= 0.2 and abs(float(got.mean()) - 0.1) < 2e-3
            assert int((got == 0).sum()) < 8  # the zeros of the constructed gradient are gone
        else:
            assert torch.equal(g.cpu(), g0.clamp(-0.2, 0.2))
            if net == W.NET_GEN:
                assert float(flag[1]) == 0.0
            else:
                assert float(flag[1]) == S  # can_change=False: the rule is not even evaluated
