"""CPU: oracle/oracle_conv_ex.py (the float64 restatement of a convolution launch with its epilogue options, the reference of
tests/test_conv_epilogue_gpu.py) against torch.autograd, and the refusals of udet_debug_conv2d_ex, which come before any HIP call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle_conv_ex as X
from oracle import oracle_torch as O
from oracle.oracle_glue import ACT_ELU, ACT_LEAKY, ACT_NONE

TOL = 1e-12  # float64 against float64: summation order only


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).double()


def _nchw_up_conv(x, w):
    """NN x2 + 3x3 SAME written without the oracle's helpers: F.interpolate, then a padded NCHW convolution"""
    xu = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return F.conv2d(xu, w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("act,alpha", [(ACT_LEAKY, 0.1), (ACT_ELU, 0.0), (ACT_NONE, 0.0)])
@pytest.mark.parametrize("k,stride,hw", [(3, 1, (9, 11)), (5, 2, (12, 16)), (3, 2, (9, 13)), (1, 2, (8, 10))])
def test_backward_data_with_skip_accumulate_and_emission_is_autograd(act, alpha, k, stride, hw):
    """a = act(convA(x0) + bA) is the saved output `ua`; out = convB(a).  With L = <out, dz> + <a, skip> + <a, old>:
    y = dgrad_B(dz) + skip + old = dL/da and the emitted u = y * act'(a) = dL/d(pre-activation of layer A), on every column."""
    h, w = hw
    ca, cb = 12, 7
    x0 = rnd(2, h, w, 5, seed=1)
    x0[:, 2:7, 3:8] = 0  # exact zeros in `a` (bA = 0 there is not needed: the bias is 0 on channel 0) -- act' at ua == 0
    wa = rnd(3, 3, 5, ca, seed=2, scale=0.3)
    ba = rnd(ca, seed=3, scale=0.1)
    ba[0] = 0
    wb = rnd(k, k, ca, cb, seed=4, scale=0.2)
    pre = (O.conv2d_same(x0, wa, ba, 1, 1)).requires_grad_(True)
    a = X.act_fwd(pre, act, alpha)
    a.retain_grad()
    assert int((a[..., 0] == 0).sum()) >= 9
    out = O.conv2d_same(a, wb, None, stride, 1)
    dz, skip, old = rnd(*out.shape, seed=5), rnd(*a.shape, seed=6), rnd(*a.shape, seed=7)
    ((out * dz).sum() + (a * skip).sum() + (a * old).sum()).backward()
    # the launch: dz in a window of a wider row, y accumulated into a window, res at its own offset, emission on all columns
    ldx, xc, kc = 16, 4, 8
    x = torch.full((2, *out.shape[1:3], ldx), 3.0, dtype=torch.float64)
    x[..., xc:xc + cb] = dz
    y = torch.full((2, h, w, ca + 8), -5.0, dtype=torch.float64)
    y[..., 4:4 + ca] = old
    res = torch.zeros(2, h, w, ca + 4, dtype=torch.float64)
    res[..., 2:2 + ca] = skip
    ua = torch.zeros(2, h, w, ca + 4, dtype=torch.float64)
    ua[..., 4:] = a.detach()
    uo = torch.full((2, h, w, ca + 8), -9.0, dtype=torch.float64)
    yn, _, un = X.conv_ex(X.DGRAD, x, xc, kc, wb, y, 4, stride=stride, res=res, res_coff=2, accumulate=1, uo=uo, u_coff=8, ua=ua, ua_coff=4,
                          uact=act, ualpha=alpha, u_c0=0, u_c1=ca)
    assert (yn[..., 4:4 + ca] - a.grad).abs().max() < TOL
    assert (un[..., 8:8 + ca] - pre.grad).abs().max() < TOL
    # outside the windows: untouched
    assert torch.equal(yn[..., :4], y[..., :4]) and torch.equal(yn[..., 4 + ca:], y[..., 4 + ca:])
    assert torch.equal(un[..., :8], uo[..., :8])
    # a proper sub-range of the columns emits only there
    _, _, us = X.conv_ex(X.DGRAD, x, xc, kc, wb, y, 4, stride=stride, res=res, res_coff=2, accumulate=1, uo=uo, u_coff=8, ua=ua, ua_coff=4,
                         uact=act, ualpha=alpha, u_c0=4, u_c1=8)
    assert torch.equal(us[..., 12:16], un[..., 12:16]) and torch.equal(us[..., 8:12], uo[..., 8:12]) and torch.equal(us[..., 16:], uo[..., 16:])


def test_act_derivative_at_zero_is_the_kernels_convention():
    """common.h act_dfo at a == 0 exactly: a > 0 is false, so leaky gives alpha, ELU a + 1 = 1, none 1"""
    z = torch.tensor([0.0, -0.0, 1.5, -0.25], dtype=torch.float64)
    assert X.act_dfo(z, ACT_LEAKY, 0.1).tolist() == [0.1, 0.1, 1.0, 0.1]
    assert X.act_dfo(z, ACT_ELU, 0.0).tolist() == [1.0, 1.0, 1.0, 0.75]
    assert X.act_dfo(z, ACT_NONE, 0.0).tolist() == [1.0, 1.0, 1.0, 1.0]


def test_act_on_load_is_the_chain_rule():
    """form 1 with xa: dx = dgrad(dy * act'(y)) is autograd's input gradient through act(conv(x))"""
    x0 = rnd(1, 7, 9, 6, seed=11).requires_grad_(True)
    w = rnd(3, 3, 6, 8, seed=12, scale=0.3)
    yv = F.elu(O.conv2d_same(x0, w, None, 1, 1))
    dy = rnd(*yv.shape, seed=13)
    g, = torch.autograd.grad((yv * dy).sum(), [x0])
    yn, _, _ = X.conv_ex(X.DGRAD, dy, 0, 8, w, torch.zeros(1, 7, 9, 6, dtype=torch.float64), 0, xa=yv.detach(), xact=ACT_ELU)
    assert (yn - g).abs().max() < TOL


@pytest.mark.parametrize("hw", [(6, 10), (7, 9)])
def test_up_forms_are_autograd_through_nn_x2_and_3x3(hw):
    h, w = hw
    cin, cout = 6, 5
    x0 = rnd(2, h, w, cin, seed=21).requires_grad_(True)
    wt = rnd(3, 3, cin, cout, seed=22, scale=0.3)
    b = rnd(cout, seed=23, scale=0.1)
    ref = F.elu(_nchw_up_conv(x0, wt) + b)
    du = rnd(2, 2 * h, 2 * w, cout, seed=24)
    lin = _nchw_up_conv(x0, wt)
    g, = torch.autograd.grad((lin * du).sum(), [x0])
    x = torch.full((2, h, w, 12), 2.0, dtype=torch.float64)
    x[..., 4:4 + cin] = x0.detach()
    y = torch.full((2, 2 * h, 2 * w, cout + 3), -5.0, dtype=torch.float64)
    yn, y2n, _ = X.conv_ex(X.UP_FWD, x, 4, 8, wt, y, 1, bias=b, act=ACT_ELU, y2=y.clone(), y2_coff=2)
    assert (yn[..., 1:1 + cout] - ref.detach()).abs().max() < TOL and (y2n[..., 2:2 + cout] - ref.detach()).abs().max() < TOL
    assert torch.equal(yn[..., :1], y[..., :1]) and torch.equal(yn[..., 1 + cout:], y[..., 1 + cout:])
    xd = torch.full((2, 2 * h, 2 * w, 8), 2.0, dtype=torch.float64)
    xd[..., :cout] = du
    old = rnd(2, h, w, cin, seed=25)
    dn, _, _ = X.conv_ex(X.UP_DGRAD, xd, 0, 8, wt, old, 0, accumulate=1)
    assert (dn - (g + old)).abs().max() < TOL


def test_gap_map_is_the_convolution_over_the_channels_with_the_gap_removed():
    """the PWC slab in small: 21 real channels, three junk channels at 13, a K window of 32 at x_coff = 8"""
    cin, ks, kg, kc, xc = 21, 13, 3, 32, 8
    wt = rnd(3, 3, cin, 2, seed=31, scale=0.3)
    b = rnd(2, seed=32)
    x = rnd(1, 6, 8, 48, seed=33)  # junk everywhere, the gap included
    real = torch.cat([x[..., xc:xc + ks], x[..., xc + ks + kg:xc + cin + kg]], -1)
    ref = O.conv2d_same(real, wt, b, 1, 1)
    y = torch.zeros(1, 6, 8, 4, dtype=torch.float64)
    yn, _, _ = X.conv_ex(X.FWD, x, xc, kc, wt, y, 0, bias=b, k_split=ks, k_gap=kg)
    assert (yn[..., :2] - ref).abs().max() < TOL
    # the same through the packed weights' own picture: zero rows at the gap and past the real channels, all 32 window channels multiplied
    wz = torch.zeros(3, 3, kc, 2, dtype=torch.float64)
    wz[:, :, :ks] = wt[:, :, :ks]
    wz[:, :, ks + kg:cin + kg] = wt[:, :, ks:]
    assert (O.conv2d_same(x[..., xc:xc + kc], wz, b, 1, 1) - ref).abs().max() < TOL
    # junk in the gap does not count; a junk value moved INTO a real channel does
    x2 = x.clone()
    x2[..., xc + ks:xc + ks + kg] += 100.0
    assert torch.equal(X.conv_ex(X.FWD, x2, xc, kc, wt, y, 0, bias=b, k_split=ks, k_gap=kg)[0], yn)
    x2[..., xc + ks + kg] += 1.0
    assert not torch.equal(X.conv_ex(X.FWD, x2, xc, kc, wt, y, 0, bias=b, k_split=ks, k_gap=kg)[0], yn)


# ---- the refusals of udet_debug_conv2d_ex: every argument is checked before the first HIP call, so they run without a device ----------------
P16 = 0x10000  # a "pointer": never dereferenced, the call is refused first
GOOD = dict(form=0, n=1, h=8, wd=8, cin=21, cout=8, k=3, stride=1, dilation=1, up=0, kc=32, k_split=13, k_gap=3, x=P16, ldx=48, x_coff=8,
            w=P16, bias=P16, act=2, alpha=0.0, y=P16, ldy=24, y_coff=8, res=P16, ldres=12, res_coff=4, y2=P16, ldy2=8, y2_coff=0,
            accumulate=0)
GOOD_BWD = dict(form=1, n=1, h=8, wd=8, cin=16, cout=8, k=3, stride=1, dilation=1, up=0, kc=8, k_split=8, k_gap=0, x=P16, ldx=8, x_coff=0,
                w=P16, y=P16, ldy=24, y_coff=4, accumulate=1, uo=P16, ldu=24, u_coff=4, ua=P16, ldua=16, ua_coff=0, uact=1, ualpha=0.1,
                u_c0=4, u_c1=12)
ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -5
REFUSALS = [
    # UDET_ERR_ARG: NULL pointers, bad counts, an unknown act or form
    (GOOD, dict(form=4), ERR_ARG), (GOOD, dict(form=-1), ERR_ARG), (GOOD, dict(x=0), ERR_ARG), (GOOD, dict(w=0), ERR_ARG),
    (GOOD, dict(y=0), ERR_ARG), (GOOD, dict(n=0), ERR_ARG), (GOOD, dict(h=0), ERR_ARG), (GOOD, dict(cout=0), ERR_ARG),
    (GOOD, dict(k=8), ERR_ARG), (GOOD, dict(stride=3), ERR_ARG), (GOOD, dict(dilation=0), ERR_ARG), (GOOD, dict(act=3), ERR_ARG),
    (GOOD, dict(accumulate=2), ERR_ARG), (GOOD, dict(up=2), ERR_ARG), (GOOD, dict(k_gap=-1), ERR_ARG), (GOOD, dict(xa=P16, xact=1), ERR_ARG),
    (GOOD, dict(form=2), ERR_ARG),                    # the gap map belongs to form 0
    (GOOD, dict(pack_job=2), ERR_ARG), (GOOD, dict(h=1 << 30, wd=1 << 30), ERR_ARG),   # (4 n h wd is formed in 64 bits)
    (GOOD_BWD, dict(uact=7), ERR_ARG), (GOOD_BWD, dict(ua=0), ERR_ARG), (GOOD_BWD, dict(bias=P16), ERR_ARG), (GOOD_BWD, dict(act=1), ERR_ARG),
    (GOOD_BWD, dict(up=1), ERR_ARG), (GOOD_BWD, dict(form=3, k=5), ERR_ARG), (GOOD_BWD, dict(xact=9), ERR_ARG),
    # UDET_ERR_ALIGN: the A operand's window in float4 groups, float pointers
    (GOOD, dict(ldx=50), ERR_ALIGN), (GOOD, dict(x_coff=6), ERR_ALIGN), (GOOD, dict(kc=30), ERR_ALIGN), (GOOD, dict(x=P16 + 4), ERR_ALIGN),
    (GOOD, dict(y=P16 + 2), ERR_ALIGN), (GOOD, dict(res=P16 + 1), ERR_ALIGN), (GOOD_BWD, dict(ua=P16 + 2), ERR_ALIGN),
    (GOOD_BWD, dict(xa=P16 + 8, xact=1), ERR_ALIGN),
    # UDET_ERR_SHAPE: a window outside its row
    (GOOD, dict(x_coff=20), ERR_SHAPE), (GOOD, dict(kc=20, k_gap=0, k_split=20), ERR_SHAPE), (GOOD, dict(kc=20), ERR_SHAPE),
    (GOOD, dict(k_split=22), ERR_SHAPE), (GOOD, dict(y_coff=17), ERR_SHAPE), (GOOD, dict(y_coff=-1), ERR_SHAPE), (GOOD, dict(res_coff=5), ERR_SHAPE),
    (GOOD, dict(ldy2=7), ERR_SHAPE), (GOOD_BWD, dict(u_c1=17), ERR_SHAPE), (GOOD_BWD, dict(u_c0=13), ERR_SHAPE), (GOOD_BWD, dict(u_coff=16), ERR_SHAPE),
    (GOOD_BWD, dict(ua_coff=8), ERR_SHAPE), (GOOD_BWD, dict(kc=4, k_split=4), ERR_SHAPE), (GOOD_BWD, dict(ldy=16, y_coff=4), ERR_SHAPE),
]


@pytest.fixture(scope="module")
def devel():
    from unsupervised_detection_amd import _devel
    return _devel


@pytest.mark.parametrize("base,change,code", REFUSALS)
def test_conv2d_ex_refuses_before_any_hip_call(devel, base, change, code):
    f = dict(base, **change)
    with pytest.raises(ValueError, match=f"libudet error {code}:.*debug_conv2d_ex"):
        devel.conv2d_ex(workspace=(P16, 1 << 40), stream=0, **f)


@pytest.mark.parametrize("base", [GOOD, GOOD_BWD])
def test_conv2d_ex_refuses_a_bad_workspace(devel, base):
    need = devel.conv2d_ex_workspace_bytes(**base)
    nout = base["cin"] if base["form"] in (1, 3) else base["cout"]
    assert need == 4 * (4224 + (9 * base["kc"] * ((nout + 3) // 4 * 4) + 63) // 64 * 64 + (8 << 20))
    for ws in ((0, need), (P16 + 32, need), (P16, need - 4)):
        with pytest.raises(ValueError, match="libudet error -5:.*workspace"):
            devel.conv2d_ex(workspace=ws, stream=0, **base)
    assert devel.conv2d_ex_workspace_bytes(form=5, kc=8, cin=8, cout=8, k=3) == 0


# ---- the refusals of udet_debug_conv2d_pair_ex: the same discipline for two structs ----------------------------------------------------------
PAIR_FWD = dict(GOOD, k_split=32, k_gap=0, cin=32)                      # a plain forward problem: what fwd_is_plain lets a pair carry
PAIR_BWD = dict(GOOD_BWD)
PAIR_BWD_S2 = dict(GOOD_BWD, stride=2, h=8, wd=12)                      # stride 2 on an even grid: four merged classes, ONE launch
OWN = [  # a struct's own refusals, forwarded: a few of each error class
    (PAIR_FWD, dict(x=0), ERR_ARG), (PAIR_FWD, dict(stride=3), ERR_ARG), (PAIR_BWD, dict(bias=P16), ERR_ARG), (PAIR_BWD, dict(ua=0), ERR_ARG),
    (PAIR_FWD, dict(ldx=50), ERR_ALIGN), (PAIR_FWD, dict(x=P16 + 4), ERR_ALIGN), (PAIR_BWD, dict(ua=P16 + 2), ERR_ALIGN),
    (PAIR_FWD, dict(x_coff=20), ERR_SHAPE), (PAIR_FWD, dict(y_coff=17), ERR_SHAPE), (PAIR_BWD, dict(u_c1=17), ERR_SHAPE),
    (PAIR_BWD, dict(ldy=16, y_coff=4), ERR_SHAPE),
]
PAIR_ONLY = [  # what the single entry takes and a pair does not
    (GOOD_BWD, dict(form=3, k_split=8), ERR_ARG), (dict(PAIR_FWD, cin=32, cout=8), dict(form=2), ERR_ARG),   # forms 2 / 3
    (PAIR_FWD, dict(up=1), ERR_ARG),
    (PAIR_BWD_S2, dict(h=7), ERR_ARG), (PAIR_BWD_S2, dict(wd=11), ERR_ARG), (PAIR_BWD_S2, dict(h=7, wd=11), ERR_ARG),   # one launch per class
]
PAIR_REFUSALS = [(which, base, change, code) for base, change, code in OWN + PAIR_ONLY for which in (0, 1)]


def _pair_partner(base):
    return PAIR_BWD if base["form"] in (1, 3) else PAIR_FWD


@pytest.mark.parametrize("which,base,change,code", PAIR_REFUSALS)
def test_conv2d_pair_ex_refuses_before_any_hip_call(devel, which, base, change, code):
    """problem `which` carries the fault, the other one is sound: either position is checked"""
    bad, good = dict(base, **change), _pair_partner(base)
    with pytest.raises(ValueError, match=f"libudet error {code}:.*debug_conv2d_pair_ex"):
        devel.conv2d_pair_ex(*((good, bad) if which else (bad, good)), workspace=(P16, 1 << 40), stream=0)


def test_conv2d_pair_ex_takes_what_the_single_entry_takes_of_those_bases(devel):
    """the bases of PAIR_ONLY are sound for udet_debug_conv2d_ex with the same change (so the pair's refusal is the pair's own); of these the
    single entry refuses only a bad workspace here"""
    for base, change, _ in PAIR_ONLY:
        f = dict(base, **change)
        assert devel.conv2d_ex_workspace_bytes(**f) > 0
        with pytest.raises(ValueError, match="libudet error -5:.*workspace"):
            devel.conv2d_ex(workspace=(0, 1 << 40), stream=0, **f)


@pytest.mark.parametrize("a,b", [(None, PAIR_FWD), (PAIR_FWD, None), (None, None)])
def test_conv2d_pair_ex_refuses_a_null_struct(devel, a, b):
    with pytest.raises(ValueError, match="libudet error -5:.*debug_conv2d_pair_ex"):
        devel.conv2d_pair_ex(a, b, workspace=(P16, 1 << 40), stream=0)
    assert devel.conv2d_pair_ex_workspace_bytes(a, b) == 0


@pytest.mark.parametrize("a,b", [(PAIR_FWD, dict(PAIR_FWD, n=3, cout=12, ldy=28, ldres=16, ldy2=12)),(PAIR_BWD, PAIR_BWD_S2), (PAIR_BWD_S2, PAIR_FWD)])
def test_conv2d_pair_ex_workspace_formula_and_a_bad_workspace(devel, a, b):
    """header of 4224 floats, the two packed-weight regions (each rounded up to 64 floats), ONE 8 Mi split-K region"""
    def wfl(f):
        nout = f["cin"] if f["form"] == 1 else f["cout"]
        return (f["k"] ** 2 * f["kc"] * ((nout + 3) // 4 * 4) + 63) // 64 * 64
    need = devel.conv2d_pair_ex_workspace_bytes(a, b)
    assert need == 4 * (4224 + wfl(a) + wfl(b) + (8 << 20))
    assert need == devel.conv2d_ex_workspace_bytes(**a) + 4 * wfl(b)
    for ws in ((0, need), (P16 + 32, need), (P16, need - 4)):
        with pytest.raises(ValueError, match="libudet error -5:.*debug_conv2d_pair_ex.*workspace"):
            devel.conv2d_pair_ex(a, b, workspace=ws, stream=0)
    assert devel.conv2d_pair_ex_workspace_bytes(a, dict(b, form=5)) == 0
