"""A convolution launch as a step plan builds it, restated plainly in float64 (csrc/conv_epilogue.h conv_epilogue is the contract):

    v = act(conv + bias);   y2 <- v;   v += res;   v += old y (accumulate);   y <- v;   u <- v * act'(ua) on columns [u_c0, u_c1)

on channel windows of wider buffers, everything outside the windows untouched.  The linear part is oracle_torch.conv2d_same (and the
nearest-neighbour x2 of the generator's up-sampling layers) or, for the backward-data forms, torch.autograd through exactly that -- never a
second hand-derived formula.  tests/test_conv_epilogue_oracle.py ties this file to autograd through a two-layer composite;
tests/test_conv_epilogue_gpu.py holds every kernel family's epilogue to it (include/udet_debug.h udet_debug_conv2d_ex)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import oracle_torch as O
from .oracle_glue import ACT_ELU, ACT_LEAKY, ACT_NONE, act_derivative_from_output

FWD, DGRAD, UP_FWD, UP_DGRAD = 0, 1, 2, 3


def act_fwd(v, act, alpha):
    if act == ACT_LEAKY:
        return O.leaky_relu(v, alpha)
    if act == ACT_ELU:
        return F.elu(v)
    assert act == ACT_NONE
    return v


def act_dfo(a, act, alpha):
    """common.h act_dfo: act' through the stored OUTPUT a; at a == 0 exactly: alpha (leaky), 1 (ELU: a + 1; none)"""
    return act_derivative_from_output(a, act, torch.tensor(alpha, dtype=a.dtype))


def nn_x2(x):
    return O.resize_nearest_align_corners(x, 2 * x.shape[1], 2 * x.shape[2])


def drop_gap(xw, creal, k_split, k_gap):
    """the `creal` real channels of the K window xw [.., kc]: packed row r < k_split is channel r, rows [k_split, k_split + k_gap) are the
    gap (zero weight rows: whatever the tensor holds there does not count), row r beyond is channel r - k_gap; the rest is padding"""
    if k_gap == 0:
        return xw[..., :creal]
    return torch.cat([xw[..., :k_split], xw[..., k_split + k_gap:creal + k_gap]], -1)


def head(x, x_coff, kc, w, bias=None, k_split=None, k_gap=0, transposed=False):
    """a 2-channel head as a plan launches it (udet_debug_conv2d_head_ex): the K window [x_coff, x_coff + kc) of x with the gap dropped,
    through conv2d_same (w HWIO, stride 1) or, transposed, conv2d_transpose_k4s2_same (w HWOI [4, 4, cout, cin]), plus bias"""
    creal = w.shape[3] if transposed else w.shape[2]
    xr = drop_gap(x[..., x_coff:x_coff + kc], creal, kc if k_split is None else k_split, k_gap)
    return O.conv2d_transpose_k4s2_same(xr, w, bias) if transposed else O.conv2d_same(xr, w, bias, 1, 1)


def linear(form, xr, w, out_hw, stride=1, dilation=1, up=0):
    """the launch's sum over taps and real channels; xr: the A operand's real channels (forward forms: the layer's input, backward forms:
    the gradient w.r.t. the layer's output); w HWIO [k, k, cin, cout]; out_hw: the grid of the launch's output (backward forms)"""
    if form == FWD:
        return O.conv2d_same(nn_x2(xr) if up else xr, w, None, stride, dilation)
    if form == UP_FWD:
        return O.conv2d_same(nn_x2(xr), w, None, 1, 1)
    n, cin = xr.shape[0], w.shape[2]
    x0 = torch.zeros(n, out_hw[0], out_hw[1], cin, dtype=xr.dtype, requires_grad=True)
    with torch.enable_grad():
        f = O.conv2d_same(nn_x2(x0), w, None, 1, 1) if form == UP_DGRAD else O.conv2d_same(x0, w, None, stride, dilation)
        assert f.shape == xr.shape, (f.shape, xr.shape)
        g, = torch.autograd.grad((f * xr).sum(), [x0])  # linear in x0: the vector-Jacobian product is the backward-data pass
    return g


def linear_part(form, x, x_coff, kc, w, out_hw, k_split=None, k_gap=0, stride=1, dilation=1, up=0, xa=None, xact=ACT_NONE, xalpha=0.0):
    """the sum a launch's epilogue starts from: the K window of x (times act'(xa) on load), the gap dropped, through linear()"""
    creal = w.shape[3] if form in (DGRAD, UP_DGRAD) else w.shape[2]
    xw = x[..., x_coff:x_coff + kc]
    if xa is not None and xact != ACT_NONE:
        xw = xw * act_dfo(xa[..., x_coff:x_coff + kc], xact, xalpha)
    xr = drop_gap(xw, creal, kc if k_split is None else k_split, k_gap)
    return linear(form, xr, w, out_hw, stride, dilation, up)


def conv_ex(form, x, x_coff, kc, w, y, y_coff, bias=None, k_split=None, k_gap=0, stride=1, dilation=1, up=0, xa=None, xact=ACT_NONE, xalpha=0.0,
            act=ACT_NONE, alpha=0.0, res=None, res_coff=0, y2=None, y2_coff=0, accumulate=0, uo=None, u_coff=0, ua=None, ua_coff=0,
            uact=ACT_NONE, ualpha=0.0, u_c0=0, u_c1=0, lin=None):
    """All tensors NHWC float64 at their full row width; returns (y, y2, uo) after the launch (copies; None where not given).
    lin: the launch's linear part [n, oh, ow, columns] where the caller has it already (linear_part: one convolution serves every option set)."""
    backward = form in (DGRAD, UP_DGRAD)
    cols = w.shape[2] if backward else w.shape[3]
    v = lin if lin is not None else linear_part(form, x, x_coff, kc, w, y.shape[1:3], k_split, k_gap, stride, dilation, up, xa, xact, xalpha)
    assert v.shape[:3] == y.shape[:3] and v.shape[3] == cols, (v.shape, y.shape)
    if bias is not None:
        v = v + bias
    v = act_fwd(v, act, alpha)
    y_new, y2_new, u_new = y.clone(), None, None
    if y2 is not None:
        y2_new = y2.clone()
        y2_new[..., y2_coff:y2_coff + cols] = v
    if res is not None:
        v = v + res[..., res_coff:res_coff + cols]
    if accumulate:
        v = v + y[..., y_coff:y_coff + cols]
    y_new[..., y_coff:y_coff + cols] = v
    if uo is not None:
        u_new = uo.clone()
        u_new[..., u_coff + u_c0:u_coff + u_c1] = v[..., u_c0:u_c1] * act_dfo(ua[..., ua_coff + u_c0:ua_coff + u_c1], uact, ualpha)
    return y_new, y2_new, u_new
