"""CPU checks of what tests/test_heads_gpu.py and tests/test_warp_cost_volume_slab_gpu.py rely on: the head reference of
oracle/oracle_conv_ex.py (window + gap map + convolution + bias) against torch.nn.functional in float64 with the channel map written out as
an index list, the operands of the head cases, and the warp oracle's index math on the saturating flow vectors."""
import torch
import torch.nn.functional as F

from oracle import oracle_conv_ex as X
from oracle import oracle_torch as O
from test_heads_gpu import CASES, FORWARD, FP16_CASES, GAP_GARBAGE, TRANSPOSED, X_COFF, geometry, operands, reference, x_nhwc
from test_warp_cost_volume_slab_gpu import SATURATING, saturating_flow


def real_channel_columns(g):
    """column of x of every real channel, from the packed-row rule of include/udet_debug.h: row r < k_split is channel r, rows
    [k_split, k_split + k_gap) are the gap, row r beyond is channel r - k_gap"""
    cols = [None] * g["cin"]
    for r in range(g["kc"]):
        ch = r if r < g["k_split"] else (None if r < g["k_split"] + g["k_gap"] else r - g["k_gap"])
        if ch is not None and ch < g["cin"]:
            cols[ch] = X_COFF + r
    assert None not in cols
    return cols


def test_head_reference_is_torch_functional_on_the_real_channels():
    for case in (FORWARD[4], TRANSPOSED[2], FORWARD[0]):  # both gap maps and a gap-free window
        g, d = geometry(case), operands(case)
        x = x_nhwc(case).double()
        xr = x[..., real_channel_columns(g)].permute(0, 3, 1, 2)
        assert float(xr.abs().max()) < 100  # neither the sentinel nor the gap's garbage is among the real channels
        w, b = d["w"].double(), d["bias"].double()
        if g["tr"]:
            y = F.conv_transpose2d(xr, w.permute(3, 2, 0, 1), b, stride=2, padding=1)
        else:
            y = F.conv2d(xr, w.permute(3, 2, 0, 1), b, padding=g["k"] // 2)
        y = y.permute(0, 2, 3, 1).reshape(-1, 2)
        ref = reference(case)
        assert ref.shape == y.shape and float((ref - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))


def test_head_cases_hold_what_they_claim():
    for case in CASES:
        g, d = geometry(case), operands(case)
        x = x_nhwc(case)
        assert g["ldx"] % 4 == 0 and g["kc"] % 4 == 0 and g["cin"] + g["k_gap"] <= g["kc"] and g["k"] * g["k"] * 2 <= 64
        win = x[..., X_COFF:X_COFF + g["kc"]]
        gap = win[..., g["k_split"]:g["k_split"] + g["k_gap"]]
        assert (gap == GAP_GARBAGE).all() and torch.isfinite(win).all()
        assert int((win == GAP_GARBAGE).sum()) == gap.numel()
        assert (x[..., :X_COFF] == x[0, 0, 0, 0]).all() and (x[..., X_COFF + g["kc"]:] == x[0, 0, 0, 0]).all()  # the sentinel around the window
        assert d["w"].shape == ((4, 4, 2, g["cin"]) if g["tr"] else (g["k"], g["k"], g["cin"], 2))
    assert sum(1 for c in CASES if geometry(c)["k_gap"]) == 2
    for case in FP16_CASES:  # fp16 operands: normal fp16 numbers throughout the K window, no gap
        from test_fp16_kernels_gpu import r16
        g = geometry(case)
        assert g["k_gap"] == 0
        r16(x_nhwc(case, True)[..., X_COFF:X_COFF + g["kc"]])
        r16(operands(case, True)["w"])


def test_warp_oracle_saturates_on_huge_flow_vectors():
    """the +-1e9 vectors of the slab test: O.warp_indices clamps them to in-range corner indices and alphas in [0, 1], so the float64
    reference of that case is well defined (and finite)"""
    n, h, w, c, scale = SATURATING
    flow = saturating_flow()
    assert int((flow.abs() >= 1e9).sum()) >= 8 and torch.isfinite(flow).all()
    fy, fx, ay, ax = O.warp_indices(flow * scale)
    assert int(fy.min()) >= 0 and int(fy.max()) <= h - 2 and int(fx.min()) >= 0 and int(fx.max()) <= w - 2
    for a in (ay, ax):
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and torch.isfinite(a).all()
    big = flow.abs().amax(-1) >= 1e9
    assert ((ay[big] == 0) | (ay[big] == 1) | (ax[big] == 0) | (ax[big] == 1)).all()
    img = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(3)).double()
    assert torch.isfinite(O.dense_image_warp(img, (flow * scale).double())).all()
