"""The fused warp -> cost volume launch with the arguments a plan gives it (csrc/plan_step.hip pwc_forward_on), through
udet_debug_warp_cost_volume_ex (include/udet_debug.h): IN PLACE on a level's slab -- the flow read from columns [532 + C, 532 + C + 2) of
the buffer that is written, the 81 correlations to columns [448, 529), c1 copied to [532, 532 + C) -- where the public udet_warp_cost_volume
only ever passes a dense flow, a dense 81-column output and no c1 segment.

Each case builds the slab of a level (row width 532 + C + 4 rounded up to 8) between guard rows, fills all of it with SENTINEL, puts the
flow into its columns and calls the launcher in place.  Then
  * the corr window equals udet_warp_cost_volume on contiguous copies of the same data bit for bit, and the float64 oracle
    O.cost_volume(c1, O.dense_image_warp(c2, flow * scale)) within 1e-5 (the bound of test_ops_gpu.py);
  * the c1 window equals c1 bit for bit;
  * every other float of the slab and of the guard rows is unchanged: the gap columns 529..531, the flow, the columns behind it;
  * a second call into a fresh slab with the flow in a separate [P, 2] tensor gives the same two windows bit for bit.
The shapes reach the launcher's regimes: 4x4 tiles on 4 XCDs with the last XCD's surplus workgroups leaving, 8x8 tiles with a narrower
last channel slice and partial tiles, level 6 (no flow, no c1 segment), a single XCD, and flow vectors of +-1e9 whose indices saturate."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_torch as O  # noqa: E402
from oracle.oracle_glue import SENTINEL  # noqa: E402

GUARD = 2
CORR, C1 = 448, 532
# (n, h, w, C, scale); scale None: flow = NULL and c1_coff = -1, as level 6
CASES = [(2, 20, 28, 32, 5.0),      # 4x4 tiles: 70 tiles on 4 XCDs, 18 workgroups each -- the last XCD's slots 70 and 71 leave
         (1, 67, 70, 36, 2.5),      # 8x8 tiles (4690 pixels): channel slices 16 + 16 + 4, partial tiles on both axes
         (4, 6, 10, 196, None),     # level 6
         (1, 5, 7, 4, 1.0),         # one XCD, tiles wider than the image's remainder
         (2, 13, 21, 36, 1.25)]
SATURATING = (2, 13, 21, 36, 1.25)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ordinary_flow(n, h, w):
    return rnd(n, h, w, 2, seed=73, scale=2.0)


def saturating_flow():
    """ordinary vectors with a handful of +-1e9 components among them: corners, an edge, the interior, both signs on both axes"""
    n, h, w, _, _ = SATURATING
    f = ordinary_flow(n, h, w)
    for (b, y, x), v in (((0, 0, 0), (1e9, 0.5)), ((0, 0, w - 1), (-1e9, -1e9)), ((0, h - 1, 0), (0.25, 1e9)), ((1, h - 1, w - 1), (1e9, 1e9)),
                         ((1, 6, 10), (-1e9, 0.75)), ((0, 7, 3), (1e9, -1e9)), ((1, 0, 11), (-0.5, -1e9)), ((0, 12, 20), (-1e9, 1e9))):
        f[b, y, x, 0], f[b, y, x, 1] = v
    return f


@functools.lru_cache(maxsize=None)
def problem(case, saturating=False):
    """host operands and the float64 reference, computed once"""
    n, h, w, c, scale = case
    c1, c2 = rnd(n, h, w, c, seed=71), rnd(n, h, w, c, seed=72)
    flow = None if scale is None else (saturating_flow() if saturating else ordinary_flow(n, h, w))
    warped = c2.double() if flow is None else O.dense_image_warp(c2.double(), flow * np.float32(scale))
    ref = O.cost_volume(c1.double(), warped)
    assert torch.isfinite(ref).all()
    return dict(c1=c1, c2=c2, flow=flow, ref=ref)


def slab_of(case, flow):
    """the level's slab between guard rows, all SENTINEL, the flow (when given) in its columns"""
    n, h, w, c, _ = case
    ld = (C1 + c + 4 + 7) // 8 * 8
    s = torch.full((GUARD + n * h * w + GUARD, ld), SENTINEL)
    if flow is not None:
        s[GUARD:GUARD + n * h * w, C1 + c:C1 + c + 2] = flow.reshape(-1, 2)
    return s


@pytest.fixture(scope="module")
def devel():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import _devel
    return _devel


def run_case(devel, case, saturating=False):
    from unsupervised_detection_amd import ops
    n, h, w, c, scale = case
    p = problem(case, saturating)
    rows = n * h * w
    c1g, c2g = p["c1"].cuda(), p["c2"].cuda()
    flow = p["flow"]
    c1_coff = C1 if flow is not None else -1
    fscale = 1.0 if scale is None else scale

    # in place on the slab, as the plan calls it
    init = slab_of(case, flow)
    slab = init.cuda()
    ld = init.shape[1]
    body = (slab, GUARD * ld)
    devel.warp_cost_volume_ex(c1g, c2g, body if flow is not None else None, ld, C1 + c, fscale, body, ld, CORR, c1_coff, n, h, w, c)
    torch.cuda.synchronize()
    got = slab.cpu()
    # the public entry on contiguous copies
    pub = ops.warp_cost_volume(c1g, c2g, None if flow is None else flow.cuda(), fscale).cpu().reshape(rows, 81)

    def windows_and_rest(buf, start):
        """(corr window, c1 window, everything else flattened) of a slab after a call"""
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[GUARD:GUARD + rows, CORR:CORR + 81] = False
        if c1_coff >= 0:
            keep[GUARD:GUARD + rows, C1:C1 + c] = False
        assert torch.equal(buf[keep], start[keep]), ("floats outside the corr / c1 windows changed", int((buf[keep] != start[keep]).sum()))
        b = buf[GUARD:GUARD + rows]
        return b[:, CORR:CORR + 81], (b[:, C1:C1 + c] if c1_coff >= 0 else None)

    corr, c1w = windows_and_rest(got, init)
    assert torch.isfinite(corr).all()
    assert torch.equal(corr, pub), ("corr window against udet_warp_cost_volume", int((corr != pub).sum()), float((corr - pub).abs().max()))
    err = float((corr.double() - p["ref"].reshape(rows, 81)).abs().max())
    print("%s%s: corr %.2e against float64 (bound 1e-5)" % (case, " saturating" if saturating else "", err))
    assert err < 1e-5
    if c1_coff >= 0:
        assert torch.equal(c1w, p["c1"].reshape(rows, c)), "c1 window"
        # the flow in a tensor of its own, a fresh slab without it
        init2 = slab_of(case, None)
        slab2 = init2.cuda()
        fg = flow.reshape(rows, 2).contiguous().cuda()
        devel.warp_cost_volume_ex(c1g, c2g, fg, 2, 0, fscale, (slab2, GUARD * ld), ld, CORR, c1_coff, n, h, w, c)
        torch.cuda.synchronize()
        corr2, c1w2 = windows_and_rest(slab2.cpu(), init2)
        assert torch.equal(corr2, corr) and torch.equal(c1w2, c1w), "a separate flow tensor gives other windows than the in-place call"
        assert torch.equal(fg.cpu(), flow.reshape(rows, 2))
    assert torch.equal(c1g.cpu(), p["c1"]) and torch.equal(c2g.cpu(), p["c2"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_warp_cost_volume_in_place_on_a_slab(devel, case):
    run_case(devel, case)


def test_warp_cost_volume_saturating_flow_vectors(devel):
    """+-1e9 among ordinary vectors: floor indices clamp to [0, H - 2] x [0, W - 2], alphas to 0 / 1 (tests/test_heads_oracle.py checks the
    oracle's side of this on the CPU); the result is finite and still the oracle's"""
    run_case(devel, SATURATING, saturating=True)
