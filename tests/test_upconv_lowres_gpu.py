"""GPU: one level of the recover decoder in its low-resolution up-conv form (csrc/plan_exec.hip upb_forward / upb_dgrad, reached through
libudet_debug's udet_debug_upconv_lowres_fwd / _bwd, which run the plan's own ring kernels, pack jobs, tables and launches) against the
float64 definition of the layer on the CPU: oracle_torch's legacy bilinear x2, conv2d_same 4x4, bias, leaky 0.2; backward-data =
torch.autograd.grad of the linear layer.  Nothing in a reference comes from the algebra under test, except the ringed gradient BEFORE the
fold, which only exists as the gradient of a function of the ringed source: that function is test_upconv_tables.lowres_forward, stated
from merged weights the CPU test derives from the definition and holds to resize + conv at 1e-12.

Bounds: the project's fp32 rule of the same operators (test_ops_gpu.py, test_fp16_kernels_gpu.py),
    forward 1e-4 * max(1, max|ref|),  backward-data 2e-4 * max(1, max|ref|),
asserted per REGION of the tables (first row / column, last two rows / columns, corner blocks, interior; row groups R < h-1, h-1, h, h+1
of the ringed gradient) so that a failure names the segment family at fault.  The worst ratio error / scale per group is printed at the end."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_torch as O  # noqa: E402
from test_fp16_kernels_gpu import GRAD_RUNS, mag, r16  # noqa: E402
from test_ops_gpu import FAMILIES, GEMM_TILES, TILE_CONFIGS, TILE_FAMILIES, WS_OF  # noqa: E402
from test_upconv_tables import (dyadic_weights, layer_linear, lowres_forward, merged_exact_in_fp16, merged_weights, ring,  # noqa: E402
                                ring_fold)

LEAKY, ALPHA = 1, 0.2
WORST = {}  # group -> worst error / scale


def _r4(v):
    return (v + 3) // 4 * 4


def _kt(cout):
    return (cout + 3) // 4 * 4 if cout <= 4 else (cout + 7) // 8 * 8


# (h, w, n, cin, cout, ldx).  Every source grid at both batch sizes on a ragged channel pair (cin % 8 != 0, cout % 4 != 0; cout <= 16: the split
# form runs too); the decoder's own pairs (DEC, csrc/plan_build.hip) at one small grid each, read out of a wider slab where the plan's
# slab is wider; sources with ldx > cin.
GRIDS = [(2, 2), (2, 5), (3, 2), (4, 4), (4, 8), (5, 7), (12, 20), (9, 33)]
CASES = [(h, w, n, 12, 6, 12) for h, w in GRIDS for n in (1, 3)] + [
    (4, 4, 1, 384, 128, 384),   # deconv4
    (4, 8, 1, 386, 64, 392),    # deconv3
    (5, 7, 3, 194, 32, 200),    # deconv2
    (12, 20, 1, 98, 16, 104),   # deconv1: the plan's split level
    (5, 7, 3, 12, 6, 20),       # ldx > cin
    (4, 8, 1, 24, 16, 40),
]
IDS = ["%dx%d-n%d-%dto%d-ld%d" % c for c in CASES]


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def reference(case):
    """float32 operands of a case and its float64 results, computed once and never modified"""
    h, w, n, cin, cout, ldx = case
    x = rnd(n, h, w, ldx, seed=1)  # (channels past cin meet zero weight rows: finite values, as in the plan's slab)
    wt = rnd(4, 4, cin, cout, seed=2, scale=(2.0 / (16 * cin)) ** 0.5)
    b = rnd(cout, seed=3, scale=0.1)
    dy = rnd(n, 2 * h, 2 * w, cout, seed=4)
    return dict(x=x, w=wt, b=b, dy=dy, **results(x[..., :cin].double(), wt.double(), b.double(), dy.double()))


def results(x, wt, b, dy):
    xv = x.clone().requires_grad_(True)
    lin = layer_linear(xv, wt)
    gx, = torch.autograd.grad((lin * dy).sum(), [xv])
    lin = lin.detach()
    xh = ring(x).requires_grad_(True)
    gh, = torch.autograd.grad((lowres_forward(xh, merged_weights(wt)) * dy).sum(), [xh])
    return dict(lin=lin, y=O.leaky_relu(lin + b, ALPHA), gx=gx, gh=gh)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
class Dev:
    def __init__(self):
        from unsupervised_detection_amd import _devel
        from unsupervised_detection_amd._ffi import check, lib
        self.dbg, self.check, self.lib, self.wsets_off = _devel.dbg, check, lib, _devel.UPCONV_WSETS_OFFSET
        need = max(self.dbg.udet_debug_upconv_lowres_workspace_bytes(c[5], c[3], c[4]) for c in CASES + [(0, 0, 0, 40, 100, 40)])
        self.ws = torch.zeros(need // 4 + (4 << 20), dtype=torch.float32, device="cuda")  # (+ 4 Mi floats of split-K slabs)

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def fwd(self, case, x, wt, b, act=LEAKY, alpha=ALPHA, split=False, ldy=None, y_coff=0, canary=0.0, status=False):
        """-> (y buffer [n,2h,2w,ldy], xhat [n,h+2,w+2,ldx]) on the CPU"""
        h, w, n, cin, cout, ldx = case
        ldy = _r4(cout) if ldy is None else ldy
        y = torch.full((n, 2 * h, 2 * w, ldy), canary, device="cuda")
        xhat = torch.full((n, h + 2, w + 2, ldx), canary, device="cuda")
        xd, wd, bd = x.cuda().contiguous(), wt.cuda().contiguous(), None if b is None else b.cuda().contiguous()
        st = self.dbg.udet_debug_upconv_lowres_fwd(self._p(xd), ldx, self._p(wd), self._p(bd), act, alpha, self._p(y), ldy, y_coff, self._p(xhat), n, h, w,
                                                   cin, cout, 1 if split else 0, self._p(self.ws), self.ws.numel() * 4,
                                                   torch.cuda.current_stream().cuda_stream)
        if status:
            return st, y.cpu(), xhat.cpu()
        self.check(st)
        return y.cpu(), xhat.cpu()

    def bwd(self, case, dy, wt, ldy=None, y_coff=0, canary=0.0, status=False):
        """dy [n,2h,2w,cout] placed at y_coff of a buffer of random finite values -> (dx [n,h,w,ldx], dxhat [n,h+2,w+2,ldx]) on the CPU"""
        h, w, n, cin, cout, ldx = case
        ldy = _kt(cout) if ldy is None else ldy
        buf = rnd(n, 2 * h, 2 * w, ldy, seed=9)
        if y_coff + cout <= ldy:
            buf[..., y_coff:y_coff + cout] = dy
        dyd, wd = buf.cuda().contiguous(), wt.cuda().contiguous()
        dx = torch.full((n, h, w, ldx), canary, device="cuda")
        dxhat = torch.full((n, h + 2, w + 2, ldx), canary, device="cuda")
        st = self.dbg.udet_debug_upconv_lowres_bwd(self._p(dyd), ldy, y_coff, self._p(wd), self._p(dx), ldx, self._p(dxhat), n, h, w, cin, cout,
                                                   self._p(self.ws), self.ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
        if status:
            return st, dx.cpu(), dxhat.cpu()
        self.check(st)
        return dx.cpu(), dxhat.cpu()

    def last(self):
        v = self.dbg.udet_debug_last_conv()
        return dict(fam=v & 0xff, bm=(v >> 8) & 0xfff, ks=(v >> 20) & 0xff, fold=(v >> 28) & 1, tail=(v >> 29) & 1)

    def wsets(self, k, ld):
        """the four packed weight sets of the last call: [144][k][ld]"""
        return self.ws[self.wsets_off:self.wsets_off + 144 * k * ld].cpu().reshape(144, k, ld)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = Dev()
    yield d
    d.dbg.udet_debug_force_conv(0, 0, -1)
    d.dbg.udet_debug_conv_fp16_grad_scale(0.0)
    d.dbg.udet_debug_conv_fp16(0)
    print()
    for group in sorted(WORST):
        print("upconv lowres %-46s worst error / scale %.2e" % (group, WORST[group]))


@pytest.fixture
def hooks(dev):
    yield dev.dbg
    dev.dbg.udet_debug_force_conv(0, 0, -1)
    dev.dbg.udet_debug_conv_fp16_grad_scale(0.0)
    dev.dbg.udet_debug_conv_fp16(0)


# ---- regions ------------------------------------------------------------------------------------------------------------------------------
def forward_regions(h, w):
    """name -> mask [2h, 2w]: where the negated ring has to cancel, where the last-row / last-column / corner weight sets act, the rest"""
    oy, ox = torch.arange(2 * h)[:, None], torch.arange(2 * w)[None, :]
    first, last2 = (oy == 0) | (ox == 0), (oy >= 2 * h - 2) | (ox >= 2 * w - 2)
    return {"first row / column": first, "last two rows / columns": last2,
            "corner 2x2 blocks": ((oy < 2) | (oy >= 2 * h - 2)) & ((ox < 2) | (ox >= 2 * w - 2)), "interior": ~first & ~last2}


def ringed_regions(h, w):
    """name -> mask [h + 2, w + 2]: the 16 segments of the backward-data table (n = h for rows, w for columns)"""
    def groups(n):
        r = torch.arange(n + 2)
        return {"< n-1": r < n - 1, "= n-1": r == n - 1, "= n": r == n, "= n+1": r == n + 1}
    return {"rows R %s, columns C %s" % (a, b): ma[:, None] & mb[None, :] for a, ma in groups(h).items() for b, mb in groups(w).items()}


def check(group, got, ref, coeff, regions, unit=1.0, record=True):
    """got / ref [n, H, W, c]: the bound on every region, every region that misses it named in the failure; -> worst ratio"""
    assert torch.isfinite(got).all(), group
    err = (got.double() - ref).abs().amax(dim=(0, 3))
    scale = max(unit, float(ref.abs().max()))
    bad, worst = [], 0.0
    for name, mask in regions.items():
        if not bool(mask.any()):
            continue
        e = float(err[mask].max()) / scale
        worst = max(worst, e)
        for part in (name.split(", ") if record else []):  # (ringed gradient: booked under its row group and under its column group)
            key = "%s, %s" % (group.split(" [")[0].replace(" window", ""), part)
            WORST[key] = max(WORST.get(key, 0.0), e)
        if not e < coeff:
            bad.append("%s: %.3e" % (name, e))
    assert not bad, "%s misses %.0e of the scale %.3g in: %s" % (group, coeff, scale, "; ".join(bad))
    return worst


def forward_all_forms(dev, case, r, tag, x=None, y_ref=None):
    """unsplit, split (cout <= 16) and into a channel window of a canary-filled buffer"""
    h, w, n, cin, cout, ldx = case
    x = r["x"] if x is None else x
    y_ref = r["y"] if y_ref is None else y_ref
    regions = forward_regions(h, w)
    for split in ([False, True] if cout <= 16 else [False]):
        form = "split" if split else "unsplit"
        y, _ = dev.fwd(case, x, r["w"], r["b"], split=split)
        check("%s %s [%s]" % (tag, form, IDS[CASES.index(case)]), y[..., :cout], y_ref, 1e-4, regions)
        ldy, y_coff, canary = _r4(cout) + 12, 4, -7777.25
        yw, _ = dev.fwd(case, x, r["w"], r["b"], split=split, ldy=ldy, y_coff=y_coff, canary=canary)
        check("%s %s window [%s]" % (tag, form, IDS[CASES.index(case)]), yw[..., y_coff:y_coff + cout], y_ref, 1e-4, regions)
        outside = torch.cat([yw[..., :y_coff], yw[..., y_coff + cout:]], 3)
        assert torch.equal(outside.view(torch.int32), torch.full_like(outside, canary).view(torch.int32)), "a float outside the window changed"


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward(dev, case):
    forward_all_forms(dev, case, reference(case), "forward")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_impulse(dev, case):
    """x = one-hot pixels at the four corners and one interior pixel (each in a channel of its own), random weights: every output the
    impulse reaches is a single merged weight or a sum of two -- a wrong tap offset or weight set in ONE segment fails, by region"""
    h, w, n, cin, cout, ldx = case
    r = reference(case)
    x = torch.zeros(n, h, w, ldx)
    pixels = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)] + ([(h // 2, w // 2)] if h >= 3 and w >= 3 else [])
    for k, (py, px) in enumerate(pixels):
        x[:, py, px, k % cin] = 1.0 + k
    y_ref = O.leaky_relu(layer_linear(x[..., :cin].double(), r["w"].double()) + r["b"].double(), ALPHA)
    forward_all_forms(dev, case, r, "forward impulse", x=x, y_ref=y_ref)


# ---- backward-data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_data(dev, case):
    h, w, n, cin, cout, ldx = case
    r = reference(case)
    whole = {"whole dx": torch.ones(h, w, dtype=torch.bool)}
    for ldy, y_coff in ((None, 0), (_kt(cout) + 12, 8)):
        canary = 3.0
        dx, dxhat = dev.bwd(case, r["dy"], r["w"], ldy=ldy, y_coff=y_coff, canary=canary)
        tag = "backward-data%s [%s]" % (" window" if y_coff else "", IDS[CASES.index(case)])
        check(tag, dx[..., :cin], r["gx"], 2e-4, whole)
        # the ringed gradient before the fold, by segment (the bound is the whole gradient's: same operator, same scale rule)
        check(tag.replace("backward-data", "ringed gradient"), dxhat[..., :cin], r["gh"], 2e-4, ringed_regions(h, w))
        # channels past cin of the ringed gradient are not the launch's to write; the fold writes every channel of dx: the ring's adjoint of them
        assert torch.equal(dxhat[..., cin:], torch.full_like(dxhat[..., cin:], canary))
        fold = ring_fold(dxhat.double())
        assert float((dx.double() - fold).abs().max()) <= 1e-6 * max(1.0, float(fold.abs().max()))  # (at most four fp32 additions)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adjoint_identity(dev, case):
    """<fwd(x), dy> = <x, bwd(dy)> with bias and activation off, both sides in float64 from the GPU's outputs: ties the two tap tables and the
    two families of weight sets together without the oracle.  dy is correlated with fwd(x) so that the products do not cancel: the
    identity is held to 1e-5 of its own value."""
    h, w, n, cin, cout, ldx = case
    r = reference(case)
    lin = r["lin"]
    dy = (lin / float(lin.abs().max()) + 0.25 * rnd(*lin.shape, seed=11).double()).float()
    y, _ = dev.fwd(case, r["x"], r["w"], None, act=0, alpha=0.0)
    dx, _ = dev.bwd(case, dy, r["w"])
    lhs = float((y[..., :cout].double() * dy.double()).sum())
    rhs = float((r["x"][..., :cin].double() * dx[..., :cin].double()).sum())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    WORST["adjoint identity, relative"] = max(WORST.get("adjoint identity, relative", 0.0), rel)
    assert rel < 1e-5, (lhs, rhs)


# ---- ring kernels, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,cin", [(4, 3), (36, 33)])
@pytest.mark.parametrize("h,w,n", [(2, 2, 1), (5, 7, 3)])
def test_ring_kernels_are_exact(dev, h, w, n, ld, cin):
    """x^ = the test's own ring of x bit for bit, signs included, over all ld channels; the fold of an integer-valued ringed gradient (integer
    dy, weights that are multiples of 4: the merges carry 1/2 per axis, so every merged weight and every sum is an integer, exact in fp32 in any order) = the test's adjoint, exactly,
    the channels past cin (left at an integer canary by the launch) included"""
    case = (h, w, n, cin, 6, ld)
    g = torch.Generator().manual_seed(5)
    x = rnd(n, h, w, ld, seed=6)
    wt = (torch.randint(-2, 3, (4, 4, cin, 6), generator=g) * 4).float()
    _, xhat = dev.fwd(case, x, wt, None, act=0, alpha=0.0)
    assert torch.equal(xhat.view(torch.int32), ring(x).view(torch.int32))
    dy = torch.randint(-3, 4, (n, 2 * h, 2 * w, 6), generator=g).float()
    dx, dxhat = dev.bwd(case, dy, wt, canary=7.0)
    xv = x[..., :cin].double().requires_grad_(True)
    gx, = torch.autograd.grad((layer_linear(xv, wt.double()) * dy.double()).sum(), [xv])
    assert torch.equal(dxhat, dxhat.round()) and torch.equal(dxhat[..., cin:], torch.full_like(dxhat[..., cin:], 7.0))
    assert torch.equal(dx.double(), ring_fold(dxhat.double()))
    assert torch.equal(dx[..., :cin].double(), gx)


# ---- the pack kernel's weight sets ----------------------------------------------------------------------------------------------------------
def test_packed_weight_sets_are_the_derived_merges(dev):
    """(5, 7), 12 -> 6 channels out of a 20-channel slab: the sets pack modes 9 / 10 write, read back from the workspace, against the merge
    matrices the CPU test derives from the definition -- values to fp32 rounding of a 9-term sum, zero rows / columns exactly"""
    case = (5, 7, 3, 12, 6, 20)
    h, w, n, cin, cout, ldx = case
    r = reference(case)
    wm = merged_weights(r["w"].double())
    tol = 4 * 2.0 ** -24 * float(wm.abs().max()) * 4
    dev.fwd(case, r["x"], r["w"], r["b"])
    got = dev.wsets(ldx, _r4(cout))
    assert float((got[:, :cin, :cout].double() - wm).abs().max()) < tol
    assert not got[:, cin:].any() and not got[:, :, cout:].any()
    dev.bwd(case, r["dy"], r["w"])
    got = dev.wsets(_kt(cout), _r4(cin))
    assert float((got[:, :cout, :cin].double() - wm.transpose(1, 2)).abs().max()) < tol
    assert not got[:, cout:].any() and not got[:, :, cin:].any()


# ---- every family and tile on the segmented launches ---------------------------------------------------------------------------------------
# Families that take no segmented launch, by name, with the rule that excludes them; a forced one falls back to the built-in choice
SEGMENTS_REFUSED = {"tile8": "conv_select.hip tile_ok(): `if (p.nseg) return false;  // segmented launches: implicit-GEMM families only`",
                    "tile4": "conv_select.hip tile_ok(): `if (p.nseg) return false;  // segmented launches: implicit-GEMM families only`"}
FORCE_CASES = [(5, 7, 2, 40, 100, 40), (12, 20, 2, 40, 100, 40)]  # 40 -> 100 / 104 -> 40 channels: partial N tiles, K deep enough to split
FORCED = ([("family", f) + FAMILIES[f] + (WS_OF[f],) for f in FAMILIES]
          + [("tile", "%s_%dx%d" % (f, bm, bn), bm + ((1 << 19) if f == "self_staging" else TILE_FAMILIES[f][0]), bn, 1,
              6 if f == "self_staging" else TILE_FAMILIES[f][1]) for f, bm, bn in TILE_CONFIGS])


def test_every_implicit_gemm_family_is_forced_on_segmented_launches():
    ran = {fam for kind, name, bm, bn, ks, fam in FORCED if name not in SEGMENTS_REFUSED}
    assert ran == {0, 1, 2, 4, 5, 6} and {WS_OF[f] for f in SEGMENTS_REFUSED} == {3}
    assert len([f for f in FORCED if f[0] == "tile"]) == 5 * len(GEMM_TILES) + 5


@pytest.mark.parametrize("case", FORCE_CASES, ids=["%dx%d" % c[:2] for c in FORCE_CASES])
@pytest.mark.parametrize("forced", FORCED, ids=[f[1] for f in FORCED])
def test_forced_family_and_tile_on_segmented_launches(dev, hooks, case, forced):
    kind, name, bm, bn, ks, fam = forced
    h, w, n, cin, cout, ldx = case
    r = reference(case)
    hooks.udet_debug_force_conv(bm, bn, ks)
    y, _ = dev.fwd(case, r["x"], r["w"], r["b"])
    lf = dev.last()
    check("forward forced", y[..., :cout], r["y"], 1e-4, forward_regions(h, w))
    dx, dxhat = dev.bwd(case, r["dy"], r["w"])
    lb = dev.last()
    check("ringed gradient forced", dxhat[..., :cin], r["gh"], 2e-4, ringed_regions(h, w))
    check("backward-data forced", dx[..., :cin], r["gx"], 2e-4, {"whole dx": torch.ones(h, w, dtype=torch.bool)})
    if name in SEGMENTS_REFUSED:
        assert lf["fam"] != fam and lb["fam"] != fam
        pytest.skip("refused for segmented launches (the built-in choice ran, results checked): " + SEGMENTS_REFUSED[name])
    for direction, last in (("forward", lf), ("backward-data", lb)):
        assert last["fam"] == fam and last["bm"] == bm & 0xfff, (direction, name, last)  # the configuration under test really ran
        if ks > 1:
            assert last["ks"] > 1 and last["fold"] == (1 if "_fold" in name else 0), (direction, name, last)


# ---- fp16 mode ----------------------------------------------------------------------------------------------------------------------------
FP16_CASES = [(5, 7, 3, 24, 16, 24), (12, 20, 1, 40, 100, 40), (4, 8, 1, 24, 16, 40)]


@functools.lru_cache(maxsize=None)
def fp16_reference(case):
    """test_fp16_kernels_gpu.py's rounded-operand rule.  The kernel rounds x^ (= +-x: the same rounding) and the MERGED weights; the weights
    are drawn where every merged weight is exact in fp16 (asserted), so rounding x / dy alone gives the kernel's operands."""
    h, w, n, cin, cout, ldx = case
    x = mag(n, h, w, ldx, seed=21)
    wt = dyadic_weights(cin, cout, seed=22)
    assert merged_exact_in_fp16(wt)
    b = mag(cout, seed=23, scale=0.1)
    dys = [mag(n, 2 * h, 2 * w, cout, seed=24 + i, scale=m) for i, (_, m) in enumerate(GRAD_RUNS)]
    out = dict(x=x, w=wt, b=b, dy=dys, r=[], u=[])
    for i, (gs, _) in enumerate(GRAD_RUNS):
        out["r"].append(results(r16(x[..., :cin]), wt.double(), b.double(), r16(dys[i], gs)))
        out["u"].append(results(x[..., :cin].double(), wt.double(), b.double(), dys[i].double()))
    return out


def check_fp16(group, got, ref_r, ref_u, coeff, regions, unit=1.0):
    e_r = check(group, got, ref_r, coeff, regions, unit=unit) * max(unit, float(ref_r.abs().max()))
    e_u = float((got.double() - ref_u).abs().max())
    assert e_u > 0 and e_u >= 10 * e_r, (group, "fp16 arithmetic did not run", e_r, e_u)


@pytest.mark.parametrize("case", FP16_CASES, ids=["%dx%d-n%d-%dto%d-ld%d" % c for c in FP16_CASES])
def test_fp16_mode(dev, hooks, case):
    h, w, n, cin, cout, ldx = case
    f = fp16_reference(case)
    hooks.udet_debug_conv_fp16(1)
    for split in ([False, True] if cout <= 16 else [False]):
        y, _ = dev.fwd(case, f["x"], f["w"], f["b"], split=split)
        assert dev.last()["fam"] == 2  # the fp16 choice of an untuned launch: the two-stage LDS-DMA ring
        check_fp16("fp16 forward%s" % (" split" if split else ""), y[..., :cout], f["r"][0]["y"], f["u"][0]["y"], 1e-4, forward_regions(h, w))
    for i, (gs, m) in enumerate(GRAD_RUNS):  # (4096, 1e-6): a launch that drops the scale flushes dy to fp16 subnormals / zero
        hooks.udet_debug_conv_fp16_grad_scale(gs)
        dx, dxhat = dev.bwd(case, f["dy"][i], f["w"])
        assert dev.last()["fam"] == 2
        tag = "fp16 backward-data" + (" small gradient" if m < 1 else "")
        check_fp16(tag.replace("backward-data", "ringed gradient"), dxhat[..., :cin], f["r"][i]["gh"], f["u"][i]["gh"], 2e-4, ringed_regions(h, w), unit=m)
        check_fp16(tag, dx[..., :cin], f["r"][i]["gx"], f["u"][i]["gx"], 2e-4, {"whole dx": torch.ones(h, w, dtype=torch.bool)}, unit=m)


# ---- bad arguments ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_codes_and_launch_nothing(dev):
    """on real buffers: the documented codes (ValueError through _ffi.check's mapping is what ops raise; here the codes themselves), and the
    canary-filled outputs untouched.  tests/test_upconv_tables.py checks the same refusals without a device."""
    SHAPE, ALIGN = -1, -2
    r = reference(CASES[0])
    canary = -7777.25

    def untouched(*bufs):
        return all(torch.equal(b, torch.full_like(b, canary)) for b in bufs)
    for case, kw, code, msg in (((1, 4, 1, 12, 6, 12), {}, SHAPE, b"at least 2 x 2"), ((4, 1, 1, 12, 6, 12), {}, SHAPE, b"at least 2 x 2"),
                                ((4, 4, 1, 12, 6, 12), dict(ldy=10), ALIGN, b"multiples of 4"), ((4, 4, 1, 12, 6, 12), dict(ldy=12, y_coff=6), ALIGN, b"multiples of 4"),
                                ((4, 4, 1, 12, 6, 8), {}, SHAPE, b"outside the buffer"), ((4, 4, 1, 12, 6, 12), dict(ldy=8, y_coff=4), SHAPE, b"outside the buffer")):
        h, w, n, cin, cout, ldx = case
        st, y, xhat = dev.fwd(case, torch.zeros(n, h, w, ldx), r["w"], r["b"], canary=canary, status=True, **kw)
        assert st == code and msg in dev.lib.udet_last_error() and untouched(y, xhat), (case, kw, st)
        with pytest.raises(ValueError):
            dev.check(st)
        st, dx, dxhat = dev.bwd(case, torch.zeros(n, 2 * h, 2 * w, cout), r["w"], canary=canary, status=True,
                                **({"ldy": 12, "y_coff": 8} if kw.get("y_coff") == 4 else kw))
        assert st == code and untouched(dx, dxhat), (case, kw, st)
