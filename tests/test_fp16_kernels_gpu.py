"""Every fp16-capable forward / backward-data convolution configuration against a ROUNDED-OPERAND reference.

The product of two fp16 numbers is exact in fp32 and the kernels accumulate in fp32, so an fp16 kernel computes -- up to the fp32
summation order -- the exact convolution of the fp16-rounded operands.  The reference of every test here is therefore the float64
oracle (oracle_torch on the CPU) applied to operands rounded as the kernel rounds them,
    activations / weights:              t.half().double()                 (round to nearest even)
    gradient operand under scale s:     (t * s).half().double() / s
with bias, activation and epilogue unrounded, and the bound is the project's FP32 rule of the same operator:
    forward        1e-4 * max(unit, max|ref|)
    backward-data  2e-4 * max(unit, max|ref|)
`unit` is the magnitude of the launch's x operand: 1 everywhere except the small-gradient runs (dy = 1e-6 * U[0.25, 1] under scale 4096),
where it is 1e-6 -- the operation is linear in dy, so that is the same rule on the problem multiplied by 1e6, and it is what makes a kernel
that drops the scale (fp16 subnormals / zeros) fail; with a unit of 1 every such result would pass whatever it held.

Operands are drawn as U[0.25, 1] * scale with a random sign (r16 asserts that every rounded operand is a normal, non-zero fp16 number), so
the reference does not depend on how the hardware treats fp16 subnormals.  Every test asserts through udet_debug_last_conv which
configuration ran, and that fp16 arithmetic really ran: the error against the UNROUNDED oracle is at least 10x the error against the
rounded one (for the launches that the dispatch rules keep in fp32: the reverse).  tests/test_fp16_operands.py runs the operand checks
of every case on the CPU."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_torch as O  # noqa: E402
from test_ops_gpu import (CONV_CASES, FAMILIES, GEMM_TILES, THIN_CASES, TILE_CASE, TILE_FAMILIES, WINO_CASES, WS_OF, _oracle_conv,  # noqa: E402
                          _tile_fits)

GRAD_RUNS = ((1.0, 1.0), (4096.0, 1e-6))  # (gradient scale, magnitude of dy): an unscaled conversion of the second flushes / is subnormal
WORST = {"forward": 0.0, "backward-data": 0.0}  # worst error against the rounded reference, relative to max(unit, max|ref|)


def mag(*shape, seed, scale=1.0):
    """U[0.25, 1] * scale with a random sign (float32): nothing near zero"""
    g = torch.Generator().manual_seed(seed)
    u = 0.25 + 0.75 * torch.rand(*shape, generator=g)
    return u * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * scale


def r16(t, s=1.0):
    """the float32 operand t as an fp16 kernel multiplies it under scale s (a power of two), as float64; every value a normal fp16 number"""
    hv = (t * s).half()
    assert (hv != 0).all() and float(hv.abs().min()) >= 2.0 ** -14 and torch.isfinite(hv).all(), "zero / subnormal / infinite fp16 operand"
    return hv.double() / s


def layer(n, h, w, cin, cout, k, s, d=1, act="leaky", alpha=0.1, up=False):
    return (n, h, w, cin, cout, k, s, d, act, alpha, up)


def out_hw(c):
    n, h, w, cin, cout, k, s, d, act, alpha, up = c
    us = 2 if up else 1
    return -(-h * us // s), -(-w * us // s)


@functools.lru_cache(maxsize=4)
def operands(c, seed=0):
    """float32 operands of layer c and what an fp16 kernel makes of them; no convolution here (the CPU self-check runs this for every case)"""
    n, h, w, cin, cout, k, s, d, act, alpha, up = c
    oh, ow = out_hw(c)
    x = mag(n, h, w, cin, seed=seed + 1)
    wt = mag(k, k, cin, cout, seed=seed + 2, scale=(2.0 / (k * k * cin)) ** 0.5)
    b = mag(cout, seed=seed + 3, scale=0.1)
    dys = [mag(n, oh, ow, cout, seed=seed + 4 + i, scale=m) for i, (_, m) in enumerate(GRAD_RUNS)]
    return dict(x=x, w=wt, b=b, dy=dys, x16=r16(x), w16=r16(wt), dy16=[r16(dy, gs) for dy, (gs, _) in zip(dys, GRAD_RUNS)])


@functools.lru_cache(maxsize=4)
def reference(c, seed=0):
    """float64 results of layer c, computed once: forward (act, bias) and backward-data of the LINEAR layer for both gradient runs, each
    on the rounded (`*_r`) and on the unrounded (`*_u`) operands"""
    n, h, w, cin, cout, k, s, d, act, alpha, up = c
    op = operands(c, seed)
    r = dict(op)
    bd = op["b"].double()
    r["y_r"] = _oracle_conv(op["x16"], op["w16"], bd, s, d, act, alpha, up)
    r["y_u"] = _oracle_conv(op["x"].double(), op["w"].double(), bd, s, d, act, alpha, up)
    r["lin"] = _oracle_conv(op["x"].double(), op["w"].double(), None, s, d, "none", 0.0, up).float()
    if not up:
        xv = op["x"].double().requires_grad_(True)
        for tag, wt, dys in (("r", op["w16"], op["dy16"]), ("u", op["w"].double(), [t.double() for t in op["dy"]])):
            lin = O.conv2d_same(xv, wt, None, s, d)
            r["gx_" + tag] = [torch.autograd.grad((lin * dy).sum(), [xv], retain_graph=True)[0] for dy in dys]
    return r


def errors(got, ref_r, ref_u, unit=1.0):
    """(error against the rounded reference, against the unrounded one, the tensor's scale)"""
    g = got.double()
    return float((g - ref_r).abs().max()), float((g - ref_u).abs().max()), max(unit, float(ref_r.abs().max()))


def check(group, got, ref_r, ref_u, coeff, unit=1.0, fp16=True):
    e_r, e_u, scale = errors(got, ref_r, ref_u, unit)
    print("%s: %.2e of the scale against the rounded operands, %.2e against the unrounded ones" % (group, e_r / scale, e_u / scale))
    assert torch.isfinite(got).all()
    if fp16:
        WORST[group] = max(WORST[group], e_r / scale)
        assert e_r < coeff * scale, (group, "against the rounded-operand reference", e_r, scale)
        assert e_u > 0 and e_u >= 10 * e_r, (group, "fp16 arithmetic did not run", e_r, e_u)
    else:  # the launch stays fp32: the fp32 rule against the unrounded oracle, and visibly not the rounded operands' result
        assert e_u < coeff * scale, (group, "against the unrounded reference", e_u, scale)
        assert e_r > 0 and e_r >= 10 * e_u, (group, "the launch should have stayed fp32", e_r, e_u)


def word(lib):
    v = lib.udet_debug_last_conv()
    return dict(fam=v & 0xff, bm=(v >> 8) & 0xfff, ks=(v >> 20) & 0xff, fold=(v >> 28) & 1, tail=(v >> 29) & 1)


def split_capacity(taps, kreal):
    """max_ksplit (conv_select.hip) of a launch whose largest tap class has `taps` taps over kreal channels (the slabs of these shapes fit)"""
    kc = (kreal + 7) // 8 * 8
    return max(1, min(64, (taps * kc + 31) // 32 // 2))


@pytest.fixture(scope="module", autouse=True)
def worst_line():
    yield
    print()
    for group, bound in (("forward", "1e-4"), ("backward-data", "2e-4")):
        print("fp16 %s against the rounded-operand reference, worst error relative to the tensor's scale: %.2e (bound %s)"
              % (group, WORST[group], bound))


@pytest.fixture
def fp16():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import ops
    from unsupervised_detection_amd._devel import dbg as lib  # libudet_debug.so: the test-only hooks
    lib.udet_debug_conv_fp16(1)
    try:
        yield ops, lib
    finally:
        lib.udet_debug_force_conv(0, 0, -1)
        lib.udet_debug_conv_fp16_grad_scale(0.0)
        lib.udet_debug_conv_fp16(0)


def run_forward(ops, lib, c, r, expect=None):
    n, h, w, cin, cout, k, s, d, act, alpha, up = c
    got = ops.conv2d(r["x"].cuda(), r["w"].cuda(), r["b"].cuda(), s, d, act, alpha, up).cpu()
    last = word(lib)
    if expect:
        assert {f: last[f] for f in expect} == expect, ("forward", last)
    check("forward", got, r["y_r"], r["y_u"], 1e-4)
    return last


def run_backward(ops, lib, c, r, expect=None):
    """backward-data of the linear layer (no act' on load: the form the step uses), once per gradient run"""
    n, h, w, cin, cout, k, s, d, act, alpha, up = c
    last = None
    for i, (gs, m) in enumerate(GRAD_RUNS):
        lib.udet_debug_conv_fp16_grad_scale(gs)
        dx = ops.conv2d_backward_data(r["dy"][i].cuda(), r["lin"].cuda(), r["w"].cuda(), (h, w), s, d, "none", 0.0).cpu()
        last = word(lib)
        if expect:
            assert {f: last[f] for f in expect} == expect, ("backward-data", last)
        check("backward-data", dx, r["gx_r"][i], r["gx_u"][i], 2e-4, unit=m)
    lib.udet_debug_conv_fp16_grad_scale(0.0)
    return last


# ---- every fp16-capable tile of every LDS-DMA family ---------------------------------------------------------------------------------
F16_TILE_CONFIGS = ([(f, bm, bn) for f in ("ring2", "ring3", "ring4") for bm, bn in GEMM_TILES]
                    + [("self_staging", bm, bn) for bm, bn in GEMM_TILES if bn != 96])
TILE_LAYER = layer(*TILE_CASE)


@pytest.mark.parametrize("family,bm,bn", F16_TILE_CONFIGS)
def test_fp16_every_tile_of_every_family(fp16, family, bm, bn):
    """test_conv_every_tile_of_every_family in fp16: TILE_CASE forced on one (family, tile); family and bm asserted from the hook, a wrong N
    tile shows in the result (partial N tiles for every bn)."""
    ops, lib = fp16
    bit, fam = (1 << 19, 6) if family == "self_staging" else TILE_FAMILIES[family]
    r = reference(TILE_LAYER)
    lib.udet_debug_force_conv(bm + bit, bn, 1)
    run_forward(ops, lib, TILE_LAYER, r, dict(fam=fam, bm=bm, ks=1))
    run_backward(ops, lib, TILE_LAYER, r, dict(fam=fam, bm=bm, ks=1))


def test_fp16_tile_configs_are_the_23_instantiations():
    assert len(F16_TILE_CONFIGS) == 23 and len(set(F16_TILE_CONFIGS)) == 23


# ---- every fp16-capable entry of FAMILIES on every THIN_CASES shape -----------------------------------------------------------------
F16_FAMILIES = [f for f in FAMILIES if WS_OF[f] in (2, 3, 4, 5, 6)]


def test_fp16_family_list():
    assert F16_FAMILIES == ["lds_dma", "lds_dma_split3", "tile8", "tile4", "self_staging", "self_staging_128", "self_staging_split2",
                            "self_staging_n32", "self_staging_256x32", "lds_dma_split3_2pass", "lds_dma_split5_fold_64",
                            "self_staging_split2_2pass", "lds_dma_ring3", "lds_dma_ring4_64_split2"]


@pytest.mark.parametrize("family", F16_FAMILIES)
@pytest.mark.parametrize("case", THIN_CASES)
def test_fp16_kernel_families(fp16, family, case):
    """test_conv_kernel_families in fp16.  Forward: the family, and for the implicit-GEMM entries the tile rows and the split count (the
    forced one inside the launch's capacity) with its summation mode; backward-data: the family (its tap classes decide the capacity)."""
    ops, lib = fp16
    n, h, w, cin, cout, k, s = case
    c = layer(*case)
    r = reference(c)
    bmw, bn, ks = FAMILIES[family]
    lib.udet_debug_force_conv(bmw, bn, ks)
    fam = WS_OF[family]
    if fam == 3:
        th = 8 if family == "tile8" else 4
        fits = _tile_fits(th, cin, cout, k, s)
        last = run_forward(ops, lib, c, r, dict(fam=3, bm=th) if fits else None)
        assert fits or last["fam"] == 2  # (not eligible: the built-in fp16 choice)
        fits = cin <= 256 and cout <= 256 and _tile_fits(th, cout, cin, k, 1)
        last = run_backward(ops, lib, c, r, dict(fam=3, bm=th) if fits else None)
        assert last["fam"] in (2, 3)
        return
    want = min(ks, split_capacity(k * k, cin))
    fold = 1 if "_fold" in family and want > 1 else 0
    last = run_forward(ops, lib, c, r, dict(fam=fam, bm=bmw & 0xfff, ks=want, fold=fold, tail=0))
    if ks > 1:
        assert last["ks"] > 1  # (every THIN_CASES shape is deep enough for two slices)
    last = run_backward(ops, lib, c, r, dict(fam=fam, bm=bmw & 0xfff, tail=0))
    if s == 1:
        want = min(ks, split_capacity(k * k, cout))
        assert last["ks"] == want and last["fold"] == (1 if "_fold" in family and want > 1 else 0), last


# ---- the tile-resident kernel: all eight F16 instantiations -----------------------------------------------------------------------------
def tile_instantiation(th, cin, cout, k, s):
    """(MFMA tile width, big staging) of the tile-resident kernel's forward launch -- conv_tile_lds_bytes / launch_conv_tile restated;
    None where the launch is not eligible (register staging capacity or LDS)"""
    cqb = min((cin + 7) // 8 * 8, 32) // 4
    nw = 16 if cout <= 16 else 32
    pix = ((th - 1) * s + k) * (31 * s + k)
    if pix * cqb > 256 * 16 or k * k * cqb * (nw // 4) > 256 * 3 or not _tile_fits(th, cin, cout, k, s):
        return None
    return nw, pix * cqb > 256 * 8 or k * k * cqb * (nw // 4) > 256 * 2


TILE_RESIDENT = [
    # (n, h, w, cin, cout, k, s), tile height, the instantiation conv_tile_kernel<th, width, small / big staging, F16> its forward runs
    ((1, 32, 64, 16, 16, 3, 1), 8, (16, False)),
    ((1, 32, 64, 16, 16, 3, 1), 4, (16, False)),
    ((1, 32, 64, 104, 16, 4, 1), 8, (16, True)),    # 32 resident channels x an 11 x 35 halo: more than 8 float4 per thread
    ((1, 32, 64, 104, 16, 4, 1), 4, (16, False)),
    ((2, 16, 64, 32, 32, 3, 1), 8, (32, True)),
    ((2, 16, 64, 32, 32, 3, 1), 4, (32, True)),     # big through the weights: 9 taps x 8 channel quads x 8 float4 columns
    ((1, 30, 50, 16, 32, 3, 1), 8, (32, False)),    # ragged grid: 50 = 32 + 18 columns, 30 rows, partial tiles on both axes
    ((1, 30, 50, 16, 32, 3, 1), 4, (32, False)),
    ((1, 30, 50, 16, 16, 3, 1), 8, (16, False)),    # the ragged grid on the 16-wide (16x16x16 MFMA) path
    ((1, 32, 64, 16, 16, 3, 2), 4, (16, True)),     # stride 2: a 9 x 65 halo
    ((1, 32, 48, 4, 16, 7, 2), 8, (16, True)),      # 7x7 s2 over the 8-channel padded input
]


def test_fp16_tile_resident_cases_name_every_instantiation():
    for case, th, inst in TILE_RESIDENT:
        n, h, w, cin, cout, k, s = case
        assert tile_instantiation(th, cin, cout, k, s) == inst, (case, th)
    assert {(th, *inst) for _, th, inst in TILE_RESIDENT} == {(th, nw, big) for th in (4, 8) for nw in (16, 32) for big in (False, True)}


@pytest.mark.parametrize("case,th,inst", TILE_RESIDENT, ids=["%s-th%d" % ("x".join(map(str, t[0])), t[1]) for t in TILE_RESIDENT])
def test_fp16_tile_resident_kernel(fp16, case, th, inst):
    ops, lib = fp16
    n, h, w, cin, cout, k, s = case
    c = layer(*case)
    r = reference(c)
    lib.udet_debug_force_conv((1 << 18) + th, 0, 1)
    run_forward(ops, lib, c, r, dict(fam=3, bm=th))
    fits = _tile_fits(th, cout, cin, k, 1)  # (sufficient, as in test_conv_kernel_families; otherwise the built-in fp16 choice may run)
    last = run_backward(ops, lib, c, r, dict(fam=3, bm=th) if fits else None)
    assert last["fam"] in (2, 3)


# ---- tail split -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["lds_dma", "lds_dma_ring3"])
@pytest.mark.parametrize("stride", [1, 2])
def test_fp16_tail_split(fp16, family, stride):
    """test_conv_tail_split in fp16: 288 tiles of 64x64 = one whole round of 256 + 32 tiles cut into K slices"""
    ops, lib = fp16
    c = layer(2, 96 * stride, 96 * stride, 64, 64, 3, stride)
    r = reference(c)
    lib.udet_debug_force_conv(64 + ((1 << 17) if family == "lds_dma" else (1 << 22)), 64, 256)
    last = run_forward(ops, lib, c, r, dict(fam=WS_OF[family], bm=64, tail=1, fold=0))
    assert 2 <= last["ks"] <= 8, last  # up to 256 // 32 slices
    # (stride 2: four parity classes, the word is the last one's -- a 1-tap class cannot be split)
    run_backward(ops, lib, c, r, dict(fam=WS_OF[family], bm=64, tail=1) if stride == 1 else dict(fam=WS_OF[family], bm=64))


# ---- transposed 4x4 s2 forward ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def transposed_reference():
    x = mag(2, 12, 20, 64, seed=25)
    wt = mag(4, 4, 32, 64, seed=26, scale=(1.0 / (16 * 64)) ** 0.5)
    b = mag(32, seed=27, scale=0.1)
    return dict(x=x, w=wt, b=b, y_r=O.conv2d_transpose_k4s2_same(r16(x), r16(wt), b.double()),
                y_u=O.conv2d_transpose_k4s2_same(x.double(), wt.double(), b.double()))


@pytest.mark.parametrize("family", F16_FAMILIES)
def test_fp16_conv2d_transpose_kernel_families(fp16, family):
    """test_conv2d_transpose_kernel_families in fp16 (forward launches: scale 1 whatever the gradient-scale hook says)"""
    ops, lib = fp16
    r = transposed_reference()
    lib.udet_debug_force_conv(*FAMILIES[family])
    lib.udet_debug_conv_fp16_grad_scale(4096.0)
    y = ops.conv2d_transpose4x4s2(r["x"].cuda(), r["w"].cuda(), r["b"].cuda()).cpu()
    assert word(lib)["fam"] == WS_OF[family]
    check("forward", y, r["y_r"], r["y_u"], 1e-4)


# ---- CONV_CASES with nothing forced ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV_CASES)
def test_fp16_conv_cases_unforced(fp16, case):
    """dilation 4 / 16, 4x4 and 7x7 s2, fused NN x2, ragged Cin, Cout = 196, the two-channel heads: under the fp16 switch an untuned launch
    that dma_ok accepts is the two-stage LDS-DMA ring (heuristic_cfg; the direct two-channel kernels multiply in fp32 only and are skipped)."""
    ops, lib = fp16
    c = layer(*case)
    r = reference(c)
    run_forward(ops, lib, c, r, dict(fam=2, tail=0))
    if not c[10]:
        run_backward(ops, lib, c, r, dict(fam=2, tail=0))


# ---- configurations without an fp16 form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["plain", "wave_spec", "wave_spec_split4_2pass"])
def test_fp16_register_staged_entries_run_the_lds_dma_kernel(fp16, family):
    """runnable_cfg: a forced (or file-loaded) register-staged entry on an fp16 launch that dma_ok accepts multiplies in fp16 like every
    other configuration -- family 2 on the same tile and split."""
    ops, lib = fp16
    case = THIN_CASES[3]
    n, h, w, cin, cout, k, s = case
    c = layer(*case)
    r = reference(c)
    bmw, bn, ks = FAMILIES[family]
    lib.udet_debug_force_conv(bmw, bn, ks)
    run_forward(ops, lib, c, r, dict(fam=2, bm=128, ks=min(ks, split_capacity(k * k, cin)), fold=0, tail=0))
    run_backward(ops, lib, c, r, dict(fam=2, bm=128, ks=min(ks, split_capacity(k * k, cout)), fold=0, tail=0))


@pytest.mark.parametrize("forced,case", [((1 << 24, 0, 1), (1, 16, 64, 36, 2, 3, 1)),            # the direct two-channel kernels
                                         (((1 << 25) + 0, 0, 1), WINO_CASES[0]),             # Winograd variants
                                         (((1 << 25) + 2, 0, 2), WINO_CASES[0])])
def test_fp16_forced_fp32_only_families_fall_back_to_the_fp16_choice(fp16, forced, case):
    """a forced direct kernel or Winograd variant (fp32 only) falls back to the heuristic configuration, which multiplies in fp16"""
    ops, lib = fp16
    c = layer(*case[:5], 3, 1)
    r = reference(c)
    lib.udet_debug_force_conv(*forced)
    run_forward(ops, lib, c, r, dict(fam=2))
    run_backward(ops, lib, c, r, dict(fam=2))


def test_fp16_activation_derivative_on_load_stays_fp32(fp16):
    """backward-data with act' applied on load (xa != nullptr) is not dma_ok: the wave-specialised kernel runs, in fp32 -- the fp32 rule
    against the UNROUNDED oracle, and at least 10x further from the rounded operands' result."""
    ops, lib = fp16
    case = THIN_CASES[1]
    n, h, w, cin, cout, k, s = case
    c = layer(*case)
    op = operands(c)
    res = {}
    for tag, wt, dy in (("r", op["w16"], op["dy16"][0]), ("u", op["w"].double(), op["dy"][0].double())):
        xv = op["x"].double().requires_grad_(True)  # (x itself is no operand of backward-data; its activation pattern is the saved y's)
        y = _oracle_conv(xv, op["w"].double(), op["b"].double(), s, 1, "leaky", 0.1, False)
        lin = O.conv2d_same(xv, wt, None, s, 1)
        slope = torch.where(y.detach() > 0, 1.0, 0.1)
        res[tag] = torch.autograd.grad((lin * (dy * slope)).sum(), [xv])[0]
        ys = y.detach().float()
    dx = ops.conv2d_backward_data(op["dy"][0].cuda(), ys.cuda(), op["w"].cuda(), (h, w), s, 1, "leaky", 0.1).cpu()
    assert word(lib)["fam"] == 1
    check("backward-data", dx, res["r"], res["u"], 2e-4, fp16=False)


# every layer the tests above draw operands for (tests/test_fp16_operands.py checks them on the CPU)
ALL_LAYERS = sorted({TILE_LAYER} | {layer(*c) for c in THIN_CASES} | {layer(*t[0]) for t in TILE_RESIDENT} | {layer(*c) for c in CONV_CASES}
                    | {layer(2, 96 * s, 96 * s, 64, 64, 3, s) for s in (1, 2)} | {layer(1, 16, 64, 36, 2, 3, 1), layer(*WINO_CASES[0][:5], 3, 1)},
                    key=str)
