"""The filter gradient (csrc/conv_wgrad.hip, launch_wgrad_T) forced through every direct staging variant, split count, slab-reduction
instantiation, BN form and operand view, as the step plan calls it (channel windows included), through
udet_debug_conv2d_backward_filter_ex.  Reference everywhere: float64 PyTorch autograd on the CPU of
    y = gamma*c*(conv(x^, w) + b) + beta,   L = sum(act(y) * dy)
with the oracle's conv2d_same / resize_nearest_align_corners, computed once per case.  Every configuration asserts
  (i)   the two report words (udet_debug_last_wgrad / udet_debug_last_wgrad_reduce) against a host-side restatement of the dispatch rules,
  (ii)  every output within 2e-4 * max(1, max|ref|) of the reference (the project's filter-gradient rule; dgamma / dbeta too),
  (iii) every output within 1e-4 * max(1, max|ref|) of the heuristic configuration's result on the same data,
  (iv)  bit-identical outputs of two runs (fixed summation orders),
and that nothing was written outside the outputs (NaN guards on both sides).

The fp16 mode of the same machinery (`f16` = the gradient scale; section g): fp16 hook on, udet_debug_conv_fp16_grad_scale set, operands drawn
as U[0.25, 1] * scale with a random sign, and (ii) made against the float64 result of the operands ROUNDED as the kernel rounds them (see
tests/test_fp16_kernels_gpu.py) at the same 2e-4.  In every form -- plain, operand-swapped, fused NN x2, BN-folded (fused or separate
finalisation) and class-structured -- the GEMM of conv_wgrad_dma_kernel multiplies x and dy AS PASSED (gamma * c is applied to the fp32 sums by
the reduction / finalisation, the class-structured form's dy is the caller's dU, read on its parity sub-lattices), so exactly x and dy are
rounded, dy under the scale, whichever GEMM side it sits on.  db and dbeta are fp32 column sums of the unrounded dy; dgamma is formed from the
GEMM's dW (the dot with w), so it follows the rounded operands.  The unit of the bounds is the magnitude of dy (1, or 1e-6 under scale 4096:
the operation is linear in dy), not 1."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_torch as O  # noqa: E402
from test_fp16_kernels_gpu import mag, r16  # noqa: E402

BN_C = float(O.BN_SCALE)
ACT = {"none": 0, "leaky": 1, "elu": 2}
FUSED_BN, SEPARATE_BN, SWAPPED, CLASSES = 1 << 26, 1 << 27, 1 << 28, 1 << 29
GUARD = 64
ALL = 1 << 19  # "as many splits as fit"


@pytest.fixture(scope="module")
def dbg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd._devel import dbg as _dbg
    try:
        yield _dbg
    finally:
        _dbg.udet_debug_force_wgrad(0, -1)
        _dbg.udet_debug_conv_fp16_grad_scale(0.0)
        _dbg.udet_debug_conv_fp16(0)


def case(n, h, w, cin, cout, k, s=1, d=1, act="none", alpha=0.0, bn=False):
    """(h, w): the stored grid of x (the low-resolution grid of an up-sampling layer)"""
    return (n, h, w, cin, cout, k, s, d, act, alpha, bn)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r4(v):
    return (v + 3) // 4 * 4


# ---- reference (once per case) ----------------------------------------------------------------------------------------------------
def dy_unit(f16):
    """magnitude of dy in fp16 mode: order 1 at scale 1, 1e-6 (subnormal / flushed by an unscaled fp16 conversion) under a real scale"""
    return 1.0 if f16 in (0.0, 1.0) else 1e-6


@functools.lru_cache(maxsize=None)
def reference(c, up, f16=0.0):
    """f16 = 0: the fp32 mode.  f16 > 0 (the gradient scale): `ref` is what the launch must produce -- from the rounded x / dy where the
    dispatch rules run the fp16 kernel (no act' on load), from the unrounded ones where they keep fp32 -- and ins["alt_dw"] the other dW"""
    n, h, w, cin, cout, k, s, d, act, alpha, bn = c
    x = (mag(n, h, w, cin, seed=101) if f16 else rnd(n, h, w, cin, seed=101)).double()
    wt = rnd(k, k, cin, cout, seed=102, scale=(2.0 / (k * k * cin)) ** 0.5).double().requires_grad_(True)
    b = rnd(cout, seed=103, scale=0.1).double().requires_grad_(True)
    gamma = (1.0 + 0.3 * rnd(cout, seed=104)).double().requires_grad_(True)
    beta = rnd(cout, seed=105, scale=0.1).double().requires_grad_(True)
    leaves = [wt, b, gamma, beta] if bn else [wt, b]

    def forward(xs):
        xu = O.resize_nearest_align_corners(xs, 2 * h, 2 * w) if up else xs
        y = O.conv2d_same(xu, wt, b, s, d)
        if bn:
            y = gamma * BN_C * y + beta
        return O.leaky_relu(y, alpha) if act == "leaky" else (torch.nn.functional.elu(y) if act == "elu" else y)

    def grads(xs, dys):
        g = [t.float() for t in torch.autograd.grad((forward(xs) * dys).sum(), leaves)]
        r = dict(zip(("dw", "db", "dgamma", "dbeta"), g))
        r["dw"] = r["dw"].reshape(-1)
        return r

    a = forward(x).detach()
    dy = (mag(*a.shape, seed=106, scale=dy_unit(f16)) if f16 else rnd(*a.shape, seed=106)).double()
    ref = grads(x, dy)
    ins = dict(x=x.float(), dy=dy.float(), ya=a.float() if act != "none" else None, w=wt.detach().float(), b=b.detach().float(),
               gamma=gamma.detach().float())
    if f16:
        rounded = grads(r16(x.float()), r16(dy.float(), f16))
        ins["dgamma_u"] = ref.get("dgamma")
        if act == "none":  # the fp16 kernel runs
            ins["alt_dw"] = ref["dw"]
            ref["dw"] = rounded["dw"]
            if bn:
                ref["dgamma"] = rounded["dgamma"]
        else:
            ins["alt_dw"] = rounded["dw"]
    return ins, ref


# ---- the dispatch rules of launch_wgrad_T, restated ------------------------------------------------------------------------------------
def dispatch(c, mode):
    """geometry of the GEMM view and of the workspace for `c` in up mode `mode` (0 none, 1 fused NN x2, 2 class-structured)"""
    n, h, w, cin, cout, k, s, d, act, alpha, bn = c
    if mode == 2:  # the low-resolution GEMM: 16 effective taps, dU on its four parity sub-lattices
        H, W, OH, OW, T, ntaps, centre = h, w, h, w, 16, 16, True
    else:
        us = 1 if mode else 0
        H, W = h << us, w << us
        OH, OW = -(-H // s), -(-W // s)
        pt = max(0, (OH - 1) * s + (k - 1) * d + 1 - H) // 2
        pl = max(0, (OW - 1) * s + (k - 1) * d + 1 - W) // 2
        taps = [(ky * d - pt, kx * d - pl) for ky in range(k) for kx in range(k)]
        taps = [(ty, tx) for ty, tx in taps if not (ty >= H or (OH - 1) * s + ty < 0 or tx >= W or (OW - 1) * s + tx < 0)]
        T, ntaps, centre = k * k, len(taps), (0, 0) in taps
    co4, ci4 = r4(cout), r4(cin)

    def tile_cost(rows, cols):
        bn_ = 128 if cols > 64 else (64 if cols > 32 else 32)
        return -(-rows // 128) * 128 * (-(-cols // bn_) * bn_)
    cheaper = tile_cost(ntaps * co4, cin) < tile_cost(ntaps * ci4, cout)
    narrow = cin >= 16 if cout <= 4 else (cout <= 16 and 128 % co4 == 0 and cheaper)
    swap = narrow and s == 1 and mode == 0 and H == OH and W == OW and act == "none" and centre
    g_cin, g_cout = (cout, cin) if swap else (cin, cout)
    tile_n = 128 if g_cout > 64 else (64 if g_cout > 32 else 32)
    mreal = ntaps * r4(g_cin)
    m_tiles, co_tiles = max(1, -(-mreal // 128)), -(-g_cout // tile_n)
    ldn = co_tiles * tile_n
    nchunks = -(-(n * OH * OW) // 32)
    fused = bn and mode != 2 and not swap and ntaps == T and cout <= 128
    return dict(T=T if mode != 2 else 9, ntaps=ntaps, swap=swap, mreal=mreal, total=(mreal + 1) * g_cout, g_cout=g_cout,
                cap=max(1, nchunks // 2), fixed=(1024 * cout + 15) // 16 * 16, per_split=(4 if mode == 2 else 1) * ldn + m_tiles * 128 * ldn,
                reserve=16 * cin * cout + 64 * cout + 1024 if mode == 2 else 0, fused=fused, separate=bn and not fused,
                classes=mode == 2, dma_ok=act == "none", tile_n=tile_n)


def reduce_word(g, ns, cout):
    """what udet_debug_last_wgrad_reduce must say for `ns` slabs"""
    if g["fused"]:
        cw = 128 if cout > 64 else (64 if cout > 32 else (32 if cout > 16 else 16))
        rg = 256 // cw
        sl = min(rg, 8 if ns >= 64 else (4 if ns >= 32 else (2 if ns >= 12 else 1)))
        while sl > 1 and -(-g["mreal"] // rg) * sl > 512:
            sl //= 2
        rb = rg // sl
        while -(-g["mreal"] // rb) > 1024:
            rb *= 2
        return sl | cw << 8 | rb << 16 | FUSED_BN
    total = g["total"]
    sl = 64 if ns >= 64 and total * 64 <= 262144 else (8 if ns >= 8 and total * 8 <= 262144 else 1)
    return sl | (SWAPPED if g["swap"] else 0) | (CLASSES if g["classes"] else 0) | (SEPARATE_BN if g["separate"] else 0)


def trips(nsum, sl):
    """(some lane runs the 8-deep unrolled trip, some lane runs the remainder loop) of a slab reduction over nsum partials"""
    unrolled = remainder = False
    for lane in range(sl):
        k = lane
        while k + 7 * sl < nsum:
            unrolled, k = True, k + 8 * sl
        remainder |= k < nsum
    return unrolled, remainder


# ---- one launch ------------------------------------------------------------------------------------------------------------------------
_ws = {}
_dev = {}


def workspace(floats):
    if "t" not in _ws or _ws["t"].numel() < floats:
        _ws["t"] = torch.empty(floats + (1 << 20), dtype=torch.float32, device="cuda")
    return _ws["t"]


def place(t, ld, coff, seed):
    """t's channels inside a [..., ld] buffer at coff; tight (zero padding up to a multiple of 4, as the public entry does) when ld is None"""
    c = t.shape[-1]
    if ld is None:
        buf = torch.zeros(*t.shape[:-1], r4(c))
        coff = 0
    else:
        buf = rnd(*t.shape[:-1], ld, seed=seed, scale=1e3)  # neighbouring channels hold other tensors
    buf[..., coff:coff + c] = t
    return buf.cuda(), buf.shape[-1], coff


def operands(c, up, win, f16=0.0):
    key = (c, up, win, f16)
    if key not in _dev:
        ins, _ = reference(c, up, f16)
        ldx, xo, ldy, yo = win if win else (None, 0, None, 0)
        x, ldx, xo = place(ins["x"], ldx, xo, 201)
        dy, ldy, yo = place(ins["dy"], ldy, yo, 202)
        ya = place(ins["ya"], ldy if win else None, yo, 203)[0] if ins["ya"] is not None else None
        _dev.clear()  # (one case's operands at a time)
        _dev[key] = dict(x=x, ldx=ldx, xo=xo, dy=dy, ldy=ldy, yo=yo, ya=ya, w=ins["w"].cuda(), b=ins["b"].cuda(), gamma=ins["gamma"].cuda())
    return _dev[key]


def launch(dbg, c, mode, win=None, f16=0.0):
    """one call of the hook; outputs as CPU tensors with their NaN guards still attached"""
    n, h, w, cin, cout, k, s, d, act, alpha, bn = c
    g = dispatch(c, mode)
    op = operands(c, mode != 0, win, f16)
    floats = 64 + g["fixed"] + g["per_split"] * g["cap"] + g["reserve"]  # every split count up to the cap fits
    ws = workspace(floats)
    sizes = dict(dw=g["T"] * cin * cout, db=cout, dgamma=cout, dbeta=cout)
    names = ("dw", "db", "dgamma", "dbeta") if bn else ("dw", "db")
    out = {nm: torch.full((sizes[nm] + 2 * GUARD,), float("nan"), device="cuda") for nm in names}
    ptr = lambda nm: out[nm].data_ptr() + 4 * GUARD if nm in out else None
    rc = dbg.udet_debug_conv2d_backward_filter_ex(
        op["x"].data_ptr(), op["ldx"], op["xo"], op["dy"].data_ptr(), op["ldy"], op["yo"], op["ya"].data_ptr() if op["ya"] is not None else None,
        ACT[act], alpha, op["w"].data_ptr() if bn else None, op["b"].data_ptr() if bn else None, op["gamma"].data_ptr() if bn else None, BN_C,
        ptr("dw"), ptr("db"), ptr("dgamma"), ptr("dbeta"), n, h, w, cin, cout, k, s, d, mode, ws.data_ptr(), 4 * floats,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        from unsupervised_detection_amd._ffi import lib
        raise AssertionError(f"rc {rc}: {lib.udet_last_error().decode()}")
    words = dbg.udet_debug_last_wgrad(), dbg.udet_debug_last_wgrad_reduce()
    return {nm: t.cpu() for nm, t in out.items()}, words


def inner(t):
    return t[GUARD:-GUARD]


WORST_F16 = {"dw": 0.0}  # fp16 mode: worst dW error against the rounded-operand reference, relative to the tensor's scale


def sweep(dbg, c, mode, variants, splits, win=None, f16=0.0):
    """assertions (i)-(iv) and the guards for every (variant, split count); returns {(variant, asked): (outputs, reduce word)}.
    f16 > 0: the same in fp16 mode under that gradient scale (see the module docstring)"""
    cout = c[4]
    g = dispatch(c, mode)
    ins, ref = reference(c, mode != 0, f16)
    unit = dy_unit(f16)
    scale = {nm: max(unit, float(r.abs().max())) for nm, r in ref.items()}
    dbg.udet_debug_force_wgrad(0, -1)
    results = {}
    try:
        dbg.udet_debug_conv_fp16(1 if f16 else 0)
        dbg.udet_debug_conv_fp16_grad_scale(f16)
        heur, (hcfg, _) = launch(dbg, c, mode, win, f16)
        if f16:  # the built-in choice of an fp16 launch is the LDS-DMA kernel wherever it can run
            assert hcfg >> 20 == (1 if g["dma_ok"] else 0), hex(hcfg)
        for v in variants:
            for asked in splits:
                tag = f"variant {v}, {asked} splits" + (f", fp16 scale {f16:g}" if f16 else "")
                dbg.udet_debug_force_wgrad(asked, v)
                out, (cfg, red) = launch(dbg, c, mode, win, f16)
                again, words2 = launch(dbg, c, mode, win, f16)
                ns = min(asked, g["cap"])
                want_v = v if g["dma_ok"] else 0  # act' on load lives in the register-staged kernel only
                if f16 and g["dma_ok"]:
                    want_v = 1  # the one fp16 kernel: variants 0 / 3 multiply in fp32 only, variant 2 has no fp16 instantiation
                elif f16 and v == 3:
                    want_v = 0
                assert cfg == ns | want_v << 20, (tag, hex(cfg))                                                   # (i)
                assert red == reduce_word(g, ns, cout), (tag, hex(red), hex(reduce_word(g, ns, cout)))
                assert words2 == (cfg, red)
                for nm, r in ref.items():
                    o = out[nm]
                    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[-GUARD:]).all(), (tag, nm, "guard overwritten")
                    assert torch.isfinite(inner(o)).all(), (tag, nm)
                    err, dh = float((inner(o) - r).abs().max()), float((inner(o) - inner(heur[nm])).abs().max())
                    if f16:
                        print("%s %s: %.2e of the scale against the reference" % (tag, nm, err / scale[nm]))
                    assert err < 2e-4 * scale[nm], (tag, nm, "against the reference", err, scale[nm])  # (ii)
                    assert dh < 1e-4 * scale[nm], (tag, nm, "against the heuristic configuration", dh, scale[nm])  # (iii)
                    assert torch.equal(inner(o), inner(again[nm])), (tag, nm, "two runs differ")               # (iv)
                if f16:
                    # fp16 arithmetic ran (the unrounded operands' dW is at least 10x further away than the rounded operands'), or -- a
                    # launch the rules keep in fp32 -- provably did not; dgamma also within the fp32-mode bound of the unrounded value
                    e_ref = float((inner(out["dw"]) - ref["dw"]).abs().max())
                    e_alt = float((inner(out["dw"]) - ins["alt_dw"]).abs().max())
                    assert e_alt > 0 and e_alt >= 10 * e_ref, (tag, "fp16 arithmetic ran" if g["dma_ok"] else "stayed fp32", e_ref, e_alt)
                    if g["dma_ok"]:
                        WORST_F16["dw"] = max(WORST_F16["dw"], e_ref / scale["dw"])
                    if "dgamma" in ref:
                        du = ins["dgamma_u"]
                        assert float((inner(out["dgamma"]) - du).abs().max()) < 2e-4 * max(1.0, float(du.abs().max())), (tag, "dgamma")
                results[(v, asked)] = (out, red)
    finally:
        dbg.udet_debug_force_wgrad(0, -1)
        dbg.udet_debug_conv_fp16_grad_scale(0.0)
        dbg.udet_debug_conv_fp16(0)
    for nm, r in ref.items():  # the heuristic configuration itself
        assert float((inner(heur[nm]) - r).abs().max()) < 2e-4 * scale[nm], ("heuristic", nm)
    return results


# ---- a) direct variants x split counts, plain layers ------------------------------------------------------------------------------------
PLAIN = {
    "odd_grid_bn128": (case(2, 13, 21, 64, 128, 3), 0),          # Q = 546: not a multiple of 32
    "bn64": (case(1, 16, 32, 32, 48, 3), 0),
    "7x7_s2": (case(1, 32, 48, 4, 16, 7, s=2), 0),               # 32 taps per M tile
    "5x5_s2": (case(1, 32, 48, 16, 32, 5, s=2), 0),
    "culled_d16": (case(2, 12, 24, 128, 128, 3, d=16), 0),
    "swapped_cout2": (case(1, 24, 40, 565, 2, 3), 0),
    "swapped_cout16": (case(1, 24, 48, 104, 16, 4), 0),
    "cin5": (case(1, 24, 48, 5, 32, 5), 0),
    "nn_x2": (case(1, 12, 24, 128, 64, 3), 1),
    "leaky": (case(1, 16, 32, 32, 48, 3, act="leaky", alpha=0.1), 0),
    "elu": (case(1, 13, 21, 16, 32, 3, act="elu"), 0),
}


@pytest.mark.parametrize("name", list(PLAIN))
def test_direct_variants_and_split_counts(dbg, name):
    c, mode = PLAIN[name]
    g = dispatch(c, mode)
    assert g["swap"] == name.startswith("swapped") and not g["fused"] and not g["separate"]
    res = sweep(dbg, c, mode, (0, 1, 2), (1, 2, 3, 7, ALL))
    for (v, asked), (out, red) in res.items():
        assert bool(red & SWAPPED) == name.startswith("swapped") and (red >> 8) & 0xff == 0 and not red & (FUSED_BN | SEPARATE_BN | CLASSES)
    if name == "culled_d16":  # rows 0 and 2 of the 3x3 filter never meet the image: exactly zero
        assert g["ntaps"] == 3
        for out, _ in res.values():
            dw = inner(out["dw"]).reshape(3, 3, 128, 128)
            assert (dw[0] == 0).all() and (dw[2] == 0).all() and dw[1].abs().min() > 0


# ---- b) plain reduction lanes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,splits,sl,both", [
    (case(1, 64, 64, 8, 24, 3), (8, 11, 63), 8, False),
    (case(1, 64, 64, 8, 24, 3), (64,), 64, False),
    (case(2, 128, 128, 8, 24, 3), (500,), 64, True),
    (case(2, 24, 40, 64, 128, 3), (11, 15), 1, True),
])
def test_plain_reduction_lanes(dbg, c, splits, sl, both):
    assert max(splits) <= dispatch(c, 0)["cap"]
    if both:
        assert all(trips(ns, sl) == (True, True) for ns in splits)
    for (v, asked), (_, red) in sweep(dbg, c, 0, (1,), splits).items():
        assert red == sl, (asked, hex(red))  # wgrad_reduce_kernel<sl>, no BN, plain view


# ---- c) fused BN reduction: all 13 instantiations --------------------------------------------------------------------------------------
FUSED = [
    # case, {splits: (CW, SL)}, rows per block
    (case(1, 32, 64, 32, 128, 3, bn=True), {1: (128, 1), 11: (128, 1), 12: (128, 2), 32: (128, 2)}, None),
    (case(1, 32, 64, 32, 48, 3, bn=True), {3: (64, 1), 12: (64, 2), 32: (64, 4)}, None),
    (case(1, 64, 64, 8, 24, 3, bn=True), {5: (32, 1), 12: (32, 2), 32: (32, 4), 64: (32, 8)}, None),
    (case(1, 64, 64, 8, 16, 3, bn=True), {5: (16, 1), 12: (16, 2), 32: (16, 4), 64: (16, 8)}, None),  # (not swapped: that view pads more)
    (case(1, 64, 64, 8, 12, 3, bn=True), {40: (16, 4)}, None),                                         # ragged Cout
    (case(1, 16, 32, 96, 128, 5, bn=True), {3: (128, 1)}, 4),          # 2400 rows: 1200 blocks of 2 rows -> 600 of 4
    (case(2, 13, 21, 5, 32, 5, bn=True), {4: (32, 1)}, None),          # Cin4 = 8 with 5 real channels, odd grid
    (case(2, 24, 48, 128, 128, 3, bn=True), {12: (128, 1), 36: (128, 1)}, 2),  # the generator's own layer: the 512-row clamp keeps SL at 1
]


def test_the_fused_cases_name_every_instantiation():
    inst = {i for _, table, _ in FUSED for i in table.values()}
    assert inst == {(128, 1), (128, 2), (64, 1), (64, 2), (64, 4)} | {(cw, sl) for cw in (32, 16) for sl in (1, 2, 4, 8)} and len(inst) == 13


@pytest.mark.parametrize("c,table,rows", FUSED, ids=["x".join(map(str, f[0][:6])) for f in FUSED])
def test_fused_bn_reduction(dbg, c, table, rows):
    g = dispatch(c, 0)
    assert g["fused"] and not g["swap"] and max(table) <= g["cap"]
    for (v, asked), (_, red) in sweep(dbg, c, 0, (1, 2), tuple(table)).items():
        cw, sl = table[asked]
        assert red & FUSED_BN and not red & (SEPARATE_BN | SWAPPED | CLASSES)
        assert ((red >> 8) & 0xff, red & 0xff) == (cw, sl), (asked, hex(red))  # wgrad_reduce_bn_kernel<cw, sl>
        rb = (red >> 16) & 0x3ff
        assert rb == (rows if rows else 256 // cw // sl), (asked, rb)
        assert -(-g["mreal"] // rb) <= 1024
    if rows == 4:
        assert -(-g["mreal"] // 2) > 1024 and -(-g["mreal"] // 4) == 600  # the doubling path


# ---- d) separate BN form (bn_dot + bn_finish) ----------------------------------------------------------------------------------------
SEPARATE = {
    "swapped": case(1, 24, 48, 32, 16, 3, bn=True),
    "culled": case(2, 12, 24, 128, 128, 3, d=16, bn=True),
    "cout196": case(1, 6, 10, 64, 196, 3, bn=True),
}


@pytest.mark.parametrize("name", list(SEPARATE))
def test_separate_bn_form(dbg, name):
    c = SEPARATE[name]
    g = dispatch(c, 0)
    assert g["separate"] and g["swap"] == (name == "swapped") and (g["ntaps"] < 9) == (name == "culled")
    res = sweep(dbg, c, 0, (1, 2), (1, 3, ALL))
    for out, red in res.values():
        assert red & SEPARATE_BN and not red & (FUSED_BN | CLASSES) and bool(red & SWAPPED) == (name == "swapped") and (red >> 8) & 0xff == 0
    if name == "culled":
        for out, _ in res.values():
            dw = inner(out["dw"]).reshape(3, 3, 128, 128)
            assert (dw[0] == 0).all() and (dw[2] == 0).all()


# ---- e) class-structured up form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,splits", [(case(1, 12, 20, 128, 64, 3, bn=True), (1, 4)), (case(2, 7, 9, 64, 32, 3, bn=True), (1, 2))])
def test_class_structured_up_form(dbg, c, splits):
    g = dispatch(c, 2)
    assert g["classes"] and g["separate"] and not g["swap"] and max(splits) <= g["cap"]
    res = sweep(dbg, c, 2, (0, 1, 2), splits)
    for out, red in res.values():
        assert red & CLASSES and red & SEPARATE_BN and not red & (FUSED_BN | SWAPPED) and (red >> 8) & 0xff == 0
    # the same layer through the fused NN x2 loader (36 tap products per low-resolution pixel instead of 16) on the same data
    up1 = sweep(dbg, c, 1, (1,), (splits[-1],))
    (o1, red1), = up1.values()
    assert red1 & FUSED_BN and not red1 & CLASSES
    _, ref = reference(c, True)
    for out, _ in res.values():
        for nm, r in ref.items():
            assert float((inner(out[nm]) - inner(o1[nm])).abs().max()) < 1e-4 * max(1.0, float(r.abs().max())), nm


# ---- f) channel windows -----------------------------------------------------------------------------------------------------------------
WINDOWS = {
    # case, up mode, variants, splits, (ldx, x_coff, ldy, y_coff)
    "plain": (case(2, 13, 21, 64, 128, 3), 0, (0, 1, 2), (3,), (76, 8, 136, 4)),
    "plain_cin5": (case(1, 24, 48, 5, 32, 5), 0, (0, 1, 2), (7,), (16, 4, 44, 8)),   # the float4 group of channels 4..7 holds three strangers
    "fused_bn": (case(2, 13, 21, 5, 32, 5, bn=True), 0, (1, 2), (4,), (20, 12, 40, 4)),
    "separate_bn_swapped": (case(1, 24, 48, 32, 16, 3, bn=True), 0, (1, 2), (3,), (48, 12, 24, 4)),
    "class_structured": (case(2, 7, 9, 64, 32, 3, bn=True), 2, (0, 1, 2), (2,), (72, 4, 48, 12)),
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_channel_windows(dbg, name):
    """operands inside wider buffers whose other channels hold finite values of scale 1e3: same tolerances, same report words"""
    c, mode, variants, splits, win = WINDOWS[name]
    assert all(v % 4 == 0 for v in win) and win[1] and win[3] and win[0] > c[3] and win[2] > c[4]
    tight = sweep(dbg, c, mode, variants[-1:], splits)
    res = sweep(dbg, c, mode, variants, splits, win)
    (_, red0), = tight.values()
    assert all(red == red0 for _, red in res.values())


# ---- g) the fp16 kernel (conv_wgrad_dma_kernel<..., 2, true>) in every view ----------------------------------------------------------------
F16_SCALE = 4096.0  # what the plans use; dy = 1e-6 * U[0.25, 1]: an unscaled fp16 conversion would be subnormal or flush


@pytest.fixture(scope="module", autouse=True)
def worst_fp16_line():
    yield
    print("\nfp16 backward-filter against the rounded-operand reference, worst error relative to the tensor's scale: %.2e (bound 2e-4)"
          % WORST_F16["dw"])


def test_fp16_plain_cases_reach_every_tile():
    """wgrad_launch<128, 128>, <128, 64> and <128, 32>: every (BM, BN) launch_wgrad_T can pick"""
    assert {dispatch(c, mode)["tile_n"] for c, mode in PLAIN.values() if dispatch(c, mode)["dma_ok"]} == {32, 64, 128}


@pytest.mark.parametrize("name", list(PLAIN))
def test_fp16_direct_variant_and_split_counts(dbg, name):
    """every PLAIN case (both swapped views and the fused NN x2 loader among them) on the LDS-DMA variant in fp16, scale 4096; `leaky` and
    `elu` pass act' on load, are not dma_ok and must stay fp32: they meet the UNROUNDED reference, and the rounded one 10x worse"""
    c, mode = PLAIN[name]
    g = dispatch(c, mode)
    assert g["dma_ok"] == (name not in ("leaky", "elu"))
    res = sweep(dbg, c, mode, (1,), (1, 2, 3, 7, ALL), f16=F16_SCALE)
    for out, red in res.values():
        assert bool(red & SWAPPED) == name.startswith("swapped") and (red >> 8) & 0xff == 0 and not red & (FUSED_BN | SEPARATE_BN | CLASSES)


def test_fp16_plain_case_at_scale_1(dbg):
    c, mode = PLAIN["bn64"]
    sweep(dbg, c, mode, (1,), (1, 3, ALL), f16=1.0)


@pytest.mark.parametrize("c,splits", [(case(1, 12, 20, 128, 64, 3, bn=True), (1, 4)), (case(2, 7, 9, 64, 32, 3, bn=True), (1, 2))])
def test_fp16_class_structured_up_form(dbg, c, splits):
    res = sweep(dbg, c, 2, (1,), splits, f16=F16_SCALE)
    for out, red in res.values():
        assert red & CLASSES and red & SEPARATE_BN and not red & (FUSED_BN | SWAPPED) and (red >> 8) & 0xff == 0
    (o1, red1), = sweep(dbg, c, 1, (1,), (splits[-1],), f16=F16_SCALE).values()  # the fused NN x2 loader with the fused BN reduction
    assert red1 & FUSED_BN and not red1 & CLASSES
    _, ref = reference(c, True, F16_SCALE)
    for out, _ in res.values():
        for nm, r in ref.items():
            assert float((inner(out[nm]) - inner(o1[nm])).abs().max()) < 1e-4 * max(dy_unit(F16_SCALE), float(r.abs().max())), nm


def test_fp16_fused_bn_reduction(dbg):
    c, table, _ = FUSED[1]
    for (v, asked), (_, red) in sweep(dbg, c, 0, (1,), tuple(table), f16=F16_SCALE).items():
        assert red & FUSED_BN and ((red >> 8) & 0xff, red & 0xff) == table[asked]


def test_fp16_separate_bn_form_swapped(dbg):
    c = SEPARATE["swapped"]
    for out, red in sweep(dbg, c, 0, (1,), (1, 3, ALL), f16=F16_SCALE).values():
        assert red & SEPARATE_BN and red & SWAPPED and not red & (FUSED_BN | CLASSES)


def test_fp16_channel_window(dbg):
    c, mode, _, splits, win = WINDOWS["plain"]
    tight = sweep(dbg, c, mode, (1,), splits, f16=F16_SCALE)
    res = sweep(dbg, c, mode, (1,), splits, win, f16=F16_SCALE)
    (_, red0), = tight.values()
    assert all(red == red0 for _, red in res.values())


def test_fp16_forced_variants_without_an_fp16_form_run_the_dma_kernel(dbg):
    """every configuration of an fp16 launch multiplies alike.  The Winograd-domain family (3; wgrad_wino_ok) and the register-staged kernel
    (0) multiply in fp32 only and the three-stage ring (2) has no fp16 instantiation: forced on a shape that takes all of them in fp32 mode,
    the fp16 launch runs conv_wgrad_dma_kernel<..., 2, true> and the report word says variant 1 (sweep asserts it, and that fp16
    arithmetic ran)"""
    c = case(2, 24, 48, 64, 64, 3)
    sweep(dbg, c, 0, (0, 2, 3), (4,), f16=F16_SCALE)
