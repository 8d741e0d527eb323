"""Every convolution kernel family's epilogue options on windowed operands, one launch at a time, as a step plan builds its launches
(udet_debug_conv2d_ex, include/udet_debug.h): channel windows on x / y / res / y2 / uo / ua, the gap map of the packed weights, bias +
activation + second output + residual + accumulate + dU emission, act' on load, the two four-class forms of NN x2 + 3x3.

Every output (y, y2, uo) is a window of a wider row with guard rows in front and behind; the buffers are filled with SENTINEL, which must
survive everywhere outside the windows (y inside its window: random "old" values when the launch accumulates, else the sentinel -- a launch
that reads before it writes then shows).  Per launch:
  * against oracle/oracle_conv_ex.py in float64, relative to max(1, max|ref|): 1e-4 forward, 2e-4 backward-data and for the emitted u;
  * against the SAME forced configuration run without options (dense output, same bias / activation), whose output is v0 -- the
    accumulators of one configuration are deterministic, so this sees a one-element error:  y2 == v0;  act = none: y == (v0 + res) + old
    in float32;  with an activation the last bit is allowed (hipcc contracts the multiply of a leaky slope / the last multiply of the ELU
    polynomial into the residual add): 2 ulp of the largest operand;  u == y * act'(ua) in float32, ua holding exact zeros;
  * the family / tile / split mode under test really ran (udet_debug_last_conv), or its fall-back is asserted.
The float64 reference of a (problem, option set) is computed once per module."""
import functools
from dataclasses import dataclass, replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_conv_ex as X  # noqa: E402
from oracle.oracle_glue import ACT_ELU, ACT_LEAKY, ACT_NONE, SENTINEL  # noqa: E402
from test_fp16_kernels_gpu import mag, r16  # noqa: E402
from test_ops_gpu import FAMILIES, THIN_CASES, TILE_CASE, TILE_CONFIGS, TILE_FAMILIES, WINO_CASES, WINO_PAIRS, WS_OF, _tile_fits  # noqa: E402

GUARD = 2  # rows of the row width in front of and behind every output buffer
LEAKY = np.float32(0.1)


def up8(v):
    return (v + 7) // 8 * 8


@dataclass(frozen=True)
class Prob:
    """one launch's problem: the form and layer of udet_debug_conv_ex plus the x window"""
    form: int
    n: int
    h: int
    w: int
    cin: int
    cout: int
    k: int = 3
    stride: int = 1
    dil: int = 1
    up: int = 0
    x_coff: int = 8
    x_pad: int = 8
    kc: int = 0        # 0: the real channels (+ gap) rounded up to 8, as a plan sets it
    k_split: int = 0
    k_gap: int = 0
    xact: int = ACT_NONE  # act' on load (form 1)
    f16: bool = False
    pack_job: int = 0     # forms 0 / 1: 1 packs through a job of launch_pack_jobs (the per-step packer of the trainable networks)
    seed: int = 0         # shifts every seed of operands(): the two problems of a pair launch hold different data

    @property
    def backward(self):
        return self.form in (X.DGRAD, X.UP_DGRAD)

    @property
    def real(self):
        return self.cout if self.backward else self.cin

    @property
    def cols(self):
        return self.cin if self.backward else self.cout

    @property
    def K(self):
        return self.kc or up8(self.real + self.k_gap)

    @property
    def ldx(self):
        return self.x_coff + self.K + self.x_pad

    def grids(self):
        """(grid of x, grid of y)"""
        s = self.stride
        if self.form == X.FWD:
            return (self.h, self.w), (-(-(self.h << self.up) // s), -(-(self.w << self.up) // s))
        if self.form == X.DGRAD:
            return (-(-self.h // s), -(-self.w // s)), (self.h, self.w)
        lo, hi = (self.h, self.w), (2 * self.h, 2 * self.w)
        return (lo, hi) if self.form == X.UP_FWD else (hi, lo)


@dataclass(frozen=True)
class Opt:
    """one option set: (coff, pad) of each window; ld = coff + columns + pad"""
    name: str
    bias: bool = False
    act: int = ACT_NONE
    alpha: float = 0.0
    y: tuple = (8, 8)
    y2: tuple = None
    res: tuple = None
    accumulate: int = 0
    uact: int = -1          # >= 0: dU emission over [4, last multiple of 4 below the columns)
    ualpha: float = 0.0
    u: tuple = (4, 4)
    ua: tuple = (8, 8)
    ua_shift: int = 0       # the ua pointer offset by this many floats (1: not 16-byte aligned)
    urange: tuple = None    # the emission's [u_c0, u_c1); (0, 0): all columns; None: emit_range


S = Opt("S", bias=True, act=ACT_ELU, y=(8, 8), y2=(4, 4), res=(4, 4))
US = replace(S, name="US", res=(2, 6))                                   # res_coff = 2: epilogue4_out_ok is false
D_LEAKY = Opt("D-leaky", y=(8, 8), res=(4, 4), accumulate=1, uact=ACT_LEAKY, ualpha=float(LEAKY))
D_ELU = replace(D_LEAKY, name="D-elu", uact=ACT_ELU, ualpha=0.0)
UD = replace(D_LEAKY, name="UD", ua_shift=1)                             # the ua pointer 4 bytes off
H = Opt("H", bias=True, y=(2, 0), res=(4, 2))                            # flow head: ldy = 4, the refined flow's residual in ld = 8
HS = replace(H, name="HS", y2=(2, 0))                                    # ... and the pre-residual value as a second output
PLAIN_OF = lambda o: Opt("plain", bias=o.bias, act=o.act, alpha=o.alpha, y=(0, 0))  # noqa: E731


def emit_range(cols):
    c1 = (cols - 1) // 4 * 4
    assert 4 < c1 < cols, cols
    return 4, c1


def emit_of(o, cols):
    if o.urange is None:
        return emit_range(cols)
    c0, c1 = o.urange if o.urange != (0, 0) else (0, cols)
    assert 0 <= c0 < c1 <= cols, (o.urange, cols)
    return c0, c1


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def operands(p: Prob, o: Opt):
    """float32 host tensors of the launch, seeded by the problem alone (every option set of a problem sees the same x / w / bias)"""
    (ih, iw), (oh, ow) = p.grids()
    rows, sd = p.n * oh * ow, 100 * p.seed
    if p.f16:
        x = mag(p.n, ih, iw, p.ldx, seed=sd + 1)
        w = mag(p.k, p.k, p.cin, p.cout, seed=sd + 2, scale=(2.0 / (p.k * p.k * p.cin)) ** 0.5)
    else:
        x = randn(p.n, ih, iw, p.ldx, seed=sd + 1)
        w = randn(p.k, p.k, p.cin, p.cout, seed=sd + 2) * (2.0 / (p.k * p.k * p.cin)) ** 0.5
    d = dict(x=x, w=w, bias=randn(p.cout, seed=sd + 3) * 0.1 if o.bias else None, rows=rows)
    if p.xact != ACT_NONE:
        xa = randn(p.n, ih, iw, p.ldx, seed=sd + 4)
        xa[randn(p.n, ih, iw, p.ldx, seed=sd + 5) > 1.0] = 0.0
        d["xa"] = xa

    def out_buffer(win, old_seed=None):
        ld = win[0] + p.cols + win[1]
        b = torch.full((rows + 2 * GUARD, ld), SENTINEL)
        if old_seed is not None:
            b[GUARD:GUARD + rows, win[0]:win[0] + p.cols] = randn(rows, p.cols, seed=old_seed)
        return b

    d["y"] = out_buffer(o.y, sd + 6 if o.accumulate else None)
    if o.y2:
        d["y2"] = out_buffer(o.y2)
    if o.res:
        d["res"] = randn(rows, o.res[0] + p.cols + o.res[1], seed=sd + 7)
    if o.uact >= 0:
        d["uo"] = out_buffer(o.u)
        ua = randn(rows, o.ua[0] + p.cols + o.ua[1], seed=sd + 8)
        ua[randn(rows, ua.shape[1], seed=sd + 9) > 1.0] = 0.0   # exact zeros beside negatives and positives
        assert int((ua == 0).sum()) > 0 and int((ua < 0).sum()) > 0 and int((ua > 0).sum()) > 0
        d["ua"] = ua
    return d


def as_nhwc(buf, p: Prob, guard):
    (_, _), (oh, ow) = p.grids()
    body = buf[GUARD:GUARD + p.n * oh * ow] if guard else buf
    return body.reshape(p.n, oh, ow, -1)


@functools.lru_cache(maxsize=None)
def linear_part(p: Prob):
    """the float64 convolution of the problem, shared by its option sets; fp16 problems: of the operands as an fp16 kernel rounds them"""
    d = operands(p, PLAIN_OF(S))
    x, w = d["x"].double(), d["w"].double()
    if p.f16:
        x, w = r16(d["x"], 4096.0 if p.backward else 1.0), r16(d["w"])
    return X.linear_part(p.form, x, p.x_coff, p.K, w, p.grids()[1], p.k_split if p.k_gap else p.K, p.k_gap, p.stride, p.dil, p.up,
                         d["xa"].double() if "xa" in d else None, p.xact, float(LEAKY))


@functools.lru_cache(maxsize=None)
def reference(p: Prob, o: Opt):
    """float64 (y, y2, uo) bodies after the launch, [rows, ld]"""
    d = operands(p, o)
    f = lambda k: as_nhwc(d[k].double(), p, k in ("y", "y2", "uo")) if k in d else None  # noqa: E731
    kw = {}
    if o.uact >= 0:
        c0, c1 = emit_of(o, p.cols)
        kw = dict(uo=f("uo"), u_coff=o.u[0], ua=f("ua"), ua_coff=o.ua[0], uact=o.uact, ualpha=float(np.float32(o.ualpha)), u_c0=c0, u_c1=c1)
    # (the linear part -- x window, gap map, act' on load, the convolution -- is linear_part's: one per problem)
    yn, y2n, un = X.conv_ex(p.form, None, p.x_coff, p.K, d["w"].double(), f("y"), o.y[0], bias=None if d["bias"] is None else d["bias"].double(),
                            act=o.act, alpha=float(np.float32(o.alpha)), res=f("res"), res_coff=o.res[0] if o.res else 0, y2=f("y2"),
                            y2_coff=o.y2[0] if o.y2 else 0, accumulate=o.accumulate, lin=linear_part(p), **kw)
    flat = lambda t: None if t is None else t.reshape(d["rows"], -1)  # noqa: E731
    return flat(yn), flat(y2n), flat(un)


@pytest.fixture(scope="module")
def devel():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import _devel
    return _devel


@pytest.fixture
def lib(devel):
    yield devel.dbg
    devel.dbg.udet_debug_force_conv(0, 0, -1)
    devel.dbg.udet_debug_conv_fp16_grad_scale(0.0)
    devel.dbg.udet_debug_conv_fp16(0)


_ws = {}


def device_fields(p: Prob, o: Opt):
    """(device copies of the launch's tensors, the fields of its udet_debug_conv_ex)"""
    d = operands(p, o)
    g = {k: v.cuda() for k, v in d.items() if isinstance(v, torch.Tensor)}
    f = dict(form=p.form, n=p.n, h=p.h, wd=p.w, cin=p.cin, cout=p.cout, k=p.k, stride=p.stride, dilation=p.dil, up=p.up, kc=p.K,
             k_split=p.k_split if p.k_gap else p.K, k_gap=p.k_gap, x=g["x"], ldx=p.ldx, x_coff=p.x_coff, w=g["w"], act=o.act, alpha=o.alpha,
             y=(g["y"], GUARD * g["y"].shape[1]), ldy=g["y"].shape[1], y_coff=o.y[0], accumulate=o.accumulate, pack_job=p.pack_job)
    if "xa" in g:
        f.update(xa=g["xa"], xact=p.xact, xalpha=float(LEAKY))
    if "bias" in g:
        f["bias"] = g["bias"]
    if o.res:
        f.update(res=g["res"], ldres=g["res"].shape[1], res_coff=o.res[0])
    if o.y2:
        f.update(y2=(g["y2"], GUARD * g["y2"].shape[1]), ldy2=g["y2"].shape[1], y2_coff=o.y2[0])
    if o.uact >= 0:
        c0, c1 = emit_of(o, p.cols)
        ua = g["ua"]
        if o.ua_shift:  # the same values behind a pointer that is 4 bytes off a 16-byte boundary
            store = torch.zeros(ua.numel() + 4, device="cuda")
            store[o.ua_shift:o.ua_shift + ua.numel()] = ua.reshape(-1)
            g["ua_store"] = store
            ua = (store, o.ua_shift)
            assert (store.data_ptr() + 4 * o.ua_shift) % 16 == 4 * o.ua_shift
        f.update(uo=(g["uo"], GUARD * g["uo"].shape[1]), ldu=g["uo"].shape[1], u_coff=o.u[0], ua=ua, ldua=g["ua"].shape[1], ua_coff=o.ua[0],
                 uact=o.uact, ualpha=o.ualpha, u_c0=c0, u_c1=c1)
    return g, f


def launch(devel, p: Prob, o: Opt):
    """one udet_debug_conv2d_ex call; returns the host copies of (y, y2, uo) WITH their guard rows and the configuration word"""
    g, f = device_fields(p, o)
    need = devel.conv2d_ex_workspace_bytes(**f)
    if _ws.get("n", 0) < need:
        _ws["t"], _ws["n"] = torch.empty(need // 4, device="cuda"), need
    devel.conv2d_ex(workspace=_ws["t"], **f)
    torch.cuda.synchronize()
    out = {k: g[k].cpu() for k in ("y", "y2", "uo") if k in g}
    out["word"] = devel.dbg.udet_debug_last_conv()
    return out


def word(v):
    return dict(fam=v & 0xff, bm=(v >> 8) & 0xfff, ks=(v >> 20) & 0xff, fold=(v >> 28) & 1, tail=(v >> 29) & 1)


def dfo32(a, act, alpha):
    """act_dfo of common.h in float32: a > 0 ? 1 : fma(a, ue, us) -- one rounding, as a + 1 (ELU) or the constant (leaky, none)"""
    one = torch.ones_like(a)
    neg = {ACT_NONE: one, ACT_LEAKY: one * np.float32(alpha), ACT_ELU: a + one}[act]
    return torch.where(a > 0, one, neg)


def check(p: Prob, o: Opt, got, v0):
    """the launch's outputs against the float64 reference, against the plain run v0 [rows, cols] of the same configuration, and the
    sentinel everywhere else; returns y's deviation from float64 as a fraction of the scale"""
    d = operands(p, o)
    ref_y, ref_y2, ref_u = reference(p, o)
    rows, C = d["rows"], p.cols
    coeff = 2e-4 if p.backward else 1e-4
    body = lambda t: t[GUARD:GUARD + rows]  # noqa: E731
    rel = lambda a, r: float((a.double() - r).abs().max()) / max(1.0, float(r.abs().max()))  # noqa: E731

    def untouched(name, win, width):
        b, init = got[name], d[name]
        assert torch.equal(b[:GUARD], init[:GUARD]) and torch.equal(b[GUARD + rows:], init[GUARD + rows:]), (name, "guard rows written")
        lo, hi = win[0], win[0] + width
        assert torch.equal(body(b)[:, :lo], body(init)[:, :lo]) and torch.equal(body(b)[:, hi:], body(init)[:, hi:]), (name, "written outside its window")

    yw = body(got["y"])[:, o.y[0]:o.y[0] + C]
    untouched("y", o.y, C)
    e = rel(yw, ref_y[:, o.y[0]:o.y[0] + C])
    print("%s %s: y %.2e of the scale (bound %.0e)" % (p, o.name, e, coeff))
    assert torch.isfinite(yw).all() and e < coeff, ("y against float64", e)
    if v0 is None:
        return e
    if o.y2:
        untouched("y2", o.y2, C)
        y2w = body(got["y2"])[:, o.y2[0]:o.y2[0] + C]
        assert rel(y2w, ref_y2[:, o.y2[0]:o.y2[0] + C]) < coeff
        assert torch.equal(y2w, v0), ("y2 is not the plain run's output", int((y2w != v0).sum()))
    exp, big = v0, v0.abs()
    if o.res:
        r = d["res"][:, o.res[0]:o.res[0] + C]
        exp, big = exp + r, torch.maximum(big, r.abs())
    if o.accumulate:
        old = body(d["y"])[:, o.y[0]:o.y[0] + C]
        exp, big = exp + old, torch.maximum(big, old.abs())
    if o.act == ACT_NONE:
        assert torch.equal(yw, exp), ("y is not (v0 + res) + old in float32", int((yw != exp).sum()), float((yw - exp).abs().max()))
    else:  # the multiply in front of the residual add may be contracted: the last bit
        big = torch.maximum(big, exp.abs())
        ulp = torch.from_numpy(np.spacing(big.numpy()))
        worst = float(((yw - exp).abs() / ulp).max())
        print("   differential: %.2f ulp of the largest operand" % worst)
        assert worst <= 2.0, ("y against (v0 + res) + old beyond the contraction's last bit", worst)
    if o.uact >= 0:
        c0, c1 = emit_of(o, C)
        untouched("uo", (o.u[0] + c0, 0), c1 - c0)
        uw = body(got["uo"])[:, o.u[0] + c0:o.u[0] + c1]
        assert rel(uw, ref_u[:, o.u[0] + c0:o.u[0] + c1]) < 2e-4
        ua = d["ua"][:, o.ua[0] + c0:o.ua[0] + c1]
        expu = yw[:, c0:c1] * dfo32(ua, o.uact, o.ualpha)
        assert torch.equal(uw, expu), ("u is not y * act'(ua) in float32", int((uw != expu).sum()))
        assert torch.equal(uw[ua == 0], (yw[:, c0:c1] * (LEAKY if o.uact == ACT_LEAKY else np.float32(1)))[ua == 0])
    return e


def run(devel, p: Prob, opts, force=None, expect=None):
    """the plain run, then every option set of `opts`, all on the forced configuration; expect(word, problem): the family assertion.
    Returns the configuration words (plain first)."""
    if force is not None:
        devel.dbg.udet_debug_force_conv(*force)
    plain = PLAIN_OF(opts[0])
    assert all(PLAIN_OF(o) == plain for o in opts)
    base = launch(devel, p, plain)
    words = [base["word"]]
    rows = operands(p, plain)["rows"]
    v0 = base["y"][GUARD:GUARD + rows]
    check(p, plain, base, None)
    for o in opts:
        got = launch(devel, p, o)
        words.append(got["word"])
        check(p, o, got, v0)
    if expect:
        for v in words:
            expect(word(v))
    return [word(v) for v in words]


# ---- implicit-GEMM families ------------------------------------------------------------------------------------------------------------------
TN, TH, TW, TCIN, TCOUT, TK, TS = TILE_CASE
TILE_S = Prob(X.FWD, TN, TH, TW, TCIN, TCOUT, TK, TS)                 # 40 channels at x_coff = 8 of 56, 100 columns
TILE_D = Prob(X.DGRAD, TN, TH, TW, TCIN, TCOUT, TK, TS, x_coff=4)     # 100 real channels of kc = 104 at x_coff = 4, 40 columns
TILE_S98 = replace(TILE_S, cout=98)                                   # cout = 98: no whole quads


def expect_family(family, p: Prob):
    """the assertion of test_ops_gpu.test_conv_kernel_families, its _tile_fits exemption included"""
    th = 8 if family == "tile8" else 4

    def f(w):
        if WS_OF[family] == 3:
            fits = _tile_fits(th, p.K, p.cols, p.k, 1 if p.backward else p.stride) and p.K <= 256 and p.cols <= 256
            if not fits:
                return
            assert w["bm"] == th, w
        assert w["fam"] == WS_OF[family], (family, w)
        if "_fold" in family or "_2pass" in family:
            assert w["ks"] > 1 and w["fold"] == (1 if "_fold" in family else 0), (family, w)
    return f


@pytest.mark.parametrize("optset", ["S", "D", "U"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_gemm_families(devel, lib, family, optset):
    if optset == "S":
        run(devel, TILE_S, [S], FAMILIES[family], expect_family(family, TILE_S))
    elif optset == "D":
        run(devel, TILE_D, [D_LEAKY, D_ELU], FAMILIES[family], expect_family(family, TILE_D))
    else:
        run(devel, TILE_S, [US], FAMILIES[family], expect_family(family, TILE_S))
        run(devel, TILE_S98, [S], FAMILIES[family], expect_family(family, TILE_S98))
        run(devel, TILE_D, [UD], FAMILIES[family], expect_family(family, TILE_D))


@pytest.mark.parametrize("family,bm,bn", TILE_CONFIGS)
def test_every_tile_with_backward_options(devel, lib, family, bm, bn):
    """the batched non-plain store loop is instantiated per tile"""
    bit, fam = (1 << 19, 6) if family == "self_staging" else TILE_FAMILIES[family]

    def expect(w):
        assert w["fam"] == fam and w["bm"] == bm, w
    run(devel, TILE_D, [D_LEAKY], (bm + bit, bn, 1), expect)


@pytest.mark.parametrize("family", ["wave_spec", "lds_dma"])
def test_pack_jobs_modes_0_and_1(devel, lib, family):
    """the operands of S and D packed by jobs of modes 0 / 1 (launch_pack_jobs), as a plan packs its trainable layers every step"""
    run(devel, replace(TILE_S, pack_job=1), [S], FAMILIES[family], expect_family(family, TILE_S))
    run(devel, replace(TILE_D, pack_job=1), [D_LEAKY], FAMILIES[family], expect_family(family, TILE_D))


TAIL_D = Prob(X.DGRAD, 2, 96, 96, 64, 64, 3, 1)


@pytest.mark.parametrize("family", ["lds_dma", "lds_dma_ring3"])
def test_tail_split_with_backward_options(devel, lib, family):
    """test_ops_gpu.test_conv_tail_split's launch (288 tiles of 64 x 64: one whole round + 32 tiles cut into K slices) accumulating and
    emitting: the old y and the residual once, in the whole rounds and in the tail"""
    bm = 64 + ((1 << 17) if family == "lds_dma" else (1 << 22))

    def expect(w):
        assert w["fam"] == WS_OF[family] and w["tail"] == 1 and w["ks"] >= 2, w
    run(devel, TAIL_D, [D_LEAKY], (bm, 64, 256), expect)


# ---- Winograd ----------------------------------------------------------------------------------------------------------------------------------
def wino_variant_ok(v, cols):
    np_ = (cols + 127) // 128 * 128 if cols > 64 else (64 if cols > 32 else 32)   # conv_wino_np
    bn = 64 if (v == 4 or v % 2 == 0) else 32                                     # conv_wino_variant_ok
    return 0 <= v <= 4 and np_ % bn == 0 and (cols > bn // 2 or bn == 32)


def expect_wino(v, p: Prob, min_ks=1):
    ran = [u for u in (v, v ^ 1) if wino_variant_ok(u, p.cols)]  # apply_forced: the variant asked for, else its sibling, else the built-in choice

    def f(w):
        if ran:
            assert w["fam"] == 9 and w["bm"] == ran[0] and w["ks"] >= min_ks, (v, w)
        else:
            assert w["fam"] != 9, (v, w)
    return f


@pytest.mark.parametrize("variant,ks", WINO_PAIRS)
@pytest.mark.parametrize("case", [WINO_CASES[1], WINO_CASES[2]], ids=["odd-ragged", "dilated"])
@pytest.mark.parametrize("optset", ["S", "D"])
def test_winograd_with_options(devel, lib, optset, case, variant, ks):
    """with options the Winograd kernels leave epi4_finish_plain32 for epi4_request / epi4_finish.  On the odd / ragged case the backward-data
    launch has 24 columns: variants 0 and 2 then run their 32-column siblings 1 and 3 and variant 4 falls back to the built-in choice
    (asserted), so those runs repeat others; every variant itself runs with D on the dilated case (40 columns) and on the 128-channel case
    of test_winograd_split_k_accumulates_once."""
    n, h, w, cin, cout, d = case
    p = Prob(X.FWD if optset == "S" else X.DGRAD, n, h, w, cin, cout, 3, 1, d)
    run(devel, p, [S] if optset == "S" else [D_LEAKY, D_ELU], ((1 << 25) + variant, 0, ks), expect_wino(variant, p))


@pytest.mark.parametrize("variant,ks", [(v, k) for v, k in WINO_PAIRS if k > 1])
def test_winograd_split_k_accumulates_once(devel, lib, variant, ks):
    """K slices need >= 6 stages of 8 channels each (conv_wino_max_ksplit): the 128-channel case really splits in two"""
    n, h, w, cin, cout, d = WINO_CASES[3]
    p = Prob(X.DGRAD, n, h, w, cin, cout, 3, 1, d)
    run(devel, p, [D_LEAKY], ((1 << 25) + variant, 0, ks), expect_wino(variant, p, min_ks=2))


# ---- tile-resident -----------------------------------------------------------------------------------------------------------------------------
THIN = THIN_CASES[7]  # 1 x 30 x 50, 16 -> 16, 3x3: ragged on both axes, fits the tile kernel in both directions
assert THIN == (1, 30, 50, 16, 16, 3, 1) and all(_tile_fits(th, 16, 16, 3, 1) for th in (4, 8))


@pytest.mark.parametrize("optset", ["S", "D", "U"])
@pytest.mark.parametrize("family", ["tile8", "tile4"])
def test_tile_resident_with_options(devel, lib, family, optset):
    n, h, w, cin, cout, k, s = THIN
    ps, pd = Prob(X.FWD, n, h, w, cin, cout, k, s), Prob(X.DGRAD, n, h, w, cin, cout, k, s)
    th = 8 if family == "tile8" else 4

    def expect(wd):
        assert wd["fam"] == 3 and wd["bm"] == th, wd
    if optset == "S":
        run(devel, ps, [S], FAMILIES[family], expect)
    elif optset == "D":
        run(devel, pd, [D_LEAKY, D_ELU], FAMILIES[family], expect)
    else:
        run(devel, ps, [US], FAMILIES[family], expect)
        run(devel, pd, [UD], FAMILIES[family], expect)


# ---- direct 2-channel kernels ------------------------------------------------------------------------------------------------------------------
def expect_fam(fam):
    def f(w):
        assert w["fam"] == fam, w
    return f


@pytest.mark.parametrize("case,dil", [((2, 13, 37, 98, 3), 1), ((1, 31, 45, 50, 5), 1), ((1, 16, 64, 36, 3), 2)],
                         ids=["3x3-windowed", "5x5-windowed", "3x3-dilated-generic"])
def test_two_channel_heads_with_options(devel, lib, case, dil):
    """H (the refined flow's residual, ldy = 4) on the direct kernel for two output channels, and the backward-data mirror (two real input
    channels of kc = 8) accumulating and emitting on the direct kernel for two input channels; dense unit-stride 3x3 / 5x5 windows take
    the constant-stride variants (conv_thin_nw / conv_thin_kw), the dilated one the generic kernels"""
    n, h, w, cin, k = case
    run(devel, Prob(X.FWD, n, h, w, cin, 2, k, 1, dil), [H, HS], None, expect_fam(8))
    run(devel, Prob(X.DGRAD, n, h, w, cin, 2, k, 1, dil, x_coff=0, x_pad=0, kc=8), [D_LEAKY, D_ELU], None, expect_fam(7))


GAP = Prob(X.FWD, 1, 13, 37, 21, 2, 3, 1, x_coff=8, x_pad=8, kc=32, k_split=13, k_gap=3)  # the PWC slab in small


@pytest.mark.parametrize("packer", [0, 1], ids=["pack_weights", "pack_job"])
@pytest.mark.parametrize("family", [None, "wave_spec", "lds_dma", "plain", "self_staging", "tile8"])
def test_flow_head_over_a_gap(devel, lib, family, packer):
    """x_coff > 0 and a 3-row gap at k_split: three junk channels inside the K window meet zero weight rows.  Both packers of a plan hold
    their own copy of the gap map: pack_weights_kernel (PWC-Net, packed once) and pack_jobs_kernel mode 0 (the per-step job table)"""
    p = replace(GAP, pack_job=packer)
    run(devel, p, [H], None if family is None else FAMILIES[family], expect_fam(8) if family is None else expect_family(family, p))


@pytest.mark.parametrize("packer", [0, 1], ids=["pack_weights", "pack_job"])
def test_gap_map_on_a_wide_layer_and_winograd(devel, lib, packer):
    """the same gap under 32 output columns (no direct kernel): implicit GEMM and the Winograd operand built from the packed weights"""
    p = replace(GAP, cout=32, pack_job=packer)
    run(devel, p, [S], FAMILIES["lds_dma"], expect_family("lds_dma", p))
    run(devel, p, [S], ((1 << 25) + 1, 0, 1), expect_wino(1, p))


# ---- stride-2 backward-data ----------------------------------------------------------------------------------------------------------------------
S2_CASES = {"even-5x5-merged": Prob(X.DGRAD, 1, 32, 64, 16, 32, 5, 2), "odd-3x3-per-class": Prob(X.DGRAD, 1, 31, 47, 32, 64, 3, 2),
            "1x1-classes-without-taps": Prob(X.DGRAD, 1, 12, 20, 16, 24, 1, 2), "1x1-odd": Prob(X.DGRAD, 1, 11, 19, 16, 24, 1, 2)}


S2_FAMILIES = ["wave_spec", "lds_dma", "self_staging", "tile8", "wave_spec_split4_fold", "lds_dma_split3_2pass"]
# launches of one tap or none (1x1 kernels): the two staging forms, both split modes (which cannot split) and, on the odd grid, the tile kernel
S2_RUNS = ([(c, f) for c in ("even-5x5-merged", "odd-3x3-per-class") for f in [None] + S2_FAMILIES]
           + [(c, f) for c in ("1x1-classes-without-taps", "1x1-odd") for f in (None, "wave_spec", "lds_dma", "wave_spec_split4_fold", "lds_dma_split3_2pass")]
           + [("1x1-odd", "tile8")])


@pytest.mark.parametrize("case,family", S2_RUNS)
def test_stride2_backward_data_with_options(devel, lib, case, family):
    """four merged parity classes in one launch / one launch per class (every pixel accumulated by exactly one of them) / classes without
    taps, which still write old + res and emit from that (conv_host.hip conv_setup_dgrad).  The configuration word is that of the LAST
    launch: the merged one, or class (1, 1) of an odd grid -- four taps of the 3x3 kernel (K slices as asked for), none of the 1x1 kernel.
    A 1x1 launch has at most one tap of 24 channels, less than two K stages: a forced split runs its family unsplit (ks = 1, no fold); the
    tile kernel declines a launch without taps, which then runs the built-in choice."""
    p = S2_CASES[case]
    default = run(devel, p, [D_LEAKY])[0]
    if family is None:
        return

    def expect(w):
        if p.k > 1:
            expect_family(family, p)(w)
        elif family == "tile8":
            assert w["fam"] == default["fam"] and w["fam"] != 3, (w, default)
        else:
            assert w["fam"] == WS_OF[family] and w["ks"] == 1 and w["fold"] == 0, (family, w)
    run(devel, p, [D_LEAKY, D_ELU], FAMILIES[family], expect)


# ---- the four-class forms of NN x2 + 3x3 ---------------------------------------------------------------------------------------------------------
UP_FAMILIES = [None, "plain", "wave_spec", "lds_dma", "lds_dma_split3", "tile8", "tile4", "self_staging", "wave_spec_split4_fold",
               "lds_dma_split3_2pass", "lds_dma_ring3", "wino"]


@pytest.mark.parametrize("family", UP_FAMILIES)
@pytest.mark.parametrize("chan", [(32, 32), (128, 64)], ids=["32-32", "128-64"])
@pytest.mark.parametrize("grid", [(12, 20), (7, 9)], ids=["even", "odd"])
@pytest.mark.parametrize("form", [X.UP_FWD, X.UP_DGRAD], ids=["fwd-S", "dgrad-D"])
def test_up_forms_with_options(devel, lib, form, grid, chan, family):
    """setup_up_fwd (ncls = 4, pack mode 5) with S, setup_up_dgrad (stride-2 walk over dU, pack mode 6) with D, on the default selection and
    on every family: a forced family that does not take the launch falls back to the default's, read from udet_debug_last_conv"""
    p = Prob(form, 1, grid[0], grid[1], chan[0], chan[1])
    opts = [S] if form == X.UP_FWD else [D_LEAKY, D_ELU]
    default = run(devel, p, opts[:1])[0]
    if family is None:
        return
    force = ((1 << 25), 0, 1) if family == "wino" else FAMILIES[family]
    want = 9 if family == "wino" else WS_OF[family]

    def expect(w):
        assert w["fam"] in (want, default["fam"]), (family, w, default)
        if family == "wino":
            assert w["fam"] != 9, w  # (four classes / a stride-2 walk: never a Winograd launch)
        if want in (0, 1, 2, 4, 6):
            assert w["fam"] == want, (family, w)  # every implicit-GEMM family takes ncls = 4 and isy = 2
    run(devel, p, opts, force, expect)


@pytest.mark.parametrize("family", [None, "plain", "wave_spec", "lds_dma", "self_staging"])
def test_loader_nn_x2_with_skip_options(devel, lib, family):
    """form 0 with up = 1: x on the 7 x 9 grid read through the loader's nearest-neighbour x2 (no uniform K cursor), S on the 14 x 18 output"""
    p = Prob(X.FWD, 2, 7, 9, 24, 40, up=1)
    run(devel, p, [S, US], None if family is None else FAMILIES[family], None if family is None else expect_family(family, p))


# ---- act' on load --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES) + ["wino"])
def test_act_on_load_with_backward_options(devel, lib, family):
    """form 1 with xa: only the plain and wave-specialised families read act'(xa) on load (dma_ok, conv_wino_ok, conv_tile_lds_bytes); every
    other forced family falls back to one of them, and the values hold"""
    p = replace(TILE_D, xact=ACT_LEAKY)
    force = ((1 << 25), 0, 1) if family == "wino" else FAMILIES[family]

    def expect(w):
        assert w["fam"] in (0, 1), (family, w)
        if family != "wino" and WS_OF[family] in (0, 1):
            assert w["fam"] == WS_OF[family], (family, w)
    run(devel, p, [D_LEAKY], force, expect)


# ---- fp16 mode -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optset", ["S", "D"])
def test_fp16_with_options(devel, lib, optset):
    """against the rounded-operand reference of test_fp16_kernels_gpu (its helpers, its bounds: the fp32 rule of the operator): the
    gradient scale 4096 must come out of the accumulators before res and the old y go in"""
    lib.udet_debug_conv_fp16(1)
    lib.udet_debug_conv_fp16_grad_scale(4096.0)
    p = replace(TILE_S if optset == "S" else TILE_D, f16=True)
    run(devel, p, [S] if optset == "S" else [D_LEAKY, D_ELU], FAMILIES["lds_dma"], expect_fam(2))
