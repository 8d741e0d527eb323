"""The 2-channel heads in the form a plan runs them wherever the direct kernel is not taken (csrc/plan_exec.hip run_fwd's head branch:
every PWC-Net flow / up_feat head in fp32, every head in fp16 mode), through udet_debug_conv2d_head_ex (include/udet_debug.h):

    weights packed with the taps folded into the N axis (modes 3 / 4, k_split / k_gap)  ->  ONE 1x1 GEMM into z  ->  launch_tap_gather

Reference: oracle/oracle_conv_ex.py head() in float64 -- conv2d_same / conv2d_transpose_k4s2_same on the x window with the gap channels
dropped, plus bias -- under the project's forward rule 1e-4 * max(1, max|ref|).  x and y are windows of wider rows with guard rows in front
and behind; everything outside the windows holds SENTINEL and must come back bit-identical (x entirely, y outside [y_coff, y_coff + 2)); the
gap channels of x hold 1e30, which only exact zero weight rows annihilate.  Every shape runs through both packers (launch_pack_taps_into_n /
a job of launch_pack_jobs) and into two output windows -- (ldy, y_coff) = (4, 0): tap_gather2_kernel, (7, 3): the generic tap_gather_kernel --
and the four results are bit-identical: the packers write the same wz, the two gather kernels add the same terms in the same order.  The GEMM
runs unforced and under three forced families (always eligible here: the entry hands over a zero block and no act' operand, and the forced
tiles are instantiated), and udet_debug_last_conv says which one ran.  The float64 reference of a shape is computed once per module."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_conv_ex as X  # noqa: E402
from oracle.oracle_glue import SENTINEL  # noqa: E402
from test_fp16_kernels_gpu import check as check_fp16, mag, r16  # noqa: E402
from test_ops_gpu import FAMILIES, WS_OF  # noqa: E402

GUARD = 2          # rows of the row width in front of and behind every buffer
X_COFF, X_PAD = 8, 4
GAP_GARBAGE = 1e30
WINDOWS = ((4, 0), (7, 3))  # (ldy, y_coff): float2 gather / generic gather
# (n, h, w, cin, k, (kc, k_split, k_gap) or None: kc = cin rounded up to 8, no gap), k = 0: the transposed 4x4 stride-2 form
FORWARD = [(1, 2, 3, 40, 5, None),                 # taps culled: the grid is smaller than the filter
           (2, 7, 9, 36, 3, None),                 # 9 taps = one full trip of eight + a tail of one
           (1, 9, 11, 50, 5, None),                # 25 taps, ldz = 64
           (3, 8, 8, 196, 3, None),
           (1, 13, 37, 565, 3, (568, 529, 3))]     # the PWC level-2 head's own map
TRANSPOSED = [(1, 1, 1, 32, 0, None),
              (2, 5, 7, 36, 0, None),
              (1, 6, 10, 529, 0, (532, 200, 3)),   # a gap in the middle of the channel axis
              (1, 12, 20, 100, 0, None)]
CASES = FORWARD + TRANSPOSED
GEMM_FAMILIES = ["unforced", "plain", "lds_dma", "self_staging"]
UNFORCED_FAMILY = {False: 1, True: 2}  # heuristic_cfg (csrc/conv_select.hip): wave-specialised in fp32, LDS-DMA in fp16 mode
FP16_CASES = [FORWARD[1], FORWARD[2], FORWARD[3], TRANSPOSED[1], TRANSPOSED[3]]


def geometry(case):
    n, h, w, cin, k, gap = case
    tr = k == 0
    kc, k_split, k_gap = gap if gap else ((cin + 7) // 8 * 8, (cin + 7) // 8 * 8, 0)
    return dict(n=n, h=h, w=w, cin=cin, k=4 if tr else k, tr=tr, kc=kc, k_split=k_split, k_gap=k_gap, ldx=X_COFF + kc + X_PAD,
                oh=2 * h if tr else h, ow=2 * w if tr else w)


@functools.lru_cache(maxsize=None)
def operands(case, f16=False):
    """float32 host tensors: the guarded x buffer [GUARD + n*h*w + GUARD, ldx], w (HWIO; transposed: HWOI), bias"""
    g = geometry(case)
    rows = g["n"] * g["h"] * g["w"]
    k, cin = g["k"], g["cin"]
    wshape = (4, 4, 2, cin) if g["tr"] else (k, k, cin, 2)
    scale = (1.0 / (16 * cin)) ** 0.5 if g["tr"] else (2.0 / (k * k * cin)) ** 0.5
    gen = torch.Generator().manual_seed(7)
    if f16:
        body, w, bias = mag(rows, g["kc"], seed=61), mag(*wshape, seed=62, scale=scale), mag(2, seed=63, scale=0.1)
    else:
        body, w, bias = torch.randn(rows, g["kc"], generator=gen), torch.randn(*wshape, generator=gen) * scale, torch.randn(2, generator=gen) * 0.1
    if g["k_gap"]:
        assert not f16  # (1e30 is infinite in fp16: the fp16 cases carry no gap)
        body[:, g["k_split"]:g["k_split"] + g["k_gap"]] = GAP_GARBAGE
    x = torch.full((rows + 2 * GUARD, g["ldx"]), SENTINEL)
    x[GUARD:GUARD + rows, X_COFF:X_COFF + g["kc"]] = body
    return dict(x=x, w=w, bias=bias)


def x_nhwc(case, f16=False):
    g = geometry(case)
    rows = g["n"] * g["h"] * g["w"]
    return operands(case, f16)["x"][GUARD:GUARD + rows].reshape(g["n"], g["h"], g["w"], g["ldx"])


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 [n*oh*ow, 2]"""
    g, d = geometry(case), operands(case)
    y = X.head(x_nhwc(case).double(), X_COFF, g["kc"], d["w"].double(), d["bias"].double(), g["k_split"], g["k_gap"], g["tr"])
    assert y.shape == (g["n"], g["oh"], g["ow"], 2) and torch.isfinite(y).all()
    return y.reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def reference_fp16(case):
    """float64 (rounded-operand result, unrounded result): the real channels and the weights as an fp16 kernel multiplies them, bias unrounded"""
    g, d = geometry(case), operands(case, True)
    x = x_nhwc(case, True)
    xr = x.double().clone()
    xr[..., X_COFF:X_COFF + g["kc"]] = r16(x[..., X_COFF:X_COFF + g["kc"]])
    f = lambda xx, ww: X.head(xx, X_COFF, g["kc"], ww, d["bias"].double(), g["k_split"], g["k_gap"], g["tr"]).reshape(-1, 2)  # noqa: E731
    return f(xr, r16(d["w"])), f(x.double(), d["w"].double())


@pytest.fixture(scope="module")
def devel():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unsupervised_detection_amd import _devel
    return _devel


@pytest.fixture
def lib(devel):
    try:
        yield devel.dbg
    finally:
        devel.dbg.udet_debug_force_conv(0, 0, -1)
        devel.dbg.udet_debug_conv_fp16(0)


_ws = {}


def launch(devel, case, pack_job, window, f16=False):
    """one udet_debug_conv2d_head_ex call; (the y window [rows, 2] on the host, the GEMM's configuration word).  Asserts that nothing outside
    the y window and nothing of x changed."""
    g, d = geometry(case), operands(case, f16)
    ldy, y_coff = window
    rows = g["n"] * g["oh"] * g["ow"]
    x, w, bias = d["x"].cuda(), d["w"].cuda(), d["bias"].cuda()
    y0 = torch.full((rows + 2 * GUARD, ldy), SENTINEL)
    y = y0.cuda()
    f = dict(n=g["n"], h=g["h"], wd=g["w"], cin=g["cin"], k=g["k"], kc=g["kc"], k_split=g["k_split"], k_gap=g["k_gap"], x=(x, GUARD * g["ldx"]),
             ldx=g["ldx"], x_coff=X_COFF, w=w, bias=bias, y=(y, GUARD * ldy), ldy=ldy, y_coff=y_coff, transposed=int(g["tr"]), pack_job=pack_job)
    need = devel.conv2d_head_ex_workspace_bytes(**f)
    assert need > 0
    if _ws.get("n", 0) < need:
        _ws["t"], _ws["n"] = torch.empty(need // 4, device="cuda"), need
    devel.conv2d_head_ex(workspace=_ws["t"], **f)
    torch.cuda.synchronize()
    word = devel.dbg.udet_debug_last_conv()
    got = y.cpu()
    tag = (case, "pack_job", pack_job, "window", window)
    assert torch.equal(x.cpu(), d["x"]), (tag, "x changed")
    assert torch.equal(got[:GUARD], y0[:GUARD]) and torch.equal(got[GUARD + rows:], y0[GUARD + rows:]), (tag, "guard rows written")
    body = got[GUARD:GUARD + rows]
    assert torch.equal(body[:, :y_coff], y0[GUARD:GUARD + rows, :y_coff]) and torch.equal(body[:, y_coff + 2:], y0[GUARD:GUARD + rows, y_coff + 2:]), \
        (tag, "written outside the y window")
    return body[:, y_coff:y_coff + 2].clone(), word


def four_launches(devel, case, f16=False):
    """both packers x both output windows of one shape: {(pack_job, window): (y window, word)}"""
    return {(pj, win): launch(devel, case, pj, win, f16) for pj in (0, 1) for win in WINDOWS}


def assert_family(word, family, f16=False):
    fam = word & 0xff
    if family == "unforced":
        assert fam == UNFORCED_FAMILY[f16], ("the untuned choice of the 1x1 GEMM", fam)
    else:  # fp16 mode: the register-staged families have no fp16 form and run the LDS-DMA kernel on the same tile
        assert fam == (2 if f16 and WS_OF[family] in (0, 1) else WS_OF[family]), (family, fam)
        assert (word >> 20) & 0xff == FAMILIES[family][2], (family, "split count", word)
    assert not (word >> 30) & 1


def assert_bit_identical(runs):
    first_key = next(iter(runs))
    for key, (y, _) in runs.items():
        assert torch.equal(y, runs[first_key][0]), ("(pack_job, window)", key, "differs from", first_key, int((y != runs[first_key][0]).sum()),
                                                    float((y - runs[first_key][0]).abs().max()))


@pytest.mark.parametrize("family", GEMM_FAMILIES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_head_as_the_plan_runs_it(devel, lib, case, family):
    ref = reference(case)
    bound = 1e-4 * max(1.0, float(ref.abs().max()))
    if family != "unforced":
        lib.udet_debug_force_conv(*FAMILIES[family])
    runs = four_launches(devel, case)
    for key, (y, word) in runs.items():
        assert_family(word, family)
        err = float((y.double() - ref).abs().max())
        print("%s %s pack_job=%d window=%s: %.2e (bound %.2e)" % (case, family, key[0], key[1], err, bound))
        assert torch.isfinite(y).all() and err < bound, (key, err, bound)
    assert_bit_identical(runs)


@pytest.mark.parametrize("case", [c for c in CASES if geometry(c)["kc"] <= 64], ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_head_agrees_with_the_direct_kernel(devel, lib, case):
    """kc <= 64: a plan takes the direct kernel of conv_thin.hip in fp32 (family 8, what udet_conv2d / udet_conv2d_transpose4x4s2 run untuned);
    the GEMM + gather form of the same data agrees with it to the summation-order rule of test_two_channel_heads_run_the_direct_kernels."""
    from unsupervised_detection_amd import ops
    g, d = geometry(case), operands(case)
    xr = x_nhwc(case)[..., X_COFF:X_COFF + g["cin"]].contiguous().cuda()  # (no gap in these cases: the real channels lead the window)
    assert g["k_gap"] == 0
    if g["tr"]:
        direct = ops.conv2d_transpose4x4s2(xr, d["w"].cuda(), d["bias"].cuda()).cpu()
    else:
        direct = ops.conv2d(xr, d["w"].cuda(), d["bias"].cuda(), 1, 1, "none", 0.0, False).cpu()
    assert (lib.udet_debug_last_conv() & 0xff) == 8
    direct = direct.reshape(-1, 2)
    y, _ = launch(devel, case, 0, WINDOWS[0])
    err, bound = float((y - direct).abs().max()), 2e-5 * max(1.0, float(direct.abs().max()))
    print("%s: %.2e against the direct kernel (bound %.2e)" % (case, err, bound))
    assert err < bound


@pytest.mark.parametrize("family", ["unforced", "self_staging"])
@pytest.mark.parametrize("case", FP16_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_head_fp16_against_rounded_operands(devel, lib, case, family):
    """fp16 mode (every head of a plan takes this form then): the GEMM multiplies fp16-rounded operands and accumulates in fp32, the gather
    adds in fp32 -- the rounded-operand float64 reference under the forward rule, and visibly not the unrounded one (tests/test_fp16_kernels_gpu.py)."""
    ref_r, ref_u = reference_fp16(case)
    lib.udet_debug_conv_fp16(1)
    if family != "unforced":
        lib.udet_debug_force_conv(*FAMILIES[family])
    runs = four_launches(devel, case, f16=True)
    for key, (y, word) in runs.items():
        assert_family(word, family, f16=True)
        check_fp16("forward", y, ref_r, ref_u, 1e-4)
    assert_bit_identical(runs)
