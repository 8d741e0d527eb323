"""CPU: the segment / tap tables of the recover decoder's low-resolution up-conv form (csrc/plan_build.hip build_upb_launches, read through
libudet_debug's host-only udet_debug_upconv_tables) against the definition of the layer.

The layer is `legacy bilinear x2, then 4x4 SAME convolution` (oracle_torch.resize_bilinear_legacy + conv2d_same).  The form under test
computes it as four 3x3 convolutions over a ringed low-resolution source x^ with merged weights, 16 segments per pass.  Everything the
reference side needs is derived HERE from the definition: the resize as a 2n x n matrix U, its composition with the four SAME taps, and
the merged weights read off that composition -- nothing is copied from UPB_MERGE (csrc/conv_host.hip).  The tables then have to
reproduce resize + conv (forward) and its autograd gradient (backward-data) to 1e-12 in float64, for every grid in {2..7}^2, (4, 8), (12, 20).

tests/test_upconv_lowres_gpu.py imports the helpers of this file (ring, merged weights, the float64 reference)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_torch as O

GRIDS = [(h, w) for h in range(2, 8) for w in range(2, 8)] + [(4, 8), (12, 20)]


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def resize_matrix(n):
    """legacy bilinear x2 along one axis as a 2n x n matrix: out[2j] = x[j], out[2j+1] = (x[j] + x[min(j+1, n-1)]) / 2"""
    U = np.zeros((2 * n, n))
    for j in range(n):
        U[2 * j, j] += 1.0
        U[2 * j + 1, j] += 0.5
        U[2 * j + 1, min(j + 1, n - 1)] += 0.5
    return U


def composed(n):
    """A[k][o, j]: coefficient of x[j] in what tap k of the 4-tap SAME convolution (padding 1 before, 2 after) reads for output o"""
    U = resize_matrix(n)
    A = np.zeros((4, 2 * n, n))
    for k in range(4):
        for o in range(2 * n):
            i = o - 1 + k
            if 0 <= i < 2 * n:
                A[k, o] = U[i]
    return A


@functools.lru_cache(maxsize=1)
def merge_matrices():
    """M[parity p][variant v: 0 interior, 1 last low-resolution row][merged tap a][4x4 tap k], read off the composition on n = 8:
    output o = 2q + p is sum_a (sum_k M[a][k] w[k]) x^[q + p + a] with x^[R] = +-x[clamp(R - 1)] (ring coordinates).  Interior (q = 3):
    the three ring rows read three distinct pixels, M[a][k] = A[k][o, q + p + a - 1].  Last (q = n - 1): ring rows past R = n + 1 do
    not exist and rows n, n + 1 read the same pixel; the first ring row that reads a pixel carries its coefficient, the others none."""
    n = 8
    A = composed(n)
    M = np.zeros((2, 2, 3, 4))
    for p in range(2):
        for v, q in ((0, 3), (1, n - 1)):
            o, seen, covered = 2 * q + p, set(), np.zeros((4, n))
            for a in range(3):
                R = q + p + a
                j = min(R - 1, n - 1)
                if R > n + 1 or j in seen:
                    continue
                seen.add(j)
                M[p, v, a] = A[:, o, j]
                covered[:, j] = A[:, o, j]
            assert np.array_equal(covered, A[:, o]), "the ring rows of this output do not cover what it reads"
    return M


def merged_weights(w):
    """w HWIO [4,4,cin,cout] (float64 tensor) -> [144 = set * 36 + class * 9 + 3 a + b][cin][cout], set = (last row) + 2 (last column),
    class = 2 py + px: W~ = sum_kl My[a][k] Mx[b][l] w[k][l] (the layer is separable in rows and columns)"""
    M = torch.from_numpy(merge_matrices())
    out = []
    for s in range(4):
        for c in range(4):
            out.append(torch.einsum("ak,bl,klio->abio", M[c >> 1, s & 1], M[c & 1, s >> 1], w).reshape(9, *w.shape[2:]))
    return torch.cat(out)


def ring_index(n):
    """ring coordinate R in [0, n + 2) -> (source index, sign): the negated edge at R = 0, the clamped edge at R = n + 1"""
    idx = np.clip(np.arange(n + 2) - 1, 0, n - 1)
    sg = np.ones(n + 2)
    sg[0] = -1.0
    return torch.from_numpy(idx), torch.from_numpy(sg)


def ring(x):
    """x [N,h,w,C] -> x^ [N,h+2,w+2,C] (any float dtype; signs are exact)"""
    iy, sy = ring_index(x.shape[1])
    ix, sx = ring_index(x.shape[2])
    s = (sy[:, None] * sx[None, :]).to(x.dtype)
    return x[:, iy][:, :, ix] * s[None, :, :, None]


def ring_fold(g):
    """the adjoint of ring: g [N,h+2,w+2,C] -> [N,h,w,C]"""
    h, w = g.shape[1] - 2, g.shape[2] - 2
    iy, sy = ring_index(h)
    ix, sx = ring_index(w)
    s = (sy[:, None] * sx[None, :]).to(g.dtype)
    t = torch.zeros(g.shape[0], h, g.shape[2], g.shape[3], dtype=g.dtype).index_add_(1, iy, g * s[None, :, :, None])
    return torch.zeros(g.shape[0], h, w, g.shape[3], dtype=g.dtype).index_add_(2, ix, t)


def layer_linear(x, w):
    """the layer without bias and activation, float64 oracle"""
    return O.conv2d_same(O.resize_bilinear_legacy(x, 2 * x.shape[1], 2 * x.shape[2]), w, None, 1, 1)


def lowres_forward(xh, wm):
    """The layer as a function of the RINGED source, stated from merge_matrices' convention alone (no table): output (2 qy + py, 2 qx + px)
    = sum_ab x^[qy + py + a, qx + px + b] W~[set][class][a][b] with set = (qy == h - 1) + 2 (qx == w - 1).  Differentiable: the GPU test
    takes its reference for the ringed gradient from it."""
    n, h, w = xh.shape[0], xh.shape[1] - 2, xh.shape[2] - 2
    xp = torch.nn.functional.pad(xh, (0, 0, 0, 1, 0, 1))  # (a = 2 of an odd last row reads one row past the ring, with weight 0)
    rows = []
    for oy in range(2 * h):
        qy, py = oy >> 1, oy & 1
        cols = []
        for px in range(2):
            for cv, (q0, q1) in enumerate(((0, w - 1), (w - 1, w))):
                s = (1 if qy == h - 1 else 0) + 2 * cv
                acc = 0
                for a in range(3):
                    for b in range(3):
                        acc = acc + xp[:, qy + py + a, q0 + px + b:q1 + px + b] @ wm[s * 36 + (2 * py + px) * 9 + 3 * a + b]
                cols.append(acc)
        even, odd = torch.cat(cols[0:2], 1), torch.cat(cols[2:4], 1)
        rows.append(torch.stack([even, odd], 2).reshape(n, 2 * w, -1))
    return torch.stack(rows, 1)


# ---- the tables applied -------------------------------------------------------------------------------------------------------------------
def apply_forward(tab, xh, wm, cover):
    n, h, w = xh.shape[0], xh.shape[1] - 2, xh.shape[2] - 2
    y = torch.zeros(n, 2 * h, 2 * w, wm.shape[2], dtype=xh.dtype)
    for s, (oy, ox, sh, sw) in enumerate(tab["seg"]):
        acc = 0
        for dy, dx, widx in tab["taps"][tab["seg_tap"][s]:tab["seg_tap"][s + 1]]:
            assert 0 <= dy and dy + sh <= h + 2 and 0 <= dx and dx + sw <= w + 2, ("forward tap outside the ringed grid", s, dy, dx)
            acc = acc + xh[:, dy:dy + sh, dx:dx + sw] @ wm[widx]
        y[:, oy:oy + 2 * sh:2, ox:ox + 2 * sw:2] = acc
        cover[oy:oy + 2 * sh:2, ox:ox + 2 * sw:2] += 1
    return y


def apply_backward(tab, du, wm, cover):
    """ringed gradient: segment pixel (qy, qx) -> x^ cell (oy + qy, ox + qx), taps read dU at (2 qy + dy, 2 qx + dx), zero outside its grid"""
    n, h, w, pad = du.shape[0], du.shape[1] // 2, du.shape[2] // 2, 8
    dup = torch.nn.functional.pad(du, (0, 0, pad, pad, pad, pad))
    g = torch.zeros(n, h + 2, w + 2, wm.shape[1], dtype=du.dtype)
    for s, (oy, ox, sh, sw) in enumerate(tab["seg"]):
        acc = 0
        for dy, dx, widx in tab["taps"][tab["seg_tap"][s]:tab["seg_tap"][s + 1]]:
            assert -pad <= dy and 2 * (sh - 1) + dy < 2 * h + pad and -pad <= dx and 2 * (sw - 1) + dx < 2 * w + pad
            acc = acc + dup[:, pad + dy:pad + dy + 2 * sh:2, pad + dx:pad + dx + 2 * sw:2] @ wm[widx].T
        g[:, oy:oy + sh, ox:ox + sw] = acc
        cover[oy:oy + sh, ox:ox + sw] += 1
    return g


def dyadic_weights(cin, cout, seed):
    """4x4 HWIO weights (float32) on a grid on which every MERGED weight is exact in fp16: multiples of 2^-6 in +-[0.25, 1] times the power
    of two nearest to the usual sqrt(2 / fan-in).  A merged weight is a sum of at most 3 x 3 such values with coefficients in {1/4, 1/2, 1}
    of total weight <= 2.5^2: a multiple of 2^-8 below 8 in units of the scale -- 11 significant bits."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(16, 65, (4, 4, cin, cout), generator=g).float() / 64.0
    sign = (torch.randint(0, 2, (4, 4, cin, cout), generator=g) * 2 - 1).float()
    return m * sign * 2.0 ** round(float(np.log2((2.0 / (16 * cin)) ** 0.5)))


def merged_exact_in_fp16(wt):
    """every merged weight of wt (float32 HWIO) is a normal fp16 number or zero, exactly"""
    wm = merged_weights(wt.double())
    return bool((wm.half().double() == wm).all()) and bool(((wm == 0) | (wm.abs() >= 2.0 ** -14)).all()) and bool(torch.isfinite(wm.half()).all())


def rnd64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.fixture(scope="module")
def tables():
    from unsupervised_detection_amd._devel import dbg, upconv_tables
    return dbg, upconv_tables


def test_resize_matrix_is_the_oracles_resize():
    for n in (2, 3, 5, 8):
        eye = torch.eye(n, dtype=torch.float64).reshape(1, n, 1, n)  # pixel j carries the one-hot channel j
        up = O.resize_bilinear_legacy(eye.expand(1, n, 2, n), 2 * n, 4)[0, :, 0]
        assert np.array_equal(up.numpy(), resize_matrix(n))


def test_merge_matrices_are_small_dyadic_sums():
    """what the fp16 test of the GPU file relies on: every merged weight is a sum of at most three 4x4 taps with coefficients 1/2 and 1"""
    M = merge_matrices()
    assert set(np.unique(M)) <= {0.0, 0.5, 1.0} and int((M != 0).sum(-1).max()) <= 3


@pytest.mark.parametrize("h,w", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_tables_reproduce_resize_and_convolution(tables, h, w):
    dbg, upconv_tables = tables
    n, cin, cout = 2, 2, 3
    x = rnd64(n, h, w, cin, seed=1).requires_grad_(True)
    wt = rnd64(4, 4, cin, cout, seed=2)
    du = rnd64(n, 2 * h, 2 * w, cout, seed=3)
    ref = layer_linear(x, wt)
    gref, = torch.autograd.grad((ref * du).sum(), [x])
    ref = ref.detach()
    wm = merged_weights(wt)
    xh = ring(x.detach())
    F, B = upconv_tables(h, w, False), upconv_tables(h, w, True)
    for tab in (F, B):
        assert 1 <= tab["nseg"] <= dbg.udet_debug_max_segs()
        st = tab["seg_tap"]
        assert st[0] == 0 and st[-1] == len(tab["taps"]) and all(a <= b for a, b in zip(st, st[1:])), st
        assert all(sh >= 1 and sw >= 1 for _, _, sh, sw in tab["seg"])
        assert all(0 <= widx < 144 for _, _, widx in tab["taps"])
    cover = torch.zeros(2 * h, 2 * w)
    y = apply_forward(F, xh, wm, cover)
    assert bool((cover == 1).all()), "forward segments do not tile the output exactly once"
    scale = max(1.0, float(ref.abs().max()))
    assert float((y - ref).abs().max()) < 1e-12 * scale
    assert float((lowres_forward(xh, wm) - ref).abs().max()) < 1e-12 * scale  # (the GPU file's statement of the same)
    cover = torch.zeros(h + 2, w + 2)
    g = apply_backward(B, du, wm, cover)
    assert bool((cover == 1).all()), "backward segments do not tile the ringed grid exactly once"
    gscale = max(1.0, float(gref.abs().max()))
    assert float((ring_fold(g) - gref).abs().max()) < 1e-12 * gscale
    xhv = xh.clone().requires_grad_(True)
    gh, = torch.autograd.grad((lowres_forward(xhv, wm) * du).sum(), [xhv])
    assert float((g - gh).abs().max()) < 1e-12 * gscale  # the ringed gradient itself, before the fold


def test_ring_fold_is_the_adjoint_of_ring():
    x, g = rnd64(2, 3, 5, 2, seed=4), rnd64(2, 5, 7, 2, seed=5)
    assert abs(float((ring(x) * g).sum() - (x * ring_fold(g)).sum())) < 1e-12


def test_table_entry_refuses_degenerate_grids(tables):
    _, upconv_tables = tables
    for h, w in ((1, 4), (4, 1), (0, 0)):
        with pytest.raises(ValueError, match="at least 2 x 2"):
            upconv_tables(h, w, False)


@pytest.mark.parametrize("cin,cout", [(24, 16), (40, 100), (386, 64)])
def test_dyadic_weights_merge_exactly_in_fp16(cin, cout):
    """the fp16 tests of tests/test_upconv_lowres_gpu.py need no model of the pack kernel's summation order: on this grid every order gives
    the same merged weight and its fp16 conversion is exact; ordinary random weights do not have the property"""
    wt = dyadic_weights(cin, cout, seed=7)
    assert float(wt.abs().min()) > 0 and merged_exact_in_fp16(wt)
    assert not merged_exact_in_fp16(torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(8)))


def test_layer_entries_check_their_arguments_before_any_device_call():
    """udet_debug_upconv_lowres_fwd / _bwd (tests/test_upconv_lowres_gpu.py drives them on the GPU): the documented error codes, on the host,
    with pointers that are never dereferenced"""
    import ctypes
    from unsupervised_detection_amd._devel import dbg
    from unsupervised_detection_amd._ffi import lib
    SHAPE, ALIGN, ARG = -1, -2, -5
    fake = 1 << 20
    need = dbg.udet_debug_upconv_lowres_workspace_bytes(16, 12, 6)
    assert need > 0 and dbg.udet_debug_upconv_lowres_workspace_bytes(0, 12, 6) == 0

    def fwd(x=fake, ldx=12, ldy=8, y_coff=0, h=4, w=4, cin=12, cout=6, split=0, act=1, ws=fake, ws_bytes=need, n=1):
        return dbg.udet_debug_upconv_lowres_fwd(x, ldx, fake, fake, act, ctypes.c_float(0.2), fake, ldy, y_coff, fake, n, h, w, cin, cout, split, ws,
                                                ws_bytes, None)

    def bwd(dy=fake, ldy=8, y_coff=0, ldx=12, h=4, w=4, cin=12, cout=6, ws=fake, ws_bytes=need):
        return dbg.udet_debug_upconv_lowres_bwd(dy, ldy, y_coff, fake, fake, ldx, fake, 1, h, w, cin, cout, ws, ws_bytes, None)
    assert fwd(h=1) == SHAPE and b"at least 2 x 2" in lib.udet_last_error()
    assert fwd(w=1) == SHAPE and bwd(h=1) == SHAPE and bwd(w=0) == SHAPE
    assert fwd(ldx=14) == ALIGN and b"multiples of 4" in lib.udet_last_error()
    assert fwd(ldy=10) == ALIGN and fwd(ldy=12, y_coff=2) == ALIGN and bwd(ldx=13) == ALIGN and bwd(ldy=12, y_coff=2) == ALIGN
    assert fwd(ldx=8) == SHAPE and b"outside the buffer" in lib.udet_last_error()       # cin = 12 channels in rows of 8
    assert fwd(ldy=8, y_coff=4) == SHAPE and fwd(ldy=4) == SHAPE                         # 4 + 6 > 8
    assert bwd(ldy=12, y_coff=8) == SHAPE and bwd(ldx=8) == SHAPE                        # the dy window is cout rounded up to 8
    assert fwd(x=None) == ARG and bwd(dy=None) == ARG and fwd(n=0) == ARG and fwd(act=7) == ARG
    assert fwd(cout=32, ldy=32, split=1) == ARG and b"split" in lib.udet_last_error()
    assert fwd(ws=None) == ARG and fwd(ws=fake + 4) == ARG and fwd(ws_bytes=need // 2) == ARG and bwd(ws_bytes=4096) == ARG
