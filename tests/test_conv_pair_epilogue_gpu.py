"""Pair launches (two convolutions of the same geometry in ONE grid: launch_conv_pair -> conv_igemm_dma_pair_kernel and, for K slices,
conv_splitk_epilogue4_pair_kernel) with everything a step plan's couples carry, launch by launch, through udet_debug_conv2d_pair_ex
(include/udet_debug.h): per-problem channel windows, batches and epilogue options, on EVERY tile x ring of the pair kernel and with K
slices -- udet_debug_force_conv pins a pair's tile, ring and split count while udet_debug_force_pair(1) is set.

The problems, option sets, buffers (sentinel fill, guard rows) and checks are those of test_conv_epilogue_gpu.py; the two problems of a couple
are seeded apart (Prob.seed), so an operand or an option taken from the other problem's block changes values.  Per pair launch, for EACH
problem:
  * against oracle/oracle_conv_ex.py in float64, relative to max(1, max|ref|): 1e-4 forward, 2e-4 backward-data and for the emitted u;
  * against the plain pair run v0 -- the same forced configuration as a pair, dense outputs, no options -- bit for bit:  y2 == v0;
    act = none: y == (v0 + res) + old;  u == y * act'(ua);  the sentinel outside the windows;  with an activation in front of the residual
    2 ulp (the contraction's last bit, see test_conv_epilogue_gpu.py);
  * pair == apart, bit for bit, for a forced split count of 1 and 3: each problem alone through udet_debug_conv2d_ex on the same tile and
    ring with the second-launch summation (bit 20).  The kernel body, the tile, the K-slice boundaries and the per-element slab order of
    the quad second pass are the same.  (From 4 slices on the single launch sums with 4 or 16 lanes per element in interleaved order:
    there only the tolerance and the differential hold.)
  * what ran: udet_debug_last_pair() == 1 and udet_debug_last_conv with bit 30, the forced tile, family 2 / 4 and the split count that ran.
Couples the pair launcher declines must report last_pair == 0 and hold the same values."""
import math
from dataclasses import replace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_conv_ex as X  # noqa: E402
from oracle.oracle_glue import ACT_ELU, ACT_LEAKY, SENTINEL  # noqa: E402
from test_conv_epilogue_gpu import (D_ELU, D_LEAKY, GUARD, PLAIN_OF, UD, US, Opt, Prob, S, check, devel, device_fields, launch,  # noqa: E402,F401
                                    operands, word)
from test_ops_gpu import _tune_file_lines  # noqa: E402

GEMM_TILES = [(256, 32), (128, 32), (128, 64), (64, 64), (128, 96), (128, 128)]   # UDET_GEMM_TILES: the pair kernel exists for each, x 2 rings
RING = {2: (1 << 17, 2), 3: (1 << 22, 4)}   # stages: (family bit of udet_debug_force_conv, family of udet_debug_last_conv)
SECOND_LAUNCH = 1 << 20                     # the single launches' split-K summation by a second launch; a pair has no other
WORST = {}                                  # group -> worst deviation from float64 seen, printed per test


def forced(bm, bn, ring, ks):
    """the same word for the pair and for each problem alone"""
    return (bm + RING[ring][0] + SECOND_LAUNCH, bn, ks)


def capacity(p: Prob):
    """pair_max_ksplit / max_ksplit of these small problems (the 8 Mi float scratch never binds): half the 32-wide K stages of the class
    with the most taps"""
    taps = p.k * p.k
    if p.form == X.DGRAD and p.stride == 2:
        taps = math.ceil(p.k / 2) ** 2
    return max(1, min(64, math.ceil(taps * p.K / 32) // 2))


@pytest.fixture
def hooks(devel):
    """every process-global hook these tests touch, restored whatever happens"""
    dbg = devel.dbg
    yield dbg
    dbg.udet_debug_set_tuning(0)
    dbg.udet_debug_force_conv(0, 0, -1)
    dbg.udet_debug_force_pair(-1)
    dbg.udet_debug_conv_fp16_grad_scale(0.0)
    dbg.udet_debug_conv_fp16(0)


_ws = {}


def pair_launch(devel, pa, oa, pb, ob, one_slab=False):
    """one udet_debug_conv2d_pair_ex call -> (outputs of a, outputs of b, configuration word, last_pair).  one_slab: problem b writes its
    window of problem a's y buffer; each problem's copy of the slab then has the OTHER window put back to the sentinel, so that check()
    holds every element of the slab through one problem or the other"""
    (ga, fa), (gb, fb) = device_fields(pa, oa), device_fields(pb, ob)
    if one_slab:
        assert ga["y"].shape == gb["y"].shape and not oa.accumulate and not ob.accumulate
        assert oa.y[0] + pa.cols <= ob.y[0] or ob.y[0] + pb.cols <= oa.y[0], "the windows overlap"
        fb["y"] = fa["y"]
    need = devel.conv2d_pair_ex_workspace_bytes(fa, fb)
    if _ws.get("n", 0) < need:
        _ws["t"], _ws["n"] = torch.empty(need // 4, device="cuda"), need
    devel.conv2d_pair_ex(fa, fb, workspace=_ws["t"])
    torch.cuda.synchronize()
    v, paired = devel.dbg.udet_debug_last_conv(), devel.dbg.udet_debug_last_pair()
    outs = [{k: g[k].cpu() for k in ("y", "y2", "uo") if k in g} for g in (ga, gb)]
    if one_slab:
        slab = outs[0]["y"]
        assert torch.equal(gb["y"].cpu(), operands(pb, ob)["y"]), "problem b's own buffer was written"
        for i, (p, o) in enumerate(((pb, ob), (pa, oa))):   # outs[i] loses the window of the OTHER problem (p, o)
            mine = slab.clone()
            rows = operands(p, o)["rows"]
            win = mine[GUARD:GUARD + rows, o.y[0]:o.y[0] + p.cols]
            assert bool((win != SENTINEL).all()), "a window of the slab was not written"
            win.fill_(SENTINEL)
            outs[i]["y"] = mine
    return outs[0], outs[1], v, paired


def expect_cfg(bm, ring, ks):
    def f(v):
        w = word(v)
        assert (v >> 30) & 1 == 1 and (w["fam"], w["bm"], w["ks"], w["fold"], w["tail"]) == (RING[ring][1], bm, ks, 0, 0), (hex(v), w)
    return f


def expect_heuristic(v):
    assert (v >> 30) & 1 == 1 and word(v)["fam"] == 2, hex(v)   # pair_heuristic: always the 2-stage ring


def run_pair(devel, group, pa, pb, couples, force=None, expect=expect_heuristic, paired=1, alone=False, one_slab=False, force_pair=1):
    """the plain pair run of every couple of option sets, then the couple itself, all on one forced configuration; alone: each problem
    once more through udet_debug_conv2d_ex on the same forced word, bit for bit"""
    dbg = devel.dbg
    dbg.udet_debug_force_pair(force_pair)
    if force is not None:
        dbg.udet_debug_force_conv(*force)
    v0, ran, worst = {}, [], 0.0
    body = lambda got, p, o: got["y"][GUARD:GUARD + operands(p, o)["rows"]]  # noqa: E731
    for oa, ob in couples:
        key = (PLAIN_OF(oa), PLAIN_OF(ob))
        if key not in v0:
            ga, gb, v, pr = pair_launch(devel, pa, key[0], pb, key[1])
            ran.append((v, pr))
            worst = max(worst, check(pa, key[0], ga, None), check(pb, key[1], gb, None))
            v0[key] = (body(ga, pa, key[0]), body(gb, pb, key[1]))
        ga, gb, v, pr = pair_launch(devel, pa, oa, pb, ob, one_slab)
        ran.append((v, pr))
        worst = max(worst, check(pa, oa, ga, v0[key][0]), check(pb, ob, gb, v0[key][1]))
        if alone:
            for p, o, g in ((pa, oa, ga), (pb, ob, gb)):
                single = launch(devel, p, o)
                ws, wp = word(single["word"]), word(v)
                assert (single["word"] >> 30) & 1 == 0 and (ws["fam"], ws["bm"], ws["ks"], ws["fold"]) == (wp["fam"], wp["bm"], wp["ks"], 0), (ws, wp)
                for k in ("y", "y2", "uo"):
                    if k in g:
                        assert torch.equal(g[k], single[k]), (o.name, k, "pair != alone", int((g[k] != single[k]).sum()))
    for v, pr in ran:
        assert pr == paired, ("udet_debug_last_pair", pr, hex(v))
        if expect:
            expect(v)
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("pair group %-12s worst y deviation %.2e of the scale (this test %.2e)" % (group, WORST[group], worst))
    return ran


# ---- every tile x ring x {1, 3} slices -----------------------------------------------------------------------------------------------------------
# 13 x 9, batches 3 and 1: 351 and 117 rows -- every BM leaves a ragged last M tile in both problems and problem 1 starts at a non-zero
# x-block; 72 columns: a ragged last N block at every BN; forward 18 K stages (capacity 9), backward-data 21 (capacity 10)
SW_F = (Prob(X.FWD, 3, 13, 9, 64, 72), Prob(X.FWD, 1, 13, 9, 64, 72, x_coff=4, x_pad=12, seed=1))
SW_D = (Prob(X.DGRAD, 3, 13, 9, 64, 72), Prob(X.DGRAD, 1, 13, 9, 64, 72, x_coff=4, x_pad=12, seed=1))   # kc = 72, 64 columns
S_B = replace(S, name="S-b", y=(4, 12), y2=(8, 0), res=(0, 8))                     # problem 1: every window elsewhere
D_B = replace(D_LEAKY, name="D-leaky-b", y=(16, 4), res=(8, 0), u=(8, 4), ua=(4, 12))
assert capacity(SW_F[0]) == 9 and capacity(SW_D[0]) == 10


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("ring", [2, 3])
@pytest.mark.parametrize("bm,bn", GEMM_TILES)
@pytest.mark.parametrize("direction", ["fwd-S", "dgrad-D"])
def test_every_pair_kernel(devel, hooks, direction, bm, bn, ring, ks):
    pa, pb = SW_F if direction == "fwd-S" else SW_D
    couples = [(S, S_B)] if direction == "fwd-S" else [(D_LEAKY, D_B)]
    run_pair(devel, "tiles", pa, pb, couples, forced(bm, bn, ring, ks), expect_cfg(bm, ring, ks), alone=True)


@pytest.mark.parametrize("ring", [2, 3])
@pytest.mark.parametrize("bm,bn", [(64, 64), (128, 128)])
def test_eight_slices(devel, hooks, bm, bn, ring):
    """ks >= 4: the single launch's second pass sums in lane-interleaved order, so no pair == alone here"""
    run_pair(devel, "tiles", *SW_F, [(S, S_B)], forced(bm, bn, ring, 8), expect_cfg(bm, ring, 8))
    run_pair(devel, "tiles", *SW_D, [(D_LEAKY, D_B)], forced(bm, bn, ring, 8), expect_cfg(bm, ring, 8))


def test_a_forced_split_count_beyond_the_capacity_runs_clamped_and_says_so(devel, hooks):
    run_pair(devel, "tiles", *SW_F, [(S, S_B)], forced(128, 64, 2, 200), expect_cfg(128, 2, capacity(SW_F[0])))
    run_pair(devel, "tiles", *SW_D, [(D_LEAKY, D_B)], forced(64, 64, 3, 200), expect_cfg(64, 3, capacity(SW_D[0])))


# ---- the recover encoders' own couples -----------------------------------------------------------------------------------------------------------
# image encoder on the B images beside the flow encoder on the 3B samples; the windows as the plan lays them out: the two problems at different
# offsets of rows wider than the window.  name: (k, stride, cin of a, cin of b, cout, h, w, backward too)
ENCODERS = {"conv1": (7, 2, 3, 4, 16, 12, 20, False), "conv2": (5, 2, 16, 16, 32, 12, 20, True), "conv3": (5, 2, 32, 32, 64, 6, 10, True),
            "conv31": (3, 1, 64, 64, 64, 6, 10, True), "conv4": (3, 2, 64, 64, 128, 6, 10, True), "conv41": (3, 1, 128, 128, 128, 3, 5, True)}
ENC_F = (Opt("enc-a", bias=True, act=ACT_LEAKY, alpha=0.2, y=(0, 24)), Opt("enc-b", bias=True, act=ACT_LEAKY, alpha=0.2, y=(24, 8)))
ENC_D = (replace(D_LEAKY, name="encD-a", res=None, y=(0, 16), urange=(0, 0), u=(0, 8), ua=(8, 0)),
         replace(D_LEAKY, name="encD-b", res=None, y=(16, 0), urange=(0, 0), u=(8, 0), ua=(0, 8)))
ENC_RUNS = [(name, d) for name, e in ENCODERS.items() for d in (["fwd", "dgrad"] if e[7] else ["fwd"])]


def encoder_couple(name, direction):
    k, s, ca, cb, cout, h, w, _ = ENCODERS[name]
    if direction == "fwd":
        kc = max(ca, cb) if ca != cb else 0   # conv1: 3 and 4 input channels, both K extents 4
        return (Prob(X.FWD, 1, h, w, ca, cout, k, s, x_coff=0, x_pad=4, kc=kc), Prob(X.FWD, 3, h, w, cb, cout, k, s, x_coff=4, x_pad=0, kc=kc, seed=1))
    return (Prob(X.DGRAD, 1, h, w, ca, cout, k, s, x_coff=0, x_pad=8), Prob(X.DGRAD, 3, h, w, cb, cout, k, s, x_coff=8, x_pad=0, seed=1))


@pytest.mark.parametrize("cfg", ["heuristic", "ring3"])
@pytest.mark.parametrize("name,direction", ENC_RUNS)
def test_encoder_couples(devel, hooks, name, direction, cfg):
    """conv2 / conv3 / conv4 backward: stride 2 on an even grid, four merged parity classes in a pair launch; conv41: 15 and 45 rows, the
    heuristic cuts K in slices, which go through the pair second pass"""
    pa, pb = encoder_couple(name, direction)
    couples = [ENC_F if direction == "fwd" else ENC_D]
    if cfg == "heuristic":
        ran = run_pair(devel, "encoders", pa, pb, couples)
        if name == "conv41":
            assert all(word(v)["ks"] > 1 for v, _ in ran), [hex(v) for v, _ in ran]
    else:
        assert capacity(pa) >= 2
        run_pair(devel, "encoders", pa, pb, couples, forced(128, 64, 3, 2), expect_cfg(128, 3, 2), alone=True)


# ---- asymmetric options: an option read from the wrong problem's block -----------------------------------------------------------------------------
P_S = Opt("P", bias=True, act=ACT_ELU, y=(8, 8))                                       # S's bias and activation, no other option
S_NORES = replace(S, name="S-nores", res=None)
F_LEAKY = Opt("F-leaky", bias=True, act=ACT_LEAKY, alpha=0.2, res=(4, 4))
F_NONE = Opt("F-none", bias=True, res=(4, 4))
ASYM_F = [(S, replace(P_S, y=(4, 12))), (P_S, S_B), (S_NORES, S_B), (S, replace(S_B, res=None)), (F_LEAKY, replace(F_NONE, y=(4, 12))),
          (F_NONE, replace(F_LEAKY, y=(4, 12)))]
ACC = Opt("acc", res=(4, 4), accumulate=1)
NOACC = Opt("noacc", res=(4, 4))
NOEMIT = replace(D_LEAKY, name="D-noemit", uact=-1)
ASYM_D = [(ACC, replace(NOACC, y=(16, 4))), (NOACC, replace(ACC, y=(16, 4))), (D_LEAKY, replace(NOEMIT, y=(16, 4))), (NOEMIT, D_B),
          (replace(D_LEAKY, urange=(0, 0)), replace(D_B, urange=(8, 40))), (D_ELU, D_B)]


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("bm,bn,ring", [(128, 64, 2), (64, 64, 3)])
@pytest.mark.parametrize("batches", ["3+1", "1+3"])
@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_asymmetric_options(devel, hooks, direction, batches, bm, bn, ring, ks):
    """(S, plain) and (plain, S); res, accumulate, the emission on one side only; emissions over different column ranges and with
    different activations; leaky 0.2 beside no activation; the larger batch first and second"""
    pa, pb = SW_F if direction == "fwd" else SW_D
    if batches == "1+3":
        pa, pb = replace(pa, n=1), replace(pb, n=3)
    run_pair(devel, "asymmetric", pa, pb, ASYM_F if direction == "fwd" else ASYM_D, forced(bm, bn, ring, ks), expect_cfg(bm, ring, ks), alone=True)


# ---- unaligned twins ---------------------------------------------------------------------------------------------------------------------------------
SW_F98 = tuple(replace(p, cout=98) for p in SW_F)   # 98 columns: ldp = 100, no whole quads -- the scalar store paths, second pass included
US_B = replace(US, name="US-b", y=(4, 4), res=(6, 2))


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("bm,bn,ring", [(128, 128, 2), (64, 64, 3)])
def test_unaligned_twins(devel, hooks, bm, bn, ring, ks):
    run_pair(devel, "unaligned", *SW_F98, [(US, US_B), (S, S_B)], forced(bm, bn, ring, ks), expect_cfg(bm, ring, ks), alone=True)
    run_pair(devel, "unaligned", *SW_F, [(US, US_B)], forced(bm, bn, ring, ks), expect_cfg(bm, ring, ks), alone=True)
    run_pair(devel, "unaligned", *SW_D, [(UD, replace(D_B, ua_shift=1))], forced(bm, bn, ring, ks), expect_cfg(bm, ring, ks), alone=True)


# ---- different grids, one slab -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["heuristic", "ring3"])
def test_different_grids_go_out_as_one_launch(devel, hooks, cfg):
    """pair_compatible compares the taps, not the grids: 13 x 9 beside 6 x 10 (stride 1: the same SAME padding)"""
    pa, pb = Prob(X.FWD, 1, 13, 9, 64, 72), Prob(X.FWD, 2, 6, 10, 64, 72, x_coff=4, x_pad=12, seed=1)
    da, db = replace(pa, form=X.DGRAD), replace(pb, form=X.DGRAD)
    force, expect = (None, expect_heuristic) if cfg == "heuristic" else (forced(64, 64, 3, 3), expect_cfg(64, 3, 3))
    run_pair(devel, "grids", pa, pb, [(S, S_B)], force, expect, alone=force is not None)
    run_pair(devel, "grids", da, db, [(D_LEAKY, D_B)], force, expect, alone=force is not None)


@pytest.mark.parametrize("cfg", ["heuristic", "ring3"])
def test_two_windows_of_one_slab(devel, hooks, cfg):
    """na == nb: both problems write disjoint column windows of the SAME buffer, as the encoders do in concat_k; each window holds its
    result, the rest of the slab the sentinel"""
    pa, pb = Prob(X.FWD, 2, 6, 10, 64, 64), Prob(X.FWD, 2, 6, 10, 64, 64, x_coff=4, x_pad=12, seed=1)
    oa = Opt("slab-a", bias=True, act=ACT_LEAKY, alpha=0.2, y=(8, 80))     # [8, 72) of 152
    ob = Opt("slab-b", bias=True, act=ACT_LEAKY, alpha=0.2, y=(80, 8))     # [80, 144) of 152
    force, expect = (None, expect_heuristic) if cfg == "heuristic" else (forced(64, 64, 3, 3), expect_cfg(64, 3, 3))
    run_pair(devel, "one-slab", pa, pb, [(oa, ob)], force, expect, one_slab=True)


# ---- couples that go out apart -----------------------------------------------------------------------------------------------------------------------
def expect_single(v):
    assert (v >> 30) & 1 == 0, hex(v)


def test_fallback_different_columns(devel, hooks):
    run_pair(devel, "fall-backs", SW_F[0], replace(SW_F[1], cout=40), [(S, S_B)], None, expect_single, paired=0)


@pytest.mark.parametrize("side", [0, 1, 2], ids=["xa-on-a", "xa-on-b", "xa-on-both"])
def test_fallback_act_on_load(devel, hooks, side):
    """form 1 with xa: the LDS-DMA families do not read act'(xa) on load (dma_ok)"""
    pa, pb = (replace(p, xact=ACT_LEAKY) if side in (i, 2) else p for i, p in enumerate(SW_D))
    run_pair(devel, "fall-backs", pa, pb, [(D_LEAKY, D_B)], None, expect_single, paired=0)


@pytest.mark.parametrize("direction", ["fwd-S", "dgrad-D"])
def test_fallback_fp16_mode(devel, hooks, direction):
    """against the rounded-operand reference of test_fp16_kernels_gpu.py (Prob.f16), at the fp32 bounds"""
    hooks.udet_debug_conv_fp16(1)
    hooks.udet_debug_conv_fp16_grad_scale(4096.0)
    pa, pb = (replace(p, f16=True) for p in (SW_F if direction == "fwd-S" else SW_D))

    def expect(v):
        assert (v >> 30) & 1 == 0 and word(v)["fam"] == 2, hex(v)
    run_pair(devel, "fall-backs", pa, pb, [(S, S_B)] if direction == "fwd-S" else [(D_LEAKY, D_B)], None, expect, paired=0)


@pytest.mark.parametrize("force", [None, forced(64, 64, 3, 3)], ids=["heuristic", "forced"])
def test_fallback_force_pair_off(devel, hooks, force):
    """udet_debug_force_pair(0); with a configuration forced each of the two launches runs it"""
    def expect(v):
        expect_single(v)
        if force:
            w = word(v)
            assert (w["fam"], w["bm"], w["ks"]) == (4, 64, 3), w
    run_pair(devel, "fall-backs", *SW_F, [(S, S_B)], force, expect, paired=0, force_pair=0)
    run_pair(devel, "fall-backs", *SW_D, [(D_LEAKY, D_B)], force, expect, paired=0, force_pair=0)


def test_a_forced_configuration_without_force_pair_goes_out_apart(devel, hooks):
    """(a test that pins a family for single launches is respected: launch_conv_pair)"""
    run_pair(devel, "fall-backs", *SW_F, [(S, S_B)], forced(64, 64, 3, 3), expect_single, paired=0, force_pair=-1)


# ---- the pair cache ----------------------------------------------------------------------------------------------------------------------------------
# a couple no other test launches: 32 -> 40 channels on 10 x 14, batches 1 and 3; nine K stages: capacity 4
CACHED = (Prob(X.FWD, 1, 10, 14, 32, 40), Prob(X.FWD, 3, 10, 14, 32, 40, x_coff=4, x_pad=12, seed=1))
assert capacity(CACHED[0]) == 4


def test_tuned_pair_entry_is_what_runs_and_a_loaded_one_is_validated(devel, hooks, tmp_path):
    """The pair tuner's cache entry ("p key bm bn ks family") is what the couple's next launch runs, and an entry that arrives through
    udet_tune_load is validated: an instantiated tile with family 2 / 4 as written, anything else the heuristic's configuration, the
    split count inside [1, capacity], family -1 = the two launches apart.  Every variant holds the float64 bound."""
    from unsupervised_detection_amd import _ffi
    pa, pb = CACHED

    def run(force_pair=-1):
        hooks.udet_debug_force_pair(force_pair)
        ga, gb, v, pr = pair_launch(devel, pa, S, pb, S_B)
        check(pa, S, ga, None)
        check(pb, S_B, gb, None)
        w = word(v)
        assert (v >> 30) & 1 == pr
        return pr, w["fam"], w["bm"], w["ks"]

    heuristic = run(1)   # no entry yet, tuning off: pair_heuristic
    assert heuristic[:2] == (1, 2), heuristic
    header, before = _tune_file_lines(tmp_path / "a.txt")
    try:
        hooks.udet_debug_set_tuning(1)
        run()
    finally:
        hooks.udet_debug_set_tuning(0)
    new = sorted(l for l in _tune_file_lines(tmp_path / "b.txt")[1] - before if l.startswith("p "))
    assert len(new) == 1, new
    key, bm, bn, ks, fam = (int(v) for v in new[0].split()[1:])
    try:
        ran = run()
        assert ran == ((1, fam, bm, ks) if fam >= 0 else (0,) + ran[1:]), (ran, new[0])
        assert fam < 0 or (fam in (2, 4) and (bm, bn) in GEMM_TILES and 1 <= ks <= 4), new[0]

        def load(fields):
            f = tmp_path / "load.txt"
            f.write_text(f"{header}\np {key} {fields}\n")
            assert _ffi.lib.udet_tune_load(str(f).encode()) == 1
            return run()

        assert load("128 64 1 2") == (1, 2, 128, 1)
        assert load("64 64 3 4") == (1, 4, 64, 3)
        assert load("256 32 2 4") == (1, 4, 256, 2)
        assert load("77 32 1 2") == heuristic            # no such tile
        assert load("128 64 1 5") == heuristic           # the 4-stage ring has no pair kernel
        assert load("128 64 1 1") == heuristic           # nor has the register-staged family
        assert load("128 64 0 2") == (1, 2, 128, 1)      # ks = 0 runs as 1
        assert load("128 64 64 4") == (1, 4, 128, 4)     # clamped to the capacity
        assert load("128 64 1 -1")[0] == 0               # "faster apart"
        assert run(1) == heuristic                        # ... unless a test pairs whatever the tuner thinks
    finally:
        f = tmp_path / "restore.txt"
        f.write_text(f"{header}\n{new[0]}\n")
        _ffi.lib.udet_tune_load(str(f).encode())
