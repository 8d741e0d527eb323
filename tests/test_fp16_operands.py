"""CPU self-check of the rounded-operand references behind the fp16 kernel tests (tests/test_fp16_kernels_gpu.py, the fp16 section of
tests/test_wgrad_gpu.py): every operand of every case, scaled gradient operands included, rounds to a normal, non-zero fp16 number -- so
no reference depends on how the hardware treats fp16 subnormals -- and the case tables name the instantiations they claim to."""
import pytest
import torch

import test_fp16_kernels_gpu as K
import test_wgrad_gpu as Wg


def test_r16_rejects_what_the_references_must_not_contain():
    for bad in (torch.tensor([0.5, 0.0]), torch.tensor([0.5, 3e-5]), torch.tensor([0.5, 1e5])):  # zero, subnormal, overflow
        with pytest.raises(AssertionError):
            K.r16(bad)
    with pytest.raises(AssertionError):
        K.r16(torch.tensor([1e-6]))          # flushed / subnormal without the scale ...
    t = torch.tensor([0.3e-6, -1e-6])
    r = K.r16(t, 4096.0)                     # ... normal with it, and the scale is undone exactly
    assert float(((r - t.double()) / t.double()).abs().max()) < 2.0 ** -11
    assert torch.equal(K.r16(torch.tensor([0.333251953125])), torch.tensor([0.333251953125], dtype=torch.float64))  # an fp16 number: exact


@pytest.mark.parametrize("c", K.ALL_LAYERS, ids=lambda c: "x".join(map(str, c[:8])))
def test_forward_and_backward_data_operands_are_normal_fp16_numbers(c):
    op = K.operands(c)  # (r16 asserts)
    assert op["x16"].shape == op["x"].shape and len(op["dy16"]) == len(K.GRAD_RUNS)
    for dy, (gs, m) in zip(op["dy"], K.GRAD_RUNS):
        assert 0.25 * m * 0.999 <= float(dy.abs().min()) and float(dy.abs().max()) <= m * 1.001
        if gs != 1.0:
            assert float(dy.abs().max()) < 2.0 ** -14  # without the scale none of them is a normal fp16 number


def test_transposed_operands_are_normal_fp16_numbers():
    r = K.transposed_reference()
    assert r["y_r"].shape == r["y_u"].shape == (2, 24, 40, 32)
    assert 1e-5 < float((r["y_r"] - r["y_u"]).abs().max()) < 2e-2  # the rounding is visible, and small


def test_rounding_moves_the_tile_case_by_about_3e_4_of_its_scale():
    """TILE_CASE on the CPU: operand rounding moves the forward result by ~3e-4 of its scale -- three orders above fp32 summation error,
    fifty times below the 2e-2 of tests/test_fp16_gpu.py"""
    r = K.reference(K.TILE_LAYER)
    e = float((r["y_r"] - r["y_u"]).abs().max()) / max(1.0, float(r["y_u"].abs().max()))
    assert 5e-5 < e < 2e-3, e
    for i, (gs, m) in enumerate(K.GRAD_RUNS):
        e = float((r["gx_r"][i] - r["gx_u"][i]).abs().max()) / max(m, float(r["gx_u"][i].abs().max()))
        assert 5e-5 < e < 2e-3, (gs, e)


def test_tile_tables():
    K.test_fp16_tile_configs_are_the_23_instantiations()
    K.test_fp16_family_list()
    K.test_fp16_tile_resident_cases_name_every_instantiation()
    Wg.test_fp16_plain_cases_reach_every_tile()


WGRAD_F16 = ([(c, mode != 0, Wg.F16_SCALE) for c, mode in Wg.PLAIN.values()] + [(Wg.PLAIN["bn64"][0], False, 1.0)]
             + [(Wg.case(1, 12, 20, 128, 64, 3, bn=True), True, Wg.F16_SCALE), (Wg.case(2, 7, 9, 64, 32, 3, bn=True), True, Wg.F16_SCALE)]
             + [(Wg.FUSED[1][0], False, Wg.F16_SCALE), (Wg.SEPARATE["swapped"], False, Wg.F16_SCALE), (Wg.case(2, 24, 48, 64, 64, 3), False, Wg.F16_SCALE)])


@pytest.mark.parametrize("c,up,f16", WGRAD_F16, ids=lambda v: "x".join(map(str, v[:8])) if isinstance(v, tuple) else str(v))
def test_filter_gradient_operands_are_normal_fp16_numbers(c, up, f16):
    ins, ref = Wg.reference(c, up, f16)  # (r16 asserts on x and on the scaled dy)
    unit = Wg.dy_unit(f16)
    assert float(ins["dy"].abs().max()) <= unit * 1.001 and float(ins["dy"].abs().min()) >= 0.25 * unit * 0.999
    if f16 != 1.0:
        assert float(ins["dy"].abs().max()) < 2.0 ** -14
    e = float((ref["dw"] - ins["alt_dw"]).abs().max()) / max(unit, float(ref["dw"].abs().max()))
    # rounded and unrounded operands give visibly different filter gradients (with act' on load -- the launches that stay fp32 -- the rounded
    # x also flips derivatives at the kink: no upper figure there)
    assert 1e-5 < e and (e < 2e-3 or c[8] != "none"), e
