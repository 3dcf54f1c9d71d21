"""tests/conv_act_reference.py on the host: a CPU model of the forward-only epilogue's rounding (fp32 accumulation, SiLU on the fp32 sum
through exp2 and a reciprocal, one bf16 store) lies inside the derived bars at every kind of shape the GPU file uses, and two injected
faults lie outside them: SiLU taken after a bf16 store of the sum (the two-pass form this epilogue replaces) and act_scale dropped.
The SiLU-mean model likewise, with one fault: the terms rounded to bf16 before they are summed (the pass the fused tail replaces)."""
import pytest
import torch

import conv_act_reference as A
import conv_reference as R

F64 = torch.float64
SHAPES = [R.conv3(2, 9, 31, 64, 64, 1), R.conv3(1, 8, 30, 16, 32, 1), R.conv3(1, 1, 1, 32, 16, 1), R.conv3(2, 9, 31, 128, 128, 2),
          R.conv3(2, 17, 61, 64, 64, 1, 2), R.conv3(2, 15, 59, 64, 128, 1, 2), R.conv3(1, 1, 1, 128, 128, 2, 2)]
SCALES = (1.0, 0.6180339887)
name = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def pool():
    return R.normal_pool(torch.Generator().manual_seed(811), n=600_000)


def test_silu_slope_bound():
    z = torch.linspace(-30, 30, 600001, dtype=F64)
    s = torch.sigmoid(z)
    assert float((s + z * s * (1 - s)).abs().max()) <= A.SILU_SLOPE


def test_reference_is_torch_silu():
    z = torch.randn(1000, dtype=F64) * 4
    assert torch.allclose(A.silu64(z), torch.nn.functional.silu(z), rtol=1e-14, atol=1e-300)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("s", SHAPES, ids=name)
def test_model_inside_the_bar(pool, s, scale):
    ops = R.normal_operands(pool, s)
    want, bar = A.act_reference(s, ops, scale), A.act_bar(s, ops, scale)
    got = A.model_act(s, ops, scale)
    assert R.first_bad_nd(got, want, bar) is None
    assert 0.5 < R.worst_ratio(got, want, bar) <= 1.0          # a correctly rounded bf16 store alone reaches most of its allowance


def test_silu_after_the_store_is_outside(pool):
    """2 x 9 x 31 x 64 -> 64: 35 712 outputs, sums of 576 products with |z| up to a few units -- where silu' is near 1 the bf16
    rounding of z alone costs what the bar allows for the one store, and the second store comes on top"""
    s = SHAPES[0]
    ops = R.normal_operands(pool, s)
    want, bar = A.act_reference(s, ops, 1.0), A.act_bar(s, ops, 1.0)
    got = A.model_act(s, ops, 1.0, fault="silu_after_store")
    assert R.first_bad_nd(got, want, bar) is not None
    assert R.worst_ratio(got, want, bar) > 1.2


@pytest.mark.parametrize("s", SHAPES[:2] + SHAPES[4:5], ids=name)
def test_dropped_scale_is_outside(pool, s):
    ops = R.normal_operands(pool, s)
    want, bar = A.act_reference(s, ops, SCALES[1]), A.act_bar(s, ops, SCALES[1])
    assert R.worst_ratio(A.model_act(s, ops, SCALES[1], fault="scale_dropped"), want, bar) > 50


@pytest.mark.parametrize("B,HW,C,nsplit", [(1, 1, 8, 1), (3, 7, 3072, 1), (2, 625, 2304, 9), (1, 169, 64, 2)])
def test_gap_model_inside_the_bar(B, HW, C, nsplit):
    x = A.gap_input(torch.Generator().manual_seed(5 + HW), B, HW, C)
    for scale in (1.0, 1.7):
        want, bar = A.gap_reference(x, scale), A.gap_bar(x, scale)
        assert R.first_bad_nd(A.model_gap(x, scale, nsplit), want, bar) is None


def test_gap_of_rounded_terms_is_outside():
    """the two-pass tail stores silu(x) as bf16 before the pool reads it: 2^-9 per term against a bar of a few 2^-23 -- at 7 terms the
    rounding errors do not average out"""
    x = A.gap_input(torch.Generator().manual_seed(12), 3, 7, 3072)
    x32 = x.to(torch.float32)
    terms = (x32 / (1 + torch.exp(-x32))).to(torch.bfloat16).to(F64)
    assert R.first_bad_nd(terms.mean(1), A.gap_reference(x, 1.0), A.gap_bar(x, 1.0)) is not None
