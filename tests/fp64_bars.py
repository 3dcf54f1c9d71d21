"""The per-element bars shared by the fp64 kernel suites (tests/test_glue_kernels_gpu.py, tests/test_norm_kernels_gpu.py):

  * pure data movement is bit-exact against torch's own fp32 -> bf16 conversion of the reference (`bits`);
  * a bf16 output of fp32 arithmetic obeys, element by element, |got - want| <= 2^-8 |want| + a (`bf16_close`): one bf16 ulp -- half
    for the rounding, half for the fp32 arithmetic in front of it -- plus `a`, an fp32 bound for cancellation near zero;
  * an fp32 output that is a sum obeys, element by element, |got - want| <= c 2^-24 S (`sum_close`): S = the fp64 sum of the absolute
    values of the terms, c = the longest sequential chain of roundings in that kernel, read off the kernel and stated beside each use.

Where the bound is zero the output has to be exactly zero.  Every helper prints the largest error it saw as a fraction of its bound
(`-s` shows them); that figure is recorded, never used to set a bound.
"""
import torch

import glue_reference as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U24, ULP16 = R.U24, R.BF16_ULP
TINY = 2.0 ** -125            # results below the fp32 normal range may be flushed


def _ratio(name, err, bound):
    assert torch.isfinite(err).all(), (name, "non-finite output")
    exact = bound == 0
    assert (err[exact] == 0).all(), (name, "an element whose bound is zero is not exact", float(err[exact].max()))
    r = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"[glue] {name}: max error / bound = {r:.3f}")
    return r


def bits(name, got, want):
    """got (device tensor) equals want bit for bit; want is fp64 (converted the way torch converts) or already got's dtype."""
    got = got.detach().cpu()
    want = want.to(F32).to(got.dtype) if want.dtype == F64 else want.cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    iv = {BF16: torch.int16, F32: torch.int32}[got.dtype]
    same = got.contiguous().view(iv) == want.contiguous().view(iv)
    assert same.all(), (name, int((~same).sum()), "elements differ in their bits")


def bf16_close(name, got, want, a):
    got, want = got.detach().cpu().to(F64), want.to(F64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    a = a if torch.is_tensor(a) else torch.full_like(want, float(a))
    r = _ratio(name, (got - want).abs(), ULP16 * want.abs() + a.expand_as(want))
    assert r <= 1.0, (name, r)


def sum_close(name, got, want, S, c):
    got, want = got.detach().cpu().to(F64), want.to(F64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    r = _ratio(name, (got - want).abs(), c * U24 * S.to(F64).expand_as(want))
    assert r <= 1.0, (name, r, "c =", c)
