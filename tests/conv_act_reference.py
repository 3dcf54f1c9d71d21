"""fp64 reference and derived per-element error bounds for the forward-only entry points of csrc/conv.hip: ia_conv3x3_padded_fwd_act and
ia_conv3x3_s2_padded_fwd_act (the direct kernels whose epilogue stores bf16(silu(acc + bias) * act_scale)) and ia_silu_gap_fwd
(pooled = scale * mean over HW of silu(x), fp32).  Host only; it rests on tests/conv_reference.py (layouts, operands, the convolution in
fp64) and adds what the epilogue adds.

The references
    act_reference:  silu(conv_reference.reference(s, ops)["y"]) * scale           silu(z) = z / (1 + exp(-z)), all in fp64
    gap_reference:  scale * mean over HW of silu(x), fp64

The bars, derived from the number formats and the operation counts, never fitted to a result (U = 2^-23, BF16_STORE = 2^-8 as in
gemm_reference.py: U is what one fp32 rounding or a one-ulp hardware function may cost relative to its result).

act_bar, per element, with z = acc + bias (the fp64 value) and K = 9 * ci:
  1. z itself is off by at most the existing y bar WITHOUT its store term -- the kernel never rounds z to bf16:
         e_z = (K + 2) * U * (|x| (*) |w|) + U * (|acc| + |bias|)
     and reaches the output through silu, whose slope is bounded: |silu'| <= 1.0999 (its maximum, at z = 2.3994), so  1.1 * e_z * |scale|.
  2. the kernel evaluates silu(z) * scale as  z * v_rcp_f32(1 + v_exp_f32(z * (-log2 e))) * scale  (csrc/conv.hip dconv::epi): the two
     hardware transcendentals V_EXP_F32 (2^x) and V_RCP_F32, each documented at 1 ulp, and four fp32 roundings (the product in front of
     the exponential, the add, the two multiplies behind the reciprocal).  The exponential's ARGUMENT carries two roundings (the constant
     log2 e and the product): relative 2 U of t = -z log2 e, i.e. an absolute 2 U |t|, which 2^t turns into a relative 2 U |t| ln 2 =
     2 U |z|.  Every relative error of e = 2^t enters 1 / (1 + e) damped by e / (1 + e) <= 1; left undamped the sum is
         (1 [v_exp] + 2 |z| [its argument] + 1 [add] + 1 [v_rcp] + 2 [multiplies]) * U * |silu(z)| * |scale| = (5 + 2 |z|) * U * |ref|
  3. one bf16 store: BF16_STORE * (|ref| + the above).
The host file shows the two terms that carry weight: a kernel that takes SiLU AFTER a bf16 store of z (the two-pass form's rounding) is
outside this bar, and so is one that drops act_scale.

gap_bar, per (b, c), n = HW terms s_i = silu(x_i) of bf16 inputs x_i:
  each term is evaluated as  x / (1 + __expf(-x))  (v_exp_f32 behind a product with log2 e, an add, an IEEE division): (4 + 2 |x_i|) U |s_i|
  by the count above (the division replaces v_rcp and one multiply); the fp32 sum of n terms in ANY order -- the slices of HW, the row
  lanes folded through LDS and the fold of the slices re-order one sum -- is the accumulator rule (n + 2) * U * sum |s_i|; scale / HW is
  rounded once on the host and multiplied once: 2 U more.  So
         gap_bar = (|scale| / n) * ((n + 4) * U * sum |s_i| + sum (4 + 2 |x_i|) * U * |s_i|)
"""
import math

import torch

import conv_reference as R
from conv_reference import BF16_STORE, F64, U

SILU_SLOPE = 1.1            # >= max |silu'| = 1.09984 (at z = +-2.3994: silu'(z) = s + z s (1 - s), s = sigmoid(z))
LOG2E = 1.4426950408889634


def silu64(z):
    z = z.to(F64)
    return z / (1.0 + torch.exp(-z))


def act_reference(s, ops, scale):
    """fp64 of what ia_conv3x3[_s2]_padded_fwd_act stores, compact [B, Ho, Wo, Cout]"""
    return silu64(R.reference(s, ops)["y"]) * scale


def act_bar(s, ops, scale):
    """per-element bound of |got - act_reference| (module text)"""
    ref = R.reference(s, ops)
    x, what, bias = (R.d(ops[k]).abs() for k in ("x", "what", "bias"))
    ci = s.C // s.groups
    Sy = R._conv(s, x, what, R.d(ops["dy"]).abs())[0]
    z = ref["y"]
    e_z = (9 * ci + 2) * U * Sy + U * ((z - R.d(ops["bias"])).abs() + bias)
    out = silu64(z) * scale
    e = SILU_SLOPE * e_z * abs(scale) + (5 + 2 * z.abs()) * U * out.abs()
    return e + BF16_STORE * (out.abs() + e)


def gap_reference(x, scale):
    """x [B, HW, C] (bf16 values) -> fp64 [B, C]"""
    return silu64(x).mean(1) * scale


def gap_bar(x, scale):
    x = x.to(F64)
    n = x.shape[1]
    s = silu64(x).abs()
    return (abs(scale) / n) * ((n + 4) * U * s.sum(1) + ((4 + 2 * x.abs()) * U * s).sum(1))


# ------------------------------------------------------------------------------------------------ CPU models of the kernels' rounding
def _acc32(s, ops):
    """the convolution with fp32 accumulation (torch's order, one of the orders the accumulator rule covers) + the fp32 bias add"""
    f = lambda t: t.to(torch.float32)
    y = R._conv(s, f(ops["x"]), f(ops["what"]), f(ops["dy"]))[0]
    return y + f(ops["bias"])


def _silu32(z, scale):
    """dconv::epi in fp32, operation by operation (torch.exp2 and the reciprocal are correctly rounded here, inside the hardware's 1 ulp)"""
    t = z * torch.tensor(-LOG2E, dtype=torch.float32)
    return z * (1.0 / (1.0 + torch.exp2(t))) * torch.tensor(scale, dtype=torch.float32)


def model_act(s, ops, scale, fault=None):
    """what the kernel stores, as fp64 of a bf16 number.  fault "silu_after_store": z is rounded to bf16 first (the two-pass form);
    "scale_dropped": act_scale is not applied"""
    z = _acc32(s, ops)
    if fault == "silu_after_store":
        z = z.to(torch.bfloat16).to(torch.float32)
    y = _silu32(z, 1.0 if fault == "scale_dropped" else scale)
    return y.to(torch.bfloat16).to(F64)


def model_gap(x, scale, nsplit=1):
    """ia_silu_gap_fwd in fp32: per-slice partial sums, folded, times fl(scale / HW)"""
    x32 = x.to(torch.float32)
    n = x32.shape[1]
    s = x32 / (1.0 + torch.exp(-x32))
    per = (n + nsplit - 1) // nsplit
    part = torch.stack([s[:, i * per:(i + 1) * per].sum(1) for i in range(nsplit) if i * per < n])
    tot = part[0].clone()
    for p in part[1:]:
        tot = tot + p
    return (tot * torch.tensor(scale / n, dtype=torch.float32)).to(F64)


def gap_input(g, B, HW, C, device="cpu"):
    """randn * 2 rounded to bf16: SiLU's curved part and both tails"""
    return (torch.randn((B, HW, C), generator=g, device=g.device) * 2.0).to(torch.bfloat16).to(torch.float32).to(device)


assert math.isclose(LOG2E, 1.0 / math.log(2.0))
