"""fp64 reference, exact operands and derived per-element error bounds for the dense GEMM entry points (ia_gemm_bf16,
ia_gemm_bf16_qscale).  Host only: torch fp64 (any device) and numpy; nothing here calls the library.

A form names what gemm_core's switch dispatches: operand layouts, output type, epilogue, and which optional outputs / inputs the call has.
Operands are handed around in their LOGICAL shape, A [M, K] and B [K, N], whatever their layout in memory: the layout is the caller's
business (tests/test_gemm_kernels_gpu.py), the arithmetic is the same.

The bounds (`bars`) are derived from the number formats and the operation counts, never fitted to a result:
  fp32 accumulator   (L + 2) * 2^-23 * (|A| @ |B|), L = K: the worst-case bound L * u of a length-L sum of fp32 adds in ANY order with
                     u = 2^-24, doubled because the MFMA's internal adds are not individually rounded.  Split-K and `accumulate` add
                     splits + 1 to L (the partials are added once more, and the prior once).
  fp32 epilogue op   2^-23 of the magnitudes it combines (twice the unit roundoff of one rounding)
  bf16 store         2^-8 * |ref| (the allowance of test_gemm_gelu_epilogue_accuracy: bf16 has an 8-bit significand, so half an ulp is at
                     most 2^-8 of the value), taken of |ref| + the terms above, since the value that is stored is the reference only up
                     to them
  GELU forms         the fit errors of tools/fit_gelu.py (3.0e-5 activation, 1.1e-4 derivative, x 1.2 as in that test) plus the error of
                     the pre-activation times the slope bound (|gelu'| <= 1.13, |gelu''| <= 0.8).  The error of the pre-activation has one
                     term more than the accumulator's: the header defines both forms at x = bf16(acc + bias) and `reference` follows it,
                     while the epilogues (epi_store4 / epi_store8 in csrc/gemm.hip) evaluate the polynomial at the fp32 sum -- the two
                     arguments differ by at most half a bf16 ulp, 2^-8 * |x|.  tests/test_gemm_reference_host.py shows that the model
                     needs the term (test_gelu_bar_needs_the_preactivation_rounding_term).  On exact operands x is a bf16 number, the
                     term and the accumulator term are zero, and what is left is the fit and the store.
  column / row sums  the accumulator rule with the length of the sum (M, or K) over the summed magnitudes, plus the summed bounds of
                     the terms.  The T128 path of IA_EPI_DGELU_COLSUM sums the STORED bf16 elements (ia_colsum over C), so there the
                     store term of every element is part of the sum's bound (`stored_colsum`).
"""
import math
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -23
BF16_STORE = 2.0 ** -8
GELU_FIT_ACT, GELU_FIT_DER, GELU_FIT_SLACK = 3.0e-5, 1.1e-4, 1.2
GELU_SLOPE, GELU_CURV = 1.13, 0.8

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_ADD, EPI_DGELU, EPI_BIAS_ADD, EPI_DGELU_COLSUM, EPI_BIAS_GELU_ACT = range(8)

# aks / bks: the operand is k-strided in memory; f32: fp32 output; c2: the call has a second output; acc: accumulate onto a prior C;
# q: the call goes through ia_gemm_bf16_qscale
Form = namedtuple("Form", "name aks bks f32 epi c2 acc q", defaults=(False, False, False))
NT_BF16 = [Form("nt", 0, 0, 0, EPI_NONE), Form("nt+bias", 0, 0, 0, EPI_BIAS), Form("nt+bias_gelu", 0, 0, 0, EPI_BIAS_GELU, True),
           Form("nt+bias_gelu_act", 0, 0, 0, EPI_BIAS_GELU_ACT), Form("nt+bias_add", 0, 0, 0, EPI_BIAS_ADD), Form("nt+add", 0, 0, 0, EPI_ADD),
           Form("nt*dgelu", 0, 0, 0, EPI_DGELU), Form("nt*dgelu+colsum", 0, 0, 0, EPI_DGELU_COLSUM, True),
           Form("nt+bias,qcols", 0, 0, 0, EPI_BIAS, q=True)]
NN_BF16 = [Form("nn", 0, 1, 0, EPI_NONE), Form("nn+add", 0, 1, 0, EPI_ADD), Form("nn*dgelu", 0, 1, 0, EPI_DGELU),
           Form("nn*dgelu+colsum", 0, 1, 0, EPI_DGELU_COLSUM, True)]
TN_F32 = [Form("tn_f32", 1, 1, 1, EPI_NONE), Form("tn_f32+rowsum", 1, 1, 1, EPI_NONE, True), Form("tn_f32+acc", 1, 1, 1, EPI_NONE, False, True),
          Form("tn_f32+rowsum+acc", 1, 1, 1, EPI_NONE, True, True)]
NT_F32 = [Form("nt_f32", 0, 0, 1, EPI_NONE), Form("nt_f32+bias", 0, 0, 1, EPI_BIAS)]
FORMS = {f.name: f for f in NT_BF16 + NN_BF16 + TN_F32 + NT_F32}

HAS_BIAS = (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_ACT, EPI_BIAS_ADD)
HAS_AUX = (EPI_ADD, EPI_DGELU, EPI_BIAS_ADD, EPI_DGELU_COLSUM)
GELU = (EPI_BIAS_GELU, EPI_BIAS_GELU_ACT)


def d(x):
    return None if x is None else x.to(F64)


def bf16_round(x):
    """fp64 -> the nearest bf16 number (ties to even), as fp64, in one rounding (a cast through fp32 would round twice)"""
    # on the bit pattern of |x| (integer operations only, the same on every device): bf16 keeps 7 of fp64's 52 explicit significand bits,
    # so the low 45 go, rounded to nearest with ties to the even neighbour; a carry out of the significand moves into the exponent as it
    # should.  (fp64's wider exponent does not matter at the magnitudes of these tests, far inside bf16's normal range.)
    a = x.abs().contiguous().view(torch.int64)
    a = ((a + ((1 << 44) - 1) + ((a >> 45) & 1)) >> 45) << 45
    return torch.copysign(a.view(F64), x)


def holds(x, f32):
    """does the output type hold every element of the fp64 tensor x exactly?"""
    back = x.to(torch.float32).to(F64) if f32 else bf16_round(x)
    return bool((back == x).all()) and bool(torch.isfinite(x).all())


def unheld(x, f32):
    """the first element of x its output type does not hold, for a message"""
    back = x.to(torch.float32).to(F64) if f32 else bf16_round(x)
    bad = torch.nonzero((back != x).reshape(-1))
    return None if bad.numel() == 0 else (float(x.reshape(-1)[bad[0]]), float(back.reshape(-1)[bad[0]]))


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-x * x / 2.0) / math.sqrt(2.0 * math.pi)


def reference(form, A, B, bias=None, aux=None, prior=None, qcols=0, qscale=1.0, prior2=None):
    """fp64 of every output of `form`: {"C": [M, N], "C2": ...} -- C2 is the saved derivative [M, N] (IA_EPI_BIAS_GELU), the column sums
    of C added to prior2 [N] (IA_EPI_DGELU_COLSUM) or the row sums of A added to prior2 [M] (weight-gradient form with C2).  A [M, K],
    B [K, N] logical; prior [M, N]: what C held, when the form accumulates."""
    A, B, bias, aux, prior, prior2 = d(A), d(B), d(bias), d(aux), d(prior), d(prior2)
    acc = A @ B
    out = {}
    epi = form.epi
    v = acc + bias if epi in HAS_BIAS else acc
    if epi == EPI_BIAS and qcols:
        v = torch.cat((v[:, :qcols] * qscale, v[:, qcols:]), 1)
    if epi in GELU:
        x = bf16_round(v)
        v = gelu(x)
        if epi == EPI_BIAS_GELU:
            out["C2"] = gelu_grad(x)
    if epi in (EPI_ADD, EPI_BIAS_ADD):
        v = v + aux
    if epi in (EPI_DGELU, EPI_DGELU_COLSUM):
        v = v * aux
    if epi == EPI_DGELU_COLSUM:
        out["C2"] = v.sum(0) + (prior2 if prior2 is not None else 0.0)
    if form.aks and form.bks and form.f32 and form.c2:
        out["C2"] = A.sum(1) + (prior2 if prior2 is not None else 0.0)
    if form.acc:
        v = v + prior
    out["C"] = v
    return out


def bars(form, A, B, bias=None, aux=None, K=None, prior=None, qcols=0, qscale=1.0, prior2=None, splits=1, exact=False, stored_colsum=False):
    """per-element bound of |got - reference| for every output of `form` (see the module text).  exact: the operands are
    exact_operands', so every sum is exact and only what is inexact by nature (the GELU fit, its bf16 store) is allowed anything."""
    A, B, bias, aux, prior, prior2 = d(A), d(B), d(bias), d(aux), d(prior), d(prior2)
    K = A.shape[1] if K is None else K
    M = A.shape[0]
    epi = form.epi
    ref = reference(form, A, B, bias, aux, prior, qcols, qscale, prior2)
    zero = torch.zeros_like(ref["C"])
    if exact and epi not in GELU:
        return {k: torch.zeros_like(v) for k, v in ref.items()}
    L = K + 2 + (splits + 1 if (splits > 1 or form.acc) else 0)
    acc = A @ B
    S = A.abs() @ B.abs()
    if form.acc:
        S = S + prior.abs()
    e = zero if exact else L * U * S                      # the error of the value so far, v its magnitude
    v = acc
    if epi in HAS_BIAS:
        e = e + U * (v.abs() + bias.abs())
        v = v + bias
    if epi == EPI_BIAS and qcols:
        sc = torch.ones(v.shape[1], dtype=F64, device=v.device)
        sc[:qcols] = abs(qscale)
        e = e * sc + U * (v * sc).abs()
        v = v * sc
    out = {}
    if epi in GELU:
        dx = zero if exact else e + BF16_STORE * v.abs()   # (the fp32 argument against the header's bf16 one)
        ea, ed = GELU_FIT_ACT * GELU_FIT_SLACK + GELU_SLOPE * dx, GELU_FIT_DER * GELU_FIT_SLACK + GELU_CURV * dx
        out["C"] = ea + BF16_STORE * (ref["C"].abs() + ea)
        if epi == EPI_BIAS_GELU:
            out["C2"] = ed + BF16_STORE * (ref["C2"].abs() + ed)
        return out
    if epi in (EPI_ADD, EPI_BIAS_ADD):
        e = e + U * (v.abs() + aux.abs())
        v = v + aux
    if epi in (EPI_DGELU, EPI_DGELU_COLSUM):
        e = e * aux.abs() + U * (v * aux).abs()
        v = v * aux
    store = zero if form.f32 else BF16_STORE * (ref["C"].abs() + e)      # half an ulp of the value that is stored
    if epi == EPI_DGELU_COLSUM:
        terms = e + store if stored_colsum else e
        tot = v.abs().sum(0)
        p2 = prior2.abs() if prior2 is not None else 0.0
        out["C2"] = terms.sum(0) + (M + 2) * U * tot + U * (tot + p2)
    if form.aks and form.bks and form.f32 and form.c2:
        tot = A.abs().sum(1)
        p2 = prior2.abs() if prior2 is not None else 0.0
        out["C2"] = L * U * tot + U * (tot + p2)
    out["C"] = e + store
    return out


def _tern(g, shape, one_in):
    """{-1, 0, 1}, non-zero once in `one_in`"""
    sign = torch.randint(0, 2, shape, generator=g, device=g.device) * 2 - 1
    return (sign * (torch.randint(0, one_in, shape, generator=g, device=g.device) == 0)).to(torch.float32)


def exact_pool(g, M, N, K):
    """the draws exact_operands slices, on the generator's device: one pool serves every shape up to [M, K] x [K, N].  Two densities of A
    and B: non-zero half of the time, and a quarter as often for K above 4096."""
    ints = lambda *shape: torch.randint(-3, 4, shape, generator=g, device=g.device).to(torch.float32)
    steps = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=g.device)
    return {"A": _tern(g, (M, K), 2), "B": _tern(g, (K, N), 2), "A8": _tern(g, (M, K), 8), "B8": _tern(g, (K, N), 8),
            "bias": ints(N), "int": ints(M, N), "dgelu": steps[torch.randint(0, 7, (M, N), generator=g, device=g.device)],
            "int_m": ints(M), "int_n": ints(N)}


def normal_pool(g, M, N, K):
    """ordinary operands, as elsewhere in the suite: randn, B x 0.05 - 0.4 (one factor per column), rounded to bf16 where the call takes
    bf16"""
    r16 = lambda x: x.to(torch.bfloat16).to(torch.float32)
    randn = lambda *shape: torch.randn(shape, generator=g, device=g.device)
    rand = lambda *shape: torch.rand(shape, generator=g, device=g.device)
    col = 0.05 + 0.35 * rand(N)
    return {"A": r16(randn(M, K)), "B": r16(randn(K, N) * col), "bias": randn(N), "int": r16(randn(M, N)),
            "dgelu": r16(rand(M, N) * 1.2 - 0.1), "prior": randn(M, N), "int_m": randn(M), "int_n": randn(N)}


def _cut(pool, form, M, N, K, device, sparse, qcols, qscale, exact):
    ops = {"A": pool["A8" if sparse else "A"][:M, :K].to(device), "B": pool["B8" if sparse else "B"][:K, :N].to(device), "bias": None, "aux": None,
           "prior": None, "prior2": None, "qcols": qcols if form.q else 0, "qscale": qscale if form.q else 1.0}
    if exact and form.epi in GELU:
        ops["B"] = ops["B"] * 0.125
    if form.epi in HAS_BIAS:
        ops["bias"] = pool["bias"][:N].to(device)
    if form.epi in (EPI_ADD, EPI_BIAS_ADD):
        ops["aux"] = pool["int"][:M, :N].to(device)
    if form.epi in (EPI_DGELU, EPI_DGELU_COLSUM):
        ops["aux"] = pool["dgelu"][:M, :N].to(device)
    if form.acc:
        ops["prior"] = pool["prior" if "prior" in pool else "int"][:M, :N].to(device)
    if form.epi == EPI_DGELU_COLSUM:
        ops["prior2"] = pool["int_n"][:N].to(device)
    elif form.c2 and form.f32:
        ops["prior2"] = pool["int_m"][:M].to(device)
    return ops


def ref_of(form, ops):
    return reference(form, ops["A"], ops["B"], ops["bias"], ops["aux"], ops["prior"], ops["qcols"], ops["qscale"], ops["prior2"])


def bars_of(form, ops, splits=1, exact=False, stored_colsum=False):
    return bars(form, ops["A"], ops["B"], ops["bias"], ops["aux"], None, ops["prior"], ops["qcols"], ops["qscale"], ops["prior2"], splits, exact,
                stored_colsum)


def exact_operands(pool, form, M, N, K, device="cpu", qcols=0):
    """Inputs of `form` at M x N x K, cut from exact_pool's draws (or drawn from a torch.Generator handed in its place), on which every linear output is a number the output type holds exactly,
    whatever the order of the sum: A, B in {-1, 0, 1} (fp32 sums of whole numbers below 2^24 are exact), bias and the residual whole
    numbers in -3 .. 3, the saved derivative of IA_EPI_DGELU in {0, +-1/2, +-1, +-2}, the column scale 1/4; for the GELU forms B is
    scaled by 1/8, so the pre-activations are multiples of 1/8 the kernel forms exactly and the GELU is evaluated at known points.  That
    every expected output survives the round trip through the output type is ASSERTED here from the fp64 reference (the pre-activation,
    for the GELU forms): it is the precondition of the tests' equality check.  Returns the operands with "ref" added."""
    if isinstance(pool, torch.Generator):      # (no pool to share: draw exactly this shape)
        pool = exact_pool(pool, M, N, K)
    ops = _cut(pool, form, M, N, K, device, K > 4096, qcols, 0.25, True)
    ref = ref_of(form, ops)
    if form.epi in GELU:
        pre = d(ops["A"]) @ d(ops["B"]) + d(ops["bias"])
        assert holds(pre, False) and holds(pre, True), (form.name, M, N, K, "a pre-activation is no bf16 number")
        assert float(pre.abs().max()) <= 16.0, (form.name, float(pre.abs().max()))
    else:
        assert holds(ref["C"], form.f32), (form.name, M, N, K, "an expected element of C does not fit its type", unheld(ref["C"], form.f32))
        if "C2" in ref:
            assert holds(ref["C2"], True), (form.name, M, N, K, "an expected sum does not fit fp32")
    ops["ref"] = ref
    return ops


def normal_operands(pool, form, M, N, K, device="cpu", qcols=0, qscale=0.18033688):
    if isinstance(pool, torch.Generator):
        pool = normal_pool(pool, M, N, K)
    ops = _cut(pool, form, M, N, K, device, False, qcols, qscale, False)
    ops["ref"] = ref_of(form, ops)
    return ops


# ------------------------------------------------------------------------------------------------ comparison helpers
def first_bad(got, want, bar):
    """None, or the description of the first element of got [M, N] (or [N]) outside want +- bar: (m, n), its 256 x 256 tile and the
    coordinates inside it, got and want"""
    bad = ~((got - want).abs() <= bar)          # (a NaN in got is bad)
    if not bool(bad.any()):
        return None
    idx = int(torch.nonzero(bad.reshape(-1))[0])
    if got.dim() == 1:
        return "%d of %d bad; first at [%d]: got %r want %r (bar %.3e)" % (int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx]), float(bar[idx]))
    m, n = divmod(idx, got.shape[1])
    return "%d of %d bad; first at (m %d, n %d) = tile (%d, %d) row %d col %d: got %r want %r (bar %.3e)" % (
        int(bad.sum()), bad.numel(), m, n, m // 256, n // 256, m % 256, n % 256, float(got[m, n]), float(want[m, n]), float(bar[m, n]))


def worst_ratio(got, want, bar):
    """max |got - want| / bar over the elements with a bar above zero (inf where an element with a zero bar is off)"""
    err = (got - want).abs()
    if bool(((bar == 0) & (err != 0)).any()) or not bool(torch.isfinite(got).all()):
        return math.inf
    pos = bar > 0
    return float((err[pos] / bar[pos]).max()) if bool(pos.any()) else 0.0


# ------------------------------------------------------------------------------------------------ numpy pieces of the CPU model
def np_bf16_rne(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.view(np.float32)


def np_bf16_trunc(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)
