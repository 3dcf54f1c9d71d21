"""fp64 reference of the causal attention kernels (csrc/attention_causal.hip), the element-wise bars their GPU tests hold them to, and
a CPU model of the kernels' rounding that the host tests use to check those bars.  No call into the HIP library, no GPU.

One sequence at a time: q, dO [nh, Lq, 64] with Lq = fold * Lk, k / v [nh, Lk, 64].  Query row i attends key j iff j <= i // fold
(fold = 1: causal self-attention; fold = heads, nh = 1: the decoder block with its query heads folded into rows).  No key mask, no
dropout.  Units and the dictionary returned are those of attn_reference.attn_ref: s2 in log2 units with -inf on pairs that may not
attend, P exactly 0 there.

The bars are attn_reference.bars evaluated on this reference: functions of fp64 quantities only, nothing in them was measured.  They
see the mask through s2 (finite = attendable), so a per-pair mask needs no change to them.  The causal kernels follow the numerics
recipe of attention.hip site by site (see bars() below for the one site that differs and why it adds no term).
"""
import math

import numpy as np
import torch

import attn_reference as A

F64, F32, BF16 = A.F64, A.F32, A.BF16
LOG2E = A.LOG2E
d, bf = A.d, A.bf


def allowed(Lk, fold):
    """bool [fold * Lk, Lk]: query row i may attend key j"""
    i = torch.arange(fold * Lk)[:, None]
    j = torch.arange(Lk)[None, :]
    return j <= i // fold


def scores2(q, k, scale, fold):
    """s2 [nh, Lq, Lk] in log2 units; pairs above the diagonal are -inf"""
    s = torch.matmul(d(q), d(k).transpose(1, 2)) * (scale * LOG2E)
    return s.masked_fill(~allowed(k.shape[1], fold)[None], -math.inf)


def attn_ref(q, k, v, dO, scale, fold):
    """dict: ctx, lse2, P, dq, dk, dv, delta, dS, dPm, K, s2 (attn_reference.attn_ref's keys; K = 1: no dropout)"""
    q, k, v, dO = d(q), d(k), d(v), d(dO)
    assert q.shape[1] == fold * k.shape[1], (q.shape, k.shape, fold)
    s = scores2(q, k, scale, fold)
    m = s.max(-1, keepdim=True).values                      # finite: key 0 is attendable for every row
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    P = p / l
    lse2 = (m + torch.log2(l))[..., 0]
    ctx = torch.matmul(P, v)
    dPm = torch.matmul(dO, v.transpose(1, 2))
    delta = (P * dPm).sum(-1)
    dS = P * (dPm - delta[..., None])
    dq = scale * torch.matmul(dS, k)
    dk = scale * torch.matmul(dS.transpose(1, 2), q)
    dv = torch.matmul(P.transpose(1, 2), dO)
    return dict(ctx=ctx, lse2=lse2, P=P, dq=dq, dk=dk, dv=dv, delta=delta, dS=dS, dPm=dPm, K=torch.ones_like(P), s2=s)


def bars(q, k, v, dO, scale, ref):
    """attn_reference.bars on the causal reference.  Site by site against attention_causal.hip:
      q' = bf16(q sc), 64-term MFMA score chain              as attn_fwd3_kernel (es; no penalty MFMA here, its 4 e stay as slack)
      s - m in fp32, m = the running row maximum rounded up to an integer: |m| <= max |s2| + 1 <= M, so the 2^-22 (|s2| + M) term
        holds.  Moving m multiplies the accumulated sums by a power of two (v_ldexp_f32): exact, so the online softmax has no rounding
        site of its own -- the one place where the kernel differs from attn_fwd3_kernel adds no term.  (A product pushed below 2^-126
        by such a move is flushed: the TINY floor of the bars.)
      v_exp_f32, bf16 pack, row sum of the packed values     a, eP
      PV chain, 1 / l, the multiply, bf16 store              ctx; a row with one attendable key (token 0) is exact: bar 0
      m + log2(l)                                            lse2
      backward: P = exp2(s - lse2), delta = rowsum(dO o O^) from the stored context, dS and P packed to bf16, dq = scale * sum,
      dk = sum dS q' / log2 e, dv = sum P^ dO                rpb, edP, edl (flash-style form), EdS, dq, dk, dv
        dk / dv are summed over four per-wave partial chains that are then added in wave order: still at most Lq + 3 fp32 additions
        per element, inside the (Lq + 8) e chain term, which holds for any order of summation.
    Masked pairs have P = 0 in the kernels by selection (never by multiplication), so every term is 0 there, as bars assumes."""
    return A.bars(q, k, v, dO, scale, ref)


def model(q, k, v, dO, scale, fold, blk=32):
    """The causal kernels' rounding in torch fp32 / bf16 (inputs bf16): q * sc rounded to bf16, fp32 scores, the online softmax over
    32-key blocks with an integer reference (ceil of the running maximum; moving it is an exact power-of-two scaling), P rounded to
    bf16 before PV with the row sum taken from the rounded values, bf16 outputs; the backward recomputes P from lse2, takes delta from
    the stored bf16 context and rounds dS (and P for dV) to bf16.  It exists to check the bars on the host; it is no oracle."""
    sc = np.float32(scale) * np.float32(LOG2E)
    qf, kf, vf, gf = q.to(F32), k.to(F32), v.to(F32), dO.to(F32)
    nh, Lq, _ = qf.shape
    Lk = kf.shape[1]
    ok = allowed(Lk, fold)[None]
    qs = bf(qf * float(sc)).to(F32)
    s = torch.matmul(qs, kf.transpose(1, 2)).masked_fill(~ok, -1e30)
    m = torch.full((nh, Lq, 1), -1e30, dtype=F32)
    l = torch.zeros(nh, Lq, 1, dtype=F32)
    o = torch.zeros(nh, Lq, 64, dtype=F32)
    for j0 in range(0, Lk, blk):
        sb = s[..., j0:j0 + blk]
        m_new = torch.maximum(m, torch.ceil(sb.max(-1, keepdim=True).values))
        shift = torch.clamp(m - m_new, min=-200.0)
        ph = bf(torch.exp2(sb - m_new)).to(F32)
        l = torch.ldexp(l, shift.to(torch.int32)) + ph.sum(-1, keepdim=True)
        o = torch.ldexp(o, shift.to(torch.int32)) + torch.matmul(ph, vf[:, j0:j0 + blk])
        m = m_new
    ctx = bf(o * (np.float32(1.0) / l))
    lse2 = (m + torch.log2(l))[..., 0]
    Pb = torch.where(ok, torch.exp2(s - lse2[..., None]), torch.zeros(1, dtype=F32))
    dPm = torch.matmul(gf, vf.transpose(1, 2))
    delta = (gf * ctx.to(F32)).sum(-1)
    dS = bf(Pb * (dPm - delta[..., None])).to(F32)
    dq = bf(torch.matmul(dS, kf) * float(np.float32(scale)))
    dk = bf(torch.matmul(dS.transpose(1, 2), qs) * float(np.float32(1.0) / np.float32(LOG2E)))
    dv = bf(torch.matmul(bf(Pb).to(F32).transpose(1, 2), gf))
    return dict(ctx=ctx, lse2=lse2, dq=dq, dk=dk, dv=dv, delta=delta)


def family(name, nh, Lk, fold, seed, scale=0.125):
    """attn_reference.family at Lq = fold * Lk"""
    return A.family(name, nh, fold * Lk, Lk, seed, scale)
