"""fp64 reference of the attention kernels (csrc/attention.hip), a numpy replica of their dropout draw, the element-wise bars the GPU
tests hold the kernels to, and a CPU model of the kernels' rounding that the host tests use to check those bars.  No call into the
HIP library, no GPU.

One sequence at a time: q [nh, Lq, 64], k / v [nh, Lk, 64], key mask [Lk] bool (True = attend) or None, keep [nh, Lq, Lk] bool or
None (dropout; kept probabilities are scaled by inv_keep).  Packed sequences are the same functions applied per sequence.

Units: s2 = q . k * scale * log2(e) is a score in log2 units, P = 2^(s2 - lse2), lse2 = log2 sum_j 2^s2_j over the attendable keys
(the `lse2` of include/itemalign.h).  With q_prescaled the q rows already hold q * scale * log2(e) (ia_gemm_bf16_qscale) and are taken
as given: s2 = q' . k; dq stays the gradient of the unscaled q (scale * dS k), dk = dS^T q' / log2(e).

The bars are functions of fp64 quantities only (reference values and inputs); nothing in them was measured.  u = 2^-8 is the relative
error of one bf16 rounding
(its unit roundoff: 1.1133 rounds to 1.1172, 2^-8.2 away, so no bf16 output can meet 2^-9 |want|), e = 2^-24 that of one fp32 operation.
"""
import math

import numpy as np
import torch

import glue_reference as G

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LOG2E = 1.4426950408889634
U = 2.0 ** -8             # bf16 rounding, relative: 8 significant bits, round to nearest (half an ulp of 2^-7 at the foot of a binade)
E = 2.0 ** -24            # fp32 rounding, relative
RNG_PAIR_C = 0x9E3779B1   # IA_RNG_PAIR_C (common.h)
TINY = 2.0 ** -105        # absolute floor of a bar that is not zero: flushed denormals, see bars()


def d(x):
    return None if x is None else x.detach().to("cpu").to(F64)


# ------------------------------------------------------------------------------------------------------------ fp64 reference
def scores2(q, k, scale, mask=None, q_prescaled=False):
    """s2 [nh, Lq, Lk] in log2 units; masked keys are -inf."""
    s = torch.matmul(d(q), d(k).transpose(1, 2)) * (1.0 if q_prescaled else scale * LOG2E)
    if mask is not None:
        s = s.masked_fill(~mask.bool()[None, None, :], -math.inf)
    return s


def attn_fwd(q, k, v, scale, mask=None, keep=None, inv_keep=1.0, q_prescaled=False):
    """ctx [nh, Lq, 64], lse2 [nh, Lq], P [nh, Lq, Lk] (before dropout; exactly 0 on masked keys).  A sequence without any attendable
    key has P = 0, ctx = 0 and lse2 = 0 (what the kernels are pinned to; the reference project's additive finfo.min mask would give a
    uniform average there)."""
    s = scores2(q, k, scale, mask, q_prescaled)
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m) & (m < 0)
    m = torch.where(dead, torch.zeros_like(m), m)
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    P = torch.where(dead, torch.zeros_like(p), p / torch.where(dead, torch.ones_like(l), l))
    lse2 = torch.where(dead, torch.zeros_like(m), m + torch.log2(torch.where(dead, torch.ones_like(l), l)))[..., 0]
    Pm = P if keep is None else P * keep.to(F64) * inv_keep
    return torch.matmul(Pm, d(v)), lse2, P


def attn_ref(q, k, v, dO, scale, mask=None, keep=None, inv_keep=1.0, q_prescaled=False):
    """dict: ctx, lse2, P, dq, dk, dv, delta (= sum_j P dPm, dPm = keep / keep_prob * dO v^T), dS, dPm, s2."""
    q, k, v, dO = d(q), d(k), d(v), d(dO)
    ctx, lse2, P = attn_fwd(q, k, v, scale, mask, keep, inv_keep, q_prescaled)
    K = torch.ones_like(P) if keep is None else keep.to(F64) * inv_keep
    dPm = torch.matmul(dO, v.transpose(1, 2)) * K
    delta = (P * dPm).sum(-1)
    dS = P * (dPm - delta[..., None])
    dq = scale * torch.matmul(dS, k)
    dk = torch.matmul(dS.transpose(1, 2), q) * ((1.0 / LOG2E) if q_prescaled else scale)
    dv = torch.matmul((P * K).transpose(1, 2), dO)
    return dict(ctx=ctx, lse2=lse2, P=P, dq=dq, dk=dk, dv=dv, delta=delta, dS=dS, dPm=dPm, K=K,
                s2=scores2(q, k, scale, mask, q_prescaled))


def bias_grad(dq, dk, dv):
    """QKV bias gradient [3 * nh * 64] (q | k | v): column sums over the tokens of [tokens, nh, 64] tensors."""
    return torch.cat([d(x).sum(0).reshape(-1) for x in (dq, dk, dv)])


# ------------------------------------------------------------------------------------------------------------ dropout replica
def rng_row(seed, stream, rows):
    """ia_rng_row(seed, stream, row) for an array of rows: the same function as ia_rng (one full mix of row ^ stream key)."""
    return G.rng32(seed, stream, rows)


def rng_pair(rowkey, pair):
    """ia_rng_pair(rowkey, pair * IA_RNG_PAIR_C): h = (rowkey ^ c) * 0x846ca68b; h ^ (h >> 16)."""
    c = (np.asarray(pair, dtype=np.uint64) * np.uint64(RNG_PAIR_C)) & np.uint64(0xFFFFFFFF)
    h = ((np.asarray(rowkey, dtype=np.uint64) ^ c) * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


def drop_params(p):
    """(thr16, inv_keep) as fill_args forms them in fp32 (the same expressions as the glue kernels' host code)."""
    return G.drop_params(p)


def keep_matrix(seed, b, h, nh, Lq, Lk, p):
    """bool [Lq, Lk]: element (q, key) of stream b * nh + h is kept iff its 16-bit draw >= thr16; the draw is the low (even key) or
    high (odd key) half of ia_rng_pair(ia_rng_row(seed, stream, q), key >> 1)."""
    thr16, _ = drop_params(p)
    rk = rng_row(seed, b * nh + h, np.arange(Lq, dtype=np.uint64)).astype(np.uint64)
    key = np.arange(Lk, dtype=np.uint64)
    r = rng_pair(rk[:, None], (key >> np.uint64(1))[None, :])
    u16 = np.where(key[None, :] & np.uint64(1), r >> np.uint64(16), r & np.uint64(0xFFFF))
    return torch.from_numpy(u16 >= thr16)


def keep_tensor(seed, b, nh, Lq, Lk, p):
    return torch.stack([keep_matrix(seed, b, h, nh, Lq, Lk, p) for h in range(nh)])


# ------------------------------------------------------------------------------------------------------------ bars
def _absmm(a, b):
    return torch.matmul(a.abs(), b.abs())


def bars(q, k, v, dO, scale, ref, exact_delta=False, q_prescaled=False):
    """Element-wise bounds for ctx, lse2, dq, dk, dv and delta of the round-3 kernels, from the reference `ref` (attn_ref) and the
    inputs.  Each term is written beside the rounding site of attention.hip it stands for.

    forward (attn_fwd3_kernel)
      es   score error, log2 units: q * sc is rounded to bf16 once more (the qf fragments).  That rounding is a function of the inputs
           alone (one fp32 multiply by fp32(scale) * fp32(log2 e), round to nearest even), so its size is taken element by element,
           dqe_d = |bf16(q_d sc) - q_d sc| + e |q_d sc| <= (u + e) |q_d sc|, and enters as sum_d dqe_d |k_d| (absent with q_prescaled);
           the 64-term fp32 MFMA chain and the (1, -m_ref) penalty step add (64 + 4) e A, A = sc sum_d |q_d k_d|; forming s - m_ref in
           fp32 against a reference of size M = max_j |s2| + log2 Lk costs 2^-22 (|s2| + M).
      a    relative error of one un-normalised probability as it enters PV and the row sum: exp(ln2 es) - 1 from the score, 2^-22
           for v_exp_f32, u for the bf16 pack (pack_sum).
      eP   the normalised probability p^ / sum p^ is a ratio in which a common factor cancels:
           |P~_ij - P_ij| <= P_ij (a_ij (1 - P_ij) + sum_{k != j} P_ik a_ik) / (1 - R_i), R_i = sum_k P_ik a_ik;
           the row sum itself (fp32 adds of the packed values) adds Lk e.
      ctx  sum_j eP K |v| + (Lk + 8) e sum_j P K |v| (PV chain, the alpha rescales, inv_keep / l, the multiply), then one bf16
           rounding of the result: u |want|.  A row with one attendable key and no dropout returns p^ v / p^: exact, bar 0.
      lse2 m_ref + log2(l), absolute, log2 units: log2(e) (R + Lk e) / (1 - R) from the row sum (R holds the score errors, P-weighted,
           and the u of the pack), 2^-21 (|lse2| + M + 1) for v_log_f32, the rebase arithmetic and the final add.
    backward (attn_bwd3_dq_kernel / attn_bwd3_dkv_kernel / attn_bwd_fused_kernel; P is recomputed as exp2(s - lse2))
      rpb  relative error of the recomputed P: exp(ln2 (es + bar_lse2)) - 1 + 2^-22 (not a ratio: nothing cancels)
      edP  dO . v: 64-term fp32 chain (64 + 6) e sum_d |dO_d v_d|, times K
      edl  delta.  Default (flash style): rowsum(dO o O^) from the STORED bf16 context O^ = bf16(O~), O~ = sum_j P~ K v in fp32:
           sum_d dO_d (O^_d - O~_d) is the documented u sum_d |dO_d O~_d| term (|O~| <= |O| + the ctx error before rounding);
           sum_d dO_d (O~_d - O_d) = sum_j (P~ - P)_j dPm_j <= sum_j eP_j |dPm_j| (summed over d BEFORE the absolute value: the
           error of the probabilities meets dO . v, not 64 separate |dO_d| |v_d|), + the (Lk + 8) e PV chain per column and
           70 e sum_d |dO_d O_d| for the fp32 row sum.  IA_ATTN_EXACT_DELTA=1: sum_j P dPm in fp32 from the recomputed P:
           sum_j (P rpb |dPm| + P edP) + (Lk + 8) e sum_j P |dPm|.
      EdS  dS = P (dPm - delta) rounded to bf16: P rpb |dPm - delta| + P (1 + rpb) (edP + edl) + 3 e |dS|, then u |dS| for the pack
      dq   scale sum_j dS k: scale sum_j EdS |k| + (Lk + 8) e scale sum_j |dS k|, then u |want| for the stored bf16
      dk   scale sum_i dS q (as sum (-dS) q' / log2 e with q' = bf16(q sc): dqe again, absent with q_prescaled):
           scale sum_i EdS |q| + sum_i |dS| dqe / log2 e + (Lq + 8) e scale sum_i |dS q|, then u |want|
      dv   sum_i bf16(P K) dO / keep: sum_i (u + (1 + u) rpb) P K |dO| + (Lq + 8) e sum_i P K |dO|, then u |want|
    Where P is 0 (masked keys, sequences without an attendable key) every term is 0 and the output has to be exact.
    """
    sc32 = float(np.float32(scale) * np.float32(LOG2E))
    q_round = d(bf(q.to(F32) * sc32))                                     # what the kernels' qf fragments hold
    q, k, v, dO = d(q), d(k), d(v), d(dO)
    P, s2, K, dPm, dS, lse2 = ref["P"], ref["s2"], ref["K"], ref["dPm"], ref["dS"], ref["lse2"]
    nh, Lq, Lk = P.shape
    att = torch.isfinite(s2)
    s2f = torch.where(att, s2, torch.zeros_like(s2))
    nvalid = att.sum(-1)                                                  # [nh, Lq]
    sc = 1.0 if q_prescaled else scale * LOG2E
    A = _absmm(q, k.transpose(1, 2)) * sc
    M = s2f.abs().max(-1, keepdim=True).values + math.log2(max(Lk, 2))
    dqe = torch.zeros_like(q) if q_prescaled else (q_round - q * sc32).abs() + E * (q * sc32).abs()
    es = torch.matmul(dqe, k.abs().transpose(1, 2)) + 68 * E * A + 2.0 ** -22 * (s2f.abs() + M)
    a = torch.expm1(math.log(2.0) * es) + 2.0 ** -22 + U
    R = (P * a).sum(-1, keepdim=True)
    assert float(R.max()) < 0.5, "operands too large for a meaningful bar"
    eP = P * (a * (1 - P) + (R - P * a)) / (1 - R) + P * Lk * E
    nodrop = bool((K == 1).all())
    single = (nvalid == 1)[..., None] if nodrop else torch.zeros_like(nvalid, dtype=torch.bool)[..., None]
    eP = torch.where(single, torch.zeros_like(eP), eP)
    accf = torch.where(single, torch.zeros(1, dtype=F64), torch.full((1,), (Lk + 8) * E, dtype=F64))
    b_ctx_in = torch.matmul(eP * K, v.abs()) + accf * torch.matmul(P * K, v.abs())
    b_ctx = torch.where(single, torch.zeros(1, dtype=F64), U * ref["ctx"].abs()) + (1 + U) * b_ctx_in
    b_lse = LOG2E * (R[..., 0] + Lk * E) / (1 - R[..., 0]) + 2.0 ** -21 * (lse2.abs() + M[..., 0] + 1)
    b_lse = torch.where(nvalid > 0, b_lse, torch.zeros_like(b_lse))

    rpb = torch.expm1(math.log(2.0) * (es + b_lse[..., None])) + 2.0 ** -22
    edP = 70 * E * _absmm(dO, v.transpose(1, 2)) * K
    if exact_delta:
        edl = (P * rpb * dPm.abs() + P * edP).sum(-1) + (Lk + 8) * E * (P * dPm.abs()).sum(-1)
    else:
        edl = (U * (dO.abs() * (ref["ctx"].abs() + b_ctx_in)).sum(-1) + (eP * dPm.abs()).sum(-1)
               + (dO.abs() * accf * torch.matmul(P * K, v.abs())).sum(-1) + 70 * E * (dO * ref["ctx"]).abs().sum(-1))
    EdS = P * rpb * (dPm - ref["delta"][..., None]).abs() + P * (1 + rpb) * (edP + edl[..., None]) + 3 * E * dS.abs()
    EdS = U * dS.abs() + (1 + U) * EdS
    b_dq = U * ref["dq"].abs() + (1 + U) * scale * (torch.matmul(EdS, k.abs()) + (Lk + 8) * E * _absmm(dS, k))
    qs = 1.0 / LOG2E if q_prescaled else scale
    b_dk = U * ref["dk"].abs() + (1 + U) * qs * (torch.matmul(EdS.transpose(1, 2), q.abs()) + (Lq + 8) * E * _absmm(dS.transpose(1, 2), q))
    b_dk = b_dk + (1 + U) * torch.matmul(dS.abs().transpose(1, 2), dqe) / LOG2E
    PK = P * K
    b_dv = U * ref["dv"].abs() + (1 + U) * (torch.matmul(((U + (1 + U) * rpb) * PK).transpose(1, 2), dO.abs())
                                             + (Lq + 8) * E * torch.matmul(PK.transpose(1, 2), dO.abs()))
    # fp32 intermediates below 2^-126 (a probability 2^-140 against the row's reference, its products) and bf16 results below it may be
    # flushed to zero: at most 2^11 such terms times operands below 2^10 per output element, wherever anything is computed at all
    flo = lambda x: x + (x > 0) * TINY
    return dict(ctx=flo(b_ctx), lse2=b_lse, dq=flo(b_dq), dk=flo(b_dk), dv=flo(b_dv), delta=edl)


def delta_exact_ref(q, k, v, dO, scale, lse2_got, mask=None, keep=None, inv_keep=1.0, q_prescaled=False):
    """What attn_bwd3_delta_kernel is asked for, in fp64: sum_j P dPm with P = 2^(q' . k - lse2) from the operands the kernel has --
    q' = bf16(q sc) and the saved lse2 -- and the c 2^-24 S bar of an fp32 sum beside it: per term (Lk + 8) for the sum chain, 70 for
    dO . v, and ln2 (68 A + 4 (|s2| + |lse2|)) + 4 for the fp32 score chain, the subtraction and v_exp_f32 behind P."""
    sc = float(np.float32(scale) * np.float32(LOG2E))
    qs = d(q) if q_prescaled else d(bf(q.to(F32) * sc))
    s = scores2(qs, k, 1.0, mask, True)
    lse = d(lse2_got)[..., None]
    P = torch.exp2(s - lse)
    K = torch.ones_like(P) if keep is None else keep.to(F64) * inv_keep
    dPm = torch.matmul(d(dO), d(v).transpose(1, 2)) * K
    A = _absmm(qs, d(k).transpose(1, 2))
    sf = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
    c = (s.shape[-1] + 8 + 70 + 4) + math.log(2.0) * (68 * A + 4 * (sf.abs() + lse.abs()))
    return (P * dPm).sum(-1), E * (P * dPm.abs() * c).sum(-1)


def ratio(name, got, want, bound, tag="attn"):
    """max |got - want| / bound over the elements with a bound; elements whose bound is zero must be exact.  Prints the figure."""
    got, want, bound = d(got), d(want), d(bound)
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all(), (name, "non-finite output")
    err = (got - want).abs()
    exact = bound == 0
    assert (err[exact] == 0).all(), (name, "an element whose bound is zero is not exact", float(err[exact].max()))
    r = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"[{tag}] {name}: max error / bound = {r:.3f}")
    return r


def compare(name, got, ref, bar, keys=("ctx", "lse2", "dq", "dk", "dv"), tag="attn"):
    """every output of `got` (dict) against the reference within its bar; returns {key: ratio} and asserts ratio <= 1"""
    out = {}
    for key in keys:
        if key in got and got[key] is not None:
            out[key] = ratio(f"{name} {key}", got[key], ref[key], bar[key], tag)
    bad = {k_: r for k_, r in out.items() if r > 1.0}
    assert not bad, (name, bad)
    return out


# ------------------------------------------------------------------------------------------------------------ CPU model
def bf(x):
    return x.to(F32).to(BF16)


def model(q, k, v, dO, scale, mask=None, keep=None, inv_keep=1.0, exact_delta=False, q_prescaled=False, p_scale=None, lse_shift=0.0):
    """The kernels' rounding in torch fp32 / bf16 (inputs bf16 [nh, L, 64]): q * sc rounded to bf16, fp32 scores, a bf16-representable
    softmax reference, P rounded to bf16 before PV with the row sum taken from the rounded values, bf16 outputs; the backward
    recomputes P from the saved lse2, rounds dS (and P for dV) to bf16.  It exists to check the bars on the host; it is no oracle.
    Fault hooks of the host tests: p_scale [Lk] multiplies the probabilities that enter PV but not the row sum (accumulators left at
    a wrong scale by a faulty rebase), lse_shift is added to the lse2 that is returned and handed to the backward."""
    sc = np.float32(scale) * np.float32(LOG2E)
    qf, kf, vf, gf = q.to(F32), k.to(F32), v.to(F32), dO.to(F32)
    qs = qf if q_prescaled else bf(qf * float(sc)).to(F32)
    s = torch.matmul(qs, kf.transpose(1, 2))
    if mask is not None:
        s = s.masked_fill(~mask.bool()[None, None, :], -math.inf)
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m)
    m = bf(torch.where(dead, torch.zeros_like(m), m)).to(F32)
    ph = bf(torch.exp2(s - m)).to(F32)
    l = ph.sum(-1, keepdim=True)
    Kf = torch.ones_like(ph) if keep is None else keep.to(F32)
    inv = torch.where(l > 0, np.float32(inv_keep) / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(l))
    ctx = bf(torch.matmul(ph * Kf * (1.0 if p_scale is None else p_scale.to(F32)), vf) * inv)
    lse2 = torch.where(l > 0, m + torch.log2(torch.where(l > 0, l, torch.ones_like(l))), torch.zeros_like(m))[..., 0] + np.float32(lse_shift)
    Pb = torch.exp2(s - lse2[..., None])
    Pb = torch.where(dead, torch.zeros_like(Pb), Pb)
    dPm = torch.matmul(gf, vf.transpose(1, 2)) * Kf * np.float32(inv_keep)
    delta = (Pb * dPm).sum(-1) if exact_delta else (gf * ctx.to(F32)).sum(-1)
    dS = bf(Pb * (dPm - delta[..., None])).to(F32)
    dq = bf(torch.matmul(dS, kf) * float(np.float32(scale)))
    dk = bf(torch.matmul(dS.transpose(1, 2), qs) * (1.0 / LOG2E))      # sum dS q' / log2(e), q' = bf16(q sc), in either form
    dv = bf(torch.matmul(bf(Pb * Kf).to(F32).transpose(1, 2), gf) * float(np.float32(inv_keep)))
    return dict(ctx=ctx, lse2=lse2, dq=dq, dk=dk, dv=dv, delta=delta, P=ph / torch.where(l > 0, l, torch.ones_like(l)))


def rebase_trace(s2, mask=None):
    """Walks attn_fwd3_kernel's lazy softmax reference over the 32-key blocks of every row of s2 [.., Lq, Lk] (log2 units, fp64):
    m_ref starts at 0 and moves (rebase()) when the running row sum leaves [2^-100, 2^60].  A simplification of the kernel, which
    applies the range test to each lane's half of the row (tot = l_run + rs before the two lanes of a query are added: 16 of a block's
    32 keys) and re-bases the whole wave when any lane trips: the kernel re-bases at least where this trace does for sums above
    2^60 by a factor of 2 and more, and may re-base earlier or more often.  Returns the number of rebases that found
    something accumulated (have_prev) and the number that did not, with a block that had an attendable key (have_blk)."""
    s = d(s2).reshape(-1, s2.shape[-1])
    if mask is not None:
        s = s.masked_fill(~mask.bool()[None, :], -math.inf)
    n_prev = n_fresh = 0
    for row in s:
        m_ref, l = 0.0, 0.0
        for j0 in range(0, row.numel(), 32):
            blk = row[j0:j0 + 32]
            arg = (blk - m_ref).clamp(max=1100.0)
            rs = float(torch.exp2(arg).sum()) if bool(torch.isfinite(blk).any()) else 0.0
            rs = 0.0 if rs < 2.0 ** -126 else rs
            tot = l + rs
            if not (2.0 ** -100 <= tot <= 2.0 ** 60):
                tm = float(blk.max())
                have_prev, have_blk = l > 0.0, math.isfinite(tm)
                m_new = m_ref + math.log2(l) if have_prev else m_ref
                if have_blk:
                    m_new = max(m_new, tm) if have_prev else tm
                n_prev += int(have_prev and have_blk)
                n_fresh += int((not have_prev) and have_blk)
                l = l * 2.0 ** (m_ref - m_new) if have_prev else 0.0
                m_ref = m_new
                rs = float(torch.exp2(blk - m_ref).sum()) if have_blk else 0.0
            l += rs
    return n_prev, n_fresh


# ------------------------------------------------------------------------------------------------------------ operand families
def gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_q0(scale, lo=12.0, hi=20.0):
    """the bf16 value in [lo, hi] whose product with sc = fp32(scale) * fp32(log2 e) loses least in the kernels' bf16 rounding of
    q * sc: the one large query column of the peaked / rising / falling families, so that scores of 100 and more in log2 units carry
    a rounding error (and a bar, which takes that rounding from the inputs) of 1e-3 and not of 0.5"""
    sc32 = float(np.float32(scale) * np.float32(LOG2E))
    c = bf(torch.arange(lo, hi, 0.0625)).to(F64).unique()
    err = (d(bf(c.to(F32) * sc32)) - c * sc32).abs() / c
    return float(c[int(err.argmin())])


def family(name, nh, Lq, Lk, seed, scale=0.125):
    """bf16 q [nh, Lq, 64], k, v [nh, Lk, 64], dO [nh, Lq, 64] of one sequence.
    normal   N(0, 1)
    half     N(0, 1/4) operands (tighter bars: the fault-injection tests)
    peaked   one key per row ahead of the others by 30 .. 60 in log2 units (peaked / rising / falling: the large scores come from
             one query column, exact_q0, whose pre-scaled value is all but exact in bf16)
    rising   scores climbing by 0.9 log2 units per key up to 140: the row sum passes 2^60 against the first tile's reference in the
             first block of tile 1 (the `other` shift) and again on the plateau
    falling  scores starting at -120 and falling by 0.9 per key down to -250: the first block's sum is below 2^-100
    uniform  near-uniform P, value rows a | a + one ulp in a 1 : 3 / 3 : 1 pattern, dO = +1 | -1: the stored context is rounded
             the same way in every column, the adverse case of delta = rowsum(dO o O)
    equalv   all value rows equal, dO constant over the queries: dP - delta = 0, dq = dk = 0
    """
    g = gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v, dO = rn(nh, Lq, 64), rn(nh, Lk, 64), rn(nh, Lk, 64), rn(nh, Lq, 64)
    sc = scale * LOG2E
    if name == "half":
        q, k = q * 0.5, k * 0.5
    elif name == "peaked":
        q, k = q * 0.25, k * 0.25
        q0 = exact_q0(scale)
        q[..., 0] = q0
        k[..., 0] = 0.0
        peak = torch.randint(0, Lk, (nh, 8), generator=g)
        amp = 30.0 + 30.0 * torch.rand(nh, 8, generator=g)
        for h in range(nh):
            k[h, peak[h], 0] = amp[h] / (q0 * sc)
    elif name in ("rising", "falling"):
        q, k = q * 0.25, k * 0.25
        q0 = exact_q0(scale)
        q[..., 0] = q0
        j = torch.arange(Lk, dtype=torch.float32)
        ramp = (0.9 * j).clamp(max=140.0) if name == "rising" else (-120.0 - 0.9 * j).clamp(min=-250.0)
        k[..., 0] = (ramp / (q0 * sc))[None, :]
    elif name == "uniform":
        q = q * 0.01
        j = torch.arange(Lk)
        lo = ((j % 4) == 0).float()[:, None]              # 1 row in 4 carries the extra ulp: mean a + ulp / 4, rounds down
        hi = ((j % 4) != 0).float()[:, None]              # 3 rows in 4: mean a + 3 ulp / 4, rounds up
        v = torch.ones(nh, Lk, 64)
        v[:, :, :32] += lo * 2.0 ** -7
        v[:, :, 32:] += hi * 2.0 ** -7
        dO = torch.ones(nh, Lq, 64)
        dO[:, :, 32:] = -1.0
    elif name == "equalv":
        v = rn(nh, 1, 64).expand(nh, Lk, 64).contiguous()
        dO = rn(nh, 1, 64).expand(nh, Lq, 64).contiguous()
    else:
        assert name == "normal", name
    return bf(q), bf(k), bf(v), bf(dO)


def mask_of(kind, Lk):
    """the key masks of the tests: bool [Lk] or None"""
    m = torch.ones(Lk, dtype=torch.bool)
    if kind == "none":
        return None
    if kind == "prefix":
        m[max(1, (2 * Lk) // 3):] = False
    elif kind == "hole":
        m[Lk // 3: Lk // 3 + max(1, Lk // 5)] = False
    elif kind in ("tile_first", "tile_middle", "tile_last"):
        nt = (Lk + 63) // 64
        t = {"tile_first": 0, "tile_middle": nt // 2, "tile_last": nt - 1}[kind]
        m[t * 64:(t + 1) * 64] = False
    elif kind == "one_key":
        m[:] = False
        m[(Lk * 5) // 7] = True
    elif kind == "alternating":
        m[1::2] = False
    elif kind == "dead":
        m[:] = False
    else:
        raise ValueError(kind)
    return m


MASKS = ("none", "prefix", "hole", "tile_first", "tile_middle", "tile_last", "one_key", "alternating")
