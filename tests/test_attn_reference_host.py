"""tests/attn_reference.py checked on the host: the fp64 attention against torch autograd in fp64, the dropout replica's statistics,
the bars against the CPU model of the kernels' rounding (the reference alone must stay inside them), and the bars against injected
faults (they must not be vacuous).  No GPU."""
import math

import numpy as np
import pytest
import torch

import attn_reference as A

F64, F32 = torch.float64, torch.float32
SCALE = 0.125


def _autograd(q, k, v, dO, scale, mask, keep, inv_keep):
    q, k, v = (A.d(x).requires_grad_(True) for x in (q, k, v))
    s = torch.matmul(q, k.transpose(1, 2)) * scale
    if mask is not None:
        s = s.masked_fill(~mask[None, None, :], -math.inf)
    P = torch.softmax(s, -1)
    Pm = P if keep is None else P * keep.to(F64) * inv_keep
    ctx = torch.matmul(Pm, v)
    lse2 = torch.logsumexp(s, -1) * A.LOG2E
    ctx.backward(A.d(dO))
    return ctx.detach(), lse2.detach(), P.detach(), q.grad, k.grad, v.grad


def _close(name, got, want, tol=1e-12):
    err = float((got - want).abs().max() / max(1.0, float(want.abs().max())))
    assert err <= tol, (name, err)


@pytest.mark.parametrize("kind", A.MASKS)
@pytest.mark.parametrize("Lq,Lk", [(70, 70), (5, 200), (130, 97)])
def test_reference_matches_autograd(kind, Lq, Lk):
    q, k, v, dO = A.family("normal", 2, Lq, Lk, 11)
    mask = A.mask_of(kind, Lk)
    keep = A.keep_tensor(5, 1, 2, Lq, Lk, 0.25) if kind in ("none", "hole") else None
    inv_keep = A.drop_params(0.25)[1] if keep is not None else 1.0
    ref = A.attn_ref(q, k, v, dO, SCALE, mask, keep, inv_keep)
    ctx, lse2, P, dq, dk, dv = _autograd(q, k, v, dO, SCALE, mask, keep, inv_keep)
    for name, got, want in (("ctx", ref["ctx"], ctx), ("lse2", ref["lse2"], lse2), ("P", ref["P"], P), ("dq", ref["dq"], dq),
                            ("dk", ref["dk"], dk), ("dv", ref["dv"], dv)):
        _close(name, got, want)
    if mask is not None:
        assert (ref["P"][..., ~mask] == 0).all() and (ref["dk"][:, ~mask] == 0).all() and (ref["dv"][:, ~mask] == 0).all()
    _close("delta", ref["delta"], (A.d(dO) * ref["ctx"]).sum(-1))


def test_reference_prescaled_and_packed_and_bias():
    q, k, v, dO = A.family("normal", 2, 40, 40, 12)
    sc = SCALE * A.LOG2E
    qs = A.d(q) * sc
    a, b = A.attn_ref(q, k, v, dO, SCALE), A.attn_ref(qs, k, v, dO, SCALE, q_prescaled=True)
    for key in ("ctx", "lse2", "dq", "dk", "dv"):
        _close(key, b[key], a[key])
    # packed sequences = the same function per sequence: a block-diagonal mask over the concatenation gives the same rows
    lens = [1, 17, 22]
    tot = sum(lens)
    qg, kg, vg = (A.d(x).requires_grad_(True) for x in (q, k, v))
    s = torch.matmul(qg, kg.transpose(1, 2)) * SCALE
    blk = torch.block_diag(*[torch.ones(n, n) for n in lens]).bool()
    P = torch.softmax(s.masked_fill(~blk[None], -math.inf), -1)
    torch.matmul(P, vg).backward(A.d(dO))
    c0 = 0
    for n in lens:
        sl = slice(c0, c0 + n)
        r = A.attn_ref(q[:, sl], k[:, sl], v[:, sl], dO[:, sl], SCALE)
        _close("packed ctx", r["ctx"], torch.matmul(P, A.d(v))[:, sl].detach())
        _close("packed dq", r["dq"], qg.grad[:, sl])
        _close("packed dk", r["dk"], kg.grad[:, sl])
        _close("packed dv", r["dv"], vg.grad[:, sl])
        c0 += n
    assert c0 == tot
    g = A.bias_grad(a["dq"].transpose(0, 1), a["dk"].transpose(0, 1), a["dv"].transpose(0, 1))
    _close("bias", g[:128], a["dq"].sum(1).reshape(-1))
    _close("bias v", g[256:], a["dv"].sum(1).reshape(-1))


def test_reference_dead_sequence_is_zero():
    q, k, v, dO = A.family("normal", 2, 9, 9, 13)
    r = A.attn_ref(q, k, v, dO, SCALE, A.mask_of("dead", 9))
    for key in ("ctx", "lse2", "dq", "dk", "dv", "P"):
        assert (r[key] == 0).all(), key


# ------------------------------------------------------------------------------------------------------------ dropout replica
@pytest.mark.parametrize("p", [0.1, 0.25])
def test_replica_keep_fraction_and_determinism(p):
    thr16, inv_keep = A.drop_params(p)
    assert thr16 == int(round(p * 65536)) and abs(inv_keep - 1.0 / (1.0 - thr16 / 65536.0)) < 1e-6
    keep = A.keep_tensor(77, 3, 4, 300, 513, p)
    n = keep.numel()
    pk = 1.0 - thr16 / 65536.0
    assert abs(float(keep.double().mean()) - pk) <= 4.0 * math.sqrt(pk * (1 - pk) / n)
    again = A.keep_matrix(77, 3, 2, 4, 300, 513, p)
    assert torch.equal(keep[2], again)
    assert torch.equal(A.keep_matrix(77, 3, 2, 4, 10, 20, p), again[:10, :20])          # an element's bit depends on its coordinates only
    other = A.keep_matrix(78, 3, 2, 4, 300, 513, p)
    assert not torch.equal(other, again)
    assert not torch.equal(A.keep_matrix(77, 2, 2, 4, 300, 513, p), again)


def test_replica_against_the_written_out_hash():
    """one element by hand from common.h: ia_mix32 twice for the row key, one multiply-xorshift for the pair"""
    def mix(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    seed, b, h, nh, qrow, key = 1234, 2, 1, 3, 45, 67
    rk = mix(qrow ^ mix((b * nh + h) ^ ((seed * 0x9E3779B9) & 0xFFFFFFFF)))
    hh = ((rk ^ (((key >> 1) * 0x9E3779B1) & 0xFFFFFFFF)) * 0x846CA68B) & 0xFFFFFFFF
    hh ^= hh >> 16
    draw = (hh >> 16) if key & 1 else (hh & 0xFFFF)
    for p in (0.1, 0.25, 0.9):
        assert bool(A.keep_matrix(seed, b, h, nh, qrow + 1, key + 1, p)[qrow, key]) == (draw >= A.drop_params(p)[0])


# ------------------------------------------------------------------------------------------------------------ model within bars
def _run(fam, Lq, Lk, kind="none", p=0.0, exact=False, seed=3, nh=2, ps=False):
    q, k, v, dO = A.family(fam, nh, Lq, Lk, seed)
    mask = A.mask_of(kind, Lk)
    keep = A.keep_tensor(9, 0, nh, Lq, Lk, p) if p > 0 else None
    inv_keep = A.drop_params(p)[1]
    if ps:
        q = A.bf(q.to(F32) * float(np.float32(SCALE) * np.float32(A.LOG2E)))
    ref = A.attn_ref(q, k, v, dO, SCALE, mask, keep, inv_keep, q_prescaled=ps)
    bar = A.bars(q, k, v, dO, SCALE, ref, exact_delta=exact, q_prescaled=ps)
    got = A.model(q, k, v, dO, SCALE, mask, keep, inv_keep, exact_delta=exact, q_prescaled=ps)
    return (q, k, v, dO, mask, keep, inv_keep), ref, bar, got


MODEL_CASES = ([(f, 70, 70, "none", 0.0, False) for f in ("normal", "half", "peaked", "rising", "falling", "uniform", "equalv")]
               + [("normal", 150, 150, m, 0.0, False) for m in A.MASKS[1:]]
               + [("normal", 33, 257, "hole", 0.25, False), ("normal", 129, 129, "none", 0.1, False), ("rising", 40, 300, "none", 0.0, False),
                  ("falling", 40, 300, "tile_middle", 0.0, False), ("uniform", 64, 64, "none", 0.0, True), ("normal", 90, 90, "prefix", 0.25, True),
                  ("peaked", 20, 513, "alternating", 0.0, True), ("normal", 1, 1, "none", 0.0, False), ("normal", 31, 31, "none", 0.0, False)])


@pytest.mark.parametrize("fam,Lq,Lk,kind,p,exact", MODEL_CASES)
def test_model_stays_within_the_bars(fam, Lq, Lk, kind, p, exact):
    _, ref, bar, got = _run(fam, Lq, Lk, kind, p, exact)
    A.compare(f"model {fam} {Lq}x{Lk} {kind} p={p} exact={exact}", got, ref, bar, tag="attn-model")
    if exact:
        A.ratio("model exact delta", got["delta"], ref["delta"], bar["delta"], "attn-model")


def test_model_prescaled_stays_within_the_bars():
    _, ref, bar, got = _run("normal", 100, 100, "hole", 0.1, ps=True)
    A.compare("model prescaled", got, ref, bar, tag="attn-model")


def test_rebase_families_cross_the_thresholds():
    """the `rising` operands pass 2^60 with something accumulated (have_prev), in the first block of a tile; the `falling` ones start
    below 2^-100 (nothing accumulated); N(0, 1) operands never leave the range (which is why the older tests never ran rebase())"""
    for L in (129, 300):
        q, k, v, dO = A.family("rising", 1, 8, L, 3)
        assert A.rebase_trace(A.scores2(q, k, SCALE))[0] >= 8
        q, k, v, dO = A.family("falling", 1, 8, L, 3)
        n_prev, n_fresh = A.rebase_trace(A.scores2(q, k, SCALE))
        assert n_fresh >= 8
    q, k, v, dO = A.family("rising", 1, 4, 129, 3)
    s = A.scores2(q, k, SCALE)
    assert float(torch.exp2(s[0, :, :64]).sum(-1).max()) < 2.0 ** 60 < float(torch.exp2(s[0, :, :96]).sum(-1).min())   # block 0 of tile 1
    q, k, v, dO = A.family("normal", 1, 8, 300, 3)
    assert A.rebase_trace(A.scores2(q, k, SCALE)) == (0, 0)
    q, k, v, dO = A.family("normal", 1, 8, 300, 3)
    assert A.rebase_trace(A.scores2(q, k, SCALE), A.mask_of("tile_first", 300))[1] == 0      # a dead first block re-bases for free


# ------------------------------------------------------------------------------------------------------------ injected faults
def _fails(name, got, ref, bar, key):
    r = A.ratio(f"fault: {name} {key}", torch.nan_to_num(A.d(got[key])), ref[key], torch.where(bar[key] == 0, torch.full_like(bar[key], 1e-300), bar[key]),
                "attn-fault")
    assert r > 1.0, (name, key, r)


def test_fault_masked_key_admitted():
    (q, k, v, dO, mask, keep, ik), ref, bar, _ = _run("half", 70, 70, "hole")
    bad = mask.clone()
    bad[int((~mask).nonzero()[0])] = True
    got = A.model(q, k, v, dO, SCALE, bad)
    for key in ("ctx", "lse2", "dk", "dv"):
        _fails("masked key admitted", got, ref, bar, key)


def test_fault_last_key_of_ragged_tile_dropped():
    (q, k, v, dO, mask, keep, ik), ref, bar, _ = _run("half", 70, 70)
    bad = torch.ones(70, dtype=torch.bool)
    bad[69] = False
    got = A.model(q, k, v, dO, SCALE, bad)
    for key in ("ctx", "lse2", "dv"):
        _fails("last key dropped", got, ref, bar, key)


def test_fault_keep_matrix_shifted():
    (q, k, v, dO, mask, keep, ik), ref, bar, _ = _run("half", 70, 70, p=0.25)
    got = A.model(q, k, v, dO, SCALE, None, torch.roll(keep, 1, -1), ik)
    for key in ("ctx", "dq", "dk", "dv"):
        _fails("keep shifted by one key", got, ref, bar, key)


def test_fault_lse2_off():
    _, ref, bar, got = _run("half", 70, 70)
    got = dict(got, lse2=got["lse2"] + 2.0 ** -6)
    _fails("lse2 + 2^-6", got, ref, bar, "lse2")


def test_fault_skipped_rebase_leaves_p_unnormalised():
    """rebase() skipped: what was accumulated before the reference moved keeps its old scale, 2^(m_new - m_old) too large"""
    (q, k, v, dO, mask, keep, ik), ref, bar, got = _run("rising", 40, 129)
    s = A.scores2(q, k, SCALE)
    m_new = float(s[0, 0, 64:96].max())
    P = got["P"].clone()
    P[..., :64] *= 2.0 ** min(m_new, 120.0)
    got = dict(got, ctx=A.bf(torch.matmul(P, v.to(F32))))
    _fails("skipped rebase", got, ref, bar, "ctx")


def test_fault_four_ulps():
    """4 * 2^-8 relative (2 to 4 bf16 ulps, by where the value sits in its binade) at the element of the `peaked` family whose bar is
    closest to u |want|.  Where P is spread over many keys (N(0, 1)) the ctx bar is a few per cent of sum_j P |v_j|, more than 4 ulps of
    a typical element: such a step is only seen where the bar is tight; test_fault_scaled_and_zero_gradients covers that family."""
    _, ref, bar, got = _run("peaked", 70, 70)
    ctx = got["ctx"].to(F32).clone()
    i = int((ref["ctx"].abs() / bar["ctx"]).argmax())
    flat = ctx.view(-1)
    flat[i] = flat[i] * (1 + 4 * 2.0 ** -8)
    _fails("4 bf16 ulps", dict(got, ctx=ctx), ref, bar, "ctx")


def test_fault_flash_delta_under_the_exact_bar():
    """delta from the bf16-rounded context is inside the default bar and outside the exact-delta one (the `uniform` family rounds
    every column of the context the same way)"""
    (q, k, v, dO, mask, keep, ik), ref, bar_exact, got_exact = _run("uniform", 64, 64, exact=True)
    A.compare("exact model, exact bar", got_exact, ref, bar_exact, tag="attn-model")
    flash = A.model(q, k, v, dO, SCALE)
    A.compare("flash model, default bar", flash, ref, A.bars(q, k, v, dO, SCALE, ref), tag="attn-model")
    for key in ("dq", "dk"):
        _fails("flash delta under the exact bar", flash, ref, bar_exact, key)


@pytest.mark.parametrize("L", [129, 300])
def test_fault_scaled_and_zero_gradients(L):
    """N(0, 1) operands: every output scaled by 1.1, and every output replaced by zeros, is outside its bar"""
    _, ref, bar, got = _run("normal", L, L)
    for key in ("ctx", "dq", "dk", "dv"):
        _fails("x 1.1", {key: got[key].to(F32) * 1.1}, ref, bar, key)
        _fails("zeros", {key: torch.zeros_like(got[key])}, ref, bar, key)
    _fails("zeros", {"lse2": torch.zeros_like(got["lse2"])}, ref, bar, "lse2")


@pytest.mark.parametrize("L", [129, 300])
@pytest.mark.parametrize("fam", ["rising", "falling", "peaked"])
def test_fault_rebase_families_have_teeth(fam, L):
    """the bars used on the operands that force rebase(): zeros are outside every one of them; probabilities left a factor 2^+-0.25
    off on the keys behind the first re-base (key 96 on: accumulators rescaled by a slightly wrong alpha) move ctx outside its bar, an
    lse2 off by +-0.25 moves lse2, dq, dk and dv outside theirs"""
    (q, k, v, dO, mask, keep, ik), ref, bar, got = _run(fam, L, L)
    for key in ("ctx", "lse2", "dq", "dk", "dv"):
        _fails("zeros", {key: torch.zeros_like(got[key])}, ref, bar, key)
    for sh in (0.25, -0.25):
        if fam != "peaked":
            ps = torch.ones(L)
            ps[96:] = 2.0 ** sh
            if fam == "falling":
                ps = torch.ones(L)
                ps[:32] = 2.0 ** sh                       # the block that re-based, against what follows it
            _fails(f"P x 2^{sh}", A.model(q, k, v, dO, SCALE, p_scale=ps), ref, bar, "ctx")
        bad = A.model(q, k, v, dO, SCALE, lse_shift=sh)
        for key in ("lse2", "dq", "dk", "dv"):
            _fails(f"lse2 {sh:+}", bad, ref, bar, key)
