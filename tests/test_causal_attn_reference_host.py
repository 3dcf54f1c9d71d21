"""Host checks of tests/causal_attn_reference.py (no GPU): the fp64 causal reference against plain torch, against attn_reference.attn_ref
row by row, the CPU model of the causal kernels' rounding against the bars, and the argument refusals of the two C entry points
(which return before any launch)."""
import math

import pytest
import torch

import attn_reference as A
import causal_attn_reference as C

F64, BF16 = torch.float64, torch.bfloat16
SCALE = 0.125
SHAPES = [(33, 3), (65, 1), (129, 8)]           # (Lk, fold)


def close(name, got, want, rtol=1e-9):
    err = (got - want).abs().max().item()
    assert err <= rtol * max(want.abs().max().item(), 1e-30), (name, err)


@pytest.mark.parametrize("Lk,fold", [(5, 1), (7, 3), (33, 2)])
def test_reference_equals_masked_softmax_and_autograd(Lk, fold):
    nh = 2
    q, k, v, dO = (x.to(F64) for x in C.family("normal", nh, Lk, fold, 3))
    ref = C.attn_ref(q, k, v, dO, SCALE, fold)
    ql, kl, vl = (x.clone().requires_grad_(True) for x in (q, k, v))
    i = torch.arange(fold * Lk)[:, None]
    j = torch.arange(Lk)[None, :]
    sim = (torch.matmul(ql, kl.transpose(1, 2)) * SCALE).masked_fill((j > i // fold)[None], -math.inf)
    P = torch.softmax(sim, -1)
    ctx = torch.matmul(P, vl)
    (ctx * dO).sum().backward()
    close("P", ref["P"], P.detach())
    close("ctx", ref["ctx"], ctx.detach())
    close("lse2", ref["lse2"], torch.logsumexp(sim.detach(), -1) * A.LOG2E)
    close("dq", ref["dq"], ql.grad)
    close("dk", ref["dk"], kl.grad)
    close("dv", ref["dv"], vl.grad)
    assert bool((ref["P"][:, :, :][(j > i // fold)[None].expand_as(ref["P"])] == 0).all())
    assert bool(torch.isinf(ref["s2"]).eq((j > i // fold)[None]).all())
    # token 0 sees one key: its context is that key's value row
    assert torch.equal(ref["ctx"][:, :fold], v[:, :1].expand(nh, fold, 64))


def test_fold_one_agrees_with_the_trusted_reference_row_by_row():
    nh, Lk = 2, 19
    q, k, v, dO = C.family("normal", nh, Lk, 1, 11)
    ref = C.attn_ref(q, k, v, dO, SCALE, 1)
    dk, dv = torch.zeros(nh, Lk, 64, dtype=F64), torch.zeros(nh, Lk, 64, dtype=F64)
    for i in range(Lk):
        r = A.attn_ref(q[:, i:i + 1], k[:, :i + 1], v[:, :i + 1], dO[:, i:i + 1], SCALE)
        close(f"ctx {i}", ref["ctx"][:, i:i + 1], r["ctx"])
        close(f"lse2 {i}", ref["lse2"][:, i:i + 1], r["lse2"])
        close(f"dq {i}", ref["dq"][:, i:i + 1], r["dq"])
        close(f"delta {i}", ref["delta"][:, i:i + 1], r["delta"], rtol=1e-9)
        close(f"P {i}", ref["P"][:, i:i + 1, :i + 1], r["P"])
        dk[:, :i + 1] += r["dk"]
        dv[:, :i + 1] += r["dv"]
    close("dk", ref["dk"], dk)
    close("dv", ref["dv"], dv)


@pytest.mark.parametrize("Lk,fold", SHAPES)
@pytest.mark.parametrize("fam", ["normal", "peaked", "rising", "falling", "uniform"])
def test_cpu_model_of_the_kernels_stays_inside_the_bars(fam, Lk, fold):
    nh = 2
    q, k, v, dO = C.family(fam, nh, Lk, fold, 5)
    ref = C.attn_ref(q, k, v, dO, SCALE, fold)
    bar = C.bars(q, k, v, dO, SCALE, ref)
    got = C.model(q, k, v, dO, SCALE, fold)
    A.compare(f"model {fam} Lk={Lk} fold={fold}", got, ref, bar, tag="causal model")
    # rows of token 0: one attendable key, bar 0, exact
    assert bool((bar["ctx"][:, :fold] == 0).all())
    assert torch.equal(got["ctx"][:, :fold], v[:, :1].expand(nh, fold, 64))


def test_the_bars_catch_a_mask_that_is_off_by_one():
    """a model that lets every row see one key too many is outside the bars: they are not so wide that the mask could hide in them"""
    nh, Lk, fold = 1, 33, 3
    q, k, v, dO = C.family("normal", nh, Lk, fold, 9)
    ref = C.attn_ref(q, k, v, dO, SCALE, fold)
    bar = C.bars(q, k, v, dO, SCALE, ref)
    i = torch.arange(fold * Lk)[:, None]
    j = torch.arange(Lk)[None, :]
    s = (torch.matmul(q.to(F64), k.to(F64).transpose(1, 2)) * SCALE).masked_fill((j > i // fold + 1)[None], -math.inf)
    wrong = torch.matmul(torch.softmax(s, -1), v.to(F64))
    assert float(((wrong - ref["ctx"]).abs() / bar["ctx"].clamp(min=1e-300))[:, :-fold].max()) > 1.0


def test_argument_refusals_without_a_gpu():
    """null pointers, non-positive sizes, Lk > 2048 and short strides are refused with IA_ERR_ARG before any launch"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    P = 4096            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused
    fwd = [P, 64, P, P, 128, P, 64, P, 2, 1, 33, 3, SCALE, None]
    bwd = [P, 64, P, P, 128, P, P, 64, P, P, P, 64, P, P, 128, 2, 1, 33, 3, SCALE, None]
    def refused(fn, base, **edits):
        a = list(base)
        for i, val in edits.items():
            a[int(i[1:])] = val
        return fn(*a) == -1
    for i in (0, 2, 3, 5, 7):                                        # q, k, v, out, lse2
        assert refused(lib.ia_attn_fwd_causal_x, fwd, **{f"a{i}": None}), i
    for i, val in ((8, 0), (9, 0), (10, 0), (11, 0), (8, -1), (11, -2), (10, 2049), (1, 56), (4, 56), (6, 56), (1, 68)):
        assert refused(lib.ia_attn_fwd_causal_x, fwd, **{f"a{i}": val}), (i, val)
    assert refused(lib.ia_attn_fwd_causal_x, fwd, a9=2)              # nh = 2 needs strides >= 128
    for i in (0, 2, 3, 5, 6, 8, 9, 10, 12, 13):                      # q, k, v, out, d_out, lse2, delta, dq, dk, dv
        assert refused(lib.ia_attn_bwd_causal_x, bwd, **{f"a{i}": None}), i
    for i, val in ((15, 0), (16, 0), (17, 0), (18, 0), (17, 2049), (1, 56), (4, 56), (7, 56), (11, 56), (14, 56), (11, 68)):
        assert refused(lib.ia_attn_bwd_causal_x, bwd, **{f"a{i}": val}), (i, val)
    assert refused(lib.ia_attn_bwd_causal_x, bwd, a16=2)
