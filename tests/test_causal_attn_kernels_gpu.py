"""ia_attn_fwd_causal_x / ia_attn_bwd_causal_x (csrc/attention_causal.hip) through the C ABI against the fp64 reference of
tests/causal_attn_reference.py, element by element for ctx, lse2, dq, dk and dv, within attn_reference.bars evaluated on that reference
(checked on the host against a CPU model of the kernels' rounding by tests/test_causal_attn_reference_host.py; never fitted to a GPU
result).  Every call runs on sentinel-filled outputs with pad columns and 64 guard rows that have to come back bit-unchanged; the
strides are all different (ld_o != ld_q, ld_dq != ld_dkv).  Every comparison prints max error / bound (`-s` shows them).

Shapes: B = 2 (a batch offset), Lk around the 32-key block and the 64-key tile, fold = 3 (32-row query blocks straddle tokens),
fold = 8 / 16 (the decoder's folded heads), Lk = 300 with fold = 3 (more than one 128-query workgroup per key tile, several key
workgroups, the dK / dV reduction over many query blocks)."""
import functools

import pytest
import torch

import attn_reference as A
import causal_attn_reference as C

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SCALE = 0.125
SENT = -7.0
GUARD = 64
RATIOS = {}

LKS = (1, 2, 31, 32, 33, 63, 64, 65, 129, 255, 300)
CASES = [(1 + (i + f) % 2, Lk, f, "normal") for i, Lk in enumerate(LKS) for f in (1, 3)]
CASES += [(1, 33, 8, "normal"), (2, 65, 8, "normal"), (2, 33, 16, "normal"), (1, 65, 16, "normal")]
# operand families that move the softmax reference (rising), start far below it (falling), put all weight on one key (peaked) and
# make the stored context round one way (uniform: the adverse case of delta = rowsum(dO o O))
CASES += [(1, 129, 3, "rising"), (2, 129, 1, "falling"), (1, 65, 8, "peaked"), (1, 65, 3, "uniform")]


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


def st():
    from item_alignment_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what):
    from item_alignment_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def rows_of(x):
    """[B, nh, L, 64] -> token-major [B * L, nh * 64]"""
    B, nh, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, nh * 64)


def heads_of(rows, B, nh, L):
    return rows[:B * L, :nh * 64].reshape(B, L, nh, 64).permute(0, 2, 1, 3)


def out_buf(n_rows, H, pad):
    return torch.full((n_rows + GUARD, H + pad), SENT, dtype=BF16, device="cuda")


def untouched(name, buf, n_rows, H):
    assert bool((buf[n_rows:] == SENT).all()), (name, "rows past the last token were written")
    assert bool((buf[:, H:] == SENT).all()), (name, "columns past nh * 64 were written")


def run(lib, Q, K, V, dO, fold, bwd=True, pad_q=0, pad_o=8, pad_dq=16, pad_dkv=24):
    """One forward (+ backward).  Q, dO [B, nh, fold * Lk, 64], K, V [B, nh, Lk, 64] bf16 host tensors; k | v are packed side by side
    (ld_kv = 2 H, as the decoder block hands them over).  Returns host tensors in the [B, nh, L, 64] shape, lse2 and delta."""
    B, nh, Lq, _ = Q.shape
    Lk = K.shape[2]
    assert Lq == fold * Lk
    H = nh * 64
    Tq, Tk = B * Lq, B * Lk
    qd = torch.full((Tq, H + pad_q), 3.0, dtype=BF16, device="cuda")
    qd[:, :H] = rows_of(Q).cuda()
    kv = torch.cat((rows_of(K), rows_of(V)), 1).cuda().contiguous()
    kp, vp, ld_kv = kv.data_ptr(), kv.data_ptr() + 2 * H, 2 * H
    out = out_buf(Tq, H, pad_o)
    lse2 = torch.full((B * nh * Lq + GUARD,), float("nan"), dtype=F32, device="cuda")
    ok(lib.ia_attn_fwd_causal_x(qd.data_ptr(), H + pad_q, kp, vp, ld_kv, out.data_ptr(), H + pad_o, lse2.data_ptr(), B, nh, Lk, fold, SCALE,
                                st()), "ia_attn_fwd_causal_x")
    untouched("ctx", out, Tq, H)
    assert bool(torch.isnan(lse2[B * nh * Lq:]).all()), "lse2 was written past [B, nh, Lq]"
    res = {"ctx": heads_of(out[:Tq, :H].cpu(), B, nh, Lq), "lse2": lse2[:B * nh * Lq].reshape(B, nh, Lq).cpu()}
    if bwd:
        g = torch.full((Tq + GUARD, H + pad_o), SENT, dtype=BF16, device="cuda")
        g[:Tq, :H] = rows_of(dO).cuda()
        delta = torch.full((B * nh * Lq + GUARD,), float("nan"), dtype=F32, device="cuda")
        dq, dk, dv = out_buf(Tq, H, pad_dq), out_buf(Tk, H, pad_dkv), out_buf(Tk, H, pad_dkv)
        ok(lib.ia_attn_bwd_causal_x(qd.data_ptr(), H + pad_q, kp, vp, ld_kv, out.data_ptr(), g.data_ptr(), H + pad_o, lse2.data_ptr(),
                                    delta.data_ptr(), dq.data_ptr(), H + pad_dq, dk.data_ptr(), dv.data_ptr(), H + pad_dkv, B, nh, Lk, fold,
                                    SCALE, st()), "ia_attn_bwd_causal_x")
        untouched("dq", dq, Tq, H)
        untouched("dk", dk, Tk, H)
        untouched("dv", dv, Tk, H)
        assert bool((g[Tq:] == SENT).all()) and bool((out[Tq:] == SENT).all()) and bool((qd[:, H:] == 3.0).all())
        assert bool(torch.isnan(delta[B * nh * Lq:]).all()), "delta was written past [B, nh, Lq]"
        res.update(dq=heads_of(dq[:Tq, :H].cpu(), B, nh, Lq), dk=heads_of(dk[:Tk, :H].cpu(), B, nh, Lk),
                   dv=heads_of(dv[:Tk, :H].cpu(), B, nh, Lk), delta=delta[:B * nh * Lq].reshape(B, nh, Lq).cpu())
    return res


@functools.lru_cache(maxsize=None)
def operands(nh, Lk, fold, fam, B=2):
    """(Q, K, V, dO) stacked over B sequences, and per sequence the fp64 reference and its bars; computed once, shared, never changed"""
    ops = [C.family(fam, nh, Lk, fold, 1000 * fold + 7 * b + Lk) for b in range(B)]
    Q, K, V, dO = (torch.stack([o[i] for o in ops]) for i in range(4))
    refs = [C.attn_ref(*o, SCALE, fold) for o in ops]
    bars = [C.bars(*o, SCALE, r) for o, r in zip(ops, refs)]
    return Q, K, V, dO, refs, bars


def note(name, ratios):
    for key, r in ratios.items():
        if r >= RATIOS.get(key, (-1.0, ""))[0]:
            RATIOS[key] = (r, name)


@pytest.mark.parametrize("nh,Lk,fold,fam", CASES)
def test_every_output_against_fp64_within_the_bars(lib, nh, Lk, fold, fam):
    Q, K, V, dO, refs, bars = operands(nh, Lk, fold, fam)
    got = run(lib, Q, K, V, dO, fold)
    for b, (ref, bar) in enumerate(zip(refs, bars)):
        name = f"{fam} nh={nh} Lk={Lk} fold={fold} b={b}"
        note(name, A.compare(name, {k: got[k][b] for k in ("ctx", "lse2", "dq", "dk", "dv")}, ref, bar, tag="causal"))
        note(name, {"delta": A.ratio(f"{name} delta", got["delta"][b], ref["delta"], bar["delta"], "causal")})
        # one attendable key gives P = 1: the rows of token 0 are v[0], bit for bit
        assert torch.equal(got["ctx"][b][:, :fold], V[b][:, :1].expand(nh, fold, 64)), name


@pytest.mark.parametrize("nh,Lk,fold", [(2, 33, 3), (1, 65, 1), (1, 65, 8), (2, 129, 3)])
def test_causality_is_bitwise(lib, nh, Lk, fold):
    """keys after token t cannot reach the queries of tokens <= t, and those queries alone cannot reach dk / dv of the keys after t"""
    Q, K, V, dO, _, _ = operands(nh, Lk, fold, "normal")
    base = run(lib, Q, K, V, dO, fold, bwd=False)
    K2, V2 = (torch.stack([C.family("normal", nh, Lk, fold, 77 + b)[i] for b in range(2)]) for i in (1, 2))
    for t in (0, Lk // 2):
        Kt, Vt = K.clone(), V.clone()
        Kt[:, :, t + 1:], Vt[:, :, t + 1:] = 3 * K2[:, :, t + 1:], V2[:, :, t + 1:]
        other = run(lib, Q, Kt, Vt, dO, fold, bwd=False)
        n = (t + 1) * fold                                   # query rows with i // fold <= t
        assert torch.equal(base["ctx"][:, :, :n], other["ctx"][:, :, :n]), (t, "ctx")
        assert torch.equal(base["lse2"][:, :, :n], other["lse2"][:, :, :n]), (t, "lse2")
        if t + 1 < Lk:
            assert not torch.equal(base["ctx"][:, :, n:], other["ctx"][:, :, n:]), (t, "the changed keys reach nobody")
        g = dO.clone()
        g[:, :, n:] = 0
        back = run(lib, Q, K, V, g, fold)
        assert bool((back["dk"][:, :, t + 1:] == 0).all()) and bool((back["dv"][:, :, t + 1:] == 0).all()), t
        assert bool((back["dq"][:, :, n:] == 0).all()), t
        assert bool((back["dv"][:, :, :t + 1] != 0).any()), t


@pytest.mark.parametrize("nh,Lk,fold", [(2, 65, 3), (1, 300, 3), (1, 65, 16)])
def test_the_backward_is_deterministic(lib, nh, Lk, fold):
    Q, K, V, dO, _, _ = operands(nh, Lk, fold, "normal")
    a, b = run(lib, Q, K, V, dO, fold), run(lib, Q, K, V, dO, fold)
    for key in ("ctx", "lse2", "dq", "dk", "dv", "delta"):
        assert torch.equal(a[key].view(torch.int16 if a[key].dtype == BF16 else torch.int32),
                           b[key].view(torch.int16 if b[key].dtype == BF16 else torch.int32)), key


@pytest.mark.parametrize("nh", [1, 2])
def test_cross_check_against_the_x_form_token_by_token(lib, nh):
    """Lk = 33, fold = 3: the rows of token t against ia_attn_fwd_x called with Lq = fold, Lk = t + 1 on the same device pointers;
    the two contexts lie within the sum of their bars"""
    Lk, fold, B = 33, 3, 2
    H = nh * 64
    Q, K, V, dO, refs, bars = operands(nh, Lk, fold, "normal")
    Lq = fold * Lk
    qd = rows_of(Q).cuda().contiguous()
    kv = torch.cat((rows_of(K), rows_of(V)), 1).cuda().contiguous()
    out = out_buf(B * Lq, H, 0)
    lse2 = torch.zeros(B * nh * Lq, dtype=F32, device="cuda")
    ok(lib.ia_attn_fwd_causal_x(qd.data_ptr(), H, kv.data_ptr(), kv.data_ptr() + 2 * H, 2 * H, out.data_ptr(), H, lse2.data_ptr(), B, nh, Lk,
                                fold, SCALE, st()), "ia_attn_fwd_causal_x")
    causal = heads_of(out[:B * Lq].cpu(), B, nh, Lq)
    worst = 0.0
    for b in range(B):
        for t in range(Lk):
            xo = out_buf(fold, H, 0)
            xl = torch.zeros(nh * fold, dtype=F32, device="cuda")
            row0 = b * Lq + t * fold
            ok(lib.ia_attn_fwd_x(qd.data_ptr() + row0 * H * 2, H, kv.data_ptr() + b * Lk * 2 * H * 2, kv.data_ptr() + b * Lk * 2 * H * 2 + 2 * H,
                                 2 * H, None, xo.data_ptr(), H, xl.data_ptr(), 1, nh, fold, t + 1, SCALE, 0.0, 0, st()), "ia_attn_fwd_x")
            untouched("x ctx", xo, fold, H)
            x_ctx = heads_of(xo[:fold].cpu(), 1, nh, fold)[0]
            sl = slice(t * fold, (t + 1) * fold)
            ops = (Q[b][:, sl], K[b][:, :t + 1], V[b][:, :t + 1], dO[b][:, sl])
            xbar = A.bars(*ops, SCALE, A.attn_ref(*ops, SCALE))["ctx"]
            bound = xbar + bars[b]["ctx"][:, sl]
            err = (A.d(x_ctx) - A.d(causal[b][:, sl])).abs()
            assert bool((err[bound == 0] == 0).all()), (b, t)
            nz = bound > 0
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
    print(f"[causal] x-form cross-check nh={nh}: max |causal - x| / (bar + bar) = {worst:.3f}")
    note(f"nh={nh} Lk={Lk} fold={fold}", {"x-form ctx": worst})
    assert worst <= 1.0, worst


def test_zz_print_the_largest_ratios(lib):
    """the largest error / bound per output over everything this module ran (`-s` shows it; the figures DESIGN.md quotes)"""
    assert RATIOS, "run the whole module"
    for key, (r, name) in sorted(RATIOS.items()):
        print(f"[causal] largest {key}: {r:.3f}  ({name})")
    assert all(r <= 1.0 for r, _ in RATIOS.values())
