"""The attention entry points of csrc/attention.hip through the C ABI against the fp64 reference of tests/attn_reference.py, element by
element for ctx, lse2, dq, dk and dv, within the derived bars of attn_reference.bars (checked on the host against a CPU model of the
kernels' rounding by tests/test_attn_reference_host.py; never fitted to a GPU result).  Every call runs on sentinel-filled outputs with
pad columns and 64 guard rows that have to come back bit-unchanged.  Every comparison prints max error / bound (`-s` shows them).

The dispatch follows the shape alone (launch_fwd, fused_applies) plus IA_ATTN_EXACT_DELTA, so the kernels under test are all the file
has: attn_fwd3_kernel<*, 1 | 2>, attn_bwd_fused_kernel (33 <= L <= 256), attn_bwd3_dq / _dkv / _delta_kernel.
"""
import math
import os

import numpy as np
import pytest
import torch

import attn_reference as A

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SCALE = 0.125
ERR_ARG, ERR_WS = -1, -3
SENT = -7.0            # sentinel of the bf16 outputs (pad columns, guard rows)
GUARD = 64
RATIOS = {}


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


def note(form, ratios):
    for key, r in ratios.items():
        RATIOS[(form, key)] = max(RATIOS.get((form, key), 0.0), r)


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


def run(lib, Q, K, V, dO, masks=None, p=0.0, seed=0, form="self", flags=0, packed_in=True, pad_o=0, pad_dq=0, pad_dkv=None, lens=None,
        bwd=True):
    """One forward (+ backward) through the entry points of `form`:
      self      ia_attn_fwd / ia_attn_bwd            bias  ia_attn_fwd / ia_attn_bwd_bias        ex  ia_attn_fwd[_ps] / ia_attn_bwd_bias_ex(flags)
      ps        ia_attn_fwd_ps / ia_attn_bwd_bias_ps x     ia_attn_fwd_x / ia_attn_bwd_x
      varlen    ia_attn_fwd_varlen / ia_attn_bwd_varlen    varlen_ps  the _ps pair (lens = the sequence lengths, Q .. dO hold Lmax rows)
    Q, dO [B, nh, Lq, 64], K, V [B, nh, Lk, 64] bf16 host tensors; masks [B, Lk] bool or None.  Returns a dict of host tensors in the
    same [B, nh, L, 64] shape (varlen: rows past a sequence's length are zero), lse2 [B, nh, Lq], dbias, delta."""
    B, nh, Lq, _ = Q.shape
    Lk = K.shape[2]
    H = nh * 64
    pad_dkv = pad_dq if pad_dkv is None else pad_dkv
    varlen = form.startswith("varlen")
    if varlen:
        cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
        T = int(cu[-1])
        pack = lambda x: torch.cat([rows_of(x[b:b + 1, :, :n]) for b, n in enumerate(lens)] + [torch.zeros(0, H, dtype=BF16)])
        qr, kr, vr, gr = pack(Q), pack(K), pack(V), pack(dO)
        Tq = Tk = T
        cu_d = cu.cuda()
    else:
        qr, kr, vr, gr = rows_of(Q), rows_of(K), rows_of(V), rows_of(dO)
        Tq, Tk = B * Lq, B * Lk
    if packed_in and Lq == Lk:
        qkv = torch.cat((qr, kr, vr), 1).cuda().contiguous()
        qp, kp, vp, ld = qkv.data_ptr(), qkv.data_ptr() + 2 * H, qkv.data_ptr() + 4 * H, 3 * H
        ld_q = ld_kv = ld
    else:
        qd, kd, vd = qr.cuda().contiguous(), kr.cuda().contiguous(), vr.cuda().contiguous()
        qp, kp, vp, ld_q, ld_kv = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), H, H
        ld = H
    mk = None if masks is None else masks.to(torch.uint8).cuda().contiguous()
    mp = None if mk is None else mk.data_ptr()
    out = out_buf(Tq, H, pad_o)
    lse2 = torch.full((B, nh, Lq), float("nan"), dtype=F32, device="cuda")
    ps = form in ("ps", "varlen_ps") or (form == "ex" and (flags & 1))
    if varlen:
        fn = lib.ia_attn_fwd_varlen_ps if ps else lib.ia_attn_fwd_varlen
        ok(fn(qp, kp, vp, ld, cu_d.data_ptr(), T, out.data_ptr(), H + pad_o, lse2.data_ptr(), B, nh, Lq, SCALE, p, seed, st()), form)
    elif form == "x":
        ok(lib.ia_attn_fwd_x(qp, ld_q, kp, vp, ld_kv, mp, out.data_ptr(), H + pad_o, lse2.data_ptr(), B, nh, Lq, Lk, SCALE, p, seed, st()), form)
    else:
        fn = lib.ia_attn_fwd_ps if ps else lib.ia_attn_fwd
        ok(fn(qp, kp, vp, ld, mp, out.data_ptr(), H + pad_o, lse2.data_ptr(), B, nh, Lq, SCALE, p, seed, st()), form)
    untouched(form + " ctx", out, Tq, H)
    res = {"lse2": lse2.cpu()}
    if not bwd:
        res["ctx_rows"] = out[:Tq, :H].cpu()
    else:
        g = torch.full((Tq + GUARD, H + pad_o), SENT, dtype=BF16, device="cuda")
        g[:Tq, :H] = gr.cuda()
        delta = torch.zeros(B * nh * Lq + 64, dtype=F32, device="cuda")
        dq, dk, dv = out_buf(Tq, H, pad_dq), out_buf(Tk, H, pad_dkv), out_buf(Tk, H, pad_dkv)
        common = (out.data_ptr(), g.data_ptr(), H + pad_o, lse2.data_ptr(), delta.data_ptr())
        if varlen:
            fn = lib.ia_attn_bwd_varlen_ps if ps else lib.ia_attn_bwd_varlen
            ok(fn(qp, kp, vp, ld, cu_d.data_ptr(), T, *common, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), H + pad_dq, B, nh, Lq, SCALE, p, seed,
                  st()), form)
        elif form == "x":
            ok(lib.ia_attn_bwd_x(qp, ld_q, kp, vp, ld_kv, mp, *common, dq.data_ptr(), H + pad_dq, dk.data_ptr(), dv.data_ptr(), H + pad_dkv, B, nh,
                                 Lq, Lk, SCALE, p, seed, st()), form)
        elif form == "self":
            ok(lib.ia_attn_bwd(qp, kp, vp, ld, mp, *common, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), H + pad_dq, B, nh, Lq, SCALE, p, seed,
                               st()), form)
        else:
            wsb = lib.ia_attn_bwd_bias_workspace_bytes(B, nh, Lq)
            assert wsb == B * ((Lq + 127) // 128) * 3 * H * 4
            ws = torch.zeros(wsb // 4 + 16, dtype=F32, device="cuda")
            dbias = torch.zeros(3 * H, dtype=F32, device="cuda")
            tail = (dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), H + pad_dq, dbias.data_ptr(), ws.data_ptr(), wsb, B, nh, Lq, SCALE, p, seed, st())
            if form == "bias":
                ok(lib.ia_attn_bwd_bias(qp, kp, vp, ld, mp, *common, *tail), form)
            elif form == "ps":
                ok(lib.ia_attn_bwd_bias_ps(qp, kp, vp, ld, mp, *common, *tail), form)
            else:
                ok(lib.ia_attn_bwd_bias_ex(flags, qp, kp, vp, ld, mp, *common, *tail), form)
            res["dbias"] = dbias.cpu()
            assert bool((ws[wsb // 4:] == 0).all()), "the workspace was written past its stated size"
        untouched(form + " dq", dq, Tq, H)
        untouched(form + " dk", dk, Tk, H)
        untouched(form + " dv", dv, Tk, H)
        assert bool((g[Tq:] == SENT).all()) and bool((out[Tq:] == SENT).all())
        res["delta"] = delta[:B * nh * Lq].reshape(B, nh, Lq).cpu()
        res["rows"] = {"dq": dq[:Tq, :H].cpu(), "dk": dk[:Tk, :H].cpu(), "dv": dv[:Tk, :H].cpu()}
    rows = {"ctx": out[:Tq, :H].cpu()}
    rows.update(res.get("rows", {}))
    for key, r in rows.items():
        if varlen:
            full = torch.zeros(B, nh, Lq, 64, dtype=BF16)
            c0 = 0
            for b, n in enumerate(lens):
                full[b, :, :n] = heads_of(r[c0:c0 + n], 1, nh, n)[0]
                c0 += n
            res[key] = full
        else:
            res[key] = heads_of(r, B, nh, Lq if key in ("ctx", "dq") else Lk)
    return res


def check(lib, name, fam, B, nh, Lq, Lk=None, kinds=("none",), p=0.0, seed=0, form="self", exact=False, dead_dO=False, flags=0, lens=None, **layout):
    """the operands of `fam`, one key mask kind per sequence, through `form`; every sequence against the reference within the bars"""
    Lk = Lq if Lk is None else Lk
    ops = [A.family(fam, nh, Lq, Lk, 100 * seed + 7 * b + 1) for b in range(B)]
    Q, K, V, dO = (torch.stack([o[i] for o in ops]) for i in range(4))
    ps = form in ("ps", "varlen_ps") or (form == "ex" and (flags & 1))
    if ps:       # what ia_gemm_bf16_qscale hands over: q * scale * log2(e) rounded to bf16 once; the reference takes it as given
        Q = A.bf(Q.to(F32) * float(np.float32(SCALE) * np.float32(A.LOG2E)))
    masks = None
    if any(kd != "none" for kd in kinds):
        masks = torch.stack([torch.ones(Lk, dtype=torch.bool) if kd == "none" else A.mask_of(kd, Lk) for kd in kinds])
    if dead_dO and masks is not None:
        dO = dO * masks[:, None, :, None].to(BF16)
    got = run(lib, Q, K, V, dO, masks, p, seed, form, flags=flags, lens=lens, **layout)
    inv_keep = A.drop_params(p)[1]
    worst = {}
    for b in range(B):
        nq = nk = None
        if lens is not None:
            nq = nk = lens[b]
            if nq == 0:
                continue
        sl_q, sl_k = slice(0, nq), slice(0, nk)
        q, k, v, g = Q[b][:, sl_q], K[b][:, sl_k], V[b][:, sl_k], dO[b][:, sl_q]
        m = None if masks is None else masks[b]
        keep = A.keep_tensor(seed, b, nh, q.shape[1], k.shape[1], p) if p > 0 else None
        ref = A.attn_ref(q, k, v, g, SCALE, m, keep, inv_keep, q_prescaled=ps)
        bar = A.bars(q, k, v, g, SCALE, ref, exact_delta=exact, q_prescaled=ps)
        gb = {"ctx": got["ctx"][b][:, sl_q], "lse2": got["lse2"][b][:, sl_q], "dq": got["dq"][b][:, sl_q], "dk": got["dk"][b][:, sl_k],
              "dv": got["dv"][b][:, sl_k]}
        r = A.compare(f"{name} seq {b}", gb, ref, bar)
        if exact:
            want, bound = A.delta_exact_ref(q, k, v, g, SCALE, gb["lse2"], m, keep, inv_keep, q_prescaled=ps)
            r["delta"] = A.ratio(f"{name} seq {b} delta", got["delta"][b][:, sl_q], want, bound)
            assert r["delta"] <= 1.0
        for key, x in r.items():
            worst[key] = max(worst.get(key, 0.0), x)
    if "dbias" in got:
        # the column sums are taken from the rows as stored: fp64 sums of the stored bf16 rows, c 2^-24 S with c = 4 rows per lane + 3
        # folds + 3 levels over the waves + 2 spare, then one sequential fold over the B * ceil(L / 128) workspace rows
        c = 12 + B * ((Lq + 127) // 128)
        stored = torch.cat([got["rows"][key].to(F64).sum(0) for key in ("dq", "dk", "dv")])
        S = torch.cat([got["rows"][key].to(F64).abs().sum(0) for key in ("dq", "dk", "dv")])
        worst["dbias"] = A.ratio(f"{name} dbias", got["dbias"], stored, c * A.E * S)
        assert worst["dbias"] <= 1.0
    # the figures are bucketed by launch_fwd / fused_applies as read off attention.hip: the forward form follows the launch's Lq (the
    # packed forms launch with Lmax), the fused backward serves padded Lq == Lk in 33 .. 256 without exact delta, the packed forms
    # (not in the list below) and everything else run the pair
    fwd_form = "fwd 256q" if ((Lq - 1) & 255) >= 128 else "fwd 128q"
    bwd_form = "bwd delta+pair" if exact else ("bwd fused" if (form in ("self", "bias", "ps", "ex", "x") and Lq == Lk and 32 < Lq <= 256) else "bwd pair")
    note(fwd_form, {k_: v_ for k_, v_ in worst.items() if k_ in ("ctx", "lse2")})
    note(bwd_form, {k_: v_ for k_, v_ in worst.items() if k_ not in ("ctx", "lse2")})
    return got, (Q, K, V, dO, masks)


# =============================================================================================================== lengths
LENGTHS = [1, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 384, 385, 513, 577, 769]


@pytest.mark.parametrize("L", LENGTHS)
def test_lengths_normal(lib, L):
    """both forward forms on either side of ((L - 1) & 255) < 128, the fused backward's 33 .. 256 window and the pair outside it;
    sequence 0 without a mask, sequence 1 with a prefix mask; the bias-gradient form"""
    check(lib, f"L={L}", "normal", 2, 2, L, kinds=("none", "prefix"), form="bias", seed=L)


@pytest.mark.parametrize("L", [129, 300])
@pytest.mark.parametrize("fam", ["peaked", "rising", "falling", "uniform", "equalv"])
def test_families(lib, fam, L):
    """`rising` / `falling` force rebase() (tests/test_attn_reference_host.py::test_rebase_families_cross_the_thresholds shows that these
    operands leave [2^-100, 2^60]: with something accumulated, in the first block of a tile, and with nothing accumulated;
    ::test_fault_rebase_families_have_teeth that zeros and probabilities 2^+-0.25 off fall outside the bars used here); `equalv` has
    dq = dk = 0 in the reference, so their bars hold no |want| term"""
    got, _ = check(lib, f"{fam} L={L}", fam, 2, 2, L, form="self", seed=3)
    if fam == "equalv":
        assert float(got["dq"].abs().max()) < 2.0 ** -6 and float(got["dk"].abs().max()) < 2.0 ** -6


@pytest.mark.parametrize("L", [100, 200, 385])
@pytest.mark.parametrize("kind", A.MASKS[1:])
def test_masks(lib, kind, L):
    """a hole, whole 64-key tiles masked (first / middle / last), one attendable key (bar 0: ctx is that v row bit for bit), alternating"""
    got, (Q, K, V, dO, masks) = check(lib, f"{kind} L={L}", "normal", 2, 2, L, kinds=(kind, "none"), form="bias", seed=5)
    if kind == "one_key":
        j = int(masks[0].nonzero()[0])
        assert torch.equal(got["ctx"][0], V[0][:, j:j + 1].expand(-1, L, -1))


@pytest.mark.parametrize("L", [20, 200, 300])
def test_sequence_without_attendable_key(lib, L):
    """Pinned: such a sequence gets ctx = 0, lse2 = 0, dq = dk = dv = 0 (the reference project's additive finfo.min mask gives a uniform
    average instead); the other sequences are bit-identical to a run without it, everything is finite."""
    got, (Q, K, V, dO, masks) = check(lib, f"dead L={L}", "normal", 3, 2, L, kinds=("prefix", "dead", "none"), form="self", seed=8)
    for key in ("ctx", "lse2", "dq", "dk", "dv"):
        assert torch.isfinite(got[key].to(F32)).all(), key
        assert (got[key][1] == 0).all(), key
    keep = [0, 2]
    alone = run(lib, Q[keep], K[keep], V[keep], dO[keep], masks[keep], form="self")
    for key in ("ctx", "lse2", "dq", "dk", "dv"):
        assert torch.equal(got[key][keep], alone[key]), key


# =============================================================================================================== entry points
@pytest.mark.parametrize("L", [64, 200, 300])
def test_prescaled_forms_from_gemm_qscale(lib, L):
    """q columns written by ia_gemm_bf16_qscale, then ia_attn_fwd_ps / ia_attn_bwd_bias_ps; the reference takes the stored q' as given"""
    from item_alignment_amd import ops
    B, nh, H, Kd = 2, 2, 128, 64
    g = A.gen(L)
    x = A.bf(torch.randn(B * L, Kd, generator=g)).cuda()
    w = A.bf(torch.randn(3 * H, Kd, generator=g) * Kd ** -0.5).cuda()
    bias = torch.randn(3 * H, generator=g).cuda()
    qkv = ops.gemm_qscale(x, w, bias, H, float(np.float32(SCALE) * np.float32(A.LOG2E))).cpu()
    Q, K, V = (heads_of(qkv[:, i * H:(i + 1) * H], B, nh, L).contiguous() for i in range(3))
    dO = torch.stack([A.family("normal", nh, L, L, 50 + b)[3] for b in range(B)])
    masks = torch.stack([A.mask_of("prefix", L), torch.ones(L, dtype=torch.bool)])
    got = run(lib, Q, K, V, dO, masks, form="ps")
    for b in range(B):
        ref = A.attn_ref(Q[b], K[b], V[b], dO[b], SCALE, masks[b], q_prescaled=True)
        bar = A.bars(Q[b], K[b], V[b], dO[b], SCALE, ref, q_prescaled=True)
        r = A.compare(f"ps L={L} seq {b}", {key: got[key][b] for key in ("ctx", "lse2", "dq", "dk", "dv")}, ref, bar)
        note("ps forms", r)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("L", [200, 300])
def test_bwd_bias_ex_flags(lib, flags, L):
    """IA_ATTN_Q_PRESCALED and IA_ATTN_MASKED_ROWS_DEAD (dO zero at the masked positions, as the flag requires)"""
    check(lib, f"ex flags={flags} L={L}", "normal", 2, 2, L, kinds=("prefix", "prefix"), form="ex", flags=flags, dead_dO=bool(flags & 2), seed=6)


@pytest.mark.parametrize("Lq,Lk,kind,p", [(70, 200, "none", 0.0), (200, 70, "hole", 0.0), (33, 257, "prefix", 0.25), (130, 129, "alternating", 0.1),
                                          (70, 2047, "none", 0.0), (70, 2048, "hole", 0.1)])
def test_cross_attention(lib, Lq, Lk, kind, p):
    """ia_attn_fwd_x / ia_attn_bwd_x with Lq != Lk, a key mask, dropout, up to the Lk = 2048 limit; ld_dq != ld_dkv"""
    check(lib, f"x {Lq}x{Lk} {kind} p={p}", "normal", 2, 1 if Lk > 2000 else 2, Lq, Lk, kinds=(kind, "none"), p=p, seed=21, form="x", packed_in=False,
          pad_o=64, pad_dq=8, pad_dkv=64)


@pytest.mark.parametrize("form", ["varlen", "varlen_ps"])
def test_packed_sequences(lib, form):
    """ragged lengths with a length-1 and a zero-length sequence.  Pinned for the zero-length one: no token row exists, nothing is
    written for it, the other sequences are as if it were absent; its lse2 / delta rows are not looked at."""
    lens = [70, 1, 0, 300, 33]
    got, (Q, K, V, dO, _) = check(lib, f"{form}", "normal", len(lens), 2, max(lens), form=form, lens=lens, seed=9, pad_o=64, pad_dq=64)
    keep = [0, 1, 3, 4]
    alone = run(lib, Q[keep], K[keep], V[keep], dO[keep], form=form, lens=[lens[b] for b in keep], pad_o=64, pad_dq=64)
    for i, b in enumerate(keep):
        for key in ("ctx", "lse2", "dq", "dk", "dv"):
            assert torch.equal(got[key][b][:, :lens[b]], alone[key][i][:, :lens[b]]), (key, b)
    check(lib, f"{form} p=0.1", "half", len(lens), 2, max(lens), form=form, lens=lens, p=0.1, seed=10)


# =============================================================================================================== dropout
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("L", [100, 300])
def test_dropout_against_the_replica(lib, p, L):
    check(lib, f"dropout p={p} L={L}", "normal", 2, 2, L, kinds=("hole", "none"), p=p, seed=31, form="bias")


@pytest.mark.parametrize("p", [0.1, 0.25])
def test_recovered_mask_is_the_replica(lib, p):
    """the one-hot-V trick of the older tests (ctx[i, j] = P_ij keep_ij / keep) gives the replica's keep matrix bit for bit"""
    B, nh, L = 2, 2, 64
    ops = [A.family("half", nh, L, L, 60 + b) for b in range(B)]
    Q, K, _, dO = (torch.stack([o[i] for o in ops]) for i in range(4))
    V = torch.eye(64).to(BF16)[None, None].expand(B, nh, L, 64).contiguous()
    for seed in (0, 12345):
        got = run(lib, Q, K, V, dO, p=p, seed=seed, bwd=False)
        ctx = heads_of(got["ctx_rows"], B, nh, L)
        for b in range(B):
            assert torch.equal(ctx[b] != 0, A.keep_tensor(seed, b, nh, L, L, p)), (seed, b)


# =============================================================================================================== exact delta
@pytest.mark.parametrize("L", [129, 300])
@pytest.mark.parametrize("fam", ["uniform", "normal"])
def test_exact_delta(lib, fam, L):
    """IA_ATTN_EXACT_DELTA=1 (read on every call) against the bar without the rowsum(dO o O^) term; the delta it returns against fp64
    sum_k P dP within c 2^-24 S"""
    old = os.environ.get("IA_ATTN_EXACT_DELTA")
    os.environ["IA_ATTN_EXACT_DELTA"] = "1"
    try:
        check(lib, f"exact delta {fam} L={L}", fam, 2, 2, L, kinds=("none", "prefix"), form="self", exact=True, seed=4)
        check(lib, f"exact delta {fam} L={L} p=0.1", fam, 2, 2, L, p=0.1, form="self", exact=True, seed=4)
    finally:
        if old is None:
            del os.environ["IA_ATTN_EXACT_DELTA"]
        else:
            os.environ["IA_ATTN_EXACT_DELTA"] = old


# =============================================================================================================== layouts
@pytest.mark.parametrize("L", [65, 300])
def test_layouts(lib, L):
    """packed [T, 3H] and three separate tensors give the same bits; ld_o = H + 64 and padded gradient rows; pad columns and guard rows
    are checked inside run()"""
    a, _ = check(lib, f"packed L={L}", "normal", 2, 2, L, kinds=("hole", "none"), form="self", seed=2, packed_in=True)
    b, _ = check(lib, f"separate L={L}", "normal", 2, 2, L, kinds=("hole", "none"), form="self", seed=2, packed_in=False, pad_o=64, pad_dq=8)
    for key in ("ctx", "lse2", "dq", "dk", "dv"):
        assert torch.equal(a[key], b[key]), key


# =============================================================================================================== refusals
def test_refusals(lib):
    """every call is rejected by the host code in front of its first launch: the buffer stays zero"""
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, s = buf.data_ptr(), None
    ws = lib.ia_attn_bwd_bias_workspace_bytes(1, 1, 8)
    assert lib.ia_attn_bwd_bias_workspace_bytes(0, 1, 8) == 0 and lib.ia_attn_bwd_bias_workspace_bytes(1, 1, -1) == 0
    fwd = [p, p, p, 64, None, p, 64, p, 1, 1, 8, SCALE, 0.0, 0, s]
    bwd = [p, p, p, 64, None, p, p, 64, p, p, p, p, p, 64, 1, 1, 8, SCALE, 0.0, 0, s]
    bias = [p, p, p, 64, None, p, p, 64, p, p, p, p, p, 64, p, p, ws, 1, 1, 8, SCALE, 0.0, 0, s]
    fwdx = [p, 64, p, p, 64, None, p, 64, p, 1, 1, 8, 8, SCALE, 0.0, 0, s]
    bwdx = [p, 64, p, p, 64, None, p, p, 64, p, p, p, 64, p, p, 64, 1, 1, 8, 8, SCALE, 0.0, 0, s]
    fvar = [p, p, p, 64, p, 8, p, 64, p, 1, 1, 8, SCALE, 0.0, 0, s]
    bvar = [p, p, p, 64, p, 8, p, p, 64, p, p, p, p, p, 64, 1, 1, 8, SCALE, 0.0, 0, s]
    A_ = ERR_ARG
    fwd_bad = [({0: None}, A_), ({1: None}, A_), ({2: None}, A_), ({5: None}, A_), ({8: 0}, A_), ({9: 0}, A_), ({10: 0}, A_), ({8: -1}, A_),
               ({10: 2049}, A_), ({3: 68}, A_), ({6: 68}, A_), ({3: 56}, A_), ({9: 2}, A_), ({8: 8192, 10: 2048}, A_)]
    bwd_bad = [({i: None}, A_) for i in (0, 1, 2, 5, 6, 8, 9, 10, 11, 12)] + [({14: 0}, A_), ({15: 0}, A_), ({16: 0}, A_), ({16: 2049}, A_),
               ({3: 68}, A_), ({7: 68}, A_), ({13: 68}, A_), ({13: 56}, A_), ({15: 2}, A_), ({14: 8192, 16: 2048}, A_)]
    bias_bad = [({i: None}, A_) for i in (0, 1, 2, 5, 6, 8, 9, 10, 11, 12, 14)] + [({15: None}, ERR_WS), ({16: ws - 1}, ERR_WS), ({16: 0}, ERR_WS),
                ({17: 0}, A_), ({18: 0}, A_), ({19: 0}, A_), ({3: 68}, A_), ({7: 68}, A_), ({13: 68}, A_), ({13: 56}, A_), ({19: 2049, 16: 1 << 20}, A_)]
    cases = [("ia_attn_fwd", fwd, fwd_bad), ("ia_attn_fwd_ps", fwd, fwd_bad), ("ia_attn_bwd", bwd, bwd_bad),
             ("ia_attn_bwd_bias", bias, bias_bad), ("ia_attn_bwd_bias_ps", bias, bias_bad),
             ("ia_attn_bwd_bias_ex", [0] + bias, [({k_ + 1: v_ for k_, v_ in ch.items()}, code) for ch, code in bias_bad]
              + [({0: 4}, A_), ({0: 8 | 1}, A_), ({0: -1}, A_)]),
             ("ia_attn_fwd_x", fwdx, [({0: None}, A_), ({2: None}, A_), ({3: None}, A_), ({6: None}, A_), ({9: 0}, A_), ({10: 0}, A_), ({11: 0}, A_),
                                      ({12: 0}, A_), ({12: 2049}, A_), ({1: 68}, A_), ({4: 68}, A_), ({7: 68}, A_), ({4: 56}, A_), ({10: 2}, A_),
                                      ({9: 8192, 11: 2048}, A_), ({9: 8192, 12: 2048}, A_)]),
             ("ia_attn_bwd_x", bwdx, [({i: None}, A_) for i in (0, 2, 3, 6, 7, 9, 10, 11, 13, 14)]
              + [({16: 0}, A_), ({17: 0}, A_), ({18: 0}, A_), ({19: 0}, A_), ({19: 2049}, A_), ({12: 68}, A_), ({15: 68}, A_), ({12: 56}, A_),
                 ({15: 56}, A_), ({1: 68}, A_), ({4: 68}, A_), ({8: 68}, A_)]),
             ("ia_attn_fwd_varlen", fvar, [({0: None}, A_), ({4: None}, A_), ({6: None}, A_), ({5: 0}, A_), ({9: 0}, A_), ({10: 0}, A_), ({11: 0}, A_),
                                           ({11: 2049}, A_), ({3: 68}, A_), ({7: 68}, A_), ({5: 1 << 24}, A_)]),
             ("ia_attn_fwd_varlen_ps", fvar, [({1: None}, A_), ({4: None}, A_), ({5: -1}, A_), ({11: 2049}, A_)]),
             ("ia_attn_bwd_varlen", bvar, [({i: None}, A_) for i in (0, 4, 6, 7, 9, 10, 11, 12, 13)]
              + [({5: 0}, A_), ({15: 0}, A_), ({16: 0}, A_), ({17: 0}, A_), ({17: 2049}, A_), ({14: 68}, A_), ({14: 56}, A_), ({5: 1 << 24}, A_)]),
             ("ia_attn_bwd_varlen_ps", bvar, [({2: None}, A_), ({4: None}, A_), ({17: 2049}, A_), ({14: 68}, A_)])]
    n = 0
    for name, base, bad in cases:
        fn = getattr(lib, name)
        assert len(base) == len(fn.argtypes), name
        for change, code in bad:
            args = list(base)
            for i, v in change.items():
                args[i] = v
            assert fn(*args) == code, (name, change, code)
            n += 1
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0
    print(f"[attn] refusals: {n} calls over {len(cases)} entry points")


def test_zz_print_the_largest_ratios():
    """the largest error / bound per kernel form and output seen by this run (recorded in DESIGN.md; no input to any bar)"""
    for (form, key), r in sorted(RATIOS.items()):
        print(f"[attn] largest ratio  {form:16s} {key:6s} {r:.3f}")
