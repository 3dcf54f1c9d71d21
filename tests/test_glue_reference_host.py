"""tests/glue_reference.py against torch's own operators and autograd, all in fp64, on small inputs (no GPU): two fp64
implementations of one formula agree to 1e-12 relative; and the host replica of the dropout hash keeps the fraction of elements it
should.  This is what makes the references of tests/test_glue_kernels_gpu.py trustworthy where there is no GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_reference as R

F64 = torch.float64
TOL = 1e-12


def close(a, b):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= TOL * max(b.abs().max().item(), 1.0), err


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def test_embedding_sum_layernorm_and_backward():
    M, H, V, T, P, E, word_pad, pos_pad = 23, 24, 11, 2, 9, 4, 1, 1
    g = torch.Generator().manual_seed(1)
    ids, tts, pids = torch.randint(0, V, (M,), generator=g), torch.randint(0, T, (M,), generator=g), torch.randint(0, P, (M,), generator=g)
    xi = torch.full((M,), -1, dtype=torch.int32)
    xi[[2, 5, 6, 20]] = torch.tensor([3, 0, 3, 1], dtype=torch.int32)
    word, typ, pos, extra = (rnd(n, H, seed=s).requires_grad_() for n, s in ((V, 2), (T, 3), (P, 4), (E, 5)))
    gamma, beta = (rnd(H, seed=6) + 2).requires_grad_(), rnd(H, seed=7).requires_grad_()
    # torch: nn.Embedding with padding_idx (no gradient to that row), extra rows spliced over the word rows, F.layer_norm
    w = F.embedding(ids, word, padding_idx=word_pad)
    w = torch.where((xi >= 0)[:, None], extra[xi.clamp(min=0).long()], w)
    z = w + F.embedding(tts, typ) + F.embedding(pids, pos, padding_idx=pos_pad)
    z.retain_grad()
    y = F.layer_norm(z, (H,), gamma, beta, 1e-5)
    dy = rnd(M, H, seed=8)
    y.backward(dy)

    zr = R.embed_sum(ids, tts, pids, xi, word, typ, pos, extra)
    close(zr, z.detach())
    yr, mean, rstd = R.layernorm_fwd(zr, gamma, beta, 1e-5)
    close(yr, y.detach())
    close(mean, z.detach().mean(1))
    close(rstd, 1 / torch.sqrt(z.detach().var(1, unbiased=False) + 1e-5))
    dz, dgamma, dbeta = R.layernorm_bwd(dy, zr, mean, rstd, gamma)
    close(dz, z.grad)
    close(dgamma, gamma.grad)
    close(dbeta, beta.grad)
    tabs = R.embed_table_grads(dz, ids, tts, pids, xi, V, T, P, E, word_pad, pos_pad)
    for k, p in (("word", word), ("type", typ), ("pos", pos), ("extra", extra)):
        close(tabs[k], p.grad)
    assert tabs["word"][word_pad].abs().max() == 0 and tabs["pos"][pos_pad].abs().max() == 0


def test_patch_im2col_is_the_patch_embed_convolution():
    B, C, S, P, N = 2, 3, 16, 8, 5
    img, w = rnd(B, C, S, S, seed=1), rnd(N, C, P, P, seed=2)
    cols = R.im2col_patch(img, P)
    close(cols, F.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, C * P * P))          # unfold's column order is (c, ph, pw)
    close((cols @ w.reshape(N, -1).t()).reshape(B, -1, N), F.conv2d(img, w, stride=P).flatten(2).transpose(1, 2))


def test_vit_tokens_and_backward():
    B, NP, H = 3, 4, 8
    patch, cls, pos = rnd(B, NP, H, seed=1).requires_grad_(), rnd(H, seed=2).requires_grad_(), rnd(NP + 1, H, seed=3).requires_grad_()
    tok = torch.cat((cls.expand(B, 1, H), patch), 1) + pos
    close(R.vit_tokens(patch, cls, pos), tok.detach())
    dtok = rnd(B, NP + 1, H, seed=4)
    tok.backward(dtok)
    dpatch, dcls, dpos = R.vit_tokens_bwd(dtok)
    close(dpatch, patch.grad), close(dcls, cls.grad), close(dpos, pos.grad)


def test_row_gather():
    src, rows = rnd(9, 5, seed=1), torch.tensor([8, 0, 3], dtype=torch.int32)
    close(R.gather_rows(src, rows), torch.index_select(src, 0, rows.long()))


def test_span_mean_with_overlapping_spans_and_backward():
    L, H = 6, 8
    seq = rnd(3 * L, H, seed=1).requires_grad_()
    spans = torch.tensor([[0, 1], [1, 5], [3, 6], [12, 18]], dtype=torch.int32)        # sample 0: length 1 + two overlapping; 1: none; 2: all L
    out = torch.stack([seq[a:b].mean(0) for a, b in spans.tolist()])
    close(R.span_mean(seq, spans), out.detach())
    dout = rnd(4, H, seed=2)
    out.backward(dout)
    dseq = R.span_mean_bwd(dout, spans, 3 * L)
    close(dseq, seq.grad)
    assert dseq[L:2 * L].abs().max() == 0 and dseq[5].abs().max() > 0


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_pair_head_cross_entropy_and_backward(two, C):
    B, D = 7, 10
    x, y = rnd(B, D, seed=1).requires_grad_(), (rnd(B, D, seed=2).requires_grad_() if two else None)
    W, b = rnd(C, 2 * D if two else D, seed=3, scale=3.0).requires_grad_(), rnd(C, seed=4).requires_grad_()
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(5))
    f = torch.cat((x, y), 1) if two else x
    logits = F.linear(f, W, b)
    loss = F.cross_entropy(logits, labels)
    (loss * 0.7).backward()
    lr, pr, lossr = R.pair_head_ce(x, y, W, b, labels)
    close(lr, logits.detach()), close(pr, F.softmax(logits.detach(), 1)), close(lossr, loss.detach())
    assert R.pair_head_ce(x, y, W, b, None)[2] is None
    dx, dy, dW, db = R.pair_head_ce_bwd(pr, labels, 0.7, x, y, W)
    close(dx, x.grad), close(dW, W.grad), close(db, b.grad)
    if two:
        close(dy, y.grad)
    else:
        assert dy is None


def test_pair_head_softmax_survives_logits_of_80():
    x = torch.tensor([[80.0, 0.0], [-80.0, 0.0]], dtype=F64)
    W = torch.tensor([[1.0, 0.0], [-1.0, 0.0]], dtype=F64)
    lg, pr, loss = R.pair_head_ce(x, None, W, None, torch.tensor([0, 0]))
    assert torch.isfinite(pr).all() and torch.isfinite(loss)
    close(loss, F.cross_entropy(lg, torch.tensor([0, 0])))


def test_kg_gather_and_rows():
    B, P, Dk, NE, NR = 4, 3, 8, 6, 5
    ent, rel = rnd(NE, Dk, seed=1), rnd(NR, Dk, seed=2).requires_grad_()
    ent[2, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=F64)
    ids = torch.tensor([[9, 2, 0, 1, 1, 7], [9, 0, 4, 4, 4, 7], [9, 5, 3, 0, 2, 7], [9, 2, 1, 1, 0, 7]])        # entity at column 1, relations from 2
    h, r = R.kg_gather(ent, rel, ids, 1, 2, P)
    close(h, torch.sign(ent[ids[:, 1]]))
    assert h[0, :4].tolist() == [0.0, 0.0, 1.0, -1.0]
    rt = F.embedding(ids[:, 2:2 + P].reshape(-1), rel)
    close(r, rt.detach())
    dr = rnd(B * P, Dk, seed=3)
    rt.backward(dr)
    close(R.kg_gather_bwd(dr, ids, 2, P, NR), rel.grad)

    hh, hp, rr = rnd(B, Dk, seed=4).requires_grad_(), rnd(B, Dk, seed=5).requires_grad_(), rnd(B * P, Dk, seed=6).requires_grad_()
    r3 = rr.reshape(B, P, Dk)
    rows = torch.cat((hh[:, None] + r3, hp[:, None] - r3), 1)
    close(R.kg_rows(hh, rr, hp), rows.detach())
    g = rnd(B, 2 * P, Dk, seed=7)
    rows.backward(g)
    dh, drr, dhp = R.kg_rows_bwd(g)
    close(dh, hh.grad), close(drr, rr.grad), close(dhp, hp.grad)


@pytest.mark.parametrize("measure", [R.SIM_INNER, R.SIM_COSINE, R.SIM_L1, R.SIM_L2])
@pytest.mark.parametrize("ups", ["both", "dsim", "dprobs"])
def test_similarity_measures_and_backward(measure, ups):
    B, D = 6, 13
    x, y = rnd(B, D, seed=1, scale=0.3).requires_grad_(), rnd(B, D, seed=2, scale=0.3).requires_grad_()
    sim, probs = R.pair_sim(x, y, measure)
    want = {R.SIM_INNER: lambda: (x * y).sum(1), R.SIM_COSINE: lambda: F.cosine_similarity(x, y, eps=1e-8),
            R.SIM_L1: lambda: F.pairwise_distance(x, y, p=1.0), R.SIM_L2: lambda: F.pairwise_distance(x, y, p=2.0)}[measure]()
    close(sim.detach(), want.detach())
    wantp = {R.SIM_INNER: torch.sigmoid(want), R.SIM_COSINE: (want + 1) / 2, R.SIM_L1: torch.exp(-want), R.SIM_L2: torch.exp(-want)}[measure]
    close(probs.detach(), wantp.detach())
    dsim = rnd(B, seed=3) if ups != "dprobs" else None
    dprobs = rnd(B, seed=4) if ups != "dsim" else None
    tot = (want * (dsim if dsim is not None else 0.0)).sum() + (wantp * (dprobs if dprobs is not None else 0.0)).sum()
    tot.backward()
    dx, dy = R.pair_sim_bwd(x, y, dsim, dprobs, measure)
    close(dx, x.grad), close(dy, y.grad)


def test_cosine_of_an_all_zero_row_is_zero():
    x, y = torch.zeros(1, 5, dtype=F64), rnd(1, 5, seed=1)
    s, p = R.pair_sim(x, y, R.SIM_COSINE)
    assert s.item() == 0.0 and p.item() == 0.5


@pytest.mark.parametrize("Cout,Cg,kk,Cgp", [(4, 3, 9, 8), (3, 8, 1, 8), (2, 16, 9, 16)])
def test_weight_standardisation_and_backward(Cout, Cg, kk, Cgp):
    scale, eps = 0.37, 1e-5
    w, gain = (rnd(Cout, Cg, kk, seed=1) * 0.1 + 0.5).requires_grad_(), (rnd(Cout, seed=2) + 2).requires_grad_()
    # timm ScaledStdConv2d: batch_norm over the fan-in as one "batch" of Cout channels, then * scale
    std = F.batch_norm(w.reshape(1, Cout, -1), None, None, weight=gain * scale, training=True, momentum=0.0, eps=eps).reshape(Cout, Cg, kk)
    what, mean, rstd = R.ws_weight(w, gain, scale, eps, Cgp)
    close(what[:, :, :Cg], std.detach().permute(0, 2, 1))
    assert what[:, :, Cg:].abs().sum() == 0
    close(mean, w.detach().reshape(Cout, -1).mean(1))
    close(rstd, 1 / torch.sqrt(w.detach().reshape(Cout, -1).var(1, unbiased=False) + eps))
    dwhat = rnd(Cout, kk, Cgp, seed=3)
    std.backward(dwhat[:, :, :Cg].permute(0, 2, 1))
    dw, dgain = R.ws_weight_bwd(dwhat, w, gain, mean, rstd, scale)
    close(dw, w.grad), close(dgain, gain.grad)


@pytest.mark.parametrize("H,W", [(8, 8), (7, 9), (1, 5), (5, 5)])
def test_ceil_mode_average_pool_and_backward(H, W):
    x = rnd(2, H, W, 3, seed=1).requires_grad_()
    y = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    close(R.avgpool2(x), y.detach())
    dy = rnd(*y.shape, seed=2)
    y.backward(dy)
    close(R.avgpool2_bwd(dy, H, W), x.grad)


def test_global_average_pool_and_backward():
    x = rnd(2, 7, 5, seed=1).requires_grad_()
    y = x.mean(1)
    close(R.gap(x), y.detach())
    g = rnd(2, 5, seed=2)
    y.backward(g)
    close(R.gap_bwd(g, 7), x.grad)


@pytest.mark.parametrize("use2,useadd", [(False, False), (True, False), (False, True), (True, True)])
def test_silu_with_scale_and_backward(use2, useadd):
    x = torch.cat((torch.linspace(-20, 20, 41, dtype=F64), torch.tensor([0.0, 88.0, -88.0], dtype=F64))).requires_grad_()
    scale = 1.7
    y = F.silu(x) * scale
    close(R.silu(x, scale), y.detach())
    dy, dy2, dadd = rnd(44, seed=1), (rnd(44, seed=2) if use2 else None), (rnd(44, seed=3) if useadd else None)
    # two consumers of y, and an identity path that bypasses the activation
    tot = (y * dy).sum() + ((y * dy2).sum() if use2 else 0.0) + ((x * dadd).sum() if useadd else 0.0)
    tot.backward()
    close(R.silu_bwd(dy, x, scale, dy2, dadd), x.grad)


def test_layout_changes():
    x = rnd(2, 3, 4, 5, seed=1)
    o = R.nchw_to_nhwc(x, 8)
    close(o[..., :3], x.permute(0, 2, 3, 1))
    assert o[..., 3:].abs().sum() == 0
    c = rnd(2, 3, 4, 8, seed=2)
    p = R.pad_rows(c, False, True)
    close(p, F.pad(c.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1))
    close(R.pad_rows(p, True, False), c)
    close(R.pad_rows(p, True, True), p)


def test_weight_pack_is_undone_by_unpack():
    Cout, Cg, kk, Cgp, ldw = 3, 3, 9, 8, 80
    w = rnd(Cout, Cg, kk, seed=1).requires_grad_()
    what = R.weight_pack(w, Cgp, ldw)
    for o, c, t in ((0, 0, 0), (2, 1, 5), (1, 2, 8)):
        assert what[o, t * Cgp + c] == w[o, c, t]
    assert int((what != 0).sum()) == w.numel()                        # nothing else is non-zero
    close(R.weight_unpack_grad(what, Cg, kk, Cgp), w.detach())
    # the gradient of sum(pack(w) * g) w.r.t. w is unpack(g)
    g = rnd(Cout, ldw, seed=2)
    wp = torch.zeros(Cout, kk, Cgp, dtype=F64)
    wp[:, :, :Cg] = w.permute(0, 2, 1)
    (wp.reshape(Cout, -1) * g[:, :kk * Cgp]).sum().backward()
    close(R.weight_unpack_grad(g, Cg, kk, Cgp), w.grad)


def test_bf16_round_is_round_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0], dtype=F64)
    assert R.bf16_round(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -0.0]


# ------------------------------------------------------------------------------------------------------------ dropout hash
def _mix32_scalar(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_hash_replica_matches_a_scalar_evaluation():
    """the vectorised numpy hash against the same two rounds written out with Python integers"""
    for seed, stream, idx in ((0, 0, 0), (12345, 7, 99), (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF), (2024, 3, 1 << 31)):
        want = _mix32_scalar(idx ^ _mix32_scalar(stream ^ ((seed * 0x9E3779B9) & 0xFFFFFFFF)))
        assert int(R.rng32(seed, stream, np.asarray([idx]))[0]) == want


def test_drop_params():
    assert R.drop_params(0.0) == (0, 1.0)
    thr, inv = R.drop_params(0.1)
    assert thr == 6554 and abs(inv - 1 / (1 - 6554 / 65536)) < 1e-6
    assert R.drop_params(0.5)[0] == 32768


# (seed, stream id) pairs the GPU tests draw their masks with
MASK_KEYS = [(1234, 0), (77, 3), (20240229, 11), (5, 1)]


@pytest.mark.parametrize("seed,stream", MASK_KEYS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_hash_keep_rate(seed, stream, p):
    n = 200000
    keep = R.keep_mask(seed, stream, n, p)
    thr, _ = R.drop_params(p)
    q = thr / 65536.0
    assert abs(int(keep.sum()) - n * (1 - q)) <= 5 * math.sqrt(n * q * (1 - q))
    # the two halves of one 32-bit draw are not tied to each other
    both = int((keep[0::2] & keep[1::2]).sum())
    m = n // 2
    pb = (1 - q) ** 2
    assert abs(both - m * pb) <= 5 * math.sqrt(m * pb * (1 - pb))
    # a mask that starts at an odd element is the same mask, shifted
    assert torch.equal(R.keep_mask(seed, stream, 1001, p, start=7), keep[7:1008])
