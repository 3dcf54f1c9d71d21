"""fp64 restatement of the TextCNN tower kernels (csrc/textcnn.hip) in plain torch / numpy, with no call into the HIP library: the tap
packing, the tap projection, the pool forward (relu + max over time, ties to the lowest t, dead features) and the hand-derived backward
(dW / db gather, dx row scatter).  Written from the formulas of include/itemalign.h and the reference's TextCNN.forward
(text.py:1516-1527); tests/test_textcnn_reference_host.py checks it against autograd of F.conv2d -> relu -> max_pool1d in fp64.

Layouts: weights[s] [F, 2, K_s, H], biases[s] [F]; x_c [B * L, H]; P [B * L, ld >= NT] with column n(s, k, f) = off_s + k F + f,
off_s = F (K_0 + .. + K_{s-1}); features j = s F + f.
"""
import numpy as np
import torch

import glue_reference as R

F64 = torch.float64


def parse_sizes(text):
    return [int(v) for v in text.split(",")]


def offsets(sizes, F):
    off, n = [], 0
    for K in sizes:
        off.append(n)
        n += F * K
    return off, n, (n + 7) & ~7          # per-size first column, NT, NTP


def pack_taps(weights, sizes):
    """[2, NTP, H] in the dtype of the weights: row n(s, k, f) of channel c = W_s[f, c, k, :], padding rows zero."""
    F, H = weights[0].shape[0], weights[0].shape[3]
    off, _nt, ntp = offsets(sizes, F)
    taps = torch.zeros((2, ntp, H), dtype=weights[0].dtype)
    for s, K in enumerate(sizes):
        for k in range(K):
            for c in range(2):
                taps[c, off[s] + k * F: off[s] + (k + 1) * F] = weights[s][:, c, k, :]
    return taps


def project(x0, x1, taps):
    """P [M, NTP] fp64 = x_0 taps_0^T + x_1 taps_1^T"""
    return R.d(x0) @ R.d(taps[0]).T + R.d(x1) @ R.d(taps[1]).T


def pre_activations(P, biases, sizes, B, L):
    """per filter size: (pre [B, T_s, F] fp64, sum of |terms| [B, T_s, F]), T_s = L - K_s + 1"""
    F = biases[0].shape[0]
    off, _nt, _ntp = offsets(sizes, F)
    P3 = R.d(P).reshape(B, L, -1)
    out = []
    for s, K in enumerate(sizes):
        T = L - K + 1
        b = R.d(biases[s])
        pre, mag = b.expand(B, T, F).clone(), b.abs().expand(B, T, F).clone()
        for k in range(K):
            blk = P3[:, k:k + T, off[s] + k * F: off[s] + (k + 1) * F]
            pre, mag = pre + blk, mag + blk.abs()
        out.append((pre, mag))
    return out


def keep_mult(n, p1, p2, seed, stream_id1, stream_id2):
    """fp64 [n]: 0 where either dropout draw drops feature element e, else 1 / ((1 - p1')(1 - p2')) evaluated in fp32 like the library"""
    m = torch.ones(n, dtype=torch.bool)
    scale = np.float32(1.0)
    for p, sid in ((p1, stream_id1), (p2, stream_id2)):
        if p > 0:
            m &= R.keep_mask(seed, sid, n, p)
            scale = np.float32(scale * np.float32(R.drop_params(p)[1]))
    return m.to(F64) * float(scale)


def pool_fwd(P, biases, sizes, B, L, mult=None):
    """-> feat [B, NF] fp64, argmax [B, NF] int32 (lowest t among equals; -1 where the best pre-activation is <= 0), smax [B, NF] (the
    largest sum of |terms| over the windows of the feature), gap [B, NF] (fp64 distance from the best pre-activation to the second
    best window and to 0, whichever is nearer: how far the routing decision is from flipping)."""
    feats, args, smaxs, gaps = [], [], [], []
    for pre, mag in pre_activations(P, biases, sizes, B, L):
        a = torch.from_numpy(np.argmax(pre.numpy(), axis=1))                # first occurrence of the maximum
        best = pre.gather(1, a[:, None, :]).squeeze(1)
        if pre.shape[1] > 1:
            top2 = pre.topk(2, dim=1).values
            gap = top2[:, 0] - top2[:, 1]
        else:
            gap = torch.full_like(best, float("inf"))
        gaps.append(torch.minimum(gap, best.abs()))
        dead = best <= 0
        feats.append(torch.where(dead, torch.zeros_like(best), best))
        args.append(torch.where(dead, torch.full_like(a, -1), a))
        smaxs.append(mag.max(dim=1).values)
    feat, arg = torch.cat(feats, 1), torch.cat(args, 1).to(torch.int32)
    if mult is not None:
        feat = feat * mult.reshape(feat.shape)
    return feat, arg, torch.cat(smaxs, 1), torch.cat(gaps, 1)


def effective_grad(g, arg, mult=None):
    ge = R.d(g) if mult is None else R.d(g) * mult.reshape(g.shape)
    return torch.where(arg < 0, torch.zeros_like(ge), ge)


def pool_bwd_w(g, arg, x0, x1, sizes, L, mult=None):
    """-> dW [S] fp64 [F, 2, K, H], db [S] [F], and the sums of |terms| of both (same shapes)"""
    B, NF = g.shape
    F = NF // len(sizes)
    ge = effective_grad(g, arg, mult)
    xs = (R.d(x0), R.d(x1))
    H = xs[0].shape[1]
    base = (torch.arange(B) * L)[:, None]
    dW, db, mW, mb = [], [], [], []
    for s, K in enumerate(sizes):
        gs, a = ge[:, s * F:(s + 1) * F], arg[:, s * F:(s + 1) * F].long().clamp(min=0)      # dead features carry gs = 0
        w, m = torch.zeros((F, 2, K, H), dtype=F64), torch.zeros((F, 2, K, H), dtype=F64)
        for c in range(2):
            for k in range(K):
                terms = gs[:, :, None] * xs[c][(base + a + k).clamp(max=B * L - 1)]              # [B, F, H]
                w[:, c, k], m[:, c, k] = terms.sum(0), terms.abs().sum(0)
        dW.append(w); mW.append(m); db.append(gs.sum(0)); mb.append(gs.abs().sum(0))
    return dW, db, mW, mb


def pool_bwd_x(g, arg, weights, sizes, L, mult=None):
    """-> dx of channel 0 [B * L, H] fp64 and the sum of |terms| per element"""
    B, NF = g.shape
    F = NF // len(sizes)
    H = weights[0].shape[3]
    ge = effective_grad(g, arg, mult)
    dx, mag = torch.zeros((B * L, H), dtype=F64), torch.zeros((B * L, H), dtype=F64)
    base = (torch.arange(B) * L)[:, None]
    for s, K in enumerate(sizes):
        gs, a = ge[:, s * F:(s + 1) * F], arg[:, s * F:(s + 1) * F].long()
        live = (a >= 0).reshape(-1)
        for k in range(K):
            rows = (base + a + k).reshape(-1)[live]
            terms = (gs[:, :, None] * R.d(weights[s])[None, :, 0, k, :]).reshape(B * F, H)[live]
            dx.index_add_(0, rows, terms)
            mag.index_add_(0, rows, terms.abs())
    return dx, mag


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
# (B, L, H, F, filter sizes): a single window; L barely above the largest filter; more than one slice of t; config C1's widths with
# 36 filters (NT = 396, padded to 400); H above 1024 (a second pass over h) with NT = 15
KERNEL_SHAPES = [(1, 5, 8, 1, "5"), (3, 6, 128, 4, "1,2,3,5"), (2, 20, 128, 6, "1,2,3,5"), (3, 255, 1024, 36, "1,2,3,5"), (2, 70, 1032, 5, "3")]


def shape_id(shape):
    return "B{}-L{}-H{}-F{}-K{}".format(*shape[:4], shape[4].replace(",", "_"))


def fwd_bound(sizes, F, smax):
    """|feat error| <= c 2^-24 smax with c = K_s + 1 per feature: the pool kernel adds K_s - 1 taps and the bias one after the other
    (K_s roundings) and multiplies by the dropout scale (1)."""
    c = torch.tensor([K + 1 for K in sizes for _ in range(F)], dtype=F64)
    return c * R.U24 * smax


def seeded_case(shape, seed=20):
    """bf16 x_0 / x_1, fp32 conv weights and biases, the upstream gradient g, and P: the fp64 tap projection of the bf16 operands rounded
    to fp32 once, [B * L, NTP] -- the SAME fp32 P goes to the kernel and (converted exactly) to the fp64 reference."""
    from types import SimpleNamespace
    B, L, H, F, sizes = shape
    sizes = parse_sizes(sizes)
    g = torch.Generator().manual_seed(seed + 1000 * len(sizes) + H)
    x0, x1 = (torch.randn((B * L, H), generator=g).to(torch.bfloat16) for _ in range(2))
    Ws = [torch.randn((F, 2, K, H), generator=g) / (2 * K * H) ** 0.5 for K in sizes]
    bs = [torch.randn(F, generator=g) * 0.1 + 0.2 for _ in sizes]
    gr = torch.randn((B, F * len(sizes)), generator=g)
    taps = pack_taps(Ws, sizes).to(torch.bfloat16)
    P = project(x0, x1, taps).to(torch.float32)
    return SimpleNamespace(B=B, L=L, H=H, F=F, sizes=sizes, NF=F * len(sizes), x0=x0, x1=x1, Ws=Ws, bs=bs, g=gr, taps=taps, P=P)
