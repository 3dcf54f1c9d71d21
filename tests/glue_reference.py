"""fp64 references of the small input, head and conv-tower kernels (csrc/embed.hip, head.hip, kgsim.hip, the element-wise part of
conv.hip, the weight re-layout of resnet.hip), in plain torch / numpy with no call into the HIP library.  One function per operation,
written from the formula in the kernel's header comment and the reference project's Python, forward and (explicit) backward;
tests/test_glue_reference_host.py checks every one of them against torch's own operators and autograd in fp64.

Also here: a host replica of the counter-based dropout hash of csrc/common.h (ia_mix32 / ia_rng) in numpy uint32, which returns the
keep mask the kernels draw for a given (seed, stream id, element index, p).
"""
import numpy as np
import torch

F64 = torch.float64
U24 = 2.0 ** -24          # half an fp32 ulp, relative
BF16_ULP = 2.0 ** -8      # one bf16 ulp, relative (8 significand bits)


def d(x):
    return None if x is None else x.detach().to("cpu").to(F64)


def bf16_round(x):
    """fp64 / fp32 values rounded to bf16 the way torch converts fp32 (round to nearest even), returned as fp64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


# ------------------------------------------------------------------------------------------------------------ dropout hash
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def rng32(seed, stream, idx):
    """ia_rng(seed, stream, idx) for an array of 32-bit counters."""
    key = _mix32(np.asarray([(int(stream) ^ ((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF], dtype=np.uint64))[0]
    return _mix32((np.asarray(idx, dtype=np.uint64) & _M32) ^ key).astype(np.uint32)


def drop_params(p):
    """(thr16, inv_keep): an element is kept iff its 16-bit draw >= thr16 = round(p * 65536); kept values are scaled by inv_keep,
    evaluated in fp32 like the host code of the library."""
    if p <= 0:
        return 0, 1.0
    thr16 = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(thr16) / np.float32(65536.0)))
    return thr16, inv_keep


def keep_mask(seed, stream, n, p, start=0):
    """bool [n]: element e = start + i is kept.  One 32-bit draw per pair of neighbouring elements (counter e >> 1), the low 16 bits
    belong to the even element."""
    thr16, _ = drop_params(p)
    e = np.arange(start, start + n, dtype=np.uint64)
    r = rng32(seed, stream, e >> np.uint64(1)).astype(np.uint64)
    u16 = np.where(e & np.uint64(1), r >> np.uint64(16), r & np.uint64(0xFFFF))
    return torch.from_numpy(u16 >= thr16)


# ------------------------------------------------------------------------------------------------------------ embeddings
def embed_sum(ids, tts, pids, extra_idx, word, type_, pos, extra):
    """z[m] = (extra[extra_idx[m]] if extra_idx[m] >= 0 else word[ids[m]]) + type[tts[m]] + pos[pids[m]]  (before the bf16 round)."""
    w = d(word)[ids]
    if extra_idx is not None:
        red = extra_idx >= 0
        w = torch.where(red[:, None], d(extra)[extra_idx.clamp(min=0).long()], w)
    return w + d(type_)[tts] + d(pos)[pids]


def layernorm_fwd(z, gamma, beta, eps):
    """y, mean, rstd of LayerNorm over the last dim (biased variance, two passes)."""
    z = d(z)
    mean = z.mean(-1)
    var = ((z - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (z - mean[:, None]) * rstd[:, None] * d(gamma) + d(beta), mean, rstd


def layernorm_bwd(dy, z, mean, rstd, gamma):
    """dz [M, H], dgamma [H], dbeta [H] of y = xhat * gamma + beta, xhat = (z - mean) * rstd."""
    dy, z, mean, rstd, gamma = d(dy), d(z), d(mean), d(rstd), d(gamma)
    xhat = (z - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dz = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dz, (dy * xhat).sum(0), dy.sum(0)


def embed_table_grads(dz, ids, tts, pids, extra_idx, n_word, n_type, n_pos, n_extra, word_pad, pos_pad):
    """Scatter of the per-row input gradient into the four tables: padding_idx rows get nothing, redirected rows go to `extra`."""
    H = dz.shape[1]
    red = extra_idx >= 0 if extra_idx is not None else torch.zeros_like(ids, dtype=torch.bool)
    w_ok = (~red) & (ids != word_pad)
    p_ok = pids != pos_pad
    out = {"word": torch.zeros(n_word, H, dtype=F64).index_add_(0, ids[w_ok], dz[w_ok]),
           "type": torch.zeros(n_type, H, dtype=F64).index_add_(0, tts, dz),
           "pos": torch.zeros(n_pos, H, dtype=F64).index_add_(0, pids[p_ok], dz[p_ok])}
    if n_extra:
        out["extra"] = torch.zeros(n_extra, H, dtype=F64).index_add_(0, extra_idx[red].long(), dz[red])
    return out


# ------------------------------------------------------------------------------------------------------------ ViT input side
def im2col_patch(images, P):
    """[B, C, S, S] -> [B * (S/P)^2, C*P*P], patch rows in (py, px) order, columns in (c, ph, pw) order."""
    B, C, S, _ = images.shape
    n = S // P
    x = d(images).reshape(B, C, n, P, n, P)              # b c py ph px pw
    return x.permute(0, 2, 4, 1, 3, 5).reshape(B * n * n, C * P * P)


def vit_tokens(patch, cls, pos):
    """tokens[b, 0] = cls + pos[0]; tokens[b, 1 + p] = patch[b, p] + pos[1 + p]."""
    B = patch.shape[0]
    return torch.cat((d(cls).reshape(1, 1, -1).expand(B, 1, -1), d(patch)), 1) + d(pos)[None]


def vit_tokens_bwd(dtok):
    """dpatch, dcls, dpos."""
    dtok = d(dtok)
    return dtok[:, 1:], dtok[:, 0].sum(0), dtok.sum(0)


def gather_rows(src, rows):
    return d(src)[rows.long()]


# ------------------------------------------------------------------------------------------------------------ heads
def span_mean(seq, spans):
    """out[s] = mean of seq[spans[s, 0] : spans[s, 1]]."""
    seq = d(seq)
    return torch.stack([seq[int(a):int(b)].mean(0) for a, b in spans.tolist()])


def span_mean_bwd(dout, spans, n_rows):
    """dseq[row] = sum over the spans that contain the row of dout[s] / len(s); rows in no span get zero."""
    dout = d(dout)
    dseq = torch.zeros(n_rows, dout.shape[1], dtype=F64)
    for s, (a, b) in enumerate(spans.tolist()):
        dseq[a:b] += dout[s] / (b - a)
    return dseq


def pair_head_ce(x, y, W, bias, labels):
    """logits = [x | y] W^T + b (y may be None), probs = softmax, loss = mean cross entropy (None without labels)."""
    f = d(x) if y is None else torch.cat((d(x), d(y)), 1)
    logits = f @ d(W).t() + (d(bias) if bias is not None else 0.0)
    m = logits.max(1, keepdim=True).values
    e = torch.exp(logits - m)
    probs = e / e.sum(1, keepdim=True)
    loss = None
    if labels is not None:
        lse = m[:, 0] + torch.log(e.sum(1))
        loss = (lse - logits[torch.arange(len(labels)), labels]).mean()
    return logits, probs, loss


def pair_head_ce_bwd(probs, labels, dloss, x, y, W):
    """dx, dy (None for the one-feature form), dW, db of dloss * mean CE."""
    probs = d(probs)
    B, C = probs.shape
    onehot = torch.zeros(B, C, dtype=F64)
    onehot[torch.arange(B), labels] = 1.0
    g = (probs - onehot) * (float(dloss) / B)
    f = d(x) if y is None else torch.cat((d(x), d(y)), 1)
    df = g @ d(W)
    D = x.shape[1]
    return df[:, :D], (None if y is None else df[:, D:]), g.t() @ f, g.sum(0)


# ------------------------------------------------------------------------------------------------------------ PKGM rows
def kg_gather(ent, rel, ids, ent_col, rel_lo, P):
    """h_sign [B, Dk] = sign(ent[e]) with sign(+-0) = 0, r [B*P, Dk] = rel[r_p]."""
    h = torch.sign(d(ent)[ids[:, ent_col]])
    r = d(rel)[ids[:, rel_lo:rel_lo + P].reshape(-1)]
    return h, r


def kg_gather_bwd(dr, ids, rel_lo, P, n_rel):
    dr = d(dr)
    return torch.zeros(n_rel, dr.shape[1], dtype=F64).index_add_(0, ids[:, rel_lo:rel_lo + P].reshape(-1), dr)


def kg_rows(h, r, hp):
    """[B, 2P, H]: rows p = h + r[p], rows P + p = hp - r[p]."""
    h, hp = d(h), d(hp)
    r = d(r).reshape(h.shape[0], -1, h.shape[1])
    return torch.cat((h[:, None] + r, hp[:, None] - r), 1)


def kg_rows_bwd(g):
    """dh, dr [B*P, H], dhp from g [B, 2P, H]."""
    g = d(g)
    P = g.shape[1] // 2
    return g[:, :P].sum(1), (g[:, :P] - g[:, P:]).reshape(-1, g.shape[2]), g[:, P:].sum(1)


# ------------------------------------------------------------------------------------------------------------ similarity head
SIM_INNER, SIM_COSINE, SIM_L1, SIM_L2 = 0, 1, 2, 3
COS_EPS, DIST_EPS = 1e-8, 1e-6


def pair_sim(x, y, measure):
    """sim [B], probs [B] (differentiable fp64 torch).  cosine = x.y / sqrt(max(|x|^2 |y|^2, eps^2)), so an all-zero row gives
    sim 0 and probs 0.5; the distances add eps to the difference like F.pairwise_distance."""
    if measure == SIM_INNER:
        s = (x * y).sum(1)
        return s, torch.sigmoid(s)
    if measure == SIM_COSINE:
        s = (x * y).sum(1) / torch.sqrt(((x * x).sum(1) * (y * y).sum(1)).clamp(min=COS_EPS ** 2))
        return s, (s + 1.0) * 0.5
    df = x - y + DIST_EPS
    s = df.abs().sum(1) if measure == SIM_L1 else torch.sqrt((df * df).sum(1))
    return s, torch.exp(-s)


def pair_sim_bwd(x, y, dsim, dprobs, measure, sim=None, probs=None):
    """dx, dy for upstream gradients of sim and probs (either may be None); rows must not be degenerate.  sim / probs: the saved
    forward outputs the backward pass is handed (default: recomputed here)."""
    x, y = d(x), d(y)
    s, p = pair_sim(x, y, measure)
    s, p = (s if sim is None else d(sim)), (p if probs is None else d(probs))
    g = torch.zeros_like(s) if dsim is None else d(dsim).clone()
    if dprobs is not None:
        g = g + d(dprobs) * {SIM_INNER: p * (1 - p), SIM_COSINE: torch.full_like(p, 0.5), SIM_L1: -p, SIM_L2: -p}[measure]
    if measure == SIM_INNER:
        gx, gy = y, x
    elif measure == SIM_COSINE:
        n1, n2 = (x * x).sum(1, keepdim=True), (y * y).sum(1, keepdim=True)
        inv = 1.0 / torch.sqrt(n1 * n2)
        gx, gy = y * inv - s[:, None] * x / n1, x * inv - s[:, None] * y / n2
    else:
        df = x - y + DIST_EPS
        gx = torch.sign(df) if measure == SIM_L1 else df / s[:, None]
        gy = -gx
    return g[:, None] * gx, g[:, None] * gy


# ------------------------------------------------------------------------------------------------------------ conv tower pieces
def ws_weight(w, gain, scale, eps, Cgp):
    """ScaledStdConv2d: what [Cout, kk, Cgp] = (w - mean_o) * rstd_o * gain_o * scale, statistics over the Cg*kk fan-in (biased,
    two-pass variance, eps inside the sqrt); w is [Cout, Cg, kk]; channels >= Cg are zero.  Returns what, mean, rstd."""
    w, gain = d(w), d(gain)
    Cout, Cg, kk = w.shape
    mean = w.reshape(Cout, -1).mean(1)
    var = ((w - mean[:, None, None]) ** 2).reshape(Cout, -1).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    std = (w - mean[:, None, None]) * (rstd * gain * scale)[:, None, None]
    what = torch.zeros(Cout, kk, Cgp, dtype=F64)
    what[:, :, :Cg] = std.permute(0, 2, 1)
    return what, mean, rstd


def ws_weight_bwd(dwhat, w, gain, mean, rstd, scale):
    """dw [Cout, Cg, kk], dgain [Cout] from dwhat [Cout, kk, Cgp] (padded channels carry no gradient)."""
    w, gain, mean, rstd = d(w), d(gain), d(mean), d(rstd)
    Cout, Cg, kk = w.shape
    g = d(dwhat)[:, :, :Cg].permute(0, 2, 1)
    xh = (w - mean[:, None, None]) * rstd[:, None, None]
    mg = g.reshape(Cout, -1).mean(1)[:, None, None]
    mgx = (g * xh).reshape(Cout, -1).mean(1)[:, None, None]
    return (gain * scale * rstd)[:, None, None] * (g - mg - xh * mgx), scale * (g * xh).reshape(Cout, -1).sum(1)


def _pool_count(H, W):
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ch = torch.tensor([2 if 2 * i + 1 < H else 1 for i in range(Ho)], dtype=F64)
    cw = torch.tensor([2 if 2 * i + 1 < W else 1 for i in range(Wo)], dtype=F64)
    return ch[:, None] * cw[None, :]


def avgpool2(x):
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) on NHWC."""
    x = d(x)
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=F64)
    xp[:, :H, :W] = x
    s = xp.reshape(B, Ho, 2, Wo, 2, C).sum((2, 4))
    return s / _pool_count(H, W)[None, :, :, None]


def avgpool2_bwd(dy, H, W):
    """dx[b, iy, ix] = dy[b, iy // 2, ix // 2] / (number of in-image pixels of that window)."""
    dy = d(dy) / _pool_count(H, W)[None, :, :, None]
    return dy.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]


def gap(x):
    """[B, HW, C] -> [B, C] mean."""
    return d(x).mean(1)


def gap_bwd(dpooled, HW):
    return (d(dpooled) / HW)[:, None, :].expand(-1, HW, -1)


def silu(x, scale):
    x = d(x)
    return x * torch.sigmoid(x) * scale


def silu_bwd(dy, x, scale, dy2=None, dadd=None):
    """dx = (dy [+ dy2]) * scale * silu'(x) [+ dadd], silu'(x) = s (1 + x (1 - s)), s = sigmoid(x)."""
    x = d(x)
    s = torch.sigmoid(x)
    g = d(dy) + (d(dy2) if dy2 is not None else 0.0)
    return g * scale * s * (1.0 + x * (1.0 - s)) + (d(dadd) if dadd is not None else 0.0)


def nchw_to_nhwc(x, Cp):
    """[B, C, H, W] -> [B, H, W, Cp], channels >= C zero."""
    x = d(x)
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, Cp, dtype=F64)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def pad_rows(x, in_padded, out_padded):
    """copy between compact [B, H, W, C] and zero-bordered [B, H+2, W+2, C]."""
    x = d(x)
    if in_padded:
        x = x[:, 1:-1, 1:-1]
    if out_padded:
        x = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    return x


def weight_pack(w, Cgp, ldw):
    """what [Cout, ldw]: what[o, t*Cgp + c] = w[o, c, t], everything else zero."""
    w = d(w)
    Cout, Cg, kk = w.shape
    what = torch.zeros(Cout, kk, Cgp, dtype=F64)
    what[:, :, :Cg] = w.permute(0, 2, 1)
    out = torch.zeros(Cout, ldw, dtype=F64)
    out[:, :kk * Cgp] = what.reshape(Cout, -1)
    return out


def weight_unpack_grad(dwhat, Cg, kk, Cgp):
    """dw [Cout, Cg, kk] read back out of dwhat [Cout, ldw]."""
    dwhat = d(dwhat)
    return dwhat[:, :kk * Cgp].reshape(-1, kk, Cgp)[:, :, :Cg].permute(0, 2, 1)
