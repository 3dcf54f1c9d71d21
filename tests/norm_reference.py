"""fp64 references of the normalisation, column-sum and pooling kernels (csrc/layernorm.hip; BatchNorm / GroupNorm + ReLU, MaxPool 3x3/2,
the strided row subsampling and the NCHW patch gather of csrc/resnet.hip), in plain torch with no call into the HIP library.  One function
per operation, written from the kernel's header comment, forward and (explicit) backward; tests/test_norm_reference_host.py checks every
one of them against torch's own operators and autograd in fp64.

Activations are NHWC: rows [rows, C] for the norms, [B, H, W, C] for the pooling and subsampling.  The backward references of the two
norms take the ReLU mask as an argument (None = no ReLU): the caller decides whose zeros they are.

Also here: the input sets of the BatchNorm / GroupNorm GPU tests (`norm_inputs`) and an fp32 emulation of the pre-activation
(`preact_fp32`), so that the host test can check, without a GPU, how rarely fp32 and fp64 disagree about the sign of a pre-activation
on exactly those inputs.
"""
import torch

from glue_reference import F64, bf16_round, d, layernorm_bwd, layernorm_fwd

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------ LayerNorm tail
def ln_tail_fwd(x, bias, res, gamma, beta, eps, keep=None, inv_keep=1.0):
    """z = res + keep * (x + bias) * inv_keep (bias, res, beta, keep may be None); mean, rstd and y are those of the bf16-ROUNDED z.
    Returns (z unrounded, z rounded, y, mean, rstd)."""
    v = d(x)
    if bias is not None:
        v = v + d(bias)
    if keep is not None:
        v = torch.where(keep, v * inv_keep, torch.zeros((), dtype=F64))
    if res is not None:
        v = v + d(res)
    zr = bf16_round(v)
    y, mean, rstd = layernorm_fwd(zr, gamma, beta if beta is not None else torch.zeros_like(d(gamma)), eps)
    return v, zr, y, mean, rstd


def ln_tail_bwd(dy, dres, z, mean, rstd, gamma, keep=None, inv_keep=1.0):
    """dz = LN'(dy) (+ dres), dx = keep * dz * inv_keep (None without dropout), dgamma, dbeta, and dbias = the column sums of dx under
    dropout, of dz otherwise (the gradient of the branch the bias was added to)."""
    dz, dgamma, dbeta = layernorm_bwd(dy, z, mean, rstd, gamma)
    if dres is not None:
        dz = dz + d(dres)
    if keep is None:
        return dz, None, dgamma, dbeta, dz.sum(0)
    dx = torch.where(keep, dz * inv_keep, torch.zeros((), dtype=F64))
    return dz, dx, dgamma, dbeta, dx.sum(0)


# ------------------------------------------------------------------------------------------------------------ BatchNorm + ReLU
def bn_act_fwd(x, gamma, beta, running_mean, running_var, segments, eps, momentum, training, relu):
    """x [rows, C] in `segments` equal consecutive runs.  training: each run is normalised with its own mean and BIASED variance, and
    the running statistics (None = not kept) take the momentum update with the UNBIASED variance, run after run; eval: the running
    statistics normalise every run.  Returns (y, pre-activation, mean [segments, C], rstd [segments, C], running_mean, running_var)."""
    x, gamma, beta = d(x), d(gamma), d(beta)
    rows, C = x.shape
    n = rows // segments
    xs = x.reshape(segments, n, C)
    rm, rv = d(running_mean), d(running_var)
    if training:
        mean = xs.mean(1)
        var = ((xs - mean[:, None]) ** 2).mean(1)
        for s in range(segments):
            if rm is not None:
                rm = (1 - momentum) * rm + momentum * mean[s]
            if rv is not None:
                rv = (1 - momentum) * rv + momentum * var[s] * (n / (n - 1) if n > 1 else 1.0)
    else:
        mean, var = rm[None].expand(segments, C), rv[None].expand(segments, C)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = ((xs - mean[:, None]) * rstd[:, None] * gamma + beta).reshape(rows, C)
    return (pre.clamp(min=0) if relu else pre), pre, mean, rstd, rm, rv


def bn_act_bwd(dy, x, gamma, mean, rstd, mask, segments, training, extra=None):
    """g = dy * mask (mask None: no ReLU); xhat = (x - mean) * rstd per segment.  training: dx = gamma rstd (g - mean(g) - xhat mean(g xhat))
    with the means over the segment's rows; eval: dx = gamma rstd g.  (+ extra.)  dgamma = sum g xhat, dbeta = sum g over all rows."""
    dy, x, gamma, mean, rstd = d(dy), d(x), d(gamma), d(mean), d(rstd)
    rows, C = x.shape
    n = rows // segments
    g = dy if mask is None else dy * mask.to(F64)
    gs, xh = g.reshape(segments, n, C), (x.reshape(segments, n, C) - mean[:, None]) * rstd[:, None]
    if training:
        dx = gamma * rstd[:, None] * (gs - gs.mean(1, keepdim=True) - xh * (gs * xh).mean(1, keepdim=True))
    else:
        dx = gamma * rstd[:, None] * gs
    dx = dx.reshape(rows, C)
    if extra is not None:
        dx = dx + d(extra)
    return dx, (gs * xh).sum((0, 1)), gs.sum((0, 1))


# ------------------------------------------------------------------------------------------------------------ GroupNorm + ReLU
def gn_act_fwd(x, gamma, beta, images, groups, eps, relu):
    """x [rows, C] of `images` images; biased statistics per (image, group of C / groups consecutive channels).  Returns (y,
    pre-activation, mean [images, C], rstd [images, C]) with the group's value repeated for each of its channels."""
    x, gamma, beta = d(x), d(gamma), d(beta)
    rows, C = x.shape
    hw, cg = rows // images, C // groups
    xg = x.reshape(images, hw, groups, cg)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = ((xg - mean) * rstd).reshape(images, hw, C) * gamma + beta
    pre = pre.reshape(rows, C)
    rep = lambda t: t.reshape(images, groups, 1).expand(images, groups, cg).reshape(images, C)
    return (pre.clamp(min=0) if relu else pre), pre, rep(mean), rep(rstd)


def gn_act_bwd(dy, x, gamma, mean, rstd, mask, images, groups, extra=None):
    """g = dy * mask; with M1 = the mean over the (image, group) of gamma g and M2 = that of gamma g xhat:
    dx = rstd (gamma g - M1 - xhat M2) (+ extra); dgamma = sum g xhat, dbeta = sum g over all rows."""
    dy, x, gamma, mean, rstd = d(dy), d(x), d(gamma), d(mean), d(rstd)
    rows, C = x.shape
    hw, cg = rows // images, C // groups
    g = (dy if mask is None else dy * mask.to(F64)).reshape(images, hw, C)
    xh = (x.reshape(images, hw, C) - mean[:, None]) * rstd[:, None]
    gg = g * gamma
    grp = lambda t: t.reshape(images, hw, groups, cg).mean((1, 3), keepdim=True).expand(images, hw, groups, cg).reshape(images, hw, C)
    dx = (rstd[:, None] * (gg - grp(gg) - xh * grp(gg * xh))).reshape(rows, C)
    if extra is not None:
        dx = dx + d(extra)
    return dx, (g * xh).sum((0, 1)), g.sum((0, 1))


# ------------------------------------------------------------------------------------------------------------ MaxPool 3x3 / 2 / pad 1
def pool_out(n, stride=2):
    return (n - 1) // stride + 1


def maxpool3s2(x, pad_zero=False):
    """x [B, H, W, C] -> (y [B, Ho, Wo, C], arg uint8): the maximum of the 3x3 window at (2 oy - 1, 2 ox - 1) and the window position
    ky * 3 + kx of the FIRST maximum in scan order; a NaN in the window wins (as in torch).  Positions outside the image do not take
    part -- or, pad_zero, count as 0.0."""
    x = d(x)
    B, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=F64)
    inside = torch.zeros(2 * Ho + 1, 2 * Wo + 1, dtype=torch.bool)
    xp[:, 1:H + 1, 1:W + 1], inside[1:H + 1, 1:W + 1] = x, True
    best = torch.zeros(B, Ho, Wo, C, dtype=F64)
    arg = torch.zeros(B, Ho, Wo, C, dtype=torch.uint8)
    started = torch.zeros(B, Ho, Wo, C, dtype=torch.bool)
    for t in range(9):
        ky, kx = divmod(t, 3)
        cand = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
        valid = inside[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][None, :, :, None].expand_as(cand)
        if pad_zero:
            valid = torch.ones_like(valid)
        take = valid & (~started | (cand > best) | torch.isnan(cand))
        best = torch.where(take, cand, best)
        arg = torch.where(take, torch.full_like(arg, t), arg)
        started = started | valid
    return best, arg


def maxpool3s2_bwd(dy, arg, H, W):
    """dx [B, H, W, C]: every dy goes to the pixel its window recorded; a recorded position outside the image (a pad_zero ring winner)
    has no pixel and routes nothing."""
    dy = d(dy)
    B, Ho, Wo, C = dy.shape
    dxp = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=F64)
    for t in range(9):
        ky, kx = divmod(t, 3)
        dxp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += dy * (arg == t).to(F64)
    return dxp[:, 1:H + 1, 1:W + 1].clone()


# ------------------------------------------------------------------------------------------------------------ strided 1x1 rows
def rows_subsample(x, stride):
    return d(x)[:, ::stride, ::stride]


def rows_subsample_bwd(dy, base, H, W, stride):
    """dx [B, H, W, C] = base (None = zeros) + dy on the stride grid."""
    dy = d(dy)
    B, _, _, C = dy.shape
    dx = torch.zeros(B, H, W, C, dtype=F64) if base is None else d(base).clone()
    dx[:, ::stride, ::stride] += dy
    return dx


# ------------------------------------------------------------------------------------------------------------ patch gather
def patches_nchw(img, k, stride, pad, Kp):
    """img [B, C, H, W] -> cols [B * Ho * Wo, Kp]: column (ky * k + kx) * C + c holds img[b, c, oy * stride + ky - pad,
    ox * stride + kx - pad], zero outside the image and in the columns [k * k * C, Kp)."""
    img = d(img)
    B, C, H, W = img.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = torch.zeros(B, C, H + 2 * pad, W + 2 * pad, dtype=F64)
    xp[:, :, pad:pad + H, pad:pad + W] = img
    cols = torch.zeros(B, Ho, Wo, Kp, dtype=F64)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]      # [B, C, Ho, Wo]
            cols[..., (ky * k + kx) * C:(ky * k + kx + 1) * C] = win.permute(0, 2, 3, 1)
    return cols.reshape(B * Ho * Wo, Kp)


# ------------------------------------------------------------------------------------------------------------ test inputs
def norm_inputs(rows, C, seed, kind):
    """The two input sets of the BatchNorm / GroupNorm tests, as (x bf16 [rows, C], gamma fp32 [C], beta fp32 [C]):
    "wide": mean about 0.4, std 1.5;  "offset": per-channel mean +-3, std 0.5 (mean^2 / variance = 36)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "wide":
        x = torch.randn(rows, C, generator=g) * 1.5 + 0.4
    else:
        sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        x = torch.randn(rows, C, generator=g) * 0.5 + 3.0 * sign
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1                                     # negative scales too: the mask is that of the pre-activation, not of xhat
    beta = torch.randn(C, generator=g) * 0.3
    return x.to(BF16), gamma, beta


def preact_fp32(x, gamma, beta, segments, groups, eps):
    """fp32 emulation of the kernels' pre-activation: one-pass variance q / n - mu^2 in fp32 per segment (groups = 0, BatchNorm) or
    per (segment, group) (GroupNorm); (x - mu) * rstd * gamma + beta in fp32."""
    F32 = torch.float32
    x = x.to(F32)
    rows, C = x.shape
    n = rows // segments
    xs = x.reshape(segments, n, C)
    if groups:
        xg = xs.reshape(segments, n, groups, C // groups)
        mu = xg.mean((1, 3), keepdim=True)
        var = ((xg * xg).mean((1, 3), keepdim=True) - mu * mu).clamp(min=0)
        pre = ((xg - mu) * torch.rsqrt(var + eps)).reshape(segments, n, C)
    else:
        mu = xs.mean(1, keepdim=True)
        var = ((xs * xs).mean(1, keepdim=True) - mu * mu).clamp(min=0)
        pre = (xs - mu) * torch.rsqrt(var + eps)
    return (pre * gamma.to(F32) + beta.to(F32)).reshape(rows, C)
