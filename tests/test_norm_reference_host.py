"""tests/norm_reference.py against torch's own operators and autograd, all in fp64, on small inputs (no GPU): two fp64 implementations
of one formula agree to 1e-12 relative.  This is what makes the references of tests/test_norm_kernels_gpu.py trustworthy where there is
no GPU.  Also: on the input sets of the BatchNorm / GroupNorm GPU tests, an fp32 emulation of the forward disagrees with fp64 about the
sign of a pre-activation in far fewer than 0.1 % of the elements (the cap the GPU test puts on the kernel's own mask)."""
import pytest
import torch
import torch.nn.functional as F

import glue_reference as G
import norm_reference as N

F64 = torch.float64
TOL = 1e-12


def close(a, b):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= TOL * max(b.abs().max().item(), 1.0), err


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def bf(t):
    """fp64 values that are bf16 numbers (the LN tail rounds z: with such inputs and no arithmetic the rounding is the identity)"""
    return G.bf16_round(t)


@pytest.mark.parametrize("use_bias,use_res,use_beta,p", [(True, True, True, 0.0), (False, False, False, 0.0), (True, True, True, 0.3),
                                                         (False, True, True, 0.5), (True, False, False, 0.3)])
def test_ln_tail_against_layer_norm_and_an_explicit_mask(use_bias, use_res, use_beta, p):
    """z, y, mean, rstd and the whole backward against F.layer_norm under autograd; dropout as an explicit mask multiply.  The rounding
    of z to bf16 is checked separately (z_rounded = bf16(z)); autograd runs on the rounded z with a straight-through rounding, which is
    what the kernel's backward does (it reads the stored bf16 z and treats dz as the gradient of the unrounded sum)."""
    M, H, eps = 9, 24, 1e-6
    x = rnd(M, H, seed=1).requires_grad_()
    bias = rnd(H, seed=2).requires_grad_() if use_bias else None
    res = rnd(M, H, seed=3).requires_grad_() if use_res else None
    gamma, beta = (rnd(H, seed=4) + 2).requires_grad_(), (rnd(H, seed=5).requires_grad_() if use_beta else None)
    keep = G.keep_mask(7, 3, M * H, p).reshape(M, H) if p > 0 else None
    inv_keep = G.drop_params(p)[1]
    v = x if bias is None else x + bias
    if keep is not None:
        v = v * keep.to(F64) * inv_keep
    z = v if res is None else v + res
    zr = z + (G.bf16_round(z.detach()) - z.detach())          # straight-through rounding
    y = F.layer_norm(zr, (H,), gamma, beta, eps)
    dy = rnd(M, H, seed=6)
    y.backward(dy)

    z_, zr_, y_, mean_, rstd_ = N.ln_tail_fwd(x, bias, res, gamma, beta, eps, keep, inv_keep)
    close(z_, z.detach()), close(zr_, zr.detach()), close(y_, y.detach())
    assert torch.equal(zr_, G.bf16_round(z_))
    close(mean_, zr.detach().mean(1)), close(rstd_, 1 / torch.sqrt(zr.detach().var(1, unbiased=False) + eps))
    dz, dx, dgamma, dbeta, dbias = N.ln_tail_bwd(dy, None, zr_, mean_, rstd_, gamma, keep, inv_keep)
    if res is not None:
        close(dz, res.grad)
    close(dx if keep is not None else dz, x.grad)
    close(dgamma, gamma.grad)
    if use_beta:
        close(dbeta, beta.grad)
    if use_bias:
        close(dbias, bias.grad)
    if keep is not None:
        assert (dx[~keep] == 0).all() and 0 < int(keep.sum()) < M * H
    # dres is a plain addend of dz and, through the mask, of dx and dbias
    dres = rnd(M, H, seed=8)
    dz2, dx2, _, _, dbias2 = N.ln_tail_bwd(dy, dres, zr_, mean_, rstd_, gamma, keep, inv_keep)
    close(dz2, dz + dres)
    m = keep.to(F64) * inv_keep if keep is not None else torch.ones(M, H, dtype=F64)
    close(dbias2, dbias + (dres * m).sum(0))
    if keep is not None:
        close(dx2, dx + dres * m)


@pytest.mark.parametrize("segments,relu,training", [(1, 1, 1), (3, 1, 1), (2, 0, 1), (2, 1, 0), (1, 0, 0)])
def test_bn_act_against_batch_norm_per_segment(segments, relu, training):
    n, C, eps, mom = 7, 16, 1e-5, 0.1
    rows = n * segments
    x = (rnd(rows, C, seed=1) + 0.4).requires_grad_()
    gamma, beta = (rnd(C, seed=2) + 1.5).requires_grad_(), rnd(C, seed=3).requires_grad_()
    rm0, rv0 = rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    outs = []
    for s in range(segments):        # `segments` consecutive forward calls of nn.BatchNorm2d: the running statistics carry over
        o = F.batch_norm(x[s * n:(s + 1) * n], rm, rv, gamma, beta, bool(training), mom, eps)
        outs.append(F.relu(o) if relu else o)
    y = torch.cat(outs)
    dy, extra = rnd(rows, C, seed=6), rnd(rows, C, seed=7)
    y.backward(dy)

    y_, pre, mean, rstd, rm_, rv_ = N.bn_act_fwd(x, gamma, beta, rm0, rv0, segments, eps, mom, training, relu)
    close(y_, y.detach())
    close(rm_, rm), close(rv_, rv)
    if not training:
        close(rm_, rm0), close(rv_, rv0)
        close(mean, rm0[None].expand(segments, C)), close(rstd, (1 / torch.sqrt(rv0 + eps))[None].expand(segments, C))
    else:
        xs = x.detach().reshape(segments, n, C)
        close(mean, xs.mean(1)), close(rstd, 1 / torch.sqrt(xs.var(1, unbiased=False) + eps))
        assert N.bn_act_fwd(x, gamma, beta, None, None, segments, eps, mom, 1, relu)[4] is None
    mask = (pre > 0) if relu else None
    dx, dgamma, dbeta = N.bn_act_bwd(dy, x, gamma, mean, rstd, mask, segments, training)
    close(dx, x.grad), close(dgamma, gamma.grad), close(dbeta, beta.grad)
    close(N.bn_act_bwd(dy, x, gamma, mean, rstd, mask, segments, training, extra)[0], x.grad + extra)


def test_bn_act_single_row_segments():
    """one row per segment: the variance is zero, y = act(beta), and the running variance takes the biased (= zero) variance"""
    C = 8
    x, gamma, beta = rnd(2, C, seed=1), rnd(C, seed=2), rnd(C, seed=3)
    y, pre, mean, rstd, rm, rv = N.bn_act_fwd(x, gamma, beta, torch.zeros(C), torch.ones(C), 2, 1e-5, 0.1, 1, 1)
    close(y, beta.clamp(min=0)[None].expand(2, C)), close(mean, x), close(rv, torch.full((C,), 0.81, dtype=F64))


@pytest.mark.parametrize("images,hw,C,groups,relu", [(3, 5, 16, 4, 1), (2, 7, 24, 24, 0), (1, 1, 8, 2, 1), (2, 6, 8, 1, 1)])
def test_gn_act_against_group_norm(images, hw, C, groups, relu):
    eps = 1e-5
    rows = images * hw
    x = (rnd(rows, C, seed=1) + 0.4).requires_grad_()
    gamma, beta = (rnd(C, seed=2) + 1.5).requires_grad_(), rnd(C, seed=3).requires_grad_()
    o = F.group_norm(x.reshape(images, hw, C).permute(0, 2, 1), groups, gamma, beta, eps).permute(0, 2, 1).reshape(rows, C)
    y = F.relu(o) if relu else o
    dy, extra = rnd(rows, C, seed=6), rnd(rows, C, seed=7)
    y.backward(dy)
    y_, pre, mean, rstd = N.gn_act_fwd(x, gamma, beta, images, groups, eps, relu)
    close(y_, y.detach())
    cg = C // groups
    xg = x.detach().reshape(images, hw, groups, cg)
    close(mean.reshape(images, groups, cg)[:, :, 0], xg.mean((1, 3)))
    close(rstd.reshape(images, groups, cg)[:, :, 0], 1 / torch.sqrt(xg.var((1, 3), unbiased=False) + eps))
    assert (mean.reshape(images, groups, cg) == mean.reshape(images, groups, cg)[:, :, :1]).all()
    mask = (pre > 0) if relu else None
    dx, dgamma, dbeta = N.gn_act_bwd(dy, x, gamma, mean, rstd, mask, images, groups)
    close(dx, x.grad), close(dgamma, gamma.grad), close(dbeta, beta.grad)
    close(N.gn_act_bwd(dy, x, gamma, mean, rstd, mask, images, groups, extra)[0], x.grad + extra)


def _torch_pool(x, pad_zero):
    """F.max_pool2d on NCHW with return_indices -> (y NHWC, window position ky * 3 + kx of the recorded maximum, NHWC)"""
    B, H, W, C = x.shape
    xc = x.permute(0, 3, 1, 2)
    if pad_zero:
        y, idx = F.max_pool2d(F.pad(xc, (1, 1, 1, 1)), 3, 2, 0, return_indices=True)      # ConstantPad2d(1, 0.) + MaxPool2d(3, 2)
        Wp = W + 2
        iy, ix = idx // Wp, idx % Wp                                                       # padded coordinates = unpadded + 1
    else:
        y, idx = F.max_pool2d(xc, 3, 2, 1, return_indices=True)
        iy, ix = idx // W + 1, idx % W + 1
    Ho, Wo = y.shape[2:]
    oy, ox = torch.arange(Ho)[None, None, :, None], torch.arange(Wo)[None, None, None, :]
    arg = (iy - 2 * oy) * 3 + (ix - 2 * ox)
    return y.permute(0, 2, 3, 1), arg.permute(0, 2, 3, 1)


@pytest.mark.parametrize("pad_zero", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 1, 5, 3), (1, 2, 2, 3), (2, 7, 9, 4), (1, 8, 8, 5)])
@pytest.mark.parametrize("coarse", [False, True])
def test_maxpool_against_max_pool2d(shape, pad_zero, coarse):
    """values, the recorded window position (ties: the first in scan order; pad_zero: the zero ring can win) and the backward, which
    under pad_zero is autograd through the explicit pad (a ring winner's gradient is cut off by the pad's own backward)."""
    B, H, W, C = shape
    x = rnd(*shape, seed=H * 10 + W)
    if coarse:
        x = (x * 1.5).round() - (1.0 if pad_zero else 0.0)       # ties everywhere; shifted down so that the ring's zeros win somewhere
    y, arg = N.maxpool3s2(x, pad_zero)
    ty, targ = _torch_pool(x, pad_zero)
    assert y.shape == (B, N.pool_out(H), N.pool_out(W), C)
    assert torch.equal(y, ty) and torch.equal(arg.long(), targ)
    xr = x.clone().requires_grad_()
    ty2, _ = _torch_pool(xr, pad_zero)
    dy = rnd(*ty2.shape, seed=3)
    ty2.backward(dy)
    close(N.maxpool3s2_bwd(dy, arg, H, W), xr.grad)
    if coarse and pad_zero and H > 1:
        ky, kx = arg // 3, arg % 3
        oy, ox = torch.arange(y.shape[1])[None, :, None, None], torch.arange(y.shape[2])[None, None, :, None]
        iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
        assert ((iy < 0) | (iy >= H) | (ix < 0) | (ix >= W)).any(), "no ring winner in the coarse set"


def test_maxpool_nan_wins_every_window_it_is_in():
    x = rnd(1, 7, 9, 2, seed=1)
    x[0, 3, 4, 1] = float("nan")
    for pad_zero in (False, True):
        y, arg = N.maxpool3s2(x, pad_zero)
        ty, targ = _torch_pool(x, pad_zero)
        assert torch.equal(torch.isnan(y), torch.isnan(ty)) and int(torch.isnan(y).sum()) == 2      # rows 1..2 x column 2 of the output
        assert torch.equal(arg.long(), targ)
        assert torch.equal(y[~torch.isnan(y)], ty[~torch.isnan(ty)])


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 7, 10, 3), (1, 1, 1, 2)])
def test_rows_subsample_is_a_strided_1x1_convolution(shape, stride):
    B, H, W, C = shape
    x = rnd(*shape, seed=1).requires_grad_()
    w = torch.eye(C, dtype=F64).reshape(C, C, 1, 1)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride).permute(0, 2, 3, 1)
    close(N.rows_subsample(x, stride), y.detach())
    dy, base = rnd(*y.shape, seed=2), rnd(*shape, seed=3)
    y.backward(dy)
    close(N.rows_subsample_bwd(dy, None, H, W, stride), x.grad)
    close(N.rows_subsample_bwd(dy, base, H, W, stride), x.grad + base)


@pytest.mark.parametrize("k,C,stride,pad,Kp", [(3, 4, 1, 1, 40), (1, 8, 2, 0, 8), (7, 3, 1, 3, 152), (7, 3, 2, 3, 160), (2, 3, 3, 2, 16)])
def test_patches_against_unfold(k, C, stride, pad, Kp):
    B, H, W = 2, 11, 9
    img = rnd(B, C, H, W, seed=k)
    cols = N.patches_nchw(img, k, stride, pad, Kp)
    u = F.unfold(img, k, padding=pad, stride=stride)                       # [B, C * k * k, L], rows in (c, ky, kx) order
    L = u.shape[2]
    u = u.reshape(B, C, k * k, L).permute(0, 3, 2, 1).reshape(B * L, k * k * C)
    close(cols[:, :k * k * C], u)
    assert (cols[:, k * k * C:] == 0).all() and cols.shape == (B * L, Kp)


@pytest.mark.parametrize("kind", ["wide", "offset"])
@pytest.mark.parametrize("rows,C,segments,groups", [(63, 8, 1, 0), (130, 192, 1, 0), (231, 16, 3, 0), (200, 2056, 1, 0), (33000, 8, 1, 0),
                                                    (147, 192, 3, 32), (666, 64, 2, 8), (9, 6144, 1, 32), (5, 8, 5, 2), (5760, 8, 10, 1)])
def test_fp32_forward_flips_the_relu_mask_in_under_a_tenth_of_a_percent(rows, C, segments, groups, kind):
    """On the GPU tests' own input sets, the sign of the pre-activation computed in fp32 with the one-pass variance differs from the
    fp64 sign in fewer than 0.1 % of the elements -- and only where the fp64 pre-activation is tiny."""
    eps = 1e-5
    x, gamma, beta = N.norm_inputs(rows, C, 11 + rows + C, kind)
    p32 = N.preact_fp32(x, gamma, beta, segments, groups, eps)
    if groups:
        p64 = N.gn_act_fwd(x, gamma, beta, segments, groups, eps, 1)[1]
    else:
        p64 = N.bn_act_fwd(x, gamma, beta, None, None, segments, eps, 0.1, 1, 1)[1]
    flips = (p32 > 0) != (p64 > 0)
    assert flips.float().mean().item() < 1e-3
    assert (p64[flips].abs() < 1e-3).all()
