"""ECA-NFNet image tower on the HIP engine (reference src/models/image.py:40-199 NormFreeNet, built there from timm 0.6.5's
NormFreeBlock / create_stem / ScaledStdConv2d / EcaModule / DownsampleAvg; timm itself is absent offline, so the block
definitions follow timm's published source and only the in-tree bookkeeping, image.py:98-137, could be read directly).

Activations are NHWC bf16 ([B*H*W, C] rows): a 1x1 convolution is the bf16 MFMA GEMM, a (grouped) 3x3 convolution is a patch
gather + one GEMM per group (csrc/conv.hip).  Module / parameter names are timm's, so `image_encoder.bin` state_dicts load:
`stem.conv{1..4}.{weight,bias,gain}`, `stages.{s}.{b}.{downsample.conv,conv1,conv2,conv2b,conv3}.{weight,bias,gain}`,
`stages.{s}.{b}.attn_last.conv.weight`, `final_conv.*`, `head.fc.*`.

`NormFreeNet.embed` is the forward-only path (image_embedding.py): the SiLU behind a direct 3x3 convolution in that kernel's epilogue,
SiLU + pool in one read, standardised weights held between calls, feature maps in buffers owned per (batch, image size).
"""
import math

import torch
from torch import nn

from .. import _lib
from .._lib import check, ptr, stream_ptr
from . import functional as Fn
from ..utils import logger
from .base import HipModule

BF16, F32 = torch.bfloat16, torch.float32
NONLIN_GAMMA_SILU = 1.7881293296813965          # timm nfnet.py _nonlin_gamma['silu']

NFNET_CONFIGS = {   # timm nfnet.py model_cfgs (_nfnet_cfg): depths, channels, feat_mult
    "eca_nfnet_l0": ((1, 2, 6, 3), (256, 512, 1536, 1536), 1.5),
    "eca_nfnet_l1": ((2, 4, 12, 6), (256, 512, 1536, 1536), 2.0),
    "eca_nfnet_l2": ((3, 6, 18, 9), (256, 512, 1536, 1536), 2.0),
}


def make_divisible(v, divisor=8, min_value=None, round_limit=0.9):
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


def _ws(dev, nbytes):
    return torch.empty(max(int(nbytes), 16), device=dev, dtype=torch.uint8)


def _standardised(conv, ci, kk, Cgp):
    """the standardised bf16 weight [Cout, kk * Cgp] (tap-major, ci of Cgp channels per group used) of a ScaledStdConv2d, with the
    per-filter statistics its backward needs"""
    dev, Cout = conv.weight.device, conv.out_channels
    what = torch.empty((Cout, kk * Cgp), device=dev, dtype=BF16)
    mean = torch.empty(Cout, device=dev, dtype=F32)
    rstd = torch.empty(Cout, device=dev, dtype=F32)
    check(_lib.load().ia_ws_conv_weight_fwd(conv.weight.data_ptr(), conv.gain.data_ptr(), what.data_ptr(), mean.data_ptr(), rstd.data_ptr(), Cout,
                                            ci, kk, Cgp, conv.scale, conv.eps, stream_ptr()), "ia_ws_conv_weight_fwd")
    return what, mean, rstd


def _standardised_bwd(conv, dwhat, mean, rstd, ci, kk, Cgp):
    """the standardised weight's gradient back through the standardisation into the arena (weight and gain)"""
    check(_lib.load().ia_ws_conv_weight_bwd(dwhat.data_ptr(), conv.weight.data_ptr(), conv.gain.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            conv.weight.grad.data_ptr(), conv.gain.grad.data_ptr(), conv.out_channels, ci, kk, Cgp, conv.scale,
                                            stream_ptr()), "ia_ws_conv_weight_bwd")
    Fn._notify([p for p in (conv.weight, conv.bias, conv.gain) if p is not None])


def _bias_grad_ptr(conv):
    return conv.bias.grad.data_ptr() if conv.bias is not None and conv.bias.requires_grad else None


# ----------------------------------------------------------------------------------------- autograd glue
class StdConvFn(torch.autograd.Function):
    """ScaledStdConv2d on NHWC rows: standardise the weight (ia_ws_conv_weight_fwd), convolve (ia_conv_nhwc_fwd); backward
    = data gradient, weight gradient of the standardised weight, then back through the standardisation into the arena."""

    @staticmethod
    def forward(ctx, x, weight, conv, B, H, W):
        lib = _lib.load()
        Fn._need_gpu(x, "feature map")
        x = x.contiguous()
        C, Cout, k, s, g = conv.in_pad, conv.out_channels, conv.kernel_size, conv.stride, conv.groups
        Cg, Cgp, kk = conv.weight.shape[1], C // g, k * k
        dev = x.device
        what, mean, rstd = _standardised(conv, Cg, kk, Cgp)
        Ho, Wo = (H, W) if k == 1 else ((H - 1) // s + 1, (W - 1) // s + 1)
        y = torch.empty((B * Ho * Wo, Cout), device=dev, dtype=BF16)
        wsb = lib.ia_conv_nhwc_workspace_bytes(B, H, W, C, Cout, k, s, g)
        ws = _ws(dev, wsb)
        check(lib.ia_conv_nhwc_fwd(x.data_ptr(), what.data_ptr(), ptr(conv.bias), y.data_ptr(), B, H, W, C, Cout, k, s, g, ws.data_ptr(), wsb,
                                   stream_ptr()), "ia_conv_nhwc_fwd")
        ctx.conv, ctx.saved, ctx.dims = conv, (x, what, mean, rstd), (B, H, W, C, Cout, k, s, g, Cg, Cgp, kk)
        ctx.need_dx = ctx.needs_input_grad[0]
        conv.__dict__["_last_what"] = what      # the standardised bf16 weight of this call (the block tail takes the ECA pooling from it)
        # keep the 3x3 patch matrix for the weight gradient (9x the input, a few GB per step on 288 GB of HBM) instead of
        # gathering it again in backward
        ctx.cols_ws = ws if (k == 3 and conv.weight.requires_grad and conv.keep_cols) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        conv = ctx.conv
        x, what, mean, rstd = ctx.saved
        B, H, W, C, Cout, k, s, g, Cg, Cgp, kk = ctx.dims
        dy = dy.contiguous()
        dev = dy.device
        wsb = lib.ia_conv_nhwc_workspace_bytes(B, H, W, C, Cout, k, s, g)
        ws = _ws(dev, wsb)                 # scratch of the data gradient (it overwrites the patch area)
        dx = None
        if ctx.need_dx:
            dx = torch.empty_like(x)
            check(lib.ia_conv_nhwc_bwd_data(dy.data_ptr(), what.data_ptr(), dx.data_ptr(), B, H, W, C, Cout, k, s, g, ws.data_ptr(), wsb,
                                            stream_ptr()), "ia_conv_nhwc_bwd_data")
        if conv.weight.requires_grad:
            dwhat = torch.empty((Cout, kk * Cgp), device=dev, dtype=F32)
            wws = ctx.cols_ws if ctx.cols_ws is not None else ws
            check(lib.ia_conv_nhwc_bwd_weight(x.data_ptr(), dy.data_ptr(), dwhat.data_ptr(), _bias_grad_ptr(conv), B, H, W, C, Cout, k, s, g,
                                              int(ctx.cols_ws is not None), wws.data_ptr(), wsb, stream_ptr()), "ia_conv_nhwc_bwd_weight")
            ctx.cols_ws = None
            _standardised_bwd(conv, dwhat, mean, rstd, Cg, kk, Cgp)
        ctx.saved = None
        return dx, None, None, None, None, None


class PaddedStdConvFn(torch.autograd.Function):
    """ScaledStdConv2d, 3x3 / stride 1 (power-of-two channels per group), on the zero-bordered domain [B*(H+2)*(W+2), C]: no
    patch matrix — every tap is read as the input shifted by whole rows inside the GEMM, all groups in one launch
    (ia_conv3x3_padded_*).  The input must carry a zero border (SiluPadFn writes it); the output's border rows are garbage
    and are only ever read by SiluPadFn, which ignores them.  The incoming gradient needs a zero border too:
    SiluPadFn.backward provides it."""

    @staticmethod
    def forward(ctx, xp, weight, conv, B, H, W):
        lib = _lib.load()
        Fn._need_gpu(xp, "feature map")
        Cin, Cout, g = conv.in_channels, conv.out_channels, conv.groups
        ci = Cin // g
        dev = xp.device
        what, mean, rstd = _standardised(conv, ci, 9, ci)
        yp = torch.empty((xp.shape[0], Cout), device=dev, dtype=BF16)
        check(lib.ia_conv3x3_padded_fwd(xp.data_ptr(), what.data_ptr(), ptr(conv.bias), yp.data_ptr(), B, H, W, Cin, Cout, g, stream_ptr()),
              "ia_conv3x3_padded_fwd")
        ctx.conv, ctx.saved, ctx.dims = conv, (xp, what, mean, rstd), (B, H, W, Cin, Cout, g, ci)
        ctx.need_dx = ctx.needs_input_grad[0]
        return yp

    @staticmethod
    def backward(ctx, dyp):
        lib = _lib.load()
        conv = ctx.conv
        xp, what, mean, rstd = ctx.saved
        B, H, W, Cin, Cout, g, ci = ctx.dims
        dyp = dyp.contiguous()
        dev = dyp.device
        dxp = None
        if ctx.need_dx:
            dxp = torch.empty_like(xp)
            if lib.ia_conv3x3_direct_supported(Cin, Cout, g):
                # the direct kernel on dy with the tap-flipped, transposed filter bank [Cin][9 * Cout / groups] (as many elements as `what`)
                what_t = torch.empty((Cin, 9 * (Cout // g)), device=dev, dtype=BF16)
                check(lib.ia_conv3x3_flip_weights(what.data_ptr(), what_t.data_ptr(), Cin, Cout, g, stream_ptr()), "ia_conv3x3_flip_weights")
                check(lib.ia_conv3x3_padded_bwd_data_t(dyp.data_ptr(), what_t.data_ptr(), dxp.data_ptr(), B, H, W, Cin, Cout, g, stream_ptr()),
                      "ia_conv3x3_padded_bwd_data_t")
            else:
                check(lib.ia_conv3x3_padded_bwd_data(dyp.data_ptr(), what.data_ptr(), dxp.data_ptr(), B, H, W, Cin, Cout, g, stream_ptr()),
                      "ia_conv3x3_padded_bwd_data")
        if conv.weight.requires_grad:
            dwhat = torch.empty((Cout, 9 * ci), device=dev, dtype=F32)
            wsb = lib.ia_conv3x3_padded_workspace_bytes(B, H, W, Cin, Cout, g)
            ws = _ws(dev, wsb)
            check(lib.ia_conv3x3_padded_bwd_weight(xp.data_ptr(), dyp.data_ptr(), dwhat.data_ptr(), _bias_grad_ptr(conv), B, H, W, Cin, Cout, g,
                                                   ws.data_ptr(), wsb, stream_ptr()), "ia_conv3x3_padded_bwd_weight")
            _standardised_bwd(conv, dwhat, mean, rstd, ci, 9, ci)
        ctx.saved = None
        return dxp, None, None, None, None, None


class PaddedS2ConvFn(torch.autograd.Function):
    """ScaledStdConv2d, 3x3 / stride 2 (64 channels per group, or the stem's 64 -> 128), from the zero-bordered domain at H x W to the
    bordered -- or, `y_compact`, the compact -- domain at ceil(H/2) x ceil(W/2) without a patch matrix (ia_conv3x3_s2_padded_*: forward over
    the four parity views of x, weight gradient over the same views, data gradient over the four parity classes of dx).  Borders as for
    PaddedStdConvFn: the input's must be zero, the output's is garbage, the incoming gradient's is not read."""

    @staticmethod
    def forward(ctx, xp, weight, conv, B, H, W, y_compact):
        lib = _lib.load()
        Fn._need_gpu(xp, "feature map")
        Cin, Cout, g = conv.in_channels, conv.out_channels, conv.groups
        ci = Cin // g
        dev = xp.device
        what, mean, rstd = _standardised(conv, ci, 9, ci)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        rows = B * Ho * Wo if y_compact else B * (Ho + 2) * (Wo + 2)
        yp = torch.empty((rows, Cout), device=dev, dtype=BF16)
        check(lib.ia_conv3x3_s2_padded_fwd(xp.data_ptr(), what.data_ptr(), ptr(conv.bias), yp.data_ptr(), B, H, W, Cin, Cout, g, int(y_compact),
                                           stream_ptr()), "ia_conv3x3_s2_padded_fwd")
        ctx.conv, ctx.saved, ctx.dims = conv, (xp, what, mean, rstd), (B, H, W, Cin, Cout, g, ci, int(y_compact))
        ctx.need_dx = ctx.needs_input_grad[0]
        return yp

    @staticmethod
    def backward(ctx, dyp):
        lib = _lib.load()
        conv = ctx.conv
        xp, what, mean, rstd = ctx.saved
        B, H, W, Cin, Cout, g, ci, yc = ctx.dims
        dyp = dyp.contiguous()
        dev = dyp.device
        wsb = lib.ia_conv3x3_s2_padded_workspace_bytes(B, H, W, Cin, Cout, g)
        ws = _ws(dev, wsb)
        dxp = None
        if ctx.need_dx:
            # one kernel over the four parity classes of dx, on the tap-flipped transposed bank (the incoming gradient's border is zero:
            # the SiLU backward behind this convolution writes it)
            dxp = torch.empty_like(xp)
            what_t = torch.empty((Cout, 9 * ci), device=dev, dtype=BF16)
            if Cout == Cin:
                check(lib.ia_conv3x3_flip_weights(what.data_ptr(), what_t.data_ptr(), Cin, Cout, g, stream_ptr()), "ia_conv3x3_flip_weights")
            else:       # the stem's 64 -> 128: one bank per 64-channel slice of dy (the flip sees them as groups of a 128 -> 128 layout)
                check(lib.ia_conv3x3_flip_weights(what.data_ptr(), what_t.data_ptr(), Cout, Cout, Cout // 64, stream_ptr()), "ia_conv3x3_flip_weights")
            check(lib.ia_conv3x3_s2_padded_bwd_data_t(dyp.data_ptr(), what_t.data_ptr(), dxp.data_ptr(), B, H, W, Cin, Cout, g, yc, stream_ptr()),
                  "ia_conv3x3_s2_padded_bwd_data_t")
        if conv.weight.requires_grad:
            dwhat = torch.empty((Cout, 9 * ci), device=dev, dtype=F32)
            check(lib.ia_conv3x3_s2_padded_bwd_weight(xp.data_ptr(), dyp.data_ptr(), dwhat.data_ptr(), _bias_grad_ptr(conv), B, H, W, Cin, Cout, g, yc,
                                                      ws.data_ptr(), wsb, stream_ptr()), "ia_conv3x3_s2_padded_bwd_weight")
            _standardised_bwd(conv, dwhat, mean, rstd, ci, 9, ci)
        ctx.saved = None
        return dxp, None, None, None, None, None, None


class SiluPadFn(torch.autograd.Function):
    """y = silu(x) * scale while moving between the compact [B*H*W, C] rows and the zero-bordered [B*(H+2)*(W+2), C] rows
    that PaddedStdConvFn works on (one flag per side; ia_silu_pad_*).  A padded output gets its border written as zero, a
    padded input's border is never read; the same holds for the gradients in backward."""

    @staticmethod
    def forward(ctx, x, scale, B, H, W, in_padded, out_padded):
        lib = _lib.load()
        x = x.contiguous()
        C = x.shape[1]
        rows = B * (H + 2) * (W + 2) if out_padded else B * H * W
        y = torch.empty((rows, C), device=x.device, dtype=BF16)
        check(lib.ia_silu_pad_fwd(x.data_ptr(), y.data_ptr(), B, H, W, C, scale, int(in_padded), int(out_padded), stream_ptr()), "ia_silu_pad_fwd")
        ctx.x, ctx.args = x, (B, H, W, C, scale, int(in_padded), int(out_padded))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x = ctx.x
        B, H, W, C, scale, in_p, out_p = ctx.args
        dx = torch.empty_like(x)
        check(lib.ia_silu_pad_bwd(dy.contiguous().data_ptr(), x.data_ptr(), dx.data_ptr(), B, H, W, C, scale, in_p, out_p, stream_ptr()),
              "ia_silu_pad_bwd")
        ctx.x = None
        return dx, None, None, None, None, None, None


class SiluFn(torch.autograd.Function):
    """y = silu(x) * scale.  passthrough = True: also hands x back as a second output (the identity shortcut of a NormFreeBlock);
    passthrough = 2: hands y out twice (a downsampling block's activation feeds conv1 and the projected shortcut).  Either way the
    two gradients are combined inside the SiLU backward kernel instead of by a separate torch add over the feature map."""

    @staticmethod
    def forward(ctx, x, scale, passthrough):
        lib = _lib.load()
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.ia_silu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), scale, stream_ptr()), "ia_silu_fwd")
        ctx.x, ctx.scale, ctx.mode = x, scale, passthrough
        ctx.set_materialize_grads(False)
        if passthrough == 2:
            return y, y.view_as(y)
        return (y, x.view_as(x)) if passthrough else y

    @staticmethod
    def backward(ctx, dy, dother=None):
        lib = _lib.load()
        x = ctx.x
        if ctx.mode == 2:
            if dy is None or dother is None:
                dy = dy if dother is None else dother
                if dy is None:
                    return None, None, None
                dother = None
            dx = torch.empty_like(x)
            if dother is None:
                check(lib.ia_silu_bwd(dy.contiguous().data_ptr(), x.data_ptr(), None, dx.data_ptr(), x.numel(), ctx.scale, stream_ptr()), "ia_silu_bwd")
            else:
                check(lib.ia_silu_bwd_sum(dy.contiguous().data_ptr(), dother.contiguous().data_ptr(), x.data_ptr(), None, dx.data_ptr(), x.numel(),
                                          ctx.scale, stream_ptr()), "ia_silu_bwd_sum")
            return dx, None, None
        dpass = dother
        if dy is None:
            return dpass, None, None
        dx = torch.empty_like(x)
        dp = None if dpass is None else dpass.contiguous()
        check(lib.ia_silu_bwd(dy.contiguous().data_ptr(), x.data_ptr(), ptr(dp), dx.data_ptr(), x.numel(), ctx.scale, stream_ptr()), "ia_silu_bwd")
        return dx, None, None


class AvgPool2Fn(torch.autograd.Function):
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) (timm DownsampleAvg)."""

    @staticmethod
    def forward(ctx, x, B, H, W):
        lib = _lib.load()
        x = x.contiguous()
        C = x.shape[1]
        y = torch.empty((B * ((H + 1) // 2) * ((W + 1) // 2), C), device=x.device, dtype=BF16)
        check(lib.ia_avgpool2_fwd(x.data_ptr(), y.data_ptr(), B, H, W, C, stream_ptr()), "ia_avgpool2_fwd")
        ctx.dims = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        B, H, W, C = ctx.dims
        dx = torch.empty((B * H * W, C), device=dy.device, dtype=BF16)
        check(lib.ia_avgpool2_bwd(dy.contiguous().data_ptr(), dx.data_ptr(), B, H, W, C, stream_ptr()), "ia_avgpool2_bwd")
        return dx, None, None, None


class EcaResidualFn(torch.autograd.Function):
    """out = x * sigmoid(conv1d(mean_HW x)) * (attn_gain * alpha) + shortcut  (timm EcaModule + NormFreeBlock.forward tail).

    pre = (a, what, bias): x = a what^T + bias is the output of a 1x1 convolution (conv3): the ECA pooling mean_HW(x) is then taken as
    (mean_HW a) what^T + bias -- exact, the mean commutes with the per-pixel linear map -- from the 4 x narrower tensor a
    (ia_eca_fwd_linear, round 6).
    act_mode 1 / 2: the same pass also writes act = silu(out) * act_scale, the activation the NEXT block opens with
    (act1(x) * beta; mode 2 hands it out twice: a downsampling block feeds it to conv1 and to the projected shortcut), so `out` is not
    read back by a SiLU pass of its own; the gradient that arrives through act is folded into out's by ia_eca_silu_bwd."""

    @staticmethod
    def forward(ctx, x, shortcut, conv_w, eca, B, HW, coef, pre, act_scale=1.0, act_mode=0):
        lib = _lib.load()
        x, shortcut = x.contiguous(), shortcut.contiguous()
        C, k = x.shape[1], conv_w.shape[-1]
        dev = x.device
        out = torch.empty_like(x)
        pooled = torch.empty((B, C), device=dev, dtype=F32)
        gate = torch.empty((B, C), device=dev, dtype=F32)
        a, what, bias = pre
        Cmid = a.shape[1]
        wsb = lib.ia_eca_fwd_linear_workspace_bytes(B, HW, Cmid)
        ws = _ws(dev, wsb)
        act = torch.empty_like(x) if act_mode else None
        check(lib.ia_eca_fwd_linear(x.data_ptr(), a.data_ptr(), what.data_ptr(), ptr(bias), Cmid, conv_w.data_ptr(), k, shortcut.data_ptr(),
                                    out.data_ptr(), ptr(act), act_scale, pooled.data_ptr(), gate.data_ptr(), B, HW, C, coef, ws.data_ptr(), wsb,
                                    stream_ptr()), "ia_eca_fwd_linear")
        ctx.eca, ctx.saved, ctx.dims = eca, (x, pooled, gate), (B, HW, C, k, coef)
        ctx.act_scale, ctx.out = act_scale, (out if act is not None else None)
        if act is None:
            return out
        ctx.set_materialize_grads(False)
        return (out, act, act.view_as(act)) if act_mode == 2 else (out, act)

    @staticmethod
    def backward(ctx, dout, dact=None, dact2=None):
        lib = _lib.load()
        x, pooled, gate = ctx.saved
        B, HW, C, k, coef = ctx.dims
        w = ctx.eca.conv.weight
        if ctx.out is not None:
            # out's whole gradient = what arrives at `out` itself (the next block's identity shortcut; nothing for a downsampling block)
            # + (dact [+ dact2]) * act_scale * silu'(out): formed by ia_eca_silu_bwd in the pass that also takes the gate gradient's spatial sums
            g1, g2 = (dact, dact2) if dact is not None else (dact2, None)
            out, ctx.out = ctx.out, None
            if g1 is not None:
                dtot = torch.empty_like(out)
                dadd = None if dout is None else dout.contiguous()
                g1 = g1.contiguous()
                g2 = None if g2 is None else g2.contiguous()
                dx = torch.empty_like(x)
                wsb = lib.ia_eca_bwd_workspace_bytes(B, HW, C)
                ws = _ws(dtot.device, wsb)
                check(lib.ia_eca_silu_bwd(g1.data_ptr(), ptr(g2), out.data_ptr(), ptr(dadd), ctx.act_scale, x.data_ptr(), w.data_ptr(), k,
                                          pooled.data_ptr(), gate.data_ptr(), dtot.data_ptr(), dx.data_ptr(),
                                          w.grad.data_ptr() if w.requires_grad else None, B, HW, C, coef, ws.data_ptr(), wsb, stream_ptr()),
                      "ia_eca_silu_bwd")
                Fn._notify([w])
                ctx.saved = None
                return dx, dtot, None, None, None, None, None, None, None, None
        if dout is None:
            ctx.saved = None
            return (None,) * 10
        dout = dout.contiguous()
        dx = torch.empty_like(x)
        wsb = lib.ia_eca_bwd_workspace_bytes(B, HW, C)
        ws = _ws(dout.device, wsb)
        check(lib.ia_eca_bwd(dout.data_ptr(), x.data_ptr(), w.data_ptr(), k, pooled.data_ptr(), gate.data_ptr(), dx.data_ptr(),
                             w.grad.data_ptr() if w.requires_grad else None, B, HW, C, coef, ws.data_ptr(), wsb, stream_ptr()), "ia_eca_bwd")
        Fn._notify([w])
        ctx.saved = None
        return dx, dout, None, None, None, None, None, None, None, None


class GapFn(torch.autograd.Function):
    """[B*HW, C] bf16 -> mean over HW -> [B, C] fp32 (SelectAdaptivePool2d('avg', flatten=True))."""

    @staticmethod
    def forward(ctx, x, B, HW):
        lib = _lib.load()
        x = x.contiguous()
        C = x.shape[1]
        pooled = torch.empty((B, C), device=x.device, dtype=F32)
        wsb = lib.ia_gap_workspace_bytes(B, HW, C)
        ws = _ws(x.device, wsb)
        check(lib.ia_gap_fwd(x.data_ptr(), pooled.data_ptr(), B, HW, C, ws.data_ptr(), wsb, stream_ptr()), "ia_gap_fwd")
        ctx.dims = (B, HW, C)
        return pooled

    @staticmethod
    def backward(ctx, dp):
        lib = _lib.load()
        B, HW, C = ctx.dims
        dx = torch.empty((B * HW, C), device=dp.device, dtype=BF16)
        check(lib.ia_gap_bwd(dp.contiguous().to(F32).data_ptr(), dx.data_ptr(), B, HW, C, stream_ptr()), "ia_gap_bwd")
        return dx, None, None


# ---------------------------------------------------------------------------------------------- modules
class FeatureMap:
    """NHWC feature map handed between the tower's modules: rows [B*H*W, C] bf16 + its geometry."""
    __slots__ = ("t", "B", "H", "W", "act")

    def __init__(self, t, B, H, W, act=None):
        self.t, self.B, self.H, self.W = t, B, H, W
        self.act = act          # (tensors) the next block's opening activation silu(t) * beta, when the producing block tail wrote it already

    @property
    def shape(self):
        return (self.B, self.H, self.W, self.t.shape[1])


class ScaledStdConv2d(nn.Module):
    """timm layers/std_conv.py ScaledStdConv2d (gamma folded into the weight scale, eps 1e-5, bias on)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, groups=1, gamma=NONLIN_GAMMA_SILU, eps=1e-5, gain_init=1.0):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.stride, self.groups, self.eps = in_channels, out_channels, kernel_size, stride, groups, eps
        self.in_pad = max(8, in_channels) if groups == 1 else in_channels      # the 3-channel image is zero-padded to 8
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.gain = nn.Parameter(torch.full((out_channels, 1, 1, 1), gain_init))
        self.scale = gamma * self.weight[0].numel() ** -0.5
        self.keep_cols = True              # stash the 3x3 patch matrix from forward for the weight gradient
        nn.init.kaiming_normal_(self.weight, mode="fan_in", nonlinearity="linear")       # reference image.py:156

    @property
    def shifted_views(self):
        """3x3 / stride 1 / power-of-two channels per group: runs without a patch matrix on the zero-bordered domain"""
        ci, co = self.in_channels // self.groups, self.out_channels // self.groups
        return (self.kernel_size == 3 and self.stride == 1 and ci >= 8 and co >= 8 and not (ci & (ci - 1)) and not (co & (co - 1)))

    @property
    def strided_direct(self):
        """3x3 / stride 2 with a shape the patch-matrix-free strided kernels take (64 channels per group; the stem's 64 -> 128)"""
        return (self.kernel_size == 3 and self.stride == 2
                and bool(_lib.load().ia_conv3x3_s2_supported(self.in_channels, self.out_channels, self.groups)))

    @property
    def embed_direct(self):
        """a 3x3 convolution whose direct kernel has the forward-only activation epilogue (ia_conv3x3[_s2]_padded_fwd_act)"""
        if self.kernel_size != 3:
            return False
        if self.stride == 2:
            return self.strided_direct
        return self.shifted_views and bool(_lib.load().ia_conv3x3_direct_supported(self.in_channels, self.out_channels, self.groups))

    def fits_padded(self, B, H, W):
        """row indices of the padded tensor are 32-bit ints (its byte size is not limited)"""
        return B * (H + 2) * (W + 2) < 0x7FFFFFFF

    def forward(self, f):
        y = StdConvFn.apply(f.t, self.weight, self, f.B, f.H, f.W)
        k, s = self.kernel_size, self.stride
        Ho, Wo = (f.H, f.W) if k == 1 else ((f.H - 1) // s + 1, (f.W - 1) // s + 1)
        return FeatureMap(y, f.B, Ho, Wo)


class EcaModule(nn.Module):
    """timm layers/eca.py EcaModule: kernel size from the channel count (gamma 2, beta 1)."""

    def __init__(self, channels, gamma=2, beta=1):
        super().__init__()
        t = int(abs(math.log(channels, 2) + beta) / gamma)
        k = max(t if t % 2 else t + 1, 3)
        self.conv = nn.Conv1d(1, 1, kernel_size=k, padding=(k - 1) // 2, bias=False)


class DownsampleAvg(nn.Module):
    """timm nfnet.py DownsampleAvg: 2x2 average pool (stride > 1 only) then a 1x1 ScaledStdConv2d."""

    def __init__(self, in_chs, out_chs, stride=1):
        super().__init__()
        self.stride = stride
        self.pool = nn.AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False) if stride > 1 else nn.Identity()
        self.conv = ScaledStdConv2d(in_chs, out_chs, 1)

    def forward(self, f):
        if self.stride > 1:
            f = FeatureMap(AvgPool2Fn.apply(f.t, f.B, f.H, f.W), f.B, (f.H + 1) // 2, (f.W + 1) // 2)
        return self.conv(f)


class NormFreeBlock(nn.Module):
    """timm nfnet.py NormFreeBlock (reg=False, extra_conv=True, skipinit off, eca as attn_last, no drop path)."""

    def __init__(self, in_chs, out_chs, stride=1, alpha=0.2, beta=1.0, bottle_ratio=0.25, group_size=64, ch_div=8, attn_gain=2.0):
        super().__init__()
        mid_chs = make_divisible(out_chs * bottle_ratio, ch_div)
        groups = mid_chs // group_size
        mid_chs = group_size * groups
        self.alpha, self.beta, self.attn_gain = alpha, beta, attn_gain
        self.downsample = DownsampleAvg(in_chs, out_chs, stride=stride) if (in_chs != out_chs or stride != 1) else None
        self.conv1 = ScaledStdConv2d(in_chs, mid_chs, 1)
        self.conv2 = ScaledStdConv2d(mid_chs, mid_chs, 3, stride=stride, groups=groups)
        self.conv2b = ScaledStdConv2d(mid_chs, mid_chs, 3, stride=1, groups=groups)
        self.conv3 = ScaledStdConv2d(mid_chs, out_chs, 1, gain_init=0.0)       # timm: gain_init = 1 if skipinit else 0
        self.attn_last = EcaModule(out_chs)

    def embed_direct(self, B, H, W):
        """NormFreeNet.embed runs this block, entered at H x W, on the activation-epilogue kernels"""
        return self.conv2.embed_direct and self.conv2b.embed_direct and self.conv2b.fits_padded(B, H, W)

    def forward(self, f, next_block=None):
        """next_block: the NormFreeBlock that consumes this block's output (None: something else does, e.g. final_conv) -- its opening
        activation silu(out) * beta' is then written by this block's tail pass (EcaResidualFn) and travels as FeatureMap.act"""
        act = lambda g: FeatureMap(SiluFn.apply(g.t, 1.0, False), g.B, g.H, g.W)
        if self.downsample is not None:
            ya, yb = f.act if f.act is not None else SiluFn.apply(f.t, self.beta, 2)
            out = FeatureMap(ya, f.B, f.H, f.W)
            shortcut = self.downsample(FeatureMap(yb, f.B, f.H, f.W)).t
        else:
            o, shortcut = (f.act[0], f.t) if f.act is not None else SiluFn.apply(f.t, self.beta, True)
            out = FeatureMap(o, f.B, f.H, f.W)
        out = self.conv1(out)
        B, H, W = out.B, out.H, out.W
        fits = self.conv2b.fits_padded(B, H, W)
        if self.conv2.shifted_views and self.conv2b.shifted_views and fits:
            # conv1 -> [silu -> padded] conv2 [silu, padded -> padded] conv2b [silu -> compact] -> conv3
            t = SiluPadFn.apply(out.t, 1.0, B, H, W, False, True)
            t = PaddedStdConvFn.apply(t, self.conv2.weight, self.conv2, B, H, W)
            t = SiluPadFn.apply(t, 1.0, B, H, W, True, True)
            t = PaddedStdConvFn.apply(t, self.conv2b.weight, self.conv2b, B, H, W)
            out = FeatureMap(SiluPadFn.apply(t, 1.0, B, H, W, True, False), B, H, W)
        elif self.conv2.strided_direct and self.conv2b.shifted_views and fits:
            # the same chain through a stage transition: conv2 reads the bordered map at H x W and writes the bordered map at half size
            t = SiluPadFn.apply(out.t, 1.0, B, H, W, False, True)
            t = PaddedS2ConvFn.apply(t, self.conv2.weight, self.conv2, B, H, W, False)
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            t = SiluPadFn.apply(t, 1.0, B, H, W, True, True)
            t = PaddedStdConvFn.apply(t, self.conv2b.weight, self.conv2b, B, H, W)
            out = FeatureMap(SiluPadFn.apply(t, 1.0, B, H, W, True, False), B, H, W)
        elif self.conv2b.shifted_views and fits:
            out = self.conv2(act(out))                       # the strided 3x3 keeps the patch-matrix path
            B, H, W = out.B, out.H, out.W
            t = SiluPadFn.apply(out.t, 1.0, B, H, W, False, True)
            t = PaddedStdConvFn.apply(t, self.conv2b.weight, self.conv2b, B, H, W)
            out = FeatureMap(SiluPadFn.apply(t, 1.0, B, H, W, True, False), B, H, W)
        else:
            out = self.conv2(act(out))
            out = act(self.conv2b(act(out)))
        a = out.t                                                 # conv3's input [B*H*W, mid]
        assert a.is_contiguous(), "conv3's input must be contiguous rows (every producer above allocates it): the ECA pooling reads it"
        out = self.conv3(out)
        pre = (a, self.conv3.__dict__.pop("_last_what"), self.conv3.bias)
        fuse = next_block is not None
        mode = 0 if not fuse else (2 if next_block.downsample is not None else 1)
        y = EcaResidualFn.apply(out.t, shortcut, self.attn_last.conv.weight, self.attn_last, out.B, out.H * out.W, self.attn_gain * self.alpha, pre,
                                next_block.beta if fuse else 1.0, mode)
        if mode:
            return FeatureMap(y[0], out.B, out.H, out.W, act=tuple(y[1:]))
        return FeatureMap(y, out.B, out.H, out.W)


class _GlobalPool(nn.Module):
    def forward(self, f):
        return GapFn.apply(f.t, f.B, f.H * f.W)


class _Head(nn.Module):
    """timm ClassifierHead: only `global_pool` is on the item-alignment path (reference image.py:255); `fc` is kept for
    state_dict parity with timm checkpoints."""

    def __init__(self, num_features, num_classes=1000):
        super().__init__()
        self.global_pool = _GlobalPool()
        self.fc = nn.Linear(num_features, num_classes)


class NormFreeNet(HipModule):
    """reference image.py:40-199.  forward_features(images [B,3,S,S] fp32) -> FeatureMap ([B, S/32, S/32, num_features] NHWC
    bf16); head.global_pool(map) -> [B, num_features] fp32."""

    def __init__(self, depths, channels, feat_mult, stem_chs=128, group_size=64, bottle_ratio=0.25, alpha=0.2, attn_gain=2.0, num_classes=1000):
        super().__init__()
        chs = (stem_chs // 8, stem_chs // 4, stem_chs // 2, stem_chs)
        stem, cin = [], 3
        for i, (c, s) in enumerate(zip(chs, (2, 1, 1, 2))):                       # timm create_stem('deep_quad')
            stem.append((f"conv{i + 1}", ScaledStdConv2d(cin, c, 3, stride=s)))
            if i != 3:
                stem.append((f"act{i + 2}", nn.SiLU()))
            cin = c
        from collections import OrderedDict
        self.stem = nn.Sequential(OrderedDict(stem))
        prev, expected_var, stages = stem_chs, 1.0, []
        for si, depth in enumerate(depths):                                        # reference image.py:98-137
            stride = 1 if si == 0 else 2
            blocks = []
            for bi in range(depth):
                out_chs = make_divisible(channels[si], 8)
                blocks.append(NormFreeBlock(prev, out_chs, stride=stride if bi == 0 else 1, alpha=alpha, beta=1.0 / expected_var ** 0.5,
                                            bottle_ratio=bottle_ratio, group_size=group_size, attn_gain=attn_gain))
                if bi == 0:
                    expected_var = 1.0
                expected_var += alpha ** 2
                prev = out_chs
            stages.append(nn.Sequential(*blocks))
        self.stages = nn.Sequential(*stages)
        self.num_features = make_divisible(int(channels[-1] * feat_mult), 8)
        self.final_conv = ScaledStdConv2d(prev, self.num_features, 1)
        self.final_act = nn.SiLU()
        self.head = _Head(self.num_features, num_classes)
        nn.init.normal_(self.head.fc.weight, 0.0, 0.01)
        nn.init.zeros_(self.head.fc.bias)

    def forward_features(self, images):
        (self._root if "_root" in self.__dict__ else self).ensure_arena()
        lib = _lib.load()
        Fn._need_gpu(images, "images")
        images = images.contiguous().to(F32)
        B, C, H, W = images.shape
        x = torch.empty((B * H * W, 8), device=images.device, dtype=BF16)
        check(lib.ia_nchw_to_nhwc_bf16(images.data_ptr(), x.data_ptr(), B, C, H, W, 8, stream_ptr()), "ia_nchw_to_nhwc_bf16")
        f = FeatureMap(x, B, H, W)
        # deep_quad stem: conv1 (s2) act conv2 act conv3 act conv4 (s2).  The stride-1 convs run on the zero-bordered domain,
        # the SiLU in front of each one also converts the layout (compact -> padded -> padded -> compact).
        mods = list(self.stem.children())
        padded, i = False, 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, ScaledStdConv2d):
                if padded and m.stride == 2:                  # conv4: bordered in, compact out (the blocks read compact maps)
                    y = PaddedS2ConvFn.apply(f.t, m.weight, m, f.B, f.H, f.W, True)
                    f, padded = FeatureMap(y, f.B, (f.H - 1) // 2 + 1, (f.W - 1) // 2 + 1), False
                elif padded:
                    f = FeatureMap(PaddedStdConvFn.apply(f.t, m.weight, m, f.B, f.H, f.W), f.B, f.H, f.W)
                else:
                    f = m(f)
            else:
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                to_padded = (isinstance(nxt, ScaledStdConv2d) and (nxt.shifted_views or nxt.strided_direct) and nxt.fits_padded(f.B, f.H, f.W))
                if padded or to_padded:
                    f = FeatureMap(SiluPadFn.apply(f.t, 1.0, f.B, f.H, f.W, padded, to_padded), f.B, f.H, f.W)
                else:
                    f = FeatureMap(SiluFn.apply(f.t, 1.0, False), f.B, f.H, f.W)
                padded = to_padded
            i += 1
        blocks = [blk for stage in self.stages for blk in stage]
        for i, blk in enumerate(blocks):
            f = blk(f, blocks[i + 1] if i + 1 < len(blocks) else None)
        f = self.final_conv(f)
        return FeatureMap(SiluFn.apply(f.t, 1.0, False), f.B, f.H, f.W)

    def forward(self, images):
        return self.head.global_pool(self.forward_features(images))

    # ------------------------------------------------------------------------------------------ forward-only path
    def train(self, mode=True):
        self._drop_embed_state()
        return super().train(mode)

    def load_state_dict(self, state_dict, strict=True, **kw):
        self._drop_embed_state()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _drop_embed_state(self):
        self.__dict__.pop("_embed_held", None)
        self.__dict__.pop("_embed_plan_held", None)

    def _embed_fallback(self, what):
        """a stem or block without the activation-epilogue kernels runs on the existing launches: said once per tower, never silently"""
        if not self.__dict__.get("_embed_fallback_logged"):
            self.__dict__["_embed_fallback_logged"] = True
            logger.warning(f"NormFreeNet.embed: {what} has no activation-epilogue kernel and runs through the existing forward launches")

    def _embed_plan(self, B, H, W, device):
        """ONE plan is kept: it serves every batch of its image size up to its capacity (a smaller batch -- the last partial one, or one
        with unreadable images left out -- uses a prefix of its per-image buffers); a larger batch or another image size drops it, frees
        its memory and builds a new one.  What embed retains is therefore bounded by the largest batch seen at the current size."""
        plan = self.__dict__.get("_embed_plan_held")
        if plan is None or plan.key != (H, W, device) or B > plan.capacity:
            self.__dict__.pop("_embed_plan_held", None)
            del plan
            torch.cuda.empty_cache()                   # the old buffers go back to the device before the new ones are asked for
            plan = self.__dict__["_embed_plan_held"] = _EmbedPlan(device, (H, W, device), B)
        plan.B = B
        return plan

    def _embed_weights(self, arena):
        """every ScaledStdConv2d's standardised bf16 weight, computed once and held until a weight may have changed: train(),
        load_state_dict, an optimiser step, or any write the arena's staleness guard saw (its shadow was refreshed)"""
        key = (id(arena), arena.shadow_refreshes, arena.step_count)
        held = self.__dict__.get("_embed_held")
        if held is None or held[0] != key:
            what = {}
            for m in self.modules():
                if isinstance(m, ScaledStdConv2d):
                    kk, g = m.kernel_size ** 2, m.groups
                    what[m] = _standardised(m, m.weight.shape[1], kk, m.in_pad // g)[0]
            held = self.__dict__["_embed_held"] = (key, what)
        return held[1]

    def _embed_direct(self, B, H, W):
        """does every 3x3 convolution of the stem have the activation epilogue at this size?  (conv1 reads the image through the patch
        matrix; conv2 / conv3 are stride-1 direct pairs, conv4 is a stride-2 shape)"""
        c1, c2, c3, c4 = (m for m in self.stem.children() if isinstance(m, ScaledStdConv2d))
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        first = self.stages[0][0]          # it reads conv4's epilogue as its opening activation: nothing else may want conv4's plain output
        return (c1.stride == 2 and c2.embed_direct and c3.embed_direct and c4.embed_direct and c4.stride == 2 and c2.fits_padded(B, H1, W1)
                and first.downsample is not None and first.embed_direct(B, (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1))

    @torch.no_grad()
    def embed(self, images):
        """images [B, 3, S, S] fp32 -> the pooled features [B, num_features] fp32: the tower's inference path.  The same arithmetic as
        head.global_pool(forward_features(images)) with fewer roundings and passes: the SiLU behind every direct 3x3 convolution is taken on
        the fp32 accumulator in that convolution's epilogue (ia_conv3x3[_s2]_padded_fwd_act), final_act and the pool are one read of
        final_conv's output (ia_silu_gap_fwd), the standardised weights are held between calls and the feature maps live in buffers owned
        by one _EmbedPlan per image size (see _embed_plan).  Nothing is kept for a backward pass."""
        root = self._root if "_root" in self.__dict__ else self
        arena = root.ensure_arena()
        lib = _lib.load()
        Fn._need_gpu(images, "images")
        images = images.contiguous().to(F32)
        B, C, H, W = images.shape
        if not self._embed_direct(B, H, W):
            self._embed_fallback("the stem or the first block")
            return self.forward(images)                        # the existing launches, all of them
        what = self._embed_weights(arena)
        plan = self._embed_plan(B, H, W, images.device)
        sp = stream_ptr()
        c1, c2, c3, c4 = (m for m in self.stem.children() if isinstance(m, ScaledStdConv2d))
        blocks = [blk for stage in self.stages for blk in stage]
        # ---- stem: image -> NHWC (8 channels) -> conv1 (patch matrix) -> silu, bordered -> conv2 + silu -> conv3 + silu -> conv4 + silu * beta
        x = plan.buf("image", (B * H * W, 8))
        check(lib.ia_nchw_to_nhwc_bf16(images.data_ptr(), x.data_ptr(), B, C, H, W, 8, sp), "ia_nchw_to_nhwc_bf16")
        t, H, W = plan.conv(c1, what[c1], x, "stem1", B, H, W), (H - 1) // 2 + 1, (W - 1) // 2 + 1
        p = plan.silu_pad(t, "stem1p", B, H, W)
        p = plan.conv3_act(c2, what[c2], p, "stem2p", B, H, W, 1.0, False)
        p = plan.conv3_act(c3, what[c3], p, "stem3p", B, H, W, 1.0, False)
        act = plan.conv3_act(c4, what[c4], p, "stem4", B, H, W, blocks[0].beta, True)
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        f = FeatureMap(None, B, H, W, act=(act, act))
        # ---- blocks
        for i, blk in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            if blk.embed_direct(f.B, f.H, f.W) and f.act is not None:
                f = plan.block(blk, what, f, nxt, i)
            else:
                self._embed_fallback(f"block {i}")
                f = blk(f, nxt)                                # the existing launches: freshly allocated tensors, read by the next block
        # ---- tail: final_conv -> silu + global average pool in one read
        t = plan.conv(self.final_conv, what[self.final_conv], f.t, "final", f.B, f.H, f.W)
        pooled = torch.empty((B, self.num_features), device=images.device, dtype=F32)
        wsb = lib.ia_gap_workspace_bytes(B, f.H * f.W, self.num_features)
        check(lib.ia_silu_gap_fwd(t.data_ptr(), pooled.data_ptr(), B, f.H * f.W, self.num_features, 1.0, plan.ws(wsb).data_ptr(), wsb, sp),
              "ia_silu_gap_fwd")
        return pooled


class _EmbedPlan:
    """The feature-map buffers of NormFreeNet.embed at one image size, for up to `capacity` images: allocated at first use, reused by
    every later batch.  Every buffer is laid out per image ([B * rows, C]), so a batch of B <= capacity images uses the first B images'
    worth of each (`buf` returns that prefix; the kernels' range checks end with the B images they are told about).
    A bordered buffer is zero-filled when it is created and only its interior is written afterwards (ia_silu_pad_fwd rewrites the
    zeros, the activation epilogues leave the border alone), so it stays a valid zero-bordered input.  A block's buffers are keyed by
    role and shape -- blocks of one stage share them, the two tensors that outlive a block (`out`, `act`) alternate between two sets."""

    def __init__(self, device, key, capacity):
        self.device, self.key, self.capacity, self.B = device, key, capacity, capacity
        self.bufs, self._ws = {}, None

    def buf(self, role, shape, dtype=BF16, zero=False):
        """shape = (B * rows, ...) of the current batch: the first B images of a buffer allocated for `capacity` images"""
        rows = shape[0] // self.B
        assert rows * self.B == shape[0]
        key = (role, (rows,) + tuple(shape[1:]), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = self.bufs[key] = (torch.zeros if zero else torch.empty)((self.capacity * rows,) + tuple(shape[1:]), device=self.device, dtype=dtype)
        return t[:shape[0]]

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.bufs.values()) + (0 if self._ws is None else self._ws.numel())

    def ws(self, nbytes):
        """one scratch area for every call that wants one (they run in order on one stream)"""
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = _ws(self.device, nbytes)
        return self._ws

    def conv(self, conv, what, x, role, B, H, W):
        """a ScaledStdConv2d through ia_conv_nhwc_fwd (1x1: the GEMM; the stem's conv1: patch matrix) on compact rows"""
        lib = _lib.load()
        C, Cout, k, s, g = conv.in_pad, conv.out_channels, conv.kernel_size, conv.stride, conv.groups
        Ho, Wo = (H, W) if k == 1 else ((H - 1) // s + 1, (W - 1) // s + 1)
        y = self.buf(role, (B * Ho * Wo, Cout))
        wsb = lib.ia_conv_nhwc_workspace_bytes(B, H, W, C, Cout, k, s, g)
        check(lib.ia_conv_nhwc_fwd(x.data_ptr(), what.data_ptr(), ptr(conv.bias), y.data_ptr(), B, H, W, C, Cout, k, s, g, self.ws(wsb).data_ptr(), wsb,
                                   stream_ptr()), "ia_conv_nhwc_fwd")
        return y

    def silu_pad(self, x, role, B, H, W):
        """compact -> silu -> bordered (the 1x1 GEMM's epilogue stays as it is: the layout changes here)"""
        y = self.buf(role, (B * (H + 2) * (W + 2), x.shape[1]), zero=True)
        check(_lib.load().ia_silu_pad_fwd(x.data_ptr(), y.data_ptr(), B, H, W, x.shape[1], 1.0, 0, 1, stream_ptr()), "ia_silu_pad_fwd")
        return y

    def conv3_act(self, conv, what, xp, role, B, H, W, scale, compact):
        """bordered xp at H x W -> silu(conv3x3(xp) + bias) * scale, bordered (interior written) or compact, at H x W or, stride 2, half"""
        lib = _lib.load()
        Cin, Cout, g = conv.in_channels, conv.out_channels, conv.groups
        Ho, Wo = (H, W) if conv.stride == 1 else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
        y = self.buf(role, (B * Ho * Wo, Cout)) if compact else self.buf(role, (B * (Ho + 2) * (Wo + 2), Cout), zero=True)
        fn, nm = ((lib.ia_conv3x3_padded_fwd_act, "ia_conv3x3_padded_fwd_act") if conv.stride == 1
                  else (lib.ia_conv3x3_s2_padded_fwd_act, "ia_conv3x3_s2_padded_fwd_act"))
        check(fn(xp.data_ptr(), what.data_ptr(), ptr(conv.bias), y.data_ptr(), B, H, W, Cin, Cout, g, scale, int(compact), stream_ptr()), nm)
        return y

    def block(self, blk, what, f, nxt, i):
        """one NormFreeBlock: f.act = silu(x) * beta from the producer; conv1 -> silu_pad -> conv2 + silu -> conv2b + silu -> conv3 -> ECA +
        residual (+ the next block's opening activation)"""
        lib = _lib.load()
        B, H, W = f.B, f.H, f.W
        a_in = f.act[0]
        if blk.downsample is not None:
            sx, sH, sW = a_in, H, W
            if blk.downsample.stride > 1:
                sH, sW = (H + 1) // 2, (W + 1) // 2
                sx = self.buf("pool", (B * sH * sW, a_in.shape[1]))
                check(lib.ia_avgpool2_fwd(a_in.data_ptr(), sx.data_ptr(), B, H, W, a_in.shape[1], stream_ptr()), "ia_avgpool2_fwd")
            shortcut = self.conv(blk.downsample.conv, what[blk.downsample.conv], sx, "shortcut", B, sH, sW)
        else:
            shortcut = f.t
        t = self.conv(blk.conv1, what[blk.conv1], a_in, "mid1", B, H, W)
        p = self.silu_pad(t, "mid1p", B, H, W)
        p = self.conv3_act(blk.conv2, what[blk.conv2], p, "mid2p", B, H, W, 1.0, False)
        if blk.conv2.stride == 2:
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        a = self.conv3_act(blk.conv2b, what[blk.conv2b], p, "mid3", B, H, W, 1.0, True)
        x3 = self.conv(blk.conv3, what[blk.conv3], a, "mid4", B, H, W)
        C, k, Cmid = x3.shape[1], blk.attn_last.conv.weight.shape[-1], a.shape[1]
        out = self.buf("out%d" % (i & 1), (B * H * W, C))
        act = self.buf("act%d" % (i & 1), (B * H * W, C)) if nxt is not None else None
        pooled, gate = self.buf("pooled", (B, C), F32), self.buf("gate", (B, C), F32)
        wsb = lib.ia_eca_fwd_linear_workspace_bytes(B, H * W, Cmid)
        check(lib.ia_eca_fwd_linear(x3.data_ptr(), a.data_ptr(), what[blk.conv3].data_ptr(), ptr(blk.conv3.bias), Cmid, blk.attn_last.conv.weight.data_ptr(),
                                    k, shortcut.data_ptr(), out.data_ptr(), ptr(act), nxt.beta if nxt is not None else 1.0, pooled.data_ptr(),
                                    gate.data_ptr(), B, H * W, C, blk.attn_gain * blk.alpha, self.ws(wsb).data_ptr(), wsb, stream_ptr()),
              "ia_eca_fwd_linear")
        return FeatureMap(out, B, H, W, act=None if act is None else (act, act))


def create_nfnet(model_name, **kwargs):
    depths, channels, feat_mult = NFNET_CONFIGS[model_name]
    return NormFreeNet(depths, channels, feat_mult)
