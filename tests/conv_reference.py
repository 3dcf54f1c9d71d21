"""fp64 reference, exact operands and derived per-element error bounds for the convolution entry points of csrc/conv.hip:
ia_conv3x3_padded_* (the direct kernels and the shifted-view / grouped GEMM), ia_conv3x3_s2_padded_*, ia_conv3x3_flip_weights and the
patch-matrix path ia_conv_nhwc_*.  Host only: torch fp64 on any device and numpy; nothing here calls the library, and nothing calls
torch.nn.functional.conv2d (tests/test_conv_reference_host.py compares the reference with it on the CPU).

Layouts are the library's own: activations NHWC (x [B, H, W, C], y / dy [B, Ho, Wo, Cout]), the weight what [Cout][t * ci + c] with
ci = C / groups and the tap t = ky * 3 + kx outermost in a row (k = 1: what [Cout][C]), dW in the same layout.  The convention, once:

    y[b, oy, ox, g * co + o] = bias[g * co + o] + sum over t, c of x[b, oy * s + ky - 1, ox * s + kx - 1, g * ci + c] * what[g * co + o][t * ci + c]

with x = 0 outside the image (padding 1; k = 1 has no padding and t = 0 only), Ho = (H - 1) / s + 1.  `_conv` is that sentence as code: zero-pad,
nine strided slices, one einsum per tap.

The bounds (`bars`) are derived from the number formats and the operation counts, never fitted to a result (U = 2^-23, BF16_STORE = 2^-8
as in gemm_reference.py, whose rules they follow):
  y, and dx by the view GEMM, the direct kernel or the parity-class stride-2 kernel (dx = "gemm")
                     fp32 accumulator over K = k * k * ci terms (k * k * co for dx): (K + 2) * U * (|x| (*) |w|); the bias is one epilogue
                     rounding, U * (|acc| + |bias|); the bf16 store is BF16_STORE * (|ref| + the above).  The stride-2 kernels sum
                     fewer taps at some pixels: K is an upper bound there.
  dx by ia_conv_nhwc_bwd_data, k = 3 (dx = "cols")
                     rounds twice by construction.  Each of the nine dcols entries d_t is an fp32 sum over the group's co output
                     channels stored as bf16: (co + 2) * U * S_t + BF16_STORE * (|d_t| + that).  col2im3_kernel adds up to nine of them in
                     fp32, (9 + 2) * U * sum_t |stored d_t|, and stores bf16 again.  test_conv_reference_host.py shows that the bar
                     needs the dcols store.
  dx by ia_conv3x3_s2_padded_bwd_data_t, shared-input form (dx = "slices")
                     n launches, one per 64-channel slice of dy; launch s adds its fp32 sum (K = 9 * 64) to the bf16 dx of the launches
                     before it in fp32 (one rounding) and stores bf16: per slice (K + 2) * U * S_s + U * |c_s| + BF16_STORE * (|c_s| + the
                     error so far), c_s the reference through slice s.  The host file shows that the per-slice store is needed.
  dW, dbias (fp32)   the accumulator rule with L = the number of pixels the kernel sums -- the caller counts them, zero border and
                     surplus tile pixels included -- over |dy|^T |x| (over sum |dy| for dbias), plus folds + 1 when folds > 1 partial
                     sums are folded (split-K slabs, or the direct kernels' per-workgroup banks: each fold is one more add).  dbias
                     gets one rounding more for the += onto the prior.  `folds` comes from what the library exports (the workspace
                     bytes: a slab or bank takes Cout * (K + 1) floats; for the direct kernels also at most one bank per tile, see
                     tests/test_conv_kernels_gpu.py), never from an observed error.  With L the count of ALL pixels the fold term is
                     slack -- a fold re-orders the same sum, which the any-order rule covers; it is what holds the bar when the
                     partial sums are shorter than the fold that follows them (the host file's one-pixel banks).
On `exact_operands` every bar is zero.
"""
from collections import namedtuple

import torch

from gemm_reference import BF16_STORE, F64, U, bf16_round, first_bad, holds, unheld, worst_ratio  # noqa: F401  (re-exported for the tests)

# ------------------------------------------------------------------------------------------------ the shapes of tests/test_conv_kernels_gpu.py
Conv = namedtuple("Conv", "B H W C Cout k stride groups")


def conv3(B, H, W, Cin, Cout, groups, stride=1):
    return Conv(B, H, W, Cin, Cout, 3, stride, groups)


DCONV_PAIRS = [(64, 64), (16, 32), (32, 64), (64, 32), (32, 16)]          # (ci, co) the direct kernel is built for (csrc/conv.hip)
DCONV_WGRAD_PAIRS = [(64, 64), (16, 32), (32, 64)]                       # ... and the direct weight gradient
DIRECT_MAPS = [(2, 9, 31), (1, 8, 30), (1, 1, 1), (1, 2, 61), (1, 16, 60)]
DIRECT_SHAPES = [conv3(B, H, W, ci, co, 1) for ci, co in DCONV_PAIRS for B, H, W in DIRECT_MAPS]
DIRECT_GROUP_SHAPES = [conv3(2, 9, 31, 128, 128, 2), conv3(1, 10, 33, 384, 384, 6)]
DIRECT_WALK_SHAPES = [conv3(3, 17, 61, 16 * 64, 32 * 64, 64), conv3(3, 17, 61, 64 * 32, 64 * 32, 32)]
VIEW_SHAPES = [conv3(1, 9, 10, 128, 64, 1), conv3(1, 7, 9, 256, 256, 1), conv3(2, 11, 8, 16, 16, 2), conv3(1, 10, 33, 1536, 1536, 6)]
VIEW_DGRAD_DIRECT_CAPABLE = conv3(2, 9, 31, 64, 64, 1)
S2_CHANNELS = [(64, 64, 1), (128, 128, 2), (384, 384, 6), (64, 128, 1), (64, 192, 1)]
S2_MAPS = [(5, 3, 2), (1, 1, 1), (2, 17, 61), (1, 16, 60), (2, 15, 59), (1, 8, 30)]
S2_SHAPES = [conv3(B, H, W, ci, co, g, 2) for ci, co, g in S2_CHANNELS for B, H, W in S2_MAPS]
NHWC_SHAPES = [Conv(2, 7, 9, 64, 64, 3, 1, 1), Conv(2, 7, 9, 64, 128, 3, 2, 1), Conv(1, 8, 8, 128, 128, 3, 2, 2), Conv(3, 5, 6, 48, 96, 3, 1, 6),
               Conv(1, 1, 1, 8, 8, 3, 1, 1), Conv(2, 6, 5, 256, 512, 3, 2, 1), Conv(2, 7, 9, 64, 256, 1, 1, 1), Conv(1, 3, 3, 8, 8, 1, 1, 1)]
# (Cin, Cout, groups) of ia_conv3x3_flip_weights; the stem's shared-input form asks for (Cout, Cout, Cout / 64): (128, 128, 2), (192, 192, 3)
FLIP_SHAPES = [(ci, co, 1) for ci, co in DCONV_PAIRS] + [(128, 128, 2), (192, 192, 3), (384, 384, 6)]
GPU_SHAPES = DIRECT_SHAPES + DIRECT_GROUP_SHAPES + DIRECT_WALK_SHAPES + VIEW_SHAPES + [VIEW_DGRAD_DIRECT_CAPABLE] + S2_SHAPES + NHWC_SHAPES


def shared_slices(s):
    """n for the stem's shared-input stride-2 form (groups = 1, Cin = 64, Cout = 64 n, n > 1), else 1"""
    return s.Cout // 64 if (s.stride == 2 and s.groups == 1 and s.C == 64 and s.Cout > 64) else 1


def out_hw(s):
    if s.k == 1:
        return s.H, s.W
    return (s.H - 1) // s.stride + 1, (s.W - 1) // s.stride + 1


# ------------------------------------------------------------------------------------------------ layouts
def to_bordered(t, fill=0.0):
    """compact [B, H, W, C] -> [B, H + 2, W + 2, C] with `fill` in the border"""
    B, H, W, C = t.shape
    out = torch.full((B, H + 2, W + 2, C), fill, dtype=t.dtype, device=t.device)
    out[:, 1:-1, 1:-1] = t
    return out


def interior(tp):
    """bordered [B, H + 2, W + 2, C] -> the compact view of its interior"""
    return tp[:, 1:-1, 1:-1]


def flipped_bank(what, Cin, Cout, groups):
    """what ia_conv3x3_flip_weights writes: what_t [g][ci][(8 - t) * co + o] = what [g][o][t * ci + c], as [Cin, 9 * co]"""
    ci, co = Cin // groups, Cout // groups
    return what.view(groups, co, 9, ci).flip(2).permute(0, 3, 2, 1).reshape(Cin, 9 * co).contiguous()


# ------------------------------------------------------------------------------------------------ the reference
def _conv(s, x, what, dy, per_tap=False):
    """y (without bias), dx, dW [Cout, k * k * ci] of shape `s` in the dtype of the operands; per_tap: also the nine (k * k) separate
    contributions to dx, [k * k, B, H, W, C] (what ia_conv_nhwc_bwd_data's dcols hold, at the pixel each is added to)"""
    B, H, W, C = x.shape
    g, kk = s.groups, s.k * s.k
    ci, co = C // g, s.Cout // g
    Ho, Wo = out_hw(s)
    pad = 1 if s.k == 3 else 0
    xp = torch.zeros((B, H + 2 * pad, W + 2 * pad, g, ci), dtype=x.dtype, device=x.device)
    xp[:, pad:pad + H, pad:pad + W] = x.view(B, H, W, g, ci)
    wg = what.view(g, co, kk, ci)
    dyg = dy.view(B, Ho, Wo, g, co)
    y = torch.zeros((B, Ho, Wo, g, co), dtype=x.dtype, device=x.device)
    dxp = torch.zeros_like(xp)
    dW = torch.zeros((g, co, kk, ci), dtype=x.dtype, device=x.device)
    each = []
    for t in range(kk):
        ky, kx = divmod(t, s.k)
        # output pixel (oy, ox) reads input pixel (oy * stride + ky - pad, ox * stride + kx - pad) = padded (oy * stride + ky, ox * stride + kx)
        rows = slice(ky, ky + s.stride * (Ho - 1) + 1, s.stride)
        cols = slice(kx, kx + s.stride * (Wo - 1) + 1, s.stride)
        xs = xp[:, rows, cols]
        y += torch.einsum("bhwgc,goc->bhwgo", xs, wg[:, :, t])
        d = torch.einsum("bhwgo,goc->bhwgc", dyg, wg[:, :, t])
        dxp[:, rows, cols] += d
        dW[:, :, t] = torch.einsum("bhwgo,bhwgc->goc", dyg, xs)
        if per_tap:
            one = torch.zeros_like(xp)
            one[:, rows, cols] = d
            each.append(one[:, pad:pad + H, pad:pad + W].reshape(B, H, W, C))
    out = (y.reshape(B, Ho, Wo, s.Cout), dxp[:, pad:pad + H, pad:pad + W].reshape(B, H, W, C), dW.reshape(s.Cout, kk * ci))
    return out + (torch.stack(each),) if per_tap else out


def d(x):
    return None if x is None else x.to(F64)


def reference(s, ops):
    """fp64 of every output of shape `s`: y (+ bias), dx, dW, dbias (prior + the sum of dy over the pixels)"""
    x, what, dy = d(ops["x"]), d(ops["what"]), d(ops["dy"])
    y, dx, dW = _conv(s, x, what, dy)
    return {"y": y + d(ops["bias"]), "dx": dx, "dW": dW, "dbias": d(ops["dbias0"]) + dy.sum((0, 1, 2))}


def slice_refs(s, ops):
    """the shared-input form's dx after each of its n launches: [n][B, H, W, 64] (the last one is reference()["dx"])"""
    n = shared_slices(s)
    x, what, dy = d(ops["x"]), d(ops["what"]), d(ops["dy"])
    one = Conv(s.B, s.H, s.W, 64, 64, 3, 2, 1)
    parts = [_conv(one, x, what[64 * i:64 * i + 64], dy[..., 64 * i:64 * i + 64].contiguous())[1] for i in range(n)]
    return torch.stack(parts).cumsum(0), parts


def bars(s, ops, dx="gemm", L=None, folds=1, exact=False, without=None):
    """per-element bound of |got - reference| for y, dx, dW and dbias of shape `s` (see the module text).  dx: how the data gradient is
    formed ("gemm", "cols", "slices"); L: the number of pixels the weight-gradient kernel sums; folds: the partial sums it folds.
    without ("cols_store", "slice_store", "fold"): the bar with that term left out, for the host tests that show what each term is for."""
    ref = reference(s, ops)
    if exact:
        return {k: torch.zeros_like(v) for k, v in ref.items()}
    x, what, dy, bias, prior = (d(ops[k]).abs() for k in ("x", "what", "dy", "bias", "dbias0"))
    g, kk = s.groups, s.k * s.k
    ci, co = s.C // g, s.Cout // g
    Sy, Sdx, SdW = _conv(s, x, what, dy)
    out = {}
    e = (kk * ci + 2) * U * Sy
    e = e + U * ((ref["y"] - d(ops["bias"])).abs() + bias)
    out["y"] = e + BF16_STORE * (ref["y"].abs() + e)
    if dx == "gemm":
        e = (kk * co + 2) * U * Sdx
    elif dx == "cols":
        assert s.k == 3
        St = _conv(s, x, what, dy, per_tap=True)[3]
        each = _conv(s, d(ops["x"]), d(ops["what"]), d(ops["dy"]), per_tap=True)[3].abs()      # |d_t|, where each is added
        e1 = (co + 2) * U * St                                                                  # the fp32 sum of a dcols entry ...
        if without != "cols_store":
            e1 = e1 + BF16_STORE * (each + e1)                                                  # ... and its bf16 store
        stored = (each + e1).sum(0)
        e = e1.sum(0) + (9 + 2) * U * stored                                                    # col2im3_kernel's fp32 sum of up to nine
    else:
        assert dx == "slices"
        cum, _ = slice_refs(s, ops)
        one = Conv(s.B, s.H, s.W, 64, 64, 3, 2, 1)
        e = torch.zeros_like(ref["dx"])
        for i in range(shared_slices(s)):
            Ss = _conv(one, x, what[64 * i:64 * i + 64], dy[..., 64 * i:64 * i + 64].contiguous())[1]
            e = e + (9 * 64 + 2) * U * Ss + (U * cum[i].abs() if i else 0.0)
            if i + 1 < shared_slices(s) and without != "slice_store":
                e = e + BF16_STORE * (cum[i].abs() + e)                                          # (the last store is added below)
    out["dx"] = e + BF16_STORE * (ref["dx"].abs() + e)
    assert L is not None and folds >= 1
    Lw = L + 2 + (folds + 1 if folds > 1 and without != "fold" else 0)
    tot = dy.sum((0, 1, 2))
    out["dW"] = Lw * U * SdW
    out["dbias"] = Lw * U * tot + U * (tot + prior)
    return out


# ------------------------------------------------------------------------------------------------ operands
POOL = 6_400_000       # elements per draw: the largest tensor of the GPU file is dy [3, 17, 61, 2048]


def _tern(g, n):
    """{-1, 0, 1}, non-zero half of the time"""
    sign = torch.randint(0, 2, (n,), generator=g, device=g.device) * 2 - 1
    return (sign * torch.randint(0, 2, (n,), generator=g, device=g.device)).to(torch.float32)


def exact_pool(g, n=POOL):
    ints = torch.randint(-3, 4, (2, 4096), generator=g, device=g.device).to(torch.float32)
    return {"x": _tern(g, n), "what": _tern(g, n), "dy": _tern(g, n), "bias": ints[0], "dbias0": ints[1]}


def normal_pool(g, n=POOL):
    """ordinary operands, as elsewhere in the suite: randn x and dy rounded to bf16, what = randn x a per-output-channel factor in
    0.05 .. 0.4 (applied by _cut) rounded to bf16, fp32 bias and prior"""
    r16 = lambda t: t.to(torch.bfloat16).to(torch.float32)
    randn = lambda m: torch.randn((m,), generator=g, device=g.device)
    return {"x": r16(randn(n)), "what": randn(n), "dy": r16(randn(n)), "bias": randn(4096), "dbias0": randn(4096),
            "factor": 0.05 + 0.35 * torch.rand((4096,), generator=g, device=g.device)}


def _cut(pool, s, device):
    Ho, Wo = out_hw(s)
    K = s.k * s.k * (s.C // s.groups)
    nx, nw, ny = s.B * s.H * s.W * s.C, s.Cout * K, s.B * Ho * Wo * s.Cout
    assert max(nx, nw, ny) <= pool["x"].numel() and s.Cout <= 4096, s
    what = pool["what"][:nw].view(s.Cout, K)
    if "factor" in pool:
        what = (what * pool["factor"][:s.Cout, None]).to(torch.bfloat16).to(torch.float32)
    # x from the front of its draw and dy from the back of its own: two cases of different shapes do not share a prefix of both
    return {"x": pool["x"][:nx].view(s.B, s.H, s.W, s.C).to(device), "what": what.contiguous().to(device),
            "dy": pool["dy"][-ny:].view(s.B, Ho, Wo, s.Cout).to(device), "bias": pool["bias"][:s.Cout].to(device),
            "dbias0": pool["dbias0"][:s.Cout].to(device)}


def exact_operands(pool, s, device="cpu", cols=False):
    """Inputs of shape `s` cut from exact_pool's draws (or drawn from a torch.Generator handed in its place) on which every output is a
    number its type holds exactly, whatever the order of the sum: x, what and dy in {-1, 0, 1} (non-zero half of the time), bias and
    the prior dbias whole numbers in -3 .. 3 -- bf16 holds whole numbers up to 256, fp32 sums of whole numbers stay exact below 2^24.
    That every expected output (and every intermediate the kernels store as bf16: the nine dcols entries of the patch-matrix data
    gradient, the dx of each launch of the shared-input form) survives the round trip through its type is ASSERTED here from the fp64
    reference: it is the precondition of the tests' equality check (cols: the shape goes through ia_conv_nhwc_bwd_data, check the dcols
    entries too).  Returns the operands with "ref" added."""
    if isinstance(pool, torch.Generator):
        pool = exact_pool(pool)
    ops = _cut(pool, s, device)
    ref = reference(s, ops)
    for key, f32 in (("y", False), ("dx", False), ("dW", True), ("dbias", True)):
        assert holds(ref[key], f32), (tuple(s), key, "an expected element does not fit its type", unheld(ref[key], f32))
    if cols and s.k == 3:
        each = _conv(s, d(ops["x"]), d(ops["what"]), d(ops["dy"]), per_tap=True)[3]
        assert holds(each, False), (tuple(s), "a dcols entry is no bf16 number", unheld(each, False))
    if shared_slices(s) > 1:
        cum, _ = slice_refs(s, ops)
        assert holds(cum, False), (tuple(s), "the dx of a slice launch is no bf16 number", unheld(cum, False))
    ops["ref"] = ref
    return ops


def normal_operands(pool, s, device="cpu"):
    if isinstance(pool, torch.Generator):
        pool = normal_pool(pool)
    ops = _cut(pool, s, device)
    ops["ref"] = reference(s, ops)
    return ops


def first_bad_nd(got, want, bar):
    """first_bad on tensors of any rank: rows = everything but the last (channel) axis"""
    c = got.shape[-1]
    return first_bad(got.reshape(-1, c), want.reshape(-1, c), bar.reshape(-1, c)) if got.dim() > 1 else first_bad(got, want, bar)
