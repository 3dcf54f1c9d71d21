"""The LayerNorm tail, the column sums (csrc/layernorm.hip), BatchNorm / GroupNorm + ReLU, MaxPool 3x3/2, the strided row subsampling
and the generic NCHW patch gather (csrc/resnet.hip) through the C ABI against the fp64 references of tests/norm_reference.py, element by
element, with the bars of tests/fp64_bars.py.  Every bound is derived from the kernel's arithmetic and stated beside its use.

The statistics of BatchNorm and GroupNorm are taken in ONE pass: var = q / n - mu^2 in fp32, with q = sum x^2, mu = sum x / n.  With c_s
the longest chain of roundings behind a channel's sum (`_bn_chain`, `_gn_chain`) the mean is off by at most (c_s + 1) 2^-24 E|x|, and since
|mu| E|x| <= E[x^2] the variance is off by at most

    e_var = c_v 2^-24 (E[x^2] + mu^2),    c_v = 3 c_s + 5

(on E[x^2]: c_s + 2 for q / n, 2 (c_s + 1) for the mean's error in mu^2, 1 for the subtraction; on mu^2: 1 for the product).  That is an
ABSOLUTE error: it does not shrink with the variance.  rstd carries half of it relative to the variance, so the variance error alone reaches one bf16 ulp (2^-8)
of y when e_var = 2^-7 sigma^2, i.e. with E[x^2] + mu^2 = sigma^2 + 2 mu^2 at

    mu^2 / sigma^2 = (2^17 / c_v - 1) / 2.

For the worst chain the tests run (C = 8, 33000 rows: c_s = 304, c_v = 917) that is mu^2 / sigma^2 = 71, |mean| = 8.4 sigma; for a tower
shape (C = 256, 200704 rows: c_s = 104, c_v = 317) it is 206, |mean| = 14 sigma.  The bound is the worst case of a chain whose roundings
all point one way; the error a run prints is far smaller.  The "offset" input set (mu^2 / sigma^2 = 36) sits below both limits.

The backward of both norms recomputes the ReLU mask from xhat * gamma + beta <= 0.  The references take the mask as an argument, and the
tests hand them the mask of the kernel's OWN forward output (y > 0): a pre-activation within rounding of zero cannot flip a term, while a
backward that disagrees with its forward about one element moves dx there by a whole gradient and fails the bar.  Separately, that mask
may differ from the fp64 mask only where the fp64 pre-activation lies within its fp32 bound of zero, and in fewer than 0.1 % of the
elements (tests/test_norm_reference_host.py shows on the CPU that the inputs themselves stay far below that).
"""
import math

import pytest
import torch

import glue_reference as R
import norm_reference as N
from fp64_bars import U24, _ratio, bf16_close, bits, sum_close
from test_glue_kernels_gpu import _ln_chain, nv_of

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ERR_ARG, ERR_WS = -1, -3
NAN = float("nan")


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


def P(t):
    return None if t is None else t.data_ptr()


def dv(t):
    """device copy of a host tensor; the caller keeps it in a name until the call has run -- a temporary freed right after its pointer
    was taken would be handed to the next allocation"""
    return None if t is None else t.to("cuda")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype)


def full(shape, value, dtype=F32):
    return torch.full(shape, value, device="cuda", dtype=dtype)


def cdiv(a, b):
    return (a + b - 1) // b


def f32(v):
    """a host scalar as the C ABI's float argument carries it"""
    return float(torch.tensor(v, dtype=F32))


# =============================================================================================================== refusals
def _refusal_cases(p, ws):
    """(entry point, valid tiny argument list, [(changes {index: value}, expected code)]).  p = a zeroed device buffer far larger than
    anything the tiny valid extents could touch; ws = {name: workspace bytes of the valid call}.  Every change is one the C code rejects
    in front of its first launch."""
    s = None
    nulls = lambda idx: [({i: None}, ERR_ARG) for i in idx]
    h_bad = lambda i: [({i: 0}, ERR_ARG), ({i: -8}, ERR_ARG), ({i: 12}, ERR_ARG), ({i: 4104}, ERR_ARG)]
    bn = [p] * 8 + [2, 8, 1, 1e-5, 0.1, 1, 1, p, ws["bn"], s]
    bnb = [p] * 10 + [2, 8, 1, 1, 1, p, ws["bn"], s]
    gn = [p] * 6 + [2, 8, 1, 2, 1e-5, 1, p, ws["gn"], s]
    gnb = [p] * 10 + [2, 8, 1, 2, 1, p, ws["gn"], s]
    return [
        ("ia_ln_fwd", [p] * 9 + [1, 8, 1e-5, 0.0, 0, 0, s], nulls((0, 4, 5, 6, 7)) + [({9: 0}, ERR_ARG)] + h_bad(10)),
        ("ia_ln_fwd_rows", [p] * 9 + [1, 8, 1e-5, 0.0, 0, 0, p, s], nulls((0, 4, 5, 6, 7)) + [({9: 0}, ERR_ARG)] + h_bad(10)),
        ("ia_ln_bwd", [p] * 11 + [1, 8, 0.0, 0, 0, p, ws["ln"], 0, s],
         nulls((0, 2, 3, 4, 5, 6)) + [({11: 0}, ERR_ARG)] + h_bad(12) +
         [({17: ws["ln"] - 1}, ERR_WS), ({16: None}, ERR_WS), ({7: None, 13: 0.1}, ERR_ARG)]),
        ("ia_ln_bwd2_rows", [p] * 12 + [1, 8, 0.0, 0, 0, p, p, ws["ln"], 0, s],
         nulls((0, 3, 4, 5, 6, 7)) + h_bad(13) + [({8: None, 14: 0.1}, ERR_ARG), ({19: ws["ln"] - 1}, ERR_WS)]),
        ("ia_colsum", [p, 8, 1, 8, p, 0, p, ws["cs"], s],
         nulls((0, 4)) + [({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({3: 12, 1: 16}, ERR_ARG), ({1: 12}, ERR_ARG), ({6: None}, ERR_WS),
                          ({7: ws["cs"] - 1}, ERR_WS)]),
        ("ia_bn_act_fwd", bn,
         nulls((0, 1, 2, 5, 6, 7)) + [({8: 0}, ERR_ARG), ({9: 0}, ERR_ARG), ({9: 12}, ERR_ARG), ({10: 0}, ERR_ARG), ({8: 3, 10: 2}, ERR_ARG),
                                      ({15: None}, ERR_WS), ({16: ws["bn"] - 1}, ERR_WS), ({13: 0, 3: None}, ERR_ARG), ({13: 0, 4: None}, ERR_ARG)]),
        ("ia_bn_act_bwd", bnb,
         nulls((0, 1, 2, 3, 4, 5, 7)) + [({10: 0}, ERR_ARG), ({11: 0}, ERR_ARG), ({11: 12}, ERR_ARG), ({12: 0}, ERR_ARG), ({10: 3, 12: 2}, ERR_ARG),
                                         ({15: None}, ERR_WS), ({16: ws["bn"] - 1}, ERR_WS)]),
        ("ia_gn_act_fwd", gn,
         nulls((0, 1, 2, 3, 4, 5)) + [({6: 0}, ERR_ARG), ({7: 0}, ERR_ARG), ({7: 12}, ERR_ARG), ({8: 0}, ERR_ARG), ({6: 3, 8: 2}, ERR_ARG),
                                      ({6: 65536, 8: 65536}, ERR_ARG), ({9: 0}, ERR_ARG), ({9: 3}, ERR_ARG), ({12: None}, ERR_WS),
                                      ({13: ws["gn"] - 1}, ERR_WS)]),
        ("ia_gn_act_bwd", gnb,
         nulls((0, 1, 2, 3, 4, 5, 7)) + [({10: 0}, ERR_ARG), ({11: 12}, ERR_ARG), ({12: 0}, ERR_ARG), ({10: 3, 12: 2}, ERR_ARG),
                                         ({10: 65536, 12: 65536}, ERR_ARG), ({13: 0}, ERR_ARG), ({13: 3}, ERR_ARG), ({15: None}, ERR_WS),
                                         ({16: ws["gn"] - 1}, ERR_WS)]),
        ("ia_patches_nchw", [p, p, 1, 1, 2, 2, 1, 1, 0, 8, s],
         nulls((0, 1)) + [({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({7: 0}, ERR_ARG), ({8: -1}, ERR_ARG),
                          ({9: 0}, ERR_ARG), ({9: 12}, ERR_ARG), ({6: 2, 8: 1, 3: 3, 9: 8}, ERR_ARG), ({6: 3, 9: 16}, ERR_ARG)]),
        ("ia_maxpool3s2_fwd", [p, p, p, 1, 2, 2, 8, s], nulls((0, 1, 2)) + [({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({6: 12}, ERR_ARG)]),
        ("ia_maxpool3s2_fwd_ex", [p, p, p, 1, 2, 2, 8, 1, s], nulls((0, 1, 2)) + [({3: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 12}, ERR_ARG)]),
        ("ia_maxpool3s2_bwd", [p, p, p, 1, 2, 2, 8, s], nulls((0, 1, 2)) + [({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({6: 12}, ERR_ARG)]),
        ("ia_rows_subsample_fwd", [p, p, 1, 2, 2, 8, 1, s], nulls((0, 1)) + [({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({5: 12}, ERR_ARG), ({6: 0}, ERR_ARG)]),
        ("ia_rows_subsample_bwd", [p, p, p, 1, 2, 2, 8, 1, s], nulls((0, 2)) + [({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({6: 12}, ERR_ARG), ({7: 0}, ERR_ARG)]),
    ]


def test_every_documented_precondition_is_refused_before_any_launch(gpu, lib):
    """One call per documented precondition of the entry points of this file: a null required pointer, a non-positive extent, H % 8,
    H > 4096, C % 8, rows % segments, C % groups, more than 65535 images, Kp < k k C, an empty output map, a short or null workspace,
    dropout without dx, eval mode without running statistics.  Each returns its documented code, and the buffer every pointer argument
    points at -- zeroed, far larger than the tiny valid extents -- is still all zero afterwards: nothing was launched."""
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    ws = {"ln": lib.ia_ln_bwd_workspace_bytes(1, 8), "cs": lib.ia_colsum_workspace_bytes(1, 8), "bn": lib.ia_bn_act_workspace_bytes(2, 8, 1),
          "gn": lib.ia_gn_act_workspace_bytes(2, 8, 1)}
    assert all(0 < v <= buf.numel() for v in ws.values()), ws
    assert lib.ia_bn_act_workspace_bytes(3, 8, 2) == 0 and lib.ia_gn_act_workspace_bytes(3, 8, 2) == 0
    cases = _refusal_cases(buf.data_ptr(), ws)
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
    print(f"[norm] refusals: {n} calls over {len(cases)} entry points")


# =============================================================================================================== LayerNorm tail, forward
def _ln_fwd(lib, x, bias, res, gamma, beta, eps, p=0.0, seed=0, sid=0, want_z=True, live=None):
    """outputs pre-filled (9.0 / NaN): an element the kernel does not write shows"""
    M, H = x.shape
    y, z = full((M, H), 9.0, BF16), (full((M, H), 9.0, BF16) if want_z else None)
    mean, rstd = full((M,), NAN), full((M,), NAN)
    keepalive = [dv(t) for t in (x, bias, res, gamma, beta, live)]
    xd, bd, rd, gd, betad, ld = keepalive
    if live is None:
        ok(lib.ia_ln_fwd(P(xd), P(bd), P(rd), P(z), P(y), P(mean), P(rstd), P(gd), P(betad), M, H, eps, p, seed, sid, st()), "ia_ln_fwd")
    else:
        ok(lib.ia_ln_fwd_rows(P(xd), P(bd), P(rd), P(z), P(y), P(mean), P(rstd), P(gd), P(betad), M, H, eps, p, seed, sid, P(ld), st()),
           "ia_ln_fwd_rows")
    return z, y, mean, rstd


def _check_ln_fwd(tag, x, bias, res, gamma, beta, eps, out, keep=None, inv_keep=1.0):
    z, y, mean, rstd = out
    M, H = x.shape
    z64 = N.ln_tail_fwd(x, bias, res, gamma, beta, eps, keep, inv_keep)[0]
    # z = bf16(((x + bias) * inv_keep) + res): three fp32 roundings in front of the bf16 one; a dropped element is res exactly
    branch = x.to(F64).abs() + (bias.to(F64).abs() if bias is not None else 0.0)
    if keep is not None:
        branch = branch * inv_keep * keep.to(F64)
    bf16_close(tag + " z", z, z64, 3 * U24 * (branch + (res.to(F64).abs() if res is not None else 0.0)))
    # statistics and y are documented as those of the rounded z: the fp64 LayerNorm of the z the kernel wrote
    zg = z.cpu().to(F64)
    y64, mean64, rstd64 = R.layernorm_fwd(zg, gamma, beta if beta is not None else torch.zeros(H), eps)
    A = zg.abs().mean(1)
    # mean: NV * 8 additions per lane, 6 steps of the wave reduction, one division
    c_m = nv_of(H) * 8 + 6 + 1
    sum_close(tag + " mean", mean, mean64, A, c_m)
    # rstd = rsqrt(sum d^2 / H + eps): positive terms, so S = var + eps; NV * 8 additions per lane of terms that carry a subtraction and
    # a square, 6 reduction steps, the division and the + eps: c_q; the mean's own error enters squared (sum d = 0); rsqrt halves the
    # relative error of its argument and adds its own (2 * 2^-24) and the final rounding
    c_q = nv_of(H) * 8 + 2 + 6 + 2
    rel = U24 * (0.5 * c_q + 3) + 0.5 * (c_m * U24 * A) ** 2 * rstd64 ** 2
    r = _ratio(tag + " rstd", (rstd.cpu().to(F64) - rstd64).abs(), rel * rstd64)
    assert r <= 1.0, (tag, "rstd", r)
    # y = bf16((z - mean) * rstd * gamma + beta): the mean's error and 8 roundings on the magnitudes involved, the rstd error on xhat
    dev = (zg - mean64[:, None]).abs()
    g = gamma.to(F64).abs()
    S = (dev + A[:, None]) * rstd64[:, None] * g + (beta.to(F64).abs() if beta is not None else 0.0)
    bf16_close(tag + " y", y, y64, (c_m + 8) * U24 * S + (rel * rstd64)[:, None] * dev * g)


def _ln_inputs(M, H, seed):
    g = gen(seed)
    return dict(x=randn((M, H), seed, 2.0, BF16), bias=randn((H,), seed + 1, 0.3), res=randn((M, H), seed + 2, 1.0, BF16),
                gamma=torch.rand(H, generator=g) + 0.5, beta=randn((H,), seed + 3, 0.3))


LN_FWD_SHAPES = [(37, H) for H in (8, 504, 512, 520, 768, 1024, 1536, 2048, 2056, 4096)] + [(1, 768), (5, 768), (2051, 768)]


@pytest.mark.parametrize("M,H", LN_FWD_SHAPES)
def test_ln_fwd_every_width_and_option(gpu, lib, M, H):
    """ia_ln_fwd over the NV template: NV = 1 (8, 504, 512), the partial second slab (520), NV = 2, 3, 4, the `default: 8` arm with 5 of
    its 8 slabs (2056: the col < H guard) and all of them (4096); one row, 5 rows, 37 = nine blocks and a wave, 2051.  With and without
    bias, with and without residual, beta NULL, eps 1e-12 and 1e-6; z_out NULL must change no bit of y / mean / rstd."""
    i = _ln_inputs(M, H, 1000 + M + H)
    tag = f"ln_fwd[{M}x{H}]"
    first = None
    for use_bias, use_res, use_beta, eps in ((1, 1, 1, 1e-12), (0, 1, 1, 1e-6), (1, 0, 1, 1e-6), (0, 0, 1, 1e-12), (1, 1, 0, 1e-6)):
        eps = f32(eps)
        bias, res, beta = (i["bias"] if use_bias else None), (i["res"] if use_res else None), (i["beta"] if use_beta else None)
        out = _ln_fwd(lib, i["x"], bias, res, i["gamma"], beta, eps)
        _check_ln_fwd(f"{tag} bias={use_bias} res={use_res} beta={use_beta} eps={eps:g}", i["x"], bias, res, i["gamma"], beta, eps, out)
        first = first or out
        if not (use_bias or use_res):
            bits(tag + " z of a bare LayerNorm is x", out[0], i["x"])
    _, y, mean, rstd = _ln_fwd(lib, i["x"], i["bias"], i["res"], i["gamma"], i["beta"], f32(1e-12), want_z=False)
    bits(tag + " y without z_out", y, first[1]), bits(tag + " mean without z_out", mean, first[2]), bits(tag + " rstd without z_out", rstd, first[3])


@pytest.mark.parametrize("H", [520, 768])
@pytest.mark.parametrize("eps", [1e-12, 1e-6])
def test_ln_fwd_constant_row_and_far_off_mean(gpu, lib, H, eps):
    """Row 0 is constant: every partial sum of H copies of a bf16 number (8 significand bits, H <= 4096) is exact in fp32, so the mean is
    the value itself, the variance exactly 0, rstd = eps^-1/2 and y = bf16(beta), bit for bit -- a one-pass variance would not do that.
    Rows 1 and 2 have |mean| = 100 std: the two-pass bars hold unchanged (the mean's error enters the variance squared)."""
    M, eps = 5, f32(eps)
    i = _ln_inputs(M, H, 77 + H)
    x = i["x"].to(F32)
    x[0] = 1.5
    x[1] = 100.0 + randn((H,), 5)
    x[2] = -200.0 + 2.0 * randn((H,), 6)
    x = x.to(BF16)
    out = _ln_fwd(lib, x, None, None, i["gamma"], i["beta"], eps)
    tag = f"ln_fwd rows[{H}, eps={eps:g}]"
    _check_ln_fwd(tag, x, None, None, i["gamma"], i["beta"], eps, out)
    z, y, mean, rstd = (t.cpu() for t in out)
    assert float(mean[0]) == 1.5
    bits(tag + " y of the constant row", y[0], i["beta"].to(F64))
    r = abs(float(rstd[0]) * math.sqrt(eps) - 1.0)
    assert r <= 4 * U24, (tag, "rstd of the constant row", r)         # rsqrt of an exact eps: its own error and the rounding
    s = x.to(F64)[1:3]
    ratio = s.mean(1).abs() / s.std(1, unbiased=False)
    assert (ratio > 80).all() and (ratio < 125).all(), ratio


@pytest.mark.parametrize("H", [768, 520])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_ln_fwd_dropout_is_the_host_replica_of_the_hash(gpu, lib, H, p):
    """Dropout of the GEMM branch: z equals res bit for bit (res is a bf16 number: its one rounding changes nothing) exactly where
    keep_mask(seed, stream, M * H, p) drops, kept elements carry inv_keep (checked with and without the other addends), the kept share
    lies within 4 binomial standard deviations of 1 - thr16 / 65536, another stream id draws another mask."""
    M, seed, sid, eps = 37, 20240229, 5, f32(1e-6)
    i = _ln_inputs(M, H, 500 + H)
    thr16, inv_keep = R.drop_params(p)
    keep = R.keep_mask(seed, sid, M * H, p).reshape(M, H)
    tag = f"ln_fwd dropout[{H}, p={p}]"
    out = _ln_fwd(lib, i["x"], i["bias"], i["res"], i["gamma"], i["beta"], eps, p, seed, sid)
    bits(tag + " z where dropped", out[0].cpu()[~keep], i["res"][~keep])
    _check_ln_fwd(tag, i["x"], i["bias"], i["res"], i["gamma"], i["beta"], eps, out, keep, inv_keep)
    # x alone: exact zeros where dropped (the bound is zero there), bf16(x * inv_keep) where kept
    x1 = (i["x"].to(F32).abs() + 0.5).to(BF16)
    out = _ln_fwd(lib, x1, None, None, i["gamma"], None, eps, p, seed, sid)
    _check_ln_fwd(tag + " x alone", x1, None, None, i["gamma"], None, eps, out, keep, inv_keep)
    assert torch.equal(out[0].cpu() != 0, keep), (tag, "the zeros of z are not the mask")
    q = thr16 / 65536
    assert abs(int(keep.sum()) - M * H * (1 - q)) <= 4 * math.sqrt(M * H * q * (1 - q)), (tag, int(keep.sum()))
    keep2 = R.keep_mask(seed, sid + 1, M * H, p).reshape(M, H)
    assert 0.05 < float((keep2 != keep).float().mean()) < 0.6
    out = _ln_fwd(lib, x1, None, None, i["gamma"], None, eps, p, seed, sid + 1)
    assert torch.equal(out[0].cpu() != 0, keep2), (tag, "stream id + 1 did not draw the replica's mask")


@pytest.mark.parametrize("H", [520, 768])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_ln_fwd_rows_filter(gpu, lib, H, p):
    """ia_ln_fwd_rows: live rows are bit-identical to the unfiltered call (also under dropout: the stream is indexed by position), dead
    rows are exact zeros in y, z, mean and rstd."""
    M = 37
    i = _ln_inputs(M, H, 900 + H)
    live = torch.rand(M, generator=gen(3)) < 0.6
    live[0], live[M - 1] = True, False
    args = (i["x"], i["bias"], i["res"], i["gamma"], i["beta"], f32(1e-6), p, 99, 2)
    plain = _ln_fwd(lib, *args)
    filt = _ln_fwd(lib, *args, live=live.to(torch.uint8))
    for a, b, n in zip(filt, plain, ("z", "y", "mean", "rstd")):
        bits(f"ln_fwd_rows[{H}] live rows of {n}", a.cpu()[live], b.cpu()[live])
        iv = torch.int16 if a.dtype == BF16 else torch.int32
        assert (a.cpu()[~live].contiguous().view(iv) == 0).all(), (n, "dead rows must be exact zeros")
    filt_noz = _ln_fwd(lib, *args, live=live.to(torch.uint8), want_z=False)
    bits(f"ln_fwd_rows[{H}] y without z_out", filt_noz[1], filt[1])


# =============================================================================================================== LayerNorm tail, backward
def _ln_bwd_inputs(M, H, seed):
    z, dy, dres = randn((M, H), seed, 2.0, BF16), randn((M, H), seed + 1, 1.0, BF16), randn((M, H), seed + 2, 1.0, BF16)
    gamma = torch.rand(H, generator=gen(seed + 3)) + 0.5
    zf = z.to(F64)
    mean = zf.mean(1).to(F32)
    rstd = (1.0 / torch.sqrt(zf.var(1, unbiased=False) + 1e-5)).to(F32)
    return z, dy, dres, gamma, mean, rstd


LN_BWD_SHAPES = [(M, H) for M in (37, 397) for H in (8, 520, 768, 2056, 4096)] + [(2051, H) for H in (8, 520, 768, 2056)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M,H", LN_BWD_SHAPES)
def test_ln_bwd_all_outputs_with_dropout(gpu, lib, M, H, p):
    """ia_ln_bwd (dy2 = NULL): dz, dx, dgamma, dbeta, dbias per element.  M = 37, 397, 2051 give 10, 100 and 512 blocks of partials: below,
    across and inside the four-chain loop of the second stage.  (2051 x 4096 would be 8.4 M elements and is left out: both extents are run,
    each against the other's smaller values.)  Under dropout dx = bf16(keep * dz * inv_keep) with dz before ITS rounding, exactly zero
    where the mask drops -- the mask ia_ln_fwd draws at the same (seed, stream id) -- and dbias is the column sum of that fp32 dx;
    without dropout dx is not written and dbias sums dz.  accumulate = 0 over NaN-filled outputs and accumulate = 1 over 0.5."""
    seed, sid = 4242, 9
    z, dy, dres, gamma, mean, rstd = _ln_bwd_inputs(M, H, 2000 + M + H)
    thr16, inv_keep = R.drop_params(p)
    keep = R.keep_mask(seed, sid, M * H, p).reshape(M, H) if p > 0 else None
    ws_bytes = lib.ia_ln_bwd_workspace_bytes(M, H)
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)
    zd, dyd, dresd, gd, md, rd = (dv(t) for t in (z, dy, dres, gamma, mean, rstd))
    dz64, dx64, dgamma64, dbeta64, dbias64 = N.ln_tail_bwd(dy, dres, z, mean, rstd, gamma, keep, inv_keep)
    xh = (z.to(F64) - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]
    ga = (dy.to(F64) * gamma.to(F64)).abs()
    # a row's dz: rstd * (g - mean(g) - xhat * mean(g * xhat)): per lane NV * 8 additions, 6 reduction steps, 10 operations around them
    c_row = nv_of(H) * 8 + 6 + 10
    S_row = rstd.to(F64)[:, None] * (ga + ga.mean(1, keepdim=True) + xh.abs() * (ga * xh.abs()).mean(1, keepdim=True)) + dres.to(F64).abs()
    m = keep.to(F64) * inv_keep if p > 0 else torch.ones(M, H, dtype=F64)
    c = _ln_chain(M)
    tag = f"ln_bwd[{M}x{H}, p={p}]"
    for accumulate, prior in ((0, 0.0), (1, 0.5)):
        dz = full((M, H), 9.0, BF16)
        dx = full((M, H), 9.0, BF16) if p > 0 else None
        outs = [full((H,), 0.5 if accumulate else NAN) for _ in range(3)]
        ok(lib.ia_ln_bwd(P(dyd), P(dresd), P(zd), P(md), P(rd), P(gd), P(dz), P(dx), *(P(o) for o in outs), M, H, p, seed, sid, P(ws), ws_bytes,
                         accumulate, st()), "ia_ln_bwd")
        t = f"{tag} acc={accumulate}"
        bf16_close(t + " dz", dz, dz64, (c_row + 1) * U24 * S_row)
        if p > 0:
            # one more multiplication; the bound is zero where the mask drops: exact zeros
            bf16_close(t + " dx", dx, dx64, (c_row + 2) * U24 * S_row * m)
            assert (dx.cpu()[~keep].view(torch.int16) == 0).all()
        sum_close(t + " dgamma", outs[0], dgamma64 + prior, (dy.to(F64) * xh).abs().sum(0) + prior, c)
        sum_close(t + " dbeta", outs[1], dbeta64 + prior, dy.to(F64).abs().sum(0) + prior, c)
        # dbias sums the fp32 dz / dx (before the bf16 rounding): the row's error scale, summed, behind the row's own chain
        sum_close(t + " dbias", outs[2], dbias64 + prior, (S_row * m).sum(0) + prior, c + c_row + 1)
    if p > 0:
        x1 = (randn((M, H), 5).abs() + 0.5).to(BF16)
        zf = _ln_fwd(lib, x1, None, None, gamma, None, 1e-5, p, seed, sid)[0]
        assert torch.equal(zf.cpu() != 0, keep), (tag, "the forward's mask at this (seed, stream id) is another one")


def test_ln_bwd2_rows_flag_refill(gpu, lib):
    """ia_ln_bwd2_rows at H = 8, M = 64 * 2048 + 5: 512 blocks of 4 waves, so the 131072-th row on is a wave's 65th -- the only shape at
    which the kernel refills its 64 liveness flags.  A random filter over gradients that are zero in the dead rows: bit-identical to the
    unfiltered call, dead rows exact zeros (dz, and dx under dropout); dbeta also against fp64."""
    M, H, p, seed, sid = 64 * 2048 + 5, 8, 0.1, 31, 4
    z, dy, dres, gamma, mean, rstd = _ln_bwd_inputs(M, H, 3000)
    live = torch.rand(M, generator=gen(6)) < 0.55
    live[0], live[M - 1], live[M - 3] = True, False, True
    dy, dres = (torch.where(live[:, None], t, torch.zeros((), dtype=BF16)) for t in (dy, dres))
    ws_bytes = lib.ia_ln_bwd_workspace_bytes(M, H)
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)
    zd, dyd, dresd, gd, md, rd, lived = (dv(t) for t in (z, dy, dres, gamma, mean, rstd, live.to(torch.uint8)))

    def run(rows):
        dz, dx = full((M, H), 9.0, BF16), full((M, H), 9.0, BF16)
        outs = [full((H,), NAN) for _ in range(3)]
        ok(lib.ia_ln_bwd2_rows(P(dyd), None, P(dresd), P(zd), P(md), P(rd), P(gd), P(dz), P(dx), *(P(o) for o in outs), M, H, p, seed, sid,
                               P(rows), P(ws), ws_bytes, 0, st()), "ia_ln_bwd2_rows")
        return [dz, dx] + outs

    plain, filt = run(None), run(lived)
    for a, b, n in zip(filt, plain, ("dz", "dx", "dgamma", "dbeta", "dbias")):
        bits(f"ln_bwd2_rows[{M}x{H}] {n} under the row filter", a, b)
    for t in filt[:2]:
        assert (t.cpu()[~live].view(torch.int16) == 0).all(), "dead rows must be exact zeros"
    assert (filt[0].cpu()[live].view(torch.int16) != 0).any(1).all(), "a live row came out as zeros"
    sum_close(f"ln_bwd2_rows[{M}x{H}] dbeta", filt[3], dy.to(F64).sum(0), dy.to(F64).abs().sum(0), _ln_chain(M))


# =============================================================================================================== column sums
def _colsum_fold(M, N, ld):
    if ld != N or N >= 512 or 512 % N:
        return 1
    f = 512 // N
    return 1 if M % f else f


def _colsum_chain(M, N, ld):
    """colsum_kernel: a wave adds every (4 * row blocks)-th row of the (folded) matrix, 3 additions join the waves; second stage over
    row blocks * fold partials: a slice's chain of every 128th partial, up to 3 more in its tail loop, 2 to join the four chains, 32
    across the slices, the accumulation.  The terms are bf16 numbers: no rounding inside a term."""
    f = _colsum_fold(M, N, ld)
    Mw = M // f
    rb = min(256, cdiv(Mw, 4))
    return cdiv(Mw, rb * 4) + 3 + cdiv(rb * f, 128) + 3 + 2 + 32 + 1


@pytest.mark.parametrize("M,N,ld", [(128, 8, 8), (7, 8, 8), (96, 64, 64), (100, 256, 256), (5, 192, 192), (37, 520, 520), (37, 512, 776),
                                    (1030, 1024, 1024)])
def test_colsum_folds_strides_and_caps(gpu, lib, M, N, ld):
    """ia_colsum: folds of 64 (N = 8), 8 (N = 64) and 2 (N = 256); no fold because M % f != 0 (7 x 8) or 512 % N != 0 (192); a partial
    second column block (520); ld != N with NaN in the columns beyond N, which must not reach the result; the 256-block row cap (1030
    rows: two rows to some waves).  accumulate = 0 over a NaN-filled out, accumulate = 1 over a known prior."""
    assert (_colsum_fold(M, N, ld) > 1) == ((M, N) in ((128, 8), (96, 64), (100, 256)))
    x = torch.full((M, ld), NAN, dtype=BF16)
    x[:, :N] = (randn((M, N), 10 + M + N) + 0.3).to(BF16)
    xd = x.to(gpu)
    ws_bytes = lib.ia_colsum_workspace_bytes(M, N)
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)
    x64 = x[:, :N].to(F64)
    prior = randn((N,), 3)
    c = _colsum_chain(M, N, ld)
    tag = f"colsum[{M}x{N}, ld={ld}]"
    out = full((N + 8,), NAN)          # a guard behind the N results
    ok(lib.ia_colsum(P(xd), ld, M, N, P(out), 0, P(ws), ws_bytes, st()), "ia_colsum")
    sum_close(tag + " accumulate=0", out[:N], x64.sum(0), x64.abs().sum(0), c)
    assert torch.isnan(out[N:]).all(), "written past N"
    out = torch.cat((prior, torch.full((8,), NAN))).to(gpu)
    ok(lib.ia_colsum(P(xd), ld, M, N, P(out), 1, P(ws), ws_bytes, st()), "ia_colsum")
    sum_close(tag + " accumulate=1", out[:N], x64.sum(0) + prior.to(F64), x64.abs().sum(0) + prior.to(F64).abs(), c)
    assert torch.isnan(out[N:]).all(), "written past N"


# =============================================================================================================== BatchNorm / GroupNorm
def _partial_chain(per, C):
    """bn_partial_kernel: a row lane adds every nlane-th row of its slice of `per` rows, lane 0 then adds the other nlane - 1 lanes"""
    ncol = min(C // 8, 256)
    nlane = 256 // ncol
    return cdiv(per, nlane) + nlane - 1


def _bn_chain(rps, C):
    """+ fold_partials: 16 lanes take every 16th of the nsplit partials, lane 0 adds the 16 lane sums"""
    ns = min(512, max(1, rps // 64))
    return _partial_chain(cdiv(rps, ns), C) + cdiv(ns, 16) + 16


def _gn_chain(hw, C, images, groups):
    """+ gn_fold_kernel: the nsplit partials one after another; + the C / groups channels of a group one after another"""
    ns = min(max(8, 4096 // images), max(1, hw // 64))
    return _partial_chain(cdiv(hw, ns), C) + ns + C // groups


def _stat_bounds(c_s, A1, Ex2, mu64, var64, eps):
    """(e_mu, e_var, e_rstd) of the one-pass statistics, see the module docstring; rstd = rsqrt(var + eps) is monotone, so its bound is
    the larger of the two one-sided changes of rsqrt under e_var (+ the rounding of the sum), plus rsqrt's own error and the rounding
    (3 * 2^-24 relative)"""
    e_mu = (c_s + 1) * U24 * A1
    e_var = (3 * c_s + 5) * U24 * (Ex2 + mu64 ** 2)
    v = var64 + eps
    e = e_var + U24 * v
    rstd64 = v.rsqrt()
    lo = (torch.clamp(var64 - e, min=0.0) + eps).rsqrt() - rstd64
    hi = rstd64 - (v + e).rsqrt()
    return e_mu, e_var, torch.maximum(lo, hi) + 3 * U24 * rstd64


def _check_mask(tag, y, pre64, a_pre):
    """the kernel's own ReLU mask (y > 0) against the fp64 one: different only where the fp64 pre-activation is within its fp32 bound of
    zero, and in fewer than 0.1 % of the elements"""
    mask = y.cpu() > 0
    diff = mask != (pre64 > 0)
    share = float(diff.float().mean())
    print(f"[norm] {tag}: mask differs from fp64 in {int(diff.sum())} of {diff.numel()} elements")
    assert share < 1e-3, (tag, share)
    assert (pre64[diff].abs() <= a_pre.expand_as(pre64)[diff]).all(), (tag, "a mask bit differs where the pre-activation is not near zero")
    return mask


def _seg(t, segments):
    """[segments, C] statistics -> broadcastable against [segments, n, C]"""
    return t.reshape(segments, 1, -1)


def _bn_fwd(lib, xd, gd, bd, rm, rv, rows, C, segments, eps, mom, training, relu, ws):
    y = full((rows, C), 9.0, BF16)
    mean, rstd = full((segments, C), NAN), full((segments, C), NAN)
    ok(lib.ia_bn_act_fwd(P(xd), P(gd), P(bd), P(rm), P(rv), P(y), P(mean), P(rstd), rows, C, segments, eps, mom, training, relu, P(ws), ws.numel(),
                         st()), "ia_bn_act_fwd")
    return y, mean, rstd


def _bwd_bounds(dy, x, gamma, mean, rstd, mask, segments, c_s, training, extra):
    """fp32 bound of dx = k1 (g - k2 - xhat k3) (+ extra), k1 = gamma rstd, k2 = sum g / n, k3 = sum g xhat / n: the two sums carry
    their chains (c_s, + 3 roundings inside a term g xhat, + 2 for the division by n), xhat 2 roundings, the expression 6 more on the
    magnitudes it combines.  Eval: k1 g, 4 roundings.  Also the S of dgamma and dbeta."""
    rows, C = x.shape
    n = rows // segments
    g = (dy.to(F64) * (mask.to(F64) if mask is not None else 1.0)).reshape(segments, n, C)
    xh = (x.to(F64).reshape(segments, n, C) - _seg(mean.to(F64), segments)) * _seg(rstd.to(F64), segments)
    k1 = (gamma.to(F64) * _seg(rstd.to(F64), segments)).abs()
    if training:
        mG, mGX = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
        a = k1 * U24 * ((c_s + 11) * (mG + xh.abs() * mGX) + 6 * g.abs())
    else:
        a = k1 * U24 * 4 * g.abs()
    a = a.reshape(rows, C)
    if extra is not None:
        a = a + U24 * extra.to(F64).abs()
    return a, (g * xh).abs().sum((0, 1)), g.abs().sum((0, 1))


BN_SHAPES = [(1, 8, 1), (2, 8, 2), (63, 8, 1), (130, 192, 1), (231, 16, 3), (200, 2056, 1), (33000, 8, 1)]


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("kind", ["wide", "offset"])
@pytest.mark.parametrize("rows,C,segments", BN_SHAPES)
def test_bn_act_training_fwd_bwd(gpu, lib, rows, C, segments, kind, relu):
    """ia_bn_act_fwd / ia_bn_act_bwd in training mode: one row per segment (variance 0), C = 8 (one column thread, 256 row lanes),
    24 column threads of 10 lanes (192), three segments, the second column pass (C = 2056 > 2048), the 512-slice cap (33000 rows).
    y, mean, rstd, running_mean, running_var with the one-pass bounds of the module docstring; NULL running pointers change no bit.
    Backward with the forward's own mask: dx with and without extra, dgamma / dbeta onto a non-zero prior, NULL dgamma / dbeta, and two
    identical calls give identical bits."""
    eps, mom = f32(1e-5), f32(0.1)
    n = rows // segments
    x, gamma, beta = N.norm_inputs(rows, C, 11 + rows + C, kind)
    rm0, rv0 = randn((C,), 1, 0.1), torch.rand(C, generator=gen(2)) + 0.5
    xd, gd, bd = dv(x), dv(gamma), dv(beta)
    ws = torch.empty(lib.ia_bn_act_workspace_bytes(rows, C, segments), device=gpu, dtype=torch.uint8)
    rm, rv = dv(rm0), dv(rv0)
    y, mean, rstd = _bn_fwd(lib, xd, gd, bd, rm, rv, rows, C, segments, eps, mom, 1, relu, ws)
    tag = f"bn[{rows}x{C}/{segments} {kind} relu={relu}]"

    y64, pre64, mean64, rstd64, rm64, rv64 = N.bn_act_fwd(x, gamma, beta, rm0, rv0, segments, eps, mom, 1, relu)
    xs = x.to(F64).reshape(segments, n, C)
    c_s = _bn_chain(n, C)
    var64 = ((xs - mean64[:, None]) ** 2).mean(1)
    e_mu, e_var, e_rstd = _stat_bounds(c_s, xs.abs().mean(1), (xs ** 2).mean(1), mean64, var64, eps)
    r = _ratio(tag + " mean", (mean.cpu().to(F64) - mean64).abs(), e_mu)
    assert r <= 1.0, (tag, "mean", r)
    r = _ratio(tag + " rstd", (rstd.cpu().to(F64) - rstd64).abs(), e_rstd)
    assert r <= 1.0, (tag, "rstd", r)
    # running statistics, segment after segment: r = (1 - m) r + m t costs 3 roundings on |r| + m |t| and passes the error of t on, times
    # m; t = var * n / (n - 1) has 3 more of its own (the quotient, two products)
    f = n / (n - 1) if n > 1 else 1.0
    b_rm, b_rv = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
    a_rm, a_rv = rm0.to(F64).abs(), rv0.to(F64).abs()
    for s in range(segments):
        b_rm = b_rm + mom * e_mu[s] + 3 * U24 * (a_rm + mom * mean64[s].abs())
        b_rv = b_rv + mom * f * (e_var[s] + 3 * U24 * var64[s]) + 3 * U24 * (a_rv + mom * f * var64[s])
        a_rm, a_rv = a_rm + mom * mean64[s].abs(), a_rv + mom * f * var64[s]
    r = _ratio(tag + " running_mean", (rm.cpu().to(F64) - rm64).abs(), b_rm)
    assert r <= 1.0, (tag, "running_mean", r)
    r = _ratio(tag + " running_var", (rv.cpu().to(F64) - rv64).abs(), b_rv)
    assert r <= 1.0, (tag, "running_var", r)
    # pre = (x - mu) * rstd * gamma + beta: the two statistics' errors and 4 roundings on the magnitudes; relu is a contraction
    dev = (xs - mean64[:, None]).abs()
    ga = gamma.to(F64).abs()
    a_pre = (ga * (e_mu[:, None] * rstd64[:, None] + dev * e_rstd[:, None]) + 4 * U24 * (dev * rstd64[:, None] * ga + beta.to(F64).abs())).reshape(rows, C)
    bf16_close(tag + " y", y, y64, a_pre)
    y2, mean2, rstd2 = _bn_fwd(lib, xd, gd, bd, None, None, rows, C, segments, eps, mom, 1, relu, ws)
    bits(tag + " y without running statistics", y2, y), bits(tag + " mean (same)", mean2, mean), bits(tag + " rstd (same)", rstd2, rstd)

    mask = _check_mask(tag, y, pre64, a_pre) if relu else None
    dy, extra = randn((rows, C), 5, 1.0, BF16), randn((rows, C), 6, 1.0, BF16)
    dyd, exd = dv(dy), dv(extra)
    prior = 0.5

    def bwd(ex, params):
        dx = full((rows, C), 9.0, BF16)
        dg, db = (full((C,), prior), full((C,), prior)) if params else (None, None)
        ok(lib.ia_bn_act_bwd(P(dyd), P(xd), P(gd), P(bd), P(mean), P(rstd), P(ex), P(dx), P(dg), P(db), rows, C, segments, 1, relu, P(ws), ws.numel(),
                             st()), "ia_bn_act_bwd")
        return dx, dg, db

    # the backward reads the kernel's own fp32 mean / rstd: the reference gets the same numbers
    for ex_h, ex_d, params, name in ((extra, exd, True, "with extra"), (None, None, False, "no extra, NULL dgamma / dbeta")):
        dx, dg, db = bwd(ex_d, params)
        dx64, dgamma64, dbeta64 = N.bn_act_bwd(dy, x, gamma, mean.cpu(), rstd.cpu(), mask, segments, 1, ex_h)
        a_dx, S_dg, S_db = _bwd_bounds(dy, x, gamma, mean.cpu(), rstd.cpu(), mask, segments, c_s, 1, ex_h)
        bf16_close(f"{tag} dx ({name})", dx, dx64, a_dx)
        if params:
            # + the segments one after another, + the accumulation
            sum_close(tag + " dgamma", dg, dgamma64 + prior, S_dg + prior, c_s + 3 + segments + 1)
            sum_close(tag + " dbeta", db, dbeta64 + prior, S_db + prior, c_s + segments + 1)
            again = bwd(ex_d, True)
            for a, b, nm in zip(again, (dx, dg, db), ("dx", "dgamma", "dbeta")):
                bits(f"{tag} {nm} of a second identical call", a, b)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows,C,segments", [(2, 8, 2), (231, 16, 3), (200, 2056, 1)])
def test_bn_act_eval_fwd_bwd(gpu, lib, rows, C, segments, relu):
    """training = 0: mean = running_mean and rstd = rsqrt(running_var + eps) for every segment, the running statistics untouched;
    the backward treats them as constants: dx = gamma rstd g, while dgamma / dbeta are the same sums as in training."""
    eps = f32(1e-5)
    x, gamma, beta = N.norm_inputs(rows, C, 40 + rows + C, "wide")
    rm0, rv0 = randn((C,), 1, 0.5) + 0.4, torch.rand(C, generator=gen(2)) * 2 + 1.0
    xd, gd, bd, rm, rv = dv(x), dv(gamma), dv(beta), dv(rm0), dv(rv0)
    ws = torch.empty(lib.ia_bn_act_workspace_bytes(rows, C, segments), device=gpu, dtype=torch.uint8)
    y, mean, rstd = _bn_fwd(lib, xd, gd, bd, rm, rv, rows, C, segments, eps, 0.1, 0, relu, ws)
    tag = f"bn eval[{rows}x{C}/{segments} relu={relu}]"
    bits(tag + " running_mean untouched", rm, rm0), bits(tag + " running_var untouched", rv, rv0)
    y64, pre64, mean64, rstd64, _, _ = N.bn_act_fwd(x, gamma, beta, rm0, rv0, segments, eps, 0.1, 0, relu)
    bits(tag + " mean", mean, rm0[None].expand(segments, C).contiguous())
    # rsqrt(rv + eps): the addition, rsqrt's own error, the rounding
    e_rstd = 4 * U24 * rstd64
    r = _ratio(tag + " rstd", (rstd.cpu().to(F64) - rstd64).abs(), e_rstd)
    assert r <= 1.0, (tag, "rstd", r)
    n = rows // segments
    dev = (x.to(F64).reshape(segments, n, C) - mean64[:, None]).abs()
    ga = gamma.to(F64).abs()
    a_pre = (ga * dev * e_rstd[:, None] + 4 * U24 * (dev * rstd64[:, None] * ga + beta.to(F64).abs())).reshape(rows, C)
    bf16_close(tag + " y", y, y64, a_pre)
    mask = _check_mask(tag, y, pre64, a_pre) if relu else None
    dy, extra = randn((rows, C), 5, 1.0, BF16), randn((rows, C), 6, 1.0, BF16)
    dx, dg, db = full((rows, C), 9.0, BF16), full((C,), 0.5), full((C,), 0.5)
    dyd, exd = dv(dy), dv(extra)
    ok(lib.ia_bn_act_bwd(P(dyd), P(xd), P(gd), P(bd), P(mean), P(rstd), P(exd), P(dx), P(dg), P(db), rows, C, segments, 0, relu, P(ws),
                         ws.numel(), st()), "ia_bn_act_bwd")
    dx64, dgamma64, dbeta64 = N.bn_act_bwd(dy, x, gamma, mean.cpu(), rstd.cpu(), mask, segments, 0, extra)
    c_s = _bn_chain(n, C)
    a_dx, S_dg, S_db = _bwd_bounds(dy, x, gamma, mean.cpu(), rstd.cpu(), mask, segments, c_s, 0, extra)
    bf16_close(tag + " dx", dx, dx64, a_dx)
    sum_close(tag + " dgamma", dg, dgamma64 + 0.5, S_dg + 0.5, c_s + 3 + segments + 1)
    sum_close(tag + " dbeta", db, dbeta64 + 0.5, S_db + 0.5, c_s + segments + 1)


GN_SHAPES = [(3, 49, 192, 32), (4, 100, 32, 32), (2, 333, 64, 8), (1, 9, 6144, 32), (5, 1, 8, 2), (512, 576, 8, 1)]


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("kind", ["wide", "offset"])
@pytest.mark.parametrize("images,hw,C,groups", GN_SHAPES)
def test_gn_act_fwd_bwd(gpu, lib, images, hw, C, groups, kind, relu):
    """ia_gn_act_fwd / ia_gn_act_bwd: 6-channel groups (192 / 32), one channel per group (32 / 32), 333 pixels in 5 slices, 24 column
    passes (C = 6144), one pixel per image, and 512 images of 576 pixels, where the cap of 8 slices per image binds (576 / 64 = 9).
    Outputs and bounds as for BatchNorm with the group as the population; mean / rstd are one value per group, bit for bit."""
    eps = f32(1e-5)
    rows, cg = images * hw, C // groups
    x, gamma, beta = N.norm_inputs(rows, C, 11 + rows + C, kind)
    xd, gd, bd = dv(x), dv(gamma), dv(beta)
    ws = torch.empty(lib.ia_gn_act_workspace_bytes(rows, C, images), device=gpu, dtype=torch.uint8)
    y, mean, rstd = full((rows, C), 9.0, BF16), full((images, C), NAN), full((images, C), NAN)
    ok(lib.ia_gn_act_fwd(P(xd), P(gd), P(bd), P(y), P(mean), P(rstd), rows, C, images, groups, eps, relu, P(ws), ws.numel(), st()), "ia_gn_act_fwd")
    tag = f"gn[{images}x{hw}x{C}/{groups} {kind} relu={relu}]"
    if (images, hw) == (512, 576):
        assert hw // 64 > max(8, 4096 // images)          # the cap binds
    for t, nm in ((mean, "mean"), (rstd, "rstd")):
        tg = t.cpu().reshape(images, groups, cg)
        bits(f"{tag} {nm} is one value per group", tg, tg[:, :, :1].expand(images, groups, cg).contiguous())

    y64, pre64, mean64, rstd64 = N.gn_act_fwd(x, gamma, beta, images, groups, eps, relu)
    xg = x.to(F64).reshape(images, hw, groups, cg)
    rep = lambda t: t.reshape(images, groups, 1).expand(images, groups, cg).reshape(images, C)
    c_s = _gn_chain(hw, C, images, groups)
    var64 = rep(((xg - xg.mean((1, 3), keepdim=True)) ** 2).mean((1, 3)))
    e_mu, e_var, e_rstd = _stat_bounds(c_s, rep(xg.abs().mean((1, 3))), rep((xg ** 2).mean((1, 3))), mean64, var64, eps)
    r = _ratio(tag + " mean", (mean.cpu().to(F64) - mean64).abs(), e_mu)
    assert r <= 1.0, (tag, "mean", r)
    r = _ratio(tag + " rstd", (rstd.cpu().to(F64) - rstd64).abs(), e_rstd)
    assert r <= 1.0, (tag, "rstd", r)
    dev = (x.to(F64).reshape(images, hw, C) - mean64[:, None]).abs()
    ga = gamma.to(F64).abs()
    a_pre = (ga * (e_mu[:, None] * rstd64[:, None] + dev * e_rstd[:, None]) + 4 * U24 * (dev * rstd64[:, None] * ga + beta.to(F64).abs())).reshape(rows, C)
    bf16_close(tag + " y", y, y64, a_pre)

    mask = _check_mask(tag, y, pre64, a_pre) if relu else None
    dy, extra = randn((rows, C), 5, 1.0, BF16), randn((rows, C), 6, 1.0, BF16)
    dyd, exd = dv(dy), dv(extra)
    prior = 0.5

    def bwd(ex, params):
        dx = full((rows, C), 9.0, BF16)
        dg, db = (full((C,), prior), full((C,), prior)) if params else (None, None)
        ok(lib.ia_gn_act_bwd(P(dyd), P(xd), P(gd), P(bd), P(mean), P(rstd), P(ex), P(dx), P(dg), P(db), rows, C, images, groups, relu, P(ws),
                             ws.numel(), st()), "ia_gn_act_bwd")
        return dx, dg, db

    mk, rk = mean.cpu().to(F64), rstd.cpu().to(F64)
    g = (dy.to(F64) * (mask.to(F64) if mask is not None else 1.0)).reshape(images, hw, C)
    xh = (x.to(F64).reshape(images, hw, C) - mk[:, None]) * rk[:, None]
    gg = (g * gamma.to(F64)).abs()
    grp = lambda t: t.reshape(images, hw, groups, cg).mean((1, 3), keepdim=True).expand(images, hw, groups, cg).reshape(images, hw, C)
    # dx = rstd (gamma g - M1 - xhat M2): M1, M2 = a channel's sum (the partial chain, the slices, 3 roundings inside a term), times gamma,
    # the group's channels one after another, two roundings for 1 / n; xhat 2 roundings; the expression 6 more on what it combines
    c_g = c_s + 3 + 1 + 2
    a_dx0 = (rk[:, None] * U24 * ((c_g + 6) * (grp(gg) + xh.abs() * grp(gg * xh.abs())) + 6 * gg)).reshape(rows, C)
    c_p = c_s - cg                                       # a channel's own sum
    for ex_h, ex_d, params, name in ((extra, exd, True, "with extra"), (None, None, False, "no extra, NULL dgamma / dbeta")):
        dx, dg, db = bwd(ex_d, params)
        dx64, dgamma64, dbeta64 = N.gn_act_bwd(dy, x, gamma, mean.cpu(), rstd.cpu(), mask, images, groups, ex_h)
        bf16_close(f"{tag} dx ({name})", dx, dx64, a_dx0 + (U24 * ex_h.to(F64).abs() if ex_h is not None else 0.0))
        if params:
            # + the images one after another, + the accumulation
            sum_close(tag + " dgamma", dg, dgamma64 + prior, (g * xh).abs().sum((0, 1)) + prior, c_p + 3 + images + 1)
            sum_close(tag + " dbeta", db, dbeta64 + prior, g.abs().sum((0, 1)) + prior, c_p + images + 1)
            again = bwd(ex_d, True)
            for a, b, nm in zip(again, (dx, dg, db), ("dx", "dgamma", "dbeta")):
                bits(f"{tag} {nm} of a second identical call", a, b)


# =============================================================================================================== MaxPool 3x3 / 2
POOL_SHAPES = [(1, 1, 1, 8), (2, 1, 5, 8), (1, 2, 2, 24), (2, 7, 9, 16), (1, 8, 8, 64)]


def _pool_input(shape, kind, pad_zero):
    x = randn(shape, 7 + shape[1] * 10 + shape[2])
    if kind == "coarse":         # few distinct values: ties in most windows; shifted down under pad_zero so that the ring's zeros win somewhere
        x = (x * 1.5).round() - (1.0 if pad_zero else 0.0)
    elif kind == "nan":
        x[0, shape[1] // 2, shape[2] // 2, 3] = NAN
    return x.to(BF16)


@pytest.mark.parametrize("kind", ["coarse", "fine", "nan"])
@pytest.mark.parametrize("pad_zero", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_values_argmax_and_gradient(gpu, lib, shape, pad_zero, kind):
    """ia_maxpool3s2_fwd(_ex) / _bwd: y bit-exact, arg = the reference's first maximum in scan order (a >= instead of > would take the
    last), the pad_zero ring as zeros; one NaN input makes every window holding it NaN, as in torch.  dx: at most four bf16 gradients
    added in fp32 (3 roundings) and rounded once; a ring winner routes nothing."""
    B, H, W, C = shape
    Ho, Wo = N.pool_out(H), N.pool_out(W)
    x = _pool_input(shape, kind, pad_zero)
    xd = x.to(gpu)
    y, arg = full((B, Ho, Wo, C), 9.0, BF16), torch.full((B, Ho, Wo, C), 77, device=gpu, dtype=torch.uint8)
    if pad_zero:
        ok(lib.ia_maxpool3s2_fwd_ex(P(xd), P(y), P(arg), B, H, W, C, 1, st()), "ia_maxpool3s2_fwd_ex")
    else:
        ok(lib.ia_maxpool3s2_fwd(P(xd), P(y), P(arg), B, H, W, C, st()), "ia_maxpool3s2_fwd")
    y64, arg64 = N.maxpool3s2(x, bool(pad_zero))
    tag = f"maxpool[{shape} pad_zero={pad_zero} {kind}]"
    nan = torch.isnan(y64)
    assert torch.equal(torch.isnan(y.cpu()), nan), (tag, "NaN windows")
    assert bool(nan.any()) == (kind == "nan")
    bits(tag + " y", y.cpu()[~nan], y64[~nan])
    assert torch.equal(arg.cpu(), arg64), (tag, "arg", int((arg.cpu() != arg64).sum()))
    dy = randn((B, Ho, Wo, C), 9, 1.0, BF16)
    dx, dyd = full(shape, 9.0, BF16), dv(dy)
    ok(lib.ia_maxpool3s2_bwd(P(dyd), P(arg), P(dx), B, H, W, C, st()), "ia_maxpool3s2_bwd")
    bf16_close(tag + " dx", dx, N.maxpool3s2_bwd(dy, arg64, H, W), 3 * U24 * N.maxpool3s2_bwd(dy.to(F64).abs(), arg64, H, W))
    if kind == "coarse" and pad_zero and H * W > 4:
        ky, kx = arg64 // 3, arg64 % 3
        iy = 2 * torch.arange(Ho)[None, :, None, None] + ky - 1
        ix = 2 * torch.arange(Wo)[None, None, :, None] + kx - 1
        assert ((iy < 0) | (iy >= H) | (ix < 0) | (ix >= W)).any(), "the ring wins nowhere in this set"


# =============================================================================================================== strided rows
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 7, 10, 8), (1, 1, 1, 16)])
def test_rows_subsample_fwd_bwd(gpu, lib, shape, stride):
    """ia_rows_subsample_fwd is a bit-exact gather; _bwd with base NULL is a bit-exact scatter onto zeros, with a base it is
    bf16(base + dy) on the stride grid (one fp32 addition) and base itself off it, and base may be dx."""
    B, H, W, C = shape
    Ho, Wo = N.pool_out(H, stride), N.pool_out(W, stride)
    x = randn(shape, 3, 1.0, BF16)
    y, xd = full((B, Ho, Wo, C), 9.0, BF16), dv(x)
    ok(lib.ia_rows_subsample_fwd(P(xd), P(y), B, H, W, C, stride, st()), "ia_rows_subsample_fwd")
    tag = f"subsample[{shape} s={stride}]"
    bits(tag + " y", y, N.rows_subsample(x, stride).contiguous())
    dy, base = randn((B, Ho, Wo, C), 4, 1.0, BF16), randn(shape, 5, 1.0, BF16)
    dyd = dv(dy)
    dx = full(shape, 9.0, BF16)
    ok(lib.ia_rows_subsample_bwd(P(dyd), None, P(dx), B, H, W, C, stride, st()), "ia_rows_subsample_bwd")
    bits(tag + " dx, base NULL", dx, N.rows_subsample_bwd(dy, None, H, W, stride))
    dx, based = full(shape, 9.0, BF16), dv(base)
    ok(lib.ia_rows_subsample_bwd(P(dyd), P(based), P(dx), B, H, W, C, stride, st()), "ia_rows_subsample_bwd")
    on = N.rows_subsample_bwd(dy.to(F64).abs(), None, H, W, stride)
    bf16_close(tag + " dx, base given", dx, N.rows_subsample_bwd(dy, base, H, W, stride), U24 * (on + base.to(F64).abs()) * (on != 0))
    grid = torch.zeros(shape, dtype=torch.bool)
    grid[:, ::stride, ::stride] = True
    bits(tag + " dx off the grid is base", dx.cpu()[~grid], base[~grid])
    alias = base.to(gpu)
    ok(lib.ia_rows_subsample_bwd(P(dyd), P(alias), P(alias), B, H, W, C, stride, st()), "ia_rows_subsample_bwd")
    bits(tag + " dx aliasing base", alias, dx)


# =============================================================================================================== patch gather
@pytest.mark.parametrize("k,C,stride,pad,Kp", [(3, 4, 1, 1, 40), (1, 8, 2, 0, 8), (7, 3, 1, 3, 152), (7, 3, 2, 3, 160)])
def test_patches_nchw_generic_forms(gpu, lib, k, C, stride, pad, Kp):
    """ia_patches_nchw off the LDS stem kernel: the run-time form (k = 3, k = 1), the <7, 3> form at stride 1, and the 7 x 7 / 2 stem with
    Kp = 160, which the LDS kernel (Kp == 152 only) does not take.  Bit-exact fp32 -> bf16 gather, exact zeros outside the image and in
    the padding columns."""
    B, H, W = 2, 13, 10
    img = randn((B, C, H, W), 20 + k)
    want = N.patches_nchw(img, k, stride, pad, Kp)
    cols, imgd = full(tuple(want.shape), 9.0, BF16), dv(img)
    ok(lib.ia_patches_nchw(P(imgd), P(cols), B, C, H, W, k, stride, pad, Kp, st()), "ia_patches_nchw")
    tag = f"patches[k={k} C={C} s={stride} pad={pad} Kp={Kp}]"
    bits(tag, cols, want)
    assert (cols.cpu()[:, k * k * C:].view(torch.int16) == 0).all(), (tag, "padding columns")
