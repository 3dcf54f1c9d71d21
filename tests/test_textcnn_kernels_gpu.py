"""The TextCNN tower kernels (csrc/textcnn.hip) through the C ABI against the fp64 restatement of tests/textcnn_reference.py.  The bars
are derived in the way of tests/test_glue_kernels_gpu.py, not measured:

  * forward: |feat - want| <= c 2^-24 S on the same fp32 P, S = the largest sum of |terms| over the windows of the feature,
    c = K_s + 1 (K_s - 1 tap additions and the bias, one after the other, then the dropout scale); argmax equals the reference
    wherever the fp64 gap from the best window to the runner-up (and to 0, the dead / alive decision) exceeds that bound -- at most
    2 % of the entries may be excused (tests/test_textcnn_reference_host.py holds the seeded inputs alone to that cap);
  * dW / db: c = B + 1 (one fma per sample in index order; the rounding of g times the dropout scale);
  * dx: one bf16 ulp plus (NF + 1) 2^-24 S for the fp32 sum in front of the rounding (at most NF contributions land on a row); a row
    no winning window covers has S = 0 and must be exactly zero.
The backward tests take the argmax of the reference, so routing is not in question there.  Every comparison prints its largest
error as a fraction of the bound (`-s`).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as Fnn

import glue_reference as R
import textcnn_reference as T

pytestmark = pytest.mark.gpu

F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    """seeded inputs and the fp64 reference of every shape, computed once and shared (never modified)"""
    cache = {}

    def get(shape):
        if shape not in cache:
            c = T.seeded_case(shape)
            c.feat, c.arg, c.smax, c.gap = T.pool_fwd(c.P, c.bs, c.sizes, c.B, c.L)
            cache[shape] = c
        return cache[shape]
    return get


def _sync(rc, what):
    from item_alignment_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def _pa(ts):
    return (C.c_void_p * len(ts))(*(t.data_ptr() for t in ts))


def _ia(v):
    return (C.c_int * len(v))(*v)


def _cu(ts):
    return [t.cuda().contiguous() for t in ts]


def _ratio(name, err, bound):
    assert torch.isfinite(err).all(), (name, "non-finite output")
    exact = bound == 0
    assert (err[exact] == 0).all(), (name, "an element whose bound is zero is not exact")
    r = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"[textcnn] {name}: max error / bound = {r:.3f}")
    return r


def sum_close(name, got, want, S, c):
    got = got.detach().cpu().to(F64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    r = _ratio(name, (got - want).abs(), c * R.U24 * S)
    assert r <= 1.0, (name, r, "c =", c)


def bf16_close(name, got, want, a):
    got = got.detach().cpu().to(F64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    r = _ratio(name, (got - want).abs(), R.BF16_ULP * want.abs() + a)
    assert r <= 1.0, (name, r)


def bits_equal(a, b):
    iv = {BF16: torch.int16, F32: torch.int32, I32: torch.int32}[a.dtype]
    return bool((a.contiguous().view(iv) == b.contiguous().view(iv)).all())


def run_fwd(lib, P, bs, sizes, B, L, drop=(0.0, 0.0, 0, 0, 0)):
    Pd, bd = P.cuda().contiguous(), _cu(bs)
    F = bs[0].shape[0]
    feat = torch.full((B, F * len(sizes)), float("nan"), device="cuda", dtype=F32)
    arg = torch.full((B, F * len(sizes)), -7, device="cuda", dtype=I32)
    _sync(lib.ia_textcnn_pool_fwd(Pd.data_ptr(), Pd.shape[1], _pa(bd), _ia(sizes), len(sizes), F, B, L, *drop, feat.data_ptr(),
                                  arg.data_ptr(), None), "ia_textcnn_pool_fwd")
    return feat.cpu(), arg.cpu()


def run_bwd_w(lib, g, arg, x0, x1, sizes, F, L, drop=(0.0, 0.0, 0, 0, 0)):
    gd, ad, x0d, x1d = _cu([g, arg, x0, x1])
    B, H = g.shape[0], x0.shape[1]
    dW = [torch.full((F, 2, K, H), float("nan"), device="cuda", dtype=F32) for K in sizes]
    db = [torch.full((F,), float("nan"), device="cuda", dtype=F32) for _ in sizes]
    _sync(lib.ia_textcnn_pool_bwd_w(gd.data_ptr(), ad.data_ptr(), x0d.data_ptr(), x1d.data_ptr(), _ia(sizes), len(sizes), F, B, L, H, *drop,
                                    _pa(dW), _pa(db), None), "ia_textcnn_pool_bwd_w")
    return [t.cpu() for t in dW], [t.cpu() for t in db]


def run_bwd_x(lib, g, arg, Ws, sizes, L, drop=(0.0, 0.0, 0, 0, 0)):
    gd, ad = _cu([g, arg])
    Wd = _cu(Ws)
    B, F, H = g.shape[0], Ws[0].shape[0], Ws[0].shape[3]
    dx = torch.full((B * L, H), float("nan"), device="cuda", dtype=BF16)
    _sync(lib.ia_textcnn_pool_bwd_x(gd.data_ptr(), ad.data_ptr(), _pa(Wd), _ia(sizes), len(sizes), F, B, L, H, *drop, dx.data_ptr(), None),
          "ia_textcnn_pool_bwd_x")
    return dx.cpu()


# ============================================================================================================ forward
@pytest.mark.parametrize("shape", T.KERNEL_SHAPES, ids=T.shape_id)
def test_pool_forward_against_fp64(lib, cases, shape):
    c = cases(shape)
    bound = T.fwd_bound(c.sizes, c.F, c.smax)
    excused = c.gap <= bound
    assert float(excused.to(F64).mean()) <= 0.02, ("the seeded inputs put too many routing decisions inside the bound", int(excused.sum()))
    feat, arg = run_fwd(lib, c.P, c.bs, c.sizes, c.B, c.L)
    r = _ratio("pool_fwd feat", (feat.to(F64) - c.feat).abs(), bound.expand_as(c.feat))
    assert r <= 1.0, r
    wrong = (arg != c.arg) & ~excused
    assert not wrong.any(), (int(wrong.sum()), "argmax differs where the fp64 gap exceeds the bound")
    print(f"[textcnn] pool_fwd argmax: {int((arg != c.arg).sum())} of {arg.numel()} differ, all inside the bound ({int(excused.sum())} excusable)")
    assert ((arg == -1) == (feat == 0)).all() and (arg >= -1).all() and (arg <= c.L - 1).all()


# ============================================================================================================ backward
@pytest.mark.parametrize("shape", T.KERNEL_SHAPES, ids=T.shape_id)
def test_weight_gradient_against_fp64(lib, cases, shape):
    c = cases(shape)
    dW, db = run_bwd_w(lib, c.g, c.arg, c.x0, c.x1, c.sizes, c.F, c.L)
    wW, wb, mW, mb = T.pool_bwd_w(c.g, c.arg, c.x0, c.x1, c.sizes, c.L)
    for s in range(len(c.sizes)):
        sum_close(f"dW[{s}]", dW[s], wW[s], mW[s], c.B + 1)
        sum_close(f"db[{s}]", db[s], wb[s], mb[s], c.B + 1)


@pytest.mark.parametrize("shape", T.KERNEL_SHAPES, ids=T.shape_id)
def test_input_gradient_against_fp64(lib, cases, shape):
    c = cases(shape)
    dx = run_bwd_x(lib, c.g, c.arg, c.Ws, c.sizes, c.L)
    want, mag = T.pool_bwd_x(c.g, c.arg, c.Ws, c.sizes, c.L)
    bf16_close("dx", dx, want, (c.NF + 1) * R.U24 * mag)
    # rows outside every winning window are exactly zero
    covered = torch.zeros(c.B * c.L, dtype=torch.bool)
    F = c.F
    for s, K in enumerate(c.sizes):
        a = c.arg[:, s * F:(s + 1) * F].long()
        for k in range(K):
            rows = (torch.arange(c.B)[:, None] * c.L + a + k)[a >= 0]
            covered[rows] = True
    assert (dx[~covered] == 0).all()
    if c.NF * max(c.sizes) < c.L:                 # fewer window rows than rows: some are covered by nothing
        assert (~covered).any()


def test_backward_is_bit_identical_from_run_to_run(lib, cases):
    c = cases(T.KERNEL_SHAPES[3])
    a = run_bwd_w(lib, c.g, c.arg, c.x0, c.x1, c.sizes, c.F, c.L)
    b = run_bwd_w(lib, c.g, c.arg, c.x0, c.x1, c.sizes, c.F, c.L)
    for s in range(len(c.sizes)):
        assert bits_equal(a[0][s], b[0][s]) and bits_equal(a[1][s], b[1][s])
    assert bits_equal(run_bwd_x(lib, c.g, c.arg, c.Ws, c.sizes, c.L), run_bwd_x(lib, c.g, c.arg, c.Ws, c.sizes, c.L))
    f1, f2 = run_fwd(lib, c.P, c.bs, c.sizes, c.B, c.L), run_fwd(lib, c.P, c.bs, c.sizes, c.B, c.L)
    assert bits_equal(f1[0], f2[0]) and bits_equal(f1[1], f2[1])


# ============================================================================================================ edges
def test_dead_filter_gives_zero_feature_and_zero_gradients(lib, cases):
    """a filter whose bias is -1e4: feature 0, argmax -1, and nothing flows back through it"""
    c = cases(T.KERNEL_SHAPES[2])
    s, f = 2, 1
    bs = [b.clone() for b in c.bs]
    bs[s][f] = -1e4
    feat, arg = run_fwd(lib, c.P, bs, c.sizes, c.B, c.L)
    j = s * c.F + f
    assert (feat[:, j] == 0).all() and (arg[:, j] == -1).all()
    dW, db = run_bwd_w(lib, c.g, arg, c.x0, c.x1, c.sizes, c.F, c.L)
    assert (dW[s][f] == 0).all() and db[s][f] == 0
    g_only = torch.zeros_like(c.g)
    g_only[:, j] = c.g[:, j]
    assert (run_bwd_x(lib, g_only, arg, c.Ws, c.sizes, c.L) == 0).all()


def test_ties_go_to_the_lowest_t_like_max_pool1d(lib, cases):
    """duplicated input rows: every window of a feature ties bit for bit; the kernel picks what F.max_pool1d picks on the CPU"""
    c = cases(T.KERNEL_SHAPES[2])
    P = c.P.reshape(c.B, c.L, -1)[:, :1].expand(c.B, c.L, -1).reshape(c.B * c.L, -1).contiguous()
    bs = [b.abs() + 10.0 for b in c.bs]
    _feat, arg = run_fwd(lib, P, bs, c.sizes, c.B, c.L)
    off, _nt, _ntp = T.offsets(c.sizes, c.F)
    P3 = P.reshape(c.B, c.L, -1)
    for s, K in enumerate(c.sizes):
        Tn = c.L - K + 1
        pre = sum(P3[:, k:k + Tn, off[s] + k * c.F: off[s] + (k + 1) * c.F] for k in range(K)) + bs[s]          # fp32 [B, T, F]
        _v, idx = Fnn.max_pool1d(Fnn.relu(pre.transpose(1, 2)), Tn, return_indices=True)
        assert (arg[:, s * c.F:(s + 1) * c.F].long() == idx.squeeze(2)).all()
        assert (idx == 0).all()


def test_refusals(lib, gpu):
    """every refusal happens in front of the first launch; p = a zeroed input buffer, o1 .. o3 = distinct output buffers, all far
    larger than the tiny valid extents of the last line could touch"""
    bufs = [torch.zeros(1 << 12, device="cuda", dtype=F32) for _ in range(4)]
    p, o1, o2, o3 = (b.data_ptr() for b in bufs)
    ins, out2, out3 = (C.c_void_p * 1)(p), (C.c_void_p * 1)(o2), (C.c_void_p * 1)(o3)

    def fwd(sizes, B, L):
        return lib.ia_textcnn_pool_fwd(p, 8, ins, _ia(sizes), len(sizes), 1, B, L, 0.0, 0.0, 0, 0, 0, o1, o2, None)

    def bww(sizes, B, L, H):
        return lib.ia_textcnn_pool_bwd_w(p, p, p, p, _ia(sizes), len(sizes), 1, B, L, H, 0.0, 0.0, 0, 0, 0, out2, out3, None)

    def bwx(sizes, B, L, H):
        return lib.ia_textcnn_pool_bwd_x(p, p, ins, _ia(sizes), len(sizes), 1, B, L, H, 0.0, 0.0, 0, 0, 0, o1, None)

    def pack(sizes, F, H):
        return lib.ia_textcnn_pack_taps(ins, _ia(sizes), len(sizes), F, H, o1, None)

    assert fwd([5], 1, 4) == ERR_ARG and bww([5], 1, 4, 8) == ERR_ARG and bwx([5], 1, 4, 8) == ERR_ARG          # L < K
    assert bww([3], 1, 5, 12) == ERR_ARG and bwx([3], 1, 5, 12) == ERR_ARG and pack([3], 1, 12) == ERR_ARG      # H % 8
    assert fwd([3], 0, 5) == ERR_ARG and fwd([3], 1, 0) == ERR_ARG and fwd([0], 1, 5) == ERR_ARG and fwd([], 1, 5) == ERR_ARG
    assert bww([3], 0, 5, 8) == ERR_ARG and bwx([3], -1, 5, 8) == ERR_ARG and pack([3], 0, 8) == ERR_ARG and pack([3], 1, 0) == ERR_ARG
    assert lib.ia_textcnn_pool_fwd(p, 8, ins, _ia([3]), 1, 1, 1, 5, 1.0, 0.0, 0, 0, 0, o1, o2, None) == ERR_ARG      # p = 1
    torch.cuda.synchronize()
    assert fwd([5], 1, 5) == 0 and bww([5], 1, 5, 8) == 0 and bwx([5], 1, 5, 8) == 0 and pack([5], 1, 8) == 0
    torch.cuda.synchronize()


# ============================================================================================================ dropout
def test_dropout_draws_scale_and_backward(lib, cases):
    """p = 0.5 twice: the mask is the host replica's (two independent streams on element b NF + j), the kept share is within 4 sigma
    of (1 - p)^2, kept values carry 1 / (1 - p)^2, and the backward zeroes exactly the same entries"""
    B, L, F, sizes = 16, 12, 64, [1, 2]
    g = torch.Generator().manual_seed(77)
    NF = F * len(sizes)
    _off, nt, ntp = T.offsets(sizes, F)
    P = torch.randn((B * L, ntp), generator=g)
    bs = [torch.full((F,), 5.0) for _ in sizes]                       # every feature alive
    drop = (0.5, 0.5, 4242, 31, 32)
    mult = T.keep_mult(B * NF, *drop)
    want, warg, smax, _gap = T.pool_fwd(P, bs, sizes, B, L, mult)
    feat, arg = run_fwd(lib, P, bs, sizes, B, L, drop)
    kept = feat != 0
    assert (kept.reshape(-1) == (mult != 0)).all()
    n = B * NF
    share, sigma = float(kept.to(F64).mean()), (0.25 * 0.75 / n) ** 0.5
    assert abs(share - 0.25) <= 4 * sigma, (share, sigma)
    assert float(mult.max()) == 4.0
    r = _ratio("dropout feat", (feat.to(F64) - want).abs(), 4.0 * T.fwd_bound(sizes, F, smax).expand_as(want))
    assert r <= 1.0
    plain, _a = run_fwd(lib, P, bs, sizes, B, L)
    assert (feat[kept] == 4.0 * plain[kept]).all()                      # scaling by a power of two is exact
    # backward: db of a gradient that is live in row b only is g' of that row
    gr = torch.randn((B, NF), generator=g)
    H = 8
    x = torch.zeros((B * L, H), dtype=BF16)
    for b in (0, 5, B - 1):
        gb = torch.zeros_like(gr)
        gb[b] = gr[b]
        _dW, db = run_bwd_w(lib, gb, warg, x, x, sizes, F, L, drop)
        got = torch.cat(db)
        assert ((got != 0) == kept[b]).all()
        assert (got[kept[b]] == 4.0 * gr[b][kept[b]]).all()
    Ws = [torch.ones((F, 2, K, H)) for K in sizes]
    dx = run_bwd_x(lib, gr, warg, Ws, sizes, L, drop)
    wdx, mag = T.pool_bwd_x(gr, warg, Ws, sizes, L, mult)
    bf16_close("dropout dx", dx, wdx, (NF + 1) * R.U24 * mag)


# ============================================================================================================ packing
@pytest.mark.parametrize("shape", [T.KERNEL_SHAPES[0], T.KERNEL_SHAPES[2], T.KERNEL_SHAPES[4]], ids=T.shape_id)
def test_tap_packing_is_bit_exact(lib, cases, shape):
    c = cases(shape)
    Wd = _cu(c.Ws)
    _off, _nt, ntp = T.offsets(c.sizes, c.F)
    taps = torch.full((2, ntp, c.H), 1.5, device="cuda", dtype=BF16)           # the padding rows must come back zero
    _sync(lib.ia_textcnn_pack_taps(_pa(Wd), _ia(c.sizes), len(c.sizes), c.F, c.H, taps.data_ptr(), None), "ia_textcnn_pack_taps")
    assert bits_equal(taps.cpu(), T.pack_taps(c.Ws, c.sizes).to(BF16))
