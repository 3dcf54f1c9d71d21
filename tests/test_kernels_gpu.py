"""Per-kernel parity on the GPU: each HIP kernel (through the C ABI) against a plain PyTorch fp32
reference of the same op on identical bf16-rounded inputs.  Tolerances (written per test):
bf16 outputs 2e-2 relative to the tensor's max magnitude (north_star: 5e-2 bf16), fp32 outputs 2e-3."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def rnd(shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 256, 192), (1000, 3072, 1024), (77, 64, 64), (4096, 1024, 4096)])
def test_gemm_nt_epilogues(gpu, M, N, K):
    from item_alignment_amd import ops
    a, w = rnd((M, K), gpu, 1.0, 1), rnd((N, K), gpu, 0.05, 2)
    bias = torch.randn(N, device=gpu)
    aux = rnd((M, N), gpu, 1.0, 3)
    ref = a.float() @ w.float().t()
    assert rel_err(ops.gemm(a, w), ref) < 2e-2
    assert rel_err(ops.gemm(a, w, epilogue=ops.EPI_BIAS, bias=bias), ref + bias) < 2e-2
    act, der = ops.gemm(a, w, epilogue=ops.EPI_BIAS_GELU, bias=bias)      # activation and its saved derivative
    x = (ref + bias).requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    assert rel_err(act, torch.nn.functional.gelu(x.detach())) < 2e-2
    assert rel_err(der, x.grad) < 2e-2
    assert rel_err(ops.gemm(a, w, epilogue=ops.EPI_BIAS_ADD, bias=bias, aux=aux), ref + bias + aux.float()) < 2e-2
    assert rel_err(ops.gemm(a, w, out_f32=True), ref) < 2e-3


@pytest.mark.parametrize("M,N,K", [(70000, 1024, 1024), (65280, 1024, 4096), (66000, 768, 1088), (40000, 2304, 128), (33000, 4096, 200),
                                   (130560, 1024, 1024)])
def test_gemm_lookahead_kernel_matches_the_draining_one(gpu, monkeypatch, M, N, K):
    """t256la (round 6): the plain NT GEMM whose k pipeline runs on across tile boundaries -- the last two trips of a tile fetch the NEXT
    tile's first k-tiles through a second descriptor pair -- against t256w, which drains and refills per tile (IA_GEMM_LA=0): the same
    MFMAs on the same operands in the same order, so the outputs must be bit-identical; and against torch fp32.  Shapes with several
    tiles per workgroup (otherwise the dispatcher keeps t256w), ragged M (clipped last tile row), ragged K (partial last k-tile), K = 128
    (two k-tiles: the whole loop is look-ahead), a tile count that is no multiple of the grid."""
    from item_alignment_amd import ops
    a, w = rnd((M, K), gpu, 1.0, 81), rnd((N, K), gpu, 0.05, 82)
    monkeypatch.setenv("IA_GEMM_LA", "1")
    y1 = ops.gemm(a, w).clone()
    y1b = ops.gemm(a, w).clone()
    monkeypatch.setenv("IA_GEMM_LA", "0")
    y0 = ops.gemm(a, w).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y1b)
    assert torch.equal(y1, y0)
    rows = torch.cat((torch.arange(0, 512), torch.arange(M // 2, M // 2 + 512), torch.arange(M - 512, M))).to(gpu)
    ref = a[rows].float() @ w.float().t()
    assert rel_err(y1[rows], ref) < 2e-2


@pytest.mark.parametrize("M,N", [(256, 256), (512, 128), (77, 64)])
def test_gemm_gelu_epilogue_accuracy(gpu, M, N):
    """The FFN1 epilogue's GELU pair against the exact erf form (reference hidden_act = "gelu") at chosen pre-activations.  The GEMM is
    x = 1 * bias (A = a one-hot column, W = ones in that column), so every output is exactly the bf16-exact bias value: a sweep over
    [-12, 12] including the outliers past the range the sigmoid-form polynomial was fitted on.  Bounds: the fit's own error
    (3e-5 / 1.1e-4, tools/fit_gelu.py) plus half a bf16 ulp of the stored result."""
    from item_alignment_amd import ops
    K = 64
    a = torch.zeros((M, K), device=gpu, dtype=torch.bfloat16); a[:, 0] = 1
    w = torch.zeros((N, K), device=gpu, dtype=torch.bfloat16)           # x[m][n] = bias[n] exactly
    xs = torch.linspace(-12, 12, N, device=gpu).to(torch.bfloat16).float()
    xs[0], xs[-1] = -30.0, 30.0
    act, der = ops.gemm(a, w, epilogue=ops.EPI_BIAS_GELU, bias=xs)
    x64 = xs.double().cpu()
    Phi = 0.5 * (1 + torch.erf(x64 / 2 ** 0.5))
    want_act = x64 * Phi
    want_der = Phi + x64 * torch.exp(-x64 * x64 / 2) / (2 * torch.pi) ** 0.5
    for got, want, fit_err in ((act, want_act, 3.0e-5), (der, want_der, 1.1e-4)):
        g = got.double().cpu()
        assert torch.isfinite(g).all()
        assert (g - g[0:1]).abs().max().item() == 0.0                     # every row saw the same pre-activations
        tol = fit_err * 1.2 + want.abs() * 2.0 ** -8
        assert ((g[0] - want).abs() <= tol).all(), ((g[0] - want).abs() - tol).max().item()


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 192, 256), (1000, 1024, 3072), (510, 64, 192)])
def test_gemm_nn_dgrad(gpu, M, N, K):
    """dX = dY W: A k-contiguous, B = W[K(red)][N] k-strided."""
    from item_alignment_amd import ops
    dy, w = rnd((M, K), gpu, 1.0, 4), rnd((K, N), gpu, 0.05, 5)
    aux = rnd((M, N), gpu, 1.0, 6)
    ref = dy.float() @ w.float()
    assert rel_err(ops.gemm(dy, w, b_kstrided=True), ref) < 2e-2
    assert rel_err(ops.gemm(dy, w, b_kstrided=True, epilogue=ops.EPI_ADD, aux=aux), ref + aux.float()) < 2e-2
    # EPI_DGELU multiplies by the derivative the forward's EPI_BIAS_GELU epilogue saved
    assert rel_err(ops.gemm(dy, w, b_kstrided=True, epilogue=ops.EPI_DGELU, aux=aux), ref * aux.float()) < 2e-2


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (192, 64, 300), (1024, 3072, 1000), (3072, 1024, 2040), (64, 64, 40)])
def test_gemm_tn_wgrad(gpu, M, N, K):
    """dW[M,N] = dY^T X with dY stored [K, M] and X stored [K, N]; fp32 out, accumulate."""
    from item_alignment_amd import ops
    dy, x = rnd((K, M), gpu, 1.0, 7), rnd((K, N), gpu, 1.0, 8)
    ref = dy.float().t() @ x.float()
    out = ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True)
    assert rel_err(out, ref) < 2e-3
    out2 = ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True, out=out.clone(), accumulate=True)
    assert rel_err(out2, 2 * ref) < 2e-3


@pytest.mark.parametrize("M,H", [(7, 64), (300, 768), (1021, 1024), (64, 4096)])
def test_layernorm_fwd_bwd(gpu, M, H):
    from item_alignment_amd import ops
    x, res = rnd((M, H), gpu, 1.0, 9), rnd((M, H), gpu, 1.0, 10)
    bias = torch.randn(H, device=gpu) * 0.1
    gamma, beta = torch.rand(H, device=gpu) + 0.5, torch.randn(H, device=gpu) * 0.1
    y, z, mean, rstd = ops.ln_fwd(x, gamma, beta, 1e-12, bias=bias, residual=res)
    zr = (x.float() + bias + res.float())
    assert rel_err(z, zr) < 1e-2
    zf = z.float().requires_grad_(True)
    g = gamma.clone().requires_grad_(True); b = beta.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(zf, (H,), g, b, 1e-12)
    assert rel_err(y, yr) < 1e-2
    dy = rnd((M, H), gpu, 1.0, 11)
    dres = rnd((M, H), gpu, 1.0, 12)
    yr.backward(dy.float())
    dg, db, dbias = torch.zeros(H, device=gpu), torch.zeros(H, device=gpu), torch.zeros(H, device=gpu)
    dz, _ = ops.ln_bwd(dy, z, mean, rstd, gamma, dres=dres, dgamma=dg, dbeta=db, dbias=dbias)
    assert rel_err(dz, zf.grad + dres.float()) < 1e-2
    assert rel_err(dg, g.grad) < 2e-3
    assert rel_err(db, b.grad) < 2e-3
    assert rel_err(dbias, (zf.grad + dres.float()).sum(0)) < 1e-2   # sums bf16-rounded-free fp32 values
    # plain LN (ViT): no bias / residual / z
    y2, z2, m2, r2 = ops.ln_fwd(x, gamma, beta, 1e-6, write_z=False)
    assert z2 is None
    assert rel_err(y2, torch.nn.functional.layer_norm(x.float(), (H,), gamma, beta, 1e-6)) < 1e-2


@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (1000, 776, 192), (4096 + 130, 1024, 256)])
def test_gemm_dgelu_with_fused_column_sums(gpu, M, N, K):
    """IA_EPI_DGELU_COLSUM: same C as IA_EPI_DGELU, and the fp32 column sums of C (before its rounding to bf16) added into C2."""
    from item_alignment_amd import ops
    torch.manual_seed(M + N)
    a = (torch.randn(M, K, device="cuda") * 0.5).bfloat16()
    b = (torch.randn(K, N, device="cuda") * 0.5).bfloat16()
    aux = torch.rand(M, N, device="cuda").bfloat16()
    want = ops.gemm(a, b, b_kstrided=True, epilogue=ops.EPI_DGELU, aux=aux)
    prior = torch.randn(N, device="cuda")
    cs = prior.clone()
    got = ops.gemm(a, b, b_kstrided=True, epilogue=ops.EPI_DGELU_COLSUM, aux=aux, colsum_out=cs)
    assert torch.equal(got, want)
    ref = (a.float() @ b.float()) * aux.float()
    tol = 2e-3 * ref.abs().sum(0).max().item()
    assert (cs - prior - ref.sum(0)).abs().max().item() < tol
    assert (cs - prior - want.float().sum(0)).abs().max().item() < tol


@pytest.mark.parametrize("M,N,K", [(64, 576, 5000), (128, 128, 70000), (1024, 1024, 4096 + 40)])
def test_gemm_wgrad_form_emits_row_sums(gpu, M, N, K):
    """Weight-gradient form (A, B k-strided, fp32 C) with C2: C2[m] += sum_k A[k][m] -- the bias gradient out of the same launch
    (T128: one more MFMA against ones, split-K partials folded by the reduce kernel; 256x256 shapes: the column-sum pass).  All three
    shapes run T128 today: (1024, 1024, 4136), meant for the column-sum pass, plans 16 tiles x 8 = 128 < 160.  The 256-wide form with C2
    is in tests/test_gemm_kernels_gpu.py (test_t256w_weight_gradient_split_k, K = 5120 / 5160 / 7168, path asserted)."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    torch.manual_seed(K)
    dy = torch.randn((K, M), device=gpu).bfloat16()
    x = torch.randn((K, N), device=gpu).bfloat16()
    dw = torch.empty((M, N), device=gpu, dtype=torch.float32)
    prior = torch.randn(M, device=gpu)
    db = prior.clone()
    wsb = max(lib.ia_gemm_workspace_bytes(M, N, K, 1), lib.ia_colsum_workspace_bytes(K, M), 16)
    ws = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    check(lib.ia_gemm_bf16(dy.data_ptr(), 1, M, x.data_ptr(), 1, N, dw.data_ptr(), 1, N, M, N, K, 0, None, None, 0, db.data_ptr(), 0, ws.data_ptr(), wsb,
                           stream_ptr()), "ia_gemm_bf16")
    assert rel_err(dw, dy.float().t() @ x.float()) < 2e-3
    ref = dy.float().sum(0)
    assert ((db - prior - ref).abs().max() / ref.abs().max()).item() < 2e-3


def test_colsum(gpu):
    from item_alignment_amd import ops
    x = rnd((1000, 3072), gpu, 1.0, 13)
    out = torch.ones(3072, device=gpu)
    ops.colsum(x, out, accumulate=True)
    assert rel_err(out, x.float().sum(0) + 1) < 1e-4


def attn_ref(qkv, B, L, nh, mask, dctx=None):
    H = nh * 64
    t = qkv.float().view(B, L, 3, nh, 64).requires_grad_(dctx is not None)
    q, k, v = t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2), t[:, :, 2].transpose(1, 2)
    s = q @ k.transpose(-1, -2) * 0.125
    if mask is not None:
        s = s + (1.0 - mask.float())[:, None, None, :] * torch.finfo(torch.float32).min
    p = torch.softmax(s, -1)
    ctx = (p @ v).transpose(1, 2).reshape(B * L, H)
    if dctx is None:
        return ctx, None
    ctx.backward(dctx.float())
    return ctx.detach(), t.grad.reshape(B * L, 3 * H)


@pytest.mark.parametrize("B,L,nh,masked", [(2, 20, 1, True), (3, 64, 2, False), (2, 255, 4, True), (2, 510, 16, True),
                                           (2, 577, 12, False), (1, 129, 2, True), (2, 220, 16, True), (2, 248, 16, True),
                                           # lengths just past a multiple of 256 (the 128- / 256-query forward forms meet a nearly empty last block)
                                           (2, 300, 2, True), (1, 513, 3, True), (3, 577, 2, True), (1, 769, 1, False)])
def test_attention_fwd_bwd(gpu, B, L, nh, masked):
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 14)
    dctx = rnd((B * L, H), gpu, 1.0, 15)
    mask = None
    if masked:
        lens = torch.tensor([L - 3 * (i + 1) for i in range(B)])
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(gpu)
        if L > 40:
            mask[0, 17] = 0   # a hole: the mask is arbitrary, not only a prefix
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask)
    ref, dref = attn_ref(qkv, B, L, nh, mask, dctx)
    assert rel_err(ctx, ref) < 2e-2
    dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask)
    for i, name in enumerate("qkv"):
        got = dqkv.view(B * L, 3, H)[:, i]
        want = dref.view(B * L, 3, H)[:, i]
        assert rel_err(got, want) < 3e-2, name


@pytest.mark.parametrize("B,L,nh,masked,drop", [(2, 255, 4, True, 0.0), (2, 577, 3, False, 0.0), (2, 130, 2, True, 0.1), (1, 510, 2, True, 0.0),
                                                (3, 20, 1, True, 0.0), (2, 255, 16, True, 0.1)])
def test_attention_exact_delta_opt_in(gpu, monkeypatch, B, L, nh, masked, drop):
    """IA_ATTN_EXACT_DELTA=1 (round 6): a pre-pass forms the softmax-gradient delta_q = sum_k P_qk dP_qk in fp32 and the dQ / dK,dV kernels
    read it, instead of the flash-style rowsum(dO o O) taken from the bf16-ROUNDED context (reference: torch autograd of
    transformers' RobertaSelfAttention, src/models/text.py:1241, differentiates softmax exactly).  Checked: the delta it leaves equals
    rowsum(dO o O_fp32) of the fp32 reference; the gradients keep the common bar; on an operand set built to make dP - delta a small
    difference of large numbers (near-uniform P, value rows that differ little -- the shape of the C5 last-layer case)
    the exact form is several times closer to fp32 than the default; with dropout the results stay finite and within bf16 of the
    default's; switching the variable off again restores the default bit for bit."""
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 54)
    dctx = rnd((B * L, H), gpu, 1.0, 55)
    mask = None
    if masked:
        lens = torch.tensor([L - 3 * (i + 1) for i in range(B)])
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(gpu)
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=drop, seed=9)
    flash = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=9)
    monkeypatch.setenv("IA_ATTN_EXACT_DELTA", "1")
    exact, delta = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=9, return_delta=True)
    exact_b = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=9, dbias=torch.zeros(3 * H, device=gpu))
    assert torch.equal(exact, exact_b)                              # both entry points take the same route
    assert torch.isfinite(exact).all() and torch.isfinite(delta).all()
    assert rel_err(exact, flash) < 3e-2
    if drop == 0.0:
        ref, dref = attn_ref(qkv, B, L, nh, mask, dctx)
        want = (dctx.float() * ref).view(B, L, nh, 64).sum(-1).permute(0, 2, 1)      # rowsum(dO o O) with the fp32 context = sum_k P dP
        assert rel_err(delta, want) < 1e-2
        for i, name in enumerate("qkv"):
            assert rel_err(exact.view(B * L, 3, H)[:, i], dref.view(B * L, 3, H)[:, i]) < 3e-2, name
        # the adverse case: P near uniform, dP nearly the same for every key
        g = torch.Generator(device="cpu").manual_seed(77)
        t = torch.randn((B * L, 3, nh, 64), generator=g)
        t[:, 0] *= 0.05
        t[:, 2] = torch.randn((1, nh, 64), generator=g) + 0.02 * t[:, 2]
        qkv2 = t.reshape(B * L, 3 * H).to(gpu).to(torch.bfloat16)
        ctx2, lse2 = ops.attn_fwd(qkv2, B, L, nh, key_mask=mask)
        ref2, dref2 = attn_ref(qkv2, B, L, nh, mask, dctx)
        e2 = ops.attn_bwd(qkv2, ctx2, dctx, lse2, B, L, nh, key_mask=mask)
        monkeypatch.setenv("IA_ATTN_EXACT_DELTA", "0")
        f2 = ops.attn_bwd(qkv2, ctx2, dctx, lse2, B, L, nh, key_mask=mask)
        want_q, want_k = dref2.view(B * L, 3, H)[:, 0], dref2.view(B * L, 3, H)[:, 1]
        err = {n: (rel_err(x.view(B * L, 3, H)[:, 0], want_q), rel_err(x.view(B * L, 3, H)[:, 1], want_k)) for n, x in (("exact", e2), ("flash", f2))}
        print("adverse case, (dq, dk) error against fp32:", err)
        # measured on an MI355X: flash 0.13-0.24 / 0.05-0.11, exact 0.013-0.050 / 0.005-0.030 (the largest at L = 20, where a row's 20
        # rounded probabilities are the noise floor for either form)
        assert err["exact"][0] < 6e-2 and err["exact"][1] < 4e-2, err
        assert err["exact"][0] < 0.5 * err["flash"][0] and err["exact"][1] < 0.5 * err["flash"][1], err
    monkeypatch.setenv("IA_ATTN_EXACT_DELTA", "0")
    assert torch.equal(flash, ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=9))


@pytest.mark.parametrize("B,L,nh,drop", [(6, 255, 4, 0.0), (5, 255, 16, 0.1), (4, 130, 2, 0.0), (3, 64, 1, 0.1), (2, 510, 2, 0.0), (4, 510, 3, 0.1),
                                         (3, 385, 2, 0.0), (5, 577, 1, 0.0)])
def test_attention_backward_skips_query_blocks_of_masked_positions(gpu, B, L, nh, drop):
    """ia_attn_bwd_bias_ex(IA_ATTN_MASKED_ROWS_DEAD) (round 6): where the gradient arriving at every masked position is zero -- an encoder
    whose heads read [CLS] / valid spans only; reference src/models/text.py:1241 under its attention mask -- the one-kernel backward
    leaves out the 32-query blocks that hold only masked positions.  On such inputs dqkv and the bias gradient equal the unflagged call's
    (exactly: what is skipped multiplies zeros), with ragged lengths from one valid block to a full sequence, a hole in the mask,
    dropout on and off; L > 256 runs the dQ / dK,dV kernel pair: a wave of the dQ kernel whose 32 queries are masked skips its arithmetic,
    a workgroup without a live query walks one key tile, the dK/dV kernel's query loop ends at the last unmasked position."""
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 64)
    lens = torch.tensor([max(1, (L * (i + 1)) // (B + 1) - 5 * i) for i in range(B - 1)] + [L])
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(gpu)
    if L > 40:
        mask[-1, 33:70] = 0                                        # a hole that swallows a whole 32-position block of a full-length sequence
    dctx = rnd((B * L, H), gpu, 1.0, 65) * mask.view(B * L, 1).to(torch.bfloat16)      # zero at every masked position
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=drop, seed=3)
    db0 = torch.zeros(3 * H, device=gpu)
    full = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=3, dbias=db0)
    db1 = torch.zeros(3 * H, device=gpu)
    skip = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=3, dbias=db1, masked_rows_dead=True)
    assert torch.isfinite(skip).all()
    assert torch.equal(full, skip) and torch.equal(db0, db1)
    # and the rows of masked positions carry no gradient at all (q: zero rows; k, v: masked keys get P = 0)
    dead = (mask.view(B * L) == 0)
    assert (skip[dead].float().abs().max().item() if dead.any() else 0.0) == 0.0


@pytest.mark.parametrize("B,L,nh,masked,drop", [(3, 255, 4, True, 0.0), (2, 577, 3, False, 0.0), (2, 130, 2, True, 0.1), (1, 64, 1, False, 0.0)])
def test_attention_bwd_bias_gradient(gpu, B, L, nh, masked, drop):
    """ia_attn_bwd_bias: the QKV bias gradient out of the attention backward epilogues = column sums of the dqkv it stores (exactly the
    stored bf16 values, fp32 sums), accumulated into dbias; dqkv itself is bit-identical to ia_attn_bwd's."""
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 24)
    dctx = rnd((B * L, H), gpu, 1.0, 25)
    mask = None
    if masked:
        lens = torch.tensor([L - 7 * (i + 1) for i in range(B)])
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(gpu)
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=drop, seed=5)
    plain = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=5)
    dbias = torch.full((3 * H,), 0.5, device=gpu, dtype=torch.float32)
    fused = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=5, dbias=dbias)
    assert torch.equal(plain, fused)
    want = 0.5 + fused.float().sum(0)
    assert (dbias - want).abs().max().item() <= 1e-3 * (1.0 + want.abs().max().item())


@pytest.mark.parametrize("B,L,nh", [(2, 128, 2), (1, 200, 3)])
def test_attention_dropout_mask_is_the_same_in_forward_and_both_backward_kernels(gpu, B, L, nh):
    """The dropped, rescaled probabilities A = P o M / keep are recovered from the forward kernel itself (V = shifted one-hot rows: the
    output is then a 64-column window of A), the plain P from a run without dropout; the backward of the dropout run must equal the
    closed form built from exactly that A (dV = A^T dO, dS = P o (M/keep o dP - delta)) -- i.e. the dQ and the dK/dV kernels regenerate
    the forward's mask bit for bit."""
    from item_alignment_amd import ops
    H = nh * 64
    drop, seed, scale = 0.25, 77, 0.125
    qkv = rnd((B * L, 3 * H), gpu, 0.7, 31)
    dctx = rnd((B * L, H), gpu, 1.0, 32)

    def probs(drop_p):
        A = torch.zeros((B, nh, L, L), device=gpu)
        for j0 in range(0, L, 64):
            t = qkv.clone().view(B, L, 3, nh, 64)
            t[:, :, 2] = 0
            for d in range(min(64, L - j0)):
                t[:, j0 + d, 2, :, d] = 1.0
            out, _ = ops.attn_fwd(t.view(B * L, 3 * H), B, L, nh, drop_p=drop_p, seed=seed)
            w = min(64, L - j0)
            A[:, :, :, j0:j0 + w] = out.float().view(B, L, nh, 64).permute(0, 2, 1, 3)[..., :w]
        return A

    P, A = probs(0.0), probs(drop)
    keepmask = A > 0
    frac = 1.0 - keepmask.float().mean().item() - (P <= 1e-30).float().mean().item()
    assert abs(frac - drop) < 0.02, frac
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, drop_p=drop, seed=seed)
    dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, drop_p=drop, seed=seed).float().view(B, L, 3, nh, 64)
    t = qkv.float().view(B, L, 3, nh, 64)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    do = dctx.float().view(B, L, nh, 64).permute(0, 2, 1, 3)
    o = A @ v
    assert rel_err(ctx.float().view(B, L, nh, 64).permute(0, 2, 1, 3), o) < 3e-2
    Mk = torch.where(keepmask, A / P.clamp_min(1e-30), torch.zeros_like(A))          # M / keep
    dp = Mk * (do @ v.transpose(-1, -2))
    delta = (do * o).sum(-1, keepdim=True)
    ds = P * (dp - delta)
    want = [ds @ k * scale, ds.transpose(-1, -2) @ q * scale, A.transpose(-1, -2) @ do]
    for i, name in enumerate("qkv"):
        got = dqkv[:, :, i].permute(0, 2, 1, 3)
        assert rel_err(got, want[i]) < 4e-2, name


def test_attention_dropout_statistics(gpu):
    """Dropout on the attention probabilities: mean preserved, fwd/bwd use the same mask (checked by
    linearity: with V = const the output stays ~const)."""
    from item_alignment_amd import ops
    B, L, nh = 2, 255, 4
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 16)
    qkv.view(B * L, 3, H)[:, 2] = 1.0
    ctx, _ = ops.attn_fwd(qkv, B, L, nh, drop_p=0.1, seed=123)
    m = ctx.float().mean().item()
    assert abs(m - 1.0) < 0.02, m
    ctx2, _ = ops.attn_fwd(qkv, B, L, nh, drop_p=0.1, seed=123)
    assert torch.equal(ctx, ctx2)
    ctx3, _ = ops.attn_fwd(qkv, B, L, nh, drop_p=0.1, seed=124)
    assert not torch.equal(ctx, ctx3)


# ------------------------------------------------------------------ CoCa multimodal-layer kernels
@pytest.mark.parametrize("B,nh,Lq,Lk", [(2, 3, 100, 177), (3, 1, 20 * 2, 17), (2, 1, 255 * 4, 577), (1, 2, 130, 64),
                                        # Lq == Lk in (32, 256] with ld_q != ld_kv: the general entry point takes the single-kernel
                                        # backward here too (q rows of stride H, k / v rows of stride 2H, separate dq / dkv strides)
                                        (2, 3, 130, 130), (3, 1, 200, 200), (2, 2, 256, 256), (5, 4, 33, 33)])
def test_attention_x_fwd_bwd(gpu, B, nh, Lq, Lk):
    """ia_attn_fwd_x / ia_attn_bwd_x (cross attention; nh = 1 with folded query heads = multi-query attention)
    against fp32 softmax(q k^T / 8) v on the same bf16 inputs (reference multimodal.py:605-620, :686-696)."""
    from item_alignment_amd.models import functional as Fn
    H = nh * 64
    q = rnd((B * Lq, H), gpu, 1.0, 1).requires_grad_(True)
    kv = rnd((B * Lk, 2 * H), gpu, 1.0, 2).requires_grad_(True)
    dout = rnd((B * Lq, H), gpu, 1.0, 3)
    out = Fn.AttentionXFn.apply(q, kv, B, nh, Lq, Lk, 0.125)
    out.backward(dout)
    qf = q.detach().float().view(B, Lq, nh, 64).transpose(1, 2).requires_grad_(True)
    kf = kv.detach().float()[:, :H].reshape(B, Lk, nh, 64).transpose(1, 2).requires_grad_(True)
    vf = kv.detach().float()[:, H:].reshape(B, Lk, nh, 64).transpose(1, 2).requires_grad_(True)
    ref = torch.softmax(qf @ kf.transpose(-1, -2) * 0.125, dim=-1) @ vf
    ref.backward(dout.float().view(B, Lq, nh, 64).transpose(1, 2))
    back = lambda t: t.transpose(1, 2).reshape(t.shape[0] * t.shape[2], H)
    assert rel_err(out, back(ref)) < 2e-2
    assert rel_err(q.grad, back(qf.grad)) < 3e-2
    assert rel_err(kv.grad[:, :H], back(kf.grad)) < 3e-2
    assert rel_err(kv.grad[:, H:], back(vf.grad)) < 3e-2


def test_rotary_split_and_swiglu(gpu):
    """ia_rotary_split_* and ia_swiglu_* through FusedSplitFn against the reference formulas
    (multimodal.py:495-524: inv_freq = 10000^(-2i/64), rotate_half, silu(gate) * x)."""
    from item_alignment_amd.models import functional as Fn
    B, n, heads, F_ = 3, 37, 4, 96
    M, ld = B * n, heads * 64 + 128 + 2 * F_
    fused = rnd((M, ld), gpu, 1.0, 5).requires_grad_(True)
    q, kv, s = Fn.FusedSplitFn.apply(fused, n, heads, F_)
    gq, gkv, gs = rnd(q.shape, gpu, 1.0, 6), rnd(kv.shape, gpu, 1.0, 7), rnd(s.shape, gpu, 1.0, 8)
    torch.autograd.backward([q, kv, s], [gq, gkv, gs])

    f = fused.detach().float().requires_grad_(True)
    fq, fk, fv, ff = f.split((heads * 64, 64, 64, 2 * F_), dim=-1)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2, device=gpu).float() / 64))
    pos = torch.arange(n, device=gpu).float().repeat(B)[:, None] * inv_freq[None, :]
    pos = torch.cat((pos, pos), dim=-1)                                     # [M, 64]

    def rot(t):
        x1, x2 = t[..., :32], t[..., 32:]
        return t * pos.cos().view(M, *([1] * (t.dim() - 2)), 64) + torch.cat((-x2, x1), dim=-1) * pos.sin().view(M, *([1] * (t.dim() - 2)), 64)
    rq = rot(fq.reshape(M, heads, 64)).reshape(M, heads * 64)
    rkv = torch.cat((rot(fk), fv), dim=-1)
    xg, gate = ff.chunk(2, dim=-1)
    rs = torch.nn.functional.silu(gate) * xg
    torch.autograd.backward([rq, rkv, rs], [gq.float(), gkv.float(), gs.float()])
    assert rel_err(q, rq) < 2e-2 and rel_err(kv, rkv) < 2e-2 and rel_err(s, rs) < 2e-2
    assert rel_err(fused.grad, f.grad) < 2e-2

    src = rnd((M, 2 * F_), gpu, 1.0, 9).requires_grad_(True)
    out = Fn.SwiGLUFn.apply(src)
    out.backward(gs)
    sf = src.detach().float().requires_grad_(True)
    a, b = sf.chunk(2, dim=-1)
    r = torch.nn.functional.silu(b) * a
    r.backward(gs.float())
    assert rel_err(out, r) < 2e-2 and rel_err(src.grad, sf.grad) < 2e-2


@pytest.mark.parametrize("measure", ["inner_product", "cosine", "l1", "l2"])
def test_pair_sim_head(gpu, measure):
    """ia_pair_sim_fwd/bwd against torch.nn.functional (what reference base.py:75-88 calls), fp32: 1e-4."""
    from item_alignment_amd.models import functional as Fn
    import torch.nn.functional as F
    g = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn((7, 200), generator=g) * 0.3).to(gpu).requires_grad_(True)
    y = (torch.randn((7, 200), generator=g) * 0.3).to(gpu).requires_grad_(True)
    sim, probs = Fn.PairSimFn.apply(x, y, Fn.SIM_MEASURES[measure])
    w1, w2 = torch.randn(7, device=gpu), torch.randn(7, device=gpu)
    ((sim * w1).sum() + (probs * w2).sum()).backward()
    xr, yr = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    if measure == "cosine":
        s = F.cosine_similarity(xr, yr); p = (s + 1) / 2
    elif measure in ("l1", "l2"):
        s = F.pairwise_distance(xr, yr, p=1 if measure == "l1" else 2); p = torch.exp(-s)
    else:
        s = (xr * yr).sum(-1); p = torch.sigmoid(s)
    ((s * w1).sum() + (p * w2).sum()).backward()
    assert rel_err(sim, s) < 1e-4 and rel_err(probs, p) < 1e-4
    assert rel_err(x.grad, xr.grad) < 1e-4 and rel_err(y.grad, yr.grad) < 1e-4


# ------------------------------------------------------------------ full-size properties and edge shapes
def test_gemm_full_size_checksum(gpu):
    """BASELINE-size GEMM (ffn1 of the C5 text tower: 32640 x 4096 x 1024) through a size-independent property:
    sum_mn C[m,n] == sum_k (sum_m A[m,k]) (sum_n W[n,k])  — a checksum of checksums, fp32 output, 1e-3 relative
    (the sum runs over 1.3e8 products of bf16 inputs; both sides are accumulated in fp64 on the host side of the check)."""
    from item_alignment_amd import ops
    M, N, K = 32640, 4096, 1024
    a, w = rnd((M, K), gpu, 1.0, 11), rnd((N, K), gpu, 0.05, 12)
    c = ops.gemm(a, w, out_f32=True)
    want = (a.double().sum(0) * w.double().sum(0)).sum()
    got = c.double().sum()
    scale = (a.double().abs().sum(0) * w.double().abs().sum(0)).sum()
    assert abs(got - want) / scale < 1e-6, (got.item(), want.item())
    # and one bf16-output row block against fp32 matmul
    cb = ops.gemm(a, w)
    assert rel_err(cb[-300:], a[-300:].float() @ w.float().t()) < 2e-2


@pytest.mark.parametrize("B,L,nh,masked", [(16, 577, 12, False), (32, 255, 16, True), (4, 510, 16, True)])
def test_attention_full_size_rows_sum_to_one(gpu, B, L, nh, masked):
    """Full-size attention through softmax's defining property: with V == 1 every output element is exactly the row sum
    of P, i.e. 1 (bf16: 1 +- 2^-8), for any mask that leaves a query at least one key; and dV = P^T dO column sums give
    sum(dV) == sum(dO) on attended keys (sum over keys of P is 1 per query)."""
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 21)
    qkv[:, 2 * H:] = 1.0
    mask = None
    if masked:
        g = torch.Generator().manual_seed(3)
        lens = torch.randint(1, L + 1, (B,), generator=g)
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(gpu)
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask)
    assert (ctx.float() - 1.0).abs().max().item() <= 2 ** -7
    d = rnd((B * L, H), gpu, 1.0, 22)
    dqkv = ops.attn_bwd(qkv, ctx, d, lse, B, L, nh, key_mask=mask)
    dv = dqkv[:, 2 * H:].float().view(B, L, nh, 64)
    want = d.float().view(B, L, nh, 64).sum(1)
    got = dv.sum(1)
    assert rel_err(got, want) < 2e-2
    if masked:   # keys outside the mask receive exactly zero gradient
        dead = (mask == 0).view(B, L, 1, 1)
        assert (dqkv.float().view(B, L, 3, nh, 64)[:, :, 1:] * dead.unsqueeze(2)).abs().max().item() == 0.0


@pytest.mark.parametrize("B,L,nh", [(1, 1, 1), (2, 64, 2), (3, 65, 1), (1, 129, 3)])
def test_attention_edge_lengths(gpu, B, L, nh):
    """tile-boundary sequence lengths (1, exactly one tile, one past a tile, one past two tiles) incl. a key mask that
    leaves only the first token attendable in sequence 0."""
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 31)
    mask = torch.ones((B, L), dtype=torch.uint8, device=gpu)
    mask[0, 1:] = 0
    dctx = rnd((B * L, H), gpu, 1.0, 32)
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask)
    dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask)
    ref, rgrad = attn_ref(qkv, B, L, nh, mask, dctx)
    assert rel_err(ctx, ref) < 2e-2
    got = dqkv.float().view(B * L, 3, nh, 64)
    want = rgrad.view(B * L, 3, nh, 64)
    for i in range(3):   # a sequence whose only attendable key is token 0 has dq == dk == 0: compare on an absolute floor
        assert (got[:, i] - want[:, i]).abs().max().item() < 3e-2 * max(want[:, i].abs().max().item(), 1e-2), i


def test_layernorm_full_size_statistics(gpu):
    """Full-size LayerNorm (32640 x 1024): with gamma = 1, beta = 0 every output row has mean 0 and variance 1."""
    from item_alignment_amd import ops
    M, H = 32640, 1024
    x = rnd((M, H), gpu, 3.0, 41)
    y, _, mean, rstd = ops.ln_fwd(x, torch.ones(H, device=gpu), torch.zeros(H, device=gpu), 1e-12, write_z=False)
    yf = y.float()
    assert yf.mean(1).abs().max().item() < 2e-2
    assert (yf.var(1, unbiased=False) - 1).abs().max().item() < 3e-2
    assert rel_err(mean, x.float().mean(1)) < 1e-4


@pytest.mark.parametrize("H,W,S", [(800, 800, 384), (600, 811, 384), (96, 130, 224), (801, 640, 800)])
def test_gpu_image_pipeline_bit_exact(gpu, tmp_path, H, W, S):
    """ia_resize_pass_u8(_ex) + ia_color_jitter_step_u8 + ia_u8_to_nchw_normalized against the restatement
    of the transform the reference applies on the host (oracle/timm_transform.py: timm create_transform, data.py:838-866) on the
    same decoded frames and the same random draw: plain resizes bit-exact for both filters, the evaluation transform
    (bilinear Resize(floor(S / 0.875)) + CenterCrop) bit-exact, the training transform (RandomResizedCrop window, flip, colour
    jitter in its random order) bit-exact - uint8 pixels and the normalised fp32 tensor."""
    import numpy as np
    from PIL import Image
    from item_alignment_amd.data.datasets import RawImage
    from item_alignment_amd.data.gpu_preproc import GpuImagePipeline
    from item_alignment_amd.data.transforms import ImageTransform
    from oracle import timm_transform as TT
    rs = np.random.RandomState(H + W)
    frames = rs.randint(0, 256, size=(3, H, W, 3)).astype(np.uint8)
    for filt, pil in (("bicubic", Image.BICUBIC), ("bilinear", Image.BILINEAR)):
        pipe = GpuImagePipeline(S, gpu, filt=filt)
        got_u8 = pipe.resize(torch.from_numpy(frames)).cpu().numpy()
        for i in range(3):
            assert np.array_equal(got_u8[i], np.asarray(Image.fromarray(frames[i]).resize((S, S), pil))), (filt, i)
    pipe = GpuImagePipeline(S, gpu)
    imgs = [Image.fromarray(f) for f in frames]
    # evaluation transform, batched
    ev = ImageTransform(S, False)
    out = pipe.process([RawImage(torch.from_numpy(f), ev.draw(W, H)) for f in frames]).cpu()
    for i in range(3):
        assert torch.equal(out[i], TT.eval_transform(imgs[i], S)), ("eval", i)
    # training transform with every random ingredient, several draws; evaluation and training items mixed in one batch
    tr = ImageTransform(S, True, hflip=0.5, color_jitter=0.4, seed=H * 7 + W)
    items, want = [], []
    for rep in range(3):
        for i in range(3):
            p = tr.draw(W, H)
            items.append(RawImage(torch.from_numpy(frames[i]), p))
            want.append(TT.train_transform(imgs[i], S, TT.TrainParams(p.box, p.flip, p.jitter)))
    items.append(RawImage(torch.from_numpy(frames[0]), ev.draw(W, H)))
    want.append(TT.eval_transform(imgs[0], S))
    out = pipe.process(items).cpu()
    for i in range(len(items)):
        assert torch.equal(out[i], want[i]), ("train", i, items[i].params)
    assert any(it.params.flip for it in items) and any(it.params.jitter[0][0] == 1 for it in items[:-1] if it.params.jitter)


@pytest.mark.parametrize("M,N,K", [(1024, 1024, 64), (1024, 1024, 128), (1024, 768, 8), (1000, 520, 72), (3000, 4096, 64), (8200, 2056, 256),
                                   (512, 512, 4104)])
def test_gemm_one_wave_per_simd_kernel_edges(gpu, M, N, K):
    """Written as the edge test of the T256W kernel (one wave per SIMD; serves the plain / bias / +residual / fp32 / weight-gradient forms
    of large GEMMs): one and two k-tiles (its loop prefetches k-tile u+2 and reads k-tile u+1 ahead), ragged K, clipped M / N tiles (bias
    fetched before the main loop only for full tiles, bf16-staged epilogue vs the fp32-staged fall-back), more tiles than workgroups.
    make_plan has since moved the 256-wide kernels to outputs of 160 tiles of 256 x 256 and more (fp32 output: tiles x min(32,
    k-tiles / 8)): of these seven shapes only (3000, 4096, 64) and (8200, 2056, 256) still reach T256W, the other five run T128 -- no
    shape here reaches T256W with two k-tiles, with K < 64 or with K = 72.  Those edges, with the path asserted and every element held to
    fp64, are in tests/test_gemm_kernels_gpu.py (test_t256w_bf16_edges, test_t256w_weight_gradient_split_k); this test stays as the
    norm check of both kernels at these shapes."""
    from item_alignment_amd import ops
    a, w = rnd((M, K), gpu, 1.0, 61), rnd((N, K), gpu, 0.1, 62)
    bias = torch.randn(N, device=gpu)
    aux = rnd((M, N), gpu, 1.0, 63)
    ref = a.float() @ w.float().t()
    assert rel_err(ops.gemm(a, w), ref) < 2e-2
    assert rel_err(ops.gemm(a, w, epilogue=ops.EPI_BIAS, bias=bias), ref + bias) < 2e-2
    assert rel_err(ops.gemm(a, w, epilogue=ops.EPI_BIAS_ADD, bias=bias, aux=aux), ref + bias + aux.float()) < 2e-2
    assert rel_err(ops.gemm(a, w, out_f32=True), ref) < 2e-3
    assert rel_err(ops.gemm(a, w, epilogue=ops.EPI_BIAS, bias=bias, out_f32=True), ref + bias) < 2e-3
    wt, at = w.t().contiguous(), a.t().contiguous()
    assert rel_err(ops.gemm(a, wt, b_kstrided=True), ref) < 2e-2
    assert rel_err(ops.gemm(at, wt, a_kstrided=True, b_kstrided=True, out_f32=True), ref) < 2e-3


@pytest.mark.parametrize("M,N,K,epi", [(8200, 2056, 256, "none"), (8200, 2056, 320, "bias_gelu"), (16500, 1032, 192, "add")])
def test_gemm_persistent_rounds_with_clipped_tiles(gpu, M, N, K, epi):
    """More than 256 output tiles (the T256 kernel loops over tiles per workgroup, keeps the previous tile's stores in
    flight behind a counted wait) with both M and N clipping the last tiles: the whole output against fp32 matmul."""
    from item_alignment_amd import ops
    a, w = rnd((M, K), gpu, 1.0, 51), rnd((N, K), gpu, 0.1, 52)
    ref = a.float() @ w.float().t()
    if epi == "none":
        assert rel_err(ops.gemm(a, w), ref) < 2e-2
    elif epi == "bias_gelu":
        bias = torch.randn(N, device=gpu)
        act, der = ops.gemm(a, w, epilogue=ops.EPI_BIAS_GELU, bias=bias)
        x = (ref + bias).requires_grad_(True)
        torch.nn.functional.gelu(x).sum().backward()
        assert rel_err(act, torch.nn.functional.gelu(x.detach())) < 2e-2
        assert rel_err(der, x.grad) < 2e-2
    else:
        aux = rnd((M, N), gpu, 1.0, 53)
        assert rel_err(ops.gemm(a, w, epilogue=ops.EPI_ADD, aux=aux), ref + aux.float()) < 2e-2
    # run it again right behind itself: stores of the first launch's last tiles must not be disturbed by the second
    out1 = ops.gemm(a, w)
    out2 = ops.gemm(a, w)
    assert torch.equal(out1, out2)


def _pad_nhwc(t):
    """[B,H,W,C] -> zero-bordered [B,H+2,W+2,C]"""
    return torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1)).contiguous()


@pytest.mark.parametrize("B,H,W,Cin,Cout,groups", [(2, 7, 9, 64, 64, 1), (3, 25, 25, 128, 128, 2), (1, 50, 50, 384, 384, 6), (2, 13, 200, 64, 64, 1),
                                                   (2, 30, 21, 16, 32, 1), (1, 40, 40, 32, 64, 1), (2, 12, 12, 256, 256, 1), (1, 9, 10, 128, 64, 1),
                                                   (2, 11, 8, 64, 32, 2)])
def test_conv3x3_padded_domain(gpu, B, H, W, Cin, Cout, groups):
    """Patch-matrix-free (grouped) 3x3 convolution (shifted-view GEMMs over the zero-bordered NHWC tensor, all groups in one
    launch) against torch conv2d in fp32 on the same bf16-rounded inputs: forward, data gradient, weight + bias gradient."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    ci = Cin // groups
    x = rnd((B, H, W, Cin), gpu, 1.0, 11)
    w = rnd((Cout, ci, 3, 3), gpu, 0.05, 12)                              # torch layout [Cout][Cin/groups][ky][kx]
    bias = torch.randn(Cout, device=gpu)
    dy = rnd((B, H, W, Cout), gpu, 1.0, 13)
    what = w.permute(0, 2, 3, 1).reshape(Cout, 9 * ci).contiguous()      # [o][t*ci + c]
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.float().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xr, wr, br, padding=1, groups=groups)
    ref.backward(dy.float().permute(0, 3, 1, 2))

    xp, dyp = _pad_nhwc(x), _pad_nhwc(dy)
    yp = torch.empty_like(dyp)
    check(lib.ia_conv3x3_padded_fwd(xp.data_ptr(), what.data_ptr(), bias.data_ptr(), yp.data_ptr(), B, H, W, Cin, Cout, groups, stream_ptr()), "fwd")
    assert rel_err(yp[:, 1:-1, 1:-1], ref.permute(0, 2, 3, 1)) < 2e-2
    dxp = torch.empty_like(xp)
    check(lib.ia_conv3x3_padded_bwd_data(dyp.data_ptr(), what.data_ptr(), dxp.data_ptr(), B, H, W, Cin, Cout, groups, stream_ptr()), "bwd_data")
    assert rel_err(dxp[:, 1:-1, 1:-1], xr.grad.permute(0, 2, 3, 1)) < 2e-2
    wsb = lib.ia_conv3x3_padded_workspace_bytes(B, H, W, Cin, Cout, groups)
    ws = torch.empty(max(wsb, 16), device=gpu, dtype=torch.uint8)
    dwhat = torch.empty((Cout, 9 * ci), device=gpu, dtype=torch.float32)
    dbias = torch.zeros(Cout, device=gpu)
    check(lib.ia_conv3x3_padded_bwd_weight(xp.data_ptr(), dyp.data_ptr(), dwhat.data_ptr(), dbias.data_ptr(), B, H, W, Cin, Cout, groups,
                                           ws.data_ptr(), wsb, stream_ptr()), "bwd_weight")
    assert rel_err(dwhat.view(Cout, 3, 3, ci).permute(0, 3, 1, 2), wr.grad) < 2e-3
    assert rel_err(dbias, br.grad) < 2e-3


@pytest.mark.parametrize("B,H,W,groups,ci,co", [(3, 37, 41, 1, 64, 64), (2, 25, 25, 6, 64, 64), (1, 8, 30, 2, 64, 64), (2, 9, 31, 1, 64, 64),
                                                (1, 200, 200, 1, 64, 64), (5, 50, 50, 3, 64, 64), (40, 7, 5, 2, 64, 64),
                                                (2, 61, 45, 1, 16, 32), (2, 33, 64, 1, 32, 64), (1, 400, 400, 1, 16, 32), (3, 17, 9, 2, 32, 64),
                                                (1, 317, 331, 1, 64, 64), (4, 100, 100, 2, 64, 64), (2, 250, 203, 1, 16, 32)])
def test_conv3x3_direct_few_channel_groups(gpu, monkeypatch, B, H, W, groups, ci, co):
    """The direct 3x3 convolution for groups of 64 -> 64 channels (NF-Net stages) and the stem's 16 -> 32 / 32 -> 64 (conv.hip, dconv:
    filter bank resident in LDS, 8 x 30-pixel tiles with their halo staged once, taps as LDS row offsets; reference
    src/models/image.py:253-257 -> timm NormFreeBlock.conv2 / conv2b, create_stem) against torch conv2d in fp32 on the same bf16
    inputs, forward and data gradient (the same kernel <co, ci> on dy with the flipped, transposed bank); tile edges (H, W not
    multiples of 8 / 30, fewer tiles than workgroups, more), the output border left untouched, and the shifted-view GEMM it
    replaces within bf16 of it."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    Cin, Cout = groups * ci, groups * co
    assert lib.ia_conv3x3_direct_supported(Cin, Cout, groups) == 1
    assert lib.ia_conv3x3_direct_supported(groups * 128, groups * 128, groups) == 0
    x = rnd((B, H, W, Cin), gpu, 1.0, 21)
    w = rnd((Cout, ci, 3, 3), gpu, 0.05, 22)
    bias = torch.randn(Cout, device=gpu)
    dy = rnd((B, H, W, Cout), gpu, 1.0, 23)
    what = w.permute(0, 2, 3, 1).reshape(Cout, 9 * ci).contiguous()
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = torch.nn.functional.conv2d(xr, w.float(), bias, padding=1, groups=groups)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    # The bordered operands sit in the MIDDLE of NaN-filled buffers: the last image's bottom / right tiles reach past the end of the
    # tensor whenever H % 8 or W % 30 is not zero, and what they find there must be the DMA's range-check zeros, never the neighbouring
    # bytes (0 * NaN = NaN in dW; round-5 advisor finding: the piece advance sat in the scalar offset, which the range check ignores)
    def _in_nan_sea(t):
        sea = torch.full((t.numel() + 2 * 65536,), float("nan"), device=gpu, dtype=t.dtype)
        v = sea[65536:65536 + t.numel()].view(t.shape)
        v.copy_(t)
        return v
    xp, dyp = _in_nan_sea(_pad_nhwc(x)), _in_nan_sea(_pad_nhwc(dy))
    yp = torch.full_like(dyp, float("nan"))
    check(lib.ia_conv3x3_padded_fwd(xp.data_ptr(), what.data_ptr(), bias.data_ptr(), yp.data_ptr(), B, H, W, Cin, Cout, groups, stream_ptr()), "fwd")
    got = yp[:, 1:-1, 1:-1]
    assert torch.isfinite(got).all()
    assert rel_err(got, ref.permute(0, 2, 3, 1)) < 2e-2
    assert torch.isnan(yp[:, 0]).all() and torch.isnan(yp[:, :, 0]).all() and torch.isnan(yp[:, -1]).all() and torch.isnan(yp[:, :, -1]).all()   # border untouched
    what_t = torch.empty((Cin, 9 * co), device=gpu, dtype=torch.bfloat16)
    check(lib.ia_conv3x3_flip_weights(what.data_ptr(), what_t.data_ptr(), Cin, Cout, groups, stream_ptr()), "flip")
    want_t = w.view(groups, co, ci, 3, 3).flip(3, 4).permute(0, 2, 3, 4, 1).reshape(Cin, 9 * co)       # [g][ci][tap'][co]
    assert torch.equal(what_t, want_t.contiguous())
    dxp = torch.full_like(xp, float("nan"))
    check(lib.ia_conv3x3_padded_bwd_data_t(dyp.data_ptr(), what_t.data_ptr(), dxp.data_ptr(), B, H, W, Cin, Cout, groups, stream_ptr()), "bwd_data_t")
    assert rel_err(dxp[:, 1:-1, 1:-1], xr.grad.permute(0, 2, 3, 1)) < 2e-2
    dx2 = torch.empty_like(xp)
    check(lib.ia_conv3x3_padded_bwd_data(dyp.data_ptr(), what.data_ptr(), dx2.data_ptr(), B, H, W, Cin, Cout, groups, stream_ptr()), "bwd_data")
    assert rel_err(dxp[:, 1:-1, 1:-1], dx2[:, 1:-1, 1:-1]) < 1e-2
    # weight + bias gradient: the direct kernel (dy and x tiles in LDS, transposed fragment reads, per-workgroup fp32 banks folded in
    # fixed order), twice -- bit-identical -- and against autograd
    wr = w.float().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=1, groups=groups).backward(dy.float().permute(0, 3, 1, 2))
    wsb = lib.ia_conv3x3_padded_workspace_bytes(B, H, W, Cin, Cout, groups)
    ws = torch.empty(max(wsb, 16), device=gpu, dtype=torch.uint8)
    # (maps below 1e5 pixels are routed to the split-K GEMM: the second pass forces the direct kernel onto them too, so its ragged tile
    # rows / columns are tested at every shape of the list, not only at the three large ragged ones)
    for force_direct in (False, True):
        if force_direct:
            monkeypatch.setenv("IA_CONV_DIRECT_WGRAD_MIN", "0")
        outs = []
        for _ in range(2):
            dwhat = torch.full((Cout, 9 * ci), float("nan"), device=gpu, dtype=torch.float32)
            dbias = torch.full((Cout,), 0.25, device=gpu)
            check(lib.ia_conv3x3_padded_bwd_weight(xp.data_ptr(), dyp.data_ptr(), dwhat.data_ptr(), dbias.data_ptr(), B, H, W, Cin, Cout, groups,
                                                   ws.data_ptr(), wsb, stream_ptr()), "bwd_weight")
            outs.append((dwhat, dbias))
        assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert rel_err(outs[0][0].view(Cout, 3, 3, ci).permute(0, 3, 1, 2), wr.grad) < 2e-3
        assert rel_err(outs[0][1] - 0.25, br.grad) < 2e-3


@pytest.mark.parametrize("B,HW,Cmid,C", [(3, 625, 384, 1536), (2, 10000, 128, 512), (5, 49, 64, 256)])
def test_eca_block_tail_pools_through_the_1x1_convolution(gpu, B, HW, Cmid, C):
    """ia_eca_fwd_linear: the NormFreeBlock tail out = x * sigmoid(conv1d(mean_HW x)) * coef + shortcut (reference src/models/image.py:253-257
    -> timm NormFreeBlock.forward: attn_last(conv3(.)) * alpha + shortcut) with the pooling taken from conv3's INPUT a -- mean_HW(a what^T +
    bias) = (mean_HW a) what^T + bias -- against torch in fp32 on the same bf16 operands, and against ia_eca_fwd (the reduction over the
    bf16-rounded x itself), whose gate it must match to the rounding of x; ia_eca_bwd runs unchanged on the saved pooled / gate."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    k, coef = 5, 0.4
    a = rnd((B * HW, Cmid), gpu, 1.0, 31)
    what = rnd((C, Cmid), gpu, Cmid ** -0.5, 32)
    bias = torch.randn(C, device=gpu) * 0.3
    shortcut = rnd((B * HW, C), gpu, 1.0, 33)
    conv_w = torch.randn(k, device=gpu) * 0.5
    x32 = a.float() @ what.float().t() + bias                      # what the convolution computes before its output is rounded
    x = x32.to(torch.bfloat16)
    pooled_ref = x32.view(B, HW, C).mean(1)
    gate_ref = torch.sigmoid(torch.nn.functional.conv1d(pooled_ref.view(B, 1, C), conv_w.view(1, 1, k), padding=(k - 1) // 2).view(B, C))
    out_ref = x.float().view(B, HW, C) * gate_ref[:, None, :] * coef + shortcut.float().view(B, HW, C)
    out, pooled, gate = torch.empty_like(x), torch.empty((B, C), device=gpu), torch.empty((B, C), device=gpu)
    wsb = lib.ia_eca_fwd_linear_workspace_bytes(B, HW, Cmid)
    ws = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    check(lib.ia_eca_fwd_linear(x.data_ptr(), a.data_ptr(), what.data_ptr(), bias.data_ptr(), Cmid, conv_w.data_ptr(), k, shortcut.data_ptr(),
                                out.data_ptr(), None, 1.0, pooled.data_ptr(), gate.data_ptr(), B, HW, C, coef, ws.data_ptr(), wsb, stream_ptr()),
          "ia_eca_fwd_linear")
    assert rel_err(pooled, pooled_ref) < 1e-4
    assert rel_err(gate, gate_ref) < 1e-4
    assert rel_err(out.view(B, HW, C), out_ref) < 1e-2
    assert lib.ia_eca_fwd_linear(x.data_ptr(), a.data_ptr(), what.data_ptr(), bias.data_ptr(), Cmid, conv_w.data_ptr(), k, shortcut.data_ptr(),
                                 out.data_ptr(), None, 1.0, pooled.data_ptr(), gate.data_ptr(), B, HW, C, coef, ws.data_ptr(), wsb - 1, stream_ptr()) != 0
    # the next block's opening activation out of the same pass: bit-identical to ia_silu_fwd on the stored out, and out itself unchanged
    out_a, act = torch.empty_like(x), torch.empty_like(x)
    check(lib.ia_eca_fwd_linear(x.data_ptr(), a.data_ptr(), what.data_ptr(), bias.data_ptr(), Cmid, conv_w.data_ptr(), k, shortcut.data_ptr(),
                                out_a.data_ptr(), act.data_ptr(), 0.93, pooled.data_ptr(), gate.data_ptr(), B, HW, C, coef, ws.data_ptr(), wsb,
                                stream_ptr()), "ia_eca_fwd_linear[act]")
    want_act = torch.empty_like(x)
    check(lib.ia_silu_fwd(out.data_ptr(), want_act.data_ptr(), out.numel(), 0.93, stream_ptr()), "ia_silu_fwd")
    assert torch.equal(out_a, out) and torch.equal(act, want_act)
    out2, pooled2, gate2 = torch.empty_like(x), torch.empty_like(pooled), torch.empty_like(gate)
    wsb2 = lib.ia_gap_workspace_bytes(B, HW, C)
    ws2 = torch.empty(wsb2, device=gpu, dtype=torch.uint8)
    check(lib.ia_eca_fwd(x.data_ptr(), conv_w.data_ptr(), k, shortcut.data_ptr(), out2.data_ptr(), pooled2.data_ptr(), gate2.data_ptr(), B, HW, C, coef,
                         ws2.data_ptr(), wsb2, stream_ptr()), "ia_eca_fwd")
    assert rel_err(pooled, pooled2) < 2e-3 and rel_err(gate, gate2) < 2e-3          # the old path sums the ROUNDED x: bf16 noise, averaged over HW
    assert rel_err(out.view(B, HW, C), out2.view(B, HW, C)) < 1e-2


@pytest.mark.parametrize("B,HW,C,two,direct", [(3, 625, 1536, False, True), (2, 2500, 512, True, False), (5, 49, 256, False, False), (2, 10000, 256, True, True)])
def test_eca_block_tail_backward_folds_the_next_activation(gpu, B, HW, C, two, direct):
    """ia_eca_silu_bwd (round 6): the backward of a NormFreeBlock tail that also wrote the next block's opening activation -- out's whole
    gradient dtot = (dact [+ dact2]) * act_scale * silu'(out) [+ dout_direct] and the ECA gate gradient's spatial sums of dtot * x in ONE pass
    -- is bit-identical to the two-kernel form it replaces (ia_silu_bwd / ia_silu_bwd_sum, then ia_eca_bwd on its result): dtot, dx and
    the conv1d weight gradient; and matches torch autograd of the tail in fp32 (reference src/models/image.py:253-257 -> timm
    NormFreeBlock.forward: out = attn_last(x) * alpha + shortcut, next block: act1(out) * beta)."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    k, coef, beta = 5, 0.4, 0.93
    x = rnd((B * HW, C), gpu, 1.0, 41)
    shortcut = rnd((B * HW, C), gpu, 1.0, 42)
    conv_w = torch.randn(k, device=gpu) * 0.5
    dact, dact2, ddir = rnd((B * HW, C), gpu, 1.0, 43), rnd((B * HW, C), gpu, 1.0, 44), rnd((B * HW, C), gpu, 1.0, 45)
    out, pooled, gate = torch.empty_like(x), torch.empty((B, C), device=gpu), torch.empty((B, C), device=gpu)
    wsf = lib.ia_gap_workspace_bytes(B, HW, C)
    ws = torch.empty(wsf, device=gpu, dtype=torch.uint8)
    check(lib.ia_eca_fwd(x.data_ptr(), conv_w.data_ptr(), k, shortcut.data_ptr(), out.data_ptr(), pooled.data_ptr(), gate.data_ptr(), B, HW, C, coef,
                         ws.data_ptr(), wsf, stream_ptr()), "ia_eca_fwd")
    p2 = dact2.data_ptr() if two else None
    pd = ddir.data_ptr() if direct else None
    wsb = lib.ia_eca_bwd_workspace_bytes(B, HW, C)
    wsb_t = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    # the two-kernel form
    dtot_a = torch.empty_like(x)
    if two:
        check(lib.ia_silu_bwd_sum(dact.data_ptr(), p2, out.data_ptr(), pd, dtot_a.data_ptr(), out.numel(), beta, stream_ptr()), "ia_silu_bwd_sum")
    else:
        check(lib.ia_silu_bwd(dact.data_ptr(), out.data_ptr(), pd, dtot_a.data_ptr(), out.numel(), beta, stream_ptr()), "ia_silu_bwd")
    dx_a, dw_a = torch.empty_like(x), torch.zeros(k, device=gpu)
    check(lib.ia_eca_bwd(dtot_a.data_ptr(), x.data_ptr(), conv_w.data_ptr(), k, pooled.data_ptr(), gate.data_ptr(), dx_a.data_ptr(), dw_a.data_ptr(),
                         B, HW, C, coef, wsb_t.data_ptr(), wsb, stream_ptr()), "ia_eca_bwd")
    # the fused form
    dtot_b, dx_b, dw_b = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.zeros(k, device=gpu)
    check(lib.ia_eca_silu_bwd(dact.data_ptr(), p2, out.data_ptr(), pd, beta, x.data_ptr(), conv_w.data_ptr(), k, pooled.data_ptr(), gate.data_ptr(),
                              dtot_b.data_ptr(), dx_b.data_ptr(), dw_b.data_ptr(), B, HW, C, coef, wsb_t.data_ptr(), wsb, stream_ptr()), "ia_eca_silu_bwd")
    assert torch.equal(dtot_a, dtot_b) and torch.equal(dx_a, dx_b) and torch.equal(dw_a, dw_b)
    # torch autograd of the same function in fp32
    xr, sr, wr = x.float().view(B, HW, C).requires_grad_(True), shortcut.float().view(B, HW, C).requires_grad_(True), conv_w.clone().requires_grad_(True)
    g_ = torch.sigmoid(torch.nn.functional.conv1d(xr.mean(1).view(B, 1, C), wr.view(1, 1, k), padding=(k - 1) // 2).view(B, C))
    o_ = xr * g_[:, None, :] * coef + sr
    a_ = torch.nn.functional.silu(o_) * beta
    loss = (a_ * dact.float().view(B, HW, C)).sum()
    if two:
        loss = loss + (a_ * dact2.float().view(B, HW, C)).sum()
    if direct:
        loss = loss + (o_ * ddir.float().view(B, HW, C)).sum()
    loss.backward()
    assert rel_err(dtot_b.view(B, HW, C), sr.grad) < 2e-2
    assert rel_err(dx_b.view(B, HW, C), xr.grad) < 2e-2
    assert rel_err(dw_b, wr.grad) < 2e-2


def test_silu_between_padded_and_compact_layouts(gpu):
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    B, H, W, C = 2, 6, 5, 64
    x = rnd((B, H, W, C), gpu, 2.0, 21)
    xp = _pad_nhwc(x)
    xp_dirty = xp.clone()
    xp_dirty[:, 0], xp_dirty[:, -1], xp_dirty[:, :, 0], xp_dirty[:, :, -1] = 7.0, -7.0, 3.0, -3.0     # garbage border of a conv output
    xr = x.float().requires_grad_(True)
    ref = torch.nn.functional.silu(xr) * 1.7
    dy = rnd((B, H, W, C), gpu, 1.0, 22)
    ref.backward(dy.float())
    dyp = _pad_nhwc(dy)
    for in_p, out_p in ((0, 1), (1, 1), (1, 0)):
        src = xp_dirty if in_p else x
        y = torch.full_like(xp if out_p else x, 9.0)
        check(lib.ia_silu_pad_fwd(src.data_ptr(), y.data_ptr(), B, H, W, C, 1.7, in_p, out_p, stream_ptr()), "silu_pad_fwd")
        if out_p:
            assert rel_err(y[:, 1:-1, 1:-1], ref) < 1e-2
            inner = y.clone()
            inner[:, 1:-1, 1:-1] = 0
            assert inner.abs().max().item() == 0.0                        # the border is written as zero
        else:
            assert rel_err(y, ref) < 1e-2
        g = dyp if out_p else dy
        dx = torch.full_like(src, 9.0)
        check(lib.ia_silu_pad_bwd(g.data_ptr(), src.data_ptr(), dx.data_ptr(), B, H, W, C, 1.7, in_p, out_p, stream_ptr()), "silu_pad_bwd")
        if in_p:
            assert rel_err(dx[:, 1:-1, 1:-1], xr.grad) < 1e-2
            inner = dx.clone()
            inner[:, 1:-1, 1:-1] = 0
            assert inner.abs().max().item() == 0.0
        else:
            assert rel_err(dx, xr.grad) < 1e-2


@pytest.mark.parametrize("rows,C,segments", [(64, 64, 1), (2 * 1000, 256, 2), (3 * 77, 16, 3), (4096, 2048, 1)])
def test_batchnorm_relu_fwd_bwd(gpu, rows, C, segments):
    """ia_bn_act_* (BatchNorm2d + ReLU on NHWC rows, per-segment batch statistics) against torch batch_norm in fp32 on the same
    bf16-rounded input, one call per segment as the reference's two tower calls do; running statistics included."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    x = rnd((rows, C), gpu, 1.5, 31) + 0.4
    dy = rnd((rows, C), gpu, 1.0, 32)
    extra = rnd((rows, C), gpu, 1.0, 33)
    gg = torch.Generator().manual_seed(34)
    gamma = (1 + 0.2 * torch.randn(C, generator=gg)).to(gpu).contiguous()
    beta = (0.1 * torch.randn(C, generator=gg)).to(gpu).contiguous()
    rm, rv = torch.zeros(C, device=gpu), torch.ones(C, device=gpu)
    rm_ref, rv_ref = rm.clone(), rv.clone()
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rps = rows // segments
    ys = [torch.relu(torch.nn.functional.batch_norm(xr[s * rps:(s + 1) * rps].t().reshape(1, C, rps), rm_ref, rv_ref, gr, br, True, 0.1, 1e-5))
          for s in range(segments)]
    ref = torch.cat([y.reshape(C, rps).t() for y in ys])
    ref.backward(dy.float())

    y = torch.empty_like(x)
    mean = torch.empty((segments, C), device=gpu)
    rstd = torch.empty((segments, C), device=gpu)
    wsb = lib.ia_bn_act_workspace_bytes(rows, C, segments)
    ws = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    check(lib.ia_bn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(),
                            rstd.data_ptr(), rows, C, segments, 1e-5, 0.1, 1, 1, ws.data_ptr(), wsb, stream_ptr()), "bn_fwd")
    assert rel_err(y, ref) < 1e-2
    assert rel_err(rm, rm_ref) < 1e-3 and rel_err(rv, rv_ref) < 1e-3
    dx = torch.empty_like(x)
    dg, db = torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
    check(lib.ia_bn_act_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), extra.data_ptr(),
                            dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, C, segments, 1, 1, ws.data_ptr(), wsb, stream_ptr()), "bn_bwd")
    assert rel_err(dx, xr.grad + extra.float()) < 2e-2
    assert rel_err(dg, gr.grad) < 1e-2 and rel_err(db, br.grad) < 1e-2     # a ReLU-mask flip at a pre-activation of ~0 moves one term
    # eval mode: running statistics
    check(lib.ia_bn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(),
                            rstd.data_ptr(), rows, C, segments, 1e-5, 0.1, 0, 1, ws.data_ptr(), wsb, stream_ptr()), "bn_eval")
    ref_ev = torch.relu((x.float() - rm) * torch.rsqrt(rv + 1e-5) * gamma + beta)
    assert rel_err(y, ref_ev) < 1e-2


@pytest.mark.parametrize("B,H,W,Cin,Cout,groups,yc", [(2, 37, 45, 128, 128, 2, 0), (3, 16, 60, 64, 64, 1, 0), (2, 50, 31, 64, 128, 1, 1), (1, 8, 30, 384, 384, 6, 0),
                                                      (2, 63, 64, 64, 64, 1, 1), (5, 3, 2, 64, 64, 1, 0), (2, 61, 122, 64, 128, 1, 0)])
def test_conv3x3_stride2_without_a_patch_matrix(gpu, B, H, W, Cin, Cout, groups, yc):
    """ia_conv3x3_s2_padded_* (the strided convolutions of the NF-Net: stage transitions with 64 channels per group, the stem's 64 -> 128 as
    two output halves over one shared input slice) against torch conv2d / its autograd in fp32 on the same bf16 operands: odd and even
    maps, maps smaller than a tile, several tiles per row, bordered and compact (yc) output layouts.  The border of dy is filled with NaN
    for the weight gradient (it must not be read) and the output's border is left alone by the forward."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    assert lib.ia_conv3x3_s2_supported(Cin, Cout, groups) == 1 and lib.ia_conv3x3_s2_supported(96, 96, 1) == 0
    Cg, Ho, Wo = Cin // groups, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = rnd((B, H, W, Cin), gpu, 1.0, 81)
    what = rnd((Cout, 9 * Cg), gpu, 0.05, 82)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(83)).to(gpu)
    dy = rnd((B, Ho, Wo, Cout), gpu, 1.0, 84)
    w_ref = what.float().view(Cout, 9, Cg).permute(0, 2, 1).reshape(Cout, Cg, 3, 3).requires_grad_(True)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xr, w_ref, br, stride=2, padding=1, groups=groups)
    assert tuple(ref.shape) == (B, Cout, Ho, Wo)
    ref.backward(dy.float().permute(0, 3, 1, 2))

    def bordered(t, fill):
        if yc:
            return t.contiguous()
        out = torch.full((B, Ho + 2, Wo + 2, Cout), fill, device=gpu, dtype=torch.bfloat16)
        out[:, 1:-1, 1:-1] = t
        return out

    def interior(t):
        return t if yc else t[:, 1:-1, 1:-1]

    xp = torch.zeros((B, H + 2, W + 2, Cin), device=gpu, dtype=torch.bfloat16)
    xp[:, 1:-1, 1:-1] = x
    yp = bordered(torch.full((B, Ho, Wo, Cout), 7.0, device=gpu, dtype=torch.bfloat16), 7.0)
    check(lib.ia_conv3x3_s2_padded_fwd(xp.data_ptr(), what.data_ptr(), bias.data_ptr(), yp.data_ptr(), B, H, W, Cin, Cout, groups, yc, stream_ptr()), "s2_fwd")
    assert rel_err(interior(yp), ref.detach().permute(0, 2, 3, 1)) < 1e-2
    if not yc:
        edge = yp.clone()
        edge[:, 1:-1, 1:-1] = 7.0
        assert (edge == 7.0).all()                                         # the border is not written
    wsb = lib.ia_conv3x3_s2_padded_workspace_bytes(B, H, W, Cin, Cout, groups)
    ws = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    dyp = bordered(dy, float("nan"))
    dwhat = torch.full((Cout, 9 * Cg), 3.0, device=gpu, dtype=torch.float32)
    dbias = torch.full((Cout,), 0.5, device=gpu)
    check(lib.ia_conv3x3_s2_padded_bwd_weight(xp.data_ptr(), dyp.data_ptr(), dwhat.data_ptr(), dbias.data_ptr(), B, H, W, Cin, Cout, groups, yc, ws.data_ptr(),
                                              wsb, stream_ptr()), "s2_wgrad")
    dw_ref = w_ref.grad.view(Cout, Cg, 9).permute(0, 2, 1).reshape(Cout, 9 * Cg)
    assert torch.isfinite(dwhat).all()
    assert rel_err(dwhat, dw_ref) < 2e-3 and rel_err(dbias - 0.5, br.grad) < 2e-3
    dyz = bordered(dy, 0.0)
    # the one-kernel data gradient over the four parity classes of dx (flipped bank; zero-bordered or compact dy); the 64 -> 128 form runs
    # as two launches over the 64-channel slices of dy that add up in dx (one bf16 rounding more)
    what_t = torch.empty((Cout, 9 * Cg), device=gpu, dtype=torch.bfloat16)
    if Cin == Cout:
        check(lib.ia_conv3x3_flip_weights(what.data_ptr(), what_t.data_ptr(), Cin, Cout, groups, stream_ptr()), "flip")
    else:
        check(lib.ia_conv3x3_flip_weights(what.data_ptr(), what_t.data_ptr(), Cout, Cout, Cout // 64, stream_ptr()), "flip")
    dxd = torch.full((B, H + 2, W + 2, Cin), 9.0, device=gpu, dtype=torch.bfloat16)
    check(lib.ia_conv3x3_s2_padded_bwd_data_t(dyz.data_ptr(), what_t.data_ptr(), dxd.data_ptr(), B, H, W, Cin, Cout, groups, yc, stream_ptr()), "s2_dgrad_t")
    assert rel_err(dxd[:, 1:-1, 1:-1], xr.grad.permute(0, 2, 3, 1)) < (1e-2 if Cin == Cout else 1.5e-2)
    edge = dxd.clone()
    edge[:, 1:-1, 1:-1] = 9.0
    assert (edge == 9.0).all()
    # the same numbers as the patch-matrix path the model used until round 6 (bf16 outputs of fp32 sums in another order)
    y_old = torch.empty((B * Ho * Wo, Cout), device=gpu, dtype=torch.bfloat16)
    wsb2 = lib.ia_conv_nhwc_workspace_bytes(B, H, W, Cin, Cout, 3, 2, groups)
    ws2 = torch.empty(wsb2, device=gpu, dtype=torch.uint8)
    check(lib.ia_conv_nhwc_fwd(x.data_ptr(), what.data_ptr(), bias.data_ptr(), y_old.data_ptr(), B, H, W, Cin, Cout, 3, 2, groups, ws2.data_ptr(), wsb2,
                               stream_ptr()), "nhwc_fwd")
    assert rel_err(interior(yp).reshape(-1, Cout), y_old) < 1e-2


@pytest.mark.parametrize("images,hw,C,groups", [(3, 49, 192, 32), (2, 56 * 56, 768, 32), (4, 100, 32, 32), (2, 333, 64, 8), (1, 9, 6144, 32)])
def test_groupnorm_relu_fwd_bwd(gpu, images, hw, C, groups):
    """ia_gn_act_* (GroupNorm + ReLU on NHWC rows: the norm layer of the BiT towers; statistics per (image, group), groups of 6 / 24 / 1 /
    8 / 192 channels -- narrower and wider than a thread's eight) against torch group_norm in fp32 on the same bf16-rounded input:
    output, dx (with a second gradient added, the identity shortcut of a pre-activation block), dgamma, dbeta; the saved statistics are
    the group's, repeated per channel."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    rows = images * hw
    x = rnd((rows, C), gpu, 1.5, 71) * torch.linspace(0.3, 2.0, C, device=gpu).bfloat16() + 0.4
    dy = rnd((rows, C), gpu, 1.0, 72)
    extra = rnd((rows, C), gpu, 1.0, 73)
    gg = torch.Generator().manual_seed(74)
    gamma = (1 + 0.2 * torch.randn(C, generator=gg)).to(gpu).contiguous()
    beta = (0.1 * torch.randn(C, generator=gg)).to(gpu).contiguous()
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    nchw = xr.view(images, hw, C).permute(0, 2, 1)                                        # [images, C, hw]
    ref = torch.relu(torch.nn.functional.group_norm(nchw, groups, gr, br, 1e-5)).permute(0, 2, 1).reshape(rows, C)
    ref.backward(dy.float())

    y = torch.empty_like(x)
    mean, rstd = torch.empty((images, C), device=gpu), torch.empty((images, C), device=gpu)
    wsb = lib.ia_gn_act_workspace_bytes(rows, C, images)
    ws = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    check(lib.ia_gn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C, images, groups,
                            1e-5, 1, ws.data_ptr(), wsb, stream_ptr()), "gn_fwd")
    assert rel_err(y, ref) < 1e-2
    xg = x.float().view(images, hw, groups, C // groups)
    mu_ref = xg.mean((1, 3))
    rs_ref = torch.rsqrt(xg.var((1, 3), unbiased=False) + 1e-5)
    assert rel_err(mean.view(images, groups, C // groups), mu_ref[:, :, None].expand(-1, -1, C // groups)) < 1e-4
    assert rel_err(rstd.view(images, groups, C // groups), rs_ref[:, :, None].expand(-1, -1, C // groups)) < 1e-4
    dx = torch.empty_like(x)
    dg, db = torch.full((C,), 0.5, device=gpu), torch.full((C,), -0.25, device=gpu)           # accumulated into
    check(lib.ia_gn_act_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), extra.data_ptr(),
                            dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, C, images, groups, 1, ws.data_ptr(), wsb, stream_ptr()), "gn_bwd")
    assert rel_err(dx, xr.grad + extra.float()) < 2e-2
    assert rel_err(dg - 0.5, gr.grad) < 1e-2 and rel_err(db + 0.25, br.grad) < 1e-2
    # without the second gradient, and deterministic
    dx2, dx3 = torch.empty_like(x), torch.empty_like(x)
    for out in (dx2, dx3):
        check(lib.ia_gn_act_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, out.data_ptr(),
                                None, None, rows, C, images, groups, 1, ws.data_ptr(), wsb, stream_ptr()), "gn_bwd")
    assert rel_err(dx2, xr.grad) < 2e-2 and torch.equal(dx2, dx3)
    # argument checks: channels that do not split into the groups, a short workspace
    assert lib.ia_gn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C, images, 7, 1e-5, 1,
                             ws.data_ptr(), wsb, stream_ptr()) != 0
    assert lib.ia_gn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C, images, groups,
                             1e-5, 1, ws.data_ptr(), 16, stream_ptr()) != 0


@pytest.mark.parametrize("B,H,W,C", [(2, 9, 12, 16), (1, 32, 32, 64), (2, 7, 7, 8)])
def test_maxpool_with_a_ring_of_zeros(gpu, B, H, W, C):
    """The BiT stem (timm create_resnetv2_stem 'fixed'): ConstantPad2d(1, 0.) + MaxPool2d(3, 2, padding 0) -- the ring counts as zeros, so
    a border window of negative values yields 0 and routes no gradient.  Bit-exact forward, torch's gradient routing (ties included)."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    g = torch.Generator().manual_seed(13)
    x = (torch.randint(-5, 3, (B, H, W, C), generator=g).float() * 0.5).to(gpu).bfloat16()      # mostly negative, coarse: zero ties and wins
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = torch.nn.functional.max_pool2d(torch.nn.functional.pad(xr, (1, 1, 1, 1), value=0.0), 3, 2, 0)
    assert tuple(ref.shape[2:]) == (Ho, Wo)
    dy = rnd((B, Ho, Wo, C), gpu, 1.0, 15)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    y = torch.empty((B, Ho, Wo, C), device=gpu, dtype=torch.bfloat16)
    arg = torch.empty((B, Ho, Wo, C), device=gpu, dtype=torch.uint8)
    check(lib.ia_maxpool3s2_fwd_ex(x.data_ptr(), y.data_ptr(), arg.data_ptr(), B, H, W, C, 1, stream_ptr()), "maxpool_fwd_ex")
    assert torch.equal(y.float(), ref.detach().permute(0, 2, 3, 1))
    plain = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert not torch.equal(y.float(), plain)                                                # the ring did win somewhere
    dx = torch.empty_like(x)
    check(lib.ia_maxpool3s2_bwd(dy.data_ptr(), arg.data_ptr(), dx.data_ptr(), B, H, W, C, stream_ptr()), "maxpool_bwd")
    assert rel_err(dx, xr.grad.permute(0, 2, 3, 1)) < 1e-2


@pytest.mark.parametrize("B,H,W,C", [(2, 9, 12, 16), (1, 32, 32, 64), (2, 7, 7, 8)])
def test_maxpool_stem_patches_and_subsample(gpu, B, H, W, C):
    """MaxPool 3/2/1 (ties go to the first maximum, as PyTorch routes the gradient), the strided-row gather of a 1x1/2
    convolution and the 7x7/2 stem patch matrix, each against the torch op."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(-3, 4, (B, H, W, C), generator=g).float() * 0.5).to(gpu).bfloat16()      # coarse values: many ties
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = torch.nn.functional.max_pool2d(xr, 3, 2, 1)
    dy = rnd((B, Ho, Wo, C), gpu, 1.0, 5)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    y = torch.empty((B, Ho, Wo, C), device=gpu, dtype=torch.bfloat16)
    arg = torch.empty((B, Ho, Wo, C), device=gpu, dtype=torch.uint8)
    check(lib.ia_maxpool3s2_fwd(x.data_ptr(), y.data_ptr(), arg.data_ptr(), B, H, W, C, stream_ptr()), "maxpool_fwd")
    assert torch.equal(y.float(), ref.permute(0, 2, 3, 1))
    dx = torch.empty_like(x)
    check(lib.ia_maxpool3s2_bwd(dy.data_ptr(), arg.data_ptr(), dx.data_ptr(), B, H, W, C, stream_ptr()), "maxpool_bwd")
    assert rel_err(dx, xr.grad.permute(0, 2, 3, 1)) < 1e-2

    sub = torch.empty((B, Ho, Wo, C), device=gpu, dtype=torch.bfloat16)
    check(lib.ia_rows_subsample_fwd(x.data_ptr(), sub.data_ptr(), B, H, W, C, 2, stream_ptr()), "subsample_fwd")
    assert torch.equal(sub, x[:, ::2, ::2].contiguous())
    base = rnd((B, H, W, C), gpu, 1.0, 6)
    back = torch.empty_like(x)
    check(lib.ia_rows_subsample_bwd(dy.data_ptr(), base.data_ptr(), back.data_ptr(), B, H, W, C, 2, stream_ptr()), "subsample_bwd")
    want = base.float().clone()
    want[:, ::2, ::2] += dy.float()
    assert rel_err(back, want) < 1e-2

    img = torch.randn((B, 3, H * 4, W * 4), generator=g).to(gpu)
    Hs, Ws = (H * 4 + 6 - 7) // 2 + 1, (W * 4 + 6 - 7) // 2 + 1
    cols = torch.empty((B * Hs * Ws, 152), device=gpu, dtype=torch.bfloat16)
    check(lib.ia_patches_nchw(img.data_ptr(), cols.data_ptr(), B, 3, H * 4, W * 4, 7, 2, 3, 152, stream_ptr()), "patches")
    unf = torch.nn.functional.unfold(img, 7, padding=3, stride=2)                        # [B, 3*49 (c, ky, kx), L]
    want = unf.view(B, 3, 49, Hs * Ws).permute(0, 3, 2, 1).reshape(B * Hs * Ws, 147)      # column (ky*7+kx)*3 + c
    assert torch.equal(cols[:, :147].float(), want.bfloat16().float())
    assert cols[:, 147:].abs().max().item() == 0.0
    # the LDS-staged stem form walks output rows in 64-pixel segments: several segments, a ragged last one, odd image sizes
    for (Hi, Wi) in ((262, 302), (129, 131)):
        img = torch.randn((2, 3, Hi, Wi), generator=g).to(gpu)
        Hs, Ws = (Hi + 6 - 7) // 2 + 1, (Wi + 6 - 7) // 2 + 1
        cols = torch.full((2 * Hs * Ws, 152), 7.0, device=gpu, dtype=torch.bfloat16)
        check(lib.ia_patches_nchw(img.data_ptr(), cols.data_ptr(), 2, 3, Hi, Wi, 7, 2, 3, 152, stream_ptr()), "patches")
        unf = torch.nn.functional.unfold(img, 7, padding=3, stride=2)
        want = unf.view(2, 3, 49, Hs * Ws).permute(0, 3, 2, 1).reshape(2 * Hs * Ws, 147)
        assert torch.equal(cols[:, :147].float(), want.bfloat16().float()), (Hi, Wi)
        assert cols[:, 147:].abs().max().item() == 0.0


@pytest.mark.parametrize("nh,lens,drop", [(2, [5, 64, 1, 130], 0.0), (4, [255, 17, 129, 200, 64, 65], 0.0), (2, [70, 33], 0.1)])
def test_attention_packed_sequences_match_padded(gpu, nh, lens, drop):
    """ia_attn_fwd_varlen / ia_attn_bwd_varlen (unpadded rows + cu_seqlens) against the padded kernels with a key mask on the same
    tokens: outputs and gradients of the valid rows must agree to bf16 round-off (same arithmetic, different addressing);
    with dropout the two runs use the same (sequence, head, query, key) random stream, so they agree as well."""
    from item_alignment_amd import _lib, ops
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    B, L, H = len(lens), max(lens), nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 41)
    mask = torch.zeros((B, L), dtype=torch.uint8)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    mask = mask.to(gpu)
    # padded query rows get no gradient in a model (nothing downstream reads them); they would otherwise feed dK / dV of the valid keys
    d = rnd((B * L, H), gpu, 1.0, 42) * mask.reshape(-1, 1).to(torch.bfloat16)
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=drop, seed=7)
    dqkv = ops.attn_bwd(qkv, ctx, d, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=7)
    idx = mask.reshape(-1).bool().nonzero().squeeze(1)
    T = idx.numel()
    pq, pd = qkv.index_select(0, idx).contiguous(), d.index_select(0, idx).contiguous()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=gpu)
    out = torch.empty((T, H), device=gpu, dtype=torch.bfloat16)
    lse2 = torch.zeros((B, nh, L), device=gpu)
    base = pq.data_ptr()
    check(lib.ia_attn_fwd_varlen(base, base + 2 * H, base + 4 * H, 3 * H, cu.data_ptr(), T, out.data_ptr(), H, lse2.data_ptr(), B, nh, L, 0.125,
                                 drop, 7, stream_ptr()), "fwd_varlen")
    assert rel_err(out, ctx.index_select(0, idx)) < 1e-2
    dp = torch.empty_like(pq)
    delta = torch.empty((B, nh, L), device=gpu)
    db = dp.data_ptr()
    check(lib.ia_attn_bwd_varlen(base, base + 2 * H, base + 4 * H, 3 * H, cu.data_ptr(), T, out.data_ptr(), pd.data_ptr(), H, lse2.data_ptr(),
                                 delta.data_ptr(), db, db + 2 * H, db + 4 * H, 3 * H, B, nh, L, 0.125, drop, 7, stream_ptr()), "bwd_varlen")
    assert rel_err(dp, dqkv.index_select(0, idx)) < 1e-2


SC = 0.125 * 1.4426950408889634        # softmax scale * log2(e); * 0.125 is exact, so fp32(SC) is the kernels' p.sc


def _prescaled(qkv, H):
    """the q columns as the kernels pre-scale them internally: bf16(fp32(q) * fp32(sc))"""
    out = qkv.clone()
    out[:, :H] = (qkv[:, :H].float() * torch.tensor(SC, dtype=torch.float32, device=qkv.device)).to(torch.bfloat16)
    return out


@pytest.mark.parametrize("B,L,nh,masked,drop", [(2, 20, 1, True, 0.0), (3, 64, 2, False, 0.0), (2, 255, 4, True, 0.1), (2, 510, 4, True, 0.0),
                                                (2, 577, 3, False, 0.0), (9, 193, 2, True, 0.0), (2, 385, 2, False, 0.1)])
def test_attention_prescaled_q_entry_points_are_bit_identical(gpu, B, L, nh, masked, drop):
    """ia_attn_fwd_ps / ia_attn_bwd_bias_ps given q' = bf16(q * scale * log2 e) compute exactly what ia_attn_fwd / ia_attn_bwd_bias
    compute from q (they form the same q' per tile): context, lse, dq, dk, dv and the bias gradient bit for bit, over the forward,
    the dQ + dK/dV pair and the fused backward (33 <= L <= 256)."""
    from item_alignment_amd import ops
    H = nh * 64
    qkv = rnd((B * L, 3 * H), gpu, 1.0, 61)
    dctx = rnd((B * L, H), gpu, 1.0, 62)
    mask = None
    if masked:
        lens = torch.tensor([max(1, L - 5 * (i + 1)) for i in range(B)])
        mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(gpu)
    qs = _prescaled(qkv, H)
    ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=drop, seed=3)
    ctx2, lse2 = ops.attn_fwd(qs, B, L, nh, key_mask=mask, drop_p=drop, seed=3, q_prescaled=True)
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2)
    db1 = torch.zeros(3 * H, device=gpu)
    db2 = torch.zeros(3 * H, device=gpu)
    g1 = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=3, dbias=db1)
    g2 = ops.attn_bwd(qs, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=3, dbias=db2, q_prescaled=True)
    assert torch.equal(g1, g2) and torch.equal(db1, db2)


def test_attention_prescaled_q_packed_rows_are_bit_identical(gpu):
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    nh, lens = 2, [255, 17, 129, 200, 64, 65]
    B, L, H, T = len(lens), max(lens), nh * 64, sum(lens)
    pq = rnd((T, 3 * H), gpu, 1.0, 63)
    pd = rnd((T, H), gpu, 1.0, 64)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=gpu)
    res = []
    for ps, src in ((0, pq), (1, _prescaled(pq, H))):
        out = torch.empty((T, H), device=gpu, dtype=torch.bfloat16)
        lse = torch.zeros((B, nh, L), device=gpu)
        dp = torch.empty_like(pq)
        delta = torch.empty((B, nh, L), device=gpu)
        base, db = src.data_ptr(), dp.data_ptr()
        fwd = lib.ia_attn_fwd_varlen_ps if ps else lib.ia_attn_fwd_varlen
        bwd = lib.ia_attn_bwd_varlen_ps if ps else lib.ia_attn_bwd_varlen
        check(fwd(base, base + 2 * H, base + 4 * H, 3 * H, cu.data_ptr(), T, out.data_ptr(), H, lse.data_ptr(), B, nh, L, 0.125, 0.1, 7,
                  stream_ptr()), "fwd_varlen")
        check(bwd(base, base + 2 * H, base + 4 * H, 3 * H, cu.data_ptr(), T, out.data_ptr(), pd.data_ptr(), H, lse.data_ptr(), delta.data_ptr(),
                  db, db + 2 * H, db + 4 * H, 3 * H, B, nh, L, 0.125, 0.1, 7, stream_ptr()), "bwd_varlen")
        res.append((out, lse, dp))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,H,K", [(510, 128, 128), (1000, 256, 192), (32640, 1024, 1024), (4616, 768, 768), (77, 128, 64)])
def test_gemm_qscale_scales_the_q_columns_only(gpu, M, H, K):
    """ia_gemm_bf16_qscale: columns [0, H) = bf16((x W^T + b) * s), columns [H, 3H) = the plain bias GEMM's, bit for bit"""
    from item_alignment_amd import _lib, ops
    x = rnd((M, K), gpu, 1.0, 71)
    w = rnd((3 * H, K), gpu, K ** -0.5, 72)
    b = rnd((3 * H,), gpu, 1.0, 73).float()
    plain = ops.gemm(x, w, epilogue=ops.EPI_BIAS, bias=b)
    got = ops.gemm_qscale(x, w, b, H, SC)
    assert torch.equal(got[:, H:], plain[:, H:])
    want = (x.float() @ w[:H].float().t() + b[:H]) * SC
    assert rel_err(got[:, :H], want) < 6e-3
    # at most one bf16 ulp from rounding the exact product (fp32 accumulation order differs from torch's)
    assert ((got[:, :H].float() - want).abs() <= want.abs() * 2 ** -7 + 1e-3).all()
    lib = _lib.load()
    for cols in (64, -128, 3 * H + 128):
        rc = lib.ia_gemm_bf16_qscale(x.data_ptr(), K, w.data_ptr(), K, got.data_ptr(), 3 * H, M, 3 * H, K, b.data_ptr(), cols, SC, ops.stream_ptr())
        assert rc == -1, cols


def test_conv3x3_padded_full_size_against_miopen(gpu):
    """The eca_nfnet_l0 stage-1 shape at full resolution (200x200, 64 channels, 4 images) and a stage-3 one (50x50, 6 groups of 64):
    forward and both gradients against torch.conv2d in fp32 on the GPU."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    for B, H, W, groups in ((4, 200, 200, 1), (8, 50, 50, 6)):
        C = 64 * groups
        x, dy = rnd((B, H, W, C), gpu, 1.0, 51), rnd((B, H, W, C), gpu, 1.0, 52)
        w = rnd((C, 64, 3, 3), gpu, 0.05, 53)
        what = w.permute(0, 2, 3, 1).reshape(C, 576).contiguous()
        xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
        wr = w.float().requires_grad_(True)
        ref = torch.nn.functional.conv2d(xr, wr, None, padding=1, groups=groups)
        ref.backward(dy.float().permute(0, 3, 1, 2))
        xp, dyp = _pad_nhwc(x), _pad_nhwc(dy)
        yp, dxp = torch.empty_like(xp), torch.empty_like(xp)
        check(lib.ia_conv3x3_padded_fwd(xp.data_ptr(), what.data_ptr(), None, yp.data_ptr(), B, H, W, C, C, groups, stream_ptr()), "fwd")
        check(lib.ia_conv3x3_padded_bwd_data(dyp.data_ptr(), what.data_ptr(), dxp.data_ptr(), B, H, W, C, C, groups, stream_ptr()), "dgrad")
        wsb = lib.ia_conv3x3_padded_workspace_bytes(B, H, W, C, C, groups)
        ws = torch.empty(max(wsb, 16), device=gpu, dtype=torch.uint8)
        dwhat = torch.empty((C, 576), device=gpu, dtype=torch.float32)
        check(lib.ia_conv3x3_padded_bwd_weight(xp.data_ptr(), dyp.data_ptr(), dwhat.data_ptr(), None, B, H, W, C, C, groups, ws.data_ptr(), wsb,
                                               stream_ptr()), "wgrad")
        assert rel_err(yp[:, 1:-1, 1:-1], ref.permute(0, 2, 3, 1)) < 2e-2
        assert rel_err(dxp[:, 1:-1, 1:-1], xr.grad.permute(0, 2, 3, 1)) < 2e-2
        assert rel_err(dwhat.view(C, 3, 3, 64).permute(0, 3, 1, 2), wr.grad) < 2e-3      # sums over up to 160 000 pixels, fp32 split-K


def test_conv_operands_beyond_2gib(gpu):
    """Operands larger than 2 GiB (more than 32 images of 800x800 in one tower pass): the GEMM addresses them through per-workgroup
    32-bit buffer windows.  Images are independent, so the whole batch must equal the same kernels run on sub-batches (whose
    operands are small and are checked against torch by the tests above); weight / bias gradients must equal the sum over them."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    torch.manual_seed(77)
    # --- shifted-view 3x3 on the zero-bordered domain: 56 x 400 x 400 x 128 bf16 = 2.29 GB per operand
    B, H, W, C, groups = 56, 398, 398, 128, 2
    rows = (H + 2) * (W + 2)
    xp = torch.zeros((B, H + 2, W + 2, C), device=gpu, dtype=torch.bfloat16)
    dyp = torch.zeros_like(xp)
    xp[:, 1:-1, 1:-1] = torch.randn((B, H, W, C), device=gpu).bfloat16()
    dyp[:, 1:-1, 1:-1] = torch.randn((B, H, W, C), device=gpu).bfloat16()
    assert xp.numel() * 2 > 2 ** 31
    what = (torch.randn((C, 9 * C // groups), device=gpu) * 0.05).bfloat16()
    bias = torch.randn(C, device=gpu)

    def run(b0, b1):
        n = b1 - b0
        x_, dy_ = xp[b0:b1], dyp[b0:b1]
        yp, dxp = torch.empty_like(x_), torch.empty_like(x_)
        check(lib.ia_conv3x3_padded_fwd(x_.data_ptr(), what.data_ptr(), bias.data_ptr(), yp.data_ptr(), n, H, W, C, C, groups, stream_ptr()), "fwd")
        check(lib.ia_conv3x3_padded_bwd_data(dy_.data_ptr(), what.data_ptr(), dxp.data_ptr(), n, H, W, C, C, groups, stream_ptr()), "dgrad")
        wsb = lib.ia_conv3x3_padded_workspace_bytes(n, H, W, C, C, groups)
        ws = torch.empty(max(wsb, 16), device=gpu, dtype=torch.uint8)
        dwhat = torch.empty((C, 9 * C // groups), device=gpu, dtype=torch.float32)
        dbias = torch.zeros(C, device=gpu)
        check(lib.ia_conv3x3_padded_bwd_weight(x_.data_ptr(), dy_.data_ptr(), dwhat.data_ptr(), dbias.data_ptr(), n, H, W, C, C, groups,
                                               ws.data_ptr(), wsb, stream_ptr()), "wgrad")
        return yp, dxp, dwhat, dbias

    yp, dxp, dwhat, dbias = run(0, B)
    dw_sum, db_sum = torch.zeros_like(dwhat), torch.zeros_like(dbias)
    for b0 in range(0, B, 14):
        y_, dx_, dw_, db_ = run(b0, b0 + 14)
        assert torch.equal(yp[b0:b0 + 14, 1:-1, 1:-1], y_[:, 1:-1, 1:-1]) and torch.equal(dxp[b0:b0 + 14, 1:-1, 1:-1], dx_[:, 1:-1, 1:-1]), b0
        dw_sum += dw_
        db_sum += db_
    assert rel_err(dwhat, dw_sum) < 1e-4 and rel_err(dbias, db_sum) < 1e-4
    del xp, dyp, yp, dxp
    # --- strided 3x3 through the patch matrix: 48 x 200 x 200 rows x 576 columns bf16 = 2.2 GB
    B, H, W, C, Cout, s = 48, 400, 400, 64, 64, 2
    x = torch.randn((B * H * W, C), device=gpu).bfloat16()
    Ho = Wo = (H - 1) // s + 1
    dy = torch.randn((B * Ho * Wo, Cout), device=gpu).bfloat16()
    what = (torch.randn((Cout, 9 * C), device=gpu) * 0.05).bfloat16()
    assert B * Ho * Wo * 9 * C * 2 > 2 ** 31

    def run2(b0, b1):
        n = b1 - b0
        x_, dy_ = x[b0 * H * W:b1 * H * W], dy[b0 * Ho * Wo:b1 * Ho * Wo]
        wsb = lib.ia_conv_nhwc_workspace_bytes(n, H, W, C, Cout, 3, s, 1)
        ws = torch.empty(max(wsb, 16), device=gpu, dtype=torch.uint8)
        y = torch.empty((n * Ho * Wo, Cout), device=gpu, dtype=torch.bfloat16)
        check(lib.ia_conv_nhwc_fwd(x_.data_ptr(), what.data_ptr(), bias[:Cout].data_ptr(), y.data_ptr(), n, H, W, C, Cout, 3, s, 1, ws.data_ptr(), wsb,
                                   stream_ptr()), "fwd")
        dwhat = torch.empty((Cout, 9 * C), device=gpu, dtype=torch.float32)
        dbias = torch.zeros(Cout, device=gpu)
        check(lib.ia_conv_nhwc_bwd_weight(x_.data_ptr(), dy_.data_ptr(), dwhat.data_ptr(), dbias.data_ptr(), n, H, W, C, Cout, 3, s, 1, 1, ws.data_ptr(),
                                          wsb, stream_ptr()), "wgrad")
        dx = torch.empty_like(x_)
        check(lib.ia_conv_nhwc_bwd_data(dy_.data_ptr(), what.data_ptr(), dx.data_ptr(), n, H, W, C, Cout, 3, s, 1, ws.data_ptr(), wsb, stream_ptr()),
              "dgrad")
        return y, dx, dwhat, dbias

    y, dx, dwhat, dbias = run2(0, B)
    dw_sum, db_sum = torch.zeros_like(dwhat), torch.zeros_like(dbias)
    for b0 in range(0, B, 16):
        y_, dx_, dw_, db_ = run2(b0, b0 + 16)
        assert torch.equal(y[b0 * Ho * Wo:(b0 + 16) * Ho * Wo], y_) and torch.equal(dx[b0 * H * W:(b0 + 16) * H * W], dx_), b0
        dw_sum += dw_
        db_sum += db_
    assert rel_err(dwhat, dw_sum) < 1e-4 and rel_err(dbias, db_sum) < 1e-4


def test_batchnorm_full_size_statistics(gpu):
    """resnetv2_50 stage-1 activation size (2 x 320 000 rows x 256 channels): without the ReLU every (segment, channel) of the
    output has mean beta and variance gamma^2, whatever the input scale and offset; the backward output sums to zero per
    (segment, channel) (the defining properties of BatchNorm in training mode)."""
    from item_alignment_amd import _lib
    from item_alignment_amd.ops import check, stream_ptr
    lib = _lib.load()
    rows, C, seg = 640000, 256, 2
    g = torch.Generator(device="cpu").manual_seed(61)
    x = ((torch.randn((rows, C), generator=g) * 3.0 + 1.5).to(gpu) * torch.linspace(0.1, 4.0, C, device=gpu)).to(torch.bfloat16)
    gamma, beta = torch.linspace(0.5, 1.5, C, device=gpu), torch.linspace(-1, 1, C, device=gpu)
    y = torch.empty_like(x)
    mean, rstd = torch.empty((seg, C), device=gpu), torch.empty((seg, C), device=gpu)
    wsb = lib.ia_bn_act_workspace_bytes(rows, C, seg)
    ws = torch.empty(wsb, device=gpu, dtype=torch.uint8)
    check(lib.ia_bn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C,
                            seg, 1e-5, 0.1, 1, 0, ws.data_ptr(), wsb, stream_ptr()), "bn_fwd")
    yv = y.float().view(seg, rows // seg, C)
    assert (yv.mean(1) - beta).abs().max().item() < 5e-3
    assert (yv.var(1, unbiased=False) / gamma ** 2 - 1).abs().max().item() < 1e-2
    dy = torch.randn((rows, C), generator=g).to(gpu).to(torch.bfloat16)
    dx = torch.empty_like(x)
    check(lib.ia_bn_act_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(),
                            None, None, rows, C, seg, 1, 0, ws.data_ptr(), wsb, stream_ptr()), "bn_bwd")
    s = dx.float().view(seg, rows // seg, C).sum(1)
    assert (s.abs() / (dx.float().abs().view(seg, rows // seg, C).sum(1) + 1e-6)).max().item() < 2e-3


def _sampled_attention_reference(qkv, dctx, B, L, nh, mask, pairs):
    """fp32 softmax attention + its backward for the sampled (sequence, head) pairs only, from the same bf16 inputs"""
    H = nh * 64
    t = qkv.view(B, L, 3, nh, 64)
    b_idx = torch.tensor([p[0] for p in pairs], device=qkv.device)
    h_idx = torch.tensor([p[1] for p in pairs], device=qkv.device)
    sel = t[b_idx, :, :, h_idx].float()                         # [P, L, 3, 64]
    sel.requires_grad_(True)
    q, k, v = sel[:, :, 0], sel[:, :, 1], sel[:, :, 2]
    s = q @ k.transpose(-1, -2) * 0.125
    if mask is not None:
        s = s + (1.0 - mask[b_idx].float())[:, None, :] * torch.finfo(torch.float32).min
    o = torch.softmax(s, -1) @ v                                # [P, L, 64]
    do = dctx.view(B, L, nh, 64)[b_idx, :, h_idx].float()
    o.backward(do)
    return o.detach(), sel.grad                                 # [P, L, 64], [P, L, 3, 64]


@pytest.mark.parametrize("B,L,nh,masked", [(512, 577, 12, False), (512, 255, 16, True), (128, 385, 12, False), (128, 193, 12, True),
                                           (128, 510, 16, True)])        # the last: a C2 batch (roberta_large one_tower, L = 2 x 255)
def test_attention_bench_shapes_whole_output_scan(gpu, B, L, nh, masked):
    """The attention kernels AT THE BENCH SHAPES (512 images x 577 tokens x 12 heads, 512 sequences x 255 x 16 heads with the padding
    mask) and at the two shapes whose ragged last key tile once faulted (385, 193): 20 launches on fresh random data, every element
    of ctx and dqkv scanned for non-finite or absurd values (round 3's dQ fault produced one bad row per few thousand (sequence,
    head) pairs at these sizes only), and 64 sampled (sequence, head) pairs per launch compared element-wise with the fp32 softmax
    attention and its backward (dQ, dK, dV)."""
    from item_alignment_amd import ops
    H = nh * 64
    g = torch.Generator(device=gpu)
    worst = {"o": 0.0, "dq": 0.0, "dk": 0.0, "dv": 0.0}
    for it in range(20):
        g.manual_seed(1000 + it)
        qkv = (torch.randn((B * L, 3 * H), device=gpu, generator=g) * (1.0 + 0.5 * (it % 3))).to(torch.bfloat16)
        dctx = torch.randn((B * L, H), device=gpu, generator=g).to(torch.bfloat16)
        mask = None
        if masked:
            lens = torch.randint(1, L + 1, (B,), device=gpu, generator=g)
            mask = (torch.arange(L, device=gpu)[None, :] < lens[:, None]).to(torch.uint8)
        ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask)
        dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask)
        for name, t_ in (("ctx", ctx), ("dqkv", dqkv), ("lse", lse)):
            assert torch.isfinite(t_).all().item(), (name, it)
        # |ctx| <= max |v|; |dqkv| is bounded by L * max|dO| * max|operand| far below 1e4 on unit-variance data
        assert ctx.float().abs().max().item() <= qkv[:, 2 * H:].float().abs().max().item() * (1 + 2 ** -6), it
        assert dqkv.float().abs().max().item() < 1e4, (it, dqkv.float().abs().max().item())
        if it % 4 == 0:
            pr = torch.randint(0, B * nh, (64,), device="cpu", generator=torch.Generator().manual_seed(it)).tolist()
            pairs = [(p // nh, p % nh) for p in pr]
            o_ref, d_ref = _sampled_attention_reference(qkv, dctx, B, L, nh, mask, pairs)
            b_idx = torch.tensor([p[0] for p in pairs], device=gpu)
            h_idx = torch.tensor([p[1] for p in pairs], device=gpu)
            o_got = ctx.view(B, L, nh, 64)[b_idx, :, h_idx].float()
            d_got = dqkv.view(B, L, 3, nh, 64)[b_idx, :, :, h_idx].float()
            worst["o"] = max(worst["o"], rel_err(o_got, o_ref))
            for i, name in enumerate(("dq", "dk", "dv")):
                worst[name] = max(worst[name], rel_err(d_got[:, :, i], d_ref[:, :, i]))
        del qkv, dctx, ctx, dqkv, lse
    assert worst["o"] < 2e-2 and max(worst["dq"], worst["dk"], worst["dv"]) < 3e-2, worst


@pytest.mark.parametrize("B,L,nh,drop", [(128, 193, 12, 0.0), (256, 255, 16, 0.1)])
def test_attention_backward_first_launch_equals_repeats(gpu, B, L, nh, drop):
    """The backward launched right behind the forward (lse and the context still on their way out of the writer's L2: the first item
    of every persistent workgroup waits for its pieces, each wave for its own) must equal the same launch repeated, bit for bit.
    Round 4's fused kernel failed this one launch in four at 128 x 193 x 12: the lse piece's out-of-range lanes zeroed the delta
    another wave had already written (40 fresh inputs: a 25 % fault has 1e-5 left to slip through)."""
    from item_alignment_amd import ops
    H = nh * 64
    g = torch.Generator(device=gpu)
    for it in range(40):
        g.manual_seed(1000 + it)
        qkv = (torch.randn((B * L, 3 * H), device=gpu, generator=g) * (1.0 + 0.5 * (it % 3))).to(torch.bfloat16)
        dctx = torch.randn((B * L, H), device=gpu, generator=g).to(torch.bfloat16)
        lens = torch.randint(1, L + 1, (B,), device=gpu, generator=g)
        mask = (torch.arange(L, device=gpu)[None, :] < lens[:, None]).to(torch.uint8)
        ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=drop, seed=it)
        outs = [ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=drop, seed=it) for _ in range(3)]
        assert torch.equal(outs[1], outs[2]), it
        assert torch.equal(outs[0], outs[1]), (it, int((outs[0] != outs[1]).sum()))
        del qkv, dctx, ctx, lse, outs


@pytest.mark.parametrize("B,L,nh", [(512, 255, 16), (128, 577, 12)])
def test_attention_bench_shapes_with_dropout_stay_finite(gpu, B, L, nh):
    """the text tower's configuration (attention dropout 0.1) at full size: whole outputs finite and bounded over 10 seeds"""
    from item_alignment_amd import ops
    H = nh * 64
    g = torch.Generator(device=gpu)
    for it in range(10):
        g.manual_seed(2000 + it)
        qkv = torch.randn((B * L, 3 * H), device=gpu, generator=g).to(torch.bfloat16)
        dctx = torch.randn((B * L, H), device=gpu, generator=g).to(torch.bfloat16)
        lens = torch.randint(1, L + 1, (B,), device=gpu, generator=g)
        mask = (torch.arange(L, device=gpu)[None, :] < lens[:, None]).to(torch.uint8)
        ctx, lse = ops.attn_fwd(qkv, B, L, nh, key_mask=mask, drop_p=0.1, seed=it + 1)
        dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, B, L, nh, key_mask=mask, drop_p=0.1, seed=it + 1)
        assert torch.isfinite(ctx).all().item() and torch.isfinite(dqkv).all().item() and torch.isfinite(lse).all().item(), it
        assert dqkv.float().abs().max().item() < 1e4 and ctx.float().abs().max().item() < 1e2, it


@pytest.mark.parametrize("B,N,K,act", [(200, 100, 72, 1), (512, 1024, 768, 0), (64, 8, 130, 1), (3, 40, 24, 1)])
def test_linear_small_tiled_and_per_output_paths(gpu, B, N, K, act):
    """ia_linear_small_fwd / bwd (fp32 heads; reference base.py:139-157, 530): the tiled kernels that take over from 64 rows up (the
    image-CLS projection sees one row per image) and the one-output-per-thread kernels below that, against torch fp32 autograd;
    dW / db accumulate."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * 7 + N)
    x = torch.randn((B, K), generator=g).to(gpu)
    W = (torch.randn((N, K), generator=g) * 0.1).to(gpu)
    b = (torch.randn((N,), generator=g) * 0.1).to(gpu)
    dy = torch.randn((B, N), generator=g).to(gpu)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((B, N), device=gpu)
    _lib.check(lib.ia_linear_small_fwd(x.data_ptr(), K, W.data_ptr(), b.data_ptr(), y.data_ptr(), B, N, K, act, st), "fwd")
    xr, Wr, br = x.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = xr @ Wr.t() + br
    yr = torch.tanh(pre) if act else pre
    assert rel_err(y, yr.detach()) < 1e-5
    yr.backward(dy)
    dx = torch.empty_like(x)
    dW = torch.full_like(W, 0.5)
    db = torch.full_like(b, 0.25)
    _lib.check(lib.ia_linear_small_bwd(dy.data_ptr(), y.data_ptr(), x.data_ptr(), K, W.data_ptr(), dx.data_ptr(), K, dW.data_ptr(), db.data_ptr(),
                                       B, N, K, act, st), "bwd")
    torch.cuda.synchronize()
    assert rel_err(dx, xr.grad) < 1e-4
    assert rel_err(dW - 0.5, Wr.grad) < 1e-4
    assert rel_err(db - 0.25, br.grad) < 1e-4


def test_gemm_dynamic_tile_claim_under_cu_contention(gpu):
    """The large persistent GEMM launches hand their tiles out through per-XCD claim counters (gemm.hip, t256w::gemm_kernel): whatever
    the claim order -- alone, next to a kernel that holds 24 whole CUs on another stream (ia_debug_cu_hog: workgroups that start late find
    no work left), from two streams at once, and after the counter slots have come round (> 1024 launches) -- every tile is computed exactly
    once: outputs bit-identical to the undisturbed launch, and equal to the fp32 reference within the bf16 bar."""
    import time
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    prev = lib.ia_debug_gemm_dynamic(0)             # the undisturbed static order first
    M, N, K = 5000, 4096, 512                       # 20 x 16 = 320 tiles (one clipped row of tiles): more than one per workgroup
    a, b = rnd((M, K), gpu, 1.0, 71), rnd((N, K), gpu, 0.05, 72)
    bias = torch.linspace(-1, 1, N, device=gpu)
    ref = a.float() @ b.float().t() + bias
    base = ops.gemm(a, b, epilogue=ops.EPI_BIAS, bias=bias).clone()
    assert rel_err(base, ref) < 2e-2
    a2, b2 = rnd((4352, 64), gpu, 1.0, 73), rnd((4096, 64), gpu, 0.1, 74)       # 17 x 16 = 272 tiles, one k-tile each
    first = ops.gemm(a2, b2).clone()
    w = rnd((K, N), gpu, 0.05, 75)
    d0 = ops.gemm(a, w, b_kstrided=True).clone()
    torch.cuda.synchronize()
    lib.ia_debug_gemm_dynamic(1)
    assert torch.equal(ops.gemm(a, b, epilogue=ops.EPI_BIAS, bias=bias), base)
    side = torch.cuda.Stream()
    for hog in (8, 24):
        torch.cuda.synchronize()
        _lib.check(lib.ia_debug_cu_hog(hog, 20.0, side.cuda_stream), "ia_debug_cu_hog")
        time.sleep(0.003)
        outs = [ops.gemm(a, b, epilogue=ops.EPI_BIAS, bias=bias) for _ in range(6)]
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, base), hog
    # two streams launching the same shape concurrently (each launch has its own counter slot)
    outs = []
    for i in range(8):
        with torch.cuda.stream(side if i & 1 else torch.cuda.current_stream()):
            outs.append(ops.gemm(a, b, epilogue=ops.EPI_BIAS, bias=bias))
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, base)
    # slot reuse: more launches than counter slots, the last ones still exact (a slot left non-zero would skip tiles)
    out2 = torch.empty_like(first)
    for _ in range(1100):
        ops.gemm(a2, b2, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(out2, first)
    assert rel_err(first, a2.float() @ b2.float().t()) < 2e-2
    # the data-gradient and GELU forms go through the same loop
    _lib.check(lib.ia_debug_cu_hog(16, 10.0, side.cuda_stream), "ia_debug_cu_hog")
    time.sleep(0.003)
    d1 = ops.gemm(a, w, b_kstrided=True)
    torch.cuda.synchronize()
    lib.ia_debug_gemm_dynamic(prev)
    assert torch.equal(d0, d1) and rel_err(d0, a.float() @ w.float()) < 2e-2


def test_embed_ln_bwd_tables_across_pieces_match_an_independent_sum(gpu):
    """ia_embed_ln_bwd's table gradients (embed.hip: rows summed along a stable sort of the rows by table row, in pieces of 512 sorted
    positions; a run that crosses pieces is joined by the piece it starts in).  Here one word id covers ~1500 rows (a run over 3-4
    pieces), token type 0 covers nearly all 2800 rows (every piece), positions make runs of 70 rows, and padding rows add to no word /
    position row.  Against an fp64 index_add of the LayerNorm input gradient, and a second call must repeat the first bit for bit."""
    from item_alignment_amd import _lib
    from item_alignment_amd.models.functional import embed_table_orders
    lib = _lib.load()
    S, L, H, V, P, T, word_pad, pos_pad = 70, 40, 256, 300, 48, 2, 1, 1
    M = S * L
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(2, V, (S, L), generator=gen)
    ids.view(-1)[:1500] = 7
    ids.view(-1)[torch.randperm(M, generator=gen)[:200]] = word_pad
    pids = (torch.arange(L) + 2).repeat(S, 1)
    pids[ids == word_pad] = pos_pad
    tts = torch.zeros(S, L, dtype=torch.long)
    tts.view(-1)[torch.randperm(M, generator=gen)[:100]] = 1
    z = (torch.randn(M, H, generator=gen) * 2 + 0.5).to(torch.bfloat16)
    dy = torch.randn(M, H, generator=gen).to(torch.bfloat16)
    gamma = torch.rand(H, generator=gen) + 0.5
    zf = z.double()
    mean, var = zf.mean(1), zf.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    # reference: LayerNorm input gradient per row in fp64, scattered with index_add
    xhat = (zf - mean[:, None]) * rstd[:, None]
    gg = dy.double() * gamma.double()
    o = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xhat * (gg * xhat).mean(1, keepdim=True))
    fi, fp, ft = ids.view(-1), pids.view(-1), tts.view(-1)
    w_ok, p_ok = fi != word_pad, fp != pos_pad
    want = {"word": torch.zeros(V, H, dtype=torch.float64).index_add_(0, fi[w_ok], o[w_ok]),
            "pos": torch.zeros(P, H, dtype=torch.float64).index_add_(0, fp[p_ok], o[p_ok]),
            "type": torch.zeros(T, H, dtype=torch.float64).index_add_(0, ft, o)}

    dev = {k: v.to(gpu) for k, v in dict(ids=ids, pids=pids, tts=tts, z=z, dy=dy, gamma=gamma, mean=mean.float(), rstd=rstd.float()).items()}
    orders = embed_table_orders(dev["ids"], dev["tts"], dev["pids"], None, word_pad, pos_pad)
    ws_bytes = lib.ia_embed_ln_bwd_workspace_bytes(M, H)
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)

    def run():
        got = {"word": torch.zeros(V, H, device=gpu), "pos": torch.zeros(P, H, device=gpu), "type": torch.zeros(T, H, device=gpu)}
        dg, db = torch.zeros(H, device=gpu), torch.zeros(H, device=gpu)
        _lib.check(lib.ia_embed_ln_bwd(dev["dy"].data_ptr(), dev["z"].data_ptr(), dev["mean"].data_ptr(), dev["rstd"].data_ptr(),
                                       dev["gamma"].data_ptr(), dev["ids"].data_ptr(), dev["tts"].data_ptr(), dev["pids"].data_ptr(), None, None,
                                       *(t.data_ptr() for t in orders), got["word"].data_ptr(), got["type"].data_ptr(), got["pos"].data_ptr(),
                                       None, dg.data_ptr(), db.data_ptr(), M, H, L, word_pad, pos_pad, 0.0, 0, 0, ws.data_ptr(), ws_bytes,
                                       _lib.stream_ptr()), "ia_embed_ln_bwd")
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in got.items()}

    g1, g2 = run(), run()
    for k in want:
        assert torch.equal(g1[k], g2[k]), ("a second call must repeat the table gradient bit for bit", k)
        assert rel_err(g1[k], want[k]) < 1e-5, (k, rel_err(g1[k], want[k]))
    assert want["word"][7].abs().max() > 0 and g1["word"][word_pad].abs().max() == 0 and g1["pos"][pos_pad].abs().max() == 0
