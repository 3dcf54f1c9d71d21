"""Residual(ParallelTransformerBlock(dim=128, dim_head=64, heads=2, ff_mult=1, is_decoding=True)) -- the decoder layer of CoCa
pre-training -- against tests/golden/coca/decoder_block.npz, captured from the reference's own classes in fp32
(tools/gen_golden_coca_decoder.py).  Tolerances are those test_coca_cross_attn (tests/test_models_gpu.py) holds the non-causal block
to: outputs and gradients within 5e-2 of the tensor's largest magnitude, gradient direction cosine above 0.99 -- the same GEMM /
LayerNorm / rotary path with one kernel swapped."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-2               # tests/test_models_gpu.py: TOL
GRAD_REL = 5e-2          # tests/test_models_gpu.py: GRAD_REL
COS_MIN = 0.99           # tests/test_models_gpu.py: COS_MIN
BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coca", "decoder_block.npz")
GRADS = ("fn.norm.gamma", "fn.fused_attn_ff_proj.weight", "fn.attn_out.weight", "fn.ff_out.1.weight")


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def cosine(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return (torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)).item()


@pytest.fixture(scope="module")
def case():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def build(case, is_decoding):
    """the block inside a top-level module that owns the parameter arena, loaded with the golden weights (strict: the state-dict keys
    of a decoding block are those of the reference, which keeps its mask / pos_emb caches out of the state dict)"""
    import item_alignment_amd.models as M
    from item_alignment_amd.models.base import HipModule

    class Host(HipModule):
        def __init__(self):
            super().__init__()
            self.layer = M.Residual(M.ParallelTransformerBlock(dim=int(case["dim"]), dim_head=64, heads=int(case["heads"]),
                                                               ff_mult=int(case["ff_mult"]), is_decoding=is_decoding))

        def forward(self, x2d, B, n):
            self.ensure_arena()
            return self.layer(x2d, B, n)

    host = Host()
    host.load_state_dict({"layer." + k[2:]: v for k, v in case.items() if k.startswith("w.")}, strict=True)
    return host.cuda().eval()


@pytest.fixture(scope="module")
def blocks(gpu, case):
    return build(case, True), build(case, False)


@pytest.mark.parametrize("n", [5, 70])
def test_decoder_block_against_the_reference(blocks, case, n):
    dec, _ = blocks
    B, dim = 2, int(case["dim"])
    x = case[f"x.{n}"].reshape(B * n, dim).to(BF16).cuda().requires_grad_(True)
    dy = case[f"dy.{n}"].reshape(B * n, dim).to(BF16).cuda()
    out = dec(x, B, n)
    r = rel(out.detach().reshape(B, n, dim), case[f"out.{n}"])
    print(f"[decoder n={n}] out rel {r:.4f}")
    assert r < TOL, ("out", r)
    dec.param_arena.zero_grad()
    out.backward(dy)
    torch.cuda.synchronize()
    params = dict(dec.named_parameters())
    pairs = [("x", x.grad.reshape(B, n, dim), case[f"grad.x.{n}"])]
    pairs += [(k, params["layer." + k].grad, case[f"grad.{k}.{n}"]) for k in GRADS]
    for k, got, want in pairs:
        assert got is not None and torch.isfinite(got).all(), k
        c, r = cosine(got, want), rel(got, want)
        print(f"[decoder n={n}] grad {k}: cosine {c:.5f} rel {r:.4f}")
        assert c > COS_MIN, (k, "cosine", c)
        assert r <= GRAD_REL, (k, "rel", r)


@pytest.mark.parametrize("n", [5, 70])
def test_the_flag_matters_and_the_plain_block_is_unchanged(blocks, case, n):
    """is_decoding=False on the same weights and input: differs from the decoding block, matches the reference's non-causal block, and is
    bit for bit what the block computed before the flag existed (its forward restated here on AttentionXFn)."""
    from item_alignment_amd.models import functional as Fn
    dec, plain = blocks
    B, dim = 2, int(case["dim"])
    x = case[f"x.{n}"].reshape(B * n, dim).to(BF16).cuda()
    with torch.no_grad():
        y_dec, y_plain = dec(x, B, n), plain(x, B, n)
        blk = plain.layer.fn
        h = blk.heads
        xn = blk.norm(x)
        fused = Fn.LinearBf16Fn.apply(xn, None, blk.fused_attn_ff_proj.weight, blk)
        q, kv, s = Fn.FusedSplitFn.apply(fused, n, h, blk.ff_inner_dim)
        o = Fn.AttentionXFn.apply(q.view(B * n * h, 64), kv, B, 1, n * h, n, blk.scale)
        y = Fn.LinearBf16Fn.apply(o.view(B * n, h * 64), x, blk.attn_out.weight, blk)
        before = Fn.LinearBf16Fn.apply(s, y, blk.ff_out[1].weight, blk, (fused, h * 64 + 128, blk.ff_inner_dim))
    assert torch.equal(y_plain.view(torch.int16), before.view(torch.int16))
    assert rel(y_plain.reshape(B, n, dim), case[f"out_nc.{n}"]) < TOL
    # token 0 of a decoding block sees itself alone; the plain block lets it see the whole sequence
    assert rel(y_dec.reshape(B, n, dim), case[f"out_nc.{n}"]) > TOL
    assert not torch.equal(y_dec, y_plain)
    # the last token sees every key either way: its attention output is the same in exact arithmetic
    last = torch.arange(B) * n + n - 1
    assert rel(y_dec[last.cuda()], y_plain[last.cuda()]) < TOL
