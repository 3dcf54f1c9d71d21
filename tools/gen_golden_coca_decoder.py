"""Writes tests/golden/coca/decoder_block.npz from the reference's own decoder block.

    python tools/gen_golden_coca_decoder.py <reference checkout>

The reference's src/models/multimodal.py classes ParallelTransformerBlock and Residual are imported under the stub recipe of SURVEY.md
Appendix B (oracle/ref_harness.py) and run as they are: Residual(ParallelTransformerBlock(dim=128, dim_head=64, heads=2, ff_mult=1,
is_decoding=True)) -- the decoder layer of CoCa pre-training -- in fp32 on the CPU, B = 2 sequences of n = 5 and n = 70 tokens (one
32-key block; more than one 64-key tile), seeded inputs and weights.  Per n: the input x [B, n, 128], the cotangent dy, the output
and the gradients of x, norm.gamma, fused_attn_ff_proj.weight, attn_out.weight and ff_out.1.weight of loss = sum(out * dy); the same
block with is_decoding=False on the same weights is stored beside it (out_nc.<n>), so a test can see that the flag matters.  Inputs and
the cotangent and the weights are bf16-representable (what the engine's bf16 activations and weight shadows hold exactly).  To keep the
file under the size limit of a committed file, outputs and gradients are stored as fp32 rounded to 11 significant bits (relative
2^-11, a hundredth of the 5e-2 the test allows): their low 13 mantissa bits are zero and deflate removes them.  The file is
byte-reproducible.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "coca")
DIM, HEADS, FF_MULT, B, NS = 128, 2, 1, 2, (5, 70)
GRADS = ("fn.norm.gamma", "fn.fused_attn_ff_proj.weight", "fn.attn_out.weight", "fn.ff_out.1.weight")


def write_npz(path, arrays):
    """np.savez with a fixed timestamp per member (zipfile stamps the current time otherwise)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def short(t):
    """fp32 rounded to nearest at 11 significant bits (low 13 mantissa bits zero)"""
    a = np.ascontiguousarray(t.detach().numpy(), dtype=np.float32).view(np.uint32).astype(np.uint64)
    a = ((a + 0x0FFF + ((a >> 13) & 1)) >> 13) << 13
    return a.astype(np.uint32).view(np.float32)


def main(reference):
    sys.path.insert(0, ROOT)
    from oracle import ref_harness
    ref_harness.REFERENCE_ROOT = reference
    ref_harness.load_reference()
    import src.models.multimodal as MM

    torch.use_deterministic_algorithms(True)
    torch.manual_seed(20221101)
    block = MM.Residual(MM.ParallelTransformerBlock(dim=DIM, dim_head=64, heads=HEADS, ff_mult=FF_MULT, is_decoding=True)).eval()
    plain = MM.Residual(MM.ParallelTransformerBlock(dim=DIM, dim_head=64, heads=HEADS, ff_mult=FF_MULT, is_decoding=False)).eval()
    with torch.no_grad():
        block.fn.norm.gamma.copy_((1.0 + 0.1 * torch.randn(DIM)).bfloat16().float())
        for lin in (block.fn.fused_attn_ff_proj, block.fn.attn_out, block.fn.ff_out[1]):
            lin.weight.copy_((torch.randn_like(lin.weight) / lin.weight.shape[1] ** 0.5).bfloat16().float())
    plain.load_state_dict(block.state_dict())
    assert sorted(block.state_dict()) == sorted(plain.state_dict()), "the mask / pos_emb caches must not be persistent"
    arrays = {"dim": np.int64(DIM), "heads": np.int64(HEADS), "ff_mult": np.int64(FF_MULT), "ns": np.asarray(NS, np.int64)}
    for k, v in block.state_dict().items():
        arrays["w." + k] = v.detach().numpy().copy()
    for n in NS:
        x = torch.randn(B, n, DIM).bfloat16().float().requires_grad_(True)
        dy = torch.randn(B, n, DIM).bfloat16().float()
        block.zero_grad()
        out = block(x)
        (out * dy).sum().backward()
        arrays[f"x.{n}"], arrays[f"dy.{n}"] = x.detach().numpy().copy(), dy.numpy().copy()
        arrays[f"out.{n}"], arrays[f"grad.x.{n}"] = short(out), short(x.grad)
        params = dict(block.named_parameters())
        for k in GRADS:
            arrays[f"grad.{k}.{n}"] = short(params[k].grad)
        with torch.no_grad():
            arrays[f"out_nc.{n}"] = short(plain(x))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "decoder_block.npz")
    write_npz(path, arrays)
    print("wrote", path, os.path.getsize(path), "bytes", sorted(arrays))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
