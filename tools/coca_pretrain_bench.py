"""Times one CoCa pre-training step on one GPU at the reference's shape: src/config/coca_base.json (12 + 12 layers, hidden 768, vocabulary
21 128) with ViT-B/16 at 384 x 384, batch 64, n = 255 text positions (256 tokens, next-token shift), synthetic tokens whose lengths give
a realistic pad share.

    python tools/coca_pretrain_bench.py [--batch 64 --positions 255 --steps 10 --warmup 3 --out profiles/coca_pretrain_bench.json]

What is timed (medians of the timed repeats after the warm-up, events on the stream):
  * the train step: forward, backward, fused AdamW;
  * the caption head alone, forward + backward, on a fixed hidden state (TiedCaptionHeadFn on the rows whose label is not pad);
  * the contrastive loss alone, forward + backward, on fixed embeddings (ContrastiveLossFn: csrc/contrastive.hip);
  * the same step with both losses composed from torch ops on the same towers and layers: dense all-rows fp32 logits [B n, V] through
    the same decoder GEMMs + F.cross_entropy(ignore_index=pad), and F.cross_entropy on a torch sim.  That step is the baseline, because
    there is no earlier CoCa pre-training step to compare with.
Recorded, not gated.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class AllRowsLogitsFn(torch.autograd.Function):
    """to_logits for every position, differentiable: what the reference materialises ([B n, V] fp32; its loss is torch's, outside)"""

    @staticmethod
    def forward(ctx, hidden, model):
        from item_alignment_amd import ops
        norm, table = model.to_logits[0], model.to_logits[1].weight
        x = hidden.contiguous()
        y, _, mean, rstd = ops.ln_fwd(x, norm.gamma, norm.beta, 1e-5, write_z=False)
        ctx.model, ctx.saved = model, (x, y, mean, rstd)
        return ops.gemm(y, model.arena.shadow_of(table), out_f32=True)

    @staticmethod
    def backward(ctx, dlogits):
        from item_alignment_amd import ops
        model = ctx.model
        norm, table = model.to_logits[0], model.to_logits[1].weight
        x, y, mean, rstd = ctx.saved
        dlogits = dlogits.to(torch.bfloat16)
        dy = ops.gemm(dlogits, model.arena.shadow_of(table), b_kstrided=True)
        ops.gemm(dlogits, y, a_kstrided=True, b_kstrided=True, out=table.grad, out_f32=True, accumulate=True)
        dx, _ = ops.ln_bwd(dy, x, mean, rstd, norm.gamma, dgamma=norm.gamma.grad)
        return dx, None


def timed(fn, steps, warmup):
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return dict(median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], repeats=steps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--positions", type=int, default=255, help="n: text positions the model sees (the items hold n + 1 tokens)")
    ap.add_argument("--image-size", type=int, default=384)
    ap.add_argument("--config", default=os.path.join(ROOT, "src", "config", "coca_base.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "coca_pretrain_bench.py needs the GPU"
    import item_alignment_amd.models as M
    from item_alignment_amd.cli_common import load_config
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.models.bert_pretrain import TiedCaptionHeadFn

    dev = torch.device("cuda:0")
    cfg = load_config(a.config, image_size=a.image_size, caption_loss_weight=1.0, contrastive_loss_weight=1.0)
    B, L = a.batch, a.positions + 1
    V, H = cfg.vocab_size, cfg.hidden_size
    g = torch.Generator().manual_seed(a.seed)
    # title + attributes of a product: 150 +- 60 tokens, at least 16, cut at the maximum length
    lens = (torch.randn(B, generator=g) * 60 + 150).round().clamp(16, L).long()
    ids = torch.randint(1000, V, (B, L), generator=g)
    mask = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).long()
    ids = ids * mask
    ids[:, 0] = 1
    batch = [t.to(dev) for t in (ids, mask, torch.zeros_like(ids), torch.arange(L).unsqueeze(0).expand(B, L).contiguous())]
    images = torch.randn((B, 3, a.image_size, a.image_size), generator=g).to(dev)
    torch.manual_seed(a.seed)
    vit = M.VisionTransformer(img_size=a.image_size, patch_size=getattr(cfg, "patch_size", 16), embed_dim=H, depth=cfg.num_hidden_layers,
                              num_heads=cfg.num_attention_heads)
    model = M.CoCaForPretraining(cfg, image_encoder=vit, text_encoder=M.RobertaModel(cfg)).to(dev).train()
    arena = model.param_arena
    cut = [t[:, :-1].contiguous() for t in batch]
    labels = batch[0][:, 1:].contiguous()
    flat = labels.reshape(-1)
    rows = (flat != 0).nonzero(as_tuple=False).squeeze(1)
    live_labels = flat.index_select(0, rows).contiguous()
    m_live, n = rows.numel(), a.positions

    def torch_losses():
        model.ensure_arena()                     # the bf16 shadows follow the optimiser step, as at the top of forward
        x, t_cls, i_cls = model.encode(*cut, images)
        caption = F.cross_entropy(AllRowsLogitsFn.apply(x, model), flat, ignore_index=0)
        sim = t_cls @ i_cls.t() * model.temperature.exp()
        target = torch.arange(B, device=dev)
        return caption + 0.5 * (F.cross_entropy(sim, target) + F.cross_entropy(sim.t(), target))

    def step(loss_fn):
        def run(i):
            Fn.set_step_seed(1000 + i)
            Fn.reset_use_counts()
            arena.zero_grad()
            loss_fn().backward()
            arena.adamw_step(1e-5, betas=(0.9, 0.98), eps=1e-8, weight_decay=1e-5)
        return run

    res = dict(gpu=torch.cuda.get_device_name(0), batch=B, positions=n, image_size=a.image_size, hidden=H, vocab=V,
               text_layers=cfg.num_hidden_layers, multimodal_layers=cfg.num_hidden_layers_multimodal, m_live=m_live,
               live_fraction=m_live / (B * n), logits_bytes_live=m_live * V * 6, logits_bytes_all_rows=B * n * V * 6)
    res["step"] = timed(step(lambda: model(*batch, images=images)), a.steps, a.warmup)
    res["step_torch_losses"] = timed(step(torch_losses), a.steps, a.warmup)
    res["step_torch_losses_over_step"] = res["step_torch_losses"]["median_ms"] / res["step"]["median_ms"]

    hidden = (torch.randn((B * n, H), device=dev) * 0.5).to(torch.bfloat16).requires_grad_(True)
    table = model.to_logits[1].weight
    res["caption_head"] = timed(lambda i: TiedCaptionHeadFn.apply(hidden, model, model.to_logits[0], table, rows, live_labels).backward(),
                                a.kernel_repeats, a.warmup)
    res["caption_head_all_rows_torch"] = timed(lambda i: F.cross_entropy(AllRowsLogitsFn.apply(hidden, model), flat, ignore_index=0).backward(),
                                               a.steps, a.warmup)
    text = torch.randn((B, H), device=dev).requires_grad_(True)
    image = torch.randn((B, H), device=dev).requires_grad_(True)

    def torch_contrastive(i):
        sim = text @ image.t() * model.temperature.exp()
        target = torch.arange(B, device=dev)
        (0.5 * (F.cross_entropy(sim, target) + F.cross_entropy(sim.t(), target))).backward()

    res["contrastive"] = timed(lambda i: Fn.ContrastiveLossFn.apply(text, image, model.temperature).backward(), a.kernel_repeats, a.warmup)
    res["contrastive_torch"] = timed(torch_contrastive, a.kernel_repeats, a.warmup)
    res["caption_head_share_of_step"] = res["caption_head"]["median_ms"] / res["step"]["median_ms"]
    res["contrastive_share_of_step"] = res["contrastive"]["median_ms"] / res["step"]["median_ms"]

    print(f"B {B} x n {n}, {m_live} live rows ({100 * res['live_fraction']:.1f} %): step {res['step']['median_ms']:.1f} ms (torch losses "
          f"{res['step_torch_losses']['median_ms']:.1f} ms, x{res['step_torch_losses_over_step']:.3f}); caption head "
          f"{res['caption_head']['median_ms']:.2f} ms = {100 * res['caption_head_share_of_step']:.1f} % of the step (all rows through torch "
          f"{res['caption_head_all_rows_torch']['median_ms']:.1f} ms); contrastive {res['contrastive']['median_ms'] * 1e3:.0f} us = "
          f"{100 * res['contrastive_share_of_step']:.3f} % (torch {res['contrastive_torch']['median_ms'] * 1e3:.0f} us)", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
