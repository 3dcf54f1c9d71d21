"""Times BERT masked-LM + next-sentence pre-training on one GPU at the reference's shape: bert-base (12 layers, hidden 768, vocabulary
21 128), batch 32, 512 positions, synthetic features with the label density of the example builder (item_alignment_amd/data/bert_pretrain.py
run on synthetic records).

    python tools/bert_pretrain_bench.py [--batch 32 --max-seq-len 510 --steps 10 --warmup 3 --out profiles/bert_pretrain_bench.json]

What is timed (medians of the timed repeats after the warm-up, events on the stream):
  * the train step: forward, backward, gradient norm, fused AdamW;
  * the masked-LM head alone, forward + backward (transform, decoder, loss) on a fixed last hidden state;
  * ia_vocab_ce_fwd and ia_vocab_ce_bwd alone, with their achieved bytes/s against M V 4 and M V (4 + 2) bytes;
  * for comparison, the same step and the same head with the head run on all B L rows, which is what the reference computes: dense
    prediction_scores [B L, V] fp32 through the same GEMMs, torch's cross_entropy(ignore_index=-1) and its autograd on them, the
    gradient cast to bf16 for the same backward GEMMs.
Recorded, not gated: there is no earlier figure to compare with.

    python tools/bert_pretrain_bench.py --world 8 [--batch 32 ...] --out profiles/bert_pretrain_bench.json

times only the train step, as bert_pretrain.py takes it under a launcher: once in one process and once on 8 data-parallel ranks that
share the same global batch, every rank a fresh child process (tools/dp_bench.py).  The two figures are merged into the profile under
"data_parallel"; a box with fewer GPUs than ranks records that the 8-rank figure is unmeasured.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHARS = [chr(c) for c in range(0x4E00, 0x4E00 + 3000)]


class _Tokenizer:
    """one token per character, ids inside the bert-base-chinese table"""

    def __init__(self, size=21128):
        self.size = size
        self.vocab = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, ":": 131, ";": 132}
        self.vocab.update({c: 1000 + i for i, c in enumerate(CHARS)})

    def __len__(self):
        return self.size

    def tokenize(self, text):
        return [c for c in text if not c.isspace()]

    def convert_tokens_to_ids(self, tokens):
        return [self.vocab.get(t, 100) for t in tokens]


def synthetic_records(n, seed):
    import random
    r = random.Random(seed)
    word = lambda a, b: "".join(r.choice(CHARS) for _ in range(r.randint(a, b)))
    out = []
    for _ in range(n):
        props = [(word(2, 4), word(2, 6)) for _ in range(r.randint(8, 40))]
        title = word(10, 30) + "".join(v for _, v in r.sample(props, 2))
        out.append({"industry_name": word(2, 4), "cate_name": word(2, 5), "cate_name_path": word(6, 12), "title": title,
                    "item_pvs": ";".join(f"{k}:{v}" for k, v in props)})
    return out


def config():
    return SimpleNamespace(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=21128,
                           max_position_embeddings=512, type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.1,
                           attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12, hidden_act="gelu", initializer_range=0.02)


class AllRowsScoresFn(torch.autograd.Function):
    """the reference's head: prediction_scores for every position, differentiable (its loss is torch's, outside)"""

    @staticmethod
    def forward(ctx, hidden, model):
        from item_alignment_amd.models.bert_pretrain import _transform_and_decode
        x = hidden.contiguous()
        logits, saved = _transform_and_decode(model, x)
        ctx.model, ctx.saved = model, (x,) + saved
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        from item_alignment_amd.models.bert_pretrain import _head_backward
        return _head_backward(ctx.model, ctx.saved[0], ctx.saved[1:], dlogits.to(torch.bfloat16)), None


def timed(fn, steps, warmup):
    import dp_bench
    times = sorted(dp_bench.timed(fn, steps, warmup))
    return dict(median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], repeats=steps, warmup=warmup)


def dp_child(a):
    """one rank of the --world measurement: its dist.deal_rows slice of the synthetic global batch, the step of bert_pretrain.py"""
    import dp_bench
    import item_alignment_amd.models as M
    from item_alignment_amd import dist as iadist
    from item_alignment_amd.data import bert_pretrain as D
    ranks = iadist.Ranks().init("cuda")
    dev = ranks.device
    rng = D.Rng(a.seed)
    examples = D.build_examples(synthetic_records(max(4, a.batch // 4), a.seed), _Tokenizer(), a.max_seq_len, rng)
    assert len(examples) >= a.batch, "too few synthetic examples"
    ids, mask, _types, labels, nsp = D.collate(examples[:a.batch])
    torch.manual_seed(a.seed)
    model = M.BertForPreTraining(config()).to(dev).train()

    staged = {}          # this rank's rows on the device, moved once as the one-process measurement moves its batch once

    def make_loss(lo, hi, rank, world):
        if not staged:
            staged.update(ids=ids[lo:hi].to(dev), mask=mask[lo:hi].to(dev), labels=labels[lo:hi].to(dev), nsp=nsp[lo:hi].to(dev))
        # the count exchange of every step, as in the script
        shares = iadist.loss_shares([int((labels[lo:hi] != -1).sum()), hi - lo])[0] if world > 1 else None
        return model(staged["ids"], attention_mask=staged["mask"], masked_lm_labels=staged["labels"], next_sentence_label=staged["nsp"],
                     loss_shares=shares)[0]

    res = dp_bench.timed_rank_step(make_loss, model.param_arena, a.batch, a.steps, a.warmup, ranks)
    res.update(positions=ids.shape[1], m_live_global=int((labels != -1).sum()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--max-seq-len", type=int, default=510)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--world", type=int, default=0, help="time the train step in one process and on this many data-parallel ranks, nothing else")
    ap.add_argument("--dp-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bert_pretrain_bench.py needs the GPU"
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dp_bench
    if a.dp_child:
        return dp_child(a)
    if a.world:
        dp_bench.measure(__file__, ["--batch", str(a.batch), "--max-seq-len", str(a.max_seq_len), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                    "--seed", str(a.seed)], a.world, a.out)
        return
    import item_alignment_amd.models as M
    from item_alignment_amd import ops
    from item_alignment_amd.data import bert_pretrain as D
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.models.bert_pretrain import MaskedLMHeadFn

    dev = torch.device("cuda:0")
    cfg = config()
    rng = D.Rng(a.seed)
    examples = D.build_examples(synthetic_records(max(4, a.batch // 4), a.seed), _Tokenizer(), a.max_seq_len, rng)
    assert len(examples) >= a.batch, "too few synthetic examples"
    ids, mask, _types, labels, nsp = (t.to(dev) for t in D.collate(examples[:a.batch]))
    B, L = ids.shape
    V, H = cfg.vocab_size, cfg.hidden_size
    m_live = int((labels != -1).sum())
    torch.manual_seed(a.seed)
    model = M.BertForPreTraining(cfg).to(dev).train()
    arena = model.param_arena

    def all_rows_loss():
        hidden = model.bert(ids, attention_mask=mask, position_ids=torch.arange(L, device=dev).unsqueeze(0).expand(B, L),
                            allow_unpad=False).last_hidden_state
        flat = hidden.reshape(B * L, H)
        scores = AllRowsScoresFn.apply(flat, model)
        pooled = Fn.GatherRowsFn.apply(flat, model.anchor, torch.arange(B, device=dev, dtype=torch.int32) * L, 0.0, 0)
        pooled = Fn.LinearSmallFn.apply(pooled, model.bert.pooler.dense.weight, model.bert.pooler.dense, 1)
        _, _, nsp_loss = Fn.PairHeadCEFn.apply(pooled, None, model.cls.seq_relationship, nsp)
        return F.cross_entropy(scores, labels.view(-1), ignore_index=-1) + nsp_loss

    step = lambda loss_fn: dp_bench.train_step(arena, loss_fn)
    live_loss = lambda: model(ids, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp)[0]
    res = dict(gpu=torch.cuda.get_device_name(0), batch=B, positions=L, layers=cfg.num_hidden_layers, hidden=H, vocab=V, m_live=m_live,
               live_fraction=m_live / (B * L))
    res["step_live_rows"] = timed(step(live_loss), a.steps, a.warmup)
    res["step_all_rows"] = timed(step(all_rows_loss), a.steps, a.warmup)
    res["step_all_rows_over_live_rows"] = res["step_all_rows"]["median_ms"] / res["step_live_rows"]["median_ms"]

    # the head alone on a fixed hidden state
    hidden = (torch.randn((B * L, H), device=dev) * 0.5).to(torch.bfloat16).requires_grad_(True)
    flat_labels = labels.view(-1)
    rows = (flat_labels != -1).nonzero(as_tuple=False).squeeze(1)
    live_labels = flat_labels.index_select(0, rows).contiguous()

    def head_live(i):
        MaskedLMHeadFn.apply(hidden, model, rows, live_labels).backward()

    def head_all(i):
        F.cross_entropy(AllRowsScoresFn.apply(hidden, model), flat_labels, ignore_index=-1).backward()

    res["head_live_rows"] = timed(head_live, a.kernel_repeats, a.warmup)
    res["head_all_rows"] = timed(head_all, a.steps, a.warmup)
    res["head_all_rows_over_live_rows"] = res["head_all_rows"]["median_ms"] / res["head_live_rows"]["median_ms"]
    res["head_live_rows_share_of_step"] = res["head_live_rows"]["median_ms"] / res["step_live_rows"]["median_ms"]
    res["head_all_rows_share_of_step"] = res["head_all_rows"]["median_ms"] / res["step_all_rows"]["median_ms"]

    # the two kernels alone on [m_live, V] logits
    logits = torch.randn((m_live, V), device=dev)
    one = torch.ones(1, device=dev)
    lse, _, loss = ops.vocab_ce_fwd(logits, live_labels)
    dl = torch.empty((m_live, V), device=dev, dtype=torch.bfloat16)
    fwd = timed(lambda i: ops.vocab_ce_fwd(logits, live_labels), a.kernel_repeats, a.warmup)
    bwd = timed(lambda i: ops.vocab_ce_bwd(logits, live_labels, lse, loss, one, out=dl), a.kernel_repeats, a.warmup)
    fwd["bytes"], bwd["bytes"] = m_live * V * 4, m_live * V * 6
    for k in (fwd, bwd):
        k["gb_per_s"] = k["bytes"] / (k["median_ms"] * 1e-3) / 1e9
    res["vocab_ce_fwd"], res["vocab_ce_bwd"] = fwd, bwd

    print(f"B {B} x L {L}, {m_live} labelled rows ({100 * res['live_fraction']:.2f} %): step {res['step_live_rows']['median_ms']:.1f} ms "
          f"(all-rows head {res['step_all_rows']['median_ms']:.1f} ms, x{res['step_all_rows_over_live_rows']:.2f}); head "
          f"{res['head_live_rows']['median_ms']:.2f} ms (all rows {res['head_all_rows']['median_ms']:.1f} ms); vocab_ce fwd "
          f"{fwd['median_ms'] * 1e3:.0f} us {fwd['gb_per_s']:.0f} GB/s, bwd {bwd['median_ms'] * 1e3:.0f} us {bwd['gb_per_s']:.0f} GB/s", flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
