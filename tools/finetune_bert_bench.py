"""Times one train step of the BERT pair classifier (BertAlignModel, finetune_bert.py) on one GPU at the reference's shape: bert-base
(12 layers, hidden 768, vocabulary 21 128), batch 16, field lengths 512 / 150 / 20 / 50 / 20 (pvs, title, cate, cate_path,
industry_name).  The valid length of every sequence is drawn from a seeded distribution that is written into the result.

    python tools/finetune_bert_bench.py [--batch 16 --steps 10 --warmup 3 --rounds 3 --seed 1 --out profiles/finetune_bert_bench.json]

Two forms of the same step (forward, backward, gradient norm, fused AdamW) over the same modules and weights:
  (a) ragged: the model's forward -- the valid tokens of all 5 B sequences as one packed batch;
  (b) padded: five passes through model.bert at the five padded lengths with the padded-row filters switched on
      (allow_unpad=True, padded_rows_unread=True, cls_only_read=True), the pooler on the five [CLS] rows, the same head.
Medians of the timed repeats after a warm-up of each form, events on the stream; the two forms alternate, `--rounds` times, and every
other round starts with the other one, so neither always runs first or behind the same neighbour.  Recorded, not gated: there is no
earlier figure to compare with.

    python tools/finetune_bert_bench.py --world 8 [--batch 16 ...] --out profiles/finetune_bert_bench.json

times only the ragged train step, as finetune_bert.py takes it under a launcher: once in one process and once on 8 data-parallel
ranks that share the same global batch, every rank a fresh child process (tools/dp_bench.py).  The two figures are merged into the
profile under "data_parallel"; a box with fewer GPUs than ranks records that the 8-rank figure is unmeasured.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("pvs", "title", "cate", "cate_path", "industry_name")
FIELD_LEN = dict(pvs=512, title=150, cate=20, cate_path=50, industry_name=20)
# valid length of a sequence = clamp(round(mean + std * N(0, 1)), 3, field length): a guess at a product corpus (attribute lists that
# rarely fill 512 positions, titles that mostly fit 150, short category names) -- written into the result so a reader can judge it
LENGTH_MODEL = dict(pvs=(260, 120), title=(90, 30), cate=(10, 3), cate_path=(28, 8), industry_name=(9, 3))
CLS, SEP = 101, 102


def config():
    return SimpleNamespace(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=21128,
                           max_position_embeddings=512, type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.1,
                           attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12, hidden_act="gelu", initializer_range=0.02)


def synthetic_batch(batch, seed, vocab=21128):
    """the fifteen keyword tensors of BertAlignModel.forward (CPU, int64), the labels, and the valid lengths per field"""
    g = torch.Generator().manual_seed(seed)
    kw, lengths = {}, {}
    for f in FIELDS:
        L = FIELD_LEN[f]
        mean, std = LENGTH_MODEL[f]
        n = (mean + std * torch.randn(batch, generator=g)).round().clamp(3, L).long()
        ids = torch.zeros((batch, L), dtype=torch.long)
        types, mask = torch.zeros_like(ids), torch.zeros_like(ids)
        for b, k in enumerate(n.tolist()):
            first = 1 + (k - 2) // 2
            ids[b, :k] = torch.randint(1000, vocab, (k,), generator=g)
            ids[b, 0], ids[b, first], ids[b, k - 1] = CLS, SEP, SEP
            types[b, first + 1:k] = 1
            mask[b, :k] = 1
        kw[f"{f}_input_ids"], kw[f"{f}_token_type_ids"], kw[f"{f}_attention_mask"] = ids, types, mask
        lengths[f] = n.tolist()
    labels = torch.randint(0, 2, (batch,), generator=g)
    return kw, labels, lengths


def summary(times, warmup):
    s = sorted(times)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1], repeats=len(s), warmup_per_round=warmup)


def dp_child(a):
    """one rank of the --world measurement: its dist.deal_rows slice of the synthetic global batch, the step of finetune_bert.py"""
    import dp_bench
    import item_alignment_amd.models as M
    from item_alignment_amd import dist as iadist
    ranks = iadist.Ranks().init("cuda")
    dev = ranks.device
    kw, labels, lengths = synthetic_batch(a.batch, a.seed, config().vocab_size)
    torch.manual_seed(a.seed)
    model = M.BertAlignModel(config()).to(dev).train()

    staged = {}          # this rank's pairs on the device, moved once as the one-process measurement moves its batch once

    def make_loss(lo, hi, rank, world):
        if not staged:
            staged.update(next_sentence_label=labels[lo:hi].to(dev), **{k: v[lo:hi].to(dev) for k, v in kw.items()})
        loss = model(**staged)[-1]
        return loss * iadist.loss_shares([hi - lo])[0][0] if world > 1 else loss          # the count exchange of every step, as in the script

    res = dp_bench.timed_rank_step(make_loss, model.param_arena, a.batch, a.steps, a.warmup, ranks)
    res.update(valid_tokens_global=sum(sum(v) for v in lengths.values()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10, help="timed steps of each form in every round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of each form in front of its timed ones, every round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--world", type=int, default=0, help="time the ragged train step in one process and on this many data-parallel ranks, nothing else")
    ap.add_argument("--dp-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "finetune_bert_bench.py needs the GPU"
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dp_bench
    if a.dp_child:
        return dp_child(a)
    if a.world:
        dp_bench.measure(__file__, ["--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup), "--seed", str(a.seed)],
                         a.world, a.out)
        return
    import item_alignment_amd.models as M
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.models.base import ACT_TANH, cls_rows

    dev = torch.device("cuda:0")
    cfg = config()
    kw_cpu, labels_cpu, lengths = synthetic_batch(a.batch, a.seed, cfg.vocab_size)
    kw = {k: v.to(dev) for k, v in kw_cpu.items()}
    labels = labels_cpu.to(dev)
    B = a.batch
    valid = sum(sum(v) for v in lengths.values())
    padded = B * sum(FIELD_LEN.values())
    torch.manual_seed(a.seed)
    model = M.BertAlignModel(cfg).to(dev).train()
    arena = model.param_arena
    positions = {f: torch.arange(FIELD_LEN[f], device=dev).unsqueeze(0).expand(B, FIELD_LEN[f]) for f in FIELDS}

    def ragged_loss():
        return model(next_sentence_label=labels, **kw)[-1]

    def padded_loss():
        pool = 0
        for f in FIELDS:
            L = FIELD_LEN[f]
            h = model.bert(kw[f"{f}_input_ids"], attention_mask=kw[f"{f}_attention_mask"], token_type_ids=kw[f"{f}_token_type_ids"],
                           position_ids=positions[f], allow_unpad=True, padded_rows_unread=True, cls_only_read=True).last_hidden_state
            x = Fn.GatherRowsFn.apply(h.reshape(B * L, -1), model.anchor, cls_rows(B, L, 0, dev), 0.0, 0)
            pool = pool + Fn.LinearSmallFn.apply(x, model.bert.pooler.dense.weight, model.bert.pooler.dense, ACT_TANH)
        return Fn.PairHeadCEFn.apply(pool, None, model.cls.seq_relationship, labels)[2]

    step = lambda loss_fn: dp_bench.train_step(arena, loss_fn)
    # the two forms compute the same function: their losses on the same weights, in evaluation mode (no dropout), side by side
    model.eval()
    with torch.no_grad():
        loss_a, loss_b = ragged_loss().item(), padded_loss().item()
    model.train()

    forms = {"ragged": step(ragged_loss), "padded": step(padded_loss)}
    times = {name: [] for name in forms}
    per_round = []
    for r in range(a.rounds):
        order = ("ragged", "padded") if r % 2 == 0 else ("padded", "ragged")
        row = {}
        for name in order:
            t = dp_bench.timed(forms[name], a.steps, a.warmup)
            times[name] += t
            row[name] = sorted(t)[len(t) // 2]
        per_round.append(dict(order=list(order), median_ms=row))

    res = dict(gpu=torch.cuda.get_device_name(0), batch=B, layers=cfg.num_hidden_layers, hidden=cfg.hidden_size, field_lengths=FIELD_LEN,
               seed=a.seed, length_model={f: dict(mean=m, std=s, clamp=[3, FIELD_LEN[f]]) for f, (m, s) in LENGTH_MODEL.items()},
               valid_lengths=lengths, valid_tokens=valid, padded_positions=padded, valid_share=valid / padded,
               eval_loss_ragged=loss_a, eval_loss_padded=loss_b,
               step_ragged=summary(times["ragged"], a.warmup), step_padded=summary(times["padded"], a.warmup), rounds=per_round)
    res["padded_over_ragged"] = res["step_padded"]["median_ms"] / res["step_ragged"]["median_ms"]
    print(f"B {B}, {valid} valid tokens of {padded} positions ({100 * res['valid_share']:.1f} %): ragged step "
          f"{res['step_ragged']['median_ms']:.2f} ms, five padded passes {res['step_padded']['median_ms']:.2f} ms "
          f"(x{res['padded_over_ragged']:.3f}); eval loss {loss_a:.5f} / {loss_b:.5f}", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
