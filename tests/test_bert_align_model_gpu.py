"""BertAlignModel on the HIP engine against transformers.BertForNextSentencePrediction (fp32, CPU, eval mode) with the same seeded
weights loaded through the shared state_dict key names: the oracle's `.bert` is called once per field, the five pooled outputs are
summed, then `.cls` and the cross-entropy -- the reference's BertAlignModel.forward, spelled out.

The tiny configuration of tests/test_bert_pretrain_model_gpu.py; four pairs; field lengths 40 / 24 / 8 / 16 / 8 (pvs, title, cate,
cate_path, industry_name).  The valid lengths hold a full-length sequence in every field, the three-token minimum [CLS][SEP][SEP],
7 / 8 / 9 and 31 / 32 / 33 (either side of an 8-row slab and of a 32-row block), and both token types.

Bars: those of tests/test_bert_pretrain_model_gpu.py -- outputs and parameter gradients within 5e-2 of the tensor's max magnitude,
gradient cosine >= 0.99 against the fp32 oracle, and its treatment of the attention key bias, whose gradient is identically zero in
exact arithmetic: the 5e-2 bar in its absolute form, against the max magnitude of the same layer's query bias gradient in the oracle.
Every figure is printed before it is asserted (`-s` shows them).

The labels are 1, 1, 0, 1 -- both classes, three to one -- for a reason that is a property of the fp32 oracle alone.  With seeded
weights of std 0.02 the four pool_out rows are nearly the same vector and every pair's match probability is 0.485, so every pair sends
the same gradient +-(1 - p) / B into the head, its sign set by the label.  With two labels of each class the parameter gradients are
differences of two nearly equal sums: in the oracle, max |sum over pairs| is 0.03 of max (sum over pairs of | . |) for every parameter
tensor, a 33-fold cancellation, and "error over the tensor's max magnitude" then measures each bf16 rounding (2^-9 of a TERM) against
a thirtieth of the terms.  Three to one leaves 0.40 - 0.52 of the terms standing (all four alike would leave 1.0 but never exercise
the other class).  tests/test_bert_pretrain_model_gpu.py notes the same experience with three samples."""
import logging
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL, COS_MIN = 5e-2, 0.99
B, V = 4, 1000
CLS, SEP = 101, 102
FIELDS = ("pvs", "title", "cate", "cate_path", "industry_name")
FIELD_LEN = dict(pvs=40, title=24, cate=8, cate_path=16, industry_name=8)
VALID = dict(pvs=[40, 33, 32, 31], title=[24, 9, 17, 7], cate=[8, 3, 5, 7], cate_path=[16, 9, 8, 3], industry_name=[3, 8, 4, 6])
FULL = {f: [FIELD_LEN[f]] * B for f in FIELDS}
LABELS = [1, 1, 0, 1]


def config(**over):
    c = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=V, max_position_embeddings=64,
             type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12,
             hidden_act="gelu", initializer_range=0.02)
    c.update(over)
    return c


def features(valid=VALID, extra=0, seed=7):
    """the fifteen keyword tensors (CPU, int64) + labels.  A sequence of n valid tokens is [CLS] a.. [SEP] b.. [SEP] with token type 0
    up to the first [SEP] and 1 behind it.  extra > 0: every field `extra` positions longer, the padded positions (and only they) filled
    with random ids and token types -- what they hold must not matter."""
    g = torch.Generator().manual_seed(seed)
    junk = torch.Generator().manual_seed(seed + 1000)
    kw = {}
    for f in FIELDS:
        L = FIELD_LEN[f]
        ids = torch.zeros((B, L + extra), dtype=torch.long)
        types, mask = torch.zeros_like(ids), torch.zeros_like(ids)
        for b, n in enumerate(valid[f]):
            first = 1 + (n - 3 + 1) // 2                # position of the first [SEP]
            ids[b, :n] = torch.randint(200, V, (n,), generator=g)
            ids[b, 0], ids[b, first], ids[b, n - 1] = CLS, SEP, SEP
            types[b, first + 1:n] = 1
            mask[b, :n] = 1
            if extra:
                ids[b, n:] = torch.randint(1, V, (L + extra - n,), generator=junk)
                types[b, n:] = torch.randint(0, 2, (L + extra - n,), generator=junk)
        kw[f"{f}_input_ids"], kw[f"{f}_token_type_ids"], kw[f"{f}_attention_mask"] = ids, types, mask
    return kw, torch.tensor(LABELS)


def oracle_forward(hf, kw, labels):
    pool = sum(hf.bert(input_ids=kw[f"{f}_input_ids"], token_type_ids=kw[f"{f}_token_type_ids"],
                       attention_mask=kw[f"{f}_attention_mask"]).pooler_output for f in FIELDS)
    score = hf.cls(pool)
    return pool, score, F.cross_entropy(score.view(-1, 2), labels.view(-1))


@pytest.fixture(scope="module")
def oracle():
    """the transformers model, its state_dict, its outputs and gradients on the ragged batch, its outputs on the all-valid batch --
    computed once, never modified"""
    import transformers
    torch.manual_seed(1234)
    hf = transformers.BertForNextSentencePrediction(transformers.BertConfig(**config())).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in hf.named_parameters():              # biases and LayerNorm weights off their 0 / 1 initial values
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    kw, labels = features()
    pool, score, loss = oracle_forward(hf, kw, labels)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in hf.named_parameters()}
    with torch.no_grad():
        full = oracle_forward(hf, *features(FULL))
    return SimpleNamespace(sd=sd, pool=pool.detach(), score=score.detach(), loss=loss.detach(), grads=grads, keys=set(hf.state_dict().keys()),
                           full=SimpleNamespace(pool=full[0], score=full[1], loss=full[2]))


def build(oracle):
    import item_alignment_amd.models as M
    model = M.BertAlignModel(SimpleNamespace(**config()))
    missing, unexpected = model.load_state_dict(oracle.sd, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k for k in missing), missing
    return model.cuda().eval()


def rel(name, got, want):
    r = ((got.detach().float().cpu() - want.float()).abs().max() / (want.float().abs().max() + 1e-6)).item()
    print(f"[bert_align] {name}: |got - want|_max / |want|_max = {r:.4f}")
    return r


def to_gpu(kw, labels):
    return {k: v.cuda() for k, v in kw.items()}, labels.cuda()


def test_the_valid_lengths_cover_what_the_docstring_says():
    kw, _ = features()
    lens = [n for f in FIELDS for n in VALID[f]]
    assert {3, 7, 8, 9, 31, 32, 33, 40} <= set(lens) and all(max(VALID[f]) == FIELD_LEN[f] for f in FIELDS)
    for f in FIELDS:
        t, m = kw[f"{f}_token_type_ids"], kw[f"{f}_attention_mask"]
        assert m.sum(dim=1).tolist() == VALID[f] and bool((m[:, 0] == 1).all())
        assert set(t[m == 1].tolist()) == {0, 1} and bool((t[m == 0] == 0).all())


def test_state_dict_keys_are_the_oracles(gpu, oracle):
    import item_alignment_amd.models as M
    own = set(M.BertAlignModel(SimpleNamespace(**config())).state_dict().keys())
    strip = lambda keys: {k for k in keys if "position_ids" not in k}
    assert strip(own) == strip(oracle.keys)
    assert "cls.seq_relationship.weight" in own and "bert.pooler.dense.bias" in own


def test_outputs_loss_and_gradients_match_the_oracle(gpu, oracle):
    model = build(oracle)
    kw, labels = to_gpu(*features())
    model.param_arena.zero_grad()
    out = model(next_sentence_label=labels, **kw)
    assert len(out) == 3
    pool, score, loss = out
    assert pool.dtype == torch.float32 and tuple(pool.shape) == (B, 128) and tuple(score.shape) == (B, 2)
    print(f"[bert_align] loss {loss.item():.5f} (oracle {oracle.loss.item():.5f})")
    assert rel("pool_out", pool, oracle.pool) < TOL
    assert rel("seq_relationship_score", score, oracle.score) < TOL
    assert abs(loss.item() - oracle.loss.item()) < TOL * abs(oracle.loss.item())
    loss.backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    assert set(params) == set(oracle.grads)
    bad = []
    for k, want in oracle.grads.items():
        got = params[k].grad
        assert torch.isfinite(got).all(), k
        if k.endswith("attention.self.key.bias"):        # identically zero in exact arithmetic: the module docstring
            scale = oracle.grads[k.replace("key.bias", "query.bias")].abs().max().item()
            g_max, w_max = got.abs().max().item(), want.abs().max().item()
            print(f"[bert_align] grad {k}: |got|_max {g_max:.3e}, |oracle|_max {w_max:.3e}, query bias gradient max {scale:.3e}")
            if not (g_max <= TOL * scale and w_max <= TOL * scale):
                bad.append((k, "got", g_max, "oracle", w_max, "scale", scale))
            continue
        a, b = got.float().cpu().flatten(), want.flatten()
        c = (torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)).item()
        r = rel(f"grad {k} (cos {c:.4f})", got, want)
        if not (c >= COS_MIN and r <= TOL):
            bad.append((k, "cos", c, "rel", r))
    assert not bad, bad


def test_without_labels_two_outputs_and_no_position_padded(gpu, oracle):
    """the all-valid batch: the ragged pass is the model's only path, also when there is nothing to drop"""
    model = build(oracle)
    kw, labels = to_gpu(*features(FULL))
    with torch.no_grad():
        out = model(**kw)
        with_labels = model(next_sentence_label=labels, **kw)
    assert len(out) == 2 and len(with_labels) == 3
    assert torch.equal(out[0], with_labels[0]) and torch.equal(out[1], with_labels[1])
    assert rel("pool_out, all valid", out[0], oracle.full.pool) < TOL
    assert rel("seq_relationship_score, all valid", out[1], oracle.full.score) < TOL
    assert abs(with_labels[2].item() - oracle.full.loss.item()) < TOL * abs(oracle.full.loss.item())


def test_what_the_padded_positions_hold_changes_no_bit(gpu, oracle):
    """every field 8 positions longer, random ids and token types in the padded positions: a padded position is never gathered, so
    pool_out, the scores, the loss and every gradient are the same bytes -- in training mode, dropout included (its streams are keyed by
    the step seed and the packed row)"""
    from item_alignment_amd.models import functional as Fn
    model = build(oracle).train()
    arena = model.param_arena
    got = []
    for extra in (0, 8):
        kw, labels = to_gpu(*features(extra=extra))
        Fn.set_step_seed(11)
        Fn.reset_use_counts()
        arena.zero_grad()
        pool, score, loss = model(next_sentence_label=labels, **kw)
        loss.backward()
        torch.cuda.synchronize()
        got.append((pool.detach().clone(), score.detach().clone(), loss.detach().clone(), arena.grad.clone()))
    assert got[0][3].abs().max().item() > 0
    for name, a, b in zip(("pool_out", "scores", "loss", "gradients"), got[0], got[1]):
        assert torch.equal(a, b), name


def test_the_ragged_pass_against_five_dense_passes(gpu, oracle):
    """the same modules as five padded passes through model.bert, every row computed (allow_unpad=False), in eval mode"""
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.models.base import ACT_TANH, cls_rows
    model = build(oracle)
    kw, _ = to_gpu(*features())
    with torch.no_grad():
        pool = model(**kw)[0]
        dense = 0
        for f in FIELDS:
            ids = kw[f"{f}_input_ids"]
            L = ids.shape[1]
            pos = torch.arange(L, device="cuda").unsqueeze(0).expand(B, L)
            h = model.bert(ids, attention_mask=kw[f"{f}_attention_mask"], token_type_ids=kw[f"{f}_token_type_ids"], position_ids=pos,
                           allow_unpad=False).last_hidden_state
            x = Fn.GatherRowsFn.apply(h.reshape(B * L, -1), model.anchor, cls_rows(B, L, 0, "cuda"), 0.0, 0)
            dense = dense + Fn.LinearSmallFn.apply(x, model.bert.pooler.dense.weight, model.bert.pooler.dense, ACT_TANH)
    print(f"[bert_align] ragged against dense: largest |difference| {(pool - dense).abs().max().item():.3e}, largest |dense| "
          f"{dense.abs().max().item():.3e}")
    assert rel("pool_out, ragged against five dense passes", pool, dense.cpu()) < TOL


def test_a_sequence_without_a_valid_token_is_refused(gpu, oracle):
    model = build(oracle)
    kw, labels = to_gpu(*features())
    kw["cate_attention_mask"] = kw["cate_attention_mask"].clone()
    kw["cate_attention_mask"][2] = 0
    with pytest.raises(ValueError, match="attention mask of zeros only"):
        model(next_sentence_label=labels, **kw)


def test_noise_arguments_are_not_implemented(gpu, oracle):
    model = build(oracle)
    kw, _ = to_gpu(*features())
    for name in ("pvs_noise", "title_noise"):
        with pytest.raises(NotImplementedError, match="adversarial"):
            model(**kw, **{name: torch.zeros(1, device="cuda")})


def test_get_sim_eval_weight_gives_the_score_from_pool_out(gpu, oracle):
    model = build(oracle)
    kw, _ = to_gpu(*features())
    with torch.no_grad():
        pool, score = model(**kw)
    w, b = model.get_sim_eval_weight()
    assert w.device.type == "cpu" and b.device.type == "cpu" and tuple(w.shape) == (128,) and b.dim() == 0
    sd = oracle.sd
    assert torch.equal(w, sd["cls.seq_relationship.weight"][1] - sd["cls.seq_relationship.weight"][0])
    assert torch.equal(b, sd["cls.seq_relationship.bias"][1] - sd["cls.seq_relationship.bias"][0])
    want = (score[:, 1] - score[:, 0]).cpu()
    got = (pool.cpu() * w).sum(dim=1) + b
    assert (got - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())       # the same fp32 dot products, regrouped


def captured_warnings(fn):
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    log = logging.getLogger("item_alignment_amd")
    log.addHandler(handler)
    try:
        out = fn()
    finally:
        log.removeHandler(handler)
    return out, " ".join(r.getMessage() for r in records)


def test_save_pretrained_round_trip(gpu, oracle, tmp_path):
    import json
    import item_alignment_amd.models as M
    model = build(oracle)
    kw, _ = to_gpu(*features())
    with torch.no_grad():
        want = model(**kw)
    model.save_pretrained(str(tmp_path))
    sd = torch.load(tmp_path / "pytorch_model.bin", map_location="cpu")
    assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())
    assert json.load(open(tmp_path / "config.json"))["hidden_size"] == 128
    again, text = captured_warnings(lambda: M.BertAlignModel.from_pretrained(str(tmp_path)))        # the configuration from config.json
    assert "no counterpart" not in text and "keep their random initialisation" not in text, text
    for k, v in oracle.sd.items():
        if "position_ids" not in k:
            assert torch.equal(again.state_dict()[k], v), k
    again = again.cuda().eval()
    with torch.no_grad():
        got = again(**kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_loads_what_bert_pretraining_saves(gpu, tmp_path):
    """the directory bert_pretrain.py writes: cls.predictions.* has no counterpart and is reported, cls.seq_relationship.* is loaded"""
    import item_alignment_amd.models as M
    torch.manual_seed(3)
    pre = M.BertForPreTraining(SimpleNamespace(**config()))
    with torch.no_grad():
        pre.cls.seq_relationship.bias.add_(0.25)
    pre.save_pretrained(str(tmp_path))
    model, text = captured_warnings(lambda: M.BertAlignModel.from_pretrained(str(tmp_path)))
    assert "cls.predictions" in text and "no counterpart" in text, text
    assert "keep their random initialisation" not in text.replace("bert.embeddings.position_ids", ""), text
    own, src = model.state_dict(), pre.state_dict()
    for k in own:
        if "position_ids" not in k:
            assert torch.equal(own[k], src[k]), k
    assert float(own["cls.seq_relationship.bias"][0]) == 0.25
    assert all(p.requires_grad for p in model.bert.pooler.parameters())
