"""BertForPreTraining on the HIP engine against transformers.BertForPreTraining (fp32, CPU, eval mode) with the same seeded weights
loaded through the shared state_dict key names.  The arithmetic is that of the reference's pytorch_transformers class (erf-GELU,
LayerNorm eps 1e-12); its ignore label -1 is mapped to transformers' -100 for the oracle.

Features in the layout of the reference's create_input_features: [CLS] / [SEP] with attention mask 0, ragged lengths, padding with
id 0 / mask 0 / label -1, between 1 and 6 labelled positions per sample and one sample with none.  Eight samples (with three,
tests/test_models_gpu.py found small gradients made of cancelling sums).

Bars: those of tests/test_models_gpu.py -- outputs and parameter gradients within 5e-2 of the tensor's max magnitude, gradient cosine
>= 0.99 against the fp32 oracle.  Every figure is printed before it is asserted (`-s` shows them).

One kind of tensor has no max magnitude to be relative to: the key bias of every attention layer.  q . (k + b) = q . k + q . b adds the
same number to every score of a query's row, which softmax ignores, so that gradient is identically zero and what either
implementation holds there is rounding residue (measured on an MI355X: cosine -0.52 / 0.50 between two such residues).  For it the
5e-2 bar is applied in its absolute form, against the max magnitude of the same layer's QUERY bias gradient in the oracle -- the
tensor of the same shape on the same path -- and the oracle's own residue has to be that small too."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL, COS_MIN = 5e-2, 0.99
B, L, V = 8, 24, 1000
CLS, SEP, MASK = 101, 102, 103


def config(**over):
    c = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=V, max_position_embeddings=64,
             type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12,
             hidden_act="gelu", initializer_range=0.02)
    c.update(over)
    return c


def features():
    """input_ids, attention_mask (float, as the reference's collate makes it), masked_lm_labels, next_sentence_label"""
    g = torch.Generator().manual_seed(7)
    ids = torch.zeros((B, L), dtype=torch.long)
    mask = torch.zeros((B, L))
    labels = torch.full((B, L), -1, dtype=torch.long)
    lengths = [22, 9, 15, 22, 5, 12, 18, 7]            # tokens between [CLS] and [SEP]
    n_labelled = [3, 1, 6, 0, 2, 4, 5, 1]
    for b, (n, k) in enumerate(zip(lengths, n_labelled)):
        tok = torch.randint(200, V, (n,), generator=g)
        ids[b, 0], ids[b, n + 1] = CLS, SEP
        ids[b, 1:n + 1] = tok
        mask[b, 1:n + 1] = 1.0
        pos = torch.randperm(n, generator=g)[:k] + 1
        for i, p in enumerate(pos.tolist()):
            labels[b, p] = ids[b, p]
            if i % 3 != 2:                             # most are replaced by [MASK], some stay as they are (the reference does both)
                ids[b, p] = MASK
    nsp = torch.tensor([1, 0, 1, 1, 0, 1, 0, 1])
    return ids, mask, labels, nsp


@pytest.fixture(scope="module")
def oracle():
    """the transformers model, its state_dict, its outputs and gradients -- computed once, never modified"""
    import transformers
    torch.manual_seed(1234)
    hf = transformers.BertForPreTraining(transformers.BertConfig(**config())).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in hf.named_parameters():              # biases and LayerNorm weights off their 0 / 1 initial values
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    ids, mask, labels, nsp = features()
    out = hf(input_ids=ids, attention_mask=mask, labels=labels.masked_fill(labels == -1, -100), next_sentence_label=nsp,
             output_hidden_states=True)
    out.loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in hf.named_parameters()}
    return SimpleNamespace(sd=sd, loss=out.loss.detach(), scores=out.prediction_logits.detach(), seq=out.seq_relationship_logits.detach(),
                           hidden=out.hidden_states[-1].detach(), grads=grads, keys=set(hf.state_dict().keys()))


def build(oracle):
    import item_alignment_amd.models as M
    model = M.BertForPreTraining(SimpleNamespace(**config()))
    missing, unexpected = model.load_state_dict(oracle.sd, strict=False)
    assert unexpected == ["cls.predictions.decoder.bias"], unexpected
    assert all("position_ids" in k for k in missing), missing
    return model.cuda().eval()


def rel(name, got, want):
    r = ((got.detach().float().cpu() - want.float()).abs().max() / (want.float().abs().max() + 1e-6)).item()
    print(f"[bert_pretrain] {name}: |got - want|_max / |want|_max = {r:.4f}")
    return r


def to_gpu(*ts):
    return [t.cuda() for t in ts]


def test_state_dict_keys_are_the_oracles(gpu, oracle):
    import item_alignment_amd.models as M
    own = set(M.BertForPreTraining(SimpleNamespace(**config())).state_dict().keys())
    strip = lambda keys: {k for k in keys if "position_ids" not in k and k != "cls.predictions.decoder.bias"}
    assert strip(own) == strip(oracle.keys)


def test_loss_outputs_and_gradients_match_the_oracle(gpu, oracle):
    model = build(oracle)
    ids, mask, labels, nsp = to_gpu(*features())
    model.param_arena.zero_grad()
    out = model(ids, token_type_ids=None, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp)
    assert out[1] is None                              # the documented deviation: no [B, L, V] scores beside a loss
    loss, seq = out[0], out[2]
    print(f"[bert_pretrain] loss {loss.item():.5f} (oracle {oracle.loss.item():.5f})")
    assert abs(loss.item() - oracle.loss.item()) < TOL * abs(oracle.loss.item())
    assert rel("seq_relationship_score", seq, oracle.seq) < TOL
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
            print(f"[bert_pretrain] grad {k}: |got|_max {g_max:.3e}, |oracle|_max {w_max:.3e}, query bias gradient max {scale:.3e}")
            if not (g_max <= TOL * scale and w_max <= TOL * scale):
                bad.append((k, "got", g_max, "oracle", w_max, "scale", scale))
            continue
        a, b = got.float().cpu().flatten(), want.flatten()
        c = (torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)).item()
        r = rel(f"grad {k} (cos {c:.4f})", got, want)
        if not (c >= COS_MIN and r <= TOL):
            bad.append((k, "cos", c, "rel", r))
    assert not bad, bad


def test_word_table_gradient_is_embedding_share_plus_decoder_share(gpu, oracle):
    """the oracle's tied gradient has both shares; rows that only the decoder reaches (ids never fed in) and rows only the embedding
    reaches would each expose a missing share"""
    model = build(oracle)
    ids, mask, labels, nsp = to_gpu(*features())
    model.param_arena.zero_grad()
    model(ids, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp)[0].backward()
    torch.cuda.synchronize()
    table = model.bert.embeddings.word_embeddings.weight
    assert model.cls.predictions.decoder.weight is table
    got, want = table.grad.float().cpu(), oracle.grads["bert.embeddings.word_embeddings.weight"]
    fed = torch.zeros(V, dtype=torch.bool)
    fed[ids.cpu().reshape(-1)] = True
    fed[0] = False                                     # the padding row takes no embedding gradient
    assert rel("table grad, rows never fed in (decoder share alone)", got[~fed], want[~fed]) < TOL
    assert rel("table grad, rows fed in (both shares)", got[fed], want[fed]) < TOL


def test_scores_without_labels_and_the_dense_loss(gpu, oracle):
    """without labels: dense fp32 prediction_scores + the NSP logits, as the reference class returns; the loss over the labelled rows
    equals F.cross_entropy over those dense scores.  Both run the same GEMM kernels on the same bf16 operands and the same fp32
    logits per row, so they differ by fp32 summation only: the loss kernel's bound (tests/vocab_ce_reference.py, below 1e-5 relative at
    V = 1000) plus torch's own -- 1e-5 relative leaves room for both."""
    model = build(oracle)
    ids, mask, labels, nsp = to_gpu(*features())
    with torch.no_grad():
        scores, seq = model(ids, attention_mask=mask)
        total = model(ids, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp)[0]
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (B, L, V)
    assert rel("prediction_scores", scores, oracle.scores) < TOL
    assert rel("seq_relationship_score", seq, oracle.seq) < TOL
    dense = F.cross_entropy(scores.view(-1, V), labels.view(-1), ignore_index=-1) + F.cross_entropy(seq, nsp)
    print(f"[bert_pretrain] labelled-rows loss {total.item():.7f}, dense loss {dense.item():.7f}")
    assert abs(total.item() - dense.item()) <= 1e-5 * abs(dense.item())


def test_no_labelled_row_gives_nan_like_torch(gpu, oracle):
    model = build(oracle)
    ids, mask, labels, nsp = to_gpu(*features())
    with torch.no_grad():
        out = model(ids, attention_mask=mask, masked_lm_labels=torch.full_like(labels, -1), next_sentence_label=nsp)
    assert torch.isnan(out[0])


def test_save_pretrained_feeds_roberta_model(gpu, oracle, tmp_path):
    import json
    import logging
    import item_alignment_amd.models as M
    model = build(oracle)
    ids, mask, _, _ = to_gpu(*features())
    pos = torch.arange(L, device="cuda").unsqueeze(0).expand(B, L)
    with torch.no_grad():
        want = model.bert(ids, attention_mask=mask, position_ids=pos, allow_unpad=False).last_hidden_state.float().cpu()
    model.save_pretrained(str(tmp_path))
    sd = torch.load(tmp_path / "pytorch_model.bin", map_location="cpu")
    assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())
    assert json.load(open(tmp_path / "config.json"))["vocab_size"] == V
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    log = logging.getLogger("item_alignment_amd")
    log.addHandler(handler)
    try:
        tower = M.RobertaModel.from_pretrained(str(tmp_path), config=SimpleNamespace(**config())).cuda().eval()
    finally:
        log.removeHandler(handler)
    text = " ".join(r.getMessage() for r in records)
    assert "bert." not in text.replace("bert.embeddings.position_ids", ""), text          # no unmatched bert.* key
    assert "keep their random initialisation" not in text, text
    with torch.no_grad():
        got = tower(ids, attention_mask=mask, position_ids=pos, allow_unpad=False).last_hidden_state.float().cpu()
    assert torch.equal(got, want)
    assert rel("last hidden state", got, oracle.hidden) < TOL


def test_vocab_size_must_be_a_multiple_of_8(gpu):
    import item_alignment_amd.models as M
    with pytest.raises(ValueError, match="multiple of 8.*resize the word table to 1008"):
        M.BertForPreTraining(SimpleNamespace(**config(vocab_size=1003)))
