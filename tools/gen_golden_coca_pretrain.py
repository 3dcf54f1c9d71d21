"""Writes tests/golden/coca/pretrain.npz from the reference's own CoCaForPretraining.

    python tools/gen_golden_coca_pretrain.py <reference checkout>

The reference's src/models classes CoCaForPretraining and RobertaModel are imported under the stub recipe of SURVEY.md Appendix B
(oracle/ref_harness.py) and run as they are, in fp32 on the CPU, in eval mode.  timm is absent, so the image encoder handed to the
reference class is a module around oracle.ref_models.vit_forward_features with timm's key names, as oracle/gen_golden.py builds one.

Geometry: text tower hidden 128, 2 layers, 2 heads (intermediate 128, 96 positions); 2 multimodal layer pairs with 2 heads and ff mult 2;
ViT 128 wide, depth 2, patch 16, image 64 (an 8-class head nobody reads, for the key list); vocabulary 64; B = 4 sequences of n = 5 and
n = 70 tokens.  Explicit labels [B, n]: random tokens on the first len_b positions, pad (0) behind them; one sequence has no pad.

Stored: every entry of the state dict (`wq.<key>` int8 with `ws.<key>` its scale for the float tensors, weight = wq * ws -- a few levels
of a power-of-two grid, bf16-representable and small in the file; `wb.<key>` the other buffers as they are), per n the inputs, the
total loss and its two parts (recomputed here from the model's own tensors), the gradients named in GRADS (ROW_STRIDE: every fourth
row of the largest), and `keys`, the sorted state-dict keys.  Outputs and gradients are fp32 rounded to 11 significant bits
(tools/gen_golden_coca_decoder.py: short()).  The `temperature` weight is chosen here, the largest value of a 1/4 grid at which every
diagonal softmax probability of sim and sim^T lies in [0.02, 0.98] for both n: a contrastive loss that is saturated would pin nothing.
The file is byte-reproducible.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_coca_decoder import ROOT, short, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "coca")
HID, VOCAB, B, NS, IMG, PATCH, VIT_CLASSES = 128, 64, 4, (5, 70), 64, 16, 8
LENS = {5: (5, 3, 2, 1), 70: (70, 40, 20, 9)}
GRADS = ("temperature", "to_logits.0.gamma", "coca.text_encoder.embeddings.word_embeddings.weight",
         "multimodal_layers.0.0.fn.fused_attn_ff_proj.weight", "multimodal_layers.1.1.fn.to_kv.weight",
         "coca.text_encoder.encoder.layer.0.attention.self.query.weight", "coca.img_encoder.pos_embed")
# the fused projection's gradient is [768, 128]: every fourth row is stored (rows of all five parts: q, k, v, x, gate), which keeps the
# file under the size limit of a committed file
ROW_STRIDE = {"multimodal_layers.0.0.fn.fused_attn_ff_proj.weight": 4}


def vit_spec():
    npatch = (IMG // PATCH) ** 2
    spec = [("cls_token", (1, 1, HID)), ("pos_embed", (1, npatch + 1, HID)), ("patch_embed.proj.weight", (HID, 3, PATCH, PATCH)),
            ("patch_embed.proj.bias", (HID,))]
    for i in range(2):
        b = f"blocks.{i}"
        spec += [(b + ".norm1.weight", (HID,)), (b + ".norm1.bias", (HID,)), (b + ".attn.qkv.weight", (3 * HID, HID)),
                 (b + ".attn.qkv.bias", (3 * HID,)), (b + ".attn.proj.weight", (HID, HID)), (b + ".attn.proj.bias", (HID,)),
                 (b + ".norm2.weight", (HID,)), (b + ".norm2.bias", (HID,)), (b + ".mlp.fc1.weight", (4 * HID, HID)),
                 (b + ".mlp.fc1.bias", (4 * HID,)), (b + ".mlp.fc2.weight", (HID, 4 * HID)), (b + ".mlp.fc2.bias", (HID,))]
    return spec + [("norm.weight", (HID,)), ("norm.bias", (HID,)), ("head.weight", (VIT_CLASSES, HID)), ("head.bias", (VIT_CLASSES,))]


def make_vit(O):
    class VitModule(torch.nn.Module):
        """the parameters of timm's VisionTransformer under its key names; the arithmetic is the oracle's restatement"""

        def __init__(self):
            super().__init__()
            self.vcfg = SimpleNamespace(embed_dim=HID, depth=2, num_heads=2, patch_size=PATCH, eps=1e-6, image_size=IMG)
            self.num_features = HID
            self.names = {}
            for k, shape in vit_spec():
                self.names[k] = k.replace(".", "__")
                self.register_parameter(self.names[k], torch.nn.Parameter(torch.zeros(shape)))

        def forward_features(self, x):
            return O.vit_forward_features({"v." + k: getattr(self, pk) for k, pk in self.names.items()}, "v", self.vcfg, x)

        def forward_head(self, x, pre_logits=False):
            return O.vit_forward_head(x)

    return VitModule()


def timm_key(k):
    p = "coca.img_encoder."
    return p + k[len(p):].replace("__", ".") if k.startswith(p) else k


def grid_weight(rs, key, shape):
    """(int8 levels, scale): levels round(N(0, 1)) clipped to +-3; matrices scaled to 2^round(log2(fan_in^-1/2)), vectors to 1/16.
    LayerNorm weights / gammas are 1 + that, the caller adds the one."""
    q = np.clip(np.rint(rs.standard_normal(shape)), -3, 3).astype(np.int8)
    if len(shape) >= 2 and shape[0] > 1:
        fan_in = int(np.prod(shape[1:]))
        return q, np.float32(2.0 ** round(np.log2(fan_in ** -0.5)))
    return q, np.float32(1.0 / 16)


def is_gain(key):
    return key.endswith("gamma") or key.endswith("LayerNorm.weight") or (".norm" in key and key.endswith(".weight"))


def main(reference):
    sys.path.insert(0, ROOT)
    from oracle import ref_harness, ref_models as O
    ref_harness.REFERENCE_ROOT = reference
    M = ref_harness.load_reference()

    torch.use_deterministic_algorithms(True)
    cfg = ref_harness.reference_config(hidden_size=HID, num_hidden_layers=2, num_attention_heads=2, intermediate_size=HID, vocab_size=VOCAB,
                                       max_position_embeddings=96, type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.0,
                                       attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, image_size=IMG,
                                       num_hidden_layers_multimodal=2, num_attention_heads_multimodal=2,
                                       feedforward_multiplication_multimodal=2, caption_loss_weight=1.0, contrastive_loss_weight=1.0)
    model = M.CoCaForPretraining(cfg, image_encoder=make_vit(O), text_encoder=M.RobertaModel(cfg)).eval()
    rs = np.random.RandomState(20221102)
    arrays = {"grad_row_stride." + k: np.int64(v) for k, v in ROW_STRIDE.items()}
    with torch.no_grad():
        for k, v in model.state_dict().items():
            name = timm_key(k)
            if not torch.is_floating_point(v) or k.endswith("inv_freq") or k.endswith(".beta"):
                arrays["wb." + name] = v.numpy().copy()
            elif name == "temperature" or name == "to_logits.1.weight":
                continue          # chosen below; the word table under its other name
            else:
                q, scale = grid_weight(rs, name, tuple(v.shape))
                arrays["wq." + name], arrays["ws." + name] = q, scale
                v.copy_(torch.from_numpy(q.astype(np.float32) * scale) + (1.0 if is_gain(name) else 0.0))
    assert model.to_logits[1].weight is model.coca.text_encoder.embeddings.word_embeddings.weight
    arrays["keys"] = np.frombuffer("\n".join(sorted(timm_key(k) for k in model.state_dict())).encode(), dtype=np.uint8)

    # one set of images for both n, on a grid of halves (bf16-representable, a few bits each in the file)
    images = np.clip(np.rint(2.0 * rs.standard_normal((B, 3, IMG, IMG))), -6, 6).astype(np.float32) / 2.0
    inputs = {}
    for n in NS:
        ids = rs.randint(3, VOCAB, size=(B, n)).astype(np.int64)
        labels = rs.randint(3, VOCAB, size=(B, n)).astype(np.int64)
        mask = np.zeros((B, n), np.int64)
        for b, ln in enumerate(LENS[n]):
            ids[b, ln:], labels[b, ln:], mask[b, :ln] = 0, 0, 1
        ids[:, 0] = 1
        pad = float((labels == 0).mean())
        assert 0.25 <= pad <= 0.75 and (labels[0] != 0).all(), pad
        inputs[n] = dict(input_ids=ids, attention_mask=mask, token_type_ids=np.zeros((B, n), np.int64),
                         position_ids=np.tile(np.arange(n, dtype=np.int64), (B, 1)), labels=labels, images=images)

    def parts(n):
        """the model's loss and, from the same tensors, its two parts and the diagonal softmax probabilities of sim and sim^T"""
        t = {k: torch.from_numpy(v) for k, v in inputs[n].items()}
        total = model(t["input_ids"], t["attention_mask"], t["token_type_ids"], t["position_ids"], images=t["images"], labels=t["labels"])
        with torch.no_grad():
            te, _tt, ie, _it = model.coca(t["input_ids"], t["attention_mask"], t["token_type_ids"], t["position_ids"], t["images"])
            sim = te @ ie.T * model.temperature.exp()
            tgt = torch.arange(B)
            contrastive = 0.5 * (torch.nn.functional.cross_entropy(sim, tgt) + torch.nn.functional.cross_entropy(sim.T, tgt))
            diag = torch.cat((sim.softmax(1).diagonal(), sim.softmax(0).diagonal()))
        return total, total.detach() - contrastive, contrastive, diag

    for step in range(0, 64):
        with torch.no_grad():
            model.temperature.fill_(1.0 - 0.25 * step)
        if all(bool(((d >= 0.02) & (d <= 0.98)).all()) for d in (parts(n)[3] for n in NS)):
            break
    else:
        raise SystemExit("no temperature on the grid keeps the diagonal probabilities inside [0.02, 0.98]")
    arrays["wb.temperature"] = model.temperature.detach().numpy().copy()

    params = {timm_key(k): p for k, p in model.named_parameters()}
    for n in NS:
        model.zero_grad()
        total, caption, contrastive, diag = parts(n)
        assert bool(((diag >= 0.02) & (diag <= 0.98)).all()), diag
        total.backward()
        for k, v in inputs[n].items():
            arrays["in.images" if k == "images" else f"in.{k}.{n}"] = v
        arrays[f"loss.{n}"], arrays[f"caption.{n}"], arrays[f"contrastive.{n}"] = short(total), short(caption), short(contrastive)
        for k in GRADS:
            arrays[f"grad.{k}.{n}"] = short(params[k].grad[::ROW_STRIDE.get(k, 1)])
        print(f"n = {n}: loss {float(total.detach()):.4f} = caption {float(caption):.4f} + contrastive {float(contrastive):.4f}; temperature "
              f"{float(model.temperature):.2f}; diagonal probabilities {float(diag.min()):.3f} .. {float(diag.max()):.3f}")
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "pretrain.npz")
    write_npz(path, arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
