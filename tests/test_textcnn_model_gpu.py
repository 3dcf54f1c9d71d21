"""TextCNNTwoTower with its input on the GPU (models/text.py -> Fn.TextCNNTowerFn -> csrc/textcnn.hip): against the reference project's
golden vector, against its own CPU path, and that the forward really goes through the new entry points."""
import copy

import pytest
import torch

from golden_util import load_case, weights
from test_models_gpu import cfg_of

pytestmark = pytest.mark.gpu

TOL = 5e-2            # the project's bf16 bar: max |got - want| / max |want|
NEW_ENTRY_POINTS = ("ia_textcnn_pack_taps", "ia_textcnn_pool_fwd", "ia_textcnn_pool_bwd_w", "ia_textcnn_pool_bwd_x")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def golden_model():
    import item_alignment_amd.models as M
    case = load_case("textcnn_two_tower")
    model = M.TextCNNTwoTower(cfg_of(case), {})
    missing, unexpected = model.load_state_dict(weights(case), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing)
    return case, model.eval()


def call(model, i, device):
    return model(input_ids_1=i["input_ids_1"].to(device), input_ids_2=i["input_ids_2"].to(device), labels=i["labels"].to(device))


class CountCalls:
    """wraps entry points of the loaded library object and counts their calls"""

    def __init__(self, names):
        from item_alignment_amd import _lib
        self.lib, self.names, self.counts, self.saved = _lib.load(), names, {n: 0 for n in names}, {}

    def __enter__(self):
        for n in self.names:
            fn = self.saved[n] = getattr(self.lib, n)

            def wrapper(*a, _fn=fn, _n=n):
                self.counts[_n] += 1
                return _fn(*a)
            setattr(self.lib, n, wrapper)
        return self.counts

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.lib, n, fn)


def test_gpu_model_matches_the_reference_golden_vector(gpu):
    case, model = golden_model()
    model = model.cuda()
    out = call(model, case.inputs, gpu)
    for k, want in case.outs.items():
        got = getattr(out, k)
        assert got.is_cuda and tuple(got.shape) == tuple(want.shape), k
        r = rel(got, want)
        print(f"[textcnn model] out {k}: rel {r:.2e}")
        assert r <= TOL, (k, r)
    out.loss.backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    assert len(case.grads) == 3
    for k, want in case.grads.items():
        got = params[k].grad
        assert got is not None and torch.isfinite(got).all(), k
        a, b = got.float().cpu().flatten(), want.float().flatten()
        cos = (torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)).item()
        r = rel(got, want)
        print(f"[textcnn model] grad {k}: cosine {cos:.5f} rel {r:.2e}")
        assert cos >= 0.99 and r <= TOL, (k, cos, r)
    assert all(p.grad is None for n, p in params.items() if "embedding2" in n)


def test_cpu_path_is_unchanged_bit_for_bit():
    """the model with its input on the CPU computes what it computed before the GPU path existed, bit for bit, outputs and gradients.
    That formula is restated here from torch.nn.functional calls on the bare parameters (no forward of the model's own modules is
    used, so a change to the embedding pipeline, the tower or the head shows)"""
    import torch.nn.functional as F
    from item_alignment_amd.models.base import create_position_ids_from_input_ids
    case, model = golden_model()
    i = case.inputs
    out = call(model, i, "cpu")
    out.loss.backward()
    ref = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in model.named_parameters()}
    pad = case.cfg.pad_token_id

    def embed(ids, p):
        pos = create_position_ids_from_input_ids(ids, pad)
        e = F.embedding(ids, ref[p + "word_embeddings.weight"], padding_idx=pad) + F.embedding(torch.zeros_like(ids), ref[p + "token_type_embeddings.weight"])
        e = e + F.embedding(pos, ref[p + "position_embeddings.weight"], padding_idx=pad)
        return F.layer_norm(e, (e.shape[-1],), ref[p + "LayerNorm.weight"], ref[p + "LayerNorm.bias"], case.cfg.layer_norm_eps)

    def tower(ids):
        x = torch.stack((embed(ids, "textcnn.embedding1."), embed(ids, "textcnn.embedding2.")), dim=1)
        x = [F.relu(F.conv2d(x, ref[f"textcnn.convs1.{s}.weight"], ref[f"textcnn.convs1.{s}.bias"])).squeeze(3) for s in range(len(model.textcnn.convs1))]
        return torch.cat([F.max_pool1d(v, v.size(2)).squeeze(2) for v in x], 1)

    logits = F.linear(torch.cat((tower(i["input_ids_1"]), tower(i["input_ids_2"])), dim=1), ref["classifier.out_proj.weight"], ref["classifier.out_proj.bias"])
    probs = torch.softmax(logits, dim=1)
    loss = F.cross_entropy(logits.view(-1, 2), i["labels"].view(-1))
    loss.backward()
    assert torch.equal(out.logits, logits) and torch.equal(out.probs, probs[:, 1]) and torch.equal(out.loss, loss)
    assert torch.equal(out.src_embeds, probs[:, 0]) and torch.equal(out.tgt_embeds, probs[:, 1])
    for n, p in model.named_parameters():
        assert (p.grad is None) == (ref[n].grad is None), n
        assert p.grad is None or torch.equal(p.grad, ref[n].grad), n


def test_gpu_forward_goes_through_the_new_entry_points(gpu):
    case, model = golden_model()
    model = model.cuda()
    with CountCalls(NEW_ENTRY_POINTS + ("ia_embed_ln_fwd", "ia_gemm_bf16", "ia_pair_head_ce_fwd", "ia_embed_ln_bwd")) as n:
        out = call(model, case.inputs, gpu)
        assert n["ia_textcnn_pack_taps"] == 1 and n["ia_textcnn_pool_fwd"] == 2       # one pack, one pool per tower
        assert n["ia_embed_ln_fwd"] == 4 and n["ia_gemm_bf16"] == 4 and n["ia_pair_head_ce_fwd"] == 1
        out.loss.backward()
        assert n["ia_textcnn_pool_bwd_w"] == 2 and n["ia_textcnn_pool_bwd_x"] == 2 and n["ia_embed_ln_bwd"] == 2
        call(model, case.inputs, gpu)
        assert n["ia_textcnn_pack_taps"] == 1                                        # weights unchanged: the shadow is reused
        with torch.no_grad():
            model.textcnn.convs1[0].weight.mul_(1.0)
        call(model, case.inputs, gpu)
        assert n["ia_textcnn_pack_taps"] == 2                                        # a written weight is repacked
    torch.cuda.synchronize()


def _synthetic(cfg, pairs, L, seed):
    g = torch.Generator().manual_seed(seed)
    ids = [torch.randint(5, cfg.vocab_size, (pairs, L), generator=g) for _ in range(2)]
    for t in ids:
        t[::3, L - 3:] = getattr(cfg, "pad_token_id", 0)                                            # some padded tails
    return dict(input_ids_1=ids[0], input_ids_2=ids[1], labels=torch.randint(0, 2, (pairs,), generator=g))


def test_three_adamw_steps_follow_the_cpu_path(gpu):
    """16 synthetic pairs, dropout off (the two paths draw different masks), TorchAdamW as the CLI builds it: the loss of each step
    stays within 5e-2 of the CPU path's"""
    from item_alignment_amd.train import TorchAdamW
    case, cpu_model = golden_model()
    cpu_model.train()
    for m in cpu_model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    gpu_model = copy.deepcopy(cpu_model).cuda()
    batch = _synthetic(case.cfg, 16, case.inputs["input_ids_1"].shape[1], 9)
    losses = {}
    for name, model, dev in (("cpu", cpu_model, "cpu"), ("gpu", gpu_model, gpu)):
        opt = TorchAdamW(model, 1e-3, 1e-8, 1e-5)
        losses[name] = []
        for _ in range(3):
            opt.zero_grad()
            loss = call(model, batch, dev).loss
            loss.backward()
            opt.step(1.0)
            losses[name].append(float(loss.detach()))
    print(f"[textcnn model] loss trajectories: {losses}")
    assert losses["cpu"][0] != losses["cpu"][2]
    for a, b in zip(losses["cpu"], losses["gpu"]):
        assert abs(a - b) <= 5e-2, losses


def test_no_grad_evaluation_equals_the_training_forward_without_dropout(gpu):
    case, model = golden_model()
    model = model.cuda().train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    train_out = call(model, case.inputs, gpu)
    model.eval()
    with torch.no_grad():
        eval_out = call(model, case.inputs, gpu)
    for k in ("loss", "logits", "probs", "src_embeds", "tgt_embeds"):
        assert torch.equal(getattr(train_out, k).detach(), getattr(eval_out, k)), k
    assert train_out.loss.requires_grad and not eval_out.loss.requires_grad
