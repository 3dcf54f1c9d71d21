"""Model-level parity on the GPU: the product classes (HIP engine, bf16 activations, fp32 master weights)
loaded with the golden fixtures' seeded weights must reproduce the REFERENCE outputs stored in
tests/golden/*.npz (captured from the reference's own classes) within the bf16 tolerance north_star states:
5e-2 relative (here: relative to the tensor's max magnitude), outputs and parameter gradients alike."""
from types import SimpleNamespace

import os

import pytest
import torch

from golden_util import load_case, weights, vit_cfg

pytestmark = pytest.mark.gpu
TOL = 5e-2
COS_MIN = 0.99           # gradient direction; see check().  Measured (tools/parity_report.py, profiles/r02_parity_report.txt): median 1.0000
# tensors measured below 0.99: none since the two-tower fixtures hold eight samples (round 5; with three, roberta_two_tower_ce's
# embedding LayerNorm.bias -- a sum over a handful of tokens with cancellation -- sat at 0.97)
COS_EXCEPTIONS = {}
# gradient magnitude: |got - want|_max / |want|_max <= 5e-2 (north_star's bf16 bar), against the reference's fp32 gradients (the fixture)
# or -- when the fixture's 3-sample batch makes the tensor a small difference of large sums -- against the gradients the CPU oracle
# produces when it rounds to bf16 where the engine stores bf16 (oracle.ref_models.rounding: weights, linear / LayerNorm / GELU outputs,
# attention probabilities, and the gradients flowing back through them), i.e. against a same-precision run of the reference
# arithmetic.  No multiplier on either.  Tensors that pass neither are named below with the value measured on an MI355X
# (tools/parity_report.py -> profiles/r04_parity_report.txt) and bounded at 1.25 x that value.
GRAD_REL = 5e-2
REL_EXCEPTIONS = {
    # (round 6: the roberta_one_tower_* and roberta_image_two_tower_begin fixtures hold eight samples too -- the six exceptions their
    # three-sample batches needed, head / embedding-table gradients that were sums over a handful of tokens, are gone; and the rounding
    # mode covers the ResNetV2 towers now: the BatchNorm tower's two tensors -- 0.19 / 0.072 from the fp32 gradients -- sit at 0.040 /
    # 0.038 from the same-precision oracle's and need no entry.)
    # The BiT tower (StdConv2d: every layer at full gain -> the ReLU gates that bf16 rounding flips are not the same ones in two bf16
    # implementations with different summation orders): distance to the same-precision oracle, 0.34-0.38 to the fp32 reference
    # (profiles/r06_parity_report.txt; direction against the fp32 reference 0.934 / 0.952 / 0.988)
    ("resnet_bit_two_tower", "img_encoder.stem.conv.weight"): 0.102,
    ("resnet_bit_two_tower", "img_encoder.stages.1.blocks.1.conv2.weight"): 0.130,
    ("resnet_bit_two_tower", "img_encoder.stages.3.blocks.0.conv3.weight"): 0.256,
}
EXCEPTION_HEADROOM = 1.25
MEASURED = []            # (case, kind, key, value) of everything check() compared: printed by tools/parity_report.py


def bf16_oracle_grads(case):
    """the oracle's gradients under bf16 storage rounding (same inputs, same weights as the fixture)"""
    from golden_util import run_oracle
    from oracle import ref_models as O
    sd = weights(case, requires_grad=True)
    with O.rounding(torch.bfloat16):
        run_oracle(case, sd).loss.backward()
    return {k: sd[k].grad for k in case.grads if sd[k].grad is not None}


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def cfg_of(case):
    c = SimpleNamespace(**vars(case.cfg))
    c.initializer_range = 0.02
    c.hidden_act = "gelu"
    return c


def build(case, cls, *args):
    import item_alignment_amd.models as M
    model = getattr(M, cls)(cfg_of(case), *args)
    sd = weights(case)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k for k in missing), missing
    return model.cuda().eval()


def check(case, out, model, tol=TOL, cos_min=None):
    cos_min = COS_MIN if cos_min is None else cos_min
    for k, want in case.outs.items():
        got = getattr(out, k)
        assert got is not None, k
        assert tuple(got.shape) == tuple(want.shape), (k, got.shape, want.shape)
        MEASURED.append((case.name, "out rel", k, rel(got.detach(), want)))
        assert rel(got.detach(), want) < tol, (case.name, k, rel(got.detach(), want))
    if case.grads:
        model.param_arena.zero_grad()
        out.loss.backward()
        torch.cuda.synchronize()
        params = dict(model.named_parameters())
        # direction: cosine >= 0.99 against the fp32 reference gradient; magnitude: GRAD_REL (above).  Kernel-level backward parity is
        # checked tighter in test_kernels_gpu.py / test_engine_gpu.py against same-precision inputs.
        same_precision = None
        for k, want in case.grads.items():
            got = params[k].grad
            assert torch.isfinite(got).all(), k
            a, b = got.float().cpu().flatten(), want.float().flatten()
            c = (torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)).item()
            r32 = rel(got, want)
            MEASURED.append((case.name, "grad cos", k, c))
            MEASURED.append((case.name, "grad rel", k, r32))
            assert c > min(cos_min, COS_EXCEPTIONS.get((case.name, k), 1.0)), (case.name, "grad cosine", k, c)
            if r32 <= GRAD_REL:
                continue
            if same_precision is None:
                same_precision = bf16_oracle_grads(case)
            r16 = ((got.float().cpu() - same_precision[k]).abs().max() / (want.abs().max() + 1e-6)).item() if k in same_precision else float("inf")
            MEASURED.append((case.name, "grad rel-bf16-oracle", k, r16))
            if r16 <= GRAD_REL:
                continue
            named = REL_EXCEPTIONS.get((case.name, k))
            assert named is not None and min(r32, r16) <= EXCEPTION_HEADROOM * named, (case.name, "grad", k, "vs fp32", r32, "vs bf16 oracle", r16,
                                                                                        "named bound", named)


def g(case, k):
    v = case.inputs.get(k)
    return None if v is None else v.cuda()


@pytest.mark.parametrize("name", ["roberta_one_tower_cls_ce", "roberta_one_tower_cls12_cat", "roberta_one_tower_cls12_avg",
                                  "roberta_one_tower_vecsim_cosine", "roberta_one_tower_vecsim_l2_bce", "roberta_one_tower_vecsim_ip_hinge",
                                  "roberta_one_tower_aux"])
def test_roberta_one_tower(gpu, name):
    from golden_util import pair_list
    case = load_case(name)
    model = build(case, "RobertaOneTower")
    labels = g(case, "labels").float() if case.cfg.loss_type == "bce" else g(case, "labels")
    out = model(input_ids=g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"),
                position_ids=None, labels=labels, output_hidden_states=True, image_indices=pair_list(case))
    check(case, out, model)
    for k, idx in (("hidden0", 0), ("hidden1", 1), ("hidden_last", -1)):
        if k not in case.extra:
            continue
        m = g(case, "attention_mask").bool().cpu()
        got, want = out.hidden_states[idx].float().cpu(), case.extra[k]
        assert rel(got[m], want[m]) < TOL, (k, rel(got[m], want[m]))


@pytest.mark.parametrize("lt", ["ce", "cosine", "hinge", "euclidean"])
def test_roberta_two_tower(gpu, lt):
    case = load_case(f"roberta_two_tower_{lt}")
    model = build(case, "RobertaTwoTower")
    out = model(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask_1"), token_type_ids_1=g(case, "token_type_ids_1"),
                input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask_2"), token_type_ids_2=g(case, "token_type_ids_2"),
                labels=g(case, "labels"))
    check(case, out, model)


@pytest.mark.parametrize("name", ["pkgm_one_tower", "pkgm_one_tower_proj"])
def test_pkgm_one_tower(gpu, name):
    case = load_case(name)
    model = build(case, "PKGMOneTower")
    out = model(input_ids=g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"),
                position_ids=g(case, "position_ids"), labels=g(case, "labels"))
    check(case, out, model)


def test_pkgm_two_tower(gpu):
    case = load_case("pkgm_two_tower")
    model = build(case, "PKGMTwoTower")
    out = model(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask"), token_type_ids_1=g(case, "token_type_ids"),
                position_ids_1=g(case, "position_ids"), input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask"),
                token_type_ids_2=g(case, "token_type_ids"), position_ids_2=g(case, "position_ids"), labels=g(case, "labels"))
    check(case, out, model)


@pytest.mark.parametrize("name", ["roberta_image_one_tower_begin", "roberta_image_one_tower_end"])
def test_roberta_image_one_tower(gpu, name):
    case = load_case(name)
    model = build(case, "RobertaImageOneTower")
    out = model(input_ids=g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"),
                position_ids=None, labels=g(case, "labels"), output_hidden_states=True, inputs_embeds=[g(case, "img1"), g(case, "img2")],
                image_indices=g(case, "image_indices"))
    check(case, out, model)


def test_roberta_image_two_tower(gpu):
    case = load_case("roberta_image_two_tower_begin")
    model = build(case, "RobertaImageTwoTower")
    out = model(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask_1"), token_type_ids_1=g(case, "token_type_ids_1"),
                position_ids_1=None, images_1=g(case, "img1"), input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask_2"),
                token_type_ids_2=g(case, "token_type_ids_2"), position_ids_2=None, images_2=g(case, "img2"), labels=g(case, "labels"))
    check(case, out, model)


def test_coca_sum(gpu):
    import item_alignment_amd.models as M
    case = load_case("coca_sum")
    v = vit_cfg(case)
    cfg = cfg_of(case)
    text = M.RobertaModel(cfg)
    vit = M.VisionTransformer(img_size=v.image_size, patch_size=v.patch_size, embed_dim=v.embed_dim, depth=v.depth, num_heads=v.num_heads)
    model = M.CoCaForItemAlignment(cfg, vit, text)
    missing, unexpected = model.load_state_dict(weights(case), strict=False)
    assert not unexpected, unexpected
    assert all(("position_ids" in k or "pooler" in k or ".head." in k) for k in missing), missing
    model = model.cuda().eval()
    out = model(g(case, "input_ids_1"), g(case, "attention_mask_1"), g(case, "token_type_ids_1"), None, g(case, "img1"),
                g(case, "input_ids_2"), g(case, "attention_mask_2"), g(case, "token_type_ids_2"), None, g(case, "img2"), labels=g(case, "labels"))
    check(case, out, model)


def test_coca_sum_two_streams(gpu):
    """IA_TOWER_STREAMS=1 (image tower on a second HIP stream, forward and backward): same outputs and gradients."""
    import item_alignment_amd.models as M
    from item_alignment_amd.models import multimodal
    case = load_case("coca_sum")
    v = vit_cfg(case)
    cfg = cfg_of(case)
    old = multimodal.TOWER_STREAMS
    multimodal.TOWER_STREAMS = True
    try:
        text = M.RobertaModel(cfg)
        vit = M.VisionTransformer(img_size=v.image_size, patch_size=v.patch_size, embed_dim=v.embed_dim, depth=v.depth, num_heads=v.num_heads)
        model = M.CoCaForItemAlignment(cfg, vit, text)
        model.load_state_dict(weights(case), strict=False)
        model = model.cuda().eval()
        args = (g(case, "input_ids_1"), g(case, "attention_mask_1"), g(case, "token_type_ids_1"), None, g(case, "img1"),
                g(case, "input_ids_2"), g(case, "attention_mask_2"), g(case, "token_type_ids_2"), None, g(case, "img2"))
        for _ in range(3):                      # repeated steps: stream hand-over of inputs, arenas and the allocator
            out = model(*args, labels=g(case, "labels"))
            check(case, out, model)
            model.param_arena.adamw_step(0.0)   # lr 0: exercises the join before the optimiser without moving the weights
        assert len(model.param_arena.side_streams) == 1
    finally:
        multimodal.TOWER_STREAMS = old


def test_coca_cross_attn(gpu):
    """--ensemble cross_attn: rotary multi-query ParallelTransformerBlock + CrossAttention over the image tokens
    (reference multimodal.py:529-706, 1003-1013), golden captured from the reference classes."""
    import item_alignment_amd.models as M
    case = load_case("coca_cross_attn")
    v = vit_cfg(case)
    cfg = cfg_of(case)
    text = M.RobertaModel(cfg)
    vit = M.VisionTransformer(img_size=v.image_size, patch_size=v.patch_size, embed_dim=v.embed_dim, depth=v.depth, num_heads=v.num_heads)
    model = M.CoCaForItemAlignment(cfg, vit, text)
    sd = weights(case)
    assert any(k.startswith("multimodal_layers.1.1.fn.ff.2.weight") for k in sd)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(("position_ids" in k or "pooler" in k or ".head." in k or "inv_freq" in k) for k in missing), missing
    model = model.cuda().eval()
    out = model(g(case, "input_ids_1"), g(case, "attention_mask_1"), g(case, "token_type_ids_1"), None, g(case, "img1"),
                g(case, "input_ids_2"), g(case, "attention_mask_2"), g(case, "token_type_ids_2"), None, g(case, "img2"), labels=g(case, "labels"))
    check(case, out, model)


@pytest.mark.parametrize("name", ["nfnet_two_tower", "resnet_two_tower", "resnet_bit_two_tower", "vit_two_tower"])
def test_image_two_tower_wrappers_vs_reference(gpu, name):
    """NFNetTwoTower / ResNetTwoTower / VitTwoTower against golden vectors captured from the REFERENCE's own wrapper classes
    (src/models/image.py:212-294, :298-378, :418-499; oracle/gen_golden_r2.py wrappers).  The encoder handed to the reference class
    evaluates the oracle's restatement of the timm tower, so the wrapper logic (pooling calls, pair head, probs[:, 0] / probs[:, 1] as
    embeds, loss) is pinned by the reference while the tower arithmetic stays parity-unpinned (timm is absent offline)."""
    import item_alignment_amd.models as M
    from golden_util import NARROW_BIT, NARROW_NFNET, NARROW_RESNET, TINY_VIT
    case = load_case(name)
    cfg = cfg_of(case)
    if name.startswith("nfnet"):
        from item_alignment_amd.models.nfnet import NormFreeNet
        model = M.NFNetTwoTower(cfg, NormFreeNet(NARROW_NFNET.depths, NARROW_NFNET.channels, 1.0))
    elif name.startswith("resnet_bit"):
        # the BiT names (resnetv2_*_bitm) take the same `"resnet" in args.model_name` branch of finetune_image.py:215-216
        from item_alignment_amd.models.resnetv2 import ResNetV2
        model = M.ResNetTwoTower(cfg, ResNetV2(NARROW_BIT.layers, NARROW_BIT.channels, stem_chs=NARROW_BIT.stem_chs, bit=True))
    elif name.startswith("resnet"):
        from item_alignment_amd.models.resnetv2 import ResNetV2
        model = M.ResNetTwoTower(cfg, ResNetV2(NARROW_RESNET.layers, NARROW_RESNET.channels, stem_chs=NARROW_RESNET.stem_chs))
    else:
        v = TINY_VIT
        model = M.VitTwoTower(cfg, M.VisionTransformer(img_size=v.image_size, patch_size=v.patch_size, embed_dim=v.embed_dim, depth=v.depth,
                                                       num_heads=v.num_heads))
    missing, unexpected = model.load_state_dict(weights(case), strict=False)
    assert not unexpected, unexpected
    assert all((".head." in k or "running_" in k or "num_batches" in k) for k in missing), missing
    model = model.cuda().eval()
    out = model(g(case, "images_1"), g(case, "images_2"), g(case, "labels"))
    # ReLU towers in bf16 flip gates near zero: direction of deep-layer gradients is looser there -- and looser
    # still in the BiT tower, whose standardised weights give every layer full gain whatever the scale of the seeded weights (the CPU
    # oracle's own gradients move to cosine 0.93 when it rounds its activations to bf16: tests/test_oracle_golden.py)
    check(case, out, model, cos_min=0.90 if name.startswith("resnet_bit") else 0.97 if name.startswith("resnet") else None)


def test_vit_tokens_vs_transformers_vit(gpu):
    """The HIP ViT tower against transformers.ViTModel's output on the same seeded weights (tests/golden/vit_hf_crosscheck.npz,
    oracle/gen_golden_r2.py vit_hf): a third-party cross-check of the tower arithmetic, not a pin by the reference."""
    import item_alignment_amd.models as M
    case = load_case("vit_hf_crosscheck")
    c = case.cfg
    vit = M.VisionTransformer(img_size=c.image_size, patch_size=c.patch_size, embed_dim=c.embed_dim, depth=c.depth, num_heads=c.num_heads)
    missing, unexpected = vit.load_state_dict({k[2:]: v for k, v in weights(case).items()}, strict=False)
    assert not unexpected and all(k.startswith("head.") for k in missing), (missing, unexpected)
    vit = vit.cuda().eval()
    with torch.no_grad():
        tok = vit.forward_features(g(case, "images"))
    r = rel(tok, case.outs["tokens"])
    MEASURED.append((case.name, "out rel", "tokens", r))
    assert r < TOL, r


def test_24_layer_stack_bf16_drift(gpu):
    """All 24 layers of roberta_large.json (config C2 shapes: B = 2, L = 510) in the bf16 engine against the fp32 reference's
    hidden states (tests/golden/roberta_large_24_layers.npz): the error after 1, 6, 12, 18 and 24 layers stays inside the bf16
    tolerance north_star states (5e-2 of the tensor's max magnitude) - i.e. bf16 rounding does not compound over depth."""
    import item_alignment_amd.models as M
    case = load_case("roberta_large_24_layers")
    model = M.RobertaModel(cfg_of(case), add_pooling_layer=False)
    model.load_state_dict(weights(case), strict=False)
    model = model.cuda().eval()
    with torch.no_grad():
        out = model(g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"))
    hs = out.hidden_states
    m = g(case, "attention_mask").bool().cpu()[:, ::15]
    for layer in (0, 1, 6, 12, 18, 24):
        got, want = hs[layer][:, ::15, ::16].float().cpu(), case.extra[f"h{layer}_sub"]
        r = rel(got[m], want[m])
        MEASURED.append((case.name, "out rel", f"hidden[{layer}]", r))
        assert r < TOL, (layer, r)


def test_full_width_layer(gpu):
    """roberta_large geometry, one layer, L = 510 (the C2 shapes): hidden states vs the reference subsample."""
    import item_alignment_amd.models as M
    case = load_case("roberta_large_one_layer")
    model = M.RobertaModel(cfg_of(case), add_pooling_layer=False)
    model.load_state_dict(weights(case), strict=False)
    model = model.cuda().eval()
    with torch.no_grad():
        out = model(g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"))
    hs = out.hidden_states
    assert rel(hs[0][0, ::16, ::16], case.extra["h0_sub"]) < TOL
    assert rel(hs[1][0, :480:16, ::16], case.extra["h1_sub"][:30]) < TOL
    assert rel(hs[1][0, :4, :], case.extra["h1_rows"]) < TOL


def test_train_step_decreases_loss_and_matches_adamw(gpu):
    """A few fused-AdamW steps: loss goes down, and one step's parameter update equals torch.optim.AdamW's."""
    case = load_case("roberta_two_tower_ce")
    model = build(case, "RobertaTwoTower").train()
    arena = model.param_arena
    args = dict(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask_1"), token_type_ids_1=g(case, "token_type_ids_1"),
                input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask_2"), token_type_ids_2=g(case, "token_type_ids_2"),
                labels=g(case, "labels"))
    model.eval()
    arena.zero_grad()
    loss0 = model(**args).loss
    loss0.backward()
    p = dict(model.named_parameters())["classifier.out_proj.weight"]
    ref_p = p.detach().clone().requires_grad_(True)
    ref_p.grad = p.grad.detach().clone()
    opt = torch.optim.AdamW([ref_p], lr=1e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=1e-5)
    opt.step()
    arena.adamw_step(1e-4)
    torch.cuda.synchronize()
    assert torch.allclose(p.detach(), ref_p.detach(), atol=1e-7, rtol=1e-5)
    losses = [loss0.item()]
    for _ in range(6):                      # (1e-3 makes the eight-sample fixture's loss jump about; the reference trains at 1e-5)
        arena.zero_grad()
        l = model(**args).loss
        l.backward()
        arena.adamw_step(1e-4)
        losses.append(l.item())
    assert losses[-1] < losses[0], losses


def test_fused_adamw_parameter_groups_match_torch(gpu):
    """The fused arena AdamW against torch.optim.AdamW with the reference's two parameter groups (finetune_multimodal.py:296-308:
    names containing "bias" or "LayerNorm.weight" get weight_decay 0).  Covers a decayed weight, a bias, a LayerNorm.weight and a
    CoCa-style `norm.gamma`, which the reference's name rule does NOT exempt (quirk A17: it is decayed); weight_decay is set large
    so a wrong group shows; two steps exercise the moment buffers and the bias correction; grad_scale = the 1/world factor."""
    from item_alignment_amd.arena import ParamArena

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dense = torch.nn.Linear(96, 80)
            self.LayerNorm = torch.nn.LayerNorm(80)
            self.norm = torch.nn.Module()
            self.norm.gamma = torch.nn.Parameter(torch.ones(80))

    torch.manual_seed(3)
    net = Net()
    for q in net.parameters():
        q.data.normal_(0, 0.5)
    ref = {n: q.detach().clone().requires_grad_(True) for n, q in net.named_parameters()}
    arena = ParamArena(net, "cuda")
    no_decay = ("bias", "LayerNorm.weight")
    wd, lr, scale = 0.1, 1e-2, 0.5
    opt = torch.optim.AdamW([{"params": [q for n, q in ref.items() if not any(nd in n for nd in no_decay)], "weight_decay": wd},
                             {"params": [q for n, q in ref.items() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}],
                            lr=lr, betas=(0.9, 0.98), eps=1e-8)
    params = dict(net.named_parameters())
    for step in range(2):
        for n, q in params.items():
            gr = torch.randn(q.shape, generator=torch.Generator().manual_seed(10 * step + len(n)))
            q.grad.copy_(gr.cuda())
            ref[n].grad = gr * scale
        opt.step()
        arena.adamw_step(lr, weight_decay=wd, grad_scale=scale)
    torch.cuda.synchronize()
    assert set(params) == {"dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias", "norm.gamma"}
    for n, q in params.items():
        assert torch.allclose(q.detach().cpu(), ref[n].detach(), atol=2e-6, rtol=1e-5), n
        # the bf16 shadow the GEMMs read follows the master weights
        assert torch.equal(arena.shadow_of(q).float().cpu(), q.detach().cpu().to(torch.bfloat16).float()), n
    # the decay really distinguishes the groups at this setting
    g0 = ref["norm.gamma"].detach()
    assert not torch.allclose(g0, (g0 + lr * wd * g0), atol=1e-7)


def test_nfnet_tower_vs_oracle(gpu):
    """ECA-NFNet tower (reference image.py:191-199,253-257; timm NormFreeNet) against the CPU oracle restatement on a
    narrow instance of the same architecture (timm is absent offline, so the reference cannot pin this tower: the oracle
    follows timm 0.6.5's published definitions — parity unpinned).  bf16 tolerance 5e-2 on the pooled
    features; parameter gradients by direction (cosine >= 0.97) as in check()."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ref_models as O
    from oracle.weights import seeded_state_dict
    from item_alignment_amd.models.nfnet import NormFreeNet
    ncfg = SimpleNamespace(depths=(1, 2, 1, 1), channels=(256, 512, 512, 512), stem_chs=128, group_size=64, bottle_ratio=0.25,
                           num_features=512, alpha=0.2, attn_gain=2.0, eps=1e-5, ch_div=8)
    spec = O.nfnet_state_spec(ncfg, prefix="e")
    sd = seeded_state_dict(spec, 21, scale=0.5)
    g = torch.Generator().manual_seed(5)
    images = torch.randn((2, 3, 64, 64), generator=g)
    wts = torch.randn((2, 512), generator=g)
    # oracle (fp32, CPU)
    ref_sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.nfnet_global_pool(O.nfnet_forward_features(ref_sd, "e", ncfg, images))
    (ref * wts).sum().backward()
    # HIP tower
    net = NormFreeNet(ncfg.depths, ncfg.channels, 1.0)
    missing, unexpected = net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("head.fc") for k in missing), (missing, unexpected)
    net = net.cuda().train()
    out = net(images.cuda())
    assert tuple(out.shape) == (2, 512)
    assert rel(out.detach(), ref.detach()) < TOL, rel(out.detach(), ref.detach())
    net.param_arena.zero_grad()
    (out * wts.cuda()).sum().backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    for k in ["stem.conv1.weight", "stem.conv2.gain", "stem.conv4.bias", "stages.0.0.downsample.conv.weight", "stages.1.0.conv2.weight",
              "stages.1.1.conv2b.weight", "stages.1.1.conv1.gain", "stages.2.0.attn_last.conv.weight", "stages.3.0.conv3.weight",
              "final_conv.weight", "final_conv.bias"]:
        got, want = params[k].grad.float().cpu().flatten(), ref_sd["e." + k].grad.flatten()
        assert torch.isfinite(got).all(), k
        c = (torch.dot(got, want) / (got.norm() * want.norm() + 1e-30)).item()
        assert c > 0.97, ("grad cosine", k, c)
        assert rel(got, want) < 0.25, ("grad", k, rel(got, want))


def _resnet_small():
    return SimpleNamespace(layers=(1, 2, 1, 1), channels=(64, 128, 256, 256), stem_chs=32, bottle_ratio=0.25, eps=1e-5, momentum=0.1,
                           num_features=256)


def test_resnetv2_tower_vs_oracle(gpu):
    """Pre-activation ResNetV2 tower (reference image.py:337-341; timm resnetv2_50 family with BatchNormAct2d) against the CPU
    oracle restatement on a narrow instance of the same architecture, training mode (batch statistics).  timm is absent
    offline: parity unpinned, as for the NFNet tower.  bf16 tolerance 5e-2 on the pooled features, running statistics within
    2e-2.  Parameter gradients by direction: >= 0.97 in the last stage, >= 0.90 further down.  The looser bound is the ReLU:
    a bf16 pre-activation within rounding distance of zero lands on the other side of the gate than the fp32 oracle's
    (measured: 0.07-0.35 % of the elements per BatchNormAct2d), each flipped element carries a full-size gradient error, i.e.
    ~sqrt(0.003) = 6 % rms per ReLU layer, and the tower stacks 16 of them; the smooth SiLU / GELU towers do not have this.
    The kernels themselves are checked against torch on identical inputs in test_kernels_gpu.py."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ref_models as O
    from oracle.weights import seeded_state_dict
    from item_alignment_amd.models.resnetv2 import ResNetV2
    rcfg = _resnet_small()
    sd = seeded_state_dict(O.resnetv2_state_spec(rcfg, prefix="e"), 31, scale=0.08)
    g = torch.Generator().manual_seed(6)
    images = torch.randn((4, 3, 128, 128), generator=g)
    wts = torch.randn((4, 256), generator=g)
    ref_sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    stats = O.resnetv2_running_stats(rcfg, "e")
    ref = O.resnetv2_forward_features(ref_sd, "e", rcfg, images, True, stats).mean((2, 3))
    (ref * wts).sum().backward()

    net = ResNetV2(rcfg.layers, rcfg.channels, stem_chs=rcfg.stem_chs)
    missing, unexpected = net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("head.fc") or "running_" in k or "num_batches" in k for k in missing), (missing, unexpected)
    net = net.cuda().train()
    out = net(images.cuda())
    assert tuple(out.shape) == (4, 256)
    assert rel(out.detach(), ref.detach()) < TOL, rel(out.detach(), ref.detach())
    bufs = dict(net.named_buffers())
    for k in ["stages.0.blocks.0.norm1", "stages.1.blocks.1.norm3", "norm"]:
        assert rel(bufs[k + ".running_mean"], stats["e." + k + ".running_mean"]) < 2e-2, k
        assert rel(bufs[k + ".running_var"], stats["e." + k + ".running_var"]) < 2e-2, k
        assert int(bufs[k + ".num_batches_tracked"]) == 1
    net.param_arena.zero_grad()
    (out * wts.cuda()).sum().backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    for k in ["stem.conv.weight", "stages.0.blocks.0.downsample.conv.weight", "stages.0.blocks.0.norm1.weight", "stages.0.blocks.0.conv2.weight",
              "stages.1.blocks.0.conv2.weight", "stages.1.blocks.0.downsample.conv.weight", "stages.1.blocks.1.norm1.bias",
              "stages.1.blocks.1.conv1.weight", "stages.2.blocks.0.norm3.weight", "stages.3.blocks.0.conv3.weight", "norm.weight", "norm.bias"]:
        got, want = params[k].grad.float().cpu().flatten(), ref_sd["e." + k].grad.flatten()
        assert torch.isfinite(got).all(), k
        c = (torch.dot(got, want) / (got.norm() * want.norm() + 1e-30)).item()
        last = k.startswith("stages.3") or k.startswith("norm")
        assert c > (0.97 if last else 0.90), ("grad cosine", k, c)
        assert 0.8 < (got.norm() / want.norm()).item() < 1.25, ("grad norm", k)
    # eval mode uses the running statistics
    net.eval()
    with torch.no_grad():
        ev = net(images.cuda())
    ref_ev = O.resnetv2_forward_features(sd, "e", rcfg, images, False, stats).mean((2, 3))
    assert rel(ev, ref_ev) < TOL, rel(ev, ref_ev)


def test_bit_tower_vs_oracle_and_transformers_bit(gpu):
    """The BiT ResNetV2 tower (`--model_name resnetv2_50x3_bitm_in21k` of finetune_image.py:23; timm resnetv2.py `_create_resnetv2_bit`:
    StdConv2d eps 1e-8 + GroupNormAct(32) + the zero-ring stem) on a narrow instance of the architecture, against (a) the features, the
    pooled output and nine parameter gradients of transformers.BitModel on the same seeded weights (tests/golden/bit_hf_crosscheck.npz,
    an independent implementation of the published architecture; the CPU oracle reproduces it to fp32 round-off,
    test_oracle_golden.py) and (b) eval mode = training mode (GroupNorm keeps no batch statistics).  bf16 bar 5e-2 on the outputs;
    gradients by direction and norm: >= 0.97 in the last stage / >= 0.90 further down against the fp32 gradients (the oracle's own
    gradients under bf16 storage rounding sit at 0.93: test_oracle_golden.py), and >= 0.97 everywhere against that same-precision
    oracle (measured 0.981-1.000)."""
    from item_alignment_amd.models.resnetv2 import ResNetV2
    case = load_case("bit_hf_crosscheck")
    c = case.cfg
    sd = weights(case)
    net = ResNetV2(tuple(c.layers), tuple(c.channels), stem_chs=c.stem_chs, bit=True)
    missing, unexpected = net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("head.fc") for k in missing), (missing, unexpected)
    assert not any("running_" in k for k in net.state_dict())
    net = net.cuda().train()
    images, wts = g(case, "images"), g(case, "wts")
    fmap = net.forward_features(images)
    feat = fmap.t.view(fmap.B, fmap.H, fmap.W, -1).permute(0, 3, 1, 2)
    r = rel(feat.detach(), case.outs["features"])
    MEASURED.append((case.name, "out rel", "features", r))
    assert r < TOL, r
    out = net(images)
    r = rel(out.detach(), case.outs["pooled"])
    MEASURED.append((case.name, "out rel", "pooled", r))
    assert tuple(out.shape) == (3, c.num_features) and r < TOL, r
    net.param_arena.zero_grad()
    (out * wts).sum().backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    # the same-precision yardstick: the CPU oracle rounding to bf16 where the engine stores bf16 (oracle.ref_models.rounding)
    from oracle import ref_models as O
    sd16 = weights(case, requires_grad=True)
    with O.rounding(torch.bfloat16):
        f16 = O.resnetv2_forward_features(sd16, "e", c, case.inputs["images"])
        (f16.mean((2, 3)) * case.inputs["wts"]).sum().backward()
    for k, want in case.grads.items():
        got = params[k].grad.float().cpu().flatten()
        want = want.flatten()
        assert torch.isfinite(got).all(), k
        cos = (torch.dot(got, want) / (got.norm() * want.norm() + 1e-30)).item()
        g16 = sd16["e." + k].grad.flatten()
        cos16 = (torch.dot(got, g16) / (got.norm() * g16.norm() + 1e-30)).item()
        MEASURED.append((case.name, "grad cos", k, cos))
        MEASURED.append((case.name, "grad rel", k, rel(got, want)))
        MEASURED.append((case.name, "grad cos-bf16-oracle", k, cos16))
        MEASURED.append((case.name, "grad rel-bf16-oracle", k, ((got - g16).abs().max() / (want.abs().max() + 1e-6)).item()))
        last = k.startswith("stages.3") or k.startswith("norm")
        assert cos > (0.97 if last else 0.90), ("grad cosine", k, cos)
        assert cos16 > 0.97, ("grad cosine against the bf16-rounding oracle", k, cos16)          # measured 0.981 .. 1.000
        assert 0.8 < (got.norm() / want.norm()).item() < 1.25, ("grad norm", k)
    net.eval()
    with torch.no_grad():
        ev = net(images)
    assert torch.equal(ev, out.detach())


def test_resnet_two_tower_normalises_each_tower_separately(gpu):
    """ResNetTwoTower (reference image.py:337-378): the reference runs the encoder once per tower, so BatchNorm statistics are
    per tower; the HIP wrapper runs one 2B batch in two segments and must give the same loss / probabilities and the same
    running statistics as the two calls of the oracle."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import item_alignment_amd.models as M
    from oracle import ref_models as O
    from oracle.weights import seeded_state_dict
    from item_alignment_amd.models.resnetv2 import ResNetV2
    rcfg = _resnet_small()
    cfg = SimpleNamespace(num_labels=2, hidden_dropout_prob=0.0, loss_type="ce", loss_margin=0.0, classification_method="cls", hidden_size=256)
    spec = O.resnetv2_state_spec(rcfg, prefix="img_encoder") + [("classifier.out_proj.weight", (2, 512)), ("classifier.out_proj.bias", (2,))]
    sd = seeded_state_dict(spec, 41, scale=0.08)
    g = torch.Generator().manual_seed(8)
    im1, im2 = torch.randn((3, 3, 96, 96), generator=g), torch.randn((3, 3, 96, 96), generator=g) * 1.5 + 0.3
    labels = torch.tensor([1, 0, 1])
    stats = O.resnetv2_running_stats(rcfg, "img_encoder")
    ref = O.resnetv2_two_tower(sd, cfg, rcfg, im1, im2, labels, training=True, stats=stats)
    model = M.ResNetTwoTower(cfg, ResNetV2(rcfg.layers, rcfg.channels, stem_chs=rcfg.stem_chs))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    model = model.cuda().train()
    out = model(im1.cuda(), im2.cuda(), labels.cuda())
    assert abs(out.loss.item() - ref.loss.item()) < 3e-2, (out.loss.item(), ref.loss.item())
    assert rel(out.probs.float().cpu(), ref.probs) < TOL
    bufs = dict(model.named_buffers())
    k = "img_encoder.stages.1.blocks.0.norm2"
    assert rel(bufs[k + ".running_mean"].cpu(), stats[k + ".running_mean"]) < 2e-2
    assert rel(bufs[k + ".running_var"].cpu(), stats[k + ".running_var"]) < 2e-2
    assert int(bufs[k + ".num_batches_tracked"]) == 2
    model.param_arena.zero_grad()
    out.loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(model.img_encoder.stem.conv.weight.grad).all()


@pytest.mark.parametrize("name,cls", [("roberta_one_tower_cls_ce", "RobertaOneTower"), ("roberta_two_tower_ce", "RobertaTwoTower")])
def test_unpadded_text_tower_matches_padded(gpu, name, cls, monkeypatch):
    """IA_UNPAD=1 (models/text.py RobertaModel._forward_unpadded): dropping the padded rows before the embedding kernel and running
    every layer on the packed tokens gives the reference golden outputs / gradients like the padded run does, and hidden states
    come back in the padded shape."""
    import item_alignment_amd.models.text as T
    case = load_case(name)
    monkeypatch.setattr(T, "UNPAD", True)
    model = build(case, cls)
    if cls == "RobertaOneTower":
        out = model(input_ids=g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"),
                    position_ids=None, labels=g(case, "labels"), output_hidden_states=True)
        m = g(case, "attention_mask").bool().cpu()
        got, want = out.hidden_states[-1].float().cpu(), case.extra["hidden_last"]
        assert rel(got[m], want[m]) < TOL
        assert got[~m].abs().max().item() == 0.0
    else:
        out = model(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask_1"), token_type_ids_1=g(case, "token_type_ids_1"),
                    input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask_2"), token_type_ids_2=g(case, "token_type_ids_2"),
                    labels=g(case, "labels"))
    check(case, out, model)


def test_nfnet_two_tower_chunked_batch_equals_whole(gpu):
    """NFNetTwoTower runs batches beyond the kernels' 2 GiB operand window in image chunks (the tower has no batch statistics):
    chunks of one image must give the loss and the gradients of the whole batch."""
    import item_alignment_amd.models as M
    from item_alignment_amd.models.nfnet import NormFreeNet
    cfg = SimpleNamespace(num_labels=2, hidden_dropout_prob=0.0, loss_type="ce", loss_margin=0.0, classification_method="cls", hidden_size=512)
    torch.manual_seed(3)
    model = M.NFNetTwoTower(cfg, NormFreeNet((1, 1, 1, 1), (256, 512, 512, 512), 1.0)).cuda().train()
    g = torch.Generator().manual_seed(9)
    im1, im2 = torch.randn((3, 3, 64, 64), generator=g).cuda(), torch.randn((3, 3, 64, 64), generator=g).cuda()
    labels = torch.tensor([1, 0, 1]).cuda()
    grads = []
    losses = []
    for max_images in (None, 0):                    # one pass; 0 -> one image per chunk
        model.max_images = max_images
        out = model(im1, im2, labels)
        model.param_arena.zero_grad()
        out.loss.backward()
        torch.cuda.synchronize()
        losses.append(out.loss.item())
        grads.append(model.img_encoder.stem.conv2.weight.grad.float().clone())
    assert abs(losses[0] - losses[1]) < 2e-3, losses
    assert rel(grads[1], grads[0]) < 2e-2


def test_coca_with_unpadding_enabled(gpu, monkeypatch):
    """IA_UNPAD=1 on the CoCa wrapper: `ensemble=sum` reads only the text CLS, so its text tower runs unpadded; `cross_attn` feeds ALL
    text positions (padding included, there is no padding mask in the reference's multimodal blocks) to the multimodal layers,
    so it must keep the padded tower run — both still reproduce the reference golden cases."""
    import item_alignment_amd.models.text as T
    monkeypatch.setattr(T, "UNPAD", True)
    test_coca_sum(gpu)
    test_coca_cross_attn(gpu)


def test_train_step_with_dropout_on(gpu):
    """Dropout ON (the bench configuration: hidden 0.1, attention 0.1) through the whole RobertaTwoTower train step.  The engine's masks
    come from a counter-based generator keyed by (step seed, layer, element) -- not torch's stream -- so the reference's masks cannot
    be reproduced bit for bit; what must hold: (a) the same step seed gives the bit-identical loss and gradients (the embedding tables
    included: their rows are summed in a fixed order), a different seed does not; (b) over 256 seeds the mean loss and the mean gradient of the pair head agree with the oracle's (training=True, torch
    dropout, 256 seeds of its own, under bf16 storage rounding) within a few standard errors of the difference (loss: plus the bf16 bias measured with dropout off)."""
    from golden_util import run_oracle
    from item_alignment_amd.models import functional as Fn
    case = load_case("roberta_two_tower_ce")
    assert case.cfg.hidden_dropout_prob == 0.1 and case.cfg.attention_probs_dropout_prob == 0.1
    model = build(case, "RobertaTwoTower").train()
    key = "classifier.out_proj.weight"
    args = dict(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask_1"), token_type_ids_1=g(case, "token_type_ids_1"),
                input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask_2"), token_type_ids_2=g(case, "token_type_ids_2"),
                labels=g(case, "labels"))

    def hip_step(seed):
        Fn.set_step_seed(seed)
        model.param_arena.zero_grad()
        out = model(**args)
        out.loss.backward()
        torch.cuda.synchronize()
        return out.loss.detach().float().cpu().clone(), {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}

    l0, g0 = hip_step(1234)
    l1, g1 = hip_step(1234)
    # bit for bit: the loss and every gradient, the three embedding tables included (each table row is summed over its input rows in
    # one fixed order, embed.hip: emb_seg_piece_kernel / emb_seg_join_kernel)
    tables = [k for k in g0 if k.startswith("roberta.embeddings.") and k.endswith("_embeddings.weight")]
    assert len(tables) == 3
    assert torch.equal(l0, l1), "same step seed must reproduce the loss bit for bit"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), ("same step seed must reproduce this gradient bit for bit", k)
    l2, g2 = hip_step(99)
    assert not torch.equal(l0, l2) and not torch.equal(g0[key], g2[key])
    model.eval()
    le, _ = hip_step(0)                                                     # dropout off: differs from every dropout-on step
    assert not torch.equal(le, l0)
    model.train()

    # 256 seeds per side (round 6; 64 until then).  The 512 z scores below are strongly correlated (the two rows of the head's weight
    # gradient are each other's negatives, every column shares the per-sample logit gradients), so their mean is itself noisy: measured
    # on one box against the bf16-rounding oracle: 64 seeds mean 1.144 / 0.859 below 2, 256 seeds 0.974 / 0.914 -- a real mismatch (a wrong
    # keep probability, a missing 1 / (1 - p)) would GROW with sqrt(n) instead.  IA_DROPOUT_SEEDS overrides n for such diagnostics.
    n = int(os.environ.get("IA_DROPOUT_SEEDS", 256))
    hl, hg = [], []
    for s in range(n):
        l, gr = hip_step(1000 + 7 * s)
        hl.append(l.item()); hg.append(gr[key])
    # The oracle's 64 dropout-on steps run under bf16 STORAGE ROUNDING (oracle.ref_models.rounding: the same places the engine stores
    # bf16), so both samples carry the deterministic bf16-against-fp32 bias and the z scores below need no bias term at all (round 6;
    # the round-5 form subtracted |eval-mode bias| and clamped at zero, which hid any mismatch smaller than that bias in either direction
    # -- advisor finding; subtracting the SIGNED eval-mode bias instead was measured too: mean z 1.10, the part of the bias that dropout
    # itself changes is not in an eval-mode measurement).
    from oracle import ref_models as O
    ol, og = [], []
    for s in range(n):
        torch.manual_seed(5000 + s)
        sd = weights(case, requires_grad=True)
        with O.rounding(torch.bfloat16):
            out = run_oracle(case, sd, training=True)
            out.loss.backward()
        ol.append(out.loss.item()); og.append(sd[key].grad.clone())
    hl, ol = torch.tensor(hl, dtype=torch.float64), torch.tensor(ol, dtype=torch.float64)
    assert hl.std() > 1e-3 and ol.std() > 1e-3                              # dropout really is on in both
    se = (hl.var() / n + ol.var() / n).sqrt().item()
    # (both samples are seeded, so the outcome is fixed for a given build; 3 standard errors leave room for another torch's CPU stream)
    assert abs(hl.mean().item() - ol.mean().item()) <= 3 * se + 1e-3, (hl.mean().item(), ol.mean().item(), se)
    hg, og = torch.stack(hg).double(), torch.stack(og).double()
    # per element of the pair head's weight gradient (2 x 256): z = |difference of the two sample means| / its standard error.
    # Two samplers of the same distribution give |N(0, 1)| scores: mean 0.80, 95 % below 2, the largest of 512 around 3.1
    # (measured with 128 seeds: 0.85 / 0.953 / 3.08); a wrong keep probability or a missing 1 / (1 - p) shifts every one of them.
    z = (hg.mean(0) - og.mean(0)).abs() / (hg.var(0) / n + og.var(0) / n).sqrt()
    print(f"dropout z scores against the bf16-rounding oracle: mean {z.mean().item():.3f}, below 2: {(z < 2).double().mean().item():.3f}, "
          f"max {z.max().item():.2f}; loss means {hl.mean().item():.4f} / {ol.mean().item():.4f}, se {se:.4f}")
    assert z.mean().item() < 1.05, z.mean().item()
    assert (z < 2).double().mean().item() > 0.90, (z < 2).double().mean().item()
    assert z.max().item() < 5.0, z.max().item()
    assert abs(hl.std().item() / ol.std().item() - 1.0) < 0.5              # the spread over masks matches too (0.162 vs 0.158 at 128 seeds)
