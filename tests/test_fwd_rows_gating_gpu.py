"""Who opts into the forward's row skip (ia_layer_cfg::masked_rows_dead bit 2, RobertaModel.forward(padded_rows_unread=True)).

Small golden configs (hidden size 128, two layers): the GEMMs there are below the 256-wide kernel's plan and run every row, the
LayerNorm filter acts at any width, so the skip shows as zeros at the padded positions of the hidden states.

A wrapper whose head reads [CLS] only (RobertaTwoTower, CoCa with ensemble sum) opts in: loss, logits and every parameter gradient
must be torch.equal to the same step with the skip switched off in the library (ia_debug_fwd_rows(0)), and last_hidden_state is zero at
the padded positions.  Everybody else keeps the dense forward, hidden states equal at EVERY position to the ia_debug_fwd_rows(0) run: a
direct RobertaModel call, output_hidden_states=True through a wrapper, vec_sim (the target embedding sits at a fixed, possibly padded
position), the auxiliary task (its spans may reach into the padding) and cross_attn (the multimodal layers attend over all text
positions)."""
import pytest
import torch

from golden_util import load_case, vit_cfg, weights
from test_models_gpu import build, cfg_of, g

pytestmark = pytest.mark.gpu


def run(model, call, skip, text_model):
    """one train-mode step (dropout on, fixed seeds) -> (output, hidden states of the text tower, flag the encoder ran under, gradients)"""
    from item_alignment_amd import _lib
    from item_alignment_amd.models import functional as Fn
    lib = _lib.load()
    seen = {}
    hook = text_model.register_forward_hook(lambda m, a, out: seen.update(hs=[h.detach().clone() for h in out.hidden_states]))
    was = lib.ia_debug_fwd_rows(1 if skip else 0)
    try:
        model.train()
        Fn.set_step_seed(77)
        torch.manual_seed(5)
        model.param_arena.zero_grad()
        out = call(model)
        flag = text_model.encoder.last_stack_rows.masked_rows_dead
        grads = None
        if out.loss is not None:
            out.loss.backward()
            grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
    finally:
        lib.ia_debug_fwd_rows(was)
        hook.remove()
    return out, seen["hs"], flag, grads


def same_step(a, b):
    for k in ("loss", "logits", "probs"):
        x, y = getattr(a[0], k, None), getattr(b[0], k, None)
        if x is not None:
            assert torch.equal(x, y), k
    if a[3] is not None:
        assert a[3].keys() == b[3].keys()
        for n in a[3]:
            assert torch.equal(a[3][n], b[3][n]), n


def two_tower_call(case):
    return lambda m: m(input_ids_1=g(case, "input_ids_1"), attention_mask_1=g(case, "attention_mask_1"), token_type_ids_1=g(case, "token_type_ids_1"),
                       input_ids_2=g(case, "input_ids_2"), attention_mask_2=g(case, "attention_mask_2"), token_type_ids_2=g(case, "token_type_ids_2"),
                       labels=g(case, "labels"))


def test_two_tower_opts_in(gpu):
    case = load_case("roberta_two_tower_ce")
    model = build(case, "RobertaTwoTower")
    model.ensure_arena()
    mask = torch.cat((g(case, "attention_mask_1"), g(case, "attention_mask_2"))).bool()
    assert (~mask).any() and mask.any(dim=1).all()                     # ragged, right-padded
    on, off = run(model, two_tower_call(case), True, model.roberta), run(model, two_tower_call(case), False, model.roberta)
    assert on[2] == 3 and off[2] == 3
    same_step(on, off)
    assert any(v.abs().max().item() > 0 for v in on[3].values())
    for h_on, h_off in zip(on[1][1:], off[1][1:]):                      # every layer's output (hidden_states[0] is the embedding)
        assert torch.equal(h_on[mask], h_off[mask])
        assert h_on[~mask].float().abs().max().item() == 0.0
    assert off[1][-1][~mask].float().abs().max().item() > 0.0           # (the dense forward computes them)


def test_coca_sum_opts_in(gpu):
    import item_alignment_amd.models as M
    case = load_case("coca_sum")
    model, call = coca(case)
    on, off = run(model, call, True, model.coca.text_encoder), run(model, call, False, model.coca.text_encoder)
    assert on[2] == 3
    same_step(on, off)
    mask = torch.cat((g(case, "attention_mask_1"), g(case, "attention_mask_2"))).bool()
    assert torch.equal(on[1][-1][mask], off[1][-1][mask]) and on[1][-1][~mask].float().abs().max().item() == 0.0


def coca(case):
    import item_alignment_amd.models as M
    v, cfg = vit_cfg(case), cfg_of(case)
    text = M.RobertaModel(cfg)
    vit = M.VisionTransformer(img_size=v.image_size, patch_size=v.patch_size, embed_dim=v.embed_dim, depth=v.depth, num_heads=v.num_heads)
    model = M.CoCaForItemAlignment(cfg, vit, text)
    model.load_state_dict(weights(case), strict=False)
    model = model.cuda()
    model.ensure_arena()
    call = lambda m: m(g(case, "input_ids_1"), g(case, "attention_mask_1"), g(case, "token_type_ids_1"), None, g(case, "img1"),
                       g(case, "input_ids_2"), g(case, "attention_mask_2"), g(case, "token_type_ids_2"), None, g(case, "img2"), labels=g(case, "labels"))
    return model, call


def one_tower_call(case, **kw):
    from golden_util import pair_list
    labels = g(case, "labels").float() if case.cfg.loss_type == "bce" else g(case, "labels")
    return lambda m: m(input_ids=g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"),
                       position_ids=None, labels=labels, image_indices=pair_list(case), **kw)


def dense_everywhere(on, off):
    assert (on[2] & 2) == 0, on[2]                                      # the forward bit is not set ...
    same_step(on, off)
    assert len(on[1]) == len(off[1])
    for a, b in zip(on[1], off[1]):                                     # ... and every position of every hidden state is computed
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,kw", [("roberta_one_tower_cls_ce", dict(output_hidden_states=True)), ("roberta_one_tower_vecsim_cosine", {}),
                                     ("roberta_one_tower_aux", {})], ids=["output_hidden_states", "vec_sim", "auxiliary_task"])
def test_one_tower_callers_that_read_padded_rows_stay_dense(gpu, name, kw):
    case = load_case(name)
    model = build(case, "RobertaOneTower")
    model.ensure_arena()
    assert not g(case, "attention_mask").bool().all()
    call = one_tower_call(case, **kw)
    on, off = run(model, call, True, model.roberta), run(model, call, False, model.roberta)
    dense_everywhere(on, off)
    if kw:
        assert torch.equal(on[0].hidden_states[-1], on[1][-1])


def test_one_tower_cls_head_opts_in(gpu):
    """(the counterpart: without a request for hidden states the [CLS] head of the same wrapper opts in)"""
    case = load_case("roberta_one_tower_cls_ce")
    model = build(case, "RobertaOneTower")
    model.ensure_arena()
    call = one_tower_call(case)
    on, off = run(model, call, True, model.roberta), run(model, call, False, model.roberta)
    assert on[2] == 3
    same_step(on, off)
    mask = g(case, "attention_mask").bool()
    assert on[1][-1][~mask].float().abs().max().item() == 0.0


def test_direct_roberta_model_call_stays_dense(gpu):
    import item_alignment_amd.models as M
    case = load_case("roberta_two_tower_ce")
    wrapper = build(case, "RobertaTwoTower")
    wrapper.ensure_arena()
    text = wrapper.roberta
    ids, mask, tts = g(case, "input_ids_1"), g(case, "attention_mask_1"), g(case, "token_type_ids_1")

    class Out:
        loss = None

    def call(_):
        o = Out()
        o.logits = text(ids, attention_mask=mask, token_type_ids=tts).last_hidden_state
        return o
    on, off = run(wrapper, call, True, text), run(wrapper, call, False, text)
    dense_everywhere(on, off)
    assert on[1][-1][~mask.bool()].float().abs().max().item() > 0.0


def test_cross_attn_stays_dense(gpu):
    case = load_case("coca_cross_attn")
    model, call = coca(case)
    on, off = run(model, call, True, model.coca.text_encoder), run(model, call, False, model.coca.text_encoder)
    dense_everywhere(on, off)
