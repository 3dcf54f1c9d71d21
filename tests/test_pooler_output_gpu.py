"""RobertaModel.forward(..., return_pooler_output=True) against the reference's RobertaModel in fp32 (tests/golden/pred_text/pooler.npz,
tools/gen_golden_pred_text.py): 2 layers, H = 128, 13 sequences padded to 24 with valid lengths 2 .. 24.  The weights in the file are
exact in bf16, so what differs between the two sides is the arithmetic alone; the bar is the project's forward bar:
max |got - want| / max |want| <= 5e-2.  Measured on an MI355X: 1.15e-2 for pooler_output and 1.29e-2 for the [CLS] row, the same in
all three modes."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pred_text", "pooler.npz")
BAR = 5e-2
# the three ways the tower runs: every row computed; what pred_text.py asks for; the valid tokens only (IA_UNPAD=1)
MODES = {"padded": {}, "cls_only": dict(padded_rows_unread=True, cls_only_read=True), "unpad": {}}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    sd = {k[2:]: torch.from_numpy(z[k].view(np.int16)).view(torch.bfloat16).float() for k in z.files if k.startswith("w_")}
    t = lambda k: torch.from_numpy(z[k])
    return dict(config=meta["config"], sd=sd, ids=t("input_ids"), mask=t("attention_mask"), tts=t("token_type_ids"),
                pooler=t("pooler_output"), cls=t("cls_hidden"))


def build(golden, add_pooling_layer=True, trainable_pooler=False):
    from item_alignment_amd.cli_common import load_config
    from item_alignment_amd.models.text import RobertaModel
    model = RobertaModel(load_config(None, **golden["config"]), add_pooling_layer=add_pooling_layer)
    own = model.state_dict()
    sd = {k: v for k, v in golden["sd"].items() if k in own}
    assert len(sd) == len(golden["sd"]) - (0 if add_pooling_layer else 2)
    model.load_state_dict(sd, strict=False)
    assert not [k for k, v in own.items() if v.is_floating_point() and k not in sd]
    if trainable_pooler:
        for p in model.pooler.parameters():
            p.requires_grad = True
    return model.cuda().eval()


@pytest.fixture(scope="module")
def model(gpu, golden):
    return build(golden)


def run(model, golden, mode, ids=None, **kw):
    from item_alignment_amd.models import text as T
    ids = golden["ids"] if ids is None else ids
    was, T.UNPAD = T.UNPAD, mode == "unpad"
    try:
        with torch.no_grad():
            return model(ids.cuda(), attention_mask=golden["mask"].cuda(), token_type_ids=golden["tts"].cuda(), **MODES[mode], **kw)
    finally:
        T.UNPAD = was


def rel(got, want):
    return float((got.double().cpu() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize("mode", list(MODES))
def test_pooler_output_and_cls_row_match_the_reference(model, golden, mode):
    out = run(model, golden, mode, return_pooler_output=True)
    pooled, cls = out.pooler_output, out.last_hidden_state[:, 0]
    assert pooled.dtype == torch.float32 and tuple(pooled.shape) == tuple(golden["pooler"].shape) == (13, 128)
    e_pool, e_cls = rel(pooled, golden["pooler"]), rel(cls.float(), golden["cls"])
    print(f"{mode}: pooler_output {e_pool:.3e}, [CLS] hidden row {e_cls:.3e} (bar {BAR:g})")
    assert torch.isfinite(pooled).all()
    assert e_pool <= BAR and e_cls <= BAR


@pytest.mark.parametrize("mode", list(MODES))
def test_padded_positions_do_not_reach_the_pooler(model, golden, mode):
    g = torch.Generator().manual_seed(11)
    junk = torch.randint(1, golden["config"]["vocab_size"], golden["ids"].shape, generator=g)
    ids = torch.where(golden["mask"] != 0, golden["ids"], junk)
    assert not torch.equal(ids, golden["ids"])
    a = run(model, golden, mode, return_pooler_output=True)
    b = run(model, golden, mode, ids=ids, return_pooler_output=True)
    assert torch.equal(a.pooler_output, b.pooler_output)
    assert torch.equal(a.last_hidden_state[:, 0], b.last_hidden_state[:, 0])


@pytest.mark.parametrize("mode", list(MODES))
def test_the_keyword_is_opt_in(model, golden, mode):
    with_it = run(model, golden, mode, return_pooler_output=True)
    without = run(model, golden, mode)
    assert torch.equal(with_it.last_hidden_state, without.last_hidden_state)
    assert "pooler_output" in with_it and "pooler_output" not in without and list(without) == ["last_hidden_state", "hidden_states"]
    with pytest.raises(AttributeError, match="return_pooler_output"):
        without.pooler_output
    assert not hasattr(without, "pooler_output")


def test_no_pooling_layer_raises(gpu, golden):
    bare = build(golden, add_pooling_layer=False)
    assert bare.pooler is None
    with pytest.raises(ValueError, match="add_pooling_layer"):
        run(bare, golden, "padded", return_pooler_output=True)
    assert run(bare, golden, "padded").last_hidden_state.shape == (13, 24, 128)


def test_a_trainable_pooler_takes_its_gradient(gpu, golden):
    from item_alignment_amd.models import functional as Fn
    m = build(golden, trainable_pooler=True)
    m.train()
    Fn.set_step_seed(5)
    out = m(golden["ids"].cuda(), attention_mask=golden["mask"].cuda(), token_type_ids=golden["tts"].cuda(), return_pooler_output=True)
    assert out.pooler_output.requires_grad and out.pooler_output.grad_fn is not None
    m.param_arena.zero_grad()
    out.pooler_output.sum().backward()
    torch.cuda.synchronize()
    for p in (m.pooler.dense.weight, m.pooler.dense.bias):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    # ... and passes it on through the [CLS] gather into the tower
    w = m.encoder.layer[-1].output.dense.weight
    assert torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0
