"""coca_pretrain.py end to end as a fresh child process: a temporary data directory (item_info.jsonl with six items, PIL-made PNGs with
one image missing), a vocabulary, a tiny config with dropout 0 and tiny text / ViT checkpoints written here; two epochs."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CHARS = list("手机红色蓝大小号棉电池型品牌华为苹果颜尺码材质新款男女")
VOCAB = ["[PAD]"] + [f"[unused{i}]" for i in range(1, 8)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]", ":", ";", "a1", "b2", "x", "y", "<S>"] + CHARS
CONFIG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, vocab_size=64, max_position_embeddings=64,
              type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12,
              hidden_act="gelu", initializer_range=0.02, patch_size=16, num_hidden_layers_multimodal=1, num_attention_heads_multimodal=2,
              feedforward_multiplication_multimodal=2)
IMAGE = 64
LOSS = re.compile(r"\[Epoch-(\d+) Step-(\d+)\] loss: ([-+0-9.einfa]+)")


def write_inputs(tmp_path):
    import torch
    from PIL import Image

    import item_alignment_amd.models as M
    from item_alignment_amd.cli_common import load_config
    assert len(VOCAB) <= CONFIG["vocab_size"]
    data, text, image, out = (tmp_path / n for n in ("data", "text", "image", "out"))
    for d in (data / "item_images", text, image, out):
        os.makedirs(d)
    colours, sizes, brands = ["红色", "蓝色"], ["大号", "小号"], ["华为", "苹果"]
    with open(data / "item_info.jsonl", "w", encoding="utf8") as w:
        for i in range(6):
            c, s, b = colours[i % 2], sizes[(i // 2) % 2], brands[(i // 4) % 2]
            w.write(json.dumps({"item_id": f"i{i}", "title": f"{b} 新款 {c} a1 x", "item_pvs": f"颜色:{c};#尺码:{s}", "sku_pvs": f"品牌:{b}",
                                "item_image_name": f"{i}.png"}, ensure_ascii=False) + "\n")
            if i != 4:                         # item 4's image is missing: the collate drops it
                Image.new("RGB", (40, 36), (40 * i, 255 - 40 * i, 90 if i % 2 else 200)).save(data / "item_images" / f"{i}.png")
    (text / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf8")
    json.dump(CONFIG, open(out / "config.json", "w"))
    json.dump(CONFIG, open(text / "config.json", "w"))
    torch.manual_seed(3)
    cfg = load_config(str(out / "config.json"))
    torch.save(M.RobertaModel(cfg).state_dict(), text / "pytorch_model.bin")
    torch.save(M.VisionTransformer(img_size=IMAGE, patch_size=16, embed_dim=128, depth=2, num_heads=2).state_dict(), image / "image_encoder.bin")
    return data, text, image, out


def run_cli(paths, name, *more):
    data, text, image, out = paths
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HF_HUB_OFFLINE="1", TRANSFORMERS_OFFLINE="1")
    env.pop("WORLD_SIZE", None)
    argv = ["--data_dir", str(data), "--output_dir", str(out), "--model_name", name, "--config_file", "config.json",
            "--pretrained_text_model_path", str(text), "--pretrained_image_model_path", str(image), "--image_size", str(IMAGE),
            "--max_seq_len", "10", "--max_seq_len_pv", "14", "--train_batch_size", "2", "--num_train_epochs", "2", "--log_steps", "1",
            "--learning_rate", "2e-4", "--warmup_proportion", "0.0", "--seed", "5", "--fp16"] + list(more)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "coca_pretrain.py")] + argv, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log, [(int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in LOSS.finditer(log)]


@pytest.fixture(scope="module")
def first_run(gpu, tmp_path_factory):
    paths = write_inputs(tmp_path_factory.mktemp("coca_pretrain"))
    log, losses = run_cli(paths, "coca_tiny")
    return paths, log, losses


def test_two_epochs_write_the_checkpoints_and_the_loss_falls(first_run):
    import math

    import torch

    import item_alignment_amd.models as M
    from item_alignment_amd.cli_common import load_config
    paths, log, losses = first_run
    out = paths[3] / "coca_tiny"
    print("losses:", losses)
    assert [e for e, _, _ in losses] == [0, 0, 0, 1, 1, 1] and [s for _, s, _ in losses] == [0, 1, 2, 0, 1, 2]      # six items, three batches of two
    assert all(math.isfinite(v) for _, _, v in losses)
    assert losses[-1][2] < losses[0][2]
    assert "6 optimiser steps" in log
    for name in ("coca_pretrain_epoch-0.bin", "coca_pretrain_epoch-1.bin", "hyperparamter.txt"):
        assert (out / name).exists(), name
    assert "caption_loss_weight" in (out / "hyperparamter.txt").read_text()
    cfg = load_config(str(paths[3] / "config.json"), caption_loss_weight=1.0, contrastive_loss_weight=1.0)
    vit = M.VisionTransformer(img_size=IMAGE, patch_size=16, embed_dim=128, depth=2, num_heads=2)
    want = M.CoCaForPretraining(cfg, image_encoder=vit, text_encoder=M.RobertaModel(cfg)).state_dict()
    for e in (0, 1):
        sd = torch.load(out / f"coca_pretrain_epoch-{e}.bin", map_location="cpu")
        assert sorted(sd) == sorted(want)
        assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())
        assert torch.equal(sd["to_logits.1.weight"], sd["coca.text_encoder.embeddings.word_embeddings.weight"])
        assert all(tuple(sd[k].shape) == tuple(want[k].shape) for k in want)
    assert not torch.equal(sd["temperature"], torch.ones(1))


def test_resuming_from_the_first_epoch_s_file_starts_from_its_loss(first_run):
    """--start_epoch 1 with epoch 0's weights: the shuffle and the augmentation of an epoch depend on (seed, epoch) alone and there is no
    dropout, so the first step sees the batch and the weights the first run's epoch 1 started with -- the same loss, up to the six
    printed decimals."""
    paths, _, losses = first_run
    state = paths[3] / "coca_tiny" / "coca_pretrain_epoch-0.bin"
    _, resumed = run_cli(paths, "coca_resumed", "--file_state_dict", str(state), "--start_epoch", "1")
    want = [v for e, s, v in losses if (e, s) == (1, 0)][0]
    print("resumed:", resumed[0], "first run's epoch 1:", want, "first run's start:", losses[0][2])
    assert resumed[0][:2] == (1, 0) and len(resumed) == 3
    assert abs(resumed[0][2] - want) <= 2e-6 * max(1.0, abs(want))
    assert (paths[3] / "coca_resumed" / "coca_pretrain_epoch-1.bin").exists()


def test_gradient_accumulation_halves_the_optimiser_steps(first_run):
    """three micro-batches an epoch: one optimiser step every second one (the odd one out is dropped at the epoch's end, as in
    item_alignment_amd/train.py), against three without accumulation"""
    paths, first_log, _ = first_run
    log, losses = run_cli(paths, "coca_accumulated", "--gradient_accumulation_steps", "2")
    steps = [int(m.group(1)) for m in re.finditer(r"saving model \((\d+) optimiser steps so far\)", log)]
    plain = [int(m.group(1)) for m in re.finditer(r"saving model \((\d+) optimiser steps so far\)", first_log)]
    assert plain == [3, 6] and steps == [3 // 2, 2 * (3 // 2)]
    assert len(losses) == 6                      # every micro-batch is still run and logged
    assert "Num steps = 2" in log and "Num steps = 6" in first_log
