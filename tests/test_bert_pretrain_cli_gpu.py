"""bert_pretrain.py end to end as a fresh child process: a temporary model directory (vocab.txt + a tiny config.json, no weights), a
dozen synthetic records, a few optimiser steps with an evaluation every second one."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARS = list("手机红色蓝大小号棉电池型品牌华为苹果颜尺码材质新款男女")
VOCAB = ["[PAD]"] + [f"[unused{i}]" for i in range(1, 8)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]", ":", ";", "a1", "b2", "x", "y"] + CHARS
CONFIG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=64, max_position_embeddings=64,
              type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12,
              hidden_act="gelu", initializer_range=0.02)


def records(n):
    colours, sizes, brands = ["红色", "蓝色"], ["大号", "小号"], ["华为", "苹果"]
    out = []
    for i in range(n):
        c, s, b = colours[i % 2], sizes[(i // 2) % 2], brands[(i // 4) % 2]
        rec = {"industry_name": "手机", "cate_name": "电池" if i % 3 else "手机", "cate_name_path": "手机 电池", "title": f"{b} 新款 {c} a1 x",
               "item_pvs": f"颜色:{c};#尺码:{s};品牌:{b}"}
        if i % 5 == 4:
            del rec["industry_name"]                 # a missing field reads as the placeholder text
        out.append(rec)
    return out


def write_inputs(tmp_path):
    assert len(VOCAB) <= CONFIG["vocab_size"]
    model_dir, data_dir = tmp_path / "model", tmp_path / "data"
    os.makedirs(model_dir)
    os.makedirs(data_dir)
    (model_dir / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf8")
    json.dump(CONFIG, open(model_dir / "config.json", "w"))
    for name, recs in (("pretrain_train.jsonl", records(12)), ("pretrain_valid.jsonl", records(3))):
        (data_dir / name).write_text("\n".join(json.dumps(r, ensure_ascii=False) for r in recs) + "\n", encoding="utf8")
    return model_dir, data_dir


def run_cli(argv, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bert_pretrain.py")] + argv, capture_output=True, text=True, env=env, timeout=timeout,
                          cwd=ROOT)


def train(model_dir, data_dir, out_dir, seed):
    r = run_cli(["--data_dir", str(data_dir), "--model_name_or_path", str(model_dir), "--output_dir", str(out_dir), "--max_seq_len", "30",
                 "--batch_size", "4", "--num_epochs", "1", "--warmup_steps", "2", "--log_steps", "1", "--eval_steps", "2", "--max_steps", "4",
                 "--learning_rate", "1e-3", "--seed", str(seed)])
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


@pytest.mark.gpu
def test_a_few_steps_log_a_finite_loss_and_write_the_checkpoint(gpu, tmp_path):
    import torch
    model_dir, data_dir = write_inputs(tmp_path)
    out = tmp_path / "out"
    log = train(model_dir, data_dir, out, seed=7)
    losses = [float(m.group(1)) for m in re.finditer(r"Train/Loss ([-+0-9.einfa]+)", log)]
    evals = [float(m.group(1)) for m in re.finditer(r"Eval/Loss ([-+0-9.einfa]+)", log)]
    print("train losses:", losses, "eval losses:", evals)
    assert len(losses) == 4 and len(evals) == 2
    assert all(torch.isfinite(torch.tensor(losses + evals)))
    for name in ("pytorch_model.bin", "config.json", "vocab.txt", "pretrain-bert.log"):
        assert (out / name).exists(), name
    assert "Train/Loss" in (out / "pretrain-bert.log").read_text()
    assert (out / "vocab.txt").read_text(encoding="utf8") == (model_dir / "vocab.txt").read_text(encoding="utf8")
    sd = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert sd["cls.predictions.decoder.weight"].shape == (64, 128) and "bert.encoder.layer.1.output.dense.weight" in sd
    assert torch.equal(sd["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
    assert json.load(open(out / "config.json"))["hidden_size"] == 128
    # the same seed: the same examples, initialisation and dropout, and deterministic kernels -- the same first-step loss, to the digit
    again = train(model_dir, data_dir, tmp_path / "out2", seed=7)
    first = re.search(r"Steps\s+1, .*Train/Loss ([-+0-9.einfa]+)", log).group(1)
    assert re.search(r"Steps\s+1, .*Train/Loss ([-+0-9.einfa]+)", again).group(1) == first


def test_a_hub_style_model_name_is_refused_before_anything_that_could_download(tmp_path):
    """no GPU needed: the check comes first.  The child reports which modules it had loaded when it gave up -- neither transformers nor
    huggingface_hub, so nothing that could open a connection ever ran."""
    r = run_cli(["--data_dir", str(tmp_path), "--model_name_or_path", "bert-base-chinese"], timeout=120)
    assert r.returncode != 0
    assert "is not a local directory" in r.stderr and "never downloads" in r.stderr
    probe = ("import runpy, sys\n"
             "sys.argv = ['bert_pretrain.py', '--data_dir', '.', '--model_name_or_path', 'bert-base-chinese']\n"
             "try:\n    runpy.run_path(sys.argv[0], run_name='__main__')\n"
             "except SystemExit:\n    print('LOADED', sorted(m for m in ('transformers', 'huggingface_hub', 'requests', 'httpx') if m in sys.modules))\n")
    p = subprocess.run([sys.executable, "-c", probe], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert "LOADED []" in p.stdout, p.stdout + p.stderr
