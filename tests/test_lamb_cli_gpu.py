"""`--optimizer lamb` through the scripts: finetune_text.py trains, names the optimiser in hyperparamter.txt and ends elsewhere than the
adamw run of the same seed; bert_pretrain.py runs with its clipping on the device; what is refused -- an unknown optimiser, lamb for a
model without a parameter arena, a finetune_bert.py checkpoint resumed with the other optimiser."""
import json
import os
import re
import subprocess
import sys

import pytest

from test_cli_textcnn import ROOT, make_data


def run_text(root, out, extra, env=None, model=("roberta_tiny.json", "roberta_tiny")):
    cmd = [sys.executable, os.path.join(ROOT, "finetune_text.py"), "--data_dir", root, "--output_dir", out, "--config_file",
           os.path.join(root, model[0]), "--model_name", model[1], "--data_version", "v1", "--interaction_type", "two_tower",
           "--classification_method", "cls", "--similarity_measure", "NA", "--loss_type", "ce", "--do_train",
           "--train_batch_size", "8", "--num_train_epochs", "1", "--learning_rate", "1e-3", "--log_steps", "1", "--seed", "11",
           "--pretrained_model_path", os.path.join(root, "pretrained"), "--max_seq_len", "8", "--max_seq_len_pv", "12",
           "--max_position_embeddings", "64"] + extra
    return subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})), timeout=600)


def text_inputs(root):
    pre = make_data(root, n_train=16, n_test=8)
    assert os.path.normpath(pre) == os.path.join(root, "pretrained"), pre
    vocab_size = len(open(os.path.join(pre, "vocab.txt"), encoding="utf-8").read().split("\n")) - 1
    cfg = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=vocab_size,
               max_position_embeddings=64, type_vocab_size=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    json.dump(cfg, open(os.path.join(root, "roberta_tiny.json"), "w"))


@pytest.mark.gpu
def test_finetune_text_trains_with_lamb_and_ends_elsewhere_than_adamw(gpu, tmp_path):
    import torch
    root = str(tmp_path)
    text_inputs(root)
    weights = {}
    for name in ("lamb", "adamw"):
        out = os.path.join(root, "out_" + name)
        os.makedirs(out)
        r = run_text(root, out, ["--optimizer", name] if name == "lamb" else [])           # adamw is the default
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "loss:" in r.stderr
        d = os.path.join(out, os.listdir(out)[0])
        assert f"optimizer='{name}'" in open(os.path.join(d, "hyperparamter.txt")).read()
        ck = [f for f in os.listdir(d) if f.endswith("epoch-0.bin")]
        assert len(ck) == 1, os.listdir(d)
        weights[name] = torch.load(os.path.join(d, ck[0]), map_location="cpu")
    key = next(k for k in weights["lamb"] if k.endswith("encoder.layer.1.output.dense.weight"))
    assert torch.isfinite(weights["lamb"][key]).all()
    assert not torch.equal(weights["lamb"][key], weights["adamw"][key])


@pytest.mark.gpu
def test_bert_pretrain_runs_with_lamb_and_its_clipping(gpu, tmp_path):
    import torch
    from test_bert_pretrain_cli_gpu import run_cli, write_inputs
    model_dir, data_dir = write_inputs(tmp_path)
    out = tmp_path / "out"
    r = run_cli(["--data_dir", str(data_dir), "--model_name_or_path", str(model_dir), "--output_dir", str(out), "--max_seq_len", "30",
                 "--batch_size", "4", "--num_epochs", "1", "--warmup_steps", "1", "--log_steps", "1", "--eval_steps", "3",
                 "--learning_rate", "1e-3", "--seed", "7", "--optimizer", "lamb", "--max_grad_norm", "1.0"])
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    losses = [float(m.group(1)) for m in re.finditer(r"Train/Loss ([-+0-9.einfa]+)", log)]
    assert len(losses) >= 3 and all(torch.isfinite(torch.tensor(losses)))                 # one epoch over the examples of 12 records
    sd = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())


def test_an_unknown_optimizer_is_a_usage_error(tmp_path):
    import bert_pretrain
    import finetune_bert
    for parser in (bert_pretrain.get_parser(), finetune_bert.get_parser()):
        assert parser.get_default("optimizer") == "adamw"
        for action in parser._actions:
            if action.dest == "optimizer":
                assert list(action.choices) == ["adamw", "lamb"]
    r = run_text(str(tmp_path), str(tmp_path), ["--optimizer", "sgd"])
    assert r.returncode == 2 and "invalid choice: 'sgd'" in r.stderr


def test_lamb_is_refused_for_the_textcnn_on_the_cpu(tmp_path):
    root = str(tmp_path)
    make_data(root)
    out = os.path.join(root, "out")
    os.makedirs(out)
    r = run_text(root, out, ["--optimizer", "lamb", "--filter_sizes", "1,2,3,5", "--num_filters", "4"],
                 env=dict(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""), model=("textcnn.json", "textcnn"))
    assert r.returncode != 0
    assert "--optimizer lamb" in r.stderr and "parameter arena" in r.stderr and "Traceback" not in r.stderr
    assert not any(f.endswith(".bin") for _, _, files in os.walk(out) for f in files)


@pytest.mark.gpu
def test_finetune_bert_refuses_to_resume_with_the_other_optimizer(gpu, tmp_path):
    import torch
    import finetune_bert
    from test_bert_align_cli_gpu import CONFIG, VOCAB, pairs, train_args
    model_dir, data_dir = tmp_path / "model", tmp_path / "data"
    os.makedirs(model_dir)
    os.makedirs(data_dir)
    (model_dir / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf8")
    json.dump(CONFIG, open(model_dir / "config.json", "w"))
    json.dump(pairs(24), open(data_dir / "item-align-train.json", "w", encoding="utf8"), ensure_ascii=False)
    json.dump({"data": pairs(8, shift=3)}, open(data_dir / "item-align-val.json", "w", encoding="utf8"), ensure_ascii=False)
    d = (tmp_path, model_dir, data_dir)
    parser = finetune_bert.get_parser()
    done = finetune_bert.run(parser.parse_args(train_args(d, "lamb", 3) + ["--optimizer", "lamb"]))
    assert done.global_steps == 3
    path = d[0] / "lamb" / "checkpoint"
    ck = torch.load(path, map_location="cpu")
    assert ck["optimizer_state_dict"]["optimizer"] == "lamb" and ck["optimizer_state_dict"]["step"] == 3
    with pytest.raises(SystemExit, match="written with --optimizer lamb"):
        finetune_bert.run(parser.parse_args(train_args(d, "lamb", 4)))
    # the same optimiser resumes ...
    more = finetune_bert.run(parser.parse_args(train_args(d, "lamb", 4) + ["--optimizer", "lamb"]))
    assert more.global_steps == 4 and more.model.param_arena.step_count == 4
    # ... and a checkpoint from before the flag existed is adamw's
    ck = torch.load(path, map_location="cpu")
    del ck["optimizer_state_dict"]["optimizer"]
    torch.save(ck, path)
    with pytest.raises(SystemExit, match="written with --optimizer adamw"):
        finetune_bert.run(parser.parse_args(train_args(d, "lamb", 5) + ["--optimizer", "lamb"]))
