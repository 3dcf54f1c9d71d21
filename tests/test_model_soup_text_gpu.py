"""model_soup_text.py on the GPU: two tiny finetune_text.py epochs, the uniform soup over both, and the soup of one epoch alone, which
must predict what that epoch's checkpoint predicts."""
import json
import os
import subprocess
import sys

import pytest
import torch

from test_cli_textcnn import ROOT, make_data

pytestmark = pytest.mark.gpu

MODEL_DIR = "roberta_tiny-v1-one_tower-cls-NA-ce"


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r


@pytest.fixture(scope="module")
def trained(gpu, tmp_path_factory):
    """two epochs of a 2-layer one-tower model: (data dir, model dir, the flags both scripts share)"""
    root = str(tmp_path_factory.mktemp("soup"))
    pre = make_data(root, n_train=16, n_test=8)
    vocab_size = len(open(os.path.join(pre, "vocab.txt"), encoding="utf-8").read().split("\n")) - 1
    cfg = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=vocab_size,
               max_position_embeddings=64, type_vocab_size=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    json.dump(cfg, open(os.path.join(root, "roberta_tiny.json"), "w"))
    out = os.path.join(root, "out")
    os.makedirs(out)
    shared = ["--data_dir", root, "--output_dir", out, "--config_file", os.path.join(root, "roberta_tiny.json"), "--model_name", "roberta_tiny",
              "--data_version", "v1", "--interaction_type", "one_tower", "--classification_method", "cls", "--similarity_measure", "NA",
              "--loss_type", "ce", "--eval_batch_size", "4", "--pretrained_model_path", pre, "--max_seq_len", "8", "--max_seq_len_pv", "12",
              "--max_position_embeddings", "64", "--threshold", "0.5"]
    _run([sys.executable, os.path.join(ROOT, "finetune_text.py")] + shared + ["--do_train", "--train_batch_size", "8", "--num_train_epochs", "2",
                                                                              "--learning_rate", "1e-3", "--log_steps", "1"])
    d = os.path.join(out, MODEL_DIR)
    assert os.path.exists(os.path.join(d, "text_finetune_epoch-0.bin")) and os.path.exists(os.path.join(d, "text_finetune_epoch-1.bin"))
    return root, d, shared


def _soup(trained, soups, extra=()):
    root, d, shared = trained
    return _run([sys.executable, os.path.join(ROOT, "model_soup_text.py")] + shared +
                ["--file_state_dict", os.path.join(d, "text_finetune_epoch-{}.bin"), "--soups", soups, "--do_pred", *extra])


def _pairs(root):
    return [(r[1], r[4]) for r in (l.rstrip("\n").split("\t") for l in open(os.path.join(root, "processed", "v1", "finetune_test.tsv"), encoding="utf-8"))]


def test_soup_of_two_epochs(trained):
    root, d, _ = trained
    r = _soup(trained, "0,1", ["--do_eval"])
    a, b = (torch.load(os.path.join(d, f"text_finetune_epoch-{e}.bin"), map_location="cpu") for e in (0, 1))
    soup = torch.load(os.path.join(d, "pkgm_finetune-uniform_soup-epoch-0,1.bin"), map_location="cpu")
    assert list(soup) == list(a)
    from item_alignment_amd.cli_common import load_config
    from src.models import RobertaOneTower
    cfg = load_config(os.path.join(root, "roberta_tiny.json"), interaction_type="one_tower", classification_method="cls", loss_type="ce",
                      max_seq_len=8, max_seq_len_pv=12)
    params = set(dict(RobertaOneTower(cfg).named_parameters()))
    assert params and any(not torch.equal(a[k], b[k]) for k in params)                    # the two epochs differ
    for k in soup:
        want = (a[k] + b[k]) / 2 if k in params else b[k]
        assert torch.equal(soup[k], want), k
    rows = [json.loads(l) for l in open(os.path.join(d, "deepAI_result_uniform_soup_threshold=0.5.jsonl"))]
    assert [(x["src_item_id"], x["tgt_item_id"]) for x in rows] == _pairs(root) and len(rows) == 8
    assert all(list(x) == ["src_item_id", "src_item_emb", "tgt_item_id", "tgt_item_emb", "threshold"] and x["threshold"] == 0.5 for x in rows)
    assert "[Eval] threshold=0.5" in r.stderr and "f1=" in r.stderr                      # --do_eval ran on the soup


def test_soup_of_one_epoch_predicts_what_its_checkpoint_predicts(trained):
    """forward-only, the same shapes, and a forward path without float atomics: byte for byte"""
    root, d, shared = trained
    _soup(trained, "1")
    ck = os.path.join(d, "text_finetune_epoch-1.bin")
    assert all(torch.equal(v, torch.load(ck, map_location="cpu")[k])
               for k, v in torch.load(os.path.join(d, "pkgm_finetune-uniform_soup-epoch-1.bin"), map_location="cpu").items())
    _run([sys.executable, os.path.join(ROOT, "finetune_text.py")] + shared + ["--do_pred", "--file_state_dict", ck])
    got = open(os.path.join(d, "deepAI_result_uniform_soup_threshold=0.5.jsonl"), "rb").read()
    want = open(os.path.join(d, "deepAI_result_threshold=0.5.jsonl"), "rb").read()
    assert len(want.splitlines()) == 8
    assert got == want
