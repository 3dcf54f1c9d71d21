"""BASELINE.json configs[0] through finetune_text.py with the GPU visible: the command line of tests/test_cli_textcnn.py as a fresh
child process, the same files and log lines, and the log line that says the model went to the GPU."""
import json
import os
import subprocess
import sys

import pytest

from test_cli_textcnn import ROOT, make_data

pytestmark = pytest.mark.gpu


def test_finetune_text_textcnn_gpu(gpu, tmp_path):
    root = str(tmp_path)
    pre = make_data(root)
    out = os.path.join(root, "out")
    os.makedirs(out)
    cmd = [sys.executable, os.path.join(ROOT, "finetune_text.py"), "--data_dir", root, "--output_dir", out, "--config_file",
           os.path.join(root, "textcnn.json"), "--model_name", "textcnn", "--data_version", "v1", "--interaction_type", "two_tower",
           "--classification_method", "cls", "--similarity_measure", "NA", "--loss_type", "ce", "--do_train", "--do_eval", "--do_pred",
           "--train_batch_size", "16", "--eval_batch_size", "8", "--num_train_epochs", "2", "--learning_rate", "1e-3", "--log_steps", "1",
           "--pretrained_model_path", pre, "--max_seq_len", "8", "--max_seq_len_pv", "12", "--max_position_embeddings", "64",
           "--filter_sizes", "1,2,3,5", "--num_filters", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("CUDA_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = os.path.join(out, "textcnn-v1-two_tower-cls-NA-ce")
    assert os.path.exists(os.path.join(d, "text_finetune_epoch-1.bin"))
    assert os.path.exists(os.path.join(d, "hyperparamter.txt"))
    w = json.load(open(os.path.join(d, "weights.json")))
    assert len(w["w"]) == 2 and len(w["w"][0]) == 2 * 4 * 4
    lines = [json.loads(l) for l in open(os.path.join(d, "deepAI_result_threshold=0.5.jsonl"))]
    assert len(lines) == 16 and set(lines[0]) == {"src_item_id", "src_item_emb", "tgt_item_id", "tgt_item_emb", "threshold"}
    assert "threshold=0.1" in r.stderr and "f1=" in r.stderr and "[Epoch-1 Step-0] loss:" in r.stderr
    assert "device: cuda:0 (TextCNNTwoTower)" in r.stderr
