"""finetune_graph.py end to end on a synthetic item / attribute-value graph: train + eval + predict, checkpoints, the P/R/F1 log
line, the prediction jsonl, and a training loss that goes down (labels are a function of shared neighbours)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cli(data_dir, out_dir, extra, env_extra):
    cmd = [sys.executable, os.path.join(ROOT, "finetune_graph.py"), "--data_dir", str(data_dir), "--output_dir", str(out_dir), "--config_file",
           "gcn.json", "--model_name", "gcn", "--data_version", "v1", "--interaction_type", "two_tower", "--classification_method", "cls",
           "--similarity_measure", "NA", "--loss_type", "ce", "--feature_dim", "64", "--hidden_size", "64", "--num_layers", "2",
           "--train_batch_size", "128", "--eval_batch_size", "256"] + extra
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_extra)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


def test_train_eval_predict(tmp_path):
    from item_alignment_amd.data.synthetic import SyntheticItemGraph
    g = SyntheticItemGraph(2000, 600, feature_dim=64)
    data_dir, out_dir = tmp_path / "data", tmp_path / "out"
    parts = g.write(str(data_dir))
    os.makedirs(out_dir)
    json.dump({"hidden_dropout_prob": 0.1, "num_labels": 2, "num_entities": g.num_nodes}, open(out_dir / "gcn.json", "w"))
    log = run_cli(data_dir, out_dir, ["--do_train", "--do_eval", "--do_pred", "--num_train_epochs", "3", "--save_epochs", "1"],
                  {"IA_GCN_PAIRWISE_LOSS": "1"})
    mdir = out_dir / "gcn-v1-two_tower-cls-NA-ce"
    assert (mdir / "hyperparamter.txt").exists()
    for e in range(3):
        assert (mdir / f"graph_epoch-{e}.bin").exists()
    assert re.search(r"\[Epoch-2\] threshold=0\.5, precision=[\d.]+, recall=[\d.]+, f1=[\d.]+", log), log[-3000:]
    rows = [json.loads(l) for l in open(mdir / "deepAI_result_threshold=0.5.jsonl")]
    test_pairs = parts["item_valid_pair.jsonl"]
    assert len(rows) == len(test_pairs)
    for r, p in zip(rows, test_pairs):
        assert list(r) == ["src_item_id", "src_item_emb", "tgt_item_id", "tgt_item_emb", "threshold"]
        assert r["src_item_id"] == p["src_item_id"] and r["tgt_item_id"] == p["tgt_item_id"] and r["threshold"] == 0.5
        assert re.fullmatch(r"\[[-+0-9.e]+\]", r["src_item_emb"])
    losses = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"\[Epoch-(\d+)\] mean training loss: ([-+0-9.einfa]+)", log)}
    print("mean training loss per epoch:", losses)
    assert losses[2] < losses[0], losses


def test_literal_loss_form_runs_one_step(tmp_path):
    from item_alignment_amd.data.synthetic import SyntheticItemGraph
    g = SyntheticItemGraph(2000, 600, feature_dim=64, n_pairs=300)
    data_dir, out_dir = tmp_path / "data", tmp_path / "out"
    g.write(str(data_dir))
    os.makedirs(out_dir)
    json.dump({"hidden_dropout_prob": 0.1, "num_labels": 2}, open(out_dir / "gcn.json", "w"))
    log = run_cli(data_dir, out_dir, ["--do_train", "--num_train_epochs", "1", "--save_epochs", "1", "--log_steps", "1"], {"IA_GCN_PAIRWISE_LOSS": "0"})
    assert re.search(r"\[Epoch-0 Step-0\] loss: ", log)
    assert (out_dir / "gcn-v1-two_tower-cls-NA-ce" / "graph_epoch-0.bin").exists()
