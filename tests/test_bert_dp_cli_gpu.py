"""bert_pretrain.py and finetune_bert.py under the launcher (python -m torch.distributed.run --nproc-per-node 2) on loopback, on the
synthetic inputs of tests/test_bert_pretrain_cli_gpu.py and tests/test_bert_align_cli_gpu.py.  Both ranks run over gloo
(IA_DP_BACKEND), as tests/test_coca_pretrain_dp_cli_gpu.py launches its script, so a one-GPU box can hold them; on a multi-GPU node
the same path runs over RCCL with one process per GPU.  Every launch has a time limit: a rank that sat in a collective alone would
otherwise wait for the process group's."""
import csv
import json
import os
import re
import socket
import subprocess
import sys

import pytest
import torch

from test_bert_align_cli_gpu import CONFIG, VOCAB, log_text, pairs, train_args
from test_bert_pretrain_cli_gpu import ROOT, run_cli, write_inputs

pytestmark = pytest.mark.gpu
MOVED = "bert.encoder.layer.1.output.dense.weight"


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def launch(script, argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HF_HUB_OFFLINE="1", TRANSFORMERS_OFFLINE="1",
               IA_DP_BACKEND="gloo", IA_DP_TIMEOUT_MIN="3")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "IA_DP_FORCE_COLLECTIVES"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, script)] + list(argv)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    return r.returncode, r.stdout + r.stderr


def test_bert_pretrain_two_ranks_one_log_one_model_the_steps_of_one_process(gpu, tmp_path):
    """one epoch over the twelve records in global batches of four, an evaluation every fourth step; then the same in one process"""
    model_dir, data_dir = write_inputs(tmp_path)
    argv = lambda out: ["--data_dir", str(data_dir), "--model_name_or_path", str(model_dir), "--output_dir", str(out), "--max_seq_len", "30",
                        "--batch_size", "4", "--num_epochs", "1", "--warmup_steps", "2", "--log_steps", "1", "--eval_steps", "4",
                        "--learning_rate", "1e-3", "--seed", "7"]
    out = tmp_path / "out_dp"
    code, log = launch("bert_pretrain.py", argv(out))
    assert code == 0, log[-4000:]
    text = (out / "pretrain-bert.log").read_text()
    steps = [int(m.group(1).replace(",", "")) for m in re.finditer(r"Steps\s+([\d,]+), Total\s+[\d,]+, Train/Loss ([-+0-9.einfa]+)", text)]
    losses = [float(m.group(1)) for m in re.finditer(r"Train/Loss ([-+0-9.einfa]+)", text)]
    evals = [int(m.group(1).replace(",", "")) for m in re.finditer(r"Steps\s+([\d,]+), Total\s+[\d,]+, Eval/Loss [-+0-9.einfa]+", text)]
    skipped = len(re.findall(r"skipped on every rank", text))
    print("steps:", steps, "losses:", losses, "evaluated at:", evals, "skipped:", skipped)
    assert steps and steps == list(range(1, len(steps) + 1))                      # each Train/Loss line once, by rank 0 alone
    assert evals and evals == [s for s in steps if s % 4 == 0]                    # each Eval/Loss line once
    assert all(torch.isfinite(torch.tensor(losses)))
    assert sorted(os.listdir(out)) == sorted(["pretrain-bert.log", "pytorch_model.bin", "config.json", "vocab.txt"] +
                                             (["tf-logs"] if (out / "tf-logs").exists() else []))
    sd = torch.load(out / "pytorch_model.bin", map_location="cpu")
    assert torch.equal(sd["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    # one process on the same inputs: the same global batches, so the same number of optimiser steps, bar the batches two ranks skip
    r = run_cli(argv(tmp_path / "out_one"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    one = [int(m.group(1).replace(",", "")) for m in re.finditer(r"Steps\s+([\d,]+), Total\s+[\d,]+, Train/Loss", (tmp_path / "out_one" / "pretrain-bert.log").read_text())]
    print("one process steps:", one[-1])
    assert steps[-1] + skipped == one[-1] and skipped <= 1


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """the model directory and the pair files of tests/test_bert_align_cli_gpu.py"""
    root = tmp_path_factory.mktemp("bert_dp_cli")
    model_dir, data_dir = root / "model", root / "data"
    os.makedirs(model_dir)
    os.makedirs(data_dir)
    (model_dir / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf8")
    json.dump(CONFIG, open(model_dir / "config.json", "w"))
    for name, recs in (("item-align-train.json", pairs(24)), ("item-align-val.json", {"data": pairs(8, shift=3)})):
        json.dump(recs, open(data_dir / name, "w", encoding="utf8"), ensure_ascii=False)
    return root, model_dir, data_dir


@pytest.fixture(scope="module")
def first_run(gpu, dirs):
    """two ranks: six steps of 24 pairs in global batches of four (one epoch), evaluated and checkpointed at steps 3 and 6"""
    code, log = launch("finetune_bert.py", train_args(dirs, "out", 6))
    assert code == 0, log[-4000:]
    out = dirs[0] / "out"
    six = torch.load(out / "checkpoint", map_location="cpu")["model_state_dict"][MOVED].clone()      # a later test resumes into `out`
    return out, log_text(out), six


def test_finetune_bert_two_ranks_leave_one_set_of_files(first_run):
    import finetune_bert
    out, log, _ = first_run
    for d in ("F1Model", "LossModel"):
        assert sorted(os.listdir(out / d)) == ["config.json", "pytorch_model.bin", "vocab.txt"], d
    assert len([f for f in os.listdir(out / "tf-logs") if f.startswith("train-")]) == 1          # one log file
    rows = list(csv.reader(open(out / finetune_bert.CSV_FILE, newline="", encoding="utf-8")))
    assert rows[0] == finetune_bert.CSV_HEADERS and len(rows) == 3                       # one row an evaluation, not one a rank
    assert [r[-1] for r in rows[1:]] == ["3", "6"] and [r[-2] for r in rows[1:]] == ["1", "1"]
    assert all(0.0 <= float(v) <= 1.0 for r in rows[1:] for v in r[:4] + r[5:9])
    ck = torch.load(out / "checkpoint", map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "global_steps"} and ck["global_steps"] == 6
    opt = ck["optimizer_state_dict"]
    assert opt["step"] == 6 and opt["exp_avg"].abs().max() > 0 and opt["exp_avg_sq"].max() > 0
    print("log lines:", log.count("Train/Loss"), "Train/Loss,", log.count("Running Eval"), "Running Eval,", log.count("Save checkpoint"), "checkpoints")
    assert log.count("Train/Loss") == 6 and log.count("Running Eval") == 2 and log.count("Save checkpoint") == 2
    assert log.count("Data parallel: 2 ranks") == 1 and "There is no resume model path." in log


def test_finetune_bert_two_ranks_resume_on_the_same_trajectory(first_run, dirs):
    """A second two-rank invocation resumes at step 6 and takes step 7; an uninterrupted two-rank run takes seven.  Both evaluate
    and checkpoint at step 7 (a checkpoint is only written inside an evaluation), and the two checkpoints hold the same master
    weights and Adam moments, bit for bit: with two ranks the all-reduce adds two numbers, so the sum has no order."""
    out, before, six = first_run
    at_seven = ["--eval_steps", "7", "--check_steps", "7"]
    code, log = launch("finetune_bert.py", train_args(dirs, "out", 7) + at_seven)
    assert code == 0, log[-4000:]
    new = log_text(out)[len(before):]
    assert "resumed at global_steps 6" in new and new.count("Train/Loss") == 1 and new.count("Save checkpoint") == 1
    code, log = launch("finetune_bert.py", train_args(dirs, "straight", 7) + at_seven)
    assert code == 0, log[-4000:]
    straight_log = log_text(dirs[0] / "straight")
    assert "resumed" not in straight_log and straight_log.count("Train/Loss") == 7
    a = torch.load(out / "checkpoint", map_location="cpu")
    b = torch.load(dirs[0] / "straight" / "checkpoint", map_location="cpu")
    assert a["global_steps"] == b["global_steps"] == 7 and a["optimizer_state_dict"]["step"] == b["optimizer_state_dict"]["step"] == 7
    assert sorted(a["model_state_dict"]) == sorted(b["model_state_dict"])
    differ = [k for k, v in a["model_state_dict"].items() if not torch.equal(v, b["model_state_dict"][k])]
    assert not differ, differ
    assert torch.equal(a["optimizer_state_dict"]["exp_avg"], b["optimizer_state_dict"]["exp_avg"])
    assert torch.equal(a["optimizer_state_dict"]["exp_avg_sq"], b["optimizer_state_dict"]["exp_avg_sq"])
    # ... and step 7 did move the weights: against the checkpoint of step 6
    assert not torch.equal(a["model_state_dict"][MOVED], six)


def test_finetune_bert_two_ranks_skip_the_batch_that_is_shorter_than_the_world(gpu, dirs, tmp_path):
    """nine pairs in global batches of four: the third batch of an epoch holds one pair, fewer than the two ranks.  Both skip it, in
    both epochs; rank 0 logs it; the optimiser steps are the four whole batches and the run ends instead of hanging."""
    data_dir = tmp_path / "data"
    os.makedirs(data_dir)
    for name, recs in (("item-align-train.json", pairs(9)), ("item-align-val.json", pairs(4, shift=3))):
        json.dump(recs, open(data_dir / name, "w", encoding="utf8"), ensure_ascii=False)
    argv = train_args((dirs[0], dirs[1], data_dir), "short", -1) + ["--eval_steps", "4", "--check_steps", "4"]
    code, log = launch("finetune_bert.py", argv)
    assert code == 0, log[-4000:]
    text = log_text(dirs[0] / "short")
    steps = [int(m.group(1).replace(",", "")) for m in re.finditer(r"Steps\s+([\d,]+) - Total\s+[\d,]+ - Train/Loss", text)]
    print("steps:", steps, "skipped:", text.count("skipped on every rank"))
    assert steps == [1, 2, 3, 4] and text.count("a batch of 1 pairs skipped on every rank") == 2
    assert text.count("Running Eval") == 1 and "Training successfully." in text
    assert torch.load(dirs[0] / "short" / "checkpoint", map_location="cpu")["global_steps"] == 4
