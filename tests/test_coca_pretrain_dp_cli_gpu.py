"""coca_pretrain.py under the launcher (python -m torch.distributed.run --nproc-per-node 2), on the tiny inputs of
tests/test_coca_pretrain_cli_gpu.py: six items, one of them without its image.  One GPU here, so both ranks share it over gloo
(IA_DP_BACKEND); on a multi-GPU node the same path runs over RCCL with one process per GPU.  Every child gets a timeout: a rank that
sat in a collective alone would otherwise wait for the process group's."""
import os
import re
import subprocess
import sys

import pytest

from test_coca_pretrain_cli_gpu import IMAGE, LOSS, ROOT, write_inputs

pytestmark = pytest.mark.gpu


def launch(paths, name, port, *more, batch=2):
    data, text, image, out = paths
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HF_HUB_OFFLINE="1", TRANSFORMERS_OFFLINE="1",
               IA_DP_BACKEND="gloo", IA_DP_TIMEOUT_MIN="3")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "IA_DP_FORCE_COLLECTIVES"):
        env.pop(k, None)
    argv = ["--data_dir", str(data), "--output_dir", str(out), "--model_name", name, "--config_file", "config.json",
            "--pretrained_text_model_path", str(text), "--pretrained_image_model_path", str(image), "--image_size", str(IMAGE),
            "--max_seq_len", "10", "--max_seq_len_pv", "14", "--train_batch_size", str(batch), "--num_train_epochs", "2", "--log_steps", "1",
            "--learning_rate", "2e-4", "--warmup_proportion", "0.0", "--seed", "5", "--fp16"] + list(more)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "coca_pretrain.py")] + argv
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    return r.returncode, r.stdout + r.stderr


@pytest.fixture(scope="module")
def paths(gpu, tmp_path_factory):
    return write_inputs(tmp_path_factory.mktemp("coca_pretrain_dp"))


def test_two_ranks_write_one_set_of_files_and_skip_the_short_micro_batch_together(paths):
    """Two epochs of three micro-batches, one item a rank.  Item 4 has no image: in each epoch the micro-batch in which a rank is dealt
    it leaves that rank without an item, and both ranks skip it (the run ends instead of hanging); the other two are optimiser steps."""
    import math

    import torch

    import item_alignment_amd.models as M
    from item_alignment_amd.cli_common import load_config
    code, log = launch(paths, "coca_dp", 29741)
    assert code == 0, log[-4000:]
    losses = [(int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in LOSS.finditer(log)]
    skipped = re.findall(r"\[Epoch-(\d+) Step-(\d+)\] skipped on every rank", log)
    print("losses:", losses, "skipped:", skipped)
    assert [e for e, _ in skipped] == ["0", "1"]                                   # once an epoch, logged by rank 0 alone
    assert [e for e, _, _ in losses] == [0, 0, 1, 1] and all(math.isfinite(v) for _, _, v in losses)      # one line a step, not one a rank
    assert {(int(e), int(s)) for e, s in skipped}.isdisjoint({(e, s) for e, s, _ in losses})
    assert len(re.findall(r"saving model \((\d+) optimiser steps so far\)", log)) == 2 and "(4 optimiser steps so far)" in log
    out = paths[3] / "coca_dp"
    assert sorted(os.listdir(out)) == ["coca_pretrain_epoch-0.bin", "coca_pretrain_epoch-1.bin", "hyperparamter.txt"]
    cfg = load_config(str(paths[3] / "config.json"), caption_loss_weight=1.0, contrastive_loss_weight=1.0)
    vit = M.VisionTransformer(img_size=IMAGE, patch_size=16, embed_dim=128, depth=2, num_heads=2)
    want = M.CoCaForPretraining(cfg, image_encoder=vit, text_encoder=M.RobertaModel(cfg)).state_dict()
    for e in (0, 1):
        sd = torch.load(out / f"coca_pretrain_epoch-{e}.bin", map_location="cpu")
        assert sorted(sd) == sorted(want)
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
        assert torch.equal(sd["to_logits.1.weight"], sd["coca.text_encoder.embeddings.word_embeddings.weight"])
    assert not torch.equal(sd["temperature"], torch.ones(1))


def test_a_batch_size_the_world_does_not_divide_is_refused(paths):
    code, log = launch(paths, "coca_dp_refused", 29742, batch=3)
    assert code != 0 and "--train_batch_size 3 must be divisible by the world size 2" in log, log[-3000:]
    assert not (paths[3] / "coca_dp_refused").exists()
