"""Host side of the knowledge-graph pretraining job (pkgm_pretrain.py): Bernoulli probabilities, data loading, the learning-rate
schedule, the gradient-accumulation quirk, the Xavier + normalise initialisation and the CLI's refusals (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from item_alignment_amd.models import kg_pretrain as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")


def golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def test_bernoulli_probs_equal_the_reference():
    z = golden("pkgm_l2")
    kg = K.KnowledgeGraph(*(torch.from_numpy(z[k]) for k in ("h", "t", "r")), 300, 7)
    got = K.bernoulli_probs(kg)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), z["bern_probs"])


def test_bernoulli_probs_unseen_relation_is_one_half():
    kg = K.KnowledgeGraph(torch.tensor([0, 0, 1]), torch.tensor([1, 2, 2]), torch.tensor([0, 0, 0]), 3, 3)
    p = K.bernoulli_probs(kg)
    assert p[1] == 0.5 and p[2] == 0.5
    # relation 0: 2 tails per head (tph = 3 / 2), 1.5 heads per tail (hpt = 3 / 2) -> 0.5; then a skewed one
    kg = K.KnowledgeGraph(torch.tensor([0, 0, 0]), torch.tensor([1, 2, 3]), torch.tensor([0, 0, 0]), 4, 1)
    assert K.bernoulli_probs(kg)[0].item() == pytest.approx(3.0 / 4.0)


@pytest.mark.parametrize("name", ["pkgm_l2", "pkgm_l1", "transe_l2"])
def test_initialisation_matches_the_reference_rng_order(name):
    z = golden(name)
    cls = K.PKGMPretrainModel if name.startswith("pkgm") else K.TransEPretrainModel
    torch.manual_seed(11)
    m = cls(64, 300, 7, dissimilarity_type="L1" if name.endswith("l1") else "L2")
    sd = m.state_dict()
    want = sorted(k[5:] for k in z.files if k.startswith("init_"))
    assert sorted(sd) == want
    for k in want:
        assert np.array_equal(sd[k].numpy(), z["init_" + k]), k


def test_torus_norms_are_rejected():
    with pytest.raises(ValueError, match="torus"):
        K.PKGMPretrainModel(8, 4, 2, dissimilarity_type="torus_L2")


def write_kg(d, facts, n_ent, n_rel):
    with open(os.path.join(d, "train2id.txt"), "w") as f:
        for h, r, t in facts:
            f.write(f"{h}\t{r}\t{t}\n")
    with open(os.path.join(d, "entity2id.txt"), "w") as f:
        for i in range(n_ent):
            f.write(f"/item/{i}\t{i}\n")
    with open(os.path.join(d, "relation2id.txt"), "w") as f:
        for i in range(n_rel):
            f.write(f"rel_{i}\t{i}\n")


def test_load_ccks_uses_the_written_ids(tmp_path):
    write_kg(tmp_path, [(3, 0, 5), (0, 1, 9), (7, 0, 3)], n_ent=12, n_rel=2)
    kg = K.load_ccks(str(tmp_path))
    assert (kg.n_ent, kg.n_rel, len(kg)) == (12, 2, 3)
    assert kg.head_idx.tolist() == [3, 0, 7] and kg.relations.tolist() == [0, 1, 0] and kg.tail_idx.tolist() == [5, 9, 3]
    assert kg.head_idx.dtype == torch.int64


def test_load_ccks_rejects_ids_outside_the_id_files(tmp_path):
    write_kg(tmp_path, [(3, 0, 12)], n_ent=12, n_rel=2)
    with pytest.raises(ValueError, match="'to'"):
        K.load_ccks(str(tmp_path))


def test_schedule_counts_and_lr_sequence():
    # pkgm_pretrain.py: int(len(kg) / bs / gas) * (epochs - start_epoch), warm-up int(total * proportion)
    assert K.schedule_steps(100_000, 32768, 1, 2000, 0, 0.2) == (3 * 2000, 1200)
    assert K.schedule_steps(100_000, 32768, 2, 10, 4, 0.2) == (6, 1)
    total, warm = K.schedule_steps(1000, 100, 1, 3, 0, 0.2)
    assert (total, warm) == (30, 6)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, K.linear_schedule_lambda(warm, total))
    lrs = []
    for _ in range(total + 2):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    want = [1e-3 * (s / warm if s < warm else max(0.0, (total - s) / (total - warm))) for s in range(total + 2)]
    assert lrs == pytest.approx(want, abs=1e-12)
    assert lrs[0] == 0.0 and lrs[warm] == pytest.approx(1e-3)


def test_accumulation_quirk_only_every_kth_batch_steps():
    assert K.n_batches(10, 3) == 4 and K.n_batches(9, 3) == 3
    assert K.stepping_batches(7, 1) == list(range(7))
    assert K.stepping_batches(7, 3) == [2, 5]          # batch 6 is computed and dropped; batches 0, 1, 3, 4 are cleared unused


def run_cli(*args):
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "pkgm_pretrain.py"), *args], capture_output=True, text=True, env=env,
                          timeout=120)


@pytest.mark.parametrize("extra,msg", [(["--norm", "torus_L2"], "torus"), (["--norm", "torus_L1"], "torus"), (["--do_test"], "do_test"),
                                       (["--do_eval"], "do_eval"), (["--model_name", "distmult_{}.bin"], "Unsuported model name")])
def test_cli_rejects_what_is_not_built(tmp_path, extra, msg):
    write_kg(tmp_path, [(1, 0, 2)], n_ent=4, n_rel=1)
    res = run_cli("--data_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--model_name", "pkgm_epoch-{}.bin", *extra)
    assert res.returncode != 0
    assert msg in res.stderr
    assert not (tmp_path / "out").exists()
