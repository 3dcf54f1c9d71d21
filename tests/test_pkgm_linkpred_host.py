"""Host side of the link-prediction evaluation of pkgm_pretrain.py (--do_eval / --do_test): the fp64 reference against the torchkge
goldens, the CSR filter groups against torchkge's dict-of-sets, the metric expressions and print format, and the CLI's refusals of
empty or out-of-range split files (no GPU needed)."""
import contextlib
import io
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

from item_alignment_amd.models import kg_pretrain as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linkpred_reference as LR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")
CASES = ["pkgm_l2", "pkgm_l1", "transe_l2"]
# (prefix, evaluated split, splits loaded into the filter)
RUNS = [("t", "test", ("train", "test")), ("vt", "test", ("train", "valid", "test")), ("vv", "valid", ("train", "valid", "test"))]


def golden(name):
    return np.load(os.path.join(GOLDEN, f"linkpred_{name}.npz"))


def kg_of(z, split):
    return K.KnowledgeGraph(*(torch.from_numpy(z[f"{split}_{c}"]) for c in ("h", "t", "r")), 300, 8)


def filters_of(z, loaded):
    return K.KGFilters.build([kg_of(z, s) for s in loaded])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prefix,split,loaded", RUNS)
def test_fp64_reference_reproduces_the_golden_ranks(name, prefix, split, loaded):
    z = golden(name)
    norm = 1 if name.endswith("l1") else 2
    ent, rel = torch.from_numpy(z["sd_ent_emb.weight"]), torch.from_numpy(z["sd_rel_emb.weight"])
    h, t, r = (torch.from_numpy(z[f"{split}_{c}"]) for c in ("h", "t", "r"))
    f = filters_of(z, loaded)
    for side, sname, groups, anchor in ((LR.TAIL, "tails", f.tails, h), (LR.HEAD, "heads", f.heads, t)):
        s, _ = LR.scores_fp64(ent, rel, h, t, r, norm, side)
        true = LR.true_ids(h, t, side)
        mask = LR.filter_mask(groups, groups.group_of(anchor.numpy(), r.numpy()), 300)
        ok = ~torch.from_numpy(z[f"near_tie_{split}_{sname}"])
        assert ok.sum() > len(ok) // 2
        raw, filt = LR.exact_rank(s, true), LR.exact_rank(s, true, mask)
        assert torch.equal(raw[ok], torch.from_numpy(z[f"{prefix}_rank_{sname}"])[ok]), (sname, "raw")
        assert torch.equal(filt[ok], torch.from_numpy(z[f"{prefix}_filt_{sname}"])[ok]), (sname, "filtered")


def test_goldens_have_spread_ranks():
    """A random ranker (mean rank ~150 of 300) cannot pass the rank tests: the trained tables rank far better."""
    for name in CASES:
        z = golden(name)
        assert z["t_rank_tails"].mean() < 100 and z["t_rank_heads"].mean() < 110
        assert len(np.unique(z["t_rank_tails"])) > 30


@pytest.mark.parametrize("loaded", [("train", "test"), ("train", "valid", "test")])
def test_filter_groups_equal_torchkge_dicts(loaded):
    z = golden("pkgm_l2")
    heads, tails = defaultdict(set), defaultdict(set)          # torchkge KnowledgeGraph.evaluate_dicts over every loaded fact
    for s in loaded:
        for h, t, r in zip(z[f"{s}_h"].tolist(), z[f"{s}_t"].tolist(), z[f"{s}_r"].tolist()):
            heads[(t, r)].add(h)
            tails[(h, r)].add(t)
    f = filters_of(z, loaded)
    for groups, want in ((f.heads, heads), (f.tails, tails)):
        assert len(groups) == len(want)
        for (a, r), members in want.items():
            g = int(groups.group_of(np.array([a]), np.array([r]))[0])
            assert g >= 0
            got = groups.members(g)
            assert got.tolist() == sorted(members)
        assert int(groups.group_of(np.array([299]), np.array([7]))[0]) == -1 or (299, 7) in want
    # the hot relation's groups are large
    assert max(len(v) for (a, r), v in heads.items() if r == 0) >= 10


def evaluator_with(z, prefix):
    ev = K.LinkPredictionEvaluator(None, K.KnowledgeGraph(*(torch.zeros(0, dtype=torch.int64),) * 3, 300, 8), None)
    ev.rank_true_heads, ev.rank_true_tails = (torch.from_numpy(z[f"{prefix}_rank_{s}"]) for s in ("heads", "tails"))
    ev.filt_rank_true_heads, ev.filt_rank_true_tails = (torch.from_numpy(z[f"{prefix}_filt_{s}"]) for s in ("heads", "tails"))
    ev.evaluated = True
    return ev


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prefix", ["t", "vt", "vv"])
def test_metrics_reproduce_the_golden_text(name, prefix):
    z = golden(name)
    ev = evaluator_with(z, prefix)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ev.print_results()
    assert buf.getvalue() == bytes(z[f"{prefix}_text"]).decode()
    assert ev.results_text() == buf.getvalue()


def test_metrics_refuse_before_evaluate():
    ev = K.LinkPredictionEvaluator(None, K.KnowledgeGraph(*(torch.zeros(2, dtype=torch.int64),) * 3, 4, 1), None)
    for f in (ev.mean_rank, ev.hit_at_k, ev.mrr, ev.print_results):
        with pytest.raises(RuntimeError):
            f()


def write_split(d, fname, facts):
    with open(os.path.join(d, fname), "w") as f:
        for h, r, t in facts:
            f.write(f"{h}\t{r}\t{t}\n")


def write_kg(d, n_ent=6, n_rel=2):
    write_split(d, "train2id.txt", [(1, 0, 2), (3, 1, 4)])
    with open(os.path.join(d, "entity2id.txt"), "w") as f:
        f.writelines(f"/item/{i}\t{i}\n" for i in range(n_ent))
    with open(os.path.join(d, "relation2id.txt"), "w") as f:
        f.writelines(f"rel_{i}\t{i}\n" for i in range(n_rel))


def run_cli(*args):
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "pkgm_pretrain.py"), *args], capture_output=True, text=True, env=env,
                          timeout=120)


@pytest.mark.parametrize("flag,fname,facts,msg", [
    ("--do_test", "test2id.txt", [], "holds no facts"),
    ("--do_eval", "valid2id.txt", [], "holds no facts"),
    ("--do_test", "test2id.txt", [(1, 0, 6)], "outside [0, 6)"),
    ("--do_eval", "valid2id.txt", [(1, 2, 3)], "outside [0, 2)"),
    ("--do_eval", "valid2id.txt", [(-1, 0, 3)], "outside [0, 6)"),
])
def test_cli_refuses_bad_split_files(tmp_path, flag, fname, facts, msg):
    write_kg(tmp_path)
    write_split(tmp_path, fname, facts)
    res = run_cli("--data_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--model_name", "pkgm_epoch-{}.bin", flag)
    assert res.returncode != 0
    assert msg in res.stderr and fname in res.stderr
    if not facts:
        assert flag in res.stderr and "data_prepare.py" in res.stderr
    assert not (tmp_path / "out").exists()


def test_load_ccks_splits_reads_the_flagged_files(tmp_path):
    write_kg(tmp_path)
    write_split(tmp_path, "valid2id.txt", [(0, 1, 5)])
    write_split(tmp_path, "test2id.txt", [(1, 0, 3), (1, 0, 2)])
    tr, va, te, f = K.load_ccks_splits(str(tmp_path), False, True)
    assert va is None and len(tr) == 2 and te.tail_idx.tolist() == [3, 2]
    assert f.tails.members(int(f.tails.group_of([1], [0])[0])).tolist() == [2, 3]
    assert int(f.tails.group_of([0], [1])[0]) == -1                   # valid not loaded: not in the filter
    tr, va, te, f = K.load_ccks_splits(str(tmp_path), True, True)
    assert f.tails.members(int(f.tails.group_of([0], [1])[0])).tolist() == [5]
    assert K.load_ccks(str(tmp_path)).head_idx.tolist() == tr.head_idx.tolist()


@pytest.mark.parametrize("bs", ["0", "-4"])
def test_cli_refuses_a_nonpositive_eval_batch_size(tmp_path, bs):
    write_kg(tmp_path)
    write_split(tmp_path, "test2id.txt", [(1, 0, 3)])
    res = run_cli("--data_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--model_name", "pkgm_epoch-{}.bin", "--do_test",
                  "--eval_batch_size", bs)
    assert res.returncode != 0 and "--eval_batch_size" in res.stderr
    assert not (tmp_path / "out").exists()
