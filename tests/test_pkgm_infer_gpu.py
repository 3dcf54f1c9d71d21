"""EntityInference / RelationInference and pkgm_infer.py on the device, on the trained tables of the link-prediction goldens: batch
size independence, the dictionary forms, the kernel's own results under the classes, and the CLI's file line for line.

The comparison with goldens of the reference's torchkge (infer_*.npz, tools/gen_golden_pkgm_infer.py) is not here: on these tables
11 to 28 of the 80 test queries per entity mode have two of their first 11 fp64 scores within 1e-4 (S_a + S_b), more than the one in
ten the generator allows, so it writes no file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from item_alignment_amd.models import kg_pretrain as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")
DEV = "cuda"
N_ENT, N_REL, DIM = 300, 8, 64
pytestmark = pytest.mark.gpu


def golden(name):
    return np.load(os.path.join(GOLDEN, f"linkpred_{name}.npz"))


def kg_of(z, split):
    return K.KnowledgeGraph(*(torch.from_numpy(z[f"{split}_{c}"]) for c in ("h", "t", "r")), N_ENT, N_REL)


def model_of(z, name):
    cls = K.PKGMPretrainModel if name.startswith("pkgm") else K.TransEPretrainModel
    m = cls(DIM, N_ENT, N_REL, dissimilarity_type="L1" if name.endswith("l1") else "L2")
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    return m.to(DEV)


def queries(z, missing):
    h, t, r = (torch.from_numpy(z[f"test_{c}"]) for c in ("h", "t", "r"))
    return {"tails": (h, r), "heads": (t, r), "relations": (h, t)}[missing]


def known_groups(z, missing, splits=("train", "test")):
    kgs = [kg_of(z, s) for s in splits]
    f = K.KGFilters.build(kgs)
    return {"tails": f.tails, "heads": f.heads}.get(missing) if missing != "relations" else K.relation_filter_groups(kgs)


def infer(model, missing, a, b, top_k, dictionary=None, b_size=1000):
    if missing == "relations":
        inf = K.RelationInference(model, a, b, top_k=top_k, dictionary=dictionary)
    else:
        inf = K.EntityInference(model, a, b, top_k=top_k, missing=missing, dictionary=dictionary)
    inf.evaluate(b_size, verbose=False)
    return inf


@pytest.mark.parametrize("name", ["pkgm_l2", "pkgm_l1", "transe_l2"])
@pytest.mark.parametrize("missing", ["tails", "heads", "relations"])
def test_classes(gpu, name, missing):
    z = golden(name)
    model = model_of(z, name)
    a, b = queries(z, missing)
    groups = known_groups(z, missing)
    mode = {"tails": K.TOPK_TAILS, "heads": K.TOPK_HEADS, "relations": K.TOPK_RELS}[missing]
    ent, rel = model.ent_emb.weight.data, model.rel_emb.weight.data
    for dictionary in (None, groups):
        big = infer(model, missing, a, b, 10, dictionary, 1000)
        small = infer(model, missing, a, b, 10, dictionary, 7)
        for x in (big.predictions, big.scores):
            assert x.device.type == "cpu" and x.shape == (len(a), 10)
        assert big.predictions.dtype == torch.int64 and big.scores.dtype == torch.float32
        assert torch.equal(big.predictions, small.predictions) and torch.equal(big.scores, small.scores)
        qg = None if dictionary is None else groups.group_of(a.numpy(), b.numpy())
        idx, score = K.kg_topk(ent, rel, a, b, model.norm, mode, 10, dictionary, qg)
        assert torch.equal(big.predictions, idx.cpu()) and torch.equal(big.scores, score.cpu())
    # the known completions are never predicted; every query of the test split has at least its own fact in its group
    pred = big.predictions
    for i in range(len(a)):
        members = set(groups.members(int(qg[i])).tolist())
        assert members and not members & set(pred[i].tolist())
    n_cand = N_REL if missing == "relations" else N_ENT
    assert bool(((pred >= 0).sum(1) == torch.tensor([min(10, n_cand - len(groups.members(int(g)))) for g in qg])).all())
    # a plain torchkge dictionary gives what the FilterGroups give
    base = N_ENT if missing == "relations" else N_REL
    plain = {(int(k) // base, int(k) % base): set(groups.members(g).tolist()) for g, k in enumerate(groups.keys)}
    from_dict = infer(model, missing, a, b, 10, plain, 33)
    assert torch.equal(from_dict.predictions, big.predictions) and torch.equal(from_dict.scores, big.scores)
    # PKGM infers like TransE: the projection is not used
    if name.startswith("pkgm"):
        bare = K.TransEPretrainModel(DIM, N_ENT, N_REL, dissimilarity_type=model.dissimilarity_type)
        bare.load_state_dict({k: v for k, v in model.state_dict().items() if k != "proj_mat.weight"})
        other = infer(bare.to(DEV), missing, a, b, 10, groups)
        assert torch.equal(other.predictions, big.predictions) and torch.equal(other.scores, big.scores)


def test_top_k_bounds_and_empty_queries(gpu):
    z = golden("transe_l2")
    model = model_of(z, "transe_l2")
    a, b = queries(z, "tails")
    for bad in (0, 65):
        with pytest.raises(ValueError):
            infer(model, "tails", a, b, bad)
    inf = infer(model, "tails", a[:0], b[:0], 5)
    assert inf.predictions.shape == (0, 5) and inf.scores.shape == (0, 5)
    with pytest.raises(ValueError):
        K.EntityInference(model, a, b).evaluate(0)


def write_data(d, z):
    for s in ("train", "valid", "test"):
        with open(os.path.join(d, f"{s}2id.txt"), "w") as f:
            f.writelines(f"{h}\t{r}\t{t}\n" for h, r, t in zip(z[f"{s}_h"].tolist(), z[f"{s}_r"].tolist(), z[f"{s}_t"].tolist()))
    with open(os.path.join(d, "entity2id.txt"), "w") as f:
        f.writelines(f"/item/{i}\t{i}\n" for i in range(N_ENT))
    with open(os.path.join(d, "relation2id.txt"), "w") as f:
        f.writelines(f"rel_{i}\t{i}\n" for i in range(N_REL))


def run_cli(*args):
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "pkgm_infer.py"), *args], capture_output=True, text=True, env=env, timeout=300)


def lines_of(inf, a, b, names):
    out = []
    for i, (qa, qb) in enumerate(zip(a.tolist(), b.tolist())):
        for rank, (c, s) in enumerate(zip(inf.predictions[i].tolist(), inf.scores[i].tolist()), 1):
            if c >= 0:
                out.append(f"{i}\t{qa}\t{qb}\t{rank}\t{c}\t{names.format(c)}\t{s:.9g}")
    return out


@pytest.mark.parametrize("missing", ["tails", "heads", "relations"])
def test_cli_end_to_end(gpu, tmp_path, missing):
    name = "pkgm_l1"
    z = golden(name)
    write_data(tmp_path, z)
    torch.save({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}, tmp_path / "pkgm.bin")     # with proj_mat.weight
    a, b = queries(z, missing)
    with open(tmp_path / "q.txt", "w") as f:
        f.writelines(f"{x}\t{y}\n" for x, y in zip(a.tolist(), b.tolist()))
    model = model_of(z, name)
    names = "rel_{}" if missing == "relations" else "/item/{}"
    common = ["--data_dir", str(tmp_path), "--model_path", str(tmp_path / "pkgm.bin"), "--query_file", str(tmp_path / "q.txt"), "--missing",
              missing, "--norm", "L1", "--eval_batch_size", "33"]
    res = run_cli(*common, "--output_file", str(tmp_path / "raw.tsv"))
    assert res.returncode == 0, res.stderr[-2000:]
    want = lines_of(infer(model, missing, a, b, 10), a, b, names)
    assert open(tmp_path / "raw.tsv").read().splitlines() == want
    assert len(want) == len(a) * min(10, N_REL if missing == "relations" else N_ENT)
    res = run_cli(*common, "--output_file", str(tmp_path / "filt.tsv"), "--top_k", "7", "--filter_known", "--do_test")
    assert res.returncode == 0, res.stderr[-2000:]
    want = lines_of(infer(model, missing, a, b, 7, known_groups(z, missing)), a, b, names)
    got = open(tmp_path / "filt.tsv").read().splitlines()
    assert got == want
    if missing == "relations":
        assert len(got) < len(a) * 7                           # slots with idx = -1 are not written
    # --do_eval widens the filter with valid2id.txt
    res = run_cli(*common, "--output_file", str(tmp_path / "all.tsv"), "--top_k", "7", "--filter_known", "--do_eval", "--do_test")
    assert res.returncode == 0, res.stderr[-2000:]
    want = lines_of(infer(model, missing, a, b, 7, known_groups(z, missing, ("train", "valid", "test"))), a, b, names)
    assert open(tmp_path / "all.tsv").read().splitlines() == want
