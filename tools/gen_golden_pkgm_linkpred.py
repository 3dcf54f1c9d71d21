"""TEST INFRASTRUCTURE -- golden link-prediction ranks of the knowledge-graph pretraining job (reference pkgm_pretrain.py --do_test /
--do_eval) captured from the reference's own torchkge KnowledgeGraph, split_kg and LinkPredictionEvaluator on CPU: writes
tests/golden/pkgm_pretrain/linkpred_{pkgm_l2,pkgm_l1,transe_l2}.npz.

    python tools/gen_golden_pkgm_linkpred.py <reference checkout>

The KG: 300 entities, 8 relations, 2400 train / 80 valid / 80 test facts.  Relation r in 1..6 maps entity e to e + 37 r or
e + 37 r + 1 (mod 300); relation 0 is a hot many-to-many relation (heads 0..19, tails 20..59), so its filter groups are large; 12 test facts repeat
train facts, 6 have entity 0 as head or tail, and relation 7 appears only in test.  The tables are trained with the reference's
MarginLoss + Bernoulli sampling + Adam (full batch, entity rows normalised after every step) until the ranks spread, then every
entity row is scaled by a random factor in [0.5, 2] (a kernel that normalises rows fails) -- proj_mat stays in the state dict.

Each file holds the state dict (sd_*), the splits, the four rank vectors of the test split for the test-only run (t_*) and the
valid + test run (vt_*), those of the valid split (vv_*), the print_results() text of each (*_text), and near_tie_{valid,test}_
{heads,tails}: a query is a near tie if a candidate's fp64 score lies within 1e-4 (S_c + S_true) of the true one
(tests/linkpred_reference.py).  Re-running reproduces the files byte for byte.
"""
import contextlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linkpred_reference as LR  # noqa: E402

N_ENT, N_REL, DIM = 300, 8, 64
N_TRAIN, N_VALID, N_TEST = 2400, 80, 80
MARGIN, LR_, STEPS, EVAL_BS = 1.0, 1e-2, 300, 32
SCALE_SEEDS = 64
CASES = {"pkgm_l2": ("PKGMModel", "L2"), "pkgm_l1": ("PKGMModel", "L1"), "transe_l2": ("TransEModel", "L2")}


def draw(g, n, rels):
    r = g.choice(rels, n)
    h = g.integers(0, N_ENT, n)
    t = np.empty(n, np.int64)
    for i in range(n):
        if r[i] == 0:
            h[i] = g.integers(0, 20)
            t[i] = g.integers(20, 60)
        else:
            t[i] = (h[i] + 37 * r[i] + g.integers(0, 2)) % N_ENT
    return h.astype(np.int64), t, r.astype(np.int64)


def make_kg():
    g = np.random.default_rng(20261016)
    tr = draw(g, N_TRAIN, np.arange(0, 7))
    va = draw(g, N_VALID, np.arange(0, 7))
    te = [x.copy() for x in draw(g, N_TEST, np.arange(0, 7))]
    rep = g.choice(N_TRAIN, 12, replace=False)                        # test facts that repeat train facts
    for x, y in zip(te, tr):
        x[:12] = y[rep]
    te[2][12:16] = 7                                                   # a relation seen only in test
    te[1][16:19] = 0                                                   # entity 0 as the tail target
    te[0][19:22] = 0                                                   # and as the head
    return tr, va, te


def near_ties(ent, rel, norm, va, te):
    """near_tie_{valid,test}_{heads,tails} masks of the tables (tests/linkpred_reference.py near_tie)."""
    out = {}
    for tag, (h, t, r) in (("valid", va), ("test", te)):
        h, t, r = (torch.from_numpy(x) for x in (h, t, r))
        for side, sname in ((LR.TAIL, "tails"), (LR.HEAD, "heads")):
            s, S = LR.scores_fp64(ent, rel, h, t, r, norm, side)
            out[f"near_tie_{tag}_{sname}"] = LR.near_tie(s, S, LR.true_ids(h, t, side)).numpy()
    return out


def write_npz(path, arrays):
    """np.savez with a fixed timestamp per member (zipfile stamps the current time otherwise)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def text_of(ev):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ev.print_results()
    return np.frombuffer(buf.getvalue().encode(), np.uint8)


def ranks(prefix, ev):
    return {f"{prefix}_rank_heads": ev.rank_true_heads.numpy().astype(np.int64), f"{prefix}_rank_tails": ev.rank_true_tails.numpy().astype(np.int64),
            f"{prefix}_filt_heads": ev.filt_rank_true_heads.numpy().astype(np.int64),
            f"{prefix}_filt_tails": ev.filt_rank_true_tails.numpy().astype(np.int64), f"{prefix}_text": text_of(ev)}


def main(reference):
    sys.path.insert(0, os.path.join(reference, "torchkge"))
    from torchkge.data_structures import KnowledgeGraph
    from torchkge.evaluation import LinkPredictionEvaluator
    from torchkge.models import translation as T
    from torchkge.sampling import BernoulliNegativeSampler
    from torchkge.utils.losses import MarginLoss
    import pandas as pd

    torch.use_deterministic_algorithms(True)
    os.makedirs(OUT, exist_ok=True)
    tr, va, te = make_kg()
    ents, rels = {i: i for i in range(N_ENT)}, {i: i for i in range(N_REL)}

    def kg_of(parts):
        h, t, r = (np.concatenate([p[i] for p in parts]) for i in (0, 1, 2))
        return KnowledgeGraph(df=pd.DataFrame({"from": h, "rel": r, "to": t}), ent2ix=ents, rel2ix=rels)

    kg_train = kg_of([tr])
    kg_t = kg_of([tr, te]).split_kg(sizes=[N_TRAIN, N_TEST])              # load_ccks(do_eval=False, do_test=True)
    kg_vt = kg_of([tr, va, te]).split_kg(sizes=[N_TRAIN, N_VALID, N_TEST])  # load_ccks(do_eval=True, do_test=True)
    total_near = 0
    for name, (cls_name, norm) in CASES.items():
        torch.manual_seed(11)
        model = getattr(T, cls_name)(DIM, N_ENT, N_REL, dissimilarity_type=norm)
        crit = MarginLoss(MARGIN)
        opt = torch.optim.Adam(model.parameters(), lr=LR_)
        sampler = BernoulliNegativeSampler(kg_train)
        for _ in range(STEPS):
            nh, nt = sampler.corrupt_batch(kg_train.head_idx, kg_train.tail_idx, kg_train.relations, n_neg=1)
            opt.zero_grad()
            p, n = model(kg_train.head_idx, kg_train.tail_idx, kg_train.relations, nh, nt)
            crit(p, n).backward()
            opt.step()
            model.normalize_parameters()
        nn = 2 if norm == "L2" else 1
        trained = model.ent_emb.weight.detach().clone()
        best = None
        for seed in range(SCALE_SEEDS):                                # the row scaling with the fewest near ties
            scale = torch.from_numpy(np.random.default_rng(seed).uniform(0.5, 2.0, (N_ENT, 1)).astype(np.float32))
            masks = near_ties(trained * scale, model.rel_emb.weight.detach(), nn, va, te)
            n_near = sum(int(m.sum()) for m in masks.values())
            if best is None or n_near < best[0]:
                best = (n_near, seed, scale, masks)
        n_near, scale_seed, scale, masks = best
        with torch.no_grad():
            model.ent_emb.weight.copy_(trained * scale)
        out = {"sd_" + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
        for tag, (h, t, r) in (("train", tr), ("valid", va), ("test", te)):
            out[f"{tag}_h"], out[f"{tag}_t"], out[f"{tag}_r"] = h, t, r
        ev = LinkPredictionEvaluator(model, kg_t[1])
        ev.evaluate(EVAL_BS, verbose=False)
        out.update(ranks("t", ev))
        for prefix, kg in (("vv", kg_vt[1]), ("vt", kg_vt[2])):
            ev = LinkPredictionEvaluator(model, kg)
            ev.evaluate(EVAL_BS, verbose=False)
            out.update(ranks(prefix, ev))
        for k, m in masks.items():
            out[k] = m
        total_near += n_near
        out["meta"] = np.frombuffer(json.dumps(dict(model=cls_name, norm=norm, n_ent=N_ENT, n_rel=N_REL, dim=DIM, steps=STEPS, lr=LR_,
                                                    margin=MARGIN, eval_batch_size=EVAL_BS, scale_seed=scale_seed), sort_keys=True).encode(),
                                    np.uint8)
        write_npz(os.path.join(OUT, f"linkpred_{name}.npz"), out)
        print(name, "scale seed", scale_seed, "near ties", n_near, {k[9:]: int(m.sum()) for k, m in masks.items()})
        for k in ("t_text", "vt_text", "vv_text"):
            print(f"  {k}:", bytes(out[k]).decode().replace("\n", " | "))
    print("near ties in all files:", total_near)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
