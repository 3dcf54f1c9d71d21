"""TEST INFRASTRUCTURE -- golden completions of the knowledge-graph tables (torchkge inference.py EntityInference / RelationInference)
captured from the reference's own torchkge on CPU: writes tests/golden/pkgm_pretrain/infer_{pkgm_l2,pkgm_l1,transe_l2}.npz.

    python tools/gen_golden_pkgm_infer.py <reference checkout>

The tables and the splits are those of linkpred_*.npz (tools/gen_golden_pkgm_linkpred.py).  The queries are the test split's:
(h, r) for tails, (t, r) for heads, (h, t) for relations; k = 10.  The scores and the sorted ids come from the four calls of the
reference's evaluate() loop -- inference_prepare_candidates, inference_scoring_function, filter_scores, sort -- since evaluate() itself
raises at its score store (inference.py:151, 246), and with missing='heads' already at the scoring call (see main).  Filtered: with
the dictionaries of a KnowledgeGraph over train + test (dict_of_tails, dict_of_heads, dict_of_rels), as pkgm_infer.py --filter_known --do_test loads them.

Per mode m in {tails, heads, rels} and f in {raw, filt}: {m}_{f}_idx int64 [n, w], {m}_{f}_score fp32 [n, w], w = min(10, candidates);
filtered candidates the reference could not avoid returning keep its score -inf.  {m}_{f}_keep bool [n]: False for a query with a near
tie -- two consecutive fp64 scores among its ranks 1 .. k + 1 (filtered candidates set aside) within 1e-4 (S_a + S_b)
(tests/linkpred_reference.py) -- whose order fp32 rounding decides.  At most one query in ten may be left out of any vector.
Re-running reproduces the files byte for byte.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kgtopk_reference as KR  # noqa: E402
from gen_golden_pkgm_linkpred import CASES, DIM, N_ENT, N_REL, write_npz  # noqa: E402

K_TOP = 10
NEAR = 1e-4


def near_tie(s, S, mask, k):
    """bool [n]: two consecutive fp64 scores among ranks 1 .. k + 1 of the unmasked candidates within NEAR (S_a + S_b)."""
    s = s.clone()
    s[mask] = -float("inf")
    top, order = s.sort(dim=1, descending=True)
    top, St = top[:, :k + 1], S.gather(1, order)[:, :k + 1]
    live = torch.isfinite(top[:, 1:])
    close = (top[:, :-1] - top[:, 1:]).abs() <= NEAR * (St[:, :-1] + St[:, 1:])
    return (close & live).any(1)


def main(reference):
    sys.path.insert(0, os.path.join(reference, "torchkge"))
    from torchkge.data_structures import KnowledgeGraph
    from torchkge.models import translation as T
    from torchkge.utils import filter_scores
    import pandas as pd

    empty = torch.tensor([]).long()
    over, files = [], {}
    for name, (cls_name, norm) in CASES.items():
        z = np.load(os.path.join(OUT, f"linkpred_{name}.npz"))
        model = getattr(T, cls_name)(DIM, N_ENT, N_REL, dissimilarity_type=norm)
        model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
        h, t, r = (torch.from_numpy(z[f"test_{c}"]) for c in ("h", "t", "r"))
        known = KnowledgeGraph(df=pd.DataFrame({"from": np.concatenate([z["train_h"], z["test_h"]]),
                                                "rel": np.concatenate([z["train_r"], z["test_r"]]),
                                                "to": np.concatenate([z["train_t"], z["test_t"]])}),
                               ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
        ent, rel = model.ent_emb.weight.data, model.rel_emb.weight.data
        nn = 2 if norm == "L2" else 1
        out = {}
        with torch.no_grad():
            h_emb, _, r_emb, cand = model.inference_prepare_candidates(h, empty, r, entities=True)
            tails = model.inference_scoring_function(h_emb, cand, r_emb)
            # missing='heads' passes an empty head index, from which the reference takes the batch size: its candidates come out
            # [0, n_ent, D] and the scoring call raises.  The tails stand in for the (unused) head index here.
            _, t_emb, r_emb, cand = model.inference_prepare_candidates(t, t, r, entities=True)
            heads = model.inference_scoring_function(cand, t_emb, r_emb)
            h_emb, t_emb, _, cand = model.inference_prepare_candidates(h, t, empty, entities=False)
            rels = model.inference_scoring_function(h_emb, t_emb, cand)
        for m, scores, (a, b), mode, dic in (("tails", tails, (h, r), KR.TAILS, known.dict_of_tails),
                                             ("heads", heads, (t, r), KR.HEADS, known.dict_of_heads),
                                             ("rels", rels, (h, t), KR.RELS, known.dict_of_rels)):
            assert scores.dtype == torch.float32 and scores.shape == (len(h), N_REL if m == "rels" else N_ENT)
            s64, S = KR.scores_fp64(ent, rel, a, b, nn, mode)
            for f, sc in (("raw", scores), ("filt", filter_scores(scores, dic, a, b, None))):
                top, idx = sc.sort(descending=True)
                w = min(K_TOP, sc.shape[1])
                near = near_tie(s64, S, torch.isinf(sc), K_TOP)
                if near.sum() * 10 > len(near):
                    over.append(f"{name} {m} {f}: {int(near.sum())} of {len(near)}")
                out[f"{m}_{f}_idx"] = idx[:, :w].numpy().astype(np.int64)
                out[f"{m}_{f}_score"] = top[:, :w].numpy().astype(np.float32)
                out[f"{m}_{f}_keep"] = (~near).numpy()
                print(name, m, f, "near ties", int(near.sum()), "of", len(near))
        files[name] = out
    if over:                                                       # a condition on the inputs: nothing is written
        raise SystemExit("more than one query in ten is a near tie (no golden written): " + "; ".join(over))
    for name, out in files.items():
        write_npz(os.path.join(OUT, f"infer_{name}.npz"), out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
