"""References of knowledge-graph completion (ia_kgpt_topk; torchkge inference.py EntityInference / RelationInference).

Modes: TAILS q = ent[a] + rel[b] over the entity rows, HEADS q = ent[a] - rel[b] over the entity rows, RELS q = ent[b] - ent[a] over
the relation rows.  Score s_c = -d(q, c), d = |q - c|_2^2 (norm 2) or |q - c|_1 (norm 1).

* scores_fp64: fp64 scores and the error scale S of tests/linkpred_reference.py, for every mode (the entity modes are that file's).
* relation_scores_fp32: the kernel's own arithmetic for the relation mode restated in numpy: q in fp32, one fp32 accumulator per pair,
  k in order, fma(x, x, acc) for norm 2.  The fma is formed in fp64 (x * x is exact there) and rounded to fp32; the sum is rounded
  twice that way, which differs from one rounding only when the fp64 sum lands on an fp32 midpoint (about 2^-29 per step).
* select: the k best ids of a score matrix in the total order (score descending, id ascending), members of a mask set aside,
  unused slots -1 / -inf.
"""
import numpy as np
import torch

import linkpred_reference as LR

TAILS, HEADS, RELS = 0, 1, 2
TAU = LR.TAU


def scores_fp64(ent, rel, a, b, norm, mode, chunk=256):
    """(s [B, n_cand], S [B, n_cand]) in fp64 on ent's device."""
    if mode == TAILS:
        return LR.scores_fp64(ent, rel, a, a, b, norm, LR.TAIL, chunk)
    if mode == HEADS:
        return LR.scores_fp64(ent, rel, a, a, b, norm, LR.HEAD, chunk)
    q = ent.double()[b] - ent.double()[a]
    c = rel.double()
    p = 2.0 if norm == 2 else 1.0
    d = torch.cdist(q, c, p=p, compute_mode="donot_use_mm_for_euclid_dist")
    n = q.norm(p=p, dim=1)[:, None] + c.norm(p=p, dim=1)[None, :]
    return (-(d * d), n ** 2) if norm == 2 else (-d, n)


def relation_scores_fp32(ent, rel, a, b, norm):
    """fp32 [B, n_rel] numpy: -(sum over k in order) of the relation mode, as the kernel forms it."""
    ent, rel = (np.asarray(x.detach().cpu().numpy(), np.float32) for x in (ent, rel))
    a, b = (np.asarray(x.detach().cpu().numpy()) for x in (a, b))
    q = ent[b] - ent[a]
    acc = np.zeros((q.shape[0], rel.shape[0]), np.float32)
    for k in range(ent.shape[1]):
        x = q[:, k:k + 1] - rel[None, :, k]
        if norm == 2:
            acc = (x.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = acc + np.abs(x)
    return -acc


def select(scores, k, mask=None):
    """(idx int64 [B, k], score fp32 [B, k]) torch CPU tensors from a numpy fp32 [B, n] score matrix; mask [B, n] bool = set aside."""
    B, n = scores.shape
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float32)
    for i in range(B):
        ids = np.arange(n) if mask is None else np.nonzero(~mask[i])[0]
        s = scores[i, ids]
        order = np.lexsort((ids, -s))[:k]
        idx[i, :len(order)] = ids[order]
        sc[i, :len(order)] = s[order]
    return torch.from_numpy(idx), torch.from_numpy(sc)
